"""CPU: the host side of ``frag_end_context`` - the numpy restatement of the "end context" rule against a per-fragment
loop, the row-sum invariant, ``EndContext.mono`` / ``dinuc`` / ``frequency`` / ``enrichment`` on a hand table, the TSV
rows and their round trip, the command line's parser, the flat names and the C symbols.  The kernels are held against the
restatement in ``tests/test_gpu_end_context.py``."""
import gzip
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import end_context_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftk_end_context", "ftk_ref_context", "ftk_end_context_lds_classes")
A, Cc, G, T, N = range(5)


@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(20261020)
    seqs = H.make_genome(rng)
    return seqs, {name: H.fragments_of(name, len(seq), rng) for name, seq in seqs.items()}


@pytest.mark.parametrize("anchor", ["ends", "centre"])
@pytest.mark.parametrize("half_width, edges", [(1, H.ONE_CLASS), (7, H.DEFAULT_EDGES), (33, H.EIGHT_CLASSES)])
def test_restatement_equals_the_fragment_loop(genome, anchor, half_width, edges):
    seqs, frags = genome
    rng = np.random.default_rng(5)
    for name, seq in seqs.items():
        s, e, q = frags[name]
        idx = np.sort(rng.choice(len(s), min(len(s), 200), replace=False))
        idx = np.concatenate([idx, idx[:20]])  # and some fragments twice
        got, kept = H.restated_end_context(H.Bases(seq), s[idx], e[idx], q[idx], half_width, edges, 30, anchor)
        want, want_kept = H.looped_end_context(seq, s[idx], e[idx], q[idx], half_width, edges, 30, anchor)
        assert got.dtype == np.int64 and got.shape == (len(edges) - 1, 2, 2 * half_width, 25)
        assert np.array_equal(got, want) and np.array_equal(kept, want_kept) and kept.sum() > 50


@pytest.mark.parametrize("anchor", ["ends", "centre"])
def test_every_row_sums_to_the_kept_fragments(genome, anchor):
    seqs, frags = genome
    for name, seq in seqs.items():
        s, e, q = frags[name]
        for w, edges in ((32, H.DEFAULT_EDGES), (128, H.EIGHT_CLASSES)):
            table, kept = H.restated_end_context(H.Bases(seq), s, e, q, w, edges, 30, anchor)
            assert np.array_equal(table.sum(axis=-1), np.broadcast_to(kept[:, None, None], table.shape[:3]))
            ln = e.astype(np.int64) - s
            assert kept.sum() == int(((q >= 30) & (ln >= edges[0]) & (ln < edges[-1])).sum())
            assert table[..., 20:].sum() > 0 and table[..., 4::5].sum() > 0  # N as first and as second base
            if edges is H.EIGHT_CLASSES:
                assert kept[H.EMPTY_CLASS] == 0 and (np.delete(kept, H.EMPTY_CLASS) > 0).all()
    # the background: one cell per position, N behind the last base
    for name, seq in seqs.items():
        bases = H.Bases(seq)
        bg = H.restated_ref_context(bases, 0, len(seq) + 500)
        assert bg.sum() == len(seq) and bg[4::5].sum() >= 1
        m = 12_347 if len(seq) > 12_347 else 17
        assert np.array_equal(H.restated_ref_context(bases, 0, m) + H.restated_ref_context(bases, m, len(seq)), bg)


def hand_made(anchor="ends"):
    """One class, W = 1 (offsets -1 and 0), both kinds; a background with a motif that never occurs."""
    from finaletoolkit_amd import utils
    table = np.zeros((1, 2, 2, 25), np.int64)
    table[0, 0, 0, [5 * A + Cc, 5 * Cc + Cc, 5 * N + A, 5 * G + N]] = [6, 2, 1, 1]  # kind 0, o = -1
    table[0, 0, 1, [5 * Cc + Cc, 5 * T + G]] = [5, 5]                               # kind 0, o = 0
    table[0, 1, 0, [5 * A + A, 5 * G + T]] = [4, 6]                                 # kind 1, o = -1
    table[0, 1, 1, 5 * N + N] = 10                                                  # kind 1, o = 0: nothing defined
    bg = np.zeros(25, np.int64)
    bg[[5 * A + Cc, 5 * Cc + Cc, 5 * T + T, 5 * G + T, 5 * Cc + N, 5 * N + N]] = [10, 30, 40, 20, 1, 3]
    return utils.EndContext(table, np.array([10], np.int64), bg, 1, (100, 200), anchor, ("chrUn",))


def test_mono_dinuc_frequency_and_enrichment():
    from finaletoolkit_amd import utils
    assert utils.EndContext._fields == ("table", "n_kept", "background", "half_width", "length_edges", "anchor", "skipped_contigs")
    res = hand_made()
    mono, dinuc = res.mono, res.dinuc
    assert mono.shape == (1, 2, 2, 5) and dinuc.shape == (1, 2, 2, 16) and mono.dtype == np.int64 and dinuc.dtype == np.int64
    assert mono[0, 0, 0].tolist() == [6, 2, 1, 0, 1] and mono[0, 0, 1].tolist() == [0, 5, 0, 5, 0]
    assert mono[0, 1, 0].tolist() == [4, 0, 6, 0, 0] and mono[0, 1, 1].tolist() == [0, 0, 0, 0, 10]
    assert dinuc[0, 0, 0, 4 * A + Cc] == 6 and dinuc[0, 0, 0, 4 * Cc + Cc] == 2 and dinuc[0, 0, 0].sum() == 8  # N pairs left out
    assert dinuc[0, 1, 0, 4 * G + T] == 6 and dinuc[0, 1, 1].sum() == 0
    assert (mono.sum(axis=-1) == 10).all()
    f1, f2 = res.frequency(1), res.frequency(2)
    assert f1.shape == (1, 2, 2, 4) and f2.shape == (1, 2, 2, 16) and f1.dtype == np.float64
    assert f1[0, 0, 0].tolist() == [6 / 9, 2 / 9, 1 / 9, 0.0] and f2[0, 0, 0, 4 * A + Cc] == 6 / 8
    assert np.isnan(f1[0, 1, 1]).all() and np.isnan(f2[0, 1, 1]).all()
    # background counts: + strand for kind 0, the reverse complement's count for kind 1
    b1, b2 = res.background_counts(1), res.background_counts(2)
    assert b1[0].tolist() == [10, 31, 20, 40] and b1[1].tolist() == [40, 20, 31, 10]  # (C: CC and CN; N rows are no base)
    assert b2[0, 4 * A + Cc] == 10 and b2[1, 4 * G + T] == 10 and b2[1, 4 * A + A] == 40 and b2[1, 4 * A + Cc] == 20
    assert b2[0].sum() == b2[1].sum() == 100
    e1, e2 = res.enrichment(1), res.enrichment(2)
    assert e1.shape == f1.shape and e2.shape == f2.shape and e2.dtype == np.float64
    assert e1[0, 0, 0, A] == (6 / 9) / (10 / 101) and e1[0, 0, 0, T] == 0.0
    assert e1[0, 1, 0, A] == (4 / 10) / (40 / 101) and e1[0, 1, 0, G] == (6 / 10) / (31 / 101)
    assert e2[0, 0, 0, 4 * A + Cc] == (6 / 8) / (10 / 100) and e2[0, 0, 0, 4 * Cc + Cc] == (2 / 8) / (30 / 100)
    assert e2[0, 1, 0, 4 * G + T] == (6 / 10) / (10 / 100) and e2[0, 1, 0, 4 * A + A] == (4 / 10) / (40 / 100)
    assert math.isnan(e2[0, 0, 1, 4 * T + G])        # counted, but the + strand never reads TG
    assert e2[0, 0, 1, 4 * Cc + Cc] == (5 / 10) / (30 / 100)
    assert math.isnan(e2[0, 0, 0, 4 * A + A])        # neither counted nor in the background: 0 / 0
    assert np.isnan(e1[0, 1, 1]).all() and np.isnan(e2[0, 1, 1]).all()  # a row without a defined motif
    empty = res._replace(background=np.zeros(25, np.int64))
    assert np.isnan(empty.enrichment(1)).all() and np.isnan(empty.enrichment(2)).all()
    for bad in (0, 3):
        with pytest.raises(ValueError):
            res.frequency(bad)
        with pytest.raises(ValueError):
            res.enrichment(bad)


def parse_rows(text, res):
    """The tables of a TSV back: (mono + dinuc counts [n_classes, 2, 2W, 21], the rows)."""
    from finaletoolkit_amd import writers
    lines = text.splitlines()
    assert lines[0] + "\n" == writers.END_CONTEXT_HEADER
    assert lines[0].split("\t") == ["length_lo", "length_hi", "end", "offset", "motif", "count", "frequency", "enrichment"]
    w, edges = res.half_width, list(res.length_edges)
    ends = "UD" if res.anchor == "ends" else "+-"
    count = np.zeros((len(edges) - 1, 2, 2 * w, 21), np.int64)
    rows = [ln.split("\t") for ln in lines[1:]]
    for lo, hi, end, o, motif, k, f, x in rows:
        c = edges.index(int(lo))
        assert edges[c + 1] == int(hi)
        count[c, ends.index(end), int(o) + w, writers.END_CONTEXT_MOTIFS.index(motif)] = int(k)
    return count, rows


def test_tsv_text_rows():
    from finaletoolkit_amd import writers
    assert writers.END_CONTEXT_MOTIFS[:5] == tuple("ACGTN") and writers.END_CONTEXT_MOTIFS[5:9] == ("AA", "AC", "AG", "AT")
    assert writers.END_CONTEXT_MOTIFS[-1] == "TT" and len(writers.END_CONTEXT_MOTIFS) == 21
    res = hand_made()
    count, rows = parse_rows(writers.end_context_text(res), res)
    assert np.array_equal(count[..., :5], res.mono) and np.array_equal(count[..., 5:], res.dinuc)
    by_key = {(r[2], int(r[3]), r[4]): r for r in rows}
    assert by_key[("U", -1, "AC")][5:] == ["6", repr(6 / 8), repr((6 / 8) / (10 / 100))]
    assert by_key[("U", -1, "A")][5:] == ["6", repr(6 / 9), repr((6 / 9) / (10 / 101))]
    assert by_key[("U", -1, "N")][5:] == ["1", "nan", "nan"]            # N: a count, no frequency
    assert by_key[("U", 0, "TG")][5:] == ["5", "0.5", "nan"]            # counted, never in the background
    assert by_key[("U", 0, "TT")][5:] == ["0", "0.0", "0.0"]            # in the background, never counted
    assert by_key[("D", 0, "N")][5:] == ["10", "nan", "nan"]
    assert by_key[("D", -1, "GT")][5:] == ["6", "0.6", repr((6 / 10) / (10 / 100))]
    assert ("U", -1, "AA") not in by_key and ("U", 0, "GA") not in by_key  # neither a count nor a background
    assert ("D", 0, "AA") in by_key and by_key[("D", 0, "AA")][5:] == ["0", "nan", "nan"]  # TT on the + strand; the row has nothing defined
    assert all(r[0] == "100" and r[1] == "200" for r in rows)
    centre = hand_made("centre")
    assert {r[2] for r in parse_rows(writers.end_context_text(centre), centre)[1]} == {"+", "-"}


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_tsv_round_trip(tmp_path, suffix, genome):
    from finaletoolkit_amd import utils, writers
    seqs, frags = genome
    s, e, q = frags["eB"]
    bases = H.Bases(seqs["eB"])
    table, kept = H.restated_end_context(bases, s, e, q, 7, H.DEFAULT_EDGES)
    res = utils.EndContext(table, kept, H.restated_ref_context(bases, 0, bases.n), 7, H.DEFAULT_EDGES, "ends", ())
    out = str(tmp_path / ("ctx" + suffix))
    writers.write_end_context_rows(out, res)
    raw = open(out, "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == suffix.endswith(".gz")
    text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else raw.decode()
    assert text == writers.end_context_text(res)
    count, rows = parse_rows(text, res)
    assert np.array_equal(count[..., :5], res.mono) and np.array_equal(count[..., 5:], res.dinuc)
    f = np.concatenate([res.frequency(1), np.full(res.mono.shape[:-1] + (1,), np.nan), res.frequency(2)], axis=-1)
    x = np.concatenate([res.enrichment(1), np.full(res.mono.shape[:-1] + (1,), np.nan), res.enrichment(2)], axis=-1)
    for lo, hi, end, o, motif, k, fr, en in rows:
        cell = (list(H.DEFAULT_EDGES).index(int(lo)), "UD".index(end), int(o) + 7, writers.END_CONTEXT_MOTIFS.index(motif))
        for text_v, v in ((fr, f[cell]), (en, x[cell])):
            assert (text_v == "nan") == bool(np.isnan(v)) and (text_v == "nan" or float(text_v) == v)
    assert len(rows) == 3 * 2 * 14 * 21  # every motif is in this background
    with pytest.raises(ValueError, match="suffix"):
        writers.write_end_context_rows(str(tmp_path / "ctx.txt"), res)


def test_signature():
    from finaletoolkit_amd import utils
    sig = inspect.signature(utils.frag_end_context)
    assert list(sig.parameters) == ["input_file", "reference_file", "output_file", "contig", "quality_threshold", "half_width",
                                    "length_edges", "anchor", "workers", "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["input_file"] is inspect.Parameter.empty and d["reference_file"] is inspect.Parameter.empty
    assert (d["output_file"], d["contig"], d["quality_threshold"], d["half_width"], d["length_edges"], d["anchor"], d["workers"],
            d["verbose"]) == (None, None, 30, 32, (1, 150, 221, 1001), "ends", None, False)


@pytest.mark.parametrize("kwargs, match", [
    (dict(half_width=0), "half_width"),
    (dict(half_width=129), "half_width"),
    (dict(length_edges=(100,)), "length_edges"),
    (dict(length_edges=tuple(range(1, 11))), "length_edges"),
    (dict(length_edges=(0, 100)), "length_edges"),
    (dict(length_edges=(100, 100)), "length_edges"),
    (dict(length_edges=(1, 200, 150)), "length_edges"),
    (dict(length_edges=(1, (1 << 30) + 1)), "length_edges"),
    (dict(anchor="middle"), "anchor"),
    (dict(output_file="out.tsv.bgz"), "suffix"),
    (dict(output_file="out.txt"), "suffix"),
    (dict(output_file="-"), "suffix"),
])
def test_bad_arguments_raise_before_any_file_is_opened(tmp_path, kwargs, match):
    from finaletoolkit_amd import utils
    missing_in = str(tmp_path / "no_such_input.frag.gz")
    missing_ref = str(tmp_path / "no_such_reference.2bit")
    if kwargs.get("output_file") not in (None, "-"):
        kwargs = dict(kwargs, output_file=str(tmp_path / kwargs["output_file"]))
    with pytest.raises(ValueError, match=match):
        utils.frag_end_context(missing_in, missing_ref, **kwargs)
    assert os.listdir(tmp_path) == []


def test_parser_maps_flags_onto_the_arguments():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.endcontext import build_parser
    sig = inspect.signature(utils.frag_end_context)
    ap = build_parser()
    flags = [a.dest for a in ap._actions if a.dest != "help"]
    assert sorted(flags) == sorted(sig.parameters)  # every flag an argument and every argument a flag
    d = {k: v.default for k, v in sig.parameters.items()}
    got = vars(ap.parse_args(["in.bam", "ref.2bit", "out.tsv"]))
    assert got == dict(d, input_file="in.bam", reference_file="ref.2bit", output_file="out.tsv")
    got = vars(ap.parse_args(["in.frag.gz", "hg38.fa", "out.tsv.gz", "-c", "chr7", "-q", "5", "--half-width", "25",
                              "--length-edges", "50", "120", "167", "--anchor", "centre", "-w", "3", "-v"]))
    assert got == dict(input_file="in.frag.gz", reference_file="hg38.fa", output_file="out.tsv.gz", contig="chr7",
                       quality_threshold=5, half_width=25, length_edges=[50, 120, 167], anchor="centre", workers=3, verbose=True)
    got = vars(ap.parse_args(["a", "b", "c", "--contig", "12", "--min-mapq", "0", "--workers", "8", "--verbose"]))
    assert (got["contig"], got["quality_threshold"], got["workers"], got["verbose"], got["anchor"]) == ("12", 0, 8, True, "ends")
    for bad in (["in", "ref"], ["a", "b", "c", "--anchor", "middle"], ["a", "b", "c", "--length-edges"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.endcontext", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--half-width" in r.stdout and "--length-edges" in r.stdout and "--anchor" in r.stdout and "REF" in r.stdout


def test_flat_names():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    names = {"frag_end_context", "EndContext"}
    assert names <= set(dir(f)) and names <= set(utils.__all__) and names <= set(f._FLAT_BY_MODULE["utils"])
    assert f.frag_end_context is utils.frag_end_context and f.EndContext is utils.EndContext
    code = ("import finaletoolkit_amd as f\n"
            "f.install_alias()\n"
            "import finaletoolkit\n"
            "from finaletoolkit_amd import utils\n"
            "assert finaletoolkit.frag_end_context is utils.frag_end_context and finaletoolkit.utils.EndContext is utils.EndContext\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_symbols_exported_and_declared():
    from finaletoolkit_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ftk.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTS
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"^#define FTK_CONTEXT_MAX_HALF 128$", header, re.M) and L.CONTEXT_MAX_HALF == 128 == H.MAX_HALF
    assert re.search(r"^#define FTK_CONTEXT_MAX_CLASSES 8$", header, re.M) and L.CONTEXT_MAX_CLASSES == 8 == H.MAX_CLASSES
    assert re.search(r"^#define FTK_CONTEXT_ENDS 0$", header, re.M) and re.search(r"^#define FTK_CONTEXT_CENTRE 1$", header, re.M)
    assert L.CONTEXT_ANCHOR == {"ends": 0, "centre": 1}
    assert "end context" in header
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    # the LDS query needs no device: more classes fit a narrow table, and the widest leaves some to further grid rows
    fit = [lib.ftk_end_context_lds_classes(w) for w in (1, 32, 128)]
    assert fit[0] == 8 and 1 <= fit[2] < 8 and fit[0] >= fit[1] >= fit[2]
    assert lib.ftk_end_context_lds_classes(0) == 0 and lib.ftk_end_context_lds_classes(129) == 0
