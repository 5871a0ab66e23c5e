"""CPU: the host side of ``frag_motif_lengths`` - the numpy restatement of the "motif x length" rule against a loop over
fragments and bases, the row-sum identity, ``MotifLengths.frequency`` / ``mds`` / ``pooled`` on a hand table, both TSVs and
their round trip, the argument errors, the command line's parser, the flat names and the C symbols.  The kernels are held
against the restatement in ``tests/test_gpu_motif_lengths.py``."""
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
from tests import motif_length_helpers as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftk_motif_length_table", "ftk_motif_length_lds_rows")


def lds_rows():
    """The band sizes the library reports (a host-only query)."""
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    return {k: int(lib.ftk_motif_length_lds_rows(k)) for k in M.KS}


@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(20261021)
    seqs = H.make_genome(rng)
    sets = M.edge_sets_for(lds_rows().values())
    return seqs, {name: H.fragments_of(name, len(seq), rng, edge_sets=sets) for name, seq in seqs.items()}


@pytest.mark.parametrize("shift", [0, -1, -2, 1])
@pytest.mark.parametrize("k", M.KS)
def test_restatement_equals_the_fragment_loop(genome, k, shift):
    seqs, frags = genome
    rng = np.random.default_rng(5)
    for name, seq in seqs.items():
        s, e, q = frags[name]
        idx = np.sort(rng.choice(len(s), min(len(s), 300), replace=False))
        idx = np.concatenate([idx, idx[:20]])  # and some fragments twice
        for lo, hi, b in ((1, 1000, 1), (20, 45_000, 44)):
            got, kept = M.restated_motif_lengths(H.Bases(seq), s[idx], e[idx], q[idx], k, shift, lo, hi, b, 30)
            want, want_kept = M.looped_motif_lengths(seq, s[idx], e[idx], q[idx], k, shift, lo, hi, b, 30)
            assert got.dtype == np.int64 and got.shape == (2, M.n_rows_of(lo, hi, b), 4 ** k + 1)
            assert np.array_equal(got, want) and np.array_equal(kept, want_kept) and kept.sum() > 50


@pytest.mark.parametrize("k", M.KS)
def test_every_row_sums_to_the_kept_fragments(genome, k):
    seqs, frags = genome
    for name, seq in seqs.items():
        s, e, q = frags[name]
        ln = e.astype(np.int64) - s
        for shift in (0, -(k // 2)):
            for lo, hi, b in ((1, 1024, 1), (1, 40_960, 40), (100, 220, 7)):
                table, kept = M.restated_motif_lengths(H.Bases(seq), s, e, q, k, shift, lo, hi, b, 30)
                assert M.row_sums_hold(table, kept)
                assert kept.sum() == int(((q >= 30) & (ln >= lo) & (ln <= hi)).sum())
                assert lo != 1 or (table[0, :, -1].sum() > 0 and table[1, :, -1].sum() > 0)  # undefined readings at either end
    # the hand-placed lengths: both sides of every band start of every k, and len_lo, len_hi, len_hi + 1 of the 1024-row plan
    bands = lds_rows()
    assert all(1 <= bands[k] <= M.MAX_ROWS for k in M.KS) and bands[4] < bands[3] < bands[2] <= bands[1]
    for name, (s, e, q) in frags.items():
        ln = (e.astype(np.int64) - s)[q >= 30]
        for v in M.band_starts(bands.values()) + [1, 1024, 1025]:
            assert (ln == v).any() and (v == 1 or (ln == v - 1).any()), (name, v)


def hand_made():
    """k = 1, four rows of 10 lengths from 100: a uniform row, a single motif, an empty row, undefined readings only."""
    from finaletoolkit_amd import utils
    table = np.zeros((2, 4, 5), np.int64)
    table[0, 0] = [5, 5, 5, 5, 0]
    table[1, 0] = [20, 0, 0, 0, 0]
    table[0, 1] = [0, 0, 7, 0, 1]
    table[1, 1] = [2, 2, 0, 4, 0]
    table[:, 3] = [0, 0, 0, 0, 3]
    return utils.MotifLengths(table, np.array([20, 8, 0, 3], np.int64), 1, "end", 100, 10, ("chrUn",))


def test_frequency_mds_and_pooled():
    from finaletoolkit_amd import utils
    assert utils.MotifLengths._fields == ("table", "n_kept", "k", "kind", "min_length", "length_bin", "skipped_contigs")
    res = hand_made()
    assert res.lengths().tolist() == [100, 110, 120, 130] and res.lengths().dtype == np.int64
    assert res.motifs() == ["A", "C", "G", "T"] and res._replace(k=2).motifs()[:5] == ["AA", "AC", "AG", "AT", "CA"]
    f = res.frequency()
    assert f.shape == (2, 4, 4) and f.dtype == np.float64
    assert f[0, 0].tolist() == [0.25] * 4 and f[1, 0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert f[0, 1].tolist() == [0.0, 0.0, 1.0, 0.0]  # over the DEFINED motifs: the undefined reading is left out
    assert f[1, 1].tolist() == [0.25, 0.25, 0.0, 0.5]
    assert np.isnan(f[:, 2]).all() and np.isnan(f[:, 3]).all()  # an empty row; a row with nothing defined
    mds = res.mds()
    assert mds.shape == (3, 4) and mds.dtype == np.float64
    assert mds[0, 0] == 1.0 and mds[1, 0] == 0.0 and mds[0, 1] == 0.0  # uniform; a single motif
    assert mds[1, 1] == pytest.approx(-(2 * 0.25 * math.log(0.25) + 0.5 * math.log(0.5)) / math.log(4), rel=1e-15)
    p = np.array([25, 5, 5, 5]) / 40  # both ends of row 0 pooled
    assert mds[2, 0] == pytest.approx(-(p * np.log(p)).sum() / math.log(4), rel=1e-15)
    assert np.isnan(mds[:, 2]).all() and np.isnan(mds[:, 3]).all()
    # the reference's motif_diversity_score on the same frequencies
    from finaletoolkit_amd.frag._motif_common import normalized_shannon_mds
    assert mds[1, 1] == pytest.approx(normalized_shannon_mds(f[1, 1], 1), rel=1e-15)
    two = utils.MotifLengths(np.ones((2, 1, 17), np.int64), np.array([17]), 2, "breakpoint", 1, 1, ())
    assert np.allclose(two.mds(), 1.0, rtol=1e-15, atol=0) and two.mds().shape == (3, 1)
    # pooled: whole rows
    assert np.array_equal(res.pooled(100, 139), res.table.sum(axis=1)) and res.pooled(100, 139).shape == (2, 5)
    assert np.array_equal(res.pooled(110, 119), res.table[:, 1]) and np.array_equal(res.pooled(100, 119), res.table[:, :2].sum(axis=1))
    assert np.array_equal(res.pooled(130, 133), res.table[:, 3])  # the last row may be narrower: any end inside it
    for lo, hi in ((99, 139), (100, 140), (105, 119), (100, 115), (120, 119)):
        with pytest.raises(ValueError, match="length range"):
            res.pooled(lo, hi)


def parse_rows(text, res):
    """The table of a rows TSV back."""
    from finaletoolkit_amd import writers
    lines = text.splitlines()
    assert lines[0] + "\n" == writers.MOTIF_LENGTH_HEADER
    assert lines[0].split("\t") == ["length_lo", "length_hi", "end", "motif", "count", "frequency"]
    names = res.motifs() + ["N"]
    first = res.lengths().tolist()
    table = np.zeros_like(res.table)
    rows = [ln.split("\t") for ln in lines[1:]]
    for lo, hi, end, motif, count, freq in rows:
        assert int(hi) == int(lo) + res.length_bin - 1
        cell = ("UD".index(end), first.index(int(lo)), names.index(motif))
        assert table[cell] == 0
        table[cell] = int(count)
    return table, rows


def parse_summary(text):
    from finaletoolkit_amd import writers
    lines = text.splitlines()
    assert lines[0] + "\n" == writers.MOTIF_LENGTH_SUMMARY_HEADER
    assert lines[0].split("\t") == ["length_lo", "length_hi", "n_frags", "undefined_u", "undefined_d", "mds_u", "mds_d", "mds"]
    return [ln.split("\t") for ln in lines[1:]]


def test_tsv_text_rows():
    from finaletoolkit_amd import writers
    res = hand_made()
    table, rows = parse_rows(writers.motif_length_text(res), res)
    assert np.array_equal(table, res.table) and len(rows) == int((res.table != 0).sum())  # one row per non-zero cell
    by_key = {(int(r[0]), r[2], r[3]): r for r in rows}
    assert by_key[(100, "U", "A")] == ["100", "109", "U", "A", "5", "0.25"]
    assert by_key[(110, "U", "N")] == ["110", "119", "U", "N", "1", "nan"]  # the undefined column: a count, no frequency
    assert by_key[(110, "U", "G")][4:] == ["7", "1.0"] and by_key[(110, "D", "T")][4:] == ["4", "0.5"]
    assert by_key[(130, "D", "N")][4:] == ["3", "nan"] and not any(r[0] == "120" for r in rows)
    summary = parse_summary(writers.motif_length_summary_text(res))
    assert [r[:5] for r in summary] == [["100", "109", "20", "0", "0"], ["110", "119", "8", "1", "0"], ["130", "139", "3", "3", "3"]]
    assert summary[0][5:] == ["1.0", "0.0", repr(float(res.mds()[2, 0]))] and summary[2][5:] == ["nan", "nan", "nan"]


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_tsv_round_trip(tmp_path, suffix, genome):
    from finaletoolkit_amd import utils, writers
    seqs, frags = genome
    s, e, q = frags["eB"]
    for k, kind, shift, lo, hi, b in ((4, "end", 0, 1, 1000, 1), (2, "breakpoint", -1, 50, 45_000, 50)):
        table, kept = M.restated_motif_lengths(H.Bases(seqs["eB"]), s, e, q, k, shift, lo, hi, b)
        res = utils.MotifLengths(table, kept, k, kind, lo, b, ())
        out, summ = str(tmp_path / (f"rows{k}" + suffix)), str(tmp_path / (f"summary{k}" + suffix))
        writers.write_motif_length_rows(out, res)
        writers.write_motif_length_summary(summ, res)
        texts = []
        for path in (out, summ):
            raw = open(path, "rb").read()
            assert (raw[:2] == b"\x1f\x8b") == suffix.endswith(".gz")
            texts.append(gzip.open(path, "rt").read() if suffix.endswith(".gz") else raw.decode())
        assert texts[0] == writers.motif_length_text(res) and texts[1] == writers.motif_length_summary_text(res)
        got, rows = parse_rows(texts[0], res)
        assert np.array_equal(got, table) and table[..., -1].any() and any(r[3] == "N" for r in rows)
        f = np.concatenate([res.frequency(), np.full(table.shape[:2] + (1,), np.nan)], axis=-1)
        names, first = res.motifs() + ["N"], res.lengths().tolist()
        for r_lo, _, end, motif, count, freq in rows:
            v = f["UD".index(end), first.index(int(r_lo)), names.index(motif)]
            assert (freq == "nan") == bool(np.isnan(v)) and (freq == "nan" or float(freq) == v)
        summary = parse_summary(texts[1])
        populated = np.flatnonzero(kept)
        assert [int(r[0]) for r in summary] == res.lengths()[populated].tolist()
        assert [int(r[2]) for r in summary] == kept[populated].tolist()
        assert [int(r[3]) for r in summary] == table[0, populated, -1].tolist()
        assert [int(r[4]) for r in summary] == table[1, populated, -1].tolist()
        mds = res.mds()[:, populated]
        for j, r in enumerate(summary):
            for text_v, v in zip(r[5:], mds[:, j]):
                assert (text_v == "nan") == bool(np.isnan(v)) and (text_v == "nan" or float(text_v) == v)
    for write in (writers.write_motif_length_rows, writers.write_motif_length_summary):
        with pytest.raises(ValueError, match="suffix"):
            write(str(tmp_path / "rows.txt"), res)


def test_signature():
    from finaletoolkit_amd import utils
    sig = inspect.signature(utils.frag_motif_lengths)
    assert list(sig.parameters) == ["input_file", "reference_file", "output_file", "summary_file", "contig", "k", "kind", "min_length",
                                    "max_length", "length_bin", "quality_threshold", "workers", "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["input_file"] is inspect.Parameter.empty and d["reference_file"] is inspect.Parameter.empty
    assert (d["output_file"], d["summary_file"], d["contig"], d["k"], d["kind"], d["min_length"], d["max_length"], d["length_bin"],
            d["quality_threshold"], d["workers"], d["verbose"]) == (None, None, None, 4, "end", 1, 1000, 1, 30, None, False)


@pytest.mark.parametrize("kwargs, match", [
    (dict(k=3, kind="breakpoint"), "even"),
    (dict(k=1, kind="breakpoint"), "even"),
    (dict(k=5), "invalid k"),
    (dict(k=0), "invalid k"),
    (dict(kind="middle"), "kind"),
    (dict(min_length=1, max_length=1025), "rows"),           # 1025 rows
    (dict(min_length=100, max_length=100 + 1024 * 7, length_bin=7), "rows"),
    (dict(min_length=0), "lengths"),
    (dict(min_length=200, max_length=199), "lengths"),
    (dict(max_length=(1 << 30) + 1, length_bin=1 << 21), "lengths"),
    (dict(length_bin=0), "lengths"),
    (dict(output_file="out.tsv.bgz"), "output_file.*suffix"),
    (dict(output_file="out.txt"), "output_file.*suffix"),
    (dict(output_file="-"), "suffix"),
    (dict(summary_file="summary.csv"), "summary_file.*suffix"),
])
def test_bad_arguments_raise_before_any_file_is_opened(tmp_path, kwargs, match):
    from finaletoolkit_amd import utils
    missing_in = str(tmp_path / "no_such_input.frag.gz")
    missing_ref = str(tmp_path / "no_such_reference.2bit")
    for key in ("output_file", "summary_file"):
        if kwargs.get(key) not in (None, "-"):
            kwargs = dict(kwargs, **{key: str(tmp_path / kwargs[key])})
    with pytest.raises(ValueError, match=match):
        utils.frag_motif_lengths(missing_in, missing_ref, **kwargs)
    assert os.listdir(tmp_path) == []


def test_parser_maps_flags_onto_the_arguments():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.motiflengths import build_parser
    sig = inspect.signature(utils.frag_motif_lengths)
    ap = build_parser()
    flags = [a.dest for a in ap._actions if a.dest != "help"]
    assert sorted(flags) == sorted(sig.parameters)  # every flag an argument and every argument a flag
    d = {k: v.default for k, v in sig.parameters.items()}
    got = vars(ap.parse_args(["in.bam", "ref.2bit", "out.tsv"]))
    assert got == dict(d, input_file="in.bam", reference_file="ref.2bit", output_file="out.tsv")
    got = vars(ap.parse_args(["in.frag.gz", "hg38.fa", "out.tsv.gz", "--summary", "s.tsv", "-c", "chr7", "-k", "2", "--kind", "breakpoint",
                              "--min-length", "50", "--max-length", "600", "--length-bin", "5", "-q", "5", "-w", "3", "-v"]))
    assert got == dict(input_file="in.frag.gz", reference_file="hg38.fa", output_file="out.tsv.gz", summary_file="s.tsv", contig="chr7",
                       k=2, kind="breakpoint", min_length=50, max_length=600, length_bin=5, quality_threshold=5, workers=3, verbose=True)
    for bad in (["in", "ref"], ["a", "b", "c", "--kind", "middle"], ["a", "b", "c", "-k"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.motiflengths", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "REF" in r.stdout
    for flag in ("--summary", "--kind", "--min-length", "--max-length", "--length-bin", "-k", "-q", "-c"):
        assert flag in r.stdout, flag


def test_flat_names():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    names = {"frag_motif_lengths", "MotifLengths"}
    assert names <= set(dir(f)) and names <= set(utils.__all__) and names <= set(f._FLAT_BY_MODULE["utils"])
    assert f.frag_motif_lengths is utils.frag_motif_lengths and f.MotifLengths is utils.MotifLengths
    code = ("import finaletoolkit_amd as f\n"
            "f.install_alias()\n"
            "import finaletoolkit\n"
            "from finaletoolkit_amd import utils\n"
            "assert finaletoolkit.frag_motif_lengths is utils.frag_motif_lengths and finaletoolkit.utils.MotifLengths is utils.MotifLengths\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_symbols_exported_and_declared():
    from finaletoolkit_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ftk.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTS
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"^#define FTK_MOTIFLEN_MAX_K 4$", header, re.M) and L.MOTIFLEN_MAX_K == 4 == M.MAX_K
    assert re.search(r"^#define FTK_MOTIFLEN_MAX_ROWS 1024$", header, re.M) and L.MOTIFLEN_MAX_ROWS == 1024 == M.MAX_ROWS
    assert "motif x length" in header
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    # the LDS query needs no device: a band of u32 cells [row][kind][4^k + 1] within 64 KiB, fewer rows the longer the motif
    fit = lds_rows()
    assert all(1 <= fit[k] and fit[k] * 2 * (4 ** k + 1) * 4 <= 64 << 10 for k in M.KS)
    assert fit[1] >= fit[2] > fit[3] > fit[4] and fit[4] + 1 <= M.MAX_ROWS
    assert lib.ftk_motif_length_lds_rows(0) == 0 and lib.ftk_motif_length_lds_rows(5) == 0 and lib.ftk_motif_length_lds_rows(-1) == 0
