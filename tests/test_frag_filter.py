"""CPU: the surface of ``frag_filter`` (names, signature, command line, argument errors that need no device), the BED
loader of the region masks, and the yardstick of the GPU tests - a literal restatement of the two intersect-policy
lines - held against ``tests/golden/export_mask.json.gz``, whose rows come from the reference's ``frag_generator`` and
``_make_intersect_checker`` (``tools/gen_golden_mask.py``)."""
import gzip
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "export_mask.json.gz")


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def in_interval(policy, r_start, r_stop, f_start, f_stop):
    """The issue's two lines, literally."""
    if policy == "midpoint":
        return r_start <= (f_start + f_stop) // 2 < r_stop
    if policy == "any":
        return f_stop > r_start and f_start < r_stop
    raise ValueError(policy)


def in_mask(policy, intervals, f_start, f_stop):
    """``intervals``: (start, stop) pairs of the fragment's contig, in any order, overlapping or not."""
    return any(in_interval(policy, a, b, f_start, f_stop) for a, b in intervals)


def restated_keep(policy, s, e, whitelist=None, blacklist=None):
    """bool[n] over the rows (s[i], e[i]); ``whitelist`` / ``blacklist``: lists of (start, stop) or None."""
    keep = np.ones(len(s), bool)
    for i in range(len(s)):
        a, b = int(s[i]), int(e[i])
        if whitelist is not None and not in_mask(policy, whitelist, a, b):
            keep[i] = False
        if blacklist is not None and in_mask(policy, blacklist, a, b):
            keep[i] = False
    return keep


def restated_keep_sorted(policy, s, e, whitelist=None, blacklist=None):
    """``restated_keep`` for many rows and many intervals: the same two lines, evaluated with numpy against every
    interval of a window of candidates (searchsorted only narrows which intervals the lines are applied to: an
    interval that starts behind the fragment's stop, or one that ends in front of its start, satisfies neither)."""
    s = np.asarray(s, np.int64)
    e = np.asarray(e, np.int64)

    def member(iv):
        a = np.array([x for x, _ in iv], np.int64)
        b = np.array([y for _, y in iv], np.int64)
        o = np.argsort(a, kind="stable")
        a, b = a[o], b[o]
        bmax = np.maximum.accumulate(b) if len(b) else b
        out = np.zeros(len(s), bool)
        hi = np.searchsorted(a, np.maximum(e, s + 1), side="right")  # intervals with r_start <= max(stop, start + 1)
        lo = np.searchsorted(bmax, s, side="left")  # in front of lo every r_stop is < start
        for i in range(len(s)):
            for j in range(lo[i], hi[i]):
                if in_interval(policy, int(a[j]), int(b[j]), int(s[i]), int(e[i])):
                    out[i] = True
                    break
        return out
    keep = np.ones(len(s), bool)
    if whitelist is not None:
        keep &= member(whitelist)
    if blacklist is not None:
        keep &= ~member(blacklist)
    return keep


def zero_length_in_any(intervals, x):
    """Is the zero-length fragment [x, x) in the mask under ``any``?"""
    return in_mask("any", intervals, x, x)


def merged_pairs(ms, me):
    return list(zip(ms.tolist(), me.tolist()))


def load_golden():
    return json.loads(gzip.open(GOLDEN, "rb").read())


def write_synth(path, recipe):
    """The golden's synthetic input, rebuilt from the recipe it records (tools/gen_golden_mask.py: write_synth)."""
    from finaletoolkit_amd import bgzf, synth
    bgzf.write_frag_gz(path, [(n, *synth.synth_contig(size, seed=seed, n=rows)) for n, size, rows, seed in recipe["contigs"]])


def write_bed(path, intervals):
    with open(path, "w") as fh:
        for c, a, b in intervals:
            fh.write(f"{c}\t{a}\t{b}\n")
    return str(path)


def parse_rows(text):
    return [(f[0], int(f[1]), int(f[2]), f[3], f[4]) for f in (ln.split("\t") for ln in text.splitlines())]


# ---- 1. surface -----------------------------------------------------------------------------------------------------
def test_flat_name_signature_and_cli_flags():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.filter import build_parser
    assert f.frag_filter is utils.frag_filter and "frag_filter" in dir(f)
    sig = inspect.signature(utils.frag_filter)
    assert list(sig.parameters) == ["input_file", "output_file", "whitelist_file", "blacklist_file", "intersect_policy", "contig",
                                    "quality_threshold", "min_length", "max_length", "layout", "workers", "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["whitelist_file"] is None and d["blacklist_file"] is None and d["intersect_policy"] == "midpoint"
    assert d["contig"] is None and d["quality_threshold"] == 30 and d["min_length"] is None and d["max_length"] is None
    assert d["layout"] == "frag" and d["workers"] is None and d["verbose"] is False
    flags = [a.dest for a in build_parser()._actions if a.dest != "help"]
    assert sorted(flags) == sorted(sig.parameters)  # every flag an argument, every argument a flag
    opts = {o for a in build_parser()._actions for o in a.option_strings}
    assert {"--whitelist", "--blacklist", "--intersect-policy", "--layout", "--min-length", "--max-length"} <= opts
    export_sig = inspect.signature(utils.frag_export)  # frag_export keeps its own parameter list
    assert set(export_sig.parameters) == set(sig.parameters) - {"whitelist_file", "blacklist_file", "intersect_policy"}
    with pytest.raises(AttributeError):
        f.filter_file
    f.install_alias("finaletoolkit", force=True)
    try:
        import finaletoolkit.utils as U
        assert U.frag_filter is utils.frag_filter
    finally:
        for k in [k for k in sys.modules if k == "finaletoolkit" or k.startswith("finaletoolkit.")]:
            del sys.modules[k]


def test_filter_cli_help_exits_zero():
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.filter", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--whitelist" in r.stdout and "--blacklist" in r.stdout and "--intersect-policy" in r.stdout
    assert "{midpoint,any}" in r.stdout and "--layout" in r.stdout


def test_bad_arguments_raise_before_any_device_use(tmp_path):
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.exceptions import InvalidInputError
    src = os.path.join(ROOT, "tests", "data", "12.3444.b37.bam")
    bed = write_bed(tmp_path / "w.bed", [("12", 10, 20)])
    with pytest.raises(ValueError, match="suffix"):
        utils.frag_filter(src, str(tmp_path / "out.bed"), whitelist_file=bed)
    with pytest.raises(ValueError, match="suffix"):
        utils.frag_filter(src, "-")
    with pytest.raises(ValueError, match="layout"):
        utils.frag_filter(src, str(tmp_path / "out.frag.gz"), layout="bed12")
    with pytest.raises(InvalidInputError, match="not a valid policy"):
        utils.frag_filter(src, str(tmp_path / "out.frag.gz"), whitelist_file=bed, intersect_policy="half")
    same = tmp_path / "same.frag.gz"
    same.write_bytes(b"")
    with pytest.raises(ValueError, match="same"):
        utils.frag_filter(str(same), str(same))
    bad = tmp_path / "bad.bed"
    bad.write_text("12\t50\t40\n")
    with pytest.raises(ValueError, match="bad.bed, line 1"):
        utils.frag_filter(src, str(tmp_path / "out.frag.gz"), blacklist_file=str(bad))
    assert not (tmp_path / "out.frag.gz").exists()


# ---- 2. the BED loader -----------------------------------------------------------------------------------------------
def test_loader_sorts_and_merges(tmp_path):
    from finaletoolkit_amd import utils
    text = ("# a comment\ntrack name=x\nbrowser position chr1:1-100\n\n"
            "chr1\t100\t200\tname\t0\t+\n"   # extra columns are ignored
            "chr1\t50\t60\n"                 # unsorted
            "chr1\t150\t300\n"               # overlaps the first
            "chr1\t300\t310\n"               # touches the merged one: stays its own (see merge_intervals)
            "chr1\t311\t320\n"               # one base apart: stays its own
            "chr1\t100\t120\n"               # inside
            "chr2\t5\t6\n"
            "chr1\t50\t60\n"                 # duplicate
            "chr2\t0\t1073741824\n")         # up to the bound
    p = tmp_path / "m.bed"
    p.write_text(text)
    m = utils.read_region_mask(str(p))
    assert list(m) == ["chr1", "chr2"]
    assert m["chr1"][0].tolist() == [50, 100, 300, 311] and m["chr1"][1].tolist() == [60, 300, 310, 320]
    assert m["chr2"][0].tolist() == [0] and m["chr2"][1].tolist() == [1 << 30]
    assert all(a.dtype == np.int32 for pair in m.values() for a in pair)
    gz = tmp_path / "m.bed.gz"
    with gzip.open(gz, "wt") as fh:
        fh.write(text)
    z = utils.read_region_mask(gz)  # (a path object, gzip input)
    assert list(z) == list(m) and all(np.array_equal(z[c][k], m[c][k]) for c in m for k in (0, 1))
    empty = tmp_path / "empty.bed"
    empty.write_text("# nothing\n\n")
    assert utils.read_region_mask(str(empty)) == {}


def test_merge_keeps_both_policies_answers():
    """Neither policy changes when intervals are sorted and overlapping ones merged.  Touching ones are NOT merged:
    a zero-length fragment at the touch point is in neither interval under ``any``, but would be in their union."""
    from finaletoolkit_amd import utils
    rng = np.random.default_rng(17)
    a = rng.integers(0, 3000, 120)
    raw = [(int(x), int(x + w)) for x, w in zip(a, rng.integers(1, 60, 120))]
    raw += [(raw[0][1], raw[0][1] + 5), raw[3]]  # touching, duplicate
    ms, me = utils.merge_intervals([x for x, _ in raw], [y for _, y in raw])
    assert np.all(ms[1:] >= me[:-1]) and np.all(ms < me) and np.any(ms[1:] == me[:-1])  # sorted, disjoint; touching stay
    touch = int(me[:-1][ms[1:] == me[:-1]][0])
    assert not zero_length_in_any(raw, touch) and not zero_length_in_any(merged_pairs(ms, me), touch)
    assert zero_length_in_any([(int(ms.min()), int(me.max()))], touch)
    merged = list(zip(ms.tolist(), me.tolist()))
    s = rng.integers(0, 3100, 3000)
    e = s + rng.integers(0, 200, 3000)  # (zero-length fragments too)
    for policy in ("midpoint", "any"):
        want = restated_keep(policy, s, e, whitelist=raw)
        assert np.array_equal(want, restated_keep(policy, s, e, whitelist=merged))
        assert np.array_equal(want, restated_keep_sorted(policy, s, e, whitelist=raw))
        assert 0 < want.sum() < len(s)


@pytest.mark.parametrize("line, word", [("chr1\t5\n", "three columns"), ("chr1\tx\t9\n", "not integers"), ("chr1\t5\t9.5\n", "not integers"),
                                        ("chr1\t-1\t9\n", "< 0"), ("chr1\t9\t9\n", "<= start"), ("chr1\t9\t3\n", "<= start"),
                                        ("chr1\t5\t1073741825\n", "2\\*\\*30")])
def test_loader_errors_name_file_and_line(tmp_path, line, word):
    from finaletoolkit_amd import utils
    p = tmp_path / "broken.bed"
    p.write_text("# head\nchr1\t1\t2\n" + line)
    with pytest.raises(ValueError, match="broken.bed, line 3.*" + word):
        utils.read_region_mask(str(p))


# ---- 3. the yardstick against the golden -----------------------------------------------------------------------------
def test_restated_policy_lines_reproduce_the_golden():
    G = load_golden()
    assert set(G) == {"fixture", "synth"}
    for tag, g in G.items():
        rows = parse_rows(g["all_rows"])
        assert len(g["cases"]) == 18 and len(rows) >= 17
        seen = set()
        for case in g["cases"]:
            policy = case["policy"]
            keep = np.ones(len(rows), bool)
            for c in dict.fromkeys(r[0] for r in rows):
                idx = [i for i, r in enumerate(rows) if r[0] == c]
                s = [rows[i][1] for i in idx]
                e = [rows[i][2] for i in idx]
                wl = None if case["whitelist"] is None else [(a, b) for cc, a, b in g["masks"][case["whitelist"]] if cc == c]
                bl = None if case["blacklist"] is None else [(a, b) for cc, a, b in g["masks"][case["blacklist"]] if cc == c]
                keep[idx] = restated_keep(policy, s, e, wl, bl)
            want = "".join(ln + "\n" for ln, k in zip(g["all_rows"].splitlines(), keep) if k)
            assert want == case["rows"] and int(keep.sum()) == case["n"], (tag, case["policy"], case["whitelist"], case["blacklist"])
            seen.add((policy, case["whitelist"] is not None, case["blacklist"] is not None))
        assert len(seen) == 6  # both policies x whitelist only, blacklist only, both


def test_golden_synth_recipe_rebuilds_the_rows(tmp_path):
    """The synthetic input is not committed: the tests rebuild it from the recipe; its rows at the golden's MAPQ cut
    are the golden's ``all_rows``."""
    g = load_golden()["synth"]
    p = str(tmp_path / "synth.frag.gz")
    write_synth(p, g["recipe"])
    q = g["quality_threshold"]
    lines = [ln for ln in gzip.open(p, "rt").read().splitlines() if int(ln.split("\t")[3]) >= q]
    assert "".join(ln + "\n" for ln in lines) == g["all_rows"]
    assert len({ln.split("\t")[0] for ln in lines}) == 3
