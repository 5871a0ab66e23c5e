"""CPU: the host side of the depth track - ``ftk_format_bedgraph_runs`` against a Python ``"\\t".join``, the output
suffix rule of ``frag_depth_track`` (raised before any file is opened), the command line of
``python -m finaletoolkit_amd.depth`` and the lazy flat names.  The kernels are held against a numpy restatement in
``tests/test_gpu_frag_depth.py``."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def joined_rows(contig, rs, re_, rd):
    return "".join("\t".join((contig, str(int(a)), str(int(b)), str(int(d)))) + "\n" for a, b, d in zip(rs, re_, rd)).encode()


def run_table(n, seed=3):
    """n sorted, disjoint runs with depths on both sides of every digit count (and, as the formatter takes any int32,
    a negative one)."""
    rng = np.random.default_rng(seed)
    gaps = rng.integers(0, 3, n)
    lens = rng.integers(1, 5000, n)
    rs = np.cumsum(gaps + np.concatenate(([0], lens[:-1]))).astype(np.int64)
    re_ = rs + lens
    assert re_[-1] < 2 ** 31 if n else True
    rd = rng.choice(np.array([0, 1, 9, 10, 99, 100, 65535, 65536, 70000, 2 ** 31 - 1, -1], np.int64), n)
    return rs.astype(np.int32), re_.astype(np.int32), rd.astype(np.int32)


@pytest.mark.parametrize("name", ["c", "n" * 255])
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("n", [0, 1, 100_003])
def test_format_bedgraph_runs_equals_python_join(n, threads, name):
    from finaletoolkit_amd import writers
    rs, re_, rd = run_table(n) if n else (np.zeros(0, np.int32),) * 3
    with writers.bedgraph_runs(name, rs, re_, rd, threads) as buf:
        got = buf.tobytes()
    assert got == joined_rows(name, rs, re_, rd)
    assert got.count(b"\n") == n


def test_format_bedgraph_runs_bad_arguments():
    import ctypes as C

    from finaletoolkit_amd import _lib as L
    from finaletoolkit_amd import writers
    lib = L.load()
    out, n = C.c_void_p(), C.c_int64()
    a = np.zeros(2, np.int32)
    assert lib.ftk_format_bedgraph_runs(None, L.ptr(a), L.ptr(a), L.ptr(a), 2, 1, C.byref(out), C.byref(n)) == L.FTK_ERR_INVALID
    assert lib.ftk_format_bedgraph_runs(b"c", None, L.ptr(a), L.ptr(a), 2, 1, C.byref(out), C.byref(n)) == L.FTK_ERR_INVALID
    assert lib.ftk_format_bedgraph_runs(b"c", L.ptr(a), L.ptr(a), L.ptr(a), -1, 1, C.byref(out), C.byref(n)) == L.FTK_ERR_INVALID
    assert lib.ftk_format_bedgraph_runs(b"c", L.ptr(a), L.ptr(a), L.ptr(a), 2, 1, None, C.byref(n)) == L.FTK_ERR_INVALID
    with pytest.raises(ValueError, match="length"):
        writers.bedgraph_runs("c", a, a[:1], a)


@pytest.mark.parametrize("name", ["out.bed", "out.bedgraph.bgz", "out.bg.gzip", "out.gz", "out.wig", "-", "out.bedgraph.gz.tmp"])
def test_suffix_check_raises_before_any_file_is_opened(tmp_path, name):
    from finaletoolkit_amd import utils
    missing = str(tmp_path / "no_such_input.frag.gz")  # (opening it would be a different error)
    target = name if name == "-" else str(tmp_path / name)
    with pytest.raises(ValueError, match="suffix"):
        utils.frag_depth_track(missing, target)
    assert os.listdir(tmp_path) == []


def test_signatures_and_parser_round_trip():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.depth import build_parser
    sig = inspect.signature(utils.frag_depth_track)
    assert list(sig.parameters) == ["input_file", "output_file", "contig", "quality_threshold", "min_length", "max_length",
                                    "include_zero", "workers", "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["contig"] is None and d["quality_threshold"] == 30 and d["min_length"] is None and d["max_length"] is None
    assert d["include_zero"] is False and d["workers"] is None and d["verbose"] is False
    assert list(inspect.signature(utils.frag_depth).parameters) == ["input_file", "contig", "start", "stop", "quality_threshold",
                                                                    "min_length", "max_length", "workers"]
    ap = build_parser()
    flags = [a.dest for a in ap._actions if a.dest != "help"]
    assert sorted(flags) == sorted(sig.parameters)  # every flag an argument, every argument a flag
    # defaults
    got = vars(ap.parse_args(["in.bam", "out.bg"]))
    assert got == dict(input_file="in.bam", output_file="out.bg", **{k: v for k, v in d.items() if k not in ("input_file", "output_file")})
    # every flag, short and long spellings
    got = vars(ap.parse_args(["in.frag.gz", "out.bedgraph.gz", "-c", "chr7", "-q", "5", "--min-length", "120", "--max-length", "180",
                              "--include-zero", "-w", "3", "-v"]))
    assert got == dict(input_file="in.frag.gz", output_file="out.bedgraph.gz", contig="chr7", quality_threshold=5, min_length=120,
                       max_length=180, include_zero=True, workers=3, verbose=True)
    got = vars(ap.parse_args(["a", "b", "--contig", "12", "--min-mapq", "0", "--workers", "8", "--verbose"]))
    assert (got["contig"], got["quality_threshold"], got["workers"], got["verbose"], got["include_zero"]) == ("12", 0, 8, True, False)
    with pytest.raises(SystemExit):
        ap.parse_args(["only_one"])


def test_depth_cli_help_exits_zero():
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.depth", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--include-zero" in r.stdout and "--min-length" in r.stdout and "--workers" in r.stdout


def test_flat_names_resolve_lazily_without_the_library():
    code = ("import sys, finaletoolkit_amd as f\n"
            "assert 'finaletoolkit_amd.utils' not in sys.modules\n"
            "fn = f.frag_depth_track\n"
            "from finaletoolkit_amd import utils, _lib\n"
            "assert fn is utils.frag_depth_track and f.frag_depth is utils.frag_depth\n"
            "assert 'frag_depth' in dir(f) and 'frag_depth_track' in dir(f)\n"
            "assert _lib._lib is None, 'the flat name loaded libftk_hip.so'\n"
            "assert not any('libftk_hip' in line for line in open('/proc/self/maps'))\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
