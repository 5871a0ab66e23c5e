"""
CPU: the interior of a window's candidate range and the counts a feature block takes from its length histogram
(csrc/ftk_feat_interior.h), checked by the stand-alone program tools/check_feat_interior.cpp against a naive
per-fragment statement of the histogram, coverage and the two DELFI counts: every window start across two multiples of
512 with a dozen lengths each, ws = 0 and below, zero-length fragments at ws, fragments at we - lmax - 1, we - lmax and
we - lmax + 1, windows shorter than lmax + 512, a contig whose fragments all have length zero, the last partial
window, the same shapes just below 2^30 and the clamped bounds.  The second test runs the same program, as a host
program of its own, built with -fsanitize=undefined,address.
"""
import os
import shutil
import subprocess

import pytest

from tests.helpers import ROOT


def _cxx():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "finaletoolkit_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_feat_interior.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failures" and len(lines) == 2, r.stdout[-2000:] + r.stderr[-4000:]
    n = {k: int(v) for k, v in (w.split("=") for w in lines[0].split())}
    assert n["windows"] > 50_000 and n["interior"] > 10_000 and n["no_interior"] > 10_000, lines[0]
    assert n["interior_fragments"] > 10_000_000 and n["edge_fragments"] > 10_000_000, lines[0]
    assert min(n["below_cut"], n["at_cut"], n["above_cut"]) > 10_000 and n["zero_length_at_ws"] > 1_000, lines[0]
    assert n["short_windows"] > 10_000 and n["ws_zero"] > 50 and n["aligned"] > 50 and n["partial_last"] > 10_000, lines[0]
    assert n["empty_ranges"] > 100 and n["clamped"] > 100, lines[0]


def test_the_block_form_equals_the_naive_counts(tmp_path):
    _build_and_run(tmp_path, "check_feat_interior", [])


def test_the_rule_overflows_nowhere(tmp_path):
    san = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    # the runtimes linked into the program where the compiler can (gcc: they are shared objects by default)
    for extra in (["-static-libasan", "-static-libubsan"], []):
        probe = subprocess.run([_cxx(), *san, *extra, "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                               input="int main() { return 0; }\n", capture_output=True, text=True, timeout=300)
        if probe.returncode == 0:
            return _build_and_run(tmp_path, "check_feat_interior_san", ["-g", *san, *extra])
    pytest.skip("this compiler links no sanitizer runtime")
