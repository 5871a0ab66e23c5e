"""
CPU: a fragment's events in a WPS tile (csrc/ftk_wps_events.h: 32-bit tile-relative cells, one OR-ed sign test, the
fetch-window tests only in edge tiles), checked by the stand-alone program tools/check_wps_events.cpp against a naive
64-bit restatement of the chain of compares it replaced: every offset of a fragment against tiles at 0, 4096 and
2^30 - 4096, whole and partial tiles, lengths around W and at 2046, W in {1, 2, 119, 120, 121, 1000}, edge and interior
tiles, the fetch window at every off-by-one around start, midpoint and end, read1 columns.  The second test runs the
same program, as a host program of its own, built with -fsanitize=undefined,address: signed overflow is how this
arithmetic would fail.
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
                    os.path.join(ROOT, "tools", "check_wps_events.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failures" and len(lines) == 2, r.stdout[-2000:] + r.stderr[-4000:]
    n_cases, n_accepted, n_interior = (int(w) for w in lines[0].replace(",", "").split() if w.isdigit())
    assert n_cases > 10_000_000 and n_accepted > 1_000_000 and n_interior > 1_000_000, lines[0]


def test_lean_events_equal_the_naive_form(tmp_path):
    _build_and_run(tmp_path, "check_wps_events", [])


def test_lean_events_overflow_nowhere(tmp_path):
    san = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    # the runtimes linked into the program where the compiler can (gcc: they are shared objects by default)
    for extra in (["-static-libasan", "-static-libubsan"], []):
        probe = subprocess.run([_cxx(), *san, *extra, "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                               input="int main() { return 0; }\n", capture_output=True, text=True, timeout=300)
        if probe.returncode == 0:
            return _build_and_run(tmp_path, "check_wps_events_san", ["-g", *san, *extra])
    pytest.skip("this compiler links no sanitizer runtime")
