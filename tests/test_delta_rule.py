"""
CPU: the start column as 1-byte deltas (ds_encode / ds_decode, csrc/ftk_packed.h), checked by the stand-alone program
tools/check_delta_columns.cpp: decoding gives every start back (0, 1, 63, 64, 65 and 129 fragments, runs of one start
longer than a group, starts up to 2^30 - 1), and a group carries the bit exactly when a delta behind its first fragment
exceeds 255 (255 and 256 at every place of a group).
"""
import os
import shutil
import subprocess

from tests.helpers import ROOT


def test_delta_columns_decode_to_the_starts(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "check_delta_columns")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "finaletoolkit_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_delta_columns.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures") and r.stdout.strip() == "0 failures", \
        r.stdout[-2000:] + r.stderr[-2000:]
