"""
CPU: the host rule that decides which calls may read the packed (length, mapq) column (packed_call_ok,
csrc/ftk_packed.h), checked by the stand-alone program tools/check_packed_rule.cpp: no admitted call makes a comparison
that could tell a word - a saturated one included - from the fragment it stands for.
"""
import os
import shutil
import subprocess

from tests.helpers import ROOT


def test_packed_rule_admits_only_exact_calls(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "check_packed_rule")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "finaletoolkit_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_packed_rule.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
