"""The digit-pair combine of the fx forward (csrc/fx_combine.h) on the host.

CPU test: a stand-alone host program (fx_combine_check.cpp, its own main), built with the host C++
compiler and -fsanitize=address,undefined and run directly.  It draws a few million cumulative
fragment sets at the header's int32 bound, adds the extreme tile (every digit +-64, every operand byte
at its maximum, 512 markers), and asserts that the pair-combined field integers equal an int64
reference exactly, that the float value is within 1 ulp of the exact value converted once, that a
field's weight 4^q taken back as 4^-q leaves the bits of k_forward_fi's x 16 form, and that the
largest |hi| and |lo| it saw (printed) are below 2^31."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")


def test_pair_combine_matches_int64_reference_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fx_combine_check")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                          "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                          os.path.join(ROOT, "tests", "fx_combine_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-2000:])
    assert run.stdout.rstrip().endswith("ok")
    m = re.search(r"checked (\d+) fragment sets", run.stdout)
    assert m and int(m.group(1)) >= 3_000_000
    m = re.search(r"max \|hi\| = (\d+), max \|lo\| = (\d+)", run.stdout)
    assert m and int(m.group(1)) < 2 ** 31 and int(m.group(2)) < 2 ** 31


def test_header_is_host_only():
    """fx_combine.h makes no HIP call and includes no HIP header, so a host program can include it"""
    txt = open(os.path.join(CSRC, "fx_combine.h")).read()
    assert "hip/" not in txt and "__builtin_amdgcn" not in txt
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', txt) == ["math.h", "stdint.h"]
