"""bann_finalize's layout planner (csrc/finalize_layout.h): plan_layout and choose_gsum.

CPU test: a stand-alone host program (finalize_layout_check.cpp), built here with the host
C++ compiler against the HIP headers only, plans a fixed table of cases -- every path
boundary, every EnvOptions field the planner reads, n up to 10^7 -- asserts the invariants
of any layout and prints every planned field; the print must equal
tests/golden/finalize_layout.txt, recorded from the mechanical move of the old bann_finalize
body, byte for byte."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
GOLDEN = os.path.join(ROOT, "tests", "golden", "finalize_layout.txt")


def test_planned_layout_matches_golden_and_keeps_its_invariants(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "finalize_layout_check")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                          "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                          os.path.join(ROOT, "tests", "finalize_layout_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    got, want = run.stdout.splitlines(), open(GOLDEN).read().splitlines()
    diff = [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff and len(got) == len(want), (len(got), len(want), diff[:5])
    assert run.stdout == open(GOLDEN).read()
