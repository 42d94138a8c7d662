"""The gx tile numbering (csrc/gx_shapes.h): gx_dims, which the GEMM kernels number their
workgroups by, and gx_tiles, by which build_plan sizes their launches.

CPU test: a stand-alone host program (gx_shapes_check.cpp), built here with the host C++
compiler against the HIP headers only, prints gx_tiles for a fixed table -- every phase and
layer of the gx parity shapes and of a 4096-unit summary layer, exact and not, 1 and 3 row
splits, n up to 10^7 -- and asserts that every count is gx_dims' tmc * tnc * ns, is 0 where
the phase has no such layer and stays below the 2^30 tiles of one launch; the print must
equal tests/golden/gx_tiles.txt, recorded from the host-side gx_tiles that restated the
numbering before the two were made one, byte for byte."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gx_tiles.txt")


def test_tile_counts_match_golden_and_the_device_numbering(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gx_shapes_check")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                          "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                          os.path.join(ROOT, "tests", "gx_shapes_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    got, want = run.stdout.splitlines(), open(GOLDEN).read().splitlines()
    diff = [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff and len(got) == len(want), (len(got), len(want), diff[:5])
    assert len(want) == 2 * 2 * 6 * 7
    assert run.stdout == open(GOLDEN).read()
