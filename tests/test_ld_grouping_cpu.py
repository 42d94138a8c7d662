"""CPU-side checks of group-by-ld: the host functions of csrc/bann_io.cpp (the graph of a PLINK --r2
table, the centered grouping, the writer) against the reference's own known answer and against
tests/ld_reference.py; the same functions in a stand-alone program under AddressSanitizer and
UBSan; the resource report of kernels_ld.hip for gfx950; the new symbols."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ld_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
PLINK = os.path.join(ROOT, "tests", "golden", "plink")
HIPCC = "/opt/rocm/bin/hipcc"
NEW_CTX = ["bann_genotypes_ld_band", "bann_genotypes_ld_graph", "bann_genotypes_ld_graph_get",
           "bann_genotypes_ld_timing", "bann_genotypes_ld_scratch_limit", "bann_bim_read", "bann_ld_graph_read_plink", "bann_grouping_centered",
           "bann_grouping_write"]


def banded_graph(rng, M, reach, p):
    edges = {(j, k) for j in range(M) for k in range(j + 1, min(M, j + reach + 1)) if rng.random() < p}
    return R.adjacency(M, edges)


def test_reference_known_answer():
    """centered.rs:174-192: small.ld over small.bim, min_group_size 1"""
    from bann.io import centered_grouping, read_plink_ld_graph
    off, nb = read_plink_ld_graph(os.path.join(PLINK, "small.ld"), os.path.join(PLINK, "small.bim"))
    assert off.size == 12 and nb.size == 14
    assert R.csr_edges(off, nb) == {(0, 1), (0, 2), (0, 3), (3, 4), (4, 5), (7, 8), (7, 9)}
    groups, ungrouped = centered_grouping(off, nb, 1)
    assert [g.tolist() for g in groups] == [[0, 1, 2, 3], [3, 4, 5], [6, 7, 8, 9, 10]]
    assert all(g.dtype == np.int32 for g in groups) and ungrouped == 0
    want, un = R.centered(R.adjacency(11, R.csr_edges(off, nb)), 1)
    assert want == [[0, 1, 2, 3], [3, 4, 5], [6, 7, 8, 9, 10]] and un == 0


@pytest.mark.parametrize("M,reach,p,min_size,seed", [
    (11, 3, 0.5, 1, 0), (72, 6, 0.4, 1, 1), (100, 8, 0.3, 1, 2), (300, 6, 0.4, 1, 3), (300, 6, 0.4, 3, 4),
    (150, 12, 0.6, 3, 5), (40, 2, 0.2, 0, 6)])
def test_centered_grouping_equals_restatement(M, reach, p, min_size, seed):
    from bann.io import centered_grouping
    adj = banded_graph(np.random.default_rng(seed), M, reach, p)
    want, want_un = R.centered(adj, min_size)
    off, nb = R.csr(adj)
    groups, ungrouped = centered_grouping(off, nb, min_size)
    print(f"M={M} min_size={min_size}: {len(want)} groups, {want_un} ungrouped")
    assert [g.tolist() for g in groups] == want
    assert ungrouped == want_un
    grouped = set().union(*want) if want else set()
    assert want_un == M - len(grouped)
    if M == 300:  # groups are looked up by GROUP index: the markers past 99 + G find none
        assert want_un > 0 and len(want) > 0
    if M <= 100 and min_size == 1:
        assert want_un == 0


def test_writer_reader_round_trip(tmp_path):
    from bann.io import read_grouping, write_grouping
    groups = [np.array([3, 0, 7], np.int32), np.array([7, 12], np.int32), np.array([5], np.int32)]
    path = str(tmp_path / "x.groups")
    write_grouping(path, groups)
    assert open(path, "rb").read() == b"3\t0\n0\t0\n7\t0\n7\t1\n12\t1\n5\t2\n"
    back = read_grouping(path)
    assert [g.tolist() for g in back] == [g.tolist() for g in groups]


def test_read_bim_mixed_whitespace(tmp_path):
    from bann.io import read_bim
    chrom, bp = read_bim(os.path.join(PLINK, "small.bim"))
    assert chrom.dtype == np.int32 and bp.dtype == np.int64
    assert chrom.tolist() == [0] * 11 and bp.tolist() == list(range(1, 12))
    p = tmp_path / "two.bim"
    p.write_text("7\ta 0 10 A C\nX b\t0   25 A C\n7 c 0 31 A C\n")
    chrom, bp = read_bim(str(p))
    assert chrom.tolist() == [0, 1, 0] and bp.tolist() == [10, 25, 31]


def test_error_codes(tmp_path):
    from bann import BannError
    from bann.io import read_bim, read_plink_ld_graph
    bim = os.path.join(PLINK, "small.bim")
    unk = tmp_path / "unknown.ld"
    unk.write_text(" CHR_A BP_A SNP_A CHR_B BP_B SNP_B R2\n 19 1 rs1 19 2 rs404 1\n")
    with pytest.raises(BannError) as e:
        read_plink_ld_graph(str(unk), bim)
    assert e.value.code == -5 and "rs404" in str(e.value)
    short = tmp_path / "short.ld"
    short.write_text(" CHR_A BP_A SNP_A CHR_B BP_B SNP_B R2\n 19 1 rs1 19 2\n")
    with pytest.raises(BannError) as e:
        read_plink_ld_graph(str(short), bim)
    assert e.value.code == -2
    with pytest.raises(BannError) as e:
        read_plink_ld_graph(str(tmp_path / "none.ld"), bim)
    assert e.value.code == -5
    with pytest.raises(BannError) as e:
        read_bim(str(tmp_path / "none.bim"))
    assert e.value.code == -5


def test_host_functions_under_sanitizers(tmp_path):
    """tests/ld_grouping_check.cpp + csrc/bann_io.cpp alone, -fsanitize=address,undefined, as a child
    process: the known answer, an empty graph, a graph with no group, a truncated .ld, a one-column .bim"""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ld_grouping_check")
    # the sanitizer runtimes are linked statically: the program then does not care what else the
    # process loads or in which order, and runs in the environment it is given
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                          "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                          os.path.join(ROOT, "tests", "ld_grouping_check.cpp"), os.path.join(CSRC, "bann_io.cpp"),
                          "-o", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe, os.path.join(PLINK, "small.ld"), os.path.join(PLINK, "small.bim"), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ld_kernels_do_not_spill(tmp_path):
    """kernels_ld.hip for gfx950 with the product's flags: no VGPR or SGPR spill, no scratch"""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-c",
                          os.path.join(CSRC, "kernels_ld.hip"), "-o", str(tmp_path / "k.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    for k in ("k_ld_stats", "k_ld_band", "k_ld_r2", "k_ld_mask"):
        assert any(k in f for f in res), (k, sorted(res))
    for k, v in res.items():
        assert v == {"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize": 0}, (k, v)


def test_new_symbols_in_headers_library_and_binding():
    import ctypes
    import bann._lib as L
    from bann import BannContext
    import bann.io as IO
    hdr = open(os.path.join(ROOT, "include", "bann.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "rs-bann_amd", "librsbann_amd.so"))
    for f in NEW_CTX:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
        assert f in L.SIGNATURES, f
        assert hasattr(lib, f), f
    # the message carrier of the host-only functions returns a string
    assert re.search(r"\bconst char\* bann_io_last_error\s*\(void\)", hdr)
    assert "bann_io_last_error" in L.SIGNATURES and hasattr(lib, "bann_io_last_error")
    lib.bann_io_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.bann_io_last_error(), bytes)
    for name in ("ld_band", "ld_graph", "ld_timing", "ld_scratch_limit"):
        assert callable(getattr(BannContext, name))
    for name in ("read_bim", "read_plink_ld_graph", "centered_grouping", "write_grouping", "group_by_ld"):
        assert callable(getattr(IO, name))
