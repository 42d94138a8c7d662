"""CPU-side checks of the cohort subset: the index-list helpers of bann.io, read_fam, the numpy oracle
itself, the new entry points in the header, the binding and the built library, and the resource report
of kernels_subset.hip for gfx950."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import subset_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
LIB = os.path.join(ROOT, "rs-bann_amd", "librsbann_amd.so")
PLINK = os.path.join(ROOT, "tests", "golden", "plink")
HIPCC = "/opt/rocm/bin/hipcc"
NEW_FUNCTIONS = ["bann_genotypes_subset", "bann_genotypes_subset_timing", "bann_genotypes_fill_missing_a2"]
NEW_KERNELS = ["k_subsetPK", "k_subset_rows"]


@pytest.mark.parametrize("n,test_n", [(2, 1), (10, 3), (257, 86), (1000, 999)])
def test_split_indices(n, test_n):
    from bann.io import split_indices
    train, test = split_indices(n, test_n, seed=7)
    assert train.dtype == np.int64 and test.dtype == np.int64
    assert test.size == test_n and train.size == n - test_n
    assert np.all(np.diff(train) > 0) and np.all(np.diff(test) > 0)          # ascending, no repeat
    assert np.intersect1d(train, test).size == 0
    assert np.array_equal(np.sort(np.concatenate([train, test])), np.arange(n))
    again = split_indices(n, test_n, seed=7)
    assert np.array_equal(again[0], train) and np.array_equal(again[1], test)
    if n >= 257:
        assert not np.array_equal(split_indices(n, test_n, seed=8)[1], test)


@pytest.mark.parametrize("test_n", [0, 10, -1, 11])
def test_split_indices_refuses_an_empty_side(test_n):
    from bann.io import split_indices
    with pytest.raises(ValueError):
        split_indices(10, test_n, seed=1)


@pytest.mark.parametrize("n,k", [(2, 2), (10, 3), (10, 10), (257, 5), (1000, 7)])
def test_kfold_indices(n, k):
    from bann.io import kfold_indices
    folds = kfold_indices(n, k, seed=3)
    assert len(folds) == k
    sizes = [f.size for f in folds]
    assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 1
    for f in folds:
        assert f.dtype == np.int64 and np.all(np.diff(f) > 0)
    assert np.array_equal(np.sort(np.concatenate(folds)), np.arange(n))      # disjoint and covering
    again = kfold_indices(n, k, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(folds, again))


@pytest.mark.parametrize("n,k", [(5, 6), (5, 1), (5, 0)])
def test_kfold_indices_refuses(n, k):
    from bann.io import kfold_indices
    with pytest.raises(ValueError):
        kfold_indices(n, k, seed=3)


def test_read_fam():
    from bann.io import bed_dims, read_fam
    path = os.path.join(PLINK, "small.fam")
    lines, count = read_fam(path)
    raw = open(path, "rb").read()
    assert count == len(lines) == bed_dims(os.path.join(PLINK, "small"))[0]
    assert b"".join(lines) == raw                                            # verbatim, line ends included
    assert all(len(line.split()) == 6 for line in lines)


def test_reference_on_a_hand_written_case():
    g = np.array([[0, 1, 2, -1, 1],
                  [2, 2, 0, 1, -1],
                  [1, -1, 0, 0, 2]], np.int8)
    assert np.array_equal(S.subset(g), g)
    assert S.subset(g, individuals=[4, 0]).tolist() == [[1, 0], [-1, 2], [2, 1]]
    assert S.subset(g, markers=[2, 2, 0]).tolist() == [[1, -1, 0, 0, 2], [1, -1, 0, 0, 2], [0, 1, 2, -1, 1]]
    assert S.subset(g, individuals=[3, 3, 1], markers=[1, 0]).tolist() == [[1, 1, 2], [-1, -1, 1]]
    assert S.zero_coded(g)[0].tolist() == [0, 1, 2, 0, 1]
    # the decoder against the library's encoder, and against bytes written by hand
    from bann.io import encode_bed_payload
    assert np.array_equal(S.decode_bed(encode_bed_payload(g), 5, 3), g)
    assert np.array_equal(S.decode_bed(b"\x6c\x1b\x01" + bytes([0b01111000, 0]), 5, 1), [[2, 1, 0, -1, 2]])
    c = S.cohort(7, 300, seed=1)
    assert c.shape == (7, 300) and c.min() == -1 and c.max() == 2
    assert abs((c < 0).mean() - S.MISSING_RATE) < 0.05


def test_new_entry_points_declared_bound_and_exported():
    import bann._lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bann.h")).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for f in NEW_FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % f, header), f
        assert f in L.SIGNATURES and hasattr(lib, f) and f in exported, f
    from bann import BannContext, io
    for name in ("subset", "subset_timing", "fill_missing_a2"):
        assert callable(getattr(BannContext, name)), name
    for name in ("read_fam", "split_indices", "kfold_indices", "split_train_test", "fill_missing_a2"):
        assert callable(getattr(io, name)), name


def test_strip_constants():
    """the strip width the GPU tests take from the source: 256 lanes of one destination dword each"""
    text = open(os.path.join(CSRC, "bann_internal.h")).read()
    fpl = int(re.search(r"#define SUBSET_FPL (\d+)", text).group(1))
    strip = int(re.search(r"#define SUBSET_STRIP (\d+)", text).group(1))
    assert fpl == 16 and strip == 256 * fpl


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_subset_kernels_do_not_spill(tmp_path):
    """every kernel of kernels_subset.hip for gfx950, the product's flags: no VGPR or SGPR spill, no scratch"""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-c",
                          os.path.join(CSRC, "kernels_subset.hip"), "-o", str(tmp_path / "k.o"),
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
    for k in NEW_KERNELS:
        assert sum(k in fn for fn in res) == 1, (k, sorted(res))
    for fn, v in res.items():
        assert v == {"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize": 0}, (fn, v)
