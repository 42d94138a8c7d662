"""CPU-side checks of the pairwise-complete LD: tests/ld_pairwise_reference.py against numpy's own
correlation and against tests/ld_reference.py, the test cohorts (so that the GPU comparisons are not
ones of zeros), the .bed encoder, the new symbols, and the resource report of kernels_ld.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bann_oracle as O
import ld_pairwise_reference as P
import ld_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW_CTX = ["bann_genotypes_keep_missing", "bann_genotypes_missing_counts", "bann_genotypes_ld_band_pairwise",
           "bann_genotypes_ld_graph_pairwise"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_reference_against_numpy_corrcoef():
    """50 edge pairs of `blocks`: r2 equals np.corrcoef squared over the jointly present individuals"""
    gm = P.cohort("blocks")
    r2 = P.r2_matrix(gm)
    pairs = sorted(P.edges(gm, 137, 0.5))
    pick = np.random.default_rng(3).choice(len(pairs), 50, replace=False)
    worst = 0.0
    for j, k in (pairs[i] for i in pick):
        both = (gm[j] >= 0) & (gm[k] >= 0)
        c = np.corrcoef(gm[j, both].astype(np.float64), gm[k, both].astype(np.float64))[0, 1]
        worst = max(worst, abs(c * c - r2[j, k]))
    print("largest |corrcoef^2 - r2| over 50 pairs:", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("name,window", [("blocks", 137), ("deep", 69), ("groups", 40)])
def test_reference_without_missing_calls_is_the_plain_one(name, window):
    g = P.complete(name)
    assert np.array_equal(P.r2_matrix(g), R.r2_matrix(g))
    assert np.array_equal(bits(P.band(g, window)), bits(R.band(g, window)))
    assert P.edges(g, window, 0.5) == R.edges(g, window, 0.5)
    inside = np.add.outer(np.arange(g.shape[0]), np.arange(1, window + 1)) < g.shape[0]
    assert np.array_equal(P.npairs(g, window), np.where(inside, g.shape[1], 0))


def test_cohorts_keep_pairwise_and_zero_coded_apart():
    """a pass on the GPU cannot come from comparing zeros, or from a pairwise band that is the plain one"""
    gm = P.cohort("blocks")
    z = P.zero_coded(gm)
    pw, zc = P.edges(gm, 137, 0.5), R.edges(z, 137, 0.5)
    differ = int((bits(P.ref_band("blocks", 137)) != bits(R.band(z, 137))).sum())
    print("blocks: pairwise edges", len(pw), "zero-coded edges", len(zc), "band entries that differ", differ)
    assert len(pw) >= 1000 and len(zc) <= 100 and differ >= 10000
    gm = P.cohort("deep")
    pw, zc = P.edges(gm, 69, 0.5), R.edges(P.zero_coded(gm), 69, 0.5)
    print("deep: pairwise edges", len(pw), "zero-coded edges", len(zc))
    assert len(pw) >= 200 and len(zc) == 0


def test_deep_cohort_has_the_pair_constant_case():
    """marker 40 varies over the cohort (v > 0 with 42), but is constant where 41 is present"""
    gm = P.cohort("deep")
    N, a, b, qa, qb, S = P.sums(gm)
    va = N * qa - a * a
    r2 = P.r2_matrix(gm)
    assert va[40, 41] == 0 and r2[40, 41] == 0.0 and N[40, 41] > 0
    assert va[40, 42] > 0 and r2[40, 42] > 0.0
    assert np.all(r2[17] == 0) and np.all(r2[:, 17] == 0) and np.all(N[17] == 0)
    assert np.all(r2[30] == 0)


@pytest.mark.parametrize("n", [1, 4, 5, 193])
def test_encode_bed_payload_round_trip(n):
    from bann.io import encode_bed_payload
    rng = np.random.default_rng(100 + n)
    M = 7
    gm = rng.integers(-1, 3, size=(M, n)).astype(np.int8)
    gm[0, 0] = -1
    payload = encode_bed_payload(gm)
    assert isinstance(payload, bytes) and len(payload) == M * ((n + 3) // 4)
    assert payload == P.encode_bed(gm)
    assert np.array_equal(O.bed_decode(payload, n, M), P.zero_coded(gm))   # the missing positions come back as 0
    assert np.array_equal(P.decode_bed(payload, n, M), gm)
    if n % 4:  # padding bits are 0
        last = np.frombuffer(payload, np.uint8).reshape(M, -1)[:, -1]
        assert np.all(last >> (2 * (n % 4)) == 0)
    with pytest.raises(ValueError):
        encode_bed_payload(np.full((2, 3), 3, np.int8))


def test_new_symbols_in_header_library_and_binding():
    import bann._lib as L
    import bann.io as IO
    from bann import BannContext
    hdr = open(os.path.join(ROOT, "include", "bann.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "rs-bann_amd", "librsbann_amd.so"))
    for f in NEW_CTX:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
        assert f in L.SIGNATURES, f
        assert hasattr(lib, f), f
    for name in ("keep_missing", "missing_counts"):
        assert callable(getattr(BannContext, name))
    assert callable(IO.encode_bed_payload)
    with pytest.raises(ValueError):
        IO.group_by_ld(None, 5, 0.5, 1, missing="drop")


def test_pairwise_ld_kernels_do_not_spill(tmp_path):
    """kernels_ld.hip for gfx950 with the product's flags: the five band instantiations, k_ld_r2_pw and
    k_ld_mask_pw are there, and each reports no VGPR or SGPR spill and no scratch"""
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
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    band = sorted(f for f in res if "k_ld_band_pw" in f)
    assert len(band) == 5, band
    # <row side, column side>: 0 genotype, 1 presence, 2 genotype squared
    for ra, rb in ((1, 1), (0, 1), (1, 0), (2, 1), (1, 2)):
        assert any("ILi%dELi%dEE" % (ra, rb) in f for f in band), (ra, rb, band)
    new = band + [f for f in res if "k_ld_r2_pw" in f or "k_ld_mask_pw" in f]
    assert len(new) == 7, new
    for f in new:
        v = dict(res[f])
        occ = v.pop("Occupancy")
        assert v == {"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize": 0}, (f, v)
        if f in band:
            assert occ == 2, (f, occ)
    k = [f for f in res if "k_ld_band" in f and "_pw" not in f]
    assert len(k) == 1 and res[k[0]]["Occupancy"] == 2, k
