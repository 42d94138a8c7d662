"""Independent restatement of the pairwise-complete LD band for the tests: numpy int64 arithmetic,
written from include/bann.h's definition (six matrix products and one f64 division), not from the
library's C++.  A cohort here is int8 [M][n] with -1 for a missing call.  Also the test cohorts with
their missing calls, and a .bed encoder and decoder of this module's own (not the library's)."""
from __future__ import annotations

import functools
import os

import numpy as np

import ld_reference as R

PLINK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plink")


# ------------------------------------------------------------------ .bed codes
def encode_bed(gm: np.ndarray) -> bytes:
    """variant-major payload: 2 -> 00, 1 -> 10, 0 -> 11, -1 -> 01, individual 4q+p in bits 2p of byte q,
    padding bits 0"""
    M, n = gm.shape
    out = np.zeros((M, (n + 3) // 4), np.uint8)
    code_of = {2: 0, 1: 2, 0: 3, -1: 1}
    for j in range(M):
        for i in range(n):
            out[j, i >> 2] |= code_of[int(gm[j, i])] << (2 * (i & 3))
    return out.tobytes()


def decode_bed(payload: bytes, n: int, M: int) -> np.ndarray:
    """the inverse, -1 for the code 01"""
    bpc = (n + 3) // 4
    raw = np.frombuffer(payload, np.uint8)[:bpc * M].reshape(M, bpc)
    value_of = np.array([2, -1, 1, 0], np.int8)
    out = np.zeros((M, n), np.int8)
    for i in range(n):
        out[:, i] = value_of[(raw[:, i >> 2] >> (2 * (i & 3))) & 3]
    return out


def zero_coded(gm: np.ndarray) -> np.ndarray:
    """what the genotype image holds: a missing call as 0"""
    return np.where(gm < 0, 0, gm).astype(np.int8)


# ------------------------------------------------------------------ the definition
def sums(gm: np.ndarray):
    """(N, a, b, qa, qb, S), each (M, M) int64, entry [j][k] for the pair (j, k)"""
    m = (np.asarray(gm) >= 0).astype(np.int64)
    g = np.where(np.asarray(gm) < 0, 0, gm).astype(np.int64)
    g2 = g * g
    return m @ m.T, g @ m.T, m @ g.T, g2 @ m.T, m @ g2.T, g @ g.T


def r2_matrix(gm: np.ndarray) -> np.ndarray:
    """(M, M) float64: cov = N S - a b, v_a = N qa - a^2, v_b = N qb - b^2 in int64,
    r2 = (f64(cov) * f64(cov)) / (f64(v_a) * f64(v_b)), 0 where v_a == 0 or v_b == 0"""
    N, a, b, qa, qb, S = sums(gm)
    cov = N * S - a * b
    va = N * qa - a * a
    vb = N * qb - b * b
    cf = cov.astype(np.float64)
    num = cf * cf
    den = va.astype(np.float64) * vb.astype(np.float64)
    ok = (va != 0) & (vb != 0)
    out = np.zeros(N.shape, np.float64)
    out[ok] = num[ok] / den[ok]
    return out


def _band_of(mat: np.ndarray, window: int, dtype) -> np.ndarray:
    M = mat.shape[0]
    out = np.zeros((M, window), dtype)
    for d in range(1, min(window, M - 1) + 1):
        out[:M - d, d - 1] = np.diagonal(mat, d).astype(dtype)
    return out


def band(gm: np.ndarray, window: int) -> np.ndarray:
    """(M, window) float32: [j][d - 1] = f32(r2(j, j + d)), 0 where j + d >= M"""
    return _band_of(r2_matrix(gm), window, np.float32)


def npairs(gm: np.ndarray, window: int) -> np.ndarray:
    """(M, window) int32: [j][d - 1] = N(j, j + d), 0 where j + d >= M"""
    return _band_of(sums(gm)[0], window, np.int32)


def edges(gm: np.ndarray, window: int, r2_min, chrom=None, bp=None, max_bp: int = 0):
    """set of (j, k), j < k <= j + window, r2 >= f64(f32(r2_min)) on the f64 value, and the chrom / bp filter"""
    r2 = r2_matrix(gm)
    thr = float(np.float32(r2_min))
    M = r2.shape[0]
    out = set()
    for j in range(M):
        for k in range(j + 1, min(M, j + window + 1)):
            if not r2[j, k] >= thr:
                continue
            if chrom is not None:
                if chrom[j] != chrom[k] or (max_bp > 0 and abs(int(bp[j]) - int(bp[k])) > max_bp):
                    continue
            out.add((j, k))
    return out


# ------------------------------------------------------------------ the cohorts
def _with_missing(g: np.ndarray, miss: np.ndarray) -> np.ndarray:
    gm = g.astype(np.int8).copy()
    gm[miss] = -1
    gm.setflags(write=False)
    return gm


@functools.lru_cache(maxsize=None)
def complete(name: str) -> np.ndarray:
    """the cohorts of test_ld_gpu.py without a missing call, [M][n] int8"""
    if name == "blocks":  # n = 3 * 64 + 1; 300 markers
        return R.ld_block_cohort(np.random.default_rng(5), 193, 27, 10, 30)
    if name == "deep":    # n = 4099: many K stages, the K split is active; 70 markers
        g = R.ld_block_cohort(np.random.default_rng(6), 4099, 7, 9, 7)
        g[30, :] = 2      # zero variance
        g[40, :] = 0      # varies over the cohort, but only among individuals 0..9
        g[40, :10] = 1
        return g
    if name == "groups":  # 57 markers x 257 individuals
        return R.ld_block_cohort(np.random.default_rng(7), 257, 6, 9, 3)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cohort(name: str) -> np.ndarray:
    """the test cohorts with their missing calls, [M][n] int8 with -1 = missing, built once, read-only"""
    if name in ("small", "random"):  # the PLINK fixtures, with whatever missing codes they hold
        n, M = {"small": (20, 11), "random": (100, 20)}[name]
        gm = decode_bed(open(os.path.join(PLINK, name + ".bed"), "rb").read()[3:], n, M)
        gm.setflags(write=False)
        return gm
    if name in ("blocks", "blocks_dups"):
        g = complete("blocks").copy()
        miss = np.random.default_rng(11).random(g.shape) < 0.15
        miss[17, :] = True   # a marker without any call: its row and column are r2 0, N 0
        miss[:, 5] = True    # an individual without any call
        # the last individual sits alone in the last byte, next to three padding codes
        miss[:, 192] = np.random.default_rng(13).random(g.shape[0]) < 0.5
        if name == "blocks_dups":  # three exact duplicates whose missing patterns differ
            g[205] = g[203]
            g[206] = g[203]
        return _with_missing(g, miss)
    if name == "deep":
        g = complete("deep")
        miss = np.random.default_rng(11).random(g.shape) < 0.15
        miss[17, :] = True
        miss[:, 5] = True
        miss[40, :] = False   # fully present
        miss[41, :10] = True  # so marker 40 is constant among the pair (40, 41)'s present individuals
        return _with_missing(g, miss)
    if name == "groups":
        g = complete("groups")
        return _with_missing(g, np.random.default_rng(12).random(g.shape) < 0.15)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref_band(name: str, window: int) -> np.ndarray:
    b = band(cohort(name), window)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def ref_npairs(name: str, window: int) -> np.ndarray:
    b = npairs(cohort(name), window)
    b.setflags(write=False)
    return b
