"""The oracle of the cohort subset for the tests, in numpy: a cohort is int8 [M][n] with -1 for a
missing call, and its subset is plain fancy indexing.  Also the seeded cohorts of the GPU tests and a
.bed decoder written from the format, not from the library."""
from __future__ import annotations

import numpy as np

MISSING_RATE = 0.15


def subset(g, individuals=None, markers=None) -> np.ndarray:
    """g[np.ix_(markers, individuals)]; None stands for all, in order.  Lists may repeat and reorder."""
    g = np.asarray(g)
    mk = np.arange(g.shape[0]) if markers is None else np.asarray(markers, dtype=np.int64)
    ind = np.arange(g.shape[1]) if individuals is None else np.asarray(individuals, dtype=np.int64)
    return g[np.ix_(mk, ind)]


def cohort(M: int, n: int, seed: int, missing: float = MISSING_RATE) -> np.ndarray:
    """int8 [M][n]: allele counts of a per-marker frequency in (0.05, 0.5), `missing` of the calls -1"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    g = rng.binomial(2, p, size=(M, n)).astype(np.int8)
    g[rng.random((M, n)) < missing] = -1
    return g


def zero_coded(g) -> np.ndarray:
    """what the genotype image holds: a missing call as 0"""
    g = np.asarray(g)
    return np.where(g < 0, 0, g).astype(np.int8)


def decode_bed(data: bytes, n: int, M: int) -> np.ndarray:
    """int8 [M][n] of a variant-major .bed (signature allowed): 00 -> 2, 10 -> 1, 11 -> 0, 01 -> -1"""
    if data[:3] == b"\x6c\x1b\x01" and len(data) == 3 + (n + 3) // 4 * M:
        data = data[3:]
    raw = np.frombuffer(data, np.uint8).reshape(M, (n + 3) // 4)
    fields = np.stack([(raw >> (2 * p)) & 3 for p in range(4)], axis=2).reshape(M, -1)[:, :n]
    return np.array([2, -1, 1, 0], np.int8)[fields]
