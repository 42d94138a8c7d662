"""Independent restatement of the LD band, the LD graph and the centered grouping for the tests:
numpy int64 arithmetic and Python sets, written from include/bann.h's definition of r2 and from the
reference's group/centered.rs (CorrGraph::from_plink_ld 54-89, centered_grouping 91-133), not from
the library's C++."""
from __future__ import annotations

import numpy as np


def r2_matrix(g: np.ndarray) -> np.ndarray:
    """g: [M][n] genotypes in {0,1,2}.  (M, M) float64 r2 by the integer definition:
    cov = n S_jk - s_j s_k, v_j = n q_j - s_j^2 in int64, r2 = (f64(cov) * f64(cov)) / (f64(v_j) * f64(v_k)),
    0 where v_j == 0 or v_k == 0."""
    x = np.asarray(g).astype(np.int64)
    n = np.int64(x.shape[1])
    s = x.sum(axis=1)
    q = (x * x).sum(axis=1)
    S = x @ x.T
    cov = n * S - np.outer(s, s)
    v = n * q - s * s
    cf = cov.astype(np.float64)
    vf = v.astype(np.float64)
    num = cf * cf
    den = np.outer(vf, vf)
    ok = np.outer(v != 0, v != 0)
    out = np.zeros(S.shape, np.float64)
    out[ok] = num[ok] / den[ok]
    return out


def band(g: np.ndarray, window: int) -> np.ndarray:
    """(M, window) float32: [j][d - 1] = f32(r2(j, j + d)), 0 where j + d >= M"""
    r2 = r2_matrix(g)
    M = r2.shape[0]
    out = np.zeros((M, window), np.float32)
    for d in range(1, min(window, M - 1) + 1):
        out[:M - d, d - 1] = np.diagonal(r2, d).astype(np.float32)
    return out


def edges(g: np.ndarray, window: int, r2_min, chrom=None, bp=None, max_bp: int = 0):
    """set of (j, k), j < k <= j + window, r2 >= f64(f32(r2_min)) on the f64 value, and the chrom / bp filter"""
    r2 = r2_matrix(g)
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


def adjacency(num_markers: int, edge_set):
    adj = {j: set() for j in range(num_markers)}
    for j, k in edge_set:
        adj[j].add(k)
        adj[k].add(j)
    return adj


def csr(adj):
    M = len(adj)
    off = np.zeros(M + 1, np.int64)
    nb = []
    for j in range(M):
        nb.extend(sorted(adj[j]))
        off[j + 1] = len(nb)
    return off, np.asarray(nb, dtype=np.int32)


def csr_edges(off, nb):
    """the (j, k), j < k set of a symmetric CSR; asserts symmetry and ascending lists"""
    out, directed = set(), set()
    for j in range(len(off) - 1):
        lst = [int(k) for k in nb[off[j]:off[j + 1]]]
        assert lst == sorted(set(lst)), (j, lst)
        for k in lst:
            directed.add((j, k))
            if j < k:
                out.add((j, k))
    assert all((k, j) in directed for j, k in directed)
    return out


def centered(adj, min_group_size: int):
    """centered.rs:91-133.  Returns (groups as sorted lists, number of nodes left in no group)."""
    order = sorted(adj, key=lambda k: (-len(adj[k]), k))
    groups = {}
    no_centers = set()
    gix = 0
    ungrouped = 0
    for cix in order:
        if cix in no_centers:
            continue
        nbrs = adj[cix]
        if len(nbrs) > 0 and len(nbrs) > min_group_size:
            group = list(nbrs) + [cix]
            no_centers.update(group)
            groups[gix] = group
            gix += 1
        else:
            placed = False
            for d in range(1, 100):
                # usize arithmetic of the release build: cix - d wraps to a huge key, which is absent
                if cix - d >= 0 and (cix - d) in groups:
                    groups[cix - d].append(cix)
                    placed = True
                    break
                if (cix + d) in groups:
                    groups[cix + d].append(cix)
                    placed = True
                    break
            if not placed:
                ungrouped += 1
    return [sorted(groups[k]) for k in range(gix)], ungrouped


def ld_block_cohort(rng, n: int, num_blocks: int, block_size: int, singletons: int, flip: float = 0.10):
    """[M][n] int8: blocks of block_size markers that copy a Binomial(2, p) base column, p ~ U(0.2, 0.5),
    each copy with a `flip` share of the individuals redrawn; one singleton between blocks while they last"""
    cols = []
    left = singletons
    for _ in range(num_blocks):
        p = rng.uniform(0.2, 0.5)
        base = rng.binomial(2, p, size=n)
        for _ in range(block_size):
            c = base.copy()
            redo = rng.random(n) < flip
            c[redo] = rng.binomial(2, p, size=int(redo.sum()))
            cols.append(c)
        if left > 0:
            cols.append(rng.binomial(2, rng.uniform(0.2, 0.5), size=n))
            left -= 1
    for _ in range(left):
        cols.append(rng.binomial(2, rng.uniform(0.2, 0.5), size=n))
    return np.asarray(cols, dtype=np.int8)
