"""numpy restatement of the linear-model simulator (include/bann.h "linear scores ..."), written from
its formulas: the inclusion keys and masks, the effect draws, the f64 score and the .bed codes.  The
Philox words come from init_reference.philox4x32; statistics.NormalDist().inv_cdf is AS 241, the
routine the device uses.  The tests compare the device against it."""
from statistics import NormalDist

import numpy as np

from init_reference import philox4x32

STREAM_NOISE = 0xB300000000000000
STREAM_EFFECT = 0xB400000000000000
STREAM_INCLUDE = 0xB500000000000000
_INV = NormalDist().inv_cdf
# at p = 0.25 this seed keeps at least one entry for E in {1, 255, 257, 70001} (test_linear_cpu checks it)
P_SEED = 11


def include_keys(seed, E):
    """key_t of entry t of the concatenated entry list: word 0 of stream (seed, INCLUDE) at counter t"""
    return philox4x32(np.arange(E, dtype=np.uint64), STREAM_INCLUDE, seed)[0]


def keep_mask(seed, E, num_effective=None, proportion_effective=None):
    """num_effective = e: t is kept iff fewer than e entries precede it in the order of (key, index);
    else proportion p: iff u01(key) < p, u01(x) = f32(x >> 8) * 2^-24; neither: every entry"""
    if num_effective is not None:
        key = include_keys(seed, E)
        order = np.lexsort((np.arange(E), key))      # by key, ties by index
        rank = np.empty(E, np.int64)
        rank[order] = np.arange(E)
        return rank < num_effective
    if proportion_effective is not None:
        key = include_keys(seed, E)
        u = (key >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
        return u < np.float32(proportion_effective)
    return np.ones(E, bool)


def normals(seed, stream, count):
    """standard normal numbers 0 .. count of a stream, f64: word idx % 4 of the block at counter
    idx / 4, u = (word + 0.5) / 2^32, z = the inverse distribution function of u"""
    blocks = philox4x32(np.arange((count + 3) // 4, dtype=np.uint64), stream, seed)
    words = np.stack(blocks, axis=1).reshape(-1)[:count]
    u = (words.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
    return np.array([_INV(float(v)) for v in u], np.float64)


def effects(seed, E, heritability, num_effective=None, proportion_effective=None):
    """(effects f32 [E], m_incl): sd = sqrt(h / m_incl) in f32, a kept entry sd * f32(z_t), others 0"""
    mask = keep_mask(seed, E, num_effective, proportion_effective)
    m_incl = int(mask.sum())
    if m_incl == 0:
        raise ValueError("no effective marker")
    sd = np.sqrt(np.float32(heritability) / np.float32(m_incl)).astype(np.float32)
    z = normals(seed, STREAM_EFFECT, E).astype(np.float32)
    return np.where(mask, sd * z, np.float32(0.0)).astype(np.float32), m_incl


def standardize(g, mu, sd):
    """x_std [n][M] f64 from int8 g [M][n]: (g - mu) / sigma, 0 where sigma = 0"""
    mu64, sd64 = np.asarray(mu, np.float64), np.asarray(sd, np.float64)
    safe = np.where(sd64 > 0, sd64, 1.0)
    x = (np.asarray(g, np.float64).T - mu64) / safe
    x[:, sd64 <= 0] = 0.0
    return x


def score(x_std, groups, eff):
    """f64 [K][n]: sum over the entries t of eff[k][t] x_std[:, marker_t]"""
    mk = np.concatenate([np.asarray(g, np.int64) for g in groups])
    e = np.atleast_2d(np.asarray(eff, np.float64))
    return e @ x_std[:, mk].T


def bed_file_bytes(g):
    """the .bed file of int8 [M][n] genotypes in {0, 1, 2}, -1 missing: signature and payload"""
    from bann.io import encode_bed_payload
    return b"\x6c\x1b\x01" + encode_bed_payload(g)


def linear_model_line(groups, eff):
    """the LinearModel as serde_json writes it (linear_model.rs:102-107) plus the newline"""
    from bann.io import format_f32

    def num(v):
        t = format_f32(v)
        return t if "." in t or "e" in t else t + ".0"
    sizes = [len(g) for g in groups]
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows = ["[" + ",".join(num(v) for v in eff[off[b]:off[b + 1]]) + "]" for b in range(len(sizes))]
    return ('{"num_branches":%d,"num_markers_per_branch":[%s],"effects":[%s]}\n'
            % (len(sizes), ",".join(str(s) for s in sizes), ",".join(rows)))
