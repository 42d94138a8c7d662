"""numpy restatement of the model initialisation (include/bann.h "starting a model"), written from
its formulas: Philox4x32-10 in integer arithmetic, the marker keep masks, the maximum-likelihood
precisions in f64 and the width rules.  The tests compare the device against it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_SELECT = 0xB200000000000000
ARD = ("ridge_ard", "lasso_ard")
LASSO = ("lasso_ard", "lasso_base")


def philox4x32(counter, stream, seed):
    """the four 32-bit words of Philox4x32-10 at counters `counter` (uint64 array) of (seed, stream):
    counter words (counter lo, counter hi, stream lo, stream hi), key words (seed lo, seed hi)"""
    c = np.asarray(counter, dtype=np.uint64)
    x, y = c & MASK, c >> np.uint64(32)
    z = np.full_like(x, stream & MASK)
    w = np.full_like(x, stream >> 32)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * x          # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * z
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        x, y, z, w = hi1 ^ y ^ np.uint64(k0), lo1, hi0 ^ w ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return x, y, z, w


def select_keys(seed, branch, m):
    """key_j of marker j of a branch: word 0 of stream (seed, branch, SELECT) at counter j"""
    return philox4x32(np.arange(m, dtype=np.uint64), STREAM_SELECT | branch, seed)[0]


def keep_mask_exact(seed, branch, m, e):
    """exactly e markers: j is kept iff the rank of (key_j, j) is below e"""
    key = select_keys(seed, branch, m)
    order = np.lexsort((np.arange(m), key))      # by key, ties by index
    rank = np.empty(m, np.int64)
    rank[order] = np.arange(m)
    return rank < e


def keep_mask_proportion(seed, branch, m, p):
    """j is kept iff u01(key_j) < p, u01(x) = f32(x >> 8) * 2^-24"""
    key = select_keys(seed, branch, m)
    u = (key >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u < np.float32(p)


def split_params(theta, m, widths):
    """param_vec -> (weights [in x out, element (j, k) at k * in + j -> array [out][in]], biases)"""
    ws, bs, o, win = [], [], 0, m
    for wo in widths:
        ws.append(np.asarray(theta[o:o + win * wo]).reshape(wo, win))
        o += win * wo
        win = wo
    for wo in widths[:-1]:
        bs.append(np.asarray(theta[o:o + wo]))
        o += wo
    assert o == len(theta)
    return ws, bs


def _ratio(num, s):
    return np.inf if s == 0.0 else num / s


def precisions(theta, m, widths, prior, fixed=None):
    """precision_vec of the initial BranchCfg at parameters theta, in f64: +inf where a sum is zero"""
    ws, bs = split_params(np.asarray(theta, np.float64), m, widths)
    L = len(widths)
    out = []
    for l, w in enumerate(ws):
        if prior in ARD and l < L - 1:
            out += [_ratio(float(widths[l]), float(np.sum(w[:, j] ** 2))) for j in range(w.shape[1])]
        elif prior in ARD:
            out.append(1.0)
        else:
            out.append(_ratio(float(w.size), float(np.sum(w ** 2))))
    out += [_ratio(float(widths[l]), float(np.sum(bs[l] ** 2))) for l in range(L - 1)]
    out.append(2.0)
    v = np.array(out, np.float64)
    return np.full_like(v, fixed) if fixed is not None else v


def output_weights(theta, m, widths):
    return split_params(np.asarray(theta, np.float64), m, widths)[0][-1].ravel()


def joint_output_precision(thetas, ms, widths_list):
    """nb / sum_b sum w_out,b^2"""
    return len(thetas) / sum(float(np.sum(output_weights(t, m, w) ** 2)) for t, m, w in zip(thetas, ms, widths_list))


def reg_sum(thetas, ms, widths_list, prior):
    f = np.abs if prior in LASSO else np.square
    return sum(float(np.sum(f(output_weights(t, m, w)))) for t, m, w in zip(thetas, ms, widths_list))


def out_precision_index(m, widths, prior):
    """index of the output-layer entry in precision_vec"""
    ins = [m] + list(widths[:-2])
    return sum(ins) if prior in ARD else len(widths) - 1


def layer_widths(m, depth, hidden=("fraction", 0.5), summary=("like_hidden",)):
    """the width rules: f32 products truncated toward zero, at least 1"""
    def frac(a, f):
        return max(1, int(np.float32(a) * np.float32(f)))
    h = int(hidden[1]) if hidden[0] == "fixed" else frac(m, hidden[1])
    if summary[0] == "fixed":
        s = int(summary[1])
    elif summary[0] == "like_hidden":
        s = h
    else:
        s = frac(h, summary[1])
    return [h] * depth + [s, 1]


def num_params(m, widths):
    ins = [m] + list(widths[:-1])
    return sum(i * o for i, o in zip(ins, widths)) + sum(widths[:-1])
