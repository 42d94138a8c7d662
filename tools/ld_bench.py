#!/usr/bin/env python3
"""The LD band at scale (kernels_ld.hip): a synthetic cohort on the device (bann_genotypes_synthetic),
n = 50 000, M = 100 000, windows 500 and 100.  Per window one warm-up call, then --reps calls of

  band   BannContext.ld_band over all markers (the f32 band comes back to the host: M x window floats)
  graph  BannContext.ld_graph at r2_min 0.2 (only the per-marker bit masks come back)

with the HIP-event time of the device kernels (ld_timing) and the host-clock time of every call, and
MAC/s = n M window / t against the dense int8 MFMA peak.  One JSON line per window.

  --host-markers H   the comparison arm, for scale only: the same band for the first H markers with
                     numpy int64 on the host (at most 16 threads), checked bit for bit against the
                     device band and EXTRAPOLATED linearly in M to the full cohort
  --host-only        the comparison arm alone on a numpy cohort of the same shape (needs no device)
  --pairwise RATE    the pairwise-complete band against the plain one on one context: a numpy cohort
                     with every call missing independently at RATE, encoded to a .bed payload and
                     loaded with keep_missing + upload_bed; per window one warm-up call, then --reps
                     calls of ld_band and of ld_band(pairwise=True).  The M marker rows are drawn with
                     replacement from --pool distinct random markers (drawing 5e9 calls one by one
                     would take minutes; the kernels' time does not depend on the values).  --out FILE
                     also writes the records as one JSON document.

  python tools/ld_bench.py [--n 50000] [--markers 100000] [--windows 500,100] [--reps 3] [--host-markers 0]
  python tools/ld_bench.py --pairwise 0.02 [--pool 4096] [--out profiles/ld_pairwise.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-bann_amd"))

# MI355X: BF16 ~2.5 PF dense, and "I8: 32x32x32 / 16x16x64: the cycles of the BF16 form of the same
# MxN at 2x the K, so 2x BF16 per clock": ~5e15 int8 op/s = 2.5e15 MAC/s
I8_PEAK_MACS = 2.5e15


def host_band(g, window, threads=min(16, os.cpu_count() or 1)):
    """numpy int64 restatement of the band of every row of g that has its whole window inside g
    (the definition of include/bann.h), in row blocks over a thread pool"""
    x = g.astype(np.int64)
    M, n = x.shape
    s = x.sum(axis=1)
    q = (x * x).sum(axis=1)
    v = n * q - s * s
    rows = M - window
    out = np.zeros((rows, window), np.float32)

    def block(r0):
        r1 = min(rows, r0 + 128)
        S = x[r0:r1] @ x[r0:r1 + window].T
        for j in range(r0, r1):
            k = np.arange(j + 1, j + window + 1)
            cov = (n * S[j - r0, k - r0] - s[j] * s[k]).astype(np.float64)
            den = np.float64(v[j]) * v[k].astype(np.float64)
            ok = (v[j] != 0) & (v[k] != 0)
            out[j, ok] = ((cov[ok] * cov[ok]) / den[ok]).astype(np.float32)

    with ThreadPoolExecutor(max_workers=min(threads, 16)) as ex:
        list(ex.map(block, range(0, rows, 128)))
    return out


def spread(ts):
    return {"best": round(min(ts), 3), "all": [round(t, 3) for t in ts],
            "spread_pct": round(100.0 * (max(ts) - min(ts)) / min(ts), 2)}


def pairwise_arm(args, n, M, windows):
    from bann import BannContext
    from bann.io import encode_bed_payload
    rng = np.random.default_rng(1000003)
    P = min(args.pool, M)
    bpc = (n + 3) // 4
    pool = np.zeros((P, bpc), np.uint8)
    missing = 0
    for p0 in range(0, P, 256):
        m = min(256, P - p0)
        g = rng.binomial(2, rng.uniform(0.01, 0.5, size=(m, 1)), size=(m, n)).astype(np.int8)
        miss = rng.random((m, n)) < args.pairwise
        g[miss] = -1
        missing += int(miss.sum())
        pool[p0:p0 + m] = np.frombuffer(encode_bed_payload(g), np.uint8).reshape(m, bpc)
    pick = rng.integers(0, P, size=M)
    payload = pool[pick]
    ctx = BannContext(0)
    ctx.keep_missing()
    ctx.upload_bed(payload.tobytes(), n, M)
    del payload
    counts = ctx.missing_counts()
    lib, h = ctx._lib, ctx._h

    def timed(f, *a, **kw):
        lib.bann_synchronize(h)
        t0 = time.perf_counter()
        r = f(*a, **kw)
        lib.bann_synchronize(h)
        return (time.perf_counter() - t0) * 1e3, ctx.ld_timing(), r

    recs = []
    for w in windows:
        arms = {}
        for name, kw in (("plain", {}), ("pairwise", {"pairwise": True})):
            timed(ctx.ld_band, w, **kw)  # warm-up
            host, kern = [], []
            for _ in range(args.reps):
                t, k, band = timed(ctx.ld_band, w, **kw)
                host.append(t)
                kern.append(k)
                del band
            arms[name] = (kern, host)
        rec = {"arm": "pairwise against plain ld_band", "n": n, "markers": M, "window": w,
               "missing_rate": args.pairwise, "pool_markers": P, "missing_calls": int(counts.sum()),
               "plain_kernel_ms": spread(arms["plain"][0]), "plain_host_ms": spread(arms["plain"][1]),
               "pairwise_kernel_ms": spread(arms["pairwise"][0]), "pairwise_host_ms": spread(arms["pairwise"][1]),
               "kernel_ratio_best": round(min(arms["pairwise"][0]) / min(arms["plain"][0]), 3),
               "image_bytes": int((n + 63) // 64 * 16) * M}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/ld_bench.py --pairwise", "records": recs}, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--windows", default="500,100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-markers", type=int, default=0)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--pairwise", type=float, default=None, metavar="RATE")
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, M = args.n, args.markers
    windows = [int(w) for w in args.windows.split(",")]
    if args.pairwise is not None:
        pairwise_arm(args, n, M, windows)
        return
    if args.host_only:
        rng = np.random.default_rng(1000003)
        for w in windows:
            H = args.host_markers or 2000
            g = rng.binomial(2, rng.uniform(0.01, 0.5, size=(H + w, 1)), size=(H + w, n)).astype(np.int8)
            t0 = time.perf_counter()
            host_band(g, w)
            t = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"arm": "host numpy int64", "n": n, "window": w, "host_markers": H,
                              "threads": min(16, os.cpu_count() or 1), "host_ms": round(t, 1),
                              "extrapolated_to_markers": M, "extrapolated_ms": round(t * M / H, 1),
                              "note": "linear extrapolation in M of the first host_markers markers"}), flush=True)
        return
    from bann import BannContext
    ctx = BannContext(0)
    ctx.synthetic_genotypes(n, M, seed=1000003)
    lib, h = ctx._lib, ctx._h

    def timed(f, *a):
        lib.bann_synchronize(h)
        t0 = time.perf_counter()
        r = f(*a)
        lib.bann_synchronize(h)
        return (time.perf_counter() - t0) * 1e3, ctx.ld_timing(), r

    for w in windows:
        macs = float(n) * M * w
        timed(ctx.ld_band, w)  # warm-up
        band_host, band_kern = [], []
        for _ in range(args.reps):
            t, k, band = timed(ctx.ld_band, w)
            band_host.append(t)
            band_kern.append(k)
        timed(ctx.ld_graph, w, 0.2)
        graph_host, graph_kern = [], []
        for _ in range(args.reps):
            t, k, (off, nb) = timed(ctx.ld_graph, w, 0.2)
            graph_host.append(t)
            graph_kern.append(k)
        rec = {"n": n, "markers": M, "window": w, "macs_band": macs,
               "band_kernel_ms": spread(band_kern), "band_host_ms": spread(band_host),
               "graph_kernel_ms": spread(graph_kern), "graph_host_ms": spread(graph_host),
               "graph_edges_at_0.2": int(nb.size // 2),
               "band_kernel_mac_per_s": round(macs / (min(band_kern) * 1e-3), 1),
               "graph_kernel_mac_per_s": round(macs / (min(graph_kern) * 1e-3), 1),
               "i8_mfma_peak_mac_per_s": I8_PEAK_MACS,
               "band_kernel_share_of_i8_peak": round(macs / (min(band_kern) * 1e-3) / I8_PEAK_MACS, 4),
               "image_bytes": int((n + 63) // 64 * 16) * M}
        if args.host_markers > 0:
            H = args.host_markers
            g = ctx.download_genotypes(np.arange(H + w))
            t0 = time.perf_counter()
            hb = host_band(g, w)
            th = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(hb.view(np.uint32), band[:H].view(np.uint32)), "host and device bands differ"
            rec.update({"host_markers": H, "host_threads": min(16, os.cpu_count() or 1),
                        "host_numpy_ms": round(th, 1), "host_numpy_extrapolated_ms": round(th * M / H, 1),
                        "host_note": "numpy int64 on the host; extrapolated_ms is a linear extrapolation in M, "
                                     "not a measurement; the H rows are bit-equal to the device band"})
        print(json.dumps(rec), flush=True)
        del band
    ctx.close()


if __name__ == "__main__":
    main()
