#!/usr/bin/env python3
"""The linear score at scale (kernels_lin.hip): a synthetic cohort on the device, by default the C3
shape (n = 50 000, 1 000 uniform groups of 500 markers), effects from linear_effects.

  arm A   what the library offered before: download_genotypes in blocks of --block markers, the
          standardisation and the product in numpy f32 on the host (at most 16 threads).  Only the
          first --host-markers markers are processed and the time is SCALED linearly in M to the whole
          cohort: a1_scaled_ms is an extrapolation, not a measurement.
  arm B   BannContext.linear_score at K = 1, 4, 8: host-clock time of the call (uploads of the effects
          and the copy back included) and the HIP-event time of its device kernels (linear_timing).

One warm-up of each arm, then --reps rounds in which the arms alternate (A, B1, B4, B8, each round
starting one arm later, so that no arm always follows the same one); every timed window ends with the
device synchronised; best of the rounds.  kernel_ms_per_pass = kernel time /
ceil(K / 4) genotype passes, against (rowb x entries) bytes at 8 TB/s.
The accuracy record compares the K = 8 scores of --sample individuals with an f64 host score over all
entries (the genotypes come back through download_genotypes in blocks): norm-relative error per column.

  python tools/linear_bench.py [--n 50000] [--groups 1000] [--group-size 500] [--reps 3]
                               [--host-markers 5000] [--sample 1000] [--out profiles/linear_score.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-bann_amd"))

HBM_SPEC = 8.0e12
KP = 4  # columns per genotype pass (LIN_KP)


def spread(ts):
    return {"best": round(min(ts), 3), "all": [round(t, 3) for t in ts],
            "spread_pct": round(100.0 * (max(ts) - min(ts)) / min(ts), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--group-size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=5000)
    ap.add_argument("--host-markers", type=int, default=5000)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bann import BannContext
    from bann.io import uniform_grouping
    n, M = args.n, args.groups * args.group_size
    groups = uniform_grouping(args.groups, args.group_size)
    ctx = BannContext(0)
    ctx.synthetic_genotypes(n, M, seed=1000003)
    lib, h = ctx._lib, ctx._h
    mu, sd = ctx.genotype_stats()
    eff = np.stack([ctx.linear_effects(M, 0.5, seed=100 + k)[0] for k in range(8)])
    H = min(args.host_markers, M)

    def arm_a():
        """scores of the first H markers' entries, K = 1, on the host"""
        out = np.zeros(n, np.float32)
        for j0 in range(0, H, args.block):
            idx = np.arange(j0, min(H, j0 + args.block))
            g = ctx.download_genotypes(idx).astype(np.float32)
            s = np.where(sd[idx] > 0, sd[idx], 1.0)
            w = np.where(sd[idx] > 0, eff[0, idx] / s, 0.0).astype(np.float32)
            out += w @ g - np.float32(w @ mu[idx])
        return out

    def timed(f, *a):
        lib.bann_synchronize(h)
        t0 = time.perf_counter()
        r = f(*a)
        lib.bann_synchronize(h)
        return (time.perf_counter() - t0) * 1e3, r

    ks = (1, 4, 8)
    timed(arm_a)
    for K in ks:
        timed(ctx.linear_score, groups, eff[:K])
    a_ms, b_host, b_kern = [], {K: [] for K in ks}, {K: [] for K in ks}
    score8 = None
    order = ["A"] + list(ks)
    for rep in range(args.reps):
        for arm in order[rep % len(order):] + order[:rep % len(order)]:   # the round starts one arm later each time
            if arm == "A":
                a_ms.append(timed(arm_a)[0])
                continue
            t, r = timed(ctx.linear_score, groups, eff[:arm])
            b_host[arm].append(t)
            b_kern[arm].append(ctx.linear_timing())
            if arm == 8:
                score8 = r
    rowb = (n + 63) // 64 * 16
    pass_bytes = rowb * M
    floor_ms = pass_bytes / HBM_SPEC * 1e3
    rec = {"tool": "tools/linear_bench.py", "n": n, "markers": M, "groups": args.groups,
           "group_size": args.group_size, "entries": M, "image_bytes_per_pass": pass_bytes,
           "stream_ms_at_8TBs": round(floor_ms, 4), "columns_per_pass": KP,
           "a_host_markers": H, "a_host_threads": min(16, os.cpu_count() or 1), "a_ms": spread(a_ms),
           "a1_scaled_ms": round(min(a_ms) * M / H, 1),
           "a_note": "K = 1; numpy f32 on the host over the first a_host_markers markers through "
                     "download_genotypes; a1_scaled_ms scales the best window linearly in M, an extrapolation",
           "b": {}}
    for K in ks:
        passes = -(-K // KP)
        per_pass = min(b_kern[K]) / passes
        rec["b"][f"K{K}"] = {"host_ms": spread(b_host[K]), "kernel_ms": spread(b_kern[K]), "passes": passes,
                             "kernel_ms_per_pass": round(per_pass, 4),
                             "ratio_to_8TBs_stream": round(per_pass / floor_ms, 3),
                             "a1_scaled_over_b_host": round(min(a_ms) * M / H / min(b_host[K]), 1)}
    # accuracy: f64 on the host, every entry, a sample of the individuals
    rng = np.random.default_rng(7)
    pick = np.sort(rng.choice(n, size=min(args.sample, n), replace=False))
    ref = np.zeros((8, pick.size), np.float64)
    sd64, mu64 = sd.astype(np.float64), mu.astype(np.float64)
    for j0 in range(0, M, 2 * args.block):
        idx = np.arange(j0, min(M, j0 + 2 * args.block))
        g = ctx.download_genotypes(idx)[:, pick].astype(np.float64)
        safe = np.where(sd64[idx] > 0, sd64[idx], 1.0)
        x = (g - mu64[idx, None]) / safe[:, None]
        x[sd64[idx] <= 0] = 0.0
        ref += eff[:, idx].astype(np.float64) @ x
    got = score8[:, pick].astype(np.float64)
    err = [float(np.linalg.norm(got[k] - ref[k]) / np.linalg.norm(ref[k])) for k in range(8)]
    rec["accuracy"] = {"sampled_individuals": int(pick.size), "entries": M, "chunk_entries": 2048,
                       "norm_rel_error_per_column": [float(f"{e:.3e}") for e in err],
                       "max": float(f"{max(err):.3e}")}
    ctx.close()
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
