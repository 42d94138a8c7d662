#!/usr/bin/env python3
"""A/B of the chain-level branch statistics at C3 (1000 branches x 500 markers, n = 50 000, widths
4,4,1, synthetic genotypes, seeded parameters): per model and branch the rss against y and the
population effect sizes of K saved models

  arm A  one by one through the live state, what a user does per model without the slots: set every
         branch's parameters, bann_population_effect_sizes over all branches, then bann_set_target_all
         + bann_log_density_gradient_many for the rss;
  arm B  from the model slots: bann_models_branch_stats on pre-filled slots (kernels_fs.hip).

Both arms run in one process, alternating, after a warm-up of every shape that also checks the arms
against each other (pop norm-relative 1e-5 per model, rss 1e-5 relative); every timed window ends
with the device synchronised.  One JSON line per K: the arms' times (best and every repeat), the
HIP-event time of arm B's k_stats_fe launches (bann_models_branch_stats_timed, a call of its own
after the timed windows) per call and per model, and the algorithmic bytes.

  python tools/chain_stats_bench.py [--ks 1,4,8] [--reps 3] [--branches 1000] [--n 50000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-bann_amd"))

from bann import BannContext  # noqa: E402

# profiles/ensemble_c3.json's kernel trace: k_forward_fe per model at K = 8, and the
# stream floor of one pass over the C3 image, for scale
FORWARD_FE_MS_PER_MODEL = 0.64
STREAM_FLOOR_MS = 0.92


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--branches", type=int, default=1000)
    ap.add_argument("--markers", type=int, default=500)
    ap.add_argument("--n", type=int, default=50000)
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    nb, m, n, widths = args.branches, args.markers, args.n, [4, 4, 1]
    ctx = BannContext(0)
    ctx.synthetic_genotypes(n, nb * m, seed=1000003)
    for b in range(nb):
        ctx.add_branch(np.arange(b * m, (b + 1) * m, dtype=np.int32), widths, "tanh", "ridge_ard")
    ctx.finalize(free_raw=True)
    P = ctx.num_params(0)
    kmax = max(ks)
    rng = np.random.default_rng(12345)
    # W ~ N(0, 1/fan-in) as the default init (branch_cfg_builder.rs:180-186), small biases
    params = (rng.normal(size=(kmax, nb, P)) / np.sqrt(m)).astype(np.float32)
    y = rng.normal(size=n).astype(np.float32)
    lib, h = ctx._lib, ctx._h
    fp = C.POINTER(C.c_float)
    all_b = list(range(nb))

    def arm_a(K):
        pop = np.zeros((K, nb * m), np.float32)
        rss = np.zeros((K, nb), np.float64)
        for k in range(K):
            for b in range(nb):
                rc = lib.bann_branch_set_params(h, b, params[k, b].ctypes.data_as(fp))
                assert rc == 0
            pop[k] = ctx.population_effect_sizes(all_b)
            ctx.set_target_all(y)
            rss[k] = ctx.log_density_gradient_many(all_b)[1]
        return pop, rss

    ctx.models_reserve(kmax)
    for k in range(kmax):
        for b in range(nb):
            ctx.models_set_params(k, b, params[k, b])

    def arm_b(K):
        st = ctx.models_branch_stats(0, K, y=y)
        return st["pop"], st["rss"]

    def kernel_ms(K):
        bl = np.arange(nb, dtype=np.int32)
        pop = np.zeros((K, nb * m), np.float32)
        rss = np.zeros((K, nb), np.float64)
        ms = C.c_float()
        rc = lib.bann_models_branch_stats_timed(h, 0, K, bl.ctypes.data_as(C.POINTER(C.c_int32)), nb,
                                                y.ctypes.data_as(fp), rss.ctypes.data_as(C.POINTER(C.c_double)),
                                                pop.ctypes.data_as(fp), C.byref(ms))
        assert rc == 0
        return ms.value

    def timed(f, *a):
        lib.bann_synchronize(h)
        t0 = time.perf_counter()
        r = f(*a)
        lib.bann_synchronize(h)
        return (time.perf_counter() - t0) * 1e3, r

    image = ctx.packed_genotype_bytes
    ks_pass = ctx.models_stats_pass_width()
    for K in ks:  # warm-up of every shape, and the arms agree
        (pa, ra), (pb, rb) = arm_a(K), arm_b(K)
        for k in range(K):
            err = np.linalg.norm(pa[k].astype(np.float64) - pb[k]) / np.linalg.norm(pa[k].astype(np.float64))
            assert err < 1e-5, f"K={K} model {k}: the arms' population effect sizes differ by {err:.3e}"
            assert np.all(np.abs(ra[k] - rb[k]) <= 1e-5 * np.maximum(1.0, np.abs(ra[k]))), f"K={K} model {k}: rss"
    for K in ks:
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(arm_a, K)[0])
            tb.append(timed(arm_b, K)[0])
        kms = [kernel_ms(K) for _ in range(args.reps)]
        passes = (K + ks_pass - 1) // ks_pass
        print(json.dumps({
            "config": "c3", "branches": nb, "markers_per_branch": m, "n": n, "widths": widths, "K": K,
            "models_per_pass": ks_pass, "passes": passes,
            "arm_a_ms": round(min(ta), 3), "arm_b_ms": round(min(tb), 3),
            "arm_a_ms_all": [round(t, 3) for t in ta], "arm_b_ms_all": [round(t, 3) for t in tb],
            "speedup_b_over_a": round(min(ta) / min(tb), 3),
            # HIP events around the k_stats_fe launches of one arm-B call (every pass)
            "k_stats_fe_ms_per_call": round(min(kms), 4), "k_stats_fe_ms_per_call_all": [round(t, 4) for t in kms],
            "k_stats_fe_ms_per_model": round(min(kms) / K, 4),
            "k_stats_fe_ms_per_pass": round(min(kms) / passes, 4),
            "k_forward_fe_ms_per_model_for_scale": FORWARD_FE_MS_PER_MODEL,
            "stream_floor_ms_per_pass": STREAM_FLOOR_MS,
            "k_stats_fe_pass_over_stream_floor": round(min(kms) / passes / STREAM_FLOOR_MS, 3),
            # arm A: per model the image by forward_feed's layer 0 and again by the gradient launch, and
            # 200 MB of targets; its [w][n] f32 layer scratch is not counted
            "arm_a_bytes": K * (2 * image + nb * n * 4),
            # arm B: the image once per pass; y (200 KB) stays in L2; 40 bytes per model and work item out
            "arm_b_bytes": passes * image,
            "image_bytes": image}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
