#!/usr/bin/env python3
"""A/B of the chain-level predict at C3 (1000 branches x 500 markers, n = 50 000, widths 4,4,1,
synthetic genotypes, seeded parameters): K saved models predicted

  arm A  one by one, the per-model path: K x (set every branch's parameters + bann_net_predict);
  arm B  from the model slots: bann_models_predict on pre-filled slots (kernels_fe.hip).

Both arms run in one process, alternating, after a warm-up of every shape; every timed window
ends with the device synchronised (both calls return after their copy to the host).  One JSON
line per K: the arms' times (best and every repeat), arm A's predict-only part (the K
bann_net_predict calls without the parameter uploads), and the algorithmic bytes.

  python tools/ensemble_bench.py [--ks 1,2,4,8,16] [--reps 3] [--branches 1000] [--n 50000]
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

from bann import BannContext, Net  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16")
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
    bias = rng.normal(scale=0.1, size=kmax).astype(np.float32)
    for b in range(nb):
        ctx.set_params(b, params[0, b])
    net = Net(ctx, seed=1)
    lib, h = ctx._lib, ctx._h
    fp = C.POINTER(C.c_float)

    def arm_a(K, upload=True):
        out = np.zeros((K, n), np.float32)
        for k in range(K):
            if upload:
                for b in range(nb):
                    rc = lib.bann_branch_set_params(h, b, params[k, b].ctypes.data_as(fp))
                    assert rc == 0
            net.set_global(2.0, 0.05, float(bias[k]))
            out[k] = net.predict()
        return out

    ctx.models_reserve(kmax)
    for k in range(kmax):
        for b in range(nb):
            ctx.models_set_params(k, b, params[k, b])
        ctx.models_set_bias(k, bias[k])

    def arm_b(K):
        return ctx.models_predict(0, K)

    def timed(f, *a):
        lib.bann_synchronize(h)
        t0 = time.perf_counter()
        r = f(*a)
        lib.bann_synchronize(h)
        return (time.perf_counter() - t0) * 1e3, r

    image = ctx.packed_genotype_bytes
    rows = nb * n * 4
    km = ctx.models_pass_width()
    for K in ks:  # warm-up of every shape, and the arms agree bit for bit
        ra, rb = arm_a(K), arm_b(K)
        assert np.array_equal(ra, rb), f"K={K}: the arms' rows differ"
    for K in ks:
        ta, tb, tp = [], [], []
        for _ in range(args.reps):
            ta.append(timed(arm_a, K)[0])
            tb.append(timed(arm_b, K)[0])
            tp.append(timed(arm_a, K, False)[0])
        passes = (K + km - 1) // km
        print(json.dumps({
            "config": "c3", "branches": nb, "markers_per_branch": m, "n": n, "widths": widths, "K": K,
            "models_per_pass": km, "passes": passes,
            "arm_a_ms": round(min(ta), 3), "arm_b_ms": round(min(tb), 3), "arm_a_predict_only_ms": round(min(tp), 3),
            "arm_a_ms_all": [round(t, 3) for t in ta], "arm_b_ms_all": [round(t, 3) for t in tb],
            "arm_a_predict_only_ms_all": [round(t, 3) for t in tp],
            "speedup_b_over_a": round(min(ta) / min(tb), 3),
            "speedup_b_over_a_predict_only": round(min(tp) / min(tb), 3),
            # arm A: per model the image, the rows written and the rows copied to the host
            "arm_a_bytes": K * (image + 2 * rows),
            # arm B: the image once per pass, the rows written and read again by the device sum
            "arm_b_bytes": passes * image + 2 * K * rows,
            "image_bytes": image}), flush=True)
    net.close()
    ctx.close()


if __name__ == "__main__":
    main()
