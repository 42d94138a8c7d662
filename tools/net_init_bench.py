#!/usr/bin/env python3
"""Starting a model at C3 (1000 branches x 500 markers, n = 50 000, widths 4,4,1, ridge_ard, synthetic
genotypes), one MI355X, two arms in one process:

  arm A  the host construction: numpy draws of every branch's parameters (weights ~ N(0, 1/m), biases
         0), the maximum-likelihood precisions and the joint output-layer precision in numpy f64, then
         one set_params and one set_precisions per branch (2 x 1000 calls);
  arm B  Net.init: bann_net_init, the same construction on the device (kernels_init.hip).

A warm-up of each arm, then the arms alternate, --reps windows each, host clock, the device
synchronised at each window's end; arm A's numpy part is also timed alone.  Beside it simulate_y
(h = 0.5): bann_net_simulate_y against bann_net_predict + numpy noise and moments on the host.
Times only: no ratio is promised; the result names the faster arm.

  python tools/net_init_bench.py [--out profiles/net_init_c3.json] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-bann_amd"))

from bann import BannContext, InitConfig, Net  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_init_c3.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--branches", type=int, default=1000)
    ap.add_argument("--markers", type=int, default=500)
    ap.add_argument("--n", type=int, default=50000)
    args = ap.parse_args()
    nb, m, n, widths = args.branches, args.markers, args.n, [4, 4, 1]
    ctx = BannContext(0)
    ctx.synthetic_genotypes(n, nb * m, seed=1000003)
    for b in range(nb):
        ctx.add_branch(np.arange(b * m, (b + 1) * m, dtype=np.int32), widths, "tanh", "ridge_ard")
    ctx.finalize(free_raw=True)
    P, Q = ctx.num_params(0), ctx.num_precisions(0)
    nw = m * 4 + 4 * 4 + 4                    # weights; the 8 biases follow
    net = Net(ctx, seed=7)
    rng = np.random.default_rng(12345)

    def host_construct():
        theta = np.zeros((nb, P), np.float32)
        theta[:, :nw] = (rng.standard_normal((nb, nw)) * np.sqrt(np.float32(1.0) / np.float32(m))).astype(np.float32)
        t64 = theta.astype(np.float64)
        prec = np.empty((nb, Q), np.float64)
        with np.errstate(divide="ignore"):
            prec[:, :m] = 4.0 / np.sum(t64[:, :4 * m].reshape(nb, 4, m) ** 2, axis=1)               # ARD rows of W0
            prec[:, m:m + 4] = 4.0 / np.sum(t64[:, 4 * m:4 * m + 16].reshape(nb, 4, 4) ** 2, axis=1)  # of W1
            prec[:, m + 4] = nb / np.sum(t64[:, 4 * m + 16:nw] ** 2)                                # joint output
            prec[:, m + 5] = 4.0 / np.sum(t64[:, nw:nw + 4] ** 2, axis=1)                           # biases: +inf
            prec[:, m + 6] = 4.0 / np.sum(t64[:, nw + 4:] ** 2, axis=1)
        prec[:, m + 7] = 2.0
        return theta, prec.astype(np.float32)

    def arm_a():
        t0 = time.perf_counter()
        theta, prec = host_construct()
        t1 = time.perf_counter()
        for b in range(nb):
            ctx.set_params(b, theta[b])
            ctx.set_precisions(b, prec[b])
        ctx.synchronize()
        t2 = time.perf_counter()
        return {"total_ms": (t2 - t0) * 1e3, "numpy_ms": (t1 - t0) * 1e3, "setters_ms": (t2 - t1) * 1e3}

    def arm_b(seed):
        t0 = time.perf_counter()
        net.init(InitConfig(), seed=seed)
        ctx.synchronize()
        return {"total_ms": (time.perf_counter() - t0) * 1e3}

    arm_a()
    arm_b(0)
    runs = {"A": [], "B": []}
    for r in range(args.reps):
        runs["A"].append(arm_a())
        runs["B"].append(arm_b(r + 1))

    # simulate_y at h = 0.5 against predict + host noise; the parameters are arm B's last draw
    def sim_device(seed):
        t0 = time.perf_counter()
        y, st = net.simulate_y(0.5, seed=seed)
        return (time.perf_counter() - t0) * 1e3

    def sim_host(seed):
        t0 = time.perf_counter()
        g = net.predict().astype(np.float64)
        rv = np.var(g, ddof=1) * (1.0 / 0.5 - 1.0)
        y = (g.astype(np.float32) + (np.sqrt(rv) * np.random.default_rng(seed).standard_normal(n)).astype(np.float32))
        y64 = y.astype(np.float64)
        _ = (float(np.mean(y64)), float(np.var(y64, ddof=1)), float(rv))
        return (time.perf_counter() - t0) * 1e3

    sim_device(0)
    sim_host(0)
    sim = {"device": [], "host": []}
    for r in range(args.reps):
        sim["host"].append(sim_host(r + 1))
        sim["device"].append(sim_device(r + 1))

    def r3(v):
        return round(float(v), 3)

    best_a = min(runs["A"], key=lambda t: t["total_ms"])
    a_ms, b_ms = best_a["total_ms"], min(t["total_ms"] for t in runs["B"])
    result = {"config": "c3", "branches": nb, "markers_per_branch": m, "n": n, "widths": widths, "prior": "ridge_ard",
              "windows": args.reps, "params_per_branch": P, "precisions_per_branch": Q,
              "arm_a_host_ms": r3(a_ms), "arm_a_numpy_ms": r3(best_a["numpy_ms"]),
              "arm_a_setters_ms": r3(best_a["setters_ms"]),
              "arm_a_ms_all": [r3(t["total_ms"]) for t in runs["A"]],
              "arm_b_net_init_ms": r3(b_ms), "arm_b_ms_all": [r3(t["total_ms"]) for t in runs["B"]],
              "faster_arm": "B (Net.init)" if b_ms < a_ms else "A (host)",
              "simulate_y_device_ms": r3(min(sim["device"])), "simulate_y_device_ms_all": [r3(v) for v in sim["device"]],
              "predict_plus_numpy_noise_ms": r3(min(sim["host"])),
              "predict_plus_numpy_noise_ms_all": [r3(v) for v in sim["host"]],
              "simulate_y_faster": "device" if min(sim["device"]) < min(sim["host"]) else "host",
              "not_measured": "kernel times of the init kernels (no kernel trace taken); how arm A's setter time splits"}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    net.close()
    ctx.close()


if __name__ == "__main__":
    main()
