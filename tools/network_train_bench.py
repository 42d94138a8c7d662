#!/usr/bin/env python3
"""A/B of the Gibbs step inside bann_net_train_network at C3 (1000 branches x 500 markers,
n = 50 000, widths 4,4,1, ridge_ard, synthetic genotypes, seeded parameters; built as
tools/chain_stats_bench.py builds it), one MI355X, L = 20, the context's default step rule:

  arm host    gibbs="host": sample_prior_precisions on the host copy of theta
              (std::gamma_distribution) and one bann_branch_set_precisions per branch;
  arm device  gibbs="device": bann_gibbs_posterior + one bann_gibbs_sample_precisions launch
              (kernels_gibbs.hip).

One process, one net: a warm-up sweep of each arm, then the arms alternate, --sweeps sweeps per
window, --reps windows each.  Per arm: ms per sweep (the three phases of bann_net_network_timing,
each ending in a device synchronise; best window and every window), the phase times of the best
window per sweep, leapfrog steps/s including the Gibbs step, the spread of the windows, and the
trajectories accepted.  The whole call per sweep (with train_begin's residual pass and first
record) is reported beside it.

  python tools/network_train_bench.py [--out profiles/network_train_c3.json] [--sweeps 5] [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-bann_amd"))

from bann import BannContext, MCMCConfig, Net  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_train_c3.json"))
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--factor", type=float, default=0.1)
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
    P = ctx.num_params(0)
    rng = np.random.default_rng(12345)
    params = (rng.normal(size=(nb, P)) / np.sqrt(m)).astype(np.float32)   # W ~ N(0, 1/fan-in)
    for b in range(nb):
        ctx.set_params(b, params[b])
    y = rng.normal(size=n).astype(np.float32)
    net = Net(ctx, seed=7)

    def window(arm, sweeps):
        before = net.summary()
        net.train_network(y, MCMCConfig(hmc_integration_length=args.L, chain_length=sweeps,
                                        hmc_step_size_factor=args.factor), gibbs=arm)
        t = net.network_timing()
        after = net.summary()
        t["accepted"] = int(after["num_accepted"] - before["num_accepted"])
        return t

    arms = ("host", "device")
    for arm in arms:   # warm-up: every kernel, buffer and plan of the arm
        window(arm, 1)
    runs = {arm: [] for arm in arms}
    for _ in range(args.reps):
        for arm in arms:
            runs[arm].append(window(arm, args.sweeps))
    result = {"config": "c3", "branches": nb, "markers_per_branch": m, "n": n, "widths": widths, "prior": "ridge_ard",
              "L": args.L, "step_factor": args.factor, "step_rule": ctx.network_step_rule_state(),
              "sweeps_per_window": args.sweeps, "windows": args.reps, "arms": {}}
    for arm in arms:
        sweep_ms = [(t["gibbs_ms"] + t["trajectory_ms"] + t["record_ms"]) / args.sweeps for t in runs[arm]]
        best = runs[arm][int(np.argmin(sweep_ms))]
        result["arms"][arm] = {
            "sweep_ms": round(min(sweep_ms), 3), "sweep_ms_all": [round(v, 3) for v in sweep_ms],
            "spread_pct": round(100.0 * (max(sweep_ms) - min(sweep_ms)) / min(sweep_ms), 2),
            "gibbs_ms": round(best["gibbs_ms"] / args.sweeps, 3),
            "trajectory_ms": round(best["trajectory_ms"] / args.sweeps, 3),
            "record_ms": round(best["record_ms"] / args.sweeps, 3),
            "gibbs_ms_all": [round(t["gibbs_ms"] / args.sweeps, 3) for t in runs[arm]],
            "call_ms_per_sweep_all": [round(t["total_ms"] / args.sweeps, 3) for t in runs[arm]],
            "leapfrog_steps_per_s": round(args.L * 1e3 / min(sweep_ms), 1),
            "accepted_all": [t["accepted"] for t in runs[arm]]}
    h, d = result["arms"]["host"], result["arms"]["device"]
    result["sweep_speedup_device_over_host"] = round(h["sweep_ms"] / d["sweep_ms"], 3)
    result["gibbs_speedup_device_over_host"] = round(h["gibbs_ms"] / d["gibbs_ms"], 3)
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
