#!/usr/bin/env python3
"""The cohort subset at scale (kernels_subset.hip): a synthetic cohort on the device, by default the C3
shape of bench.py (n = 50 000, M = 500 000), and three cases:

  split      an 80 / 20 split of the individuals, two ascending lists (bann.io.split_indices), two subsets
  extract    every second marker, every individual (the row-copy kernel)
  bootstrap  n draws of the individuals with replacement, unsorted

Per case:
  kernel_ms  HIP-event time of the subset launches (BannContext.subset_timing; for split the sum of the two)
  bytes      the source rows touched (whole rows) plus the destination image written
  copy_ms    the yardstick: HIP-event time of one plain device-to-device hipMemcpyAsync in this process
             that reads bytes / 2 and writes bytes / 2, the same traffic
  host_ms    host clock around the subset() calls: index upload, gather, column statistics, synchronise
  route_ms   the only route without the kernel: download_genotypes of a block of --host-markers markers
             as int8, numpy indexing, upload_genotypes into a new context; route_scaled_ms scales the
             best window linearly in M to the whole cohort: an extrapolation, not a measurement

One warm-up of every arm, then --reps rounds in which the arms alternate, each round starting one arm
later; best of the rounds, all values and the spread kept.  Every case is checked on --check markers
spread over the cohort (the last one included: byte offsets beyond 2^32) against numpy on the source's
downloaded rows.

  python tools/subset_bench.py [--n 50000] [--markers 500000] [--reps 3] [--host-markers 2000]
                               [--out profiles/subset.json]
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

D2D = 3  # hipMemcpyDeviceToDevice


def spread(ts):
    return {"best": round(min(ts), 3), "all": [round(t, 3) for t in ts],
            "spread_pct": round(100.0 * (max(ts) - min(ts)) / min(ts), 2)}


class Hip:
    """the few runtime calls of the yardstick"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            self.ok(self.lib.hipEventCreate(C.byref(e)))

    @staticmethod
    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.lib.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
        return p

    def free(self, p):
        self.ok(self.lib.hipFree(p))

    def copy_ms(self, dst, src, nbytes):
        self.ok(self.lib.hipDeviceSynchronize())
        self.ok(self.lib.hipEventRecord(self.ev[0], None))
        self.ok(self.lib.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), D2D, None))
        self.ok(self.lib.hipEventRecord(self.ev[1], None))
        self.ok(self.lib.hipEventSynchronize(self.ev[1]))
        ms = C.c_float()
        self.ok(self.lib.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]))
        return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--markers", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-markers", type=int, default=2000)
    ap.add_argument("--check", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bann import BannContext
    from bann.io import split_indices
    n, M = args.n, args.markers
    src = BannContext(0)
    src.synthetic_genotypes(n, M, seed=1000003)
    hip = Hip()
    rowb = lambda k: (k + 63) // 64 * 16
    rng = np.random.default_rng(11)
    train, test = split_indices(n, n // 5, seed=3)
    cases = {
        "split": [dict(individuals=train), dict(individuals=test)],
        "extract": [dict(markers=np.arange(0, M, 2))],
        "bootstrap": [dict(individuals=rng.integers(0, n, size=n))],
    }

    def moved(kw):
        nk = n if kw.get("individuals") is None else len(kw["individuals"])
        mk = M if kw.get("markers") is None else len(kw["markers"])
        return mk * rowb(n) + mk * rowb(nk)

    nbytes = {name: sum(moved(kw) for kw in parts) for name, parts in cases.items()}
    half = max(nbytes.values()) // 2
    buf_a, buf_b = hip.malloc(half), hip.malloc(half)
    H = min(args.host_markers, M)
    check = np.unique(np.linspace(0, M - 1, args.check).astype(np.int64))

    def run_subset(name, verify=False):
        """(kernel ms, host ms) of the case's subset calls"""
        kern, t_host = 0.0, 0.0
        for kw in cases[name]:
            src._lib.bann_synchronize(src._h)
            t0 = time.perf_counter()
            dst = src.subset(**kw)
            t_host += (time.perf_counter() - t0) * 1e3
            kern += dst.subset_timing()
            if verify:
                mk = np.arange(M) if kw.get("markers") is None else np.asarray(kw["markers"])
                pick = check[check < mk.size]
                want = src.download_genotypes(mk[pick])
                if kw.get("individuals") is not None:
                    want = want[:, kw["individuals"]]
                if not np.array_equal(dst.download_genotypes(pick), want):
                    raise RuntimeError(f"{name}: the subset differs from numpy on the source's rows")
            dst.close()
        return kern, t_host

    def run_route(name):
        """the case over the first H source markers through the host, ms"""
        src._lib.bann_synchronize(src._h)
        t0 = time.perf_counter()
        for kw in cases[name]:
            mk = np.arange(M) if kw.get("markers") is None else np.asarray(kw["markers"])
            g = src.download_genotypes(mk[mk < H])
            if kw.get("individuals") is not None:
                g = g[:, kw["individuals"]]
            with BannContext(0) as dst:
                dst.upload_genotypes(g)
        return (time.perf_counter() - t0) * 1e3

    arms = [(name, kind) for name in cases for kind in ("subset", "copy", "route")]
    res = {arm: [] for arm in arms}
    host = {name: [] for name in cases}

    def run(arm, record, verify=False):
        name, kind = arm
        if kind == "subset":
            k, t = run_subset(name, verify)
            if record:
                res[arm].append(k)
                host[name].append(t)
        elif kind == "copy":
            ms = hip.copy_ms(buf_b, buf_a, nbytes[name] // 2)
            if record:
                res[arm].append(ms)
        else:
            ms = run_route(name)
            if record:
                res[arm].append(ms)

    for arm in arms:                                   # warm-up, and the check against numpy
        run(arm, False, verify=True)
    for rep in range(args.reps):
        k = rep % len(arms)
        for arm in arms[k:] + arms[:k]:
            run(arm, True)
    rec = {"tool": "tools/subset_bench.py", "n": n, "markers": M, "image_bytes": rowb(n) * M, "reps": args.reps,
           "route_host_markers": H, "checked_markers": [int(c) for c in check],
           "copy_note": "one device-to-device hipMemcpyAsync of bytes / 2: it reads and writes bytes in all",
           "route_note": "download_genotypes (int8), numpy indexing, upload_genotypes over the first "
                         "route_host_markers source markers; route_scaled_ms scales the best window "
                         "linearly in M: an extrapolation",
           "cases": {}}
    for name in cases:
        k, c, r = min(res[(name, "subset")]), min(res[(name, "copy")]), min(res[(name, "route")])
        rec["cases"][name] = {"bytes": nbytes[name], "kernel_ms": spread(res[(name, "subset")]),
                              "copy_ms": spread(res[(name, "copy")]), "kernel_over_copy": round(k / c, 3),
                              "kernel_GBs": round(nbytes[name] / k / 1e6, 1), "copy_GBs": round(nbytes[name] / c / 1e6, 1),
                              "host_ms": spread(host[name]), "route_ms": spread(res[(name, "route")]),
                              "route_scaled_ms": round(r * M / H, 1),
                              "route_scaled_over_host": round(r * M / H / min(host[name]), 1)}
    rec["furthest_from_copy"] = max(cases, key=lambda nm: rec["cases"][nm]["kernel_over_copy"])
    hip.free(buf_a)
    hip.free(buf_b)
    src.close()
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
