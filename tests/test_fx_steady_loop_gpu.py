"""The fx gradient kernel's two tile loops (k_fused_grad_fx, kernels_fx.hip): a steady body for
tiles whose successor two rounds on exists and is full, the guarded body for the rest.

Shapes are chosen by how many steady iterations a wave of a ONE-item branch runs (the
contexts below are built with BANN_TARGET_ITEMS=1 and BANN_SOLO=0, so a branch is one work
item whose four waves take tiles w, w + 4, w + 8, ...; a tile is steady when tile + 8 is a
full tile of the item):
  n = 130   3 tiles, the last partial; one wave has none; no steady tile
  n = 256   one tile per wave; no steady tile
  n = 520   9 tiles, wave 0 has three; its first tile's successor is the partial tile 8,
            so it stays guarded (the steady body reads the successor's target rows unclamped)
  n = 576   9 full tiles: wave 0 runs exactly one steady iteration
  n = 1100  18 tiles, 5/5/4/4 per wave, partial last tile: 3/2/2/2 steady iterations
  n = 1280  20 full tiles: 3 steady iterations per wave, the full final tile still guarded
crossed with m = 500 (padding rows, NCH = 8), 512 (NCH = 8), 448 and 100 (NCH = 0), the
widths [4,1], [4,4,1], [4,4,4,1], [3,2,1], tanh and ReLU, three branches per launch.

The gradient of the packed launch and of a solo plan (default options: the branch alone is
re-split to about a tile per wave) is compared with the float64 oracle at the parity suite's
tolerance (tests/test_gpu_parity.py: norm-relative 1e-5, rss 1e-5 relative), and two
launches must repeat bit for bit.
"""
import ctypes

import numpy as np
import pytest

import bann_oracle as O
from helpers import build_context, f32_branch, norm_rel, x_std

pytestmark = pytest.mark.gpu

TOL = 1e-5
NS = [130, 256, 520, 576, 1100, 1280]
MS = [500, 512, 448, 100]
WIDTHS = [[4, 1], [4, 4, 1], [4, 4, 4, 1], [3, 2, 1]]
ACTS = ["tanh", "relu"]
PER_LAUNCH = 3


@pytest.fixture(scope="module")
def Ctx():
    from bann import BannContext
    return BannContext


def scalar_close(a, b, tol=TOL):
    return abs(a - b) <= tol * max(1.0, abs(b))


def test_dma_immediate_offset_addressing():
    """which addresses the immediate offset of global_load_lds_dwordx4 advances: four pieces at
    offsets 0, 1024, 2048, 3072 from one M0 against the source.  The library's steady tiles may
    share one M0 per 4 KiB half slot (mode 2) only if the offset reaches the LDS address too."""
    from bann._lib import load_library
    lib = load_library()
    follows, mode = ctypes.c_int32(-2), ctypes.c_int32(-2)
    assert lib.bann_fx_dma_offset_probe(ctypes.byref(follows), ctypes.byref(mode)) == 0
    print(f"immediate offset advances the LDS address: {follows.value}; library built for mode {mode.value}")
    assert follows.value in (0, 1), "the copy matches neither addressing"
    assert mode.value in (0, 2)
    if mode.value == 2:
        assert follows.value == 1


_problems = {}


def one_item_env(monkeypatch):
    monkeypatch.setenv("BANN_TARGET_ITEMS", "1")
    monkeypatch.setenv("BANN_SOLO", "0")


def problem(n, m):
    """genotypes, branch specs (PER_LAUNCH per widths x activation) and the oracle's gradients,
    computed once per (n, m) against the device's own standardisation constants"""
    if (n, m) not in _problems:
        rng = np.random.default_rng(1000 * n + m)
        M = m + 5
        g = O.synthetic_genotypes(rng, n, M)
        specs = []
        for w in WIDTHS:
            for act in ACTS:
                for _ in range(PER_LAUNCH):
                    snps = rng.permutation(M)[:m].astype(np.int32)
                    br = f32_branch(O.random_branch(rng, m, w, prior="ridge_ard", act=act))
                    specs.append(dict(snps=snps, branch=br, y=np.zeros(n)))
        _problems[(n, m)] = dict(g=g, specs=specs, rng=rng, ref=None)
    return _problems[(n, m)]


def with_reference(p, ctx):
    if p["ref"] is None:
        mu, sd = ctx.genotype_stats()
        ref = []
        for s in p["specs"]:
            X = x_std(p["g"][s["snps"]], mu[s["snps"]], sd[s["snps"]])
            f = O.predict(s["branch"], X)
            s["y"] = (f + p["rng"].normal(scale=max(float(np.std(f)), 0.1), size=f.size)).astype(np.float32).astype(
                np.float64)
            gw, gb, rss = O.log_density_gradient(s["branch"], X, s["y"])
            ref.append((O.param_vec(gw, gb), rss))
        p["ref"] = ref
    return p["ref"]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_packed_launch_matches_oracle_and_repeats(Ctx, monkeypatch, n, m):
    one_item_env(monkeypatch)
    p = problem(n, m)
    ctx = build_context(Ctx, p["g"], p["specs"])
    ref = with_reference(p, ctx)
    nb = len(p["specs"])
    for b, s in enumerate(p["specs"]):
        assert ctx.kernel_path(b) == "fused"
        ctx.set_target(b, s["y"])
    g1, r1 = ctx.log_density_gradient_many(list(range(nb)))
    g2, r2 = ctx.log_density_gradient_many(list(range(nb)))
    for b in range(nb):
        assert np.array_equal(g1[b], g2[b]) and r1[b] == r2[b], b
        e = norm_rel(g1[b], ref[b][0])
        assert e < TOL, (b, p["specs"][b]["branch"].layer_widths, p["specs"][b]["branch"].act, e)
        assert scalar_close(r1[b], ref[b][1]), (b, r1[b], ref[b][1])
    ctx.close()


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_solo_plan_matches_oracle_and_repeats(Ctx, n, m):
    p = problem(n, m)
    ctx = build_context(Ctx, p["g"], p["specs"])
    ref = with_reference(p, ctx)
    for b, s in enumerate(p["specs"]):
        ctx.set_target(b, s["y"])
    for b in range(0, len(p["specs"]), PER_LAUNCH):  # one branch of every widths x activation group
        g1, r1 = ctx.log_density_gradient(b)
        g2, r2 = ctx.log_density_gradient(b)
        assert np.array_equal(g1, g2) and r1 == r2, b
        e = norm_rel(g1, ref[b][0])
        assert e < TOL, (b, e)
        assert scalar_close(r1, ref[b][1]), (b, r1, ref[b][1])
    ctx.close()


def test_trajectory_beside_prediction_launches(Ctx, monkeypatch):
    """one leapfrog trajectory of 3 steps over three one-item branches: its first and last
    gradient launches write predictions (every tile guarded), the ones between run steady
    tiles; trace, status and end state against the oracle's hmc_step"""
    one_item_env(monkeypatch)
    rng = np.random.default_rng(77)
    n, m, L, nb = 1100, 500, 3, 3
    g = O.synthetic_genotypes(rng, n, nb * m)
    specs = [dict(snps=np.arange(b * m, (b + 1) * m, dtype=np.int32),
                  branch=f32_branch(O.random_branch(rng, m, [4, 4, 1], prior="ridge_ard", act="tanh")), y=np.zeros(n))
             for b in range(nb)]
    ctx = build_context(Ctx, g, specs)
    mu, sd = ctx.genotype_stats()
    eps, mom, Xs = [], [], []
    for b, s in enumerate(specs):
        X = x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]])
        s["y"] = (O.predict(s["branch"], X) + rng.normal(scale=0.5, size=n)).astype(np.float32).astype(np.float64)
        ctx.set_target(b, s["y"])
        ew, eb = O.izmailov_step_sizes(s["branch"], 0.5, L)
        eps.append(O.param_vec(ew, eb).astype(np.float32))
        mom.append(rng.normal(size=s["branch"].num_params).astype(np.float32))
        Xs.append(X)
    res = ctx.hmc_step(list(range(nb)), L, 10.0, eps=np.concatenate(eps), momentum=np.concatenate(mom), u=[0.5] * nb)
    for b, s in enumerate(specs):
        br = s["branch"].copy()
        ow, ob = O.load_param_vec(eps[b].astype(np.float64), m, br.layer_widths)
        pw, pb = O.load_param_vec(mom[b].astype(np.float64), m, br.layer_widths)
        out = O.hmc_step(br, Xs[b], s["y"], ow, ob, pw, pb, L, 10.0, 0.5)
        assert res["status"][b] == out["status"], b
        tr = np.asarray(out["trace"])
        gt = res["trace"][b][: tr.size]
        assert np.all(np.abs(gt - tr) <= 1e-5 * np.maximum(1.0, np.abs(tr))), (b, gt, tr)
        assert norm_rel(ctx.get_params(b), O.param_vec(br.weights, br.biases)) < 1e-5, b
    ctx.close()
    # the session entry points (device draws) on the same problem: two runs agree bit for bit
    ends = []
    for _ in range(2):
        ctx = build_context(Ctx, g, specs)
        ctx.leapfrog_begin(list(range(nb)), L, 10.0, "izmailov", 0.5, seed=9)
        ctx.leapfrog_steps(L)
        status, acc = ctx.leapfrog_end()
        assert acc == int(np.sum(status == 0))
        ends.append((status.copy(), [ctx.get_params(b) for b in range(nb)]))
        ctx.close()
    assert np.array_equal(ends[0][0], ends[1][0])
    for b in range(nb):
        assert np.all(np.isfinite(ends[0][1][b])) and np.array_equal(ends[0][1][b], ends[1][1][b]), b


def test_network_hmc_step_steady_tiles(Ctx, monkeypatch):
    """one network-joint trajectory: the gradient launches read the network's output error
    (the net_err path) in steady and guarded tiles; trace, status and parameters against the
    oracle's network_hmc_step"""
    one_item_env(monkeypatch)
    rng = np.random.default_rng(78)
    n, m, L, nb = 1100, 500, 4, 3
    g = O.synthetic_genotypes(rng, n, nb * m)
    specs = [dict(snps=np.arange(b * m, (b + 1) * m, dtype=np.int32),
                  branch=f32_branch(O.random_branch(rng, m, [4, 4, 1], prior="ridge_ard")), y=np.zeros(n))
             for b in range(nb)]
    ctx = build_context(Ctx, g, specs)
    assert all(ctx.kernel_path(b) == "fused" for b in range(nb))
    mu, sd = ctx.genotype_stats()
    Xs = [x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]]) for s in specs]
    f = sum(O.predict(s["branch"], X) for s, X in zip(specs, Xs))
    y = (f + rng.normal(scale=0.5, size=n)).astype(np.float32).astype(np.float64)
    eps, mom = [], []
    for s in specs:
        ew, eb = O.izmailov_step_sizes(s["branch"], 0.3, L)
        eps.append(O.param_vec(ew, eb).astype(np.float32))
        mom.append(rng.normal(size=s["branch"].num_params).astype(np.float32))
    res = ctx.network_hmc_step(y, L, bias=0.1, lambda_e=2.0, eps=np.concatenate(eps), momentum=np.concatenate(mom),
                               u=0.4)
    brs = [s["branch"].copy() for s in specs]
    out = O.network_hmc_step(brs, Xs, y, 0.1, 2.0, [e.astype(np.float64) for e in eps],
                             [q.astype(np.float64) for q in mom], L, 10.0, 0.4)
    assert res["status"] == out["status"], (res["status"], out["status"], res["trace"], out["trace"])
    tr = np.asarray(out["trace"])
    assert np.all(np.abs(res["trace"][: tr.size] - tr) <= 1e-5 * np.maximum(1.0, np.abs(tr))), (res["trace"], tr)
    for b, br in enumerate(brs):
        assert norm_rel(ctx.get_params(b), O.param_vec(br.weights, br.biases)) < 1e-5, b
    ctx.close()
