"""GPU tests of the chain-level branch statistics (bann_models_branch_stats): per model
slot and branch the rss of f_b against y (rs-bann branch-r2) and the population effect
sizes (rs-bann population-effect-sizes), from a statistics pass over the model slots
(k_stats_fe, kernels_fs.hip) that writes nothing n-sized.

References: the float64 oracle (O.rss, O.population_effect_sizes) and the live path of
the same context after set_params (population_effect_sizes, log_density_gradient_many's
rss).  Tolerances: pop norm-relative 1e-5 per branch (test_effect_sizes_gpu.py), rss
1e-5 max(1, |oracle|) (the project's rss tolerance).
"""
import ctypes as C
import os

import numpy as np
import pytest

import bann_oracle as O
from helpers import build_context, f32_branch, norm_rel, x_std

pytestmark = pytest.mark.gpu
TOL = 1e-5

FX_SHAPES = [(60, [4, 4, 1], "tanh"), (256, [4, 1], "relu"), (300, [3, 4, 1], "silu"), (512, [4, 4, 4, 1], "tanh"),
             (17, [2, 3, 1], "leaky_relu"), (500, [4, 4, 1], "identity"), (129, [4, 4, 1], "tanh")]


@pytest.fixture(scope="module")
def Ctx():
    from bann import BannContext
    return BannContext


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """every context here is created with no BANN_* switch set (the split test sets its own)"""
    for k in [k for k in os.environ if k.startswith("BANN_") and k != "BANN_LIB"]:
        monkeypatch.delenv(k)


def make_specs(rng, n, shapes):
    g = O.synthetic_genotypes(rng, n, sum(m for m, _, _ in shapes))
    specs, off = [], 0
    for m, w, act in shapes:
        specs.append(dict(snps=np.arange(off, off + m, dtype=np.int32),
                          branch=f32_branch(O.random_branch(rng, m, w, act=act)), y=np.zeros(n), shape=(m, w, act)))
        off += m
    return g, specs


def draw_models(rng, specs, K):
    return [[f32_branch(O.random_branch(rng, *s["shape"][:2], act=s["shape"][2])) for s in specs] for _ in range(K)]


def pvec(br):
    return O.param_vec(br.weights, br.biases).astype(np.float32)


def fill_slots(ctx, models):
    ctx.models_reserve(len(models))
    for k, mod in enumerate(models):
        for b, br in enumerate(mod):
            ctx.models_set_params(k, b, pvec(br))


def std_blocks(ctx, g, specs):
    mu, sd = ctx.genotype_stats()
    return [x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]]) for s in specs]


def oracle_stats(mod, Xs, y):
    """(pop per branch, rss per branch) of one model in float64"""
    y64 = np.asarray(y, np.float64)
    pops = [O.population_effect_sizes([br], [X]) for br, X in zip(mod, Xs)]
    return pops, np.array([O.rss(br, X, y64) for br, X in zip(mod, Xs)])


def live_stats(ctx, mod, y):
    """the same through the live state: set_params, population_effect_sizes, the gradient launch's rss"""
    nb = len(mod)
    for b, br in enumerate(mod):
        ctx.set_params(b, pvec(br))
    ctx.set_target_all(y)
    pop = ctx.population_effect_sizes(list(range(nb)))
    _, rss = ctx.log_density_gradient_many(list(range(nb)))
    return pop, rss


def check_against(tag, pop_row, rss_row, ms, ref_pops, ref_rss):
    at = 0
    for b, m in enumerate(ms):
        err = norm_rel(pop_row[at:at + m], ref_pops[b])
        print(f"{tag} branch {b}: pop norm-rel {err:.3e}, rss {rss_row[b]:.9g} vs {ref_rss[b]:.9g}")
        assert err < TOL, (tag, b, err)
        assert abs(rss_row[b] - ref_rss[b]) <= TOL * max(1.0, abs(ref_rss[b])), (tag, b, rss_row[b], ref_rss[b])
        at += m


def split_pop(pop, ms):
    return np.split(np.asarray(pop), np.cumsum(ms)[:-1])


@pytest.mark.parametrize("n", [65, 1000, 4093])
def test_fx_parity(Ctx, n):
    """the seven fx shapes (one to eight chunks, m = 500: unstreamed padding rows, 2 to 4 layers, every
    activation) at n = 65 (one full tile and one row), 1000 and 4093 (ragged last tile); K = 5, 1,
    KS + 1 and 2 KS for the statistics pass width KS: every model's pop and rss against the oracle
    and against the live path.  At n = 65 and 4093 additionally with y = 100 + normal, so that
    out - y is large on every row: a pass that counted the padding rows of the last tile would add
    ~1e4 per row to the rss."""
    rng = np.random.default_rng(100 + n)
    g, specs = make_specs(rng, n, FX_SHAPES)
    nb, ms = len(specs), [s["shape"][0] for s in specs]
    ctx = build_context(Ctx, g, specs)
    assert all(ctx.kernel_path(b) == "fused" for b in range(nb))
    Xs = std_blocks(ctx, g, specs)
    KS = ctx.models_stats_pass_width()
    assert KS >= 1
    Ks = (5, 1, KS + 1, 2 * KS)
    models = draw_models(rng, specs, max(Ks))
    ys = [rng.normal(size=n).astype(np.float32)]
    if n != 1000:
        ys.append((100.0 + rng.normal(size=n)).astype(np.float32))
    for yi, y in enumerate(ys):
        refs = [oracle_stats(mod, Xs, y) for mod in models]
        lives = [live_stats(ctx, mod, y) for mod in models]
        for K in (Ks if yi == 0 else (KS + 1,)):
            fill_slots(ctx, models[:K])
            st = ctx.models_branch_stats(y=y)
            assert st["rss"].shape == (K, nb) and st["pop"].shape == (K, sum(ms))
            for k in range(K):
                check_against(f"n={n} y{yi} K={K} model {k} oracle", st["pop"][k], st["rss"][k], ms, *refs[k])
                check_against(f"n={n} y{yi} K={K} model {k} live", st["pop"][k], st["rss"][k], ms,
                              split_pop(lives[k][0], ms), lives[k][1])
    ctx.close()


def test_pass_independence_and_determinism(Ctx):
    """row k of a whole-chain call is bitwise the single-slot call (k, 1)'s -- a model's numbers do
    not depend on which models share its pass -- and two identical calls are bitwise equal; pop
    alone (no y) and rss alone give the same bits as the combined call"""
    rng = np.random.default_rng(7)
    n = 1000
    g, specs = make_specs(rng, n, [(60, [4, 4, 1], "tanh"), (300, [3, 4, 1], "silu"), (512, [4, 1], "relu")])
    ctx = build_context(Ctx, g, specs)
    K = 2 * ctx.models_stats_pass_width() + 1
    fill_slots(ctx, draw_models(rng, specs, K))
    y = rng.normal(size=n).astype(np.float32)
    a = ctx.models_branch_stats(y=y)
    b = ctx.models_branch_stats(y=y)
    assert np.array_equal(a["rss"], b["rss"]) and np.array_equal(a["pop"], b["pop"])
    for k in range(K):
        one = ctx.models_branch_stats(k, 1, y=y)
        assert np.array_equal(one["rss"][0], a["rss"][k]) and np.array_equal(one["pop"][0], a["pop"][k]), k
    assert np.array_equal(ctx.models_branch_stats()["pop"], a["pop"])
    only = ctx.models_branch_stats(y=y, pop=False)
    assert set(only) == {"rss"} and np.array_equal(only["rss"], a["rss"])
    assert len({r.tobytes() for r in a["pop"]}) == K
    ctx.close()


def test_split_items(Ctx, monkeypatch):
    """every branch split over several work items.  No public accessor reports the split, so the
    context is created with BANN_TARGET_ITEMS=1024, BANN_MIN_FRAGS=16 and BANN_SOLO=0 at n = 4093:
    with either of the first two set the fx split is ceil(nfrag / max(min_frags, ceil(total frags /
    target items))) = ceil(256 / 16) = 16 items per branch (branch_splits, finalize_layout.h), and
    BANN_SOLO=0 keeps the plan from being re-split.  The items' records are folded in item order."""
    for k, v in (("BANN_TARGET_ITEMS", "1024"), ("BANN_MIN_FRAGS", "16"), ("BANN_SOLO", "0")):
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(31)
    n = 4093
    g, specs = make_specs(rng, n, [(300, [3, 4, 1], "silu"), (129, [4, 4, 1], "tanh")])
    ms = [s["shape"][0] for s in specs]
    ctx = build_context(Ctx, g, specs)
    assert all(ctx.kernel_path(b) == "fused" for b in range(2))
    Xs = std_blocks(ctx, g, specs)
    models = draw_models(rng, specs, 3)
    y = (100.0 + rng.normal(size=n)).astype(np.float32)
    fill_slots(ctx, models)
    st = ctx.models_branch_stats(y=y)
    for k, mod in enumerate(models):
        check_against(f"split model {k} oracle", st["pop"][k], st["rss"][k], ms, *oracle_stats(mod, Xs, y))
    ctx.close()


def test_every_kernel_path(Ctx):
    """one fx, one fxl (m = 700), one wx and one gx branch, K = 3, n = 1000: oracle and live parity,
    and a permuted branch list returns the same numbers in list order"""
    rng = np.random.default_rng(11)
    n = 1000
    shapes = [(60, [4, 4, 1], "tanh"), (700, [4, 3, 1], "relu"), (40, [8, 8, 1], "silu"), (90, [45, 45, 1], "tanh")]
    g, specs = make_specs(rng, n, shapes)
    ms = [s["shape"][0] for s in specs]
    ctx = build_context(Ctx, g, specs)
    assert [ctx.kernel_path(b) for b in range(4)] == ["fused", "fused_large", "wide", "layered"]
    Xs = std_blocks(ctx, g, specs)
    models = draw_models(rng, specs, 3)
    y = rng.normal(size=n).astype(np.float32)
    lives = [live_stats(ctx, mod, y) for mod in models]
    fill_slots(ctx, models)
    st = ctx.models_branch_stats(y=y)
    order = [2, 0, 3, 1]
    pm = ctx.models_branch_stats(branches=order, y=y)
    for k, mod in enumerate(models):
        check_against(f"paths model {k} oracle", st["pop"][k], st["rss"][k], ms, *oracle_stats(mod, Xs, y))
        check_against(f"paths model {k} live", st["pop"][k], st["rss"][k], ms, split_pop(lives[k][0], ms), lives[k][1])
        parts = split_pop(st["pop"][k], ms)
        assert np.array_equal(pm["pop"][k], np.concatenate([parts[b] for b in order])), k
        assert np.array_equal(pm["rss"][k], st["rss"][k][order]), k
    ctx.close()


def test_live_state_untouched(Ctx):
    """two identical contexts; one fills slots with other parameters and takes the statistics.
    get_params and predict_many are what they were, and the same hmc_step (injected eps, momentum
    and u) then gives the same statuses, traces, parameters and predictions on both, bit for bit."""
    rng = np.random.default_rng(19)
    n, L = 1000, 4
    shapes = [(60, [4, 4, 1], "tanh"), (300, [3, 4, 1], "silu"), (40, [8, 8, 1], "tanh")]
    g, specs = make_specs(rng, n, shapes)
    for s in specs:
        s["y"] = rng.normal(size=n).astype(np.float32)
    nb = len(specs)
    a, b_ = build_context(Ctx, g, specs), build_context(Ctx, g, specs)
    eps = np.concatenate([(1e-3 * rng.uniform(0.5, 1.5, size=s["branch"].num_params)) for s in specs]).astype(np.float32)
    mom = np.concatenate([rng.normal(size=s["branch"].num_params) for s in specs]).astype(np.float32)
    u = rng.uniform(size=nb).astype(np.float32)
    par0 = [a.get_params(b) for b in range(nb)]
    pred0 = a.predict_many(list(range(nb)))
    fill_slots(a, draw_models(rng, specs, 3))
    st = a.models_branch_stats(y=rng.normal(size=n).astype(np.float32), moments=True)
    assert np.isfinite(st["rss"]).all() and np.isfinite(st["pop"]).all()
    for b in range(nb):
        assert np.array_equal(a.get_params(b), par0[b]), b
    assert np.array_equal(a.predict_many(list(range(nb))), pred0)
    assert np.array_equal(pred0, b_.predict_many(list(range(nb))))
    ra = a.hmc_step(list(range(nb)), L, 10.0, eps=eps, momentum=mom, u=u)
    rb = b_.hmc_step(list(range(nb)), L, 10.0, eps=eps, momentum=mom, u=u)
    assert np.array_equal(ra["status"], rb["status"])
    assert np.array_equal(ra["trace"], rb["trace"])
    for b in range(nb):
        assert np.array_equal(a.get_params(b), b_.get_params(b)), b
    assert np.array_equal(a.predict_many(list(range(nb))), b_.predict_many(list(range(nb))))
    a.close()
    b_.close()


def test_errors(Ctx):
    """every refusal returns its documented code and leaves the outputs (pre-filled with a
    sentinel) untouched"""
    E_STATE, E_ARG = -4, -5
    rng = np.random.default_rng(29)
    n = 1000
    g, specs = make_specs(rng, n, [(60, [4, 4, 1], "tanh"), (40, [4, 1], "tanh")])
    ctx = build_context(Ctx, g, specs)
    models = draw_models(rng, specs, 2)
    y = rng.normal(size=n).astype(np.float32)
    summ = 100
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def call(k0, nk, branches, with_y=True, with_rss=True):
        bl = np.asarray(branches, np.int32)
        rss = np.full((4, 2), 7.0, np.float64)
        pop = np.full((4, summ), 7.0, np.float32)
        mean, var = np.full(summ, 7.0, np.float32), np.full(summ, 7.0, np.float32)
        rc = ctx._lib.bann_models_branch_stats(ctx._h, k0, nk, bl.ctypes.data_as(ip), bl.size,
                                               y.ctypes.data_as(fp) if with_y else None,
                                               rss.ctypes.data_as(dp) if with_rss else None, pop.ctypes.data_as(fp),
                                               mean.ctypes.data_as(fp), var.ctypes.data_as(fp))
        untouched = all(np.all(a == 7.0) for a in (rss, pop, mean, var))
        return rc, untouched

    assert call(0, 1, [0, 1]) == (E_ARG, True)          # no bank reserved: the range is empty
    ctx.models_reserve(2)
    ctx.models_set_params(0, 0, pvec(models[0][0]))
    assert call(0, 1, [0, 1]) == (E_STATE, True)        # slot 0: branch 1 never set
    assert call(0, 1, [0])[0] == 0                      # ... but branch 0 alone is served
    fill_slots(ctx, models)
    assert call(1, 2, [0, 1]) == (E_ARG, True)          # slot range past the capacity
    assert call(-1, 1, [0, 1]) == (E_ARG, True)
    assert call(0, 0, [0, 1]) == (E_ARG, True)
    assert call(0, 2, [1, 1]) == (E_ARG, True)          # duplicate branch
    assert call(0, 2, [0, 2]) == (E_ARG, True)          # branch out of range
    assert call(0, 2, [0, 1], with_rss=False) == (E_ARG, True)   # y without rss
    assert call(0, 2, [0, 1], with_y=False) == (E_ARG, True)     # rss without y
    ctx.leapfrog_begin([0, 1], 3)
    assert call(0, 2, [0, 1]) == (E_STATE, True)        # inside a leapfrog session
    ctx.leapfrog_steps(3)
    ctx.leapfrog_end()
    rc, untouched = call(0, 2, [0, 1])
    assert rc == 0 and not untouched
    ctx.close()


def test_moments(Ctx):
    """pop_mean / pop_var: numpy's f64 mean and var(ddof = 1) of the returned rows rounded to f32
    (f64 accumulation, two-pass variance); exactly the row and 0 for K = 1"""
    rng = np.random.default_rng(23)
    n = 1000
    g, specs = make_specs(rng, n, [(60, [4, 4, 1], "tanh"), (129, [4, 4, 1], "relu"), (40, [8, 8, 1], "tanh")])
    ctx = build_context(Ctx, g, specs)
    fill_slots(ctx, draw_models(rng, specs, 6))
    st = ctx.models_branch_stats(moments=True)
    p64 = st["pop"].astype(np.float64)
    assert np.allclose(st["pop_mean"], p64.mean(axis=0), rtol=1e-6, atol=1e-12)
    assert np.allclose(st["pop_var"], p64.var(axis=0, ddof=1), rtol=1e-6, atol=1e-12)
    assert st["pop_var"].max() > 0
    one = ctx.models_branch_stats(4, 1, moments=True)
    assert np.array_equal(one["pop"][0], st["pop"][4]) and np.array_equal(one["pop_mean"], st["pop"][4])
    assert np.all(one["pop_var"] == 0)
    ctx.close()
