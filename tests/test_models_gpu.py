"""GPU tests of the model slots (bann_models_*): a chain of saved models predicted
from one genotype pass.

The slots hold K parameter sets beside the live one.  The multi-model forward
(kernels_fe.hip) must write, for every model and fx branch, the bits the
single-model forward (k_forward_fx) writes for the same parameters; the other
kernel paths run their own forward launches on the slot state; the device sum is
Net::predict's f32 order (0 + bias, then += f_b in branch order).  References:
the live path of the same context (bitwise) and the float64 oracle (norm-relative
1e-5, the bound the same inputs meet through predict_many in
test_gpu_parity.py::test_forward_fi_matches_lds_forward).
"""
import os

import numpy as np
import pytest

import bann_oracle as O
from helpers import build_context, f32_branch, norm_rel, x_std

pytestmark = pytest.mark.gpu

FX_SHAPES = [(60, [4, 4, 1], "tanh"), (256, [4, 1], "relu"), (300, [3, 4, 1], "silu"), (512, [4, 4, 4, 1], "tanh"),
             (17, [2, 3, 1], "leaky_relu"), (500, [4, 4, 1], "identity"), (129, [4, 4, 1], "tanh")]


@pytest.fixture(scope="module")
def Ctx():
    from bann import BannContext
    return BannContext


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """every context here is created with no BANN_* switch set"""
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
    """K seeded parameter sets per branch (oracle branches, f32-rounded) and K biases"""
    models = [[f32_branch(O.random_branch(rng, *s["shape"][:2], act=s["shape"][2])) for s in specs] for _ in range(K)]
    bias = rng.normal(scale=0.3, size=K).astype(np.float32)
    return models, bias


def pvec(br):
    return O.param_vec(br.weights, br.biases).astype(np.float32)


def fill_slots(ctx, models, bias):
    ctx.models_reserve(len(models))
    assert ctx.models_capacity() == len(models)
    for k, mod in enumerate(models):
        for b, br in enumerate(mod):
            ctx.models_set_params(k, b, pvec(br))
        ctx.models_set_bias(k, bias[k])


def host_sum(rows, bias):
    """Net::predict's order in f32: 0 + bias, then += the rows in branch order"""
    v = np.full(rows.shape[1], np.float32(0.0) + np.float32(bias), np.float32)
    for r in rows:
        v = (v + r).astype(np.float32)
    return v


def live_rows(ctx, mod):
    """the live path's rows for one model: set every branch's parameters, predict_many"""
    for b, br in enumerate(mod):
        ctx.set_params(b, pvec(br))
    return ctx.predict_many(list(range(len(mod))))


@pytest.mark.parametrize("n", [1000, 4093])
def test_fx_shapes_bitwise(Ctx, n):
    """the seven fx shapes of test_forward_fi_matches_lds_forward (one and two 256-marker segments,
    2 to 4 layers, every activation; n = 4093: a ragged last tile), K = 5 (two passes, the second
    short) and K = 1: per model the per-branch rows are the live forward's bits, the summed row is
    the host f32 sum's bits and within 1e-5 of the oracle."""
    rng = np.random.default_rng(n)
    g, specs = make_specs(rng, n, FX_SHAPES)
    nb = len(specs)
    ctx = build_context(Ctx, g, specs)
    assert all(ctx.kernel_path(b) == "fused" for b in range(nb))
    mu, sd = ctx.genotype_stats()
    Xs = [x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]]) for s in specs]
    models, bias = draw_models(rng, specs, 5)
    for K in (5, 1):
        fill_slots(ctx, models[:K], bias[:K])
        yh = ctx.models_predict()
        assert yh.shape == (K, n)
        for k in range(K):
            live = live_rows(ctx, models[k])
            assert np.array_equal(ctx.models_branch_predictions(k, list(range(nb))), live), (K, k)
            assert np.array_equal(yh[k], host_sum(live, bias[k])), (K, k)
            ref = sum(O.predict(br, X) for br, X in zip(models[k], Xs)) + float(bias[k])
            err = norm_rel(yh[k], ref)
            print(f"n={n} K={K} model {k}: norm-rel error vs oracle {err:.3e}")
            assert err < 1e-5, (K, k, err)
        if K == 5:
            assert np.array_equal(ctx.models_predict(2, 2), yh[2:4])
            sub = ctx.models_branch_predictions(3, [5, 1, 3])  # another plan: other work items
            assert np.array_equal(sub, ctx.models_branch_predictions(3, list(range(nb)))[[5, 1, 3]])
    ctx.close()


def test_ragged_passes(Ctx):
    """K = KM + 1 and K = 2 KM for the shipped models-per-pass KM: every row of the whole call
    is bitwise the single-slot call's"""
    rng = np.random.default_rng(7)
    n = 1000
    g, specs = make_specs(rng, n, [(60, [4, 4, 1], "tanh"), (300, [3, 4, 1], "silu"), (512, [4, 1], "relu")])
    ctx = build_context(Ctx, g, specs)
    KM = ctx.models_pass_width()
    assert KM >= 1
    models, bias = draw_models(rng, specs, 2 * KM)
    for K in (KM + 1, 2 * KM):
        fill_slots(ctx, models[:K], bias[:K])
        yh = ctx.models_predict()
        for k in range(K):
            assert np.array_equal(ctx.models_predict(k, 1)[0], yh[k]), (K, k)
    ctx.close()


def test_every_kernel_path(Ctx):
    """one branch each on the fx, fxl, wx and gx paths, K = 3: every row is bitwise the
    bann_net_predict-style sum of the live predict_many rows and within 1e-5 of the oracle"""
    rng = np.random.default_rng(11)
    n = 1000
    shapes = [(60, [4, 4, 1], "tanh"), (600, [4, 4, 1], "tanh"), (40, [8, 8, 1], "tanh"), (30, [6, 5, 3, 1], "tanh")]
    g, specs = make_specs(rng, n, shapes)
    ctx = build_context(Ctx, g, specs)
    assert [ctx.kernel_path(b) for b in range(4)] == ["fused", "fused_large", "wide", "layered"]
    mu, sd = ctx.genotype_stats()
    Xs = [x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]]) for s in specs]
    models, bias = draw_models(rng, specs, 3)
    fill_slots(ctx, models, bias)
    yh = ctx.models_predict()
    for k in range(3):
        live = live_rows(ctx, models[k])
        assert np.array_equal(ctx.models_branch_predictions(k, [0, 1, 2, 3]), live), k
        assert np.array_equal(yh[k], host_sum(live, bias[k])), k
        ref = sum(O.predict(br, X) for br, X in zip(models[k], Xs)) + float(bias[k])
        err = norm_rel(yh[k], ref)
        print(f"model {k}: norm-rel error vs oracle {err:.3e}")
        assert err < 1e-5, (k, err)
    ctx.close()


def test_live_state_untouched(Ctx):
    """two identical contexts; one reserves slots, fills them with other parameters and predicts.
    Its live parameters and prediction rows are what they were, and the same hmc_step then gives
    the same statuses, parameters and prediction rows on both, bit for bit."""
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
    pred0 = [a.predict(b) for b in range(nb)]
    models, bias = draw_models(rng, specs, 3)
    fill_slots(a, models, bias)
    yh = a.models_predict()
    assert np.isfinite(yh).all()
    for b in range(nb):
        assert np.array_equal(a.get_params(b), par0[b]), b
        assert np.array_equal(a.predict(b), pred0[b]), b
        assert np.array_equal(pred0[b], b_.predict(b)), b
    ra = a.hmc_step(list(range(nb)), L, 10.0, eps=eps, momentum=mom, u=u)
    rb = b_.hmc_step(list(range(nb)), L, 10.0, eps=eps, momentum=mom, u=u)
    assert np.array_equal(ra["status"], rb["status"])
    assert np.array_equal(ra["trace"], rb["trace"])
    for b in range(nb):
        assert np.array_equal(a.get_params(b), b_.get_params(b)), b
        assert np.array_equal(a.predict(b), b_.predict(b)), b
    assert np.array_equal(a.models_predict(), yh)   # and the slots are what they were
    a.close()
    b_.close()


def test_moments(Ctx):
    """mean and sample variance over the rows: f64 accumulation rounded to f32 once (2^-24
    relative), two-pass variance (no cancellation); exactly 0 for one row"""
    rng = np.random.default_rng(23)
    n = 1000
    g, specs = make_specs(rng, n, [(60, [4, 4, 1], "tanh"), (129, [4, 4, 1], "relu")])
    ctx = build_context(Ctx, g, specs)
    models, bias = draw_models(rng, specs, 6)
    fill_slots(ctx, models, bias)
    yh, mean, var = ctx.models_predict(moments=True)
    y64 = yh.astype(np.float64)
    assert np.allclose(mean, y64.mean(axis=0), rtol=1e-6, atol=1e-12)
    assert np.allclose(var, y64.var(axis=0, ddof=1), rtol=1e-6, atol=1e-12)
    assert var.min() > 0
    yh1, mean1, var1 = ctx.models_predict(4, 1, moments=True)
    assert np.array_equal(yh1[0], yh[4]) and np.array_equal(mean1, yh[4]) and np.all(var1 == 0)
    ctx.close()


def test_refusals(Ctx):
    from bann import BannError
    rng = np.random.default_rng(29)
    n = 1000
    g, specs = make_specs(rng, n, [(60, [4, 4, 1], "tanh"), (40, [4, 1], "tanh")])
    raw = Ctx(0)
    raw.upload_genotypes(g)
    raw.add_branch(specs[0]["snps"], [4, 4, 1])
    with pytest.raises(BannError):   # before finalize
        raw.models_reserve(2)
    raw.close()
    ctx = build_context(Ctx, g, specs)
    models, bias = draw_models(rng, specs, 2)
    ctx.models_reserve(2)
    with pytest.raises(BannError):   # slot >= capacity
        ctx.models_set_params(2, 0, pvec(models[0][0]))
    with pytest.raises(BannError):
        ctx.models_set_bias(2, 0.0)
    with pytest.raises(BannError):   # branch out of range
        ctx.models_set_params(0, 2, pvec(models[0][0]))
    ctx.models_set_params(0, 0, pvec(models[0][0]))
    with pytest.raises(BannError):   # slot 0: branch 1 never set
        ctx.models_predict(0, 1)
    with pytest.raises(BannError):
        ctx.models_branch_predictions(0, [1])
    with pytest.raises(BannError):   # range past the capacity
        ctx.models_predict(1, 2)
    fill_slots(ctx, models, bias)
    ctx.leapfrog_begin([0, 1], 3)
    for call in (lambda: ctx.models_reserve(3), lambda: ctx.models_set_params(0, 0, pvec(models[0][0])),
                 lambda: ctx.models_set_bias(0, 1.0), lambda: ctx.models_predict(),
                 lambda: ctx.models_branch_predictions(0, [0])):
        with pytest.raises(BannError):
            call()
    ctx.leapfrog_steps(3)
    ctx.leapfrog_end()
    assert ctx.models_predict().shape == (2, n)
    ctx.models_reserve(0)
    assert ctx.models_capacity() == 0
    with pytest.raises(BannError):
        ctx.models_predict(0, 1)
    assert ctx.predict_many([0, 1]).shape == (2, n)   # the context keeps working
    ctx.close()
