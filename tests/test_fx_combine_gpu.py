"""Z0 from the forward's digit sums combined in pairs (csrc/fx_combine.h, fx_z0_cum in fe_util.h):
every kernel that computes an fx-shaped branch's first-layer input -- k_fused_grad_fx, k_forward_fx,
k_forward_fi, fe_head of the model chain -- against the float64 oracle and against each other, and the
fx gradient's delta0 scale test as float compares.

Shapes (contexts built with BANN_TARGET_ITEMS=1 and BANN_SOLO=0, so a branch is one work item whose
four waves take tiles w, w + 4, ...):
  n = 64    one full tile            m = 1     one marker
  n = 200   a partial last tile      m = 64    one chunk exactly
  n = 1100  18 tiles: the waves run  m = 70    a partial second chunk
            3/2/2/2 steady tiles     m = 500   the benchmark's shape (padding rows, 8 chunks)
                                     m = 512   eight full chunks
crossed with 2, 3 and 4 layers, tanh and ReLU, in contexts of one and of three branches.  Tolerances are
the parity suite's (tests/test_gpu_parity.py): norm-relative 1e-5, rss 1e-5 relative.

Targets.  With one marker a branch's output takes three values, one per genotype, so the float32
rounding of the forward is the same for every individual of a genotype class and adds up linearly in n.
A target drawn around the model's own prediction leaves a residual of independent noise, whose sums grow
as sqrt(n) only: against the float64 oracle ANY float32 evaluation of such a problem is off by about
sqrt(n) 2^-24 |f| / |noise| per class.  A plain numpy float32 evaluation of the oracle's own formulas
misses 1e-5 there (m = 1: 1.1e-5, 3.8e-5 and 1.7e-5 at n = 64, 200, 1100; this library and its parent
alike measured 1.39e-5 and 2.26e-5 at n = 200 and 1100), while from m = 64 on it stays below 2e-7.  The
targets are therefore drawn independently of the model, standard normal as in the parity suite; the
same numpy float32 evaluation is then within 6e-7 of float64 (m = 1, 64 and 500 at each n), which leaves
the 1e-5 bound to the kernels.  Measured on an MI355X with these targets, worst gradient of a case: 2.9e-6
at m = 1, 5.4e-7 at m = 64 and 70, 9.4e-8 at m = 500 and 512.
"""
import numpy as np
import pytest

import bann_oracle as O
from helpers import build_context, f32_branch, norm_rel, x_std

pytestmark = pytest.mark.gpu

TOL = 1e-5
NS = [64, 200, 1100]
MS = [1, 64, 70, 500, 512]
CONFIGS = [(w, act) for w in ([4, 1], [4, 4, 1], [4, 4, 4, 1]) for act in ("tanh", "relu")]


@pytest.fixture(scope="module")
def Ctx():
    from bann import BannContext
    return BannContext


def scalar_close(a, b, tol=TOL):
    return abs(a - b) <= tol * max(1.0, abs(b))


def one_item_env(monkeypatch):
    monkeypatch.setenv("BANN_TARGET_ITEMS", "1")
    monkeypatch.setenv("BANN_SOLO", "0")


def oracle_of(ctx, g, specs, rng, y_of=None):
    """targets (set in the specs) and the oracle's predictions, gradients and rss at the device's own
    standardisation constants.  The targets are drawn independently of the model (standard normal, as in
    the parity suite), not around its predictions: see the module docstring"""
    mu, sd = ctx.genotype_stats()
    ref = []
    for s in specs:
        X = x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]])
        f = O.predict(s["branch"], X)
        y = rng.normal(size=f.size)
        if y_of is not None:
            y = y_of(y)
        s["y"] = y.astype(np.float32).astype(np.float64)
        gw, gb, rss = O.log_density_gradient(s["branch"], X, s["y"])
        ref.append(dict(f=f, grad=O.param_vec(gw, gb), rss=rss, X=X))
    return ref


def check_against(ctx, branches, ref):
    grads, rss = ctx.log_density_gradient_many(branches)
    preds = ctx.predict_many(branches)
    for i, r in enumerate(ref):
        e = norm_rel(grads[i], r["grad"])
        print(f"branch {branches[i]}: gradient norm-rel {e:.2e}, prediction norm-rel {norm_rel(preds[i], r['f']):.2e}")
        assert e < TOL, (i, e)
        assert scalar_close(rss[i], r["rss"]), (i, rss[i], r["rss"])
        assert norm_rel(preds[i], r["f"]) < TOL, i
    return grads, rss, preds


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_gradient_and_predictions_match_oracle(Ctx, monkeypatch, n, m):
    one_item_env(monkeypatch)
    rng = np.random.default_rng(7000 * n + m)
    M = m + 5
    g = O.synthetic_genotypes(rng, n, M)
    for widths, act in CONFIGS:
        specs = [dict(snps=rng.permutation(M)[:m].astype(np.int32),
                      branch=f32_branch(O.random_branch(rng, m, widths, prior="ridge_ard", act=act)), y=np.zeros(n))
                 for _ in range(3)]
        ctx = build_context(Ctx, g, specs)
        assert all(ctx.kernel_path(b) == "fused" for b in range(3))
        ref = oracle_of(ctx, g, specs, rng)
        for b, s in enumerate(specs):
            ctx.set_target(b, s["y"])
        check_against(ctx, [0, 1, 2], ref)
        ctx.close()
        ctx = build_context(Ctx, g, specs[:1])  # the first branch alone in a context of its own
        check_against(ctx, [0], ref[:1])
        ctx.close()


def test_saturated_digit_sums_z0(Ctx, monkeypatch):
    """every digit sum at its largest: m = 512, every genotype 2 (standardisation set to mu = 0, sigma = 1,
    so x = 2), W0 constant per column at just under 127 column-scale units, so every marker's top digit is
    127.  Two layers with the identity activation and a one-hot output weight make the prediction of
    branch j column j of Z0."""
    one_item_env(monkeypatch)
    n, m = 128, 512
    g = np.full((m, n), 2, dtype=np.int8)
    col = np.array([126.9 * 2.0 ** -9, -126.9 * 2.0 ** -7, 126.6 * 2.0 ** -9, -126.51 * 2.0 ** -8])
    b0 = np.array([0.25, -1.5, 0.0, 3.0])
    rng = np.random.default_rng(5)
    specs = []
    for j in range(4):
        br = O.random_branch(rng, m, [4, 1], prior="ridge_ard", act="identity")
        br.weights[0] = np.tile(col[None, :], (m, 1))
        br.biases[0] = b0.copy()
        br.weights[1] = np.zeros((4, 1))
        br.weights[1][j, 0] = 1.0
        specs.append(dict(snps=np.arange(m, dtype=np.int32), branch=f32_branch(br), y=np.zeros(n)))
    for fi in ("0", "1"):
        monkeypatch.setenv("BANN_FWD_FI", fi)
        ctx = build_context(Ctx, g, specs, stats=(np.zeros(m), np.ones(m)))
        assert all(ctx.kernel_path(b) == "fused" for b in range(4))
        preds = ctx.predict_many([0, 1, 2, 3])
        X = np.full((n, m), 2.0)
        for j, s in enumerate(specs):
            z0 = O.forward_feed(s["branch"], X)[0][0][:, j]
            print(f"fi={fi} column {j}: Z0 {preds[j][0]!r} oracle {z0[0]!r}")
            assert norm_rel(preds[j], z0) < TOL, (fi, j, preds[j][:2], z0[:2])
            # the gradient launch's own forward: rss against a zero target is sum Z0^2
            _, rss = ctx.log_density_gradient(j)
            assert scalar_close(rss, float(np.sum(z0 * z0))), (fi, j, rss)
        ctx.close()


def test_every_path_gives_the_same_prediction_bits(Ctx, monkeypatch):
    """the same branches through k_fused_grad_fx (the prediction rows a trajectory's gradient launches
    leave; zero step sizes keep the parameters where they are), predict_many over the LDS forward
    (k_forward_fx) and over the individual-major image (k_forward_fi), and a one-model chain (fe_head)"""
    one_item_env(monkeypatch)
    rng = np.random.default_rng(11)
    n = 1100
    shapes = [(500, [4, 4, 1], "tanh"), (70, [4, 4, 4, 1], "relu"), (512, [4, 1], "tanh")]
    g = O.synthetic_genotypes(rng, n, sum(m for m, _, _ in shapes))
    specs, off = [], 0
    for m, w, act in shapes:
        specs.append(dict(snps=np.arange(off, off + m, dtype=np.int32),
                          branch=f32_branch(O.random_branch(rng, m, w, act=act)),
                          y=rng.normal(size=n).astype(np.float32)))
        off += m
    nb = len(specs)
    rows = {}
    for fi in ("0", "1"):
        monkeypatch.setenv("BANN_FWD_FI", fi)
        ctx = build_context(Ctx, g, specs)
        assert all(ctx.kernel_path(b) == "fused" for b in range(nb))
        rows["forward fi=" + fi] = ctx.predict_many(list(range(nb)))
        if fi == "0":
            P = [ctx.get_params(b) for b in range(nb)]
            res = ctx.hmc_step(list(range(nb)), 2, 10.0, eps=np.zeros(sum(p.size for p in P), np.float32),
                               momentum=np.concatenate([rng.normal(size=p.size).astype(np.float32) for p in P]),
                               u=[0.5] * nb)
            print("statuses", res["status"])  # accepted or not, the parameters are the initial ones
            assert all(np.array_equal(ctx.get_params(b), P[b]) for b in range(nb))
            rows["trajectory"] = np.stack([ctx.predict(b) for b in range(nb)])
            ctx.models_reserve(1)
            for b in range(nb):
                ctx.models_set_params(0, b, P[b])
            ctx.models_set_bias(0, 0.0)
            rows["chain"] = ctx.models_branch_predictions(0, list(range(nb)))
        ctx.close()
    mu_ref = rows["forward fi=0"]
    assert np.all(np.isfinite(mu_ref)) and float(np.std(mu_ref)) > 0
    for name, r in rows.items():
        assert np.array_equal(r, mu_ref), name


def test_scale_growth_in_a_later_tile(Ctx, monkeypatch):
    """targets 2^10 times larger from individual 64 on: wave 0 sets its delta0 scale on tile 0 and has to
    grow it on its next tile (the float threshold compare sends it down the rare path, which rescales the
    digit sums it has).  The gradient matches the oracle, and the packed launch the single one bit for bit."""
    one_item_env(monkeypatch)
    rng = np.random.default_rng(13)
    n, m, nb = 1100, 500, 3
    g = O.synthetic_genotypes(rng, n, nb * m)
    specs = [dict(snps=np.arange(b * m, (b + 1) * m, dtype=np.int32),
                  branch=f32_branch(O.random_branch(rng, m, [4, 4, 1], prior="ridge_ard", act="tanh")), y=np.zeros(n))
             for b in range(nb)]
    ctx = build_context(Ctx, g, specs)

    def grown(y):
        y = y.copy()
        y[64:] *= 1024.0
        return y

    ref = oracle_of(ctx, g, specs, rng, y_of=grown)
    for b, s in enumerate(specs):
        ctx.set_target(b, s["y"])
    grads, rss = ctx.log_density_gradient_many(list(range(nb)))
    for b in range(nb):
        e = norm_rel(grads[b], ref[b]["grad"])
        print(f"branch {b}: gradient norm-rel {e:.2e}")
        assert e < TOL, (b, e)
        assert scalar_close(rss[b], ref[b]["rss"]), (b, rss[b], ref[b]["rss"])
        g1, r1 = ctx.log_density_gradient(b)
        assert np.array_equal(g1, grads[b]) and r1 == rss[b], b
    ctx.close()


def test_wide_item_keeps_the_four_digit_combine(Ctx):
    """an fxl-shaped branch (m = 600: 10 chunks, outside the pair combine's bound) still matches the oracle"""
    rng = np.random.default_rng(17)
    n, m = 200, 600
    g = O.synthetic_genotypes(rng, n, m)
    specs = [dict(snps=np.arange(m, dtype=np.int32),
                  branch=f32_branch(O.random_branch(rng, m, [4, 3, 1], prior="ridge_ard", act="tanh")), y=np.zeros(n))]
    ctx = build_context(Ctx, g, specs)
    assert ctx.kernel_path(0) == "fused_large"
    ref = oracle_of(ctx, g, specs, rng)
    ctx.set_target(0, specs[0]["y"])
    check_against(ctx, [0], ref)
    ctx.close()
