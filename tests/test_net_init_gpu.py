"""Starting a model on the device (kernels_init.hip: bann_init_branches, bann_net_init,
bann_net_simulate_y) against the numpy restatement of tests/init_reference.py, on the toy shapes of
tests/test_gibbs_gpu.py (n = 65; the init kernels read no genotypes) plus one std-normal branch at
context level:

| markers | widths       | prior      | exercises                                            |
| 1       | [1, 1]       | ridge_ard  | one marker: removed or kept as a whole               |
| 33      | [3, 1]       | ridge_ard  | two layers                                           |
| 70      | [4, 4, 1]    | ridge_ard  | more markers than a wavefront                        |
| 129     | [5, 3, 1]    | lasso_ard  | ARD precisions from squares for lasso too            |
| 700     | [4, 4, 1]    | ridge_base | three key tiles in the selection, whole-layer sums   |
| 40      | [8, 8, 1]    | lasso_base |                                                      |
| 30      | [6, 5, 3, 1] | lasso_ard  | two dense layers and a summary layer                 |
| 20      | [3, 2, 1]    | std_normal | context level only (a Net refuses it)                |
"""
import json
import math
import os

import numpy as np
import pytest

import init_reference as R

pytestmark = pytest.mark.gpu

N = 65
SPECS = [(1, [1, 1], "ridge_ard"), (33, [3, 1], "ridge_ard"), (70, [4, 4, 1], "ridge_ard"),
         (129, [5, 3, 1], "lasso_ard"), (700, [4, 4, 1], "ridge_base"), (40, [8, 8, 1], "lasso_base"),
         (30, [6, 5, 3, 1], "lasso_ard")]
STD = (20, [3, 2, 1], "std_normal")
EPS = 2.0 ** -23   # one f32 rounding of an f64 result (2^-24) with room for the order of the f64 sums
PLINK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plink")


def make_context(specs, n=N, seed=42):
    from bann import BannContext
    ctx = BannContext(0)
    ctx.synthetic_genotypes(n, sum(m for m, _, _ in specs), seed)
    off = 0
    for m, w, prior in specs:
        ctx.add_branch(np.arange(off, off + m, dtype=np.int32), w, "tanh", prior)
        off += m
    ctx.finalize()
    return ctx


def with_prior(prior):
    return [(m, w, prior if prior else p) for m, w, p in SPECS]


def state(ctx, nb):
    return [(ctx.get_params(b), ctx.get_precisions(b)) for b in range(nb)]


def refused(code, fn, *args, **kw):
    from bann import BannError
    with pytest.raises(BannError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


@pytest.fixture(scope="module")
def ctx():
    c = make_context(SPECS + [STD])
    yield c
    c.close()


def check_mask(ctx, b, m, widths, mask):
    th = ctx.get_params(b)
    w0 = th[: m * widths[0]].reshape(widths[0], m)
    assert np.array_equal(w0 != 0, np.broadcast_to(mask, w0.shape)), b   # a kept entry is never 0
    assert np.all(th[m * widths[0]:] != 0), b                            # no layer above 0 is touched


def test_keep_masks_exact_count(ctx):
    from bann import InitConfig
    for b, (m, w, _) in enumerate(SPECS + [STD]):
        for e in sorted({0, 1, m - 1, m}):
            ctx.init_branches(InitConfig(variance=1.0, num_effective=e, proportion_effective=0.5), seed=21, branches=[b])
            mask = R.keep_mask_exact(21, b, m, e)
            assert int(mask.sum()) == e
            check_mask(ctx, b, m, w, mask)   # the exact count takes precedence over the proportion


def test_keep_masks_proportion(ctx):
    from bann import InitConfig
    ctx.init_branches(InitConfig(variance=1.0, proportion_effective=0.25), seed=22)
    kept = 0
    for b, (m, w, _) in enumerate(SPECS + [STD]):
        mask = R.keep_mask_proportion(22, b, m, 0.25)
        kept += int(mask.sum())
        check_mask(ctx, b, m, w, mask)
    assert 0 < kept < sum(m for m, _, _ in SPECS + [STD])
    ctx.init_branches(InitConfig(variance=1.0, proportion_effective=1.0), seed=22)   # >= 1: every marker kept
    for b, (m, w, _) in enumerate(SPECS + [STD]):
        check_mask(ctx, b, m, w, np.ones(m, bool))


@pytest.mark.parametrize("cfg", [dict(), dict(variance=0.4, proportion_effective=0.25), dict(gamma=(2.5, 1.5)),
                                 dict(num_effective=0)])
def test_precisions(ctx, cfg):
    """every entry against the f64 formulas at the device's own theta; +inf exactly where the sum is
    zero (mode 0: every bias precision; a removed marker: its ARD row), never NaN"""
    from bann import InitConfig
    ctx.init_branches(InitConfig(**cfg), seed=31)
    worst, infs = 0.0, 0
    for b, (m, w, prior) in enumerate(SPECS + [STD]):
        th, q = ctx.get_params(b), ctx.get_precisions(b)
        ref = R.precisions(th, m, w, prior)
        assert q.shape == ref.shape and not np.any(np.isnan(q)), b
        assert np.array_equal(np.isinf(q), np.isinf(ref)) and np.all(q > 0), (b, q, ref)
        fin = np.isfinite(ref)
        err = np.max(np.abs(q[fin].astype(np.float64) - ref[fin]) / ref[fin])
        worst, infs = max(worst, err), infs + int((~fin).sum())
        assert err <= EPS, (b, err)
        L = len(w)
        if "variance" not in cfg and "gamma" not in cfg:          # mode 0: biases 0, their precisions +inf
            assert np.all(np.isinf(q[-L:-1])), b
        if prior in R.ARD and ("proportion_effective" in cfg or "num_effective" in cfg):
            removed = ~(R.keep_mask_proportion(31, b, m, 0.25) if "proportion_effective" in cfg else np.zeros(m, bool))
            assert np.array_equal(np.isinf(q[:m]), removed), b   # the removed markers' ARD rows
    print("worst relative error", worst, "infinite entries", infs)
    assert infs > 0 or "gamma" in cfg


def test_fixed_precision():
    from bann import InitConfig
    base = [(m, w, "lasso_base" if "lasso" in p else "ridge_base") for m, w, p in SPECS] + [STD]
    c = make_context(base)
    c.init_branches(InitConfig(fixed_precision=0.7), seed=4)
    for b in range(len(base)):
        assert np.all(c.get_precisions(b) == np.float32(0.7)), b
    c.close()


def test_refusals(ctx):
    from bann import BannContext, InitConfig
    nb = len(SPECS) + 1
    before = state(ctx, nb)
    refused(-5, ctx.init_branches, InitConfig(fixed_precision=0.7), 1)                  # ARD branches listed
    refused(-5, ctx.init_branches, InitConfig(fixed_precision=0.0), 1, branches=[4])
    refused(-5, ctx.init_branches, InitConfig(), 1, branches=[1, 2, 1])                 # duplicate
    refused(-5, ctx.init_branches, InitConfig(), 1, branches=[0, nb])                   # out of range
    refused(-5, ctx.init_branches, InitConfig(), 1, branches=[])                        # empty
    refused(-5, ctx.init_branches, InitConfig(variance=0.0), 1)
    refused(-5, ctx.init_branches, InitConfig(gamma=(2.0, -1.0)), 1)
    msg = refused(-5, ctx.init_branches, InitConfig(num_effective=34), 1, branches=[2, 1])   # m = 33
    assert "branch 1" in msg, msg
    for b, (p, q) in enumerate(before):                                                 # nothing was written
        assert np.array_equal(ctx.get_params(b), p) and np.array_equal(ctx.get_precisions(b), q, equal_nan=True), b
    c = BannContext(0)
    c.synthetic_genotypes(N, 20, 1)
    c.add_branch(np.arange(10, dtype=np.int32), [2, 1], "tanh", "ridge_ard")
    refused(-4, c.init_branches, InitConfig(), 1, branches=[0])                         # before finalize
    c.finalize()
    c.init_branches(InitConfig(variance=0.5), 1)
    c.set_target_all(np.zeros(N, np.float32))
    c.leapfrog_begin([0], 2, step_factor=0.01)                                          # inside a leapfrog session
    try:
        refused(-4, c.init_branches, InitConfig(variance=0.5), 1)
        c.leapfrog_steps(2)
    finally:
        c.leapfrog_end()
    c.close()


def test_consistent_with_the_setters():
    """mode 1 (every precision finite): a twin context that receives the read-back vectors through
    set_params / set_precisions gives bitwise equal predictions, gradients and Izmailov step sizes"""
    from bann import InitConfig
    specs = SPECS + [STD]
    nb = len(specs)
    a, t = make_context(specs), make_context(specs)
    y = np.random.default_rng(3).normal(size=N).astype(np.float32)
    a.init_branches(InitConfig(variance=0.25, num_effective=None), seed=17)
    for b in range(nb):
        q = a.get_precisions(b)
        assert np.all(np.isfinite(q)) and np.all(q > 0), b
        t.set_params(b, a.get_params(b))
        t.set_precisions(b, q)
    for c in (a, t):
        c.set_target_all(y)
    assert np.array_equal(a.predict_many(range(nb)), t.predict_many(range(nb)))
    ga, ra = a.log_density_gradient_many(range(nb))
    gt, rt = t.log_density_gradient_many(range(nb))
    assert np.array_equal(ra, rt)
    for b in range(nb):
        assert np.array_equal(ga[b], gt[b]), b
        assert a.log_density(b, float(ra[b])) == t.log_density(b, float(rt[b])), b
    mom = np.random.default_rng(5).normal(size=sum(a.num_params(b) for b in range(nb))).astype(np.float32)
    u = np.full(nb, 0.5, np.float32)
    ra_ = a.hmc_step(range(nb), 2, 10.0, step_mode="izmailov", step_factor=0.01, momentum=mom, u=u)
    rt_ = t.hmc_step(range(nb), 2, 10.0, step_mode="izmailov", step_factor=0.01, momentum=mom, u=u)
    # the std-normal branch's steps take no factor: its trajectory leaves the trace's range, alike on both
    assert np.array_equal(ra_["status"], rt_["status"]) and np.array_equal(ra_["trace"], rt_["trace"], equal_nan=True)
    for b in range(nb):
        ea, et = a.get_step_sizes(b), t.get_step_sizes(b)
        assert np.all(ea > 0) and np.array_equal(ea, et), b
        assert np.array_equal(a.get_params(b), t.get_params(b)), b
    # a later setter call on the initialised context behaves as on any other
    a.set_precisions(2, t.get_precisions(2))
    assert np.array_equal(a.log_density_gradient_many([2])[0][0], t.log_density_gradient_many([2])[0][0])
    a.close()
    t.close()


def same(s1, s2):
    return np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1], equal_nan=True)


def test_determinism_and_independence(ctx):
    from bann import InitConfig
    nb = len(SPECS) + 1
    cfg = InitConfig(proportion_effective=0.5)
    ctx.init_branches(cfg, seed=7)
    s1 = state(ctx, nb)
    ctx.init_branches(cfg, seed=7)
    s2 = state(ctx, nb)
    ctx.init_branches(cfg, seed=8)
    s3 = state(ctx, nb)
    for b in range(nb):
        assert same(s1[b], s2[b]), b                          # the same seed, the same bits
        assert not np.array_equal(s1[b][0], s3[b][0]), b      # another seed changes every branch
    ctx.init_branches(cfg, seed=7, branches=[5, 2])           # alone: their values from the call over all
    s4 = state(ctx, nb)
    for b in range(nb):
        assert same(s4[b], s1[b] if b in (2, 5) else s3[b]), b


def ks_normal(v, sd):
    x = np.sort(v) / (sd * math.sqrt(2.0))
    cdf = 0.5 * (1.0 + np.array([math.erf(t) for t in x]))
    n = v.size
    return max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))


@pytest.mark.parametrize("cfg,var", [(dict(), 1.0 / 700.0), (dict(variance=0.37), 0.37),
                                     (dict(gamma=(2.5, 1.5)), 1.0 / (2.5 * 1.5))])
def test_distribution(ctx, cfg, var):
    """layer 0 of the 700 x 4 branch over 64 seeds: 179 200 draws, mean and variance at five standard
    errors, the Kolmogorov-Smirnov statistic against N(0, var) below 1.95 / sqrt(N)"""
    from bann import InitConfig
    var = float(np.float32(var)) if cfg else float(np.float32(1.0) / np.float32(700.0))
    pool = []
    for seed in range(2000, 2064):
        ctx.init_branches(InitConfig(**cfg), seed=seed, branches=[4])
        pool.append(ctx.get_params(4)[:2800].astype(np.float64))
    v = np.concatenate(pool)
    n = v.size
    assert n == 179200 and np.all(np.isfinite(v)) and np.all(v != 0)
    mean, s2, ks = float(np.mean(v)), float(np.var(v, ddof=1)), ks_normal(v, math.sqrt(var))
    print(f"var {var:.6g} N {n} mean {mean:.3e} var {s2:.6g} KS {ks:.5f} (bound {1.95 / math.sqrt(n):.5f})")
    assert abs(mean) <= 5.0 * math.sqrt(var / n)
    assert abs(s2 - var) <= 5.0 * var * math.sqrt(2.0 / (n - 1))
    assert ks < 1.95 / math.sqrt(n)


@pytest.mark.parametrize("prior", [None, "ridge_base", "lasso_ard"])
def test_output_precision_and_globals(prior):
    from bann import InitConfig, Net
    specs = with_prior(prior)
    nb = len(specs)
    c = make_context(specs)
    net = Net(c, seed=1)
    net.init(InitConfig(), seed=9)
    th = [c.get_params(b) for b in range(nb)]
    ms, ws = [m for m, _, _ in specs], [w for _, w, _ in specs]
    jp = R.joint_output_precision(th, ms, ws)
    got = [c.get_precisions(b)[R.out_precision_index(m, w, p)] for b, (m, w, p) in enumerate(specs)]
    assert len(set(float(g) for g in got)) == 1, got                    # identical in every branch
    assert abs(float(got[0]) - jp) / jp <= EPS, (got[0], jp)
    for b, (m, w, p) in enumerate(specs):                               # the other entries are the branch's own
        ref = R.precisions(th[b], m, w, p)
        ref[R.out_precision_index(m, w, p)] = got[0]
        q = c.get_precisions(b)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isinf(q), ~fin) and np.max(np.abs(q[fin] - ref[fin]) / ref[fin]) <= EPS, b
    s = net.summary()
    assert s["error_precision"] == 2.0 and s["output_layer_precision"] == np.float32(0.05) and s["output_bias"] == 0.0
    reg = sum(R.reg_sum([t], [m], [w], p) for t, (m, w, p) in zip(th, specs))
    print("joint output precision", got[0], jp, "reg_sum", s["output_reg_sum"], reg)
    # one f32 rounding of the f64 sum: inside 2^-23 nb, read as an absolute or as a relative bound
    assert abs(s["output_reg_sum"] - reg) <= EPS * nb and abs(s["output_reg_sum"] - reg) / reg <= EPS
    net.close()
    c.close()


def test_fixed_precision_globals():
    from bann import InitConfig, Net
    specs = with_prior("ridge_base")
    c = make_context(specs)
    net = Net(c, seed=1)
    net.init(InitConfig(variance=0.2, fixed_precision=0.7), seed=9)
    for b in range(len(specs)):
        assert np.all(c.get_precisions(b) == np.float32(0.7)), b
    s = net.summary()
    assert s["output_layer_precision"] == np.float32(0.7) and s["error_precision"] == 2.0
    net.close()
    c.close()
    c = make_context(SPECS)                                                # ARD branches: refused
    net = Net(c, seed=1)
    refused(-5, net.init, InitConfig(fixed_precision=0.7), 1)
    net.close()
    c.close()


@pytest.mark.parametrize("n", [65, 4093])
def test_phenotypes(n):
    from bann import InitConfig, Net
    c = make_context(SPECS, n=n, seed=5)
    net = Net(c, seed=1)
    net.init(InitConfig(variance=0.3), seed=13)
    g = net.predict()
    assert np.all(np.isfinite(g)) and np.var(g) > 0
    y1, st1 = net.simulate_y(1.0, seed=3)
    assert np.array_equal(y1, g) and st1["env_variance"] == 0.0          # h = 1: predict's bits
    other = make_context(SPECS, n=n + 7, seed=6)                         # a second cohort with the same branches
    y2, st2 = net.simulate_y(1.0, seed=3, ctx=other)
    assert y2.shape == (n + 7,) and np.array_equal(y2, net.predict(other))
    assert np.array_equal(net.predict(), g)
    y, st = net.simulate_y(0.5, seed=5)
    g64, y64 = g.astype(np.float64), y.astype(np.float64)
    s2 = float(np.var(g64, ddof=1))
    rv = st["env_variance"]
    print(f"n {n} s2 {s2:.6g} rv {rv:.6g} mean {st['mean']:.6g} variance {st['variance']:.6g}")
    assert abs(rv - s2) <= 1e-6 * s2                                     # rv = s2 (1 / 0.5 - 1)
    for ys, sts in ((y64, st), (y1.astype(np.float64), st1), (y2.astype(np.float64), st2)):
        m64, v64 = float(np.mean(ys)), float(np.var(ys, ddof=1))
        assert abs(sts["mean"] - m64) <= 1e-6 * abs(m64) and abs(sts["variance"] - v64) <= 1e-6 * v64
    d = y64 - g64
    if n == 4093:
        assert abs(float(np.mean(d))) <= 5.0 * math.sqrt(rv / n)
        assert abs(float(np.var(d, ddof=1)) - rv) <= 5.0 * math.sqrt(2.0 / (n - 1)) * rv
    y_again, st_again = net.simulate_y(0.5, seed=5)
    assert np.array_equal(y_again, y) and st_again == st                  # the same seed, the same y
    assert not np.array_equal(net.simulate_y(0.5, seed=6)[0], y)
    y3, st3 = net.simulate_y(0.25, seed=5)
    assert abs(st3["env_variance"] - 3.0 * s2) <= 1e-6 * 3.0 * s2
    for h in (0.0, 1.5, float("nan"), -0.5):
        refused(-5, net.simulate_y, h, 1)
    net.close()
    other.close()
    c.close()


def small_context(depth=1, hidden=("fraction", 0.5), summary=("fraction", 1.0)):
    from bann import BannContext, arch
    from bann.io import read_grouping
    c = BannContext(0)
    c.load_bed(os.path.join(PLINK, "small"))
    for g in read_grouping(os.path.join(PLINK, "small.gene_grouping")):
        c.add_branch(g, arch.layer_widths(len(g), depth, hidden, summary), "tanh", "ridge_ard")
    c.finalize()
    return c


def test_new_net_trains(tmp_path):
    """train-new's construction, mode 0 (every bias precision +inf), then both samplers: their first
    Gibbs step redraws the infinite entries, and everything is finite afterwards"""
    from bann import MCMCConfig, simulate
    net = simulate.new_net(os.path.join(PLINK, "small"), os.path.join(PLINK, "small.gene_grouping"), "ridge_ard",
                           "tanh", 1, seed=3)
    c = net._ctx
    nb = c.num_branches
    assert nb == 3 and [c.branch_info(b)[2] for b in range(nb)] == [[2, 2, 1], [2, 2, 1], [3, 3, 1]]
    for b in range(nb):
        q = c.get_precisions(b)
        assert np.all(np.isinf(q[-3:-1])) and np.all(np.isfinite(q[:-3])) and q[-1] == 2.0, (b, q)
    y, _ = net.simulate_y(0.5, seed=1)
    cfg = MCMCConfig(hmc_integration_length=5, chain_length=2, burn_in=0, hmc_step_size_factor=0.1)
    net.train_network(y, cfg, outdir=str(tmp_path / "network"))
    net.train(y, cfg, outdir=str(tmp_path / "sweep"))
    for b in range(nb):
        assert np.all(np.isfinite(c.get_params(b))) and np.all(np.isfinite(c.get_precisions(b))), b
    for d in ("network", "sweep"):
        assert len(os.listdir(tmp_path / d / "models")) >= 2, d
    assert np.all(np.isfinite(net.predict()))
    net.close()
    c.close()


def test_simulate_y_files(tmp_path):
    from bann import Net, simulate
    from bann.io import read_phen
    stem, groups = os.path.join(PLINK, "small"), os.path.join(PLINK, "small.gene_grouping")
    path = simulate.simulate_y(stem, stem, groups, "ridge_ard", "tanh", 1, str(tmp_path), heritability=1.0, seed=4)
    assert path == str(tmp_path / "RidgeARD_Tanh_d1_h1_rep1")
    assert sorted(os.listdir(path)) == ["args.json", "model.bin", "model.params", "test.phen", "test_phen_stats.json",
                                        "train.phen", "train_phen_stats.json"]
    args = json.load(open(os.path.join(path, "args.json")))
    assert args["model_type"] == "RidgeARD" and args["depth"] == 1 and args["heritability"] == 1.0
    cfgs = json.loads(open(os.path.join(path, "model.params")).read())
    assert [b["num_markers"] for b in cfgs] == [4, 4, 6] and cfgs[2]["layer_widths"] == [3, 3, 1]
    y_train, y_test = read_phen(os.path.join(path, "train.phen")), read_phen(os.path.join(path, "test.phen"))
    assert y_train.shape == (20,) and np.array_equal(y_train, y_test)     # the same cohort, h = 1
    st = json.load(open(os.path.join(path, "train_phen_stats.json")))
    assert st["env_variance"] == 0.0 and abs(st["mean"] - float(np.mean(y_train, dtype=np.float64))) <= 1e-6
    c = small_context(summary=("like_hidden",))                           # simulate-y's width rules
    net = Net(c)
    net.load(os.path.join(path, "model.bin"))
    assert np.array_equal(net.predict(), y_train)
    net.close()
    c.close()
    # with noise and effective markers: the next replicate of another name
    path2 = simulate.simulate_y(stem, stem, groups, "lasso_base", "relu", 0, str(tmp_path), heritability=0.5,
                                num_effective=2, init_gamma=(2.0, 0.5), seed=4)
    assert os.path.basename(path2) == "LassoBase_ReLU_d0_h0.5_me2_k2.0_s0.5_rep1"
    st2 = json.load(open(os.path.join(path2, "test_phen_stats.json")))
    assert st2["env_variance"] > 0 and len(os.listdir(path2)) == 7
