"""The device Gibbs step (kernels_gibbs.hip: bann_gibbs_posterior, bann_gibbs_sample_precisions)
and the bulk parameter getter, on one toy context (n = 65; the kernels read no genotypes):

| markers | widths       | prior      | exercises                                          |
| 1       | [1, 1]       | ridge_ard  | width-1 layers, shape 0.501                        |
| 33      | [3, 1]       | ridge_ard  | two layers: only layer 0 is local                  |
| 70      | [4, 4, 1]    | ridge_ard  | rows not a multiple of 64                          |
| 129     | [5, 3, 1]    | lasso_ard  |                                                    |
| 700     | [4, 4, 1]    | ridge_base | a 2 800-term whole-layer sum across a workgroup    |
| 40      | [8, 8, 1]    | lasso_base |                                                    |
| 30      | [6, 5, 3, 1] | lasso_ard  | two dense layers and a summary layer               |
"""
import numpy as np
import pytest

import bann_oracle as O
import net_oracle as NO
from helpers import f32_branch

pytestmark = pytest.mark.gpu

N = 65
SPECS = [(1, [1, 1], "ridge_ard"), (33, [3, 1], "ridge_ard"), (70, [4, 4, 1], "ridge_ard"),
         (129, [5, 3, 1], "lasso_ard"), (700, [4, 4, 1], "ridge_base"), (40, [8, 8, 1], "lasso_base"),
         (30, [6, 5, 3, 1], "lasso_ard")]
VAGUE = ((0.001, 1000.0),) * 3


def f32_hyper(pairs):
    """the hyperparameters as the C ABI receives them (float hyper[6]), as an oracle Hyper and flat"""
    r = [tuple(float(np.float32(v)) for v in p) for p in pairs]
    return O.Hyper(dense=r[0], summary=r[1], output=r[2]), [v for p in r for v in p]


def make_problem():
    rng = np.random.default_rng(17)
    g = O.synthetic_genotypes(rng, N, sum(m for m, _, _ in SPECS))
    branches, snps, off = [], [], 0
    for m, w, prior in SPECS:
        branches.append(f32_branch(O.random_branch(rng, m, w, prior=prior)))
        snps.append(np.arange(off, off + m, dtype=np.int32))
        off += m
    y = rng.normal(size=N).astype(np.float32)
    return g, branches, snps, y


def make_context(problem):
    from bann import BannContext
    g, branches, snps, y = problem
    ctx = BannContext(0)
    ctx.upload_genotypes(g)
    for s, br in zip(snps, branches):
        ctx.add_branch(s, br.layer_widths, br.act, br.prior)
    ctx.finalize()
    for b, br in enumerate(branches):
        ctx.set_params(b, O.param_vec(br.weights, br.biases))
        ctx.set_precisions(b, O.precision_vec(br))
    ctx.set_target_all(y)
    return ctx


@pytest.fixture(scope="module")
def problem():
    return make_problem()


@pytest.fixture(scope="module")
def ctx(problem):
    c = make_context(problem)
    yield c
    c.close()


def oracle_posterior(br, hp):
    """(shape, scale) in precision_vec order, 0 at the output-layer and the error entry"""
    L = br.num_layers
    sh, sc = [], []
    for l in range(L - 1):
        k, s = hp.layer(l, L)
        w = br.weights[l]
        if br.prior in O.ARD_PRIORS:
            rows = O.ard_row_posterior_params(br, l, hp)
        elif br.prior == "lasso_base":
            rows = [O.lasso_posterior_params(k, s, float(np.sum(np.abs(w))), w.size)]
        else:
            rows = [O.ridge_posterior_params(k, s, float(np.sum(w * w)), w.size)]
        sh += [r[0] for r in rows]
        sc += [r[1] for r in rows]
    sh.append(0.0)
    sc.append(0.0)
    for l in range(L - 1):
        k, s = hp.layer(l, L)
        bb = br.biases[l]
        a, c = O.ridge_posterior_params(k, s, float(np.sum(bb * bb)), bb.size)
        sh.append(a)
        sc.append(c)
    return np.array(sh + [0.0]), np.array(sc + [0.0])


@pytest.mark.parametrize("pairs", [((3.0, 2.0), (3.0, 2.0), (4.0, 5.0)), VAGUE])
def test_posterior_parameters(ctx, problem, pairs):
    """f64 sums of at most 2 800 exactly formed terms: worst case 2 800 x 2^-53 ~ 3e-13 < 1e-12"""
    _, branches, _, _ = problem
    hp, flat = f32_hyper(pairs)
    shape, scale, ostat = ctx.gibbs_posterior(flat)
    worst = 0.0
    for b, br in enumerate(branches):
        sh, sc = oracle_posterior(br, hp)
        assert shape[b].shape == sh.shape == (ctx.num_precisions(b),)
        local = sh > 0
        assert np.all(shape[b][~local] == 0.0) and np.all(scale[b][~local] == 0.0), b
        assert (~local).sum() == 2
        e1 = np.max(np.abs(shape[b][local] - sh[local]) / sh[local])
        e2 = np.max(np.abs(scale[b][local] - sc[local]) / sc[local])
        e3 = abs(ostat[b] - NO.out_stat(br)) / NO.out_stat(br)
        worst = max(worst, e1, e2, e3)
        assert e1 <= 1e-12 and e2 <= 1e-12 and e3 <= 1e-12, (b, e1, e2, e3)
    print("worst relative error", worst)
    # a sub-list in another order: the same values per branch; NULL outputs are skipped
    sh2, sc2, os2 = ctx.gibbs_posterior(flat, branches=[4, 1])
    assert np.array_equal(sh2[0], shape[4]) and np.array_equal(sc2[1], scale[1])
    assert np.array_equal(os2, ostat[[4, 1]])


def read_state(c, branches_n):
    return [c.get_precisions(b) for b in range(branches_n)]


def test_draw_is_consistent_with_set_precisions(problem):
    """what k_gibbs_draw writes (lam, lamld, step bases, eprec, the host mirrors) is what
    bann_branch_set_precisions derives from the same vectors: bitwise equal gradients, log
    densities and Izmailov step sizes on a twin context"""
    _, branches, _, y = problem
    nb = len(branches)
    a, t = make_context(problem), make_context(problem)
    _, flat = f32_hyper(VAGUE)
    th0 = [a.get_params(b) for b in range(nb)]
    pred0 = a.predict_many(range(nb))
    a.gibbs_sample_precisions(flat, 0.75, 1.5, seed=99)
    prec = read_state(a, nb)
    for b, br in enumerate(branches):
        L = br.num_layers
        q_out = sum(p.size for p in br.weight_precisions[:-1])
        assert prec[b][q_out] == np.float32(0.75) and prec[b][-1] == np.float32(1.5), b
        assert np.all(np.isfinite(prec[b])) and np.all(prec[b] > 0), b
        assert prec[b].size == q_out + 1 + (L - 1) + 1
        assert np.array_equal(a.get_params(b), th0[b]), b     # parameters unchanged
        t.set_precisions(b, prec[b])
    assert np.array_equal(a.predict_many(range(nb)), pred0)   # predictions unchanged
    ga, ra = a.log_density_gradient_many(range(nb))
    gt, rt = t.log_density_gradient_many(range(nb))
    assert np.array_equal(ra, rt)
    for b in range(nb):
        assert np.array_equal(ga[b], gt[b]), b
        assert a.log_density(b, float(ra[b])) == t.log_density(b, float(rt[b])), b
    # a later set_precisions on the drawn context behaves as on any other
    a.set_precisions(2, prec[2])
    assert np.array_equal(a.log_density_gradient_many([2])[0][0], gt[2])
    mom = np.random.default_rng(5).normal(size=sum(p.size for p in th0)).astype(np.float32)
    u = np.full(nb, 0.5, np.float32)
    ra_ = a.hmc_step(range(nb), 2, 10.0, step_mode="izmailov", step_factor=0.01, momentum=mom, u=u)
    rt_ = t.hmc_step(range(nb), 2, 10.0, step_mode="izmailov", step_factor=0.01, momentum=mom, u=u)
    assert np.array_equal(ra_["status"], rt_["status"]) and np.array_equal(ra_["trace"], rt_["trace"])
    for b in range(nb):
        ea, et = a.get_step_sizes(b), t.get_step_sizes(b)
        assert np.all(ea > 0) and np.array_equal(ea, et), b
        assert np.array_equal(a.get_params(b), t.get_params(b)), b
    a.close()
    t.close()


def test_determinism_and_independence(problem):
    _, branches, _, _ = problem
    nb = len(branches)
    c = make_context(problem)
    _, flat = f32_hyper(VAGUE)
    c.gibbs_sample_precisions(flat, 0.5, 2.0, seed=7)
    p1 = read_state(c, nb)
    c.gibbs_sample_precisions(flat, 0.5, 2.0, seed=7)
    p2 = read_state(c, nb)
    c.gibbs_sample_precisions(flat, 0.5, 2.0, seed=8)
    p3 = read_state(c, nb)
    for b in range(nb):
        assert np.array_equal(p1[b], p2[b]), b        # the same seed, the same bits
        assert not np.array_equal(p1[b], p3[b]), b    # another seed differs
    # branches [1, 3] alone get the values they get when all are drawn; the others keep theirs
    c.gibbs_sample_precisions(flat, 0.5, 2.0, seed=7, branches=[3, 1])
    p4 = read_state(c, nb)
    for b in range(nb):
        assert np.array_equal(p4[b], p1[b] if b in (1, 3) else p3[b]), b
    c.close()


def test_distribution_on_the_device(problem):
    """draw / scale ~ Gamma(shape, 1): over 64 fixed seeds, every ARD row of the 70-marker branch
    (shape 2.001) and the width-1 branch's two entries (shape 0.501), pooled per shape class:
    mean and variance at five standard errors (as tests/gibbs_gamma_check.cpp) and a KS test"""
    from scipy import stats
    c = make_context(problem)
    _, flat = f32_hyper(VAGUE)
    shape, scale, _ = c.gibbs_posterior(flat)
    rows = {0: [0, 2], 2: list(range(70 + 4))}   # branch -> local entries (ARD rows of both layers; row + bias)
    assert np.allclose(shape[0][rows[0]], 0.501, atol=1e-6) and np.allclose(shape[2][rows[2]], 2.001, atol=1e-6)
    pools = {0: [], 2: []}   # per branch = per shape class
    for seed in range(1000, 1064):
        c.gibbs_sample_precisions(flat, 1.0, 1.0, seed=seed, branches=[0, 2])
        for b in pools:
            pools[b].append(c.get_precisions(b)[rows[b]].astype(np.float64) / scale[b][rows[b]])
    for b, vals in pools.items():
        v = np.concatenate(vals)
        a, n = float(shape[b][0]), v.size   # the class's shape, as the kernel formed it (f32 hyperparameters)
        assert n == 64 * len(rows[b])
        assert np.all(np.isfinite(v)) and np.all(v > 0)
        mean, var = float(np.mean(v)), float(np.var(v, ddof=1))
        ks = stats.kstest(v, stats.gamma(a).cdf)
        print(f"shape {a:.6f} N {n} mean {mean:.5f} var {var:.5f} KS p {ks.pvalue:.4f}")
        assert abs(mean - a) <= 5.0 * np.sqrt(a / n), (a, mean)
        assert abs(var - a) <= 5.0 * np.sqrt((2.0 * a * a + 6.0 * a) / n), (a, var)
        assert ks.pvalue > 1e-3, (a, ks)
    c.close()


def test_refusals(ctx, problem):
    from bann import BannContext, BannError
    _, flat = f32_hyper(VAGUE)
    before = [ctx.get_precisions(b) for b in range(len(SPECS))]

    def refused(code, fn, *args, **kw):
        with pytest.raises(BannError) as e:
            fn(*args, **kw)
        assert e.value.code == code, e.value

    for fn, args in ((ctx.gibbs_posterior, (flat,)), (ctx.gibbs_sample_precisions, (flat, 1.0, 1.0, 3))):
        refused(-5, fn, *args, branches=[1, 2, 1])          # duplicate
        refused(-5, fn, *args, branches=[0, len(SPECS)])    # out of range
        refused(-5, fn, None, *args[1:])                    # null hyper
    for b in range(len(SPECS)):
        assert np.array_equal(ctx.get_precisions(b), before[b]), b
    # a std-normal branch has no precisions to sample; an unfinalized context is a state error
    g, _, _, _ = problem
    c = BannContext(0)
    c.upload_genotypes(g)
    c.add_branch(np.arange(10, dtype=np.int32), [2, 1], "tanh", "std_normal")
    c.add_branch(np.arange(10, 20, dtype=np.int32), [2, 1], "tanh", "ridge_ard")
    refused(-4, c.gibbs_posterior, flat, branches=[1])
    c.finalize()
    refused(-5, c.gibbs_posterior, flat)
    refused(-5, c.gibbs_sample_precisions, flat, 1.0, 1.0, 3, branches=[0])
    c.gibbs_sample_precisions(flat, 1.0, 1.0, 3, branches=[1])   # the ridge branch alone is fine
    c.set_target_all(np.zeros(N, np.float32))
    c.leapfrog_begin([1], 2, step_factor=0.01)   # inside a leapfrog session: a state error
    try:
        refused(-4, c.gibbs_posterior, flat, branches=[1])
        refused(-4, c.gibbs_sample_precisions, flat, 1.0, 1.0, 3, branches=[1])
        c.leapfrog_steps(2)
    finally:
        c.leapfrog_end()
    c.close()


def test_get_params_all(ctx, problem):
    _, branches, _, _ = problem
    allp = ctx.get_params_all()
    each = np.concatenate([ctx.get_params(b) for b in range(len(branches))])
    assert allp.dtype == np.float32 and np.array_equal(allp, each)
    assert np.array_equal(allp, np.concatenate([O.param_vec(br.weights, br.biases) for br in branches])
                          .astype(np.float32))
