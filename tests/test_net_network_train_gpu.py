"""bann_net_train_network (include/bann_net.h): training with the network-joint sampler -- per
chain iteration one blocked Gibbs sweep over [precisions | all theta] -- against a reference
loop written here from the oracle's pieces (O.network_hmc_step, NetOracle's Gibbs draws, LPD and
records), on the problem of tests/test_net_driver.py (n = 700, branches of 40, 64 and 30 markers).

With RNG hooks installed both sides replay the same numpy stream, in the order bann_net.h
documents: the error precision, every branch's local precisions in branch order, the output
precision, P_total normals, one uniform, then the bias draws; no shuffle.  Tolerance: the project's
chain-level CHAIN_TOL = 1e-4 (test_net_driver.py).
"""
import json
import os

import numpy as np
import pytest

import bann_oracle as O
import net_oracle as NO
from helpers import norm_rel
from test_net_driver import CHAIN_TOL, build, rel

pytestmark = pytest.mark.gpu

f32 = lambda v: float(np.float32(v))   # noqa: E731  (what the device keeps of a host draw)


def oracle_network_train(branches, X, hp, y, d, chain_length, L_int, factor=1.0, step_mode="izmailov",
                         sampled_output_bias=False, fixed_param_precisions=False, max_dH=10.0):
    """the sweeps of bann_net_train_network, float64 on the oracle's branch math; returns the
    NetOracle holding the final state and the per-sweep trajectory results"""
    ora = NO.NetOracle(branches, X, hp)
    y = np.asarray(y, dtype=np.float64)
    n, nb = y.size, len(ora.br)
    k_out, s_out = hp.output
    lasso = ora.br[0].prior.startswith("lasso")
    # start: initialize_stats (net.rs:158-171) and the first record, as NetOracle.train
    ora.residual = y - ora.ob_bias
    for b in range(nb):
        ora._from_cfg(b)
        ora.residual = ora.residual - O.predict(ora.br[b], X[b])
        ora._update_lpd(b)
    ora._record()
    outs = []
    for _sweep in range(chain_length):
        # 1. the error precision (sample_error_precision, branch_sampler.rs:190-202)
        a, s = O.ridge_posterior_params(k_out, s_out, float(np.sum(ora.residual ** 2)), n)
        ora.g_eprec = f32(d.gamma(a, s))
        # 2. every branch's local precisions in branch order, then the one output-layer precision
        if not fixed_param_precisions:
            for br in ora.br:
                ora._sample_prior_precisions(br, d)
            total = sum(NO.out_stat(br) for br in ora.br)
            post = O.lasso_posterior_params if lasso else O.ridge_posterior_params
            a, s = post(k_out, s_out, total, ora.g_num)
            ora.g_oprec = f32(d.gamma(a, s))
        for br in ora.br:   # BranchCfg::update_global_params
            br.error_precision = ora.g_eprec
            br.weight_precisions[-1] = np.array([ora.g_oprec])
        # 3. one network trajectory: P_total normals in branch and param_vec order, one uniform
        p_list = [np.array([d.normal() for _ in range(br.num_params)]).astype(np.float32).astype(np.float64)
                  for br in ora.br]
        u = f32(d.uniform())
        if step_mode == "izmailov":
            eps = [O.param_vec(*O.izmailov_step_sizes(br, factor, L_int)) for br in ora.br]
        else:
            eps = [O.param_vec(*O.uniform_step_sizes(br, factor)) for br in ora.br]
        out = O.network_hmc_step(ora.br, X, y, ora.ob_bias, ora.g_eprec, eps, p_list, L_int, max_dH, u)
        outs.append(out)
        ora.ns += 1
        ora.nacc += out["status"] == O.ACCEPTED
        ora.nearly += out["status"] == O.REJECTED_EARLY
        ora.residual = y - ora.ob_bias - sum(O.predict(br, x) for br, x in zip(ora.br, X))
        # 4. the output bias (net.rs:319-332)
        ora.ob_eprec = ora.g_eprec
        ora.residual = ora.residual + ora.ob_bias
        sr = float(np.sum(ora.residual))
        if sampled_output_bias:   # the prior SHAPE passed as the scale (net.rs:61-66)
            ora.ob_prec = d.gamma(k_out + 0.5, 2.0 * k_out / (2.0 + k_out * ora.ob_bias ** 2))
            den = n * ora.ob_eprec + ora.ob_prec
            ora.ob_bias = ora.ob_eprec / den * sr + np.sqrt(1.0 / den) * d.normal()
        else:
            ora.ob_bias = sr / n
        ora.residual = ora.residual - ora.ob_bias
        # 5. the record: the LPD as initialize_stats forms it, over the new statistic
        ora.g_reg = sum(NO.out_stat(br) for br in ora.br)
        for b in range(nb):
            ora._from_cfg(b)
            ora._update_lpd(b)
        ora._record()
    return ora, outs


# (prior, options, rejections the oracle run must contain).  With the context's step rule off the
# plain Izmailov steps at factor 1 diverge on this problem (the common mode, DESIGN.md 7: every
# trajectory is rejected at its first step), so each case runs at a factor whose oracle run --
# on the CPU, with the oracle alone -- accepts with wide margins: |dH| <= 2.2 against the early
# rejection bound 10, and dH - log u >= 0.4 at every Metropolis test.
PARITY = [
    ("ridge_ard", dict(factor=0.1), None),
    ("lasso_base", dict(factor=0.3), None),
    ("lasso_ard", dict(factor=0.3, sampled_output_bias=True), None),
    ("ridge_base", dict(step_mode="uniform", factor=0.004), None),
    # the restore path -- parameters and residual after a rejected trajectory.  Factors chosen the
    # same way: at 0.5 the third trajectory fails its Metropolis test (dH -1.30 against log u -0.41);
    # at 0.7 the first and third are rejected early (|dH| 44 and 48 at step 2) around an accepted one
    ("lasso_base", dict(factor=0.5), 1),
    ("lasso_base", dict(factor=0.7), 2),
]


@pytest.mark.parametrize("prior,opts,rejections", PARITY)
def test_chain_matches_reference_loop(prior, opts, rejections):
    from bann import MCMCConfig, Net
    ctx, branches, X, y = build(prior)
    ctx.set_network_step_rule("off")   # the device rule finds its threshold within 2^(1/4); the oracle's is exact
    hp = O.Hyper()
    net = Net(ctx, (hp.dense, hp.summary, hp.output))
    d_dev, d_ora = NO.Draws(11), NO.Draws(11)
    net.set_rng(d_dev.uniform, d_dev.normal, d_dev.gamma)
    L, chain = 6, 3
    factor, mode = opts.get("factor", 1.0), opts.get("step_mode", "izmailov")
    sampled = opts.get("sampled_output_bias", False)
    net.train_network(y, MCMCConfig(hmc_integration_length=L, chain_length=chain, hmc_step_size_factor=factor,
                                    hmc_step_size_mode=mode, sampled_output_bias=sampled))
    ora, outs = oracle_network_train(branches, X, hp, y, d_ora, chain, L, factor=factor, step_mode=mode,
                                     sampled_output_bias=sampled)
    if rejections is not None:   # the case cannot quietly lose its rejection
        assert ora.ns - ora.nacc == rejections and rejections >= 1, [o["status"] for o in outs]
    assert d_dev.uniform() == d_ora.uniform(), "draw streams diverged (different number of draws)"
    s = net.summary()
    assert (s["num_samples"], s["num_accepted"], s["num_early_rejected"]) == (ora.ns, ora.nacc, ora.nearly)
    assert s["num_samples"] == chain
    mse, lpd = net.records()
    assert len(mse) == len(lpd) == len(ora.mse) == chain + 1
    print("mse", mse, ora.mse, "lpd", lpd, ora.lpd)
    for a, b in zip(mse, ora.mse):
        assert rel(a, b) < CHAIN_TOL, (mse, ora.mse)
    for a, b in zip(lpd, ora.lpd):
        assert rel(a, b) < CHAIN_TOL, (lpd, ora.lpd)
    for b, br in enumerate(ora.br):
        assert norm_rel(ctx.get_params(b), O.param_vec(br.weights, br.biases)) < CHAIN_TOL, b
        assert norm_rel(ctx.get_precisions(b), O.precision_vec(br)) < CHAIN_TOL, b
    assert norm_rel(net.residual(), ora.residual) < CHAIN_TOL
    assert abs(s["output_bias"] - ora.ob_bias) <= CHAIN_TOL * max(1.0, abs(ora.ob_bias))
    assert rel(s["error_precision"], ora.g_eprec) < CHAIN_TOL
    assert rel(s["output_reg_sum"], ora.g_reg) < CHAIN_TOL
    net.close()
    ctx.close()


def run_device(prior, seed, cfg, gibbs="device", n=700, build_seed=3):
    from bann import Net
    ctx, _, _, y = build(prior, seed=build_seed, n=n)
    net = Net(ctx, seed=seed)
    net.train_network(y, cfg, gibbs=gibbs)
    nb = ctx.num_branches
    state = dict(params=[ctx.get_params(b) for b in range(nb)], prec=[ctx.get_precisions(b) for b in range(nb)],
                 records=net.records(), summary=net.summary(), residual=net.residual())
    net.close()
    ctx.close()
    return state


def same_chain(a, b):
    for k in ("params", "prec", "records"):
        for x, z in zip(a[k], b[k]):
            assert np.array_equal(x, z), k
    assert a["summary"] == b["summary"]
    assert np.array_equal(a["residual"], b["residual"])


def test_device_path_is_deterministic():
    """no hooks: the device Gibbs draws, the device momentum and the built-in generator -- two
    nets with the same seed give the same bits; every precision is finite and positive"""
    from bann import MCMCConfig
    cfg = MCMCConfig(hmc_integration_length=5, chain_length=3, hmc_step_size_factor=0.5)
    a = run_device("lasso_ard", 5, cfg)
    b = run_device("lasso_ard", 5, cfg)
    same_chain(a, b)
    c = run_device("lasso_ard", 6, cfg)
    assert not all(np.array_equal(x, z) for x, z in zip(a["prec"], c["prec"]))
    for p in a["prec"]:
        assert np.all(np.isfinite(p)) and np.all(p > 0)
    assert a["summary"]["num_samples"] == 3 and len(a["records"][0]) == 4


def test_device_path_reduces_mse():
    """the learnable problem of test_net_driver.test_training_reduces_mse"""
    from bann import MCMCConfig
    s = run_device("ridge_ard", 1, MCMCConfig(hmc_integration_length=20, chain_length=12, hmc_step_size_factor=0.1),
                   n=3000, build_seed=21)
    mse, lpd = s["records"]
    assert s["summary"]["num_samples"] == 12 and s["summary"]["num_accepted"] > 0, s["summary"]
    assert mse[-1] < mse[0], mse
    assert np.all(np.isfinite(lpd))


def test_fixed_precisions_host_and_device_agree():
    """fixed_param_precisions: the flag changes nothing but the local-precision draws, so the two
    Gibbs paths give bitwise equal chains"""
    from bann import MCMCConfig
    cfg = MCMCConfig(hmc_integration_length=5, chain_length=3, hmc_step_size_factor=0.5, fixed_param_precisions=True)
    same_chain(run_device("ridge_ard", 9, cfg, gibbs="host"), run_device("ridge_ard", 9, cfg, gibbs="device"))


def test_files(tmp_path):
    from bann import MCMCConfig, Net
    ctx, branches, X, y = build("ridge_ard", seed=5)
    net = Net(ctx, seed=7)
    net.train_network(y, MCMCConfig(hmc_integration_length=5, chain_length=3, burn_in=1, hmc_step_size_factor=0.5,
                                    trace=True), outdir=str(tmp_path))
    files = sorted(os.listdir(tmp_path / "models"))
    assert "2.bin" in files and "3.bin" in files and os.path.exists(tmp_path / "training_stats")
    assert files == ["1.bin", "2.bin", "3.bin"], files   # every chain_ix >= burn_in (net.rs:338-342)
    js = json.load(open(tmp_path / "training_stats"))
    assert js["num_samples"] == 3 and len(js["mse_train"]) == 4 and len(js["lpd"]) == 4
    assert len(open(tmp_path / "trace").read().splitlines()) == 4
    rows = net.predict_dir(str(tmp_path / "models"))
    assert rows.shape == (3, ctx.n) and np.array_equal(rows[-1], net.predict())
    f = NO.read_net_file(str(tmp_path / "models" / "3.bin"))
    assert f["training_stats"]["num_samples"] == 3
    ctx2, _, _, _ = build("ridge_ard", seed=9)
    net2 = Net(ctx2)
    net2.load(str(tmp_path / "models" / "3.bin"))
    for b in range(3):
        assert np.array_equal(ctx2.get_precisions(b), ctx.get_precisions(b)), b
        assert np.array_equal(ctx2.get_params(b), ctx.get_params(b)), b
    t = net.network_timing()
    assert t["total_ms"] > 0 and t["gibbs_ms"] > 0 and t["trajectory_ms"] > 0 and t["record_ms"] > 0
    assert t["gibbs_ms"] + t["trajectory_ms"] + t["record_ms"] <= t["total_ms"]
    for o in (net, net2, ctx, ctx2):
        o.close()


def test_test_data():
    from bann import BannContext, MCMCConfig, Net
    ctx, branches, X, y = build("ridge_ard", seed=5)
    rng = np.random.default_rng(77)
    ms = (40, 64, 30)
    gt = O.synthetic_genotypes(rng, 300, sum(ms))
    tctx = BannContext(0)
    tctx.upload_genotypes(gt)
    off = 0
    for m, br in zip(ms, branches):
        tctx.add_branch(np.arange(off, off + m, dtype=np.int32), br.layer_widths, "tanh", "ridge_ard")
        off += m
    tctx.finalize()
    y_test = rng.normal(size=300).astype(np.float32)
    net = Net(ctx, seed=3)
    net.set_test_data(tctx, y_test)
    chain = 3
    net.train_network(y, MCMCConfig(hmc_integration_length=4, chain_length=chain, hmc_step_size_factor=0.5))
    mt = net.records_test()
    assert mt.size == chain + 1
    pred = net.predict(tctx)
    # record_perf sums the branch rows in f64, predict in f32: <= 4 ulp (2.4e-7) of a prediction each
    assert rel(float(mt[-1]), float(np.mean((y_test.astype(np.float64) - pred) ** 2))) < 1e-5
    for o in (net, ctx, tctx):
        o.close()


class CountingAllreduce:
    """a caller all-reduce that counts its calls (and would sum nothing: one process)"""

    def __init__(self):
        from bann._lib import ALLREDUCE_FN
        self.calls = 0
        self.fn = ALLREDUCE_FN(self._call)

    def _call(self, _user, _buf, _count, _dtype):
        self.calls += 1
        return 0


def test_refusals():
    from bann import BannError, MCMCConfig, Net
    ctx, _, _, y = build("ridge_base")
    net = Net(ctx, seed=3)
    base = dict(hmc_integration_length=3, chain_length=1)
    for bad in (dict(joint_hmc=True), dict(gradient_descent=True), dict(gradient_descent_joint=True),
                dict(trajectories=True), dict(effect_sizes=True), dict(hmc_step_size_mode="random"),
                dict(hmc_step_size_mode="std_scaled")):
        with pytest.raises(BannError) as e:
            net.train_network(y, MCMCConfig(**base, **bad))
        assert e.value.code == -5, (bad, e.value)
    assert net.summary()["num_samples"] == 0 and net.summary()["num_records"] == 0
    # a two-rank communicator: refused before any collective is called
    ar = CountingAllreduce()
    ctx.comm_callback(ar, 2, 0)
    with pytest.raises(BannError) as e:
        net.train_network(y, MCMCConfig(**base))
    assert e.value.code == -4 and ar.calls == 0, (e.value, ar.calls)
    assert net.summary()["num_records"] == 0
    net.close()
    ctx.close()
