"""GPU tests of the chain-level branch-r2 and population-effect-sizes
(bann_net_branch_r2s_models, bann_net_population_effect_sizes_models; rs-bann.rs:128-166,
314-372): one row per saved model file through the context's model slots, against loading
each file into a second net and calling Net::branch_r2s / Net::population_effect_sizes."""
import ctypes as C

import numpy as np
import pytest

import bann_oracle as O
from helpers import build_context, f32_branch

pytestmark = pytest.mark.gpu

SHAPES = [(40, [4, 4, 1]), (30, [6, 3, 1])]   # test_train_effect_size_csv_and_net_population's: one fx, one gx branch
N = 300


def build(shapes=SHAPES, seed=9):
    from bann import BannContext
    rng = np.random.default_rng(seed)
    g = O.synthetic_genotypes(rng, N, sum(m for m, _ in shapes))
    specs, off = [], 0
    for m, w in shapes:
        specs.append(dict(snps=np.arange(off, off + m, dtype=np.int32),
                          branch=f32_branch(O.random_branch(rng, m, w)), y=np.zeros(N)))
        off += m
    return build_context(BannContext, g, specs), rng.normal(size=N).astype(np.float32)


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """a tiny trained chain: chain 3, burn-in 1 leaves the model files of the later sweeps"""
    from bann import MCMCConfig, Net
    out = str(tmp_path_factory.mktemp("chain"))
    ctx, y = build()
    net = Net(ctx, seed=3)
    net.train(y, MCMCConfig(hmc_step_size_factor=0.3, hmc_integration_length=5, chain_length=3, burn_in=1), outdir=out)
    yield ctx, net, y, out + "/models"
    net.close()
    ctx.close()


def test_chain_stats_match_per_file_loads(chain):
    from bann import Net, list_model_files
    ctx, net, y, mdir = chain
    files = list_model_files(mdir)
    assert len(files) >= 2
    nb = ctx.num_branches
    par0 = [ctx.get_params(b) for b in range(nb)]
    sum0, yh0 = net.summary(), net.predict()
    r2 = net.branch_r2s_dir(mdir, y)
    pop, mean, var = net.population_effect_sizes_dir(mdir, moments=True)
    assert r2.shape == (len(files), nb) and pop.shape == (len(files), sum(m for m, _ in SHAPES))
    # the training net and its context are unchanged
    assert all(np.array_equal(ctx.get_params(b), par0[b]) for b in range(nb))
    np.testing.assert_equal(net.summary(), sum0)
    assert np.array_equal(net.predict(), yh0)
    # a second net over a twin context: load each file, the per-model calls
    tw, _ = build()
    net2 = Net(tw, seed=5)
    acc = 0.0
    for v in y:   # sum y^2 in f64, in order, as the library's host loop
        acc += float(v) * float(v)
    yy = np.float32(acc)
    for j, f in enumerate(files):
        net2.load(f)
        ref = net2.branch_r2s(y)
        print(f"{f}: r2 {r2[j]} vs {ref}")
        assert np.all(np.abs(r2[j].astype(np.float64) - ref) <= 1e-5), (j, r2[j], ref)
        rpop = net2.population_effect_sizes().astype(np.float64)
        assert np.linalg.norm(pop[j] - rpop) <= 1e-5 * np.linalg.norm(rpop), j
        # the f32 expression of bann_net_branch_r2s on the slots' f64 rss
        tw.models_reserve(1)
        for b in range(nb):
            tw.models_set_params(0, b, tw.get_params(b))
        rss = tw.models_branch_stats(y=y, pop=False)["rss"][0]
        tw.models_reserve(0)
        assert np.array_equal(r2[j], (np.float32(1.0) - rss.astype(np.float32) / yy).astype(np.float32)), j
    assert len({r.tobytes() for r in pop}) == len(files)   # the chain moved: the rows differ
    p64 = pop.astype(np.float64)
    assert np.allclose(mean, p64.mean(axis=0), rtol=1e-6, atol=1e-12)
    assert np.allclose(var, p64.var(axis=0, ddof=1), rtol=1e-6, atol=1e-12)
    net2.close()
    tw.close()


def test_mismatched_file(chain, tmp_path):
    """a model file saved from a net with another branch shape: both calls fail and write nothing"""
    from bann import BannError, Net, list_model_files
    ctx, net, y, mdir = chain
    files = list_model_files(mdir)
    other, _ = build(shapes=[(40, [4, 4, 1]), (31, [6, 3, 1])])
    onet = Net(other, seed=1)
    bad = str(tmp_path / "bad.bin")
    onet.save(bad)
    onet.close()
    other.close()
    with pytest.raises(BannError):
        net.branch_r2s_models([files[0], bad], y)
    with pytest.raises(BannError):
        net.population_effect_sizes_models([files[0], bad])
    fp = C.POINTER(C.c_float)
    arr = (C.c_char_p * 2)(files[0].encode(), bad.encode())
    r2 = np.full((2, ctx.num_branches), 7.0, np.float32)
    rc = net._lib.bann_net_branch_r2s_models(net._h, None, arr, 2, y.ctypes.data_as(fp), y.size, r2.ctypes.data_as(fp))
    assert rc < 0 and np.all(r2 == 7.0)
    pop = np.full((2, 70), 7.0, np.float32)
    mean, var = np.full(70, 7.0, np.float32), np.full(70, 7.0, np.float32)
    rc = net._lib.bann_net_population_effect_sizes_models(net._h, None, arr, 2, pop.ctypes.data_as(fp),
                                                          mean.ctypes.data_as(fp), var.ctypes.data_as(fp))
    assert rc < 0 and np.all(pop == 7.0) and np.all(mean == 7.0) and np.all(var == 7.0)
    assert net.branch_r2s_models(files[:1], y).shape == (1, ctx.num_branches)   # and the net keeps working
