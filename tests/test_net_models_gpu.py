"""GPU tests of the chain-level predict (bann_net_predict_models, rs-bann predict,
rs-bann.rs:276-312): one prediction row per saved model file, through the model
slots of a context, bitwise the rows of loading each file and calling
Net::predict."""
import os

import numpy as np
import pytest

import bann_oracle as O
from helpers import f32_branch

pytestmark = pytest.mark.gpu

MS = (40, 64, 30)
WIDTHS = ((4, 4, 1), (4, 4, 1), (5, 3, 1))


def build(prior, seed=3, n=700, ms=MS, widths=WIDTHS, with_params=True):
    """the small three-branch net of test_net_driver.py's build helper"""
    from bann import BannContext
    rng = np.random.default_rng(seed)
    g = O.synthetic_genotypes(rng, n, sum(ms))
    ctx = BannContext(0)
    ctx.upload_genotypes(g)
    branches, off = [], 0
    for m, w in zip(ms, widths):
        s = np.arange(off, off + m, dtype=np.int32)
        off += m
        branches.append(f32_branch(O.random_branch(rng, m, list(w), prior=prior)))
        ctx.add_branch(s, list(w), "tanh", prior)
    ctx.finalize()
    op = branches[0].weight_precisions[-1].copy()
    for b, br in enumerate(branches):
        br.weight_precisions[-1] = op.copy()
        if with_params:
            ctx.set_params(b, O.param_vec(br.weights, br.biases))
        ctx.set_precisions(b, O.precision_vec(br))
    y = rng.normal(size=n).astype(np.float32)
    return ctx, y


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """a short trained chain with every sweep's model file"""
    from bann import MCMCConfig, Net
    out = str(tmp_path_factory.mktemp("chain"))
    ctx, y = build("ridge_ard", seed=13)
    net = Net(ctx, seed=2)
    net.train(y, MCMCConfig(hmc_integration_length=5, chain_length=6, burn_in=0, hmc_step_size_factor=0.3,
                            sampled_output_bias=True), outdir=out)
    yield ctx, net, os.path.join(out, "models")
    net.close()
    ctx.close()


def test_chain_predict(chain):
    from bann import Net, list_model_files
    ctx, net, mdir = chain
    files = list_model_files(mdir)
    assert len(files) >= 3 and files == sorted(files)
    yh0 = net.predict()
    par0 = [ctx.get_params(b) for b in range(3)]
    sum0 = net.summary()
    rows, mean, var = net.predict_dir(mdir, moments=True)
    assert rows.shape == (len(files), ctx.n)
    # the training net and its context are unchanged
    assert np.array_equal(net.predict(), yh0)
    assert all(np.array_equal(ctx.get_params(b), par0[b]) for b in range(3))
    np.testing.assert_equal(net.summary(), sum0)
    # a second net over a twin context: load each file, predict
    tw, _ = build("ridge_ard", seed=13)
    net2 = Net(tw, seed=5)
    for j, f in enumerate(files):
        net2.load(f)
        assert np.array_equal(rows[j], net2.predict()), f
    assert len({r.tobytes() for r in rows}) > 1   # the chain moved: the rows differ
    y64 = rows.astype(np.float64)
    assert np.allclose(mean, y64.mean(axis=0), rtol=1e-6, atol=1e-12)
    assert np.allclose(var, y64.var(axis=0, ddof=1), rtol=1e-6, atol=1e-12)
    # the same on a second cohort with the same branch shapes
    t1, _ = build("ridge_ard", seed=5, n=250, with_params=False)
    t2, _ = build("ridge_ard", seed=5, n=250, with_params=False)
    rows_t = net.predict_models(files, ctx=t1)
    assert rows_t.shape == (len(files), 250)
    for j, f in enumerate(files):
        net2.load(f)
        assert np.array_equal(rows_t[j], net2.predict(t2)), f
    assert np.array_equal(net.predict(), yh0)
    net2.close()
    for c in (tw, t1, t2):
        c.close()


def test_mismatched_file(chain, tmp_path):
    """a model file saved from a net with another branch shape: the call raises and the output
    array is not written"""
    import ctypes as C

    from bann import BannError, Net, list_model_files
    ctx, net, mdir = chain
    files = list_model_files(mdir)
    other, _ = build("ridge_ard", seed=13, ms=(40, 64, 31))
    onet = Net(other, seed=1)
    bad = str(tmp_path / "bad.bin")
    onet.save(bad)
    onet.close()
    other.close()
    with pytest.raises(BannError):
        net.predict_models([files[0], bad, files[1]])
    out = np.full((3, ctx.n), 7.0, np.float32)
    arr = (C.c_char_p * 3)(files[0].encode(), bad.encode(), files[1].encode())
    rc = net._lib.bann_net_predict_models(net._h, None, arr, 3, out.ctypes.data_as(C.POINTER(C.c_float)), None, None)
    assert rc < 0 and np.all(out == 7.0)
    assert net.predict_models(files[:2]).shape == (2, ctx.n)   # and the net keeps working
