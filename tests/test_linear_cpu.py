"""CPU-side checks of the linear simulators: the directory names (with simulate-xy's linear quirk), the
LinearModel line, the numpy restatement's own invariants and the seeds the GPU tests rely on, the new
entry points in the header, the binding and the built library, and the resource report of
kernels_lin.hip for gfx950."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import linear_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
LIB = os.path.join(ROOT, "rs-bann_amd", "librsbann_amd.so")
HIPCC = "/opt/rocm/bin/hipcc"
NEW_FUNCTIONS = ["bann_genotypes_linear_score", "bann_genotypes_linear_chunk", "bann_genotypes_linear_timing",
                 "bann_linear_effects", "bann_linear_simulate_y", "bann_genotypes_synthetic_maf",
                 "bann_genotypes_save_bed"]
NEW_KERNELS = ["k_lin_weights", "k_lin_offsetE", "k_lin_offset_fold", "k_lin_scoreILi1E", "k_lin_scoreILi2E", "k_lin_scoreILi3E",
               "k_lin_scoreILi4E", "k_lin_fold", "k_lin_hist", "k_lin_scan", "k_lin_count", "k_lin_draw"]


def test_directory_names():
    from bann.simulate import output_dir_name, xy_output_dir_name
    # simulate-y --model-type Linear (rs-bann.rs:530-543)
    assert output_dir_name("linear", None, 0, 0.5) == "Linear_h0.5"
    assert output_dir_name("linear", None, 0, 1.0, num_effective=3, proportion_effective=0.2) == "Linear_h1_me3"
    assert output_dir_name("linear", None, 0, 0.25, proportion_effective=0.5) == "Linear_h0.25_pe0.5"
    # the network names are what they were
    assert output_dir_name("ridge_ard", "tanh", 1, 1.0) == "RidgeARD_Tanh_d1_h1"
    # simulate-xy (rs-bann.rs:803-827)
    assert xy_output_dir_name("ridge_ard", "tanh", 3, 4, None, 1, 33, 65, 0.5) == "RidgeARD_Tanh_b3_wh4_ws4_d1_m33_n65_h0.5"
    assert xy_output_dir_name("lasso_base", "relu", 2, 4, 2, 0, 10, 100, 1.0, num_effective=3,
                              init_param_variance=1.0) == "LassoBase_ReLU_b2_wh4_ws2_d0_m10_n100_h1_me3_v1.0"
    assert xy_output_dir_name("ridge_base", "silu", 2, 4, 2, 0, 10, 100, 0.5, proportion_effective=0.5,
                              init_gamma=(2.0, 0.5)) == "RidgeBase_SiLU_b2_wh4_ws2_d0_m10_n100_h0.5_pe0.5_k2.0_s0.5"
    # its linear variant (rs-bann.rs:653-676): no activation, and "v_" / "k_" / "s_" with no underscore in front
    assert xy_output_dir_name("linear", None, 3, 4, None, 1, 33, 65, 0.5) == "Linear_b3_wh4_ws4_d1_m33_n65_h0.5"
    assert xy_output_dir_name("linear", None, 3, 4, 2, 1, 33, 65, 0.5, num_effective=7, init_param_variance=1.0) == \
        "Linear_b3_wh4_ws2_d1_m33_n65_h0.5_me7v_1.0"
    assert xy_output_dir_name("linear", None, 3, 4, 2, 1, 33, 65, 0.5, init_gamma=(2.0, 0.5)) == \
        "Linear_b3_wh4_ws2_d1_m33_n65_h0.5k_2.0s_0.5"


def test_linear_model_line():
    from bann.simulate import linear_model_line
    eff = np.array([0.5, 0.0, -1.25, 3.0, np.float32(0.1)], np.float32)
    text = linear_model_line([2, 3], eff)
    assert text == '{"num_branches":2,"num_markers_per_branch":[2,3],"effects":[[0.5,0.0],[-1.25,3.0,0.1]]}\n'
    assert text == R.linear_model_line([np.arange(2), np.arange(3)], eff)
    back = json.loads(text)
    assert np.array_equal(np.concatenate([np.asarray(e, np.float32) for e in back["effects"]]), eff)
    with pytest.raises(ValueError):
        linear_model_line([2, 2], eff)


def test_phen_json(tmp_path):
    from bann.simulate import write_phen_json
    y = np.array([1.0, -0.25, np.float32(0.1)], np.float32)
    write_phen_json(str(tmp_path / "y.json"), y)
    text = open(tmp_path / "y.json").read()
    assert text == '{"y":[1.0,-0.25,0.1]}'
    assert np.array_equal(np.asarray(json.loads(text)["y"], np.float32), y)


def test_restatement_masks():
    """the exact count, ties broken by index, and the seeds the GPU tests use for p = 0.25"""
    for E in (1, 255, 257, 70001):
        for e in (0, 1, E - 1, E):
            assert int(R.keep_mask(5, E, num_effective=e).sum()) == e
        assert int(R.keep_mask(R.P_SEED, E, proportion_effective=0.25).sum()) >= 1, E
        assert R.keep_mask(5, E).all()
    keys = R.include_keys(5, 70001)
    assert keys.dtype == np.uint64 and int(keys.max()) < 2 ** 32
    # the order of (key, index) is stable: among equal keys the smaller index comes first
    key = np.array([7, 3, 7, 3, 9], np.uint64)
    order = np.lexsort((np.arange(5), key))
    assert order.tolist() == [1, 3, 0, 2, 4]
    # another stream than the per-branch selection keys of the network initialisation
    import init_reference as I
    assert not np.array_equal(R.include_keys(5, 700), I.select_keys(5, 0, 700))
    k = int(R.keep_mask(5, 20000, proportion_effective=0.25).sum())
    assert abs(k - 5000) <= 5 * np.sqrt(20000 * 0.25 * 0.75)


def test_restatement_effects():
    eff, m = R.effects(5, 257, 0.7, num_effective=10)
    assert m == 10 and eff.dtype == np.float32 and int(np.count_nonzero(eff)) == 10
    full, m_all = R.effects(5, 257, 0.7)
    assert m_all == 257 and np.all(full != 0)
    # the same normal numbers under another sd: kept entries differ by the factor sqrt(257 / 10)
    keep = eff != 0
    assert np.allclose(eff[keep] / full[keep], np.sqrt(257.0 / 10.0), rtol=1e-6)
    z = R.normals(5, R.STREAM_EFFECT, 9)
    assert np.array_equal(z[:5], R.normals(5, R.STREAM_EFFECT, 5)) and np.all(np.abs(z) < 6.4)
    assert not np.array_equal(z, R.normals(5, R.STREAM_NOISE, 9))
    with pytest.raises(ValueError):
        R.effects(5, 10, 0.5, proportion_effective=0.0)


def test_restatement_score_and_bed():
    g = np.array([[0, 1, 2, 1], [2, 2, 2, 2], [0, 0, 1, 3]], np.int8)
    mu, sd = g.mean(axis=1), g.std(axis=1)
    x = R.standardize(g, mu, sd)
    assert x.shape == (4, 3) and np.all(x[:, 1] == 0) and abs(x[:, 0].sum()) < 1e-12
    s = R.score(x, [np.array([0, 2]), np.array([2])], np.array([1.0, 2.0, -2.0]))
    assert s.shape == (1, 4) and np.allclose(s[0], x[:, 0])     # marker 2 twice, its effects cancel
    assert R.bed_file_bytes(np.array([[2, 1, 0, -1, 2]], np.int8)) == b"\x6c\x1b\x01" + bytes([0b01111000, 0])


def test_new_entry_points_declared_bound_and_exported():
    import bann._lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bann.h")).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for f in NEW_FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % f, header), f
        assert f in L.SIGNATURES and hasattr(lib, f) and f in exported, f
    from bann import BannContext, simulate
    for name in ("linear_score", "linear_effects", "linear_simulate_y", "linear_chunk", "linear_timing", "save_bed"):
        assert callable(getattr(BannContext, name)), name
    assert callable(simulate.simulate_y_linear) and callable(simulate.simulate_xy)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_linear_kernels_do_not_spill(tmp_path):
    """every kernel of kernels_lin.hip for gfx950, the product's flags: no VGPR or SGPR spill, no scratch"""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-c",
                          os.path.join(CSRC, "kernels_lin.hip"), "-o", str(tmp_path / "k.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    for k in NEW_KERNELS:
        assert sum(k in fn for fn in res) == 1, (k, sorted(res))
    for fn, v in res.items():
        assert v == {"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize": 0}, (fn, v)
