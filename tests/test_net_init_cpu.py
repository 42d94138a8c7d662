"""CPU-side checks of starting a model: the width rules against the reference's own known answers,
the directory name and the stats file of simulate-y, the shared draw header as a host compiler
builds it (init_draw_check.cpp), the numpy restatement against that header's selection, and the
resource report of kernels_init.hip for gfx950."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import init_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ROCM_INCLUDE = "/opt/rocm/include"
NEW_KERNELS = ["k_init_theta", "k_init_select", "k_init_stats", "k_init_joint", "k_init_expand", "k_sim_partial",
               "k_sim_fold", "k_sim_noise"]


def test_width_rules_known_answers():
    """architectures.rs:246-256: m = 3, depth 1, Fixed(3) / Fixed(2) is [3, 2, 1] with 22 parameters;
    branch_cfg_builder.rs:407-418: hidden Fixed(3), summary width 1 has 17"""
    from bann import arch
    w = arch.layer_widths(3, 1, ("fixed", 3), ("fixed", 2))
    assert w == [3, 2, 1] and R.num_params(3, w) == 22
    w = arch.layer_widths(3, 1, ("fixed", 3), ("fixed", 1))
    assert w == [3, 1, 1] and R.num_params(3, w) == 17


@pytest.mark.parametrize("m,hidden", [(1, 1), (33, 16)])
def test_width_rules_fraction(m, hidden):
    from bann import arch
    for depth in (0, 1, 3):
        w = arch.layer_widths(m, depth)    # FractionOfInput(0.5) / LikeHiddenLayerWidth
        assert w == [hidden] * depth + [hidden, 1] == R.layer_widths(m, depth)
    # depth 0 still forms the hidden width: the summary width derives from it
    assert arch.layer_widths(m, 0, ("fixed", 7), ("like_hidden",)) == [7, 1]
    assert arch.layer_widths(m, 2, ("fraction", 0.5), ("fraction", 0.5)) == \
        R.layer_widths(m, 2, ("fraction", 0.5), ("fraction", 0.5)) == [hidden] * 2 + [max(1, hidden // 2), 1]


def test_width_rules_truncate_the_f32_product():
    from bann import arch
    for m, f in ((10, 0.3), (7, 0.7), (1000, 0.1), (3, 0.34), (100, 0.29)):
        assert arch.layer_widths(m, 1, ("fraction", f))[0] == max(1, int(np.float32(m) * np.float32(f))), (m, f)


def test_width_rules_refusals():
    from bann import BannError, arch
    for args in ((3, 1, ("fixed", 3), ("fixed", 0)),      # Fixed(0) summary width
                 (3, 1, ("fixed", 0), ("like_hidden",)),
                 (0, 1), (3, -1), (3, 7),
                 (3, 1, ("fraction", float("nan")))):
        with pytest.raises(BannError) as e:
            arch.layer_widths(*args)
        assert e.value.code == -5, args


def test_directory_name():
    from bann.simulate import output_dir_name, replicate_dir
    assert output_dir_name("ridge_ard", "tanh", 1, 1.0) == "RidgeARD_Tanh_d1_h1"
    assert output_dir_name("lasso_base", "leaky_relu", 0, 0.5, num_effective=3, proportion_effective=0.2,
                           init_param_variance=1.0) == "LassoBase_LeakyReLU_d0_h0.5_me3_v1.0"
    assert output_dir_name("ridge_base", "silu", 2, 0.25, proportion_effective=0.5, init_gamma=(2.0, 0.5)) == \
        "RidgeBase_SiLU_d2_h0.25_pe0.5_k2.0_s0.5"


def test_replicate_index(tmp_path):
    from bann.simulate import replicate_dir
    assert replicate_dir(str(tmp_path), "a") == str(tmp_path / "a_rep1")
    os.makedirs(tmp_path / "a_rep1")
    os.makedirs(tmp_path / "a_rep2")
    assert replicate_dir(str(tmp_path), "a") == str(tmp_path / "a_rep3")


def test_phen_stats_json(tmp_path):
    from bann import BannError
    from bann.simulate import write_phen_stats
    p = tmp_path / "stats.json"
    vals = {"mean": float(np.float32(0.1)), "variance": 2.0, "env_variance": 0.0}
    write_phen_stats(str(p), vals)
    text = open(p).read()
    js = json.loads(text)
    assert list(js) == ["mean", "variance", "env_variance"]
    assert all(np.float32(js[k]) == np.float32(v) for k, v in vals.items())
    assert text.startswith('{\n  "mean": 0.1,\n  "variance": 2.0,') and text.endswith("\n}")
    with pytest.raises(BannError):
        write_phen_stats(str(tmp_path / "missing" / "stats.json"), vals)


@pytest.mark.skipif(not os.path.isdir(ROCM_INCLUDE), reason="no HIP headers for rng.h")
def test_draw_header_host_program(tmp_path):
    """init_draw.h through a plain host compiler, with the host sanitizers on this program alone"""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "init_draw_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                          "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                          "-I", ROCM_INCLUDE, "-D__HIP_PLATFORM_AMD__",
                          os.path.join(ROOT, "tests", "init_draw_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]


def test_reference_masks():
    """the restatement's own properties: the exact count, ties broken by index, the proportion"""
    for m in (1, 64, 65, 700):
        for e in (0, 1, m - 1, m):
            assert int(R.keep_mask_exact(5, 3, m, e).sum()) == e
    keys = R.select_keys(5, 3, 700)
    assert keys.dtype == np.uint64 and int(keys.max()) < 2 ** 32 and len(set(keys.tolist())) > 690
    assert not np.array_equal(keys, R.select_keys(6, 3, 700)) and not np.array_equal(keys, R.select_keys(5, 4, 700))
    k = int(R.keep_mask_proportion(5, 3, 20000, 0.25).sum())
    assert abs(k - 5000) <= 5 * np.sqrt(20000 * 0.25 * 0.75)
    # Philox4x32-10 known answer (Random123 kat_vectors: counter and key all zero)
    x, y, z, w = R.philox4x32(np.zeros(1, np.uint64), 0, 0)
    assert [int(v[0]) for v in (x, y, z, w)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_reference_precisions():
    th = np.arange(1, 11, dtype=np.float32)            # m = 2, widths [2, 1, 1]: W0 4, W1 2, W2 1, b0 2, b1 1
    th[7:9] = 0.0                                      # b0 = 0
    q = R.precisions(th, 2, [2, 1, 1], "ridge_ard")
    assert q.tolist() == [2 / (1 + 9), 2 / (4 + 16), 1 / 25, 1 / 36, 1.0, np.inf, 1 / 100, 2.0]
    q = R.precisions(th, 2, [2, 1, 1], "lasso_base")
    assert q.tolist() == [4 / 30, 2 / 61, 1 / 49, np.inf, 1 / 100, 2.0]
    assert R.out_precision_index(2, [2, 1, 1], "ridge_ard") == 4 and R.out_precision_index(2, [2, 1, 1], "std_normal") == 2
    assert np.all(R.precisions(th, 2, [2, 1, 1], "ridge_base", fixed=0.5) == 0.5)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_init_kernels_do_not_spill(tmp_path):
    """every kernel of kernels_init.hip for gfx950, the product's flags: no VGPR or SGPR spill, no scratch"""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-c",
                          os.path.join(CSRC, "kernels_init.hip"), "-o", str(tmp_path / "k.o"),
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


def test_new_symbols_in_headers_and_binding():
    import bann._lib as L
    ctx_h = open(os.path.join(ROOT, "include", "bann.h")).read()
    net_h = open(os.path.join(ROOT, "include", "bann_net.h")).read()
    for f in ("bann_arch_layer_widths", "bann_init_branches", "bann_phen_stats_write"):
        assert re.search(r"\bint %s\s*\(" % f, ctx_h) and f in L.SIGNATURES, f
    for f in ("bann_net_init", "bann_net_simulate_y", "bann_net_write_params"):
        assert re.search(r"\bint %s\s*\(" % f, net_h) and f in L.SIGNATURES, f
    from bann import BannContext, InitConfig, Net, simulate
    assert callable(BannContext.init_branches) and callable(Net.init) and callable(Net.simulate_y)
    assert callable(simulate.simulate_y) and callable(simulate.new_net)
    c = InitConfig(gamma=(2.0, 0.5), num_effective=3).to_c()
    assert (c.mode, c.gamma_shape, c.gamma_scale, c.num_effective, c.has_fixed_precision) == (2, 2.0, 0.5, 3, 0)
    assert c.proportion_effective < 0 and InitConfig().to_c().mode == 0 and InitConfig(variance=0.5).to_c().mode == 1
