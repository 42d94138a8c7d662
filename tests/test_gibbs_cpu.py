"""CPU-side checks of the device Gibbs step: the Gamma sampler of csrc/gibbs_gamma.h as the host
compiler builds it (gibbs_gamma_check.cpp: moments at five standard errors for the shape classes
the Gibbs step meets, determinism, positivity), the resource report of kernels_gibbs.hip for
gfx950, and the new symbols in the headers and the binding."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ROCM_INCLUDE = "/opt/rocm/include"
NEW_CTX = ["bann_gibbs_posterior", "bann_gibbs_sample_precisions", "bann_get_params_all"]
NEW_NET = ["bann_net_train_network", "bann_net_network_timing"]


@pytest.mark.skipif(not os.path.isdir(ROCM_INCLUDE), reason="no HIP headers for rng.h")
def test_gamma_sampler_host_program(tmp_path):
    """gibbs_gamma.h through a plain host compiler: N = 200 000 variates per shape (0.501, 1.0,
    2.001, 250.001, 1000.001), mean within 5 sqrt(a / N) and variance within
    5 sqrt((2 a^2 + 6 a) / N) of a, every draw finite and > 0, the same counters the same bits"""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gibbs_gamma_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC,
                          "-I", ROCM_INCLUDE, "-D__HIP_PLATFORM_AMD__",
                          os.path.join(ROOT, "tests", "gibbs_gamma_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gibbs_kernels_do_not_spill(tmp_path):
    """k_gibbs_stats and k_gibbs_draw for gfx950: no VGPR or SGPR spill, no scratch (the f64
    sampler is called out of line so that its constants do not crowd the scalar registers)"""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c",
                          os.path.join(CSRC, "kernels_gibbs.hip"), "-o", str(tmp_path / "k.o"),
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
    kernels = {k: v for k, v in res.items() if "k_gibbs_stats" in k or "k_gibbs_draw" in k}
    assert len(kernels) == 2, sorted(res)
    for k, v in res.items():   # the kernels and the out-of-line draw
        assert v == {"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize": 0}, (k, v)


def test_new_symbols_in_headers_and_binding():
    import bann._lib as L
    ctx_h = open(os.path.join(ROOT, "include", "bann.h")).read()
    net_h = open(os.path.join(ROOT, "include", "bann_net.h")).read()
    for f in NEW_CTX:
        assert re.search(r"\bint %s\s*\(" % f, ctx_h), f
        assert f in L.SIGNATURES, f
    for f in NEW_NET:
        assert re.search(r"\bint %s\s*\(" % f, net_h), f
        assert f in L.SIGNATURES, f
    assert re.search(r"#define BANN_NET_GIBBS_HOST\s+1\b", net_h)
    from bann import BannContext, Net
    for name in ("gibbs_posterior", "gibbs_sample_precisions", "get_params_all"):
        assert callable(getattr(BannContext, name))
    for name in ("train_network", "network_timing"):
        assert callable(getattr(Net, name))
