"""CPU-side checks of the chain-level branch statistics: the statistics kernel
(kernels_fs.hip) compiles for gfx950 without spills or scratch at two waves per
SIMD, and the host writers of rs-bann branch-r2 (rs-bann.rs:128-166) and
population-effect-sizes (314-372) format as documented."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "rs-bann_amd", "csrc", "kernels_fs.hip")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_stats_kernel_does_not_spill(tmp_path):
    """every instantiation of k_stats_fe keeps its digit operands, accumulators and per-lane f64
    sums in registers: no VGPR or SGPR spill, no scratch (a scratch access would also break the
    tile loop's counted vector-memory waits), two waves per SIMD, LDS for two workgroups per CU"""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", SRC, "-o", str(tmp_path / "k.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    fs = {k: v for k, v in res.items() if k.startswith("_Z10k_stats_fe")}
    assert len(fs) == 15, sorted(fs)   # layers 2..4 x five activations
    for k, v in fs.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 2, (k, v)
        assert 2 * v["LDS Size"] <= 160 * 1024, (k, v)


def test_branch_r2_csv_format():
    from bann import write_branch_r2_csv
    f = io.StringIO()
    write_branch_r2_csv(f, [[0.25, -0.0, 1e-7, 0.99999994], [1.0, -3.5, float("-inf"), float("nan")]])
    assert f.getvalue() == "0.25,-0,0.0000001,0.99999994\n1,-3.5,-inf,NaN\n"
    f = io.StringIO()
    write_branch_r2_csv(f, np.array([0.5, 0.125], np.float32))   # one model: one record
    assert f.getvalue() == "0.5,0.125\n"


def test_population_effect_sizes_json_round_trip(tmp_path):
    from bann import write_population_effect_sizes_json
    rng = np.random.default_rng(3)
    v = np.concatenate([np.array([0.0, -0.0, 1e-45, -1.1754942e-38, 1e20, -3.4028235e38, 1.0, 16777216.0, 0.1],
                                 np.float32), rng.normal(scale=1e-3, size=200).astype(np.float32)])
    p = tmp_path / "pop.json"
    write_population_effect_sizes_json(str(p), v)
    back = json.loads(p.read_text())
    assert isinstance(back, list) and len(back) == v.size and all(isinstance(x, float) for x in back)
    got = np.array(back, np.float64).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), v.view(np.uint32))   # the same f32 bits, the sign of -0.0 included
    write_population_effect_sizes_json(str(p), np.zeros((2, 3), np.float32))   # flattened
    assert json.loads(p.read_text()) == [0.0] * 6


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_population_effect_sizes_json_refuses_non_finite(tmp_path, bad):
    from bann import write_population_effect_sizes_json
    p = tmp_path / "pop.json"
    with pytest.raises(ValueError):
        write_population_effect_sizes_json(str(p), [0.5, bad])
    assert not p.exists()
