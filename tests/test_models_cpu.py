"""CPU-side checks of the chain-level predict: the multi-model forward kernel
(kernels_fe.hip) compiles for gfx950 without spills or scratch, and the host
helpers of rs-bann predict (rs-bann.rs:288-311) -- the CSV records and the
model-file listing -- format and sort as the reference does."""
import io
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "rs-bann_amd", "csrc", "kernels_fe.hip")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_multi_model_forward_does_not_spill(tmp_path):
    """every instantiation of k_forward_fe keeps its digit operands in registers: no VGPR or
    SGPR spill, no scratch (a spilled operand is re-read from memory for every MFMA)"""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", SRC, "-o", str(tmp_path / "k.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    fe = {k: v for k, v in res.items() if k.startswith("_Z12k_forward_fe")}
    assert len(fe) == 15, sorted(fe)   # layers 2..4 x five activations
    for k, v in fe.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 2, (k, v)


def test_predictions_csv_format():
    from bann import write_predictions_csv
    f = io.StringIO()
    write_predictions_csv(f, [[1.0, 0.1, -0.0, 1e-7, 1e20, 16777216.0, float("nan"), float("inf")]])
    assert f.getvalue() == "1,0.1,-0,0.0000001,100000000000000000000,16777216,NaN,inf\n"
    f = io.StringIO()
    write_predictions_csv(f, [[0.5, -2.0], [3.25, float("-inf")]])
    assert f.getvalue() == "0.5,-2\n3.25,-inf\n"


def test_model_dir_listing_order(tmp_path):
    from bann import list_model_files
    for name in ("10.bin", "2.bin", "1.bin"):
        (tmp_path / name).write_bytes(b"x")
    (tmp_path / "0.dir").mkdir()
    (tmp_path / "0.dir" / "3.bin").write_bytes(b"x")
    got = list_model_files(str(tmp_path))
    assert [os.path.basename(p) for p in got] == ["1.bin", "10.bin", "2.bin"]
    assert all(os.path.dirname(p) == str(tmp_path) for p in got)
