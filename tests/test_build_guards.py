"""Build-time guards for the hand-counted memory waits of the fxl kernel.

k_fused_grad_fxl<NL <= 3, ACT, FULL = 1> loads its W0-digit operands with inline
asm and waits on them with hand-counted ``s_waitcnt vmcnt`` (kernels_fxl.hip).  A
register spill of such an operand while its load is in flight would store
garbage, so those instantiations must compile without VGPR spills.  (CPU test:
hipcc cross-compiles gfx950 here.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")
SRC = os.path.join(CSRC, "kernels_fx.hip")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_counted_fxl_instantiations_do_not_spill(tmp_path):
    # the files that hold the kernels checked below, compiled side by side
    files = ("kernels_fxl", "kernels_fx", "kernels_fx_fwd")
    procs = [subprocess.Popen([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                               "-c", os.path.join(CSRC, f + ".hip"), "-o", str(tmp_path / (f + ".o")),
                               "-Rpass-analysis=kernel-resource-usage"],
                              stdout=subprocess.DEVNULL, stderr=open(tmp_path / (f + ".err"), "w")) for f in files]
    stderr = ""
    for f, p in zip(files, procs):
        rc = p.wait(timeout=600)
        err = open(tmp_path / (f + ".err")).read()
        assert rc == 0, err[-2000:]
        stderr += err
    spills, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
    counted = [k for k in spills if re.match(r"_Z16k_fused_grad_fxlILi[23]ELi\dELi1ELi8E", k)]
    assert len(counted) == 10, counted
    assert all(spills[k] == 0 for k in counted), {k: spills[k] for k in counted}
    # 4 chunks per wave: the digit operands stay in registers for the whole item
    resident = [k for k in spills if re.match(r"_Z16k_fused_grad_fxlILi[23]ELi\dELi[01]ELi4E", k)]
    assert len(resident) == 20, resident
    assert all(spills[k] == 0 for k in resident), {k: spills[k] for k in resident}
    fx = [k for k in spills if k.startswith("_Z15k_fused_grad_fx")]
    assert len(fx) == 60, len(fx)  # (a lost instantiation must not pass as "all of none")
    assert all(spills[k] == 0 for k in fx), {k: spills[k] for k in fx}
    fwd = [k for k in spills if k.startswith("_Z12k_forward_fx")]
    assert len(fwd) == 30, len(fwd)
    assert all(spills[k] == 0 for k in fwd), {k: spills[k] for k in fwd}


def test_production_build_sets_no_profiling_switches():
    """the fx kernel's profiling switches (FX_STAMPS phase stamps, FX_ABL ablations;
    tools/build_ab.sh builds variant libraries with them) default to 0 in the source
    and the product build (Makefile, __graft_entry__.build) defines none of them; the gx
    kernels have no compile-time switch at all, and the Makefile no gx ablation target"""
    txt = open(SRC).read()
    for sw in ("FX_STAMPS", "FX_ABL"):
        assert f"#ifndef {sw}\n#define {sw} 0\n#endif" in txt, sw
    mk = open(os.path.join(CSRC, "Makefile")).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "-DFX_" not in mk and "-DFX_" not in entry and "BANN_ABLATE" not in mk
    assert "-DGX_" not in mk and "-DGX_" not in entry and "ablate_gx" not in mk
    for f in sorted(os.listdir(CSRC)):
        if os.path.isfile(os.path.join(CSRC, f)) and not f.endswith((".o", ".so")):
            assert "#ifndef GX_" not in open(os.path.join(CSRC, f), errors="replace").read(), f


def test_makefile_srcs_is_the_only_source_list():
    """every HIP source of the library is in the Makefile's SRCS, and tools/build_ab.sh takes its
    list from there (print-srcs) instead of carrying one that can drift"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    on_disk = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted(srcs) == on_disk
    assert len(set(srcs)) == len(srcs)
    assert re.search(r"^print-srcs:", mk, re.M)
    ab = open(os.path.join(ROOT, "tools", "build_ab.sh")).read()
    assert "print-srcs" in ab
    names = [s[:-4] for s in srcs]
    for line in [l for l in mk.splitlines() if not l.startswith("SRCS = ")] + ab.splitlines():
        assert sum(1 for w in re.findall(r"\w+", line) if w in names) <= 1, line
