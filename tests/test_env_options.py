"""The BANN_* switches: one reader, called once per context (csrc/env_options.h).

CPU tests: the reader's defaults and parsing, checked by a stand-alone host program
(env_options_check.cpp) built here with the host C++ compiler, and the rule that no
other library source consults the environment."""
import glob
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-bann_amd", "csrc")


def test_read_env_options_defaults_and_parsing(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "env_options_check")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                          os.path.join(ROOT, "tests", "env_options_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr[-2000:]


def test_only_the_reader_consults_the_environment():
    """every getenv of the library sits in read_env_options, but for bann_net.cpp's one
    commented read of BANN_HMC_GRAPH (built without HIP, it sees the context through the C ABI)"""
    hits = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not path.endswith((".hip", ".h", ".cpp")):
            continue
        for i, line in enumerate(open(path).read().splitlines(), 1):
            if re.search(r"\bgetenv\s*\(", line):
                hits.append((os.path.basename(path), i, line.strip()))
    outside = [h for h in hits if h[0] != "env_options.h"]
    assert [h[0] for h in outside] == ["bann_net.cpp"] and "BANN_HMC_GRAPH" in outside[0][2], outside
