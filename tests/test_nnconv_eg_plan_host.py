"""The edge-group NNConv's plan (tilingnn_amd/csrc/nnconv_eg_plan.h: the block count, the tile share of every wave for blocks of 8,
12 and 16 waves, the footprint table of the layer loop's kernels) on the CPU: tests/host/nnconv_eg_plan_test.cpp built with the host
compiler alone under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nnconv_eg_wave_shares_block_count_and_footprints_host_program():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # (the sanitizers' runtime linked into the program itself: it then runs under whatever the environment preloads)
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "nnconv_eg_plan_test")
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(REPO, "include"),
                                "-I", os.path.join(REPO, "tilingnn_amd", "csrc"),
                                os.path.join(REPO, "tests", "host", "nnconv_eg_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 301 tile counts (1 .. 300 and 6 250) x (1 + 7 + 8 + 9 + 64 + 224 + 256) blocks x (8 + 12 + 16) waves
    assert re.search(r"nnconv_eg_plan_test: 6165684 wave shares \(\d+ empty\), 4 footprints, 1 pair, 0 failures", run.stdout), run.stdout
