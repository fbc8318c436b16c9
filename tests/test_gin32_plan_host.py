"""The width-32 GINConv's plan (tilingnn_amd/csrc/gin32_plan.h: the choice between its three forms, the block count, the tile share
of a wave or team) on the CPU: tests/host/gin32_plan_test.cpp built with the host compiler alone under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gin32_tile_share_block_count_and_variant_choice_host_program():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # (the sanitizers' runtime linked into the program itself: it then runs under whatever the environment preloads)
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gin32_plan_test")
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(REPO, "include"),
                                "-I", os.path.join(REPO, "tilingnn_amd", "csrc"),
                                os.path.join(REPO, "tests", "host", "gin32_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 13 sizes x (1 + 2 + 7 + 8 + 16 + 24 + 224) blocks x 4 SIMD slots x (1 team + 2 waves); 19 rows of the hand-written table
    assert re.search(r"gin32_plan_test: 43992 tile shares, 19 choices, 0 failures", run.stdout), run.stdout
