"""The plan of the fused sigmoid-MLP adjoints (tilingnn_amd/csrc/mlp_bwd_plan.h: form predicate, tall grid and tile share, workspace)
on the CPU: tests/host/mlp_bwd_plan_test.cpp built with the host compiler alone under AddressSanitizer + UBSan, and the same
queries through the library's C ABI (host code only: no GPU is touched)."""
import os
import re
import shutil
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mlp_bwd_plan_host_program():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # (the sanitizers' runtime linked into the program itself: it then runs under whatever the environment preloads)
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mlp_bwd_plan_test")
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(REPO, "include"),
                                "-I", os.path.join(REPO, "tilingnn_amd", "csrc"),
                                os.path.join(REPO, "tests", "host", "mlp_bwd_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 12 sizes x (1 + 7 + 8 + 16 + 157 + 224 + 256 + the planned grid: 1, 1, 1, 1, 2, 2, 3, 20, 65, 256, 256, 256) blocks x 8 waves
    assert re.search(r"mlp_bwd_plan_test: 71136 tile shares, 12 grids, 2520 forms, 0 failures", run.stdout), run.stdout


def test_form_and_workspace_queries_answer_through_the_c_abi():
    from tilingnn_amd._lib import lib
    form, fused_ws, chain_ws = (lib.tgnn_sigmoid_mlp_bwd_fused_form, lib.tgnn_sigmoid_mlp_bwd_fused_workspace_bytes,
                                lib.tgnn_sigmoid_mlp_bwd_workspace_bytes)
    assert form(1254, 32, 32, 64, 32, 1) == 1 and form(1, 32, 32, 64, 32, 0) == 1
    assert form(13, 15, 32, 64, 1024, 0) == 2 and form(63, 64, 32, 64, 4096, 0) == 2
    assert form(1254, 64, 32, 64, 64, 1) == 0 and form(64, 15, 32, 64, 1024, 0) == 0
    assert form(13, 65, 32, 64, 1024, 0) == 0 and form(13, 15, 32, 64, 1024, 1) == 0
    row = (32 * 32 + 32 + 64 * 32 + 64 + 32 * 64 + 32) * 4
    assert fused_ws(1254, 32, 32, 64, 32) == 20 * row and fused_ws(100000, 32, 32, 64, 32) == 256 * row
    assert fused_ws(13, 15, 32, 64, 1024) == 16 * 13 * 64 * 4 and fused_ws(63, 64, 32, 64, 4096) == 64 * 63 * 64 * 4
    assert fused_ws(1254, 64, 32, 64, 64) == 0 and fused_ws(64, 15, 32, 64, 1024) == 0
    assert chain_ws(1254, 32, 32, 64, 32) > 0 and chain_ws(13, 15, 32, 64, 1024) > 0
