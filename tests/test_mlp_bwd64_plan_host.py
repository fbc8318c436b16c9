"""The plan of the width-64 tall adjoint (tilingnn_amd/csrc/mlp_bwd64_plan.h: predicate, grid, tile share, partial-row layout,
workspace) on the CPU: tests/host/mlp_bwd64_plan_test.cpp built with the host compiler alone under AddressSanitizer + UBSan, and
the same queries through the library's C ABI (host code only: no GPU is touched)."""
import os
import re
import shutil
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = (32 * 64 + 32 + 64 * 32 + 64 + 64 * 64 + 64) * 4       # bytes of one block's partial row


def test_mlp_bwd64_plan_host_program():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # (the sanitizers' runtime linked into the program itself: it then runs under whatever the environment preloads)
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mlp_bwd64_plan_test")
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(REPO, "include"),
                                "-I", os.path.join(REPO, "tilingnn_amd", "csrc"),
                                os.path.join(REPO, "tests", "host", "mlp_bwd64_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 12 sizes x (1 + 7 + 8 + 16 + 157 + 224 + 256 + the planned grid: 1, 1, 1, 1, 2, 2, 3, 20, 65, 256, 256, 256) blocks x 4 waves;
    # 8 row counts x 6 x 3 x 3 x 4 dims
    assert re.search(r"mlp_bwd64_plan_test: 35568 tile shares, 12 grids, 1728 shapes, 0 failures", run.stdout), run.stdout


def test_predicate_and_workspace_queries_answer_through_the_c_abi():
    from tilingnn_amd._lib import lib
    ok, ws = lib.tgnn_sigmoid_mlp_bwd_tall64_ok, lib.tgnn_sigmoid_mlp_bwd_tall64_workspace_bytes
    assert ok(1254, 64, 32, 64, 64) == 1 and ok(1, 64, 32, 64, 64) == 1 and ok(0, 64, 32, 64, 64) == 1      # no row floor
    assert ok(2000000, 64, 32, 64, 64) == 1
    for n, dims in [(1254, (32, 32, 64, 32)), (1254, (64, 32, 64, 32)), (1254, (64, 64, 64, 64)), (-1, (64, 32, 64, 64)),
                    (13, (15, 32, 64, 4096)), (1254, (64, 32, 32, 64))]:
        assert ok(n, *dims) == 0 and ws(n, *dims) == 0, (n, dims)
    assert ROW % 256 != 0                                    # (so the rounding below is exercised)
    up = lambda b: (b + 255) // 256 * 256
    assert ws(1, 64, 32, 64, 64) == up(ROW) and ws(1254, 64, 32, 64, 64) == up(20 * ROW)
    assert ws(4099, 64, 32, 64, 64) == up(65 * ROW) and ws(16320, 64, 32, 64, 64) == up(255 * ROW)
    assert ws(16321, 64, 32, 64, 64) == ws(100000, 64, 32, 64, 64) == ws(2000000, 64, 32, 64, 64) == up(256 * ROW)
    # the older queries keep refusing the shape, and the switch is off by default
    assert lib.tgnn_sigmoid_mlp_bwd_fused_form(1254, 64, 32, 64, 64, 1) == 0
    assert lib.tgnn_sigmoid_mlp_bwd_fused_workspace_bytes(1254, 64, 32, 64, 64) == 0
    assert lib.tgnn_set_mlp_bwd_tall64(-1) == 0
