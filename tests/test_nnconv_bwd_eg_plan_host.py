"""The plan of the edge-group NNConv adjoint (tilingnn_amd/csrc/nnconv_bwd_eg_plan.h: predicate, dW grid, shares of the type-major
list, partial slots, workspace) on the CPU: tests/host/nnconv_bwd_eg_plan_test.cpp built with the host compiler alone under
AddressSanitizer + UBSan, and the same queries through the library's C ABI (host code only: no GPU is touched)."""
import os
import re
import shutil
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nnconv_bwd_eg_plan_host_program():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # (the sanitizers' runtime linked into the program itself: it then runs under whatever the environment preloads)
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "nnconv_bwd_eg_plan_test")
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(REPO, "include"),
                                "-I", os.path.join(REPO, "tilingnn_amd", "csrc"),
                                os.path.join(REPO, "tests", "host", "nnconv_bwd_eg_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 12 list lengths x 8 caps; 18 + 22 workspaces
    m = re.search(r"nnconv_bwd_eg_plan_test: (\d+) shares, 96 grids, (\d+) slots, 40 workspaces, (\d+) predicates, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 96 and int(m.group(2)) > 1000 and int(m.group(3)) >= 20, run.stdout


def test_predicate_and_workspace_queries_answer_through_the_c_abi():
    from tilingnn_amd._lib import lib
    ok, ws = lib.tgnn_nnconv_bwd_eg_ok, lib.tgnn_nnconv_bwd_eg_workspace_bytes
    assert ok(64, 1254, 18, 12, 12, 1, 1) == 1 and ok(64, 1254, 19, 12, 12, 1, 1) == 0
    assert ok(32, 1254, 22, 12, 12, 1, 1) == 1 and ok(32, 1254, 23, 12, 12, 1, 1) == 0
    assert lib.tgnn_nnconv64_eg_max_types() == 18 and lib.tgnn_nnconv_cols_max_types() == 22
    assert ok(32, 1254, 13, 2048, 2048, 1, 1) == 1 and ok(32, 1254, 13, 2049, 12, 1, 1) == 0 and ok(32, 1254, 13, 12, 2049, 1, 1) == 0
    assert ok(16, 1254, 13, 12, 12, 1, 1) == 0 and ok(128, 1254, 13, 12, 12, 1, 1) == 0
    assert ok(32, 1254, 13, 12, 12, 0, 1) == 0 and ok(32, 1254, 13, 12, 12, 1, 0) == 0
    assert ok(64, (1 << 23) - 1, 13, 12, 12, 1, 1) == 1 and ok(64, 1 << 23, 13, 12, 12, 1, 1) == 0
    up = lambda b: (b + 255) // 256 * 256
    for c, image in ((32, 4096), (64, 16384)):
        for T in (1, 13, 18):
            want = 256 + up((T + 1) * c * c * 4) + up((T + 1) * image) + up((512 + T + 1) * c * c * 4)
            assert ws(1254, 2000, T, c) == want == ws(100000, 200000, T, c), (c, T)
    for n, cap, T, c in [(1254, 2000, 19, 64), (1254, 2000, 23, 32), (1254, 2000, 13, 16), (1254, 2000, 13, 128), (0, 2000, 13, 32)]:
        assert ws(n, cap, T, c) == 0, (n, cap, T, c)
    assert lib.tgnn_nnconv_bwd_eg_dw_blocks(0) == 1 and lib.tgnn_nnconv_bwd_eg_dw_blocks(17) == 2
    assert lib.tgnn_nnconv_bwd_eg_dw_blocks(8176) == 511 and lib.tgnn_nnconv_bwd_eg_dw_blocks(8177) == 512 == lib.tgnn_nnconv_bwd_eg_dw_blocks(10 ** 6)
    assert lib.tgnn_nnconv_bwd_eg_list_ints(2000) == 64 + 4000
    # the switch is off by default, and a query leaves it so
    assert lib.tgnn_set_nnconv_bwd_eg(-1) == 0 and lib.tgnn_set_nnconv_bwd_eg(7) == 0 and lib.tgnn_set_nnconv_bwd_eg(-1) == 0


def test_backward_workspace_covers_the_edge_group_route_whatever_the_switch_says():
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import lib
    import ctypes as C
    for c in (32, 64):
        dims = _lib.ModelDims()
        dims.network_width, dims.network_depth, dims.node_features_dim, dims.adj_edge_features_dim, dims.output_dim = c, 3, 1, 1, 1
        a = lib.tgnn_backward_workspace_bytes(C.byref(dims), 1254, 13)
        assert lib.tgnn_set_nnconv_bwd_eg(1) == 0
        try:
            b = lib.tgnn_backward_workspace_bytes(C.byref(dims), 1254, 13)
        finally:
            lib.tgnn_set_nnconv_bwd_eg(0)
        assert a == b and a > lib.tgnn_nnconv_bwd_eg_workspace_bytes(1254, 0, 13, c) > 0
