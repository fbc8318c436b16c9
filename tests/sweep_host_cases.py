"""What tests/test_hole_sweep_host.py and tests/test_tree_search_host.py share: the hand-made sets and their scripted collision
rows, the sanitizer build of a stand-alone walk program of tests/host/, and the writer of the case file both programs read
(tests/host/sweep_host.h)."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np

SETS = ("frame with a plus inside", "plus among four squares", "3x3 full")
# what an acceptance labels besides the node (a layout's collision rows; the sets themselves have none): symmetric, and one
# entry twice
NBR = {5: {0: [2, 2], 2: [0]}, 9: {0: [8, 8], 8: [0], 2: [6], 6: [2]}}


def build_step_program(tmp_path_factory, name):
    """tests/host/<name>.cpp, built with the host compiler alone under AddressSanitizer + UBSan (the sanitizers' runtime linked
    into the program itself), the way tests/test_union_hole_delta_host.py builds its program."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp(name) / name)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(repo, "tilingnn_amd", "csrc"),
                            os.path.join(repo, "tests", "host", name + ".cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def nbr_csr(n):
    rows = NBR[n]
    ptr = np.zeros(n + 1, dtype=np.int32)
    for i in range(n):
        ptr[i + 1] = ptr[i] + len(rows.get(i, ()))
    idx = np.array([v for i in range(n) for v in rows.get(i, ())], dtype=np.int32)
    return ptr, idx


def run_program(exe, tmp_path, tiles, want, orders, rate, more_head=()):
    """Writes the case file -- rate: thr or p by position; more_head: the program's head words behind the common five -- and runs
    the program on it.  Returns the words of its stdout line and the int32 words it wrote."""
    from tilingnn_amd.tiling.region import UNION_TOL, contact_geometry, sweep_direction, union_geometry
    n = len(tiles)
    ring_xy, ring_ptr, _, _ = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), n)
    touch_ptr, touch_idx = contact_geometry(ring_xy, ring_ptr)
    theta = sweep_direction(ring_xy, ring_ptr)
    nbr_ptr, nbr_idx = nbr_csr(n)
    path, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack(f"<{5 + len(more_head)}q3d", n, ring_xy.shape[0], touch_idx.shape[0], nbr_idx.shape[0], orders.shape[0],
                            *more_head, UNION_TOL, math.cos(theta), math.sin(theta)))
        for a in (ring_xy, ring_ptr, touch_ptr, touch_idx, nbr_ptr, nbr_idx, want.astype(np.int32), np.array(rate[:n]),
                  orders.astype(np.uint8)):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, path, out], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    return run.stdout.strip().split(), np.fromfile(out, dtype=np.int32)
