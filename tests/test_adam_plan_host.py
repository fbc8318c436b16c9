"""The fused Adam step on the CPU: its host plan (tilingnn_amd/csrc/adam_plan.h: moment layout, chunk list, the checks a launch
relies on) through tests/host/adam_plan_test.cpp, built with the host compiler alone, plain and under AddressSanitizer + UBSan;
and the gates of tests/adam_cases.py pointed at torch's own CPU Adam(foreach=False), so that they are known to be passable by the
reference before tests/test_adam_fused.py points them at the kernel."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests import adam_cases as ac

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_adam_plan_tiles_segments_and_refuses_bad_tables_host_program(sanitize):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    flags = []
    if sanitize:
        # (the sanitizers' runtime linked into the program itself: it then runs under whatever the environment preloads)
        clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                 *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"])]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "adam_plan_test")
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                                "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tilingnn_amd", "csrc"),
                                os.path.join(REPO, "tests", "host", "adam_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 2 tables of all 13 sizes + 13 x (alone, between two vectors) + the network-shaped one; chunks: 2 x 58 + 13 x 2 alone-or-not ...
    m = re.search(r"adam_plan_test: (\d+) plans, (\d+) chunks, (\d+) refusals, 0 failures", run.stdout)
    assert m, run.stdout
    per_table = sum(-(-ac.numel(s) // ac.CHUNK) for s in ac.SIZES)
    assert int(m.group(1)) == 2 + 2 * len(ac.SIZES) + 1
    assert int(m.group(2)) == 2 * per_table + sum(2 * -(-ac.numel(s) // ac.CHUNK) + 2 for s in ac.SIZES) + 342
    assert int(m.group(3)) >= 20


def test_chunk_size_restated_in_the_cases_matches_the_header():
    text = open(os.path.join(REPO, "tilingnn_amd", "csrc", "adam_plan.h")).read()
    assert int(re.search(r"constexpr int64_t kAdamChunk = (\d+);", text).group(1)) == ac.CHUNK
    assert int(re.search(r"constexpr int64_t kAdamMomentAlign = (\d+);", text).group(1)) == 64


@pytest.mark.parametrize("t", ac.STEPS)
@pytest.mark.parametrize("lr", ac.LRS)
def test_gates_hold_for_torch_cpu_adam(t, lr):
    """torch.optim.Adam(foreach=False) on the CPU, one step from the tests' inputs, against the fp64 expectation: inside every
    gate the kernel is held to (weight_decay 0)."""
    ps, gs, ms, vs = ac.make_inputs(seed=3 + t % 7, t=t)
    got_p, got_m, got_v = ac.torch_adam_step(ps, gs, ms, vs, t, lr)
    worst = np.zeros(3)
    for k in range(len(ps)):
        want = ac.adam64(ps[k], gs[k], ms[k], vs[k], t, lr)
        worst = np.maximum(worst, ac.assert_within_gates(got_p[k], got_m[k], got_v[k], want, f"torch CPU Adam, tensor {k}, t {t}, lr {lr}"))
    print(f"t {t}, lr {lr}: torch CPU Adam's worst error / gate = p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")


def test_gate_code_itself_notices_an_error():
    """The gate helper is not vacuous: one ulp-sized nudge passes, a relative error of 1e-5 on one element does not."""
    ps, gs, ms, vs = ac.make_inputs(seed=1, t=10)
    k = len(ac.SIZES) - 1
    want = ac.adam64(ps[k], gs[k], ms[k], vs[k], 10, 1e-2)
    good = [want[key].astype(np.float32) for key in ("p", "m", "v")]
    assert max(ac.gate_ratios(*good, want)) <= 1.0
    for which in range(3):
        bad = [a.copy() for a in good]
        flat = bad[which].reshape(-1)
        j = int(np.argmax(np.abs(flat)))
        flat[j] *= np.float32(1.0 + 1e-5)
        assert ac.gate_ratios(*bad, want)[which] > 1.0
    # an element whose gate is exactly zero (zero gradient on zero moments) must be reproduced exactly
    z = ac.adam64(np.ones(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32), 1, 1e-2)
    assert np.all(z["tau_m"] == 0) and ac.gate_ratios(z["p"], z["m"] + 1e-30, z["v"], z)[1] == np.inf


def _host_table(numel, moment_floats=None, params=None):
    """tgnn_adam_table_build into a numpy buffer -> (rc, buffer, n_chunks); moments laid out slice after slice."""
    import ctypes as C
    from tilingnn_amd._lib import lib
    n = len(numel)
    arr = C.c_int64 * max(n, 1)
    moff, off = [], 0
    for v in numel:
        moff.append(off)
        off += (max(v, 0) + 63) // 64 * 64
    n_chunks = int(lib.tgnn_adam_chunk_count(arr(*numel), n))
    buf = np.zeros(max(int(lib.tgnn_adam_table_bytes(n, max(n_chunks, 0))), 8) // 8, dtype=np.int64)
    out = C.c_int64(-1)
    rc = lib.tgnn_adam_table_build((C.c_void_p * max(n, 1))(*(params or [0x1000 * (k + 1) for k in range(n)])), arr(*[256 * k for k in range(n)]),
                                   arr(*moff), arr(*numel), n, off if moment_floats is None else moment_floats, buf.ctypes.data,
                                   buf.nbytes, C.byref(out))
    return rc, buf, int(out.value), off


def test_c_abi_builds_the_table_and_refuses_bad_ones_before_any_launch():
    """tgnn_adam_table_build and the argument checks of tgnn_adam_step on the host (nothing is queued: every call here ends in a
    refusal or has no chunk to run; the device pointers are null on purpose, so that a check that failed to fire could not launch)."""
    from tilingnn_amd._lib import lib
    INVALID = -1
    assert lib.tgnn_adam_chunk_elems() == ac.CHUNK
    numel = [ac.numel(s) for s in ac.SIZES]
    rc, buf, n_chunks, mfloats = _host_table(numel)
    assert rc == 0 and n_chunks == sum(-(-v // ac.CHUNK) for v in numel)
    assert int(lib.tgnn_adam_table_bytes(len(numel), n_chunks)) == 32 * len(numel) + 16 * n_chunks == buf.nbytes
    segs = buf[:4 * len(numel)].reshape(-1, 4)
    assert segs[:, 3].tolist() == numel and segs[:, 1].tolist() == [256 * k for k in range(len(numel))]
    assert np.all(segs[:, 2] % 64 == 0) and np.all(np.diff(segs[:, 2]) >= np.array(numel[:-1]))
    chunks = buf[4 * len(numel):].reshape(-1, 2)
    covered = np.zeros(len(numel), dtype=np.int64)
    for start, seg in chunks.tolist():
        assert 0 <= seg < len(numel) and start == covered[seg]                       # ascending, gap-free inside a segment
        covered[seg] = min(start + ac.CHUNK, numel[seg])
    assert covered.tolist() == numel
    # refusals of the builder
    assert _host_table([4, -1])[0] == INVALID
    assert b"negative" in lib.tgnn_last_error()
    assert _host_table([4, 8], params=[0x1000, 0])[0] == INVALID                     # a null parameter with elements
    assert _host_table([4, 0], params=[0x1000, 0])[0] == 0                           # ... without: fine
    assert _host_table([4, 8], moment_floats=71)[0] == INVALID                       # second slice ends at 72
    assert _host_table([4, 8], moment_floats=-1)[0] == INVALID

    def step(table, n_seg, n_ch, mf):
        return lib.tgnn_adam_step(table.ctypes.data, None, n_seg, n_ch, None, None, None, mf, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, None)
    # the intact image reaches the device-pointer check; a corrupted one is refused for what is wrong with it
    assert step(buf, len(numel), n_chunks, mfloats) == INVALID and b"null pointer" in lib.tgnn_last_error()
    assert step(buf, len(numel), 0, mfloats) == 0                                    # no chunk: nothing to queue
    assert step(buf, -1, n_chunks, mfloats) == INVALID and step(buf, len(numel), -1, mfloats) == INVALID
    assert step(buf, len(numel), n_chunks, -1) == INVALID
    for word, value, why in ((0, numel[-1], b"outside its segment"),                  # start == numel of the last segment
                             (0, -ac.CHUNK, b"outside its segment"),
                             (0, 4, b"multiple of the chunk"),
                             (1, len(numel), b"outside the table"),                   # (segment in the low half of word 1)
                             (1, 0xffffffff, b"outside the table")):                  # segment -1
        bad = buf.copy()
        bad[4 * len(numel) + 2 * (n_chunks - 1) + word] = value
        assert step(bad, len(numel), n_chunks, mfloats) == INVALID and why in lib.tgnn_last_error(), (word, value)
    bad = buf.copy()
    bad[4 * (len(numel) - 1) + 2] += mfloats                                         # the last moment slice behind the buffers
    assert step(bad, len(numel), n_chunks, mfloats) == INVALID and b"moment slice" in lib.tgnn_last_error()
    bad = buf.copy()
    bad[4 * 3 + 0] = 0                                                               # null parameter of a 4-element segment
    assert step(bad, len(numel), n_chunks, mfloats) == INVALID and b"null parameter" in lib.tgnn_last_error()
