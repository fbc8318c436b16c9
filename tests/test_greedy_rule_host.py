"""Host side of the shared acceptance rule (csrc/greedy_rule.h): the functions the single-layout and the K-layout greedy kernels
both call run on the host under sanitizers (tests/host/greedy_rule_test.cpp: one round in the kernels' order, the finishing
block's phases with the header's flag constants, the draw), on case tables that tests/test_greedy_ops.py builds for the GPU
tests, against the host restatement (tests/greedy_restatement.py) under that file's comparison rule: decisions, alive, selected,
the counts and `out` equal, `saved` within RTOL_SAVED.  The draw is integer arithmetic and one exact multiply: bit-equal."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import greedy_restatement as gr
from tests import test_greedy_ops as ops

ROUND_SIZES = (1, 63, 64, 65, 257)
FINISH_SIZES = (1, 3, 4, 5, 1025)                            # 3, 4, 5: the tail of the 4-bytes-per-word flags
VARIANTS = {"both", "loops_dups", "oneway", "oob"}


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    """tests/host/greedy_rule_test.cpp, built with the host compiler alone under AddressSanitizer + UBSan (the sanitizers'
    runtime linked into the program itself), the way tests/test_hole_sweep_host.py builds its program."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("greedy_rule") / "greedy_rule_test")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(repo, "tilingnn_amd", "csrc"),
                            os.path.join(repo, "tests", "host", "greedy_rule_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _record(kind, n_sub, inverse, col, rnd, max_rounds, prob, seed, saved, alive, selected):
    ec = 0 if col is None else int(col.shape[1])
    parts = [struct.pack("<8qQ", kind, n_sub, len(saved), int(inverse is not None), ec, rnd, max_rounds, int(prob is not None),
                         int(seed) % (1 << 64))]
    if inverse is not None:
        parts.append(np.ascontiguousarray(inverse, dtype=np.int64).tobytes())
    if col is not None:
        parts.append(np.ascontiguousarray(col, dtype=np.int64).tobytes())
    if prob is not None:
        parts.append(np.ascontiguousarray(prob, dtype=np.float32).tobytes())
    parts += [np.ascontiguousarray(saved, dtype=np.float64).tobytes(), np.ascontiguousarray(alive, dtype=np.int32).tobytes(),
              np.ascontiguousarray(selected, dtype=np.int32).tobytes()]
    return b"".join(parts), len(saved)


def _run(exe, tmp_path, records):
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(records)))
        for blob, _ in records:
            f.write(blob)
    run = subprocess.run([exe, path, out], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.split() == ["cases", str(len(records))]
    raw, at, results = open(out, "rb").read(), 0, []
    for _, n in records:
        saved = np.frombuffer(raw, np.float64, n, at)
        alive = np.frombuffer(raw, np.int32, n, at + 8 * n)
        selected = np.frombuffer(raw, np.int32, n, at + 12 * n)
        tail = np.frombuffer(raw, np.int64, 4, at + 16 * n)
        results.append((saved, alive, selected, [int(t) for t in tail]))
        at += 16 * n + 32
    assert at == len(raw)
    return results


def _hold(name, got, want, rounds_run=0, left=0, compare_saved=True):
    saved, alive, selected, tail = got
    assert want.margins.undecidable == 0, (name, want.margins)     # (a condition on the inputs)
    assert np.array_equal(alive, want.alive), f"{name}: alive differs at {np.flatnonzero(alive != want.alive)[:8]}"
    assert np.array_equal(selected, want.selected), f"{name}: selected differs at {np.flatnonzero(selected != want.selected)[:8]}"
    assert tail == [want.accepted, want.err, rounds_run, left], (name, tail)
    if compare_saved:
        np.testing.assert_allclose(saved, want.saved, rtol=ops.RTOL_SAVED, atol=0.0, err_msg=name)


def test_one_round_on_the_host_is_the_restated_round(rule_program, tmp_path):
    cases = [ops.round_case(k) for k in ops.ROUND_SPECS if ops.ROUND_SPECS[k][0] in ROUND_SIZES]
    assert {c.n for c in cases} == set(ROUND_SIZES) and {c.variant for c in cases} >= VARIANTS
    for n in ROUND_SIZES:
        assert {c.inverse is None for c in cases if c.n == n} == {True, False}
    records = [_record(0, c.n, c.inverse, c.col, c.rnd, 0, c.prob[:, c.column], c.seed, c.saved, c.alive, c.selected) for c in cases]
    for c, got in zip(cases, _run(rule_program, tmp_path, records)):
        _hold(c.name, got, c.want())
        assert c.want().err == int(c.variant == "oob")
    assert sum(c.want().accepted for c in cases) > 100


def test_the_finish_phases_on_the_host_are_the_restated_rounds(rule_program, tmp_path):
    cases = [ops.finish_case(k) for k in ops.FINISH_SPECS if ops.FINISH_SPECS[k][0] in FINISH_SIZES]
    cases += [ops.finish_case(k) for k in ops.BUDGET_SPECS if ops.BUDGET_SPECS[k][0] in FINISH_SIZES]
    # out-of-range ends in the finish as well (the GPU tables keep them to the round entry)
    cases += [ops.build_finish_case(f"n{n}-oob", n, 2, n == 1025, 0.3, "oob", ops.SEEDS[1], 1000, 2900 + n) for n in (5, 1025)]
    assert {c.n for c in cases} == set(FINISH_SIZES) and {c.variant for c in cases} >= VARIANTS
    records = [_record(1, c.n, c.inverse, c.col, c.first_round, c.max_rounds, None, c.seed, c.saved, c.alive, c.selected) for c in cases]
    for c, got in zip(cases, _run(rule_program, tmp_path, records)):
        w = c.want()
        # (with the budget spent the walk, like the kernel, has folded the next round's mean into saved already)
        _hold(c.name, got, w, w.rounds_run, w.left, compare_saved=w.left == 0)
        assert w.err == int(c.variant == "oob")
    assert any(c.want().left > 0 for c in cases) and max(c.want().rounds_run for c in cases) >= 5


def test_the_draw_is_bit_equal_to_the_restated_draw(rule_program, tmp_path):
    nodes = np.unique(np.concatenate([np.arange(260), 2 ** np.arange(41), 2 ** np.arange(1, 41) - 1])).astype(np.int64)
    assert nodes[0] == 0 and nodes[-1] == 2 ** 40 and len(nodes) > 300
    keys = [(seed, rnd) for seed in ops.SEEDS for rnd in ops.ROUNDS]
    zeros = np.zeros(len(nodes))
    records = [_record(2, len(nodes), nodes, None, rnd, 0, None, seed, zeros, zeros, zeros) for seed, rnd in keys]
    for (seed, rnd), (got, _, _, _) in zip(keys, _run(rule_program, tmp_path, records)):
        want = gr.uniform(seed, rnd, nodes)
        assert got.tobytes() == want.tobytes(), (seed, rnd, np.flatnonzero(got != want)[:8])
