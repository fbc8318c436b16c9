"""Host-side checks of the batched unsupervised loss (no GPU): the two entries are exported, declared and bound with one
argument list; the grouping of a split; the per-layout block count; the sums, block count and layout views that the single and
the K-layout kernels share (csrc/loss_sums.h, many_desc.h) walked on the host under sanitizers; the tests' own fp64 restatement of "K losses"
(tests/loss_many_oracle.py) against the oracle on the reference's golden cases; the new keyword of the training loops; bad
arguments rejected before anything is queued."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import loss_many_oracle as lmo
from tests.test_oracle_vs_reference_golden import LOSS_CASES, _loss_case_inputs
from tests.test_solve_many_host import _ctype_of, _declarations

ENTRIES = ("tgnn_unsupervised_loss_many_workspace_bytes", "tgnn_unsupervised_loss_many")


def test_entries_are_exported_declared_and_bound():
    from tilingnn_amd import _lib
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, f"{name} is not declared in include/tgnn.h"
        res, args = decl[name]
        fn = getattr(_lib.lib, name)                                # (AttributeError: not exported by libtgnn.so)
        assert [_ctype_of(a) for a in args] == list(fn.argtypes), name
        assert fn.restype is {"int": C.c_int, "size_t": C.c_size_t}[res], name
        assert name in _lib.EXPORTED_SYMBOLS
    args = decl[ENTRIES[1]][1]
    assert args[0] == "int32_t n_layouts" and args[-1] == "tgnn_stream_t stream" and len(args) == 27


def test_grouping_helper():
    from tilingnn_amd.solver.ml_solver.trainer import eval_groups
    for n, g in ((0, 4), (1, 1), (7, 1), (7, 3), (7, 32), (64, 32), (65, 32)):
        got = [list(r) for r in eval_groups(n, g)]
        assert got == lmo.groups(n, g)
        assert [k for r in got for k in r] == list(range(n))        # contiguous, in order, nothing dropped
        assert len(got) == -(-n // g) and all(len(r) == g for r in got[:-1])
        assert not got or 1 <= len(got[-1]) <= g                    # the short last one is kept
    with pytest.raises(ValueError):
        eval_groups(5, 0)


def test_block_count_per_layout():
    want = {0: 1, 1: 1, 1024: 1, 1025: 2, 524288: 512, 524289: 512}
    for items, blocks in want.items():
        small = min(items, 3)
        for sizes in ((items, small, small), (small, items, small), (small, small, items)):
            assert lmo.loss_blocks(*sizes) == blocks, (sizes, blocks)
    for items in (2049, 300000, 10 ** 7):
        assert lmo.loss_blocks(5, items, 9) == min(max(-(-items // 1024), 1), 512)


def test_shared_sums_walked_on_the_host_under_sanitizers(tmp_path):
    """tests/host/loss_sums_test.cpp over csrc/loss_sums.h and many_desc.h -- what the single-layout and the K-layout kernels both
    call -- built with the host compiler alone under AddressSanitizer + UBSan (the runtime linked into the program itself):
    the block count at its boundaries in each position, the final formula, and 4 000 random packed sets with broken tables."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "loss_sums_test")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(repo, "tilingnn_amd", "csrc"),
                            os.path.join(repo, "tests", "host", "loss_sums_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    words = run.stdout.split()
    assert words[0] == "ok:" and words[2:4] == ["layouts", "walked,"], run.stdout
    walked, rejected, maps_bad, score_bad = int(words[1]), int(words[4]), int(words[11]), int(words[14])
    assert walked > 5000 and rejected > 100 and maps_bad > 100 and score_bad > 20, run.stdout


@pytest.mark.parametrize("name", LOSS_CASES)
def test_restatement_agrees_with_the_oracle(name):
    _, probs, x, col, adj, adj_attr = _loss_case_inputs(name)
    want = orc.unsupervised_losses(torch.from_numpy(probs), torch.from_numpy(x), torch.from_numpy(col), torch.from_numpy(adj),
                                   torch.from_numpy(adj_attr)).numpy()
    empty = (np.zeros((0, x.shape[1])), np.zeros((2, 0), np.int64), np.zeros((0, adj_attr.shape[1])), np.zeros((2, 0), np.int64))
    got = lmo.losses_many([empty, (x, adj, adj_attr, col), (x, adj, adj_attr, col)], [np.zeros((0, probs.shape[1])), probs, None])
    assert got[0] is None and got[2] is None
    losses, terms = got[1]
    assert losses.shape == want.shape and terms.shape == want.shape + (3,)
    assert np.abs(losses - want).max() < 1e-12 * np.abs(want).max()
    assert (terms <= 0).all()
    wc, wl, wa = lmo.WEIGHTS
    assert np.allclose((1 - wa * terms[:, 0]) * (1 - wc * terms[:, 1]) * (1 - wl * terms[:, 2]), losses, rtol=1e-15, atol=0)


def test_training_loops_take_eval_group():
    from tilingnn_amd.solver.ml_solver import trainer as tr
    from tilingnn_amd.solver.ml_solver.losses import Losses
    for fn in (tr.Trainer.train, tr.Trainer.train_batches):
        p = inspect.signature(fn).parameters
        assert "eval_group" in p and p["eval_group"].default is None
    sig = inspect.signature(tr.cal_avg_loss_many)
    assert list(sig.parameters) == ["network", "dataset_or_packed", "group", "union"]
    assert sig.parameters["group"].default == 32 and sig.parameters["union"].default is True
    sig = inspect.signature(Losses.unsupervised_losses_many)
    assert list(sig.parameters)[:8] == ["probs", "packed", "first", "count", "buffers", "counts", "active", "weights"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:8]] == [0, None, None, None, None, None]


def test_results_helper_mirrors_the_single_layout_checks():
    from tilingnn_amd.solver.ml_solver.losses import Losses
    losses = np.array([[1.5, 1.25, 2.0], [np.nan] * 3, [3.0, 1.0 + 2.0 ** -30, 1.75]])
    terms = -np.ones((3, 3, 3))
    terms[1] = np.nan
    res = Losses.results_many(losses, terms, np.zeros(3, np.int32), present=[True, False, True], first=10)
    assert res[1] is None
    loss, idx, host, t = res[0]
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(loss) == 1.25 and int(idx) == 1
    assert host.dtype == np.float32 and host.tolist() == [1.5, 1.25, 2.0] and t.shape == (3, 3)
    assert float(res[2][0]) == float(np.float32(1.0 + 2.0 ** -30)) == 1.0 and int(res[2][1]) == 1
    with pytest.raises(IndexError, match="layout 11"):               # NaN rows of a layout that was evaluated
        Losses.results_many(losses, terms, np.zeros(3, np.int32), first=10)
    with pytest.raises(IndexError, match="layout 12"):               # its error word
        Losses.results_many(losses, terms, np.array([0, 0, 1], np.int32), present=[True, False, True], first=10)
    bad = terms.copy()
    bad[0, 0, 0] = 0.5
    with pytest.raises(AssertionError):
        Losses.results_many(losses, bad, np.zeros(3, np.int32), present=[True, False, True])
    low = losses.copy()
    low[2, 0] = 0.5
    with pytest.raises(AssertionError):
        Losses.results_many(low, terms, np.zeros(3, np.int32), present=[True, False, True])


def test_arguments_are_checked_before_anything_is_queued():
    from tilingnn_amd import _lib
    lib = _lib.lib
    assert lib.tgnn_unsupervised_loss_many_workspace_bytes(32, 3) >= 32 * 3 * 512 * 3 * 8
    assert lib.tgnn_unsupervised_loss_many_workspace_bytes(0, 0) > 0
    none = [None] * 8
    call = lambda k, totals, m, ldp, lda: lib.tgnn_unsupervised_loss_many(k, *none[:4], *totals, *none[:2], ldp, m, None, lda, *none[:2], 1,
                                                                       None, 1.0, 1.0, 1.0, *none[:4], 0, None)
    assert call(-1, (0, 0, 0), 1, 1, 1) == -1 and b"number of layouts" in lib.tgnn_last_error()
    assert call(2, (2 ** 31, 0, 0), 1, 1, 1) == -1 and b"totals" in lib.tgnn_last_error()
    assert call(2, (10, 0, -1), 1, 1, 1) == -1
    for m in (0, 65536):
        assert call(2, (10, 0, 0), m, 65536, 1) == -1 and b"maps" in lib.tgnn_last_error()
    assert call(2, (10, 0, 0), 3, 2, 1) == -1                         # rows of 2 floats cannot hold 3 maps
    assert call(2, (10, 0, 0), 1, 1, 0) == -1                         # ld_area 0
    assert call(2, (10, 0, 0), 1, 1, 1) == -1 and b"offset table" in lib.tgnn_last_error()
    assert call(0, (0, 0, 0), 1, 1, 1) == 0                           # an empty batch is no work and no error
    # tables given, outputs missing; then everything given but the workspace
    tab = (C.c_int64 * 3)(0, 5, 10)
    p = C.cast(tab, C.c_void_p)
    full = lambda ws, ws_bytes: lib.tgnn_unsupervised_loss_many(2, None, p, p, p, 10, 0, 0, None, p, 1, 1, p, 1, None, None, 1, None, 1.0, 1.0,
                                                               1.0, p, None, p, ws, ws_bytes, None)
    assert lib.tgnn_unsupervised_loss_many(2, None, p, p, p, 10, 0, 0, None, p, 1, 1, p, 1, None, None, 1, None, 1.0, 1.0, 1.0, None, None, p,
                                           None, 0, None) == -1 and b"null pointer" in lib.tgnn_last_error()
    assert full(None, 0) != 0 and b"workspace" in lib.tgnn_last_error()
    assert full(p, 64) != 0 and b"workspace" in lib.tgnn_last_error()
