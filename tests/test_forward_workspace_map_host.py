"""tgnn_forward_workspace_map (csrc/forward.hip): the byte offsets of the forward workspace's pieces that tests read -- the carve itself
on a null base, host only.  What the GPU tests that slice the workspace assume, checked without a GPU."""
import ctypes as C

import pytest

from tilingnn_amd import _lib

WORDS = (2 * 64 + 100) * 4       # bytes of the bounds words: 2 * kMaxDepth + 100 (csrc/forward.hip: carve)


@pytest.mark.parametrize("width,depth", [(32, 4), (32, 20), (32, 64), (64, 20), (96, 3)])
@pytest.mark.parametrize("n,halo", [(2, 0), (1237, 0), (1237, 411), (49152, 0), (100000, 0)])
def test_offsets_increase_start_at_zero_and_stay_inside_the_workspace(width, depth, n, halo):
    dims = _lib.ModelDims(3, 15, width, depth, 1)
    nr = n + halo
    m = _lib.forward_workspace_map(dims, n, nr, 13)
    total = _lib.lib.tgnn_forward_sharded_workspace_bytes(C.byref(dims), n, nr, 13)
    assert total > 0
    if halo == 0:
        assert total == _lib.lib.tgnn_forward_workspace_bytes(C.byref(dims), n, 13)
    assert m["mid"] == 0                                          # (what tests/test_small_layout.py, test_mid_layout.py slice from)
    order = [m[k] for k in ("mid", "a1", "f1", "f2", "f3", "bounds")]
    assert order == sorted(set(order)), m
    assert m["a1"] >= (depth + 1) * nr * width * 4                # the skip buffer has nr rows per slot
    assert m["f2"] - m["f1"] >= n * 256 * 4 and m["f3"] - m["f2"] >= n * 128 * 4
    assert m["bounds"] + WORDS <= total
    assert all(v % 256 == 0 for v in order)
    if width == 64:
        assert m["bounds64"] > m["bounds"] and m["bounds64"] + 2 * 64 * 4 <= total
    else:
        assert m["bounds64"] == -1


@pytest.mark.parametrize("width", [32, 64])
def test_no_piece_moves_with_the_type_count_up_to_sixteen(width):
    """tgnn_forward_begin carves with 0 types and fills its pieces before the preparation has counted them."""
    dims = _lib.ModelDims(3, 15, width, 20, 1)
    maps = [_lib.forward_workspace_map(dims, 40000, 40000, t) for t in range(17)]
    assert all(m == maps[0] for m in maps)
    assert _lib.forward_workspace_map(dims, 40000, 40000, 17)["bounds"] > maps[0]["bounds"]   # (and it does move beyond)


def test_bad_arguments_are_refused():
    dims = _lib.ModelDims(3, 15, 32, 4, 1)
    out = (C.c_int64 * 7)()
    assert _lib.lib.tgnn_forward_workspace_map(C.byref(dims), 10, 10, 0, out, 6) == -1 and b"TGNN_WS_MAP_ENTRIES" in _lib.lib.tgnn_last_error()
    assert _lib.lib.tgnn_forward_workspace_map(C.byref(dims), 10, 9, 0, out, 7) == -1
    assert _lib.lib.tgnn_forward_workspace_map(C.byref(dims), 10, 10, 0, None, 7) == -1
    bad = _lib.ModelDims(3, 15, 30, 4, 1)
    assert _lib.lib.tgnn_forward_workspace_map(C.byref(bad), 10, 10, 0, out, 7) == -1
