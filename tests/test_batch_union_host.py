"""Host-side checks of mini-batch training (no GPU): the numpy oracle of the disjoint union against a hand-written example, the
chunking of an epoch's permutation, and the declaration of `tgnn_batch_union`."""
import os

import numpy as np
import pytest

from tests import batch_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_on_a_hand_written_pair():
    a = (np.array([[1, 2, 3], [4, 5, 6]], np.float32),                    # 2 nodes
         np.array([[0, 1], [1, 0]], np.int64), np.array([[10, 11], [12, 13]], np.float32),
         np.array([[0], [1]], np.int64))
    b = (np.array([[7, 8, 9], [10, 11, 12], [13, 14, 15]], np.float32),   # 3 nodes
         np.array([[0, 2, 1], [2, 0, 0]], np.int64), np.array([[20, 21], [22, 23], [24, 25]], np.float32),
         np.array([[1, 2], [2, 1]], np.int64))
    x, adj, attr, col = batch_oracle.union([a, b], [0, 1])
    assert x.tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15]]
    assert adj.tolist() == [[0, 1, 2, 4, 3], [1, 0, 4, 2, 2]]
    assert attr.tolist() == [[10, 11], [12, 13], [20, 21], [22, 23], [24, 25]]
    assert col.tolist() == [[0, 3, 4], [1, 4, 3]]
    assert (x.dtype, adj.dtype, attr.dtype, col.dtype) == (np.float32, np.int64, np.float32, np.int64)
    # the other order, with a repeat: b, a, b
    x, adj, attr, col = batch_oracle.union([a, b], [1, 0, 1])
    assert x.tolist() == [[7, 8, 9], [10, 11, 12], [13, 14, 15], [1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15]]
    assert adj.tolist() == [[0, 2, 1, 3, 4, 5, 7, 6], [2, 0, 0, 4, 3, 7, 5, 5]]
    assert attr.tolist() == [[20, 21], [22, 23], [24, 25], [10, 11], [12, 13], [20, 21], [22, 23], [24, 25]]
    assert col.tolist() == [[1, 2, 3, 6, 7], [2, 1, 4, 7, 6]]


def test_chunks_of_an_epoch():
    from tilingnn_amd.solver.ml_solver.trainer import batch_chunks
    order = [3, 0, 4, 1, 2]
    assert batch_chunks(order, 2) == [[3, 0], [4, 1], [2]]                # the short last chunk is kept
    assert batch_chunks(order, 1) == [[3], [0], [4], [1], [2]]
    assert batch_chunks(order, 8) == [[3, 0, 4, 1, 2]]                    # larger than the data set: one batch
    assert batch_chunks(order, 5) == [[3, 0, 4, 1, 2]]
    assert batch_chunks([], 4) == []
    assert batch_chunks(np.random.default_rng(0).permutation(5), 2)[2] != []
    with pytest.raises(ValueError):
        batch_chunks(order, 0)


def test_header_declares_batch_union():
    from tilingnn_amd import _lib
    with open(os.path.join(REPO, "include", "tgnn.h")) as f:
        text = f.read()
    assert "int tgnn_batch_union(" in text
    assert "tgnn_batch_union" in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.lib, "tgnn_batch_union")
    with open(os.path.join(REPO, "tilingnn_amd", "csrc", "Makefile")) as f:
        assert "batch_union.hip" in f.read()
