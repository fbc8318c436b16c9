"""What tests/test_training_sizes.py rests on, without a GPU: the directed graphs of tests/train_graphs.py have the properties
the adjoint tests need (one direction per pair, hubs whose in- and out-degree differ, rows without in- or out-edges, exactly T
edge types), and the chunked NNConv of the oracle (`nnconv_mean_dedup`, the only form that fits at 66 003 nodes) has the
gradients of the reference's op sequence (`nnconv_mean`)."""
import numpy as np
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import train_graphs as tgr
from tilingnn_amd.weights import make_state_dict


@pytest.mark.parametrize("n,ea,ec,T", [(300, 1500, 2000, 13), (tgr.N_MID, 30000, 25000, 63), (tgr.N_MID, 30000, 25000, 1),
                                       (tgr.N_BIG, tgr.EA_BIG, tgr.EC_BIG, 13)])
def test_directed_graph_properties(n, ea, ec, T):
    x, adj, attr, col = tgr.directed_graph(n, ea, ec, T, 15, seed=n + T)
    hub_a, hub_c = tgr.hub_sizes(n)
    assert (hub_a, hub_c) == ((700, 400) if n > 2100 else (n // 3, n // 3))
    assert x.shape == (n, 3) and adj.shape == (2, ea) and attr.shape == (ea, 15) and col.shape == (2, ec)
    assert x.dtype == attr.dtype == torch.float32 and adj.dtype == col.dtype == torch.int64
    assert int(adj.min()) >= 0 and int(adj.max()) < n and int(col.min()) >= 0 and int(col.max()) < n
    assert float(x[:, 2].min()) > 0 and float(x[:, 2].max()) <= 1 and bool((x[:, :2].sum(1) == 1).all())
    # one direction per pair, no pair twice, no self loop
    src, dst = adj[0], adj[1]
    assert not bool((src == dst).any())
    key = torch.minimum(src, dst) * n + torch.maximum(src, dst)
    assert torch.unique(key).shape[0] == ea
    # the transposed graph is another graph: the two degrees differ, by hundreds at the hubs
    din, dout = tgr.degrees(adj, n)
    assert int(din[tgr.ADJ_SINK]) >= hub_a and int(dout[tgr.ADJ_SOURCE]) >= hub_a
    assert int(din[tgr.ADJ_SINK]) > 4 * int(dout[tgr.ADJ_SINK]) + 50 and int(dout[tgr.ADJ_SOURCE]) > 4 * int(din[tgr.ADJ_SOURCE]) + 50
    assert int((din != dout).sum()) > n // 2
    assert int(din[n - tgr.NO_IN_TAIL:].sum()) == 0 and int(dout[n - tgr.NO_IN_TAIL:].sum()) > 0
    assert int(dout[tgr.NO_OUT[0]:tgr.NO_OUT[1]].sum()) == 0 and int(din[tgr.NO_OUT[0]:tgr.NO_OUT[1]].sum()) > 0
    # exactly T attribute rows, every value from (0, 1); the sink hub's in-edges are of one type
    etype, n_types = tgr.edge_types(attr)
    assert n_types == T == np.unique(attr.numpy(), axis=0).shape[0]
    assert float(attr.min()) >= 0 and float(attr.max()) < 1
    into_sink = etype[dst == tgr.ADJ_SINK]
    assert int(torch.bincount(into_sink).max()) >= hub_a
    # collision edges: self loops, both hubs
    cin, cout = tgr.degrees(col, n)
    loops = int((col[0] == col[1]).sum())
    assert tgr.SELF_LOOPS <= loops <= tgr.SELF_LOOPS + 40
    assert int(cin[tgr.COL_SINK]) >= hub_c and int(cout[tgr.COL_SOURCE]) >= hub_c
    assert int(cin[tgr.COL_SINK]) > 2 * int(cout[tgr.COL_SINK]) + 50 and int(cout[tgr.COL_SOURCE]) > 2 * int(cin[tgr.COL_SOURCE]) + 50


def test_directed_graph_is_seeded():
    a = tgr.directed_graph(300, 1500, 2000, 5, 6, seed=3)
    b = tgr.directed_graph(300, 1500, 2000, 5, 6, seed=3)
    c = tgr.directed_graph(300, 1500, 2000, 5, 6, seed=4)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[1], c[1])


@pytest.mark.parametrize("width", [32, 64])
def test_dedup_nnconv_has_the_gradients_of_the_port(width):
    """fp64 autograd through `nnconv_mean_dedup` (chunks of edges, the edge MLP once per distinct row) against `nnconv_mean`
    (the reference's op sequence with its materialised [Ea, C, C]): input, root, bias and the three edge-MLP layers, to 1e-12."""
    torch.set_num_threads(4)
    n, fe, T = 300, 15, 13
    x, adj, attr, _ = tgr.directed_graph(n, 1500, 2000, T, fe, seed=1)
    p1 = "brch_1_graph_conv_layers.1"
    sd64 = orc.cast_sd(make_state_dict(fe, 2, width, 1, 3, seed=2), torch.float64)
    g = torch.Generator().manual_seed(5)
    h, dz = torch.randn(n, width, generator=g, dtype=torch.float64), torch.randn(n, width, generator=g, dtype=torch.float64)
    names = [p1 + ".nnConv.root", p1 + ".nnConv.bias"] + [f"{p1}.mlp.mlp.{k}.linear.{w}" for k in range(3) for w in ("weight", "bias")]
    grads = []
    for fn, kw in ((orc.nnconv_mean, {}), (orc.nnconv_mean_dedup, {"chunk": 400})):      # 400: four chunks, the last one short
        leaf = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd64.items()}
        hh = h.clone().requires_grad_(True)
        out = fn(hh, adj, attr.double(), leaf, p1, **kw)
        (out * dz).sum().backward()
        grads.append([out.detach(), hh.grad] + [leaf[k].grad for k in names])
    for what, a, b in zip(["output", "input"] + names, *grads):
        assert b is not None and float(b.abs().max()) > 0, what
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), what
