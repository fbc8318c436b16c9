"""CPU check of the case table behind tests/test_bf16_shapes.py: how much of TOL_BF16 the REFERENCE alone uses.

The bf16-storage path (csrc/bf16_path.hip) rounds twice per collision seam: z = (1 + eps) h + sum h[src] in front of the MLP, and
the stored output.  Both are modelled here in fp64 on the CPU -- nothing of the kernels runs -- and compared with the oracle on
the same bf16-rounded inputs: on every case of the table the model must stay at or below 0.6 x TOL_BF16, so that a GPU gate
of TOL_BF16 on these inputs is a gate on the kernels' arithmetic and not a coin toss on the inputs' conditioning."""
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import bf16_cases as bc
from tests.test_bf16_path import TOL_BF16, bf
from tilingnn_amd.weights import make_state_dict

PREFIX = "brch_2_coll_conv_layers.1"


def modelled_errors(case):
    n = case[0]
    _, _, _, col = bc.case_graph(case)
    sd64 = orc.cast_sd(make_state_dict(bc.FE, 3, bc.W, 1, bc.FX, seed=0), torch.float64)
    h = bf(torch.randn(n, bc.W, generator=torch.Generator().manual_seed(7))).double()
    leaky = torch.nn.functional.leaky_relu
    with torch.no_grad():
        want_gin = orc.gin_conv(h, col, sd64, PREFIX)
        want_cc = orc.batch_norm_train(leaky(want_gin), sd64, PREFIX + ".batch_norm")
        keep = col[0] != col[1]
        agg = torch.zeros(n, bc.W, dtype=torch.float64).index_add_(0, col[1][keep], h.index_select(0, col[0][keep]))
        z = bf((1.0 + sd64[PREFIX + ".ginConv.eps"]) * h + agg).double()                  # storage rounding 1
        pre = orc.mlp(z, sd64, PREFIX + ".ginConv.nn", 3, orc.sigmoid, bn=False)
        got_gin = bf(pre).double()                                                        # storage rounding 2 (GINConv seam)
        got_cc = bf(orc.batch_norm_train(leaky(pre), sd64, PREFIX + ".batch_norm")).double()   # ... (CollConv seam: after its BatchNorm)
    return orc.rel_max_err(got_gin, want_gin), orc.rel_max_err(got_cc, want_cc)


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_reference_uses_little_more_than_half_the_tolerance(case):
    e_gin, e_cc = modelled_errors(case)
    print(f"{bc.case_id(case)}: modelled storage error GINConv {e_gin:.2e}, CollConv incl. BatchNorm {e_cc:.2e} "
          f"(0.6 x TOL_BF16 = {0.6 * TOL_BF16:.2e})")
    assert e_gin <= 0.6 * TOL_BF16
    if case[0] >= 2:
        assert e_cc <= 0.6 * TOL_BF16


def test_the_table_exercises_what_it_claims():
    """Degrees 0 .. 19 occur (every remainder of the 4-way gather loop), node 5 is isolated in both graphs, the hub row has its
    hub's in-degree, (3000, 1, 0) leaves hundreds of rows without a collision in-edge, (3000, 0, 0) has none at all."""
    for case in bc.CASES:
        n, cpn, hub = case
        x, adj, attr, col = bc.case_graph(case)
        assert x.shape == (n, bc.FX) and attr.shape == (adj.shape[1], bc.FE) and adj.shape[0] == col.shape[0] == 2
        assert int(adj.min()) >= 0 and int(adj.max()) < n and (col.numel() == 0 or (int(col.min()) >= 0 and int(col.max()) < n))
        assert len(torch.unique(attr, dim=0)) == min(bc.N_TYPES, adj.shape[1])
        deg = bc.col_in_degree(n, col)
        if n > bc.ISOLATED_ROW + 1:
            assert int(deg[bc.ISOLATED_ROW]) == 0 and not bool((adj[1] == bc.ISOLATED_ROW).any())
        if n >= 8 + bc.DEGREE_LADDER and cpn:
            assert deg[8:8 + bc.DEGREE_LADDER].tolist() == list(range(bc.DEGREE_LADDER))
        if hub:
            assert int(deg[bc.HUB_ROW]) >= hub - 2 and int((adj[1] == bc.HUB_ROW).sum()) >= hub
        if case == (3000, 1, 0):
            assert int((deg == 0).sum()) >= 300
        if case == (3000, 0, 0):
            assert col.shape == (2, 0)
    assert {c[0] for c in bc.CASES} >= {2, 7, 17, 130, 1030, 29_000}
