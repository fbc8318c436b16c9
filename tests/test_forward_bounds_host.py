"""The precondition of the peak layouts of tests/test_forward_bounds.py, with the fp64 oracle on the CPU: |slot 0| and |slot 1| of the
network the GPU test runs peak in the chosen row, by a margin no rounding of the fp32 forward closes."""
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import bounds_cases as bc
from tilingnn_amd.weights import make_state_dict


CASES = [(bc.N_PEAK, r, 5, -1, False) for r in bc.PEAK_ROWS] + [(n, n - 1, bc.MID_SEED, -1, False) for n in (4097, 8191)] + \
    [(bc.N_PEAK, bc.BLOCK_END_ROW, 5, 0, True)]


@pytest.mark.parametrize("n,r_star,seed,column,last_float4", CASES)
def test_slot_0_and_slot_1_peak_in_the_chosen_row(n, r_star, seed, column, last_float4):
    sd = make_state_dict(15, bc.DEPTH, 32, 1, 3, seed=0)
    sd = orc.cast_sd(bc.last_float4_state_dict(sd) if last_float4 else sd, torch.float64)
    sg = bc.peak_layout(r_star, n=n, seed=seed, column=column)
    x, adj, attr, col, _ = (t.double() if t.is_floating_point() else t for t in sg.to_torch("cpu"))
    with torch.no_grad():
        h0 = orc.init_node_feature_trans(x, sd)
        slot1 = orc.graph_conv(h0, adj, attr, sd, "brch_1_graph_conv_layers.0") * orc.coll_conv(h0, col, sd, "brch_2_coll_conv_layers.0")
    others = torch.arange(n) != r_star
    if last_float4:                                               # the maximum lies in the row's last float4
        assert float(slot1[:, :28].abs().max()) == 0.0 and float(slot1[r_star, 28:].abs().max()) > 0
    for k, slot in enumerate((h0, slot1)):
        rows = slot.abs().max(dim=1).values
        ratio = float(rows[r_star] / rows[others].max())
        print(f"r* {r_star} slot {k}: |row r*| / largest other row = {ratio:.2f}")
        assert int(rows.argmax()) == r_star and ratio > 1.25, (k, ratio)
