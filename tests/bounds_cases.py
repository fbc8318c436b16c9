"""Layouts and networks of tests/test_forward_bounds.py that need no GPU to build (numpy / torch CPU): the layouts whose slot maximum
lies in a chosen row, and the x 64 network of the reused-workspace cases.  tests/test_forward_bounds_host.py checks the layouts'
precondition with the fp64 oracle.

Where the maximum lies.  A hub in the collision graph does NOT put it there: the GIN's MLP is Sigmoid on all three layers
(coll_conv.py:10-18), so the sum over 500 neighbours saturates instead of growing -- measured with the fp64 oracle over hub degrees
40 .. 500, four weight seeds and the three rows below, the hub row's BatchNorm 2 output is ~4 sigma and |slot 1| of that row
0.2 .. 1.0 x the largest other row.  What does: ONE node feature far outside the others' range (the area ratio, 100 instead of
(0, 1]).  The init MLP is LeakyReLU + BatchNorm -- nothing saturates --, so slot 0 of that row is ~30 x every other row's, the
NNConv's root term carries it into BatchNorm 1, and |slot 1| of the row is 1.5 .. 1.9 x the largest other row (seed 5)."""
N_PEAK = 1237                    # odd, not a multiple of 16 (the tile), of 8 (a float4 row group) or of 256
PEAK_ROWS = (0, N_PEAK - 1, N_PEAK - 2)
PEAK_FEATURE = 100.0
DEPTH = 4                        # the residual middle[i - 2] is in the merges of layers 2 and 3
MID_SEED = 9                     # 4 097 and 8 191 rows: the seed at which |slot 1| of the last row is 1.5 x / 27 x the largest other row
BLOCK_END_ROW = 31               # float4 255 of the slot = the last one of the first 256-thread block's stride: row 31, channels 28 .. 31


def plain_layout(n, seed=5, n_types=13):
    from tilingnn_amd.synth import make_super_graph
    return make_super_graph(n, 8 * n, 10 * n, tile_count=2, n_edge_types=n_types, seed=seed)


def peak_layout(r_star, n=N_PEAK, seed=5, column=-1):
    """plain_layout(n) with one node feature of row r_star (the last one: the area ratio) set to PEAK_FEATURE."""
    sg = plain_layout(n, seed)
    sg.node_feature[r_star, column] = PEAK_FEATURE
    return sg


def last_float4_state_dict(sd):
    """A copy of sd whose first adjacency BatchNorm is zero (gamma and beta) outside channels 28 .. 31: slot 1 is then exactly zero
    outside the LAST float4 of every row.  With peak_layout(BLOCK_END_ROW, column=0) -- the first node feature: the one whose outlier
    comes through the LeakyReLUs with the right sign in those channels -- the slot's maximum lies in float4 255."""
    out = {k: v.clone() for k, v in sd.items()}
    for name in ("weight", "bias"):
        out[f"brch_1_graph_conv_layers.0.batch_norm.{name}"][:28] = 0
    return out


def scaled_state_dict(sd, factor=64.0):
    """A copy of sd whose layer BatchNorms' gamma (both branches, every layer) are multiplied by `factor`: slot k >= 1 -- the product
    of the two branches' BatchNorm outputs -- grows by about factor^2."""
    out = {k: v.clone() for k, v in sd.items()}
    for k in out:
        if k.startswith(("brch_1_graph_conv_layers.", "brch_2_coll_conv_layers.")) and k.endswith(".batch_norm.weight"):
            out[k] = out[k] * factor
    return out
