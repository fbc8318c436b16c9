"""The disjoint union of layouts, restated in numpy: what PyG's Batch.from_data_list does to the four arrays the network and
the loss read -- node features, adjacency attributes and both edge indices concatenated in member order (the indices along
their last dimension), every edge end shifted by the number of nodes of the members in front.  Written from that definition
alone: it shares no code with PackedLayouts or with csrc/batch_union.hip."""
import numpy as np


def union(layouts, ids):
    """layouts: a list of (x [N, fx] float32, adj [2, Ea] int64, attr [Ea, fe] float32, col [2, Ec] int64) numpy arrays in
    each layout's own numbering; ids: the members, in order (repeats allowed).  -> (x, adj, attr, col) of the union."""
    fx = max(l[0].shape[1] for l in layouts)
    fe = max(l[2].shape[1] for l in layouts)
    xs, adjs, attrs, cols = [np.zeros((0, fx), np.float32)], [np.zeros((2, 0), np.int64)], [np.zeros((0, fe), np.float32)], \
        [np.zeros((2, 0), np.int64)]
    first = 0                                             # number of the member's first node in the union
    for i in ids:
        x, adj, attr, col = layouts[i]
        xs.append(np.asarray(x, np.float32).reshape(-1, fx))
        adjs.append(np.asarray(adj, np.int64).reshape(2, -1) + first)
        attrs.append(np.asarray(attr, np.float32).reshape(-1, fe))
        cols.append(np.asarray(col, np.int64).reshape(2, -1) + first)
        first += xs[-1].shape[0]
    return np.concatenate(xs, 0), np.concatenate(adjs, 1), np.concatenate(attrs, 0), np.concatenate(cols, 1)
