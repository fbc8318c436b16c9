"""Identity-keyed cache of prepared graphs.

A layout's graph is constant across the 20 layers of a forward and usually across several
forwards (ML_Solver.solve calls predict on the same BrickLayout repeatedly), so the CSR /
edge-type preparation is cached.  Entries are keyed by the IDENTITY and `_version` of the input
tensors and hold references to them, so a recycled device address can never alias a stale entry."""
from collections import OrderedDict

from .. import ops

_MAX = 4
_entries = OrderedDict()
enabled = True


def reserve(n_layouts: int) -> None:
    """Make room for `n_layouts` prepared graphs (a data set kept on the GPU: `LayoutDataset` calls this with its
    size, so that neither a training step nor a validation forward re-prepares a layout it has already seen -- with the
    default of 4 every step of an epoch over more layouts would rebuild both CSRs and synchronise)."""
    global _MAX
    _MAX = max(_MAX, int(n_layouts) + 2)


def _key(*tensors):
    return tuple((id(t), t._version, tuple(t.shape)) for t in tensors)


def _lookup(key, tensors, build):
    if not enabled:
        return build()
    hit = _entries.get(key)
    if hit is not None and all(a is b for a, b in zip(hit[0], tensors)):
        _entries.move_to_end(key)
        return hit[1]
    val = build()
    _entries[key] = (tensors, val)
    while len(_entries) > _MAX:
        _entries.popitem(last=False)
    return val


def clear():
    _entries.clear()


def _full_key(n_nodes, ts):
    # (what a prepared graph carries depends on the size range of the mid-size persistent kernel and on the schedule its
    #  size is run by -- type columns and mid-size batches, or edge groups: part of the key)
    return ("full", n_nodes, ops.mid_layout_range(), ops.GROUPS and ops.runs_general_schedule(n_nodes)) + _key(*ts)


def peek_full(n_nodes, adj_e_index, adj_e_features, col_e_idx):
    """The cached graph `get_full` would return, or None (a miss, or the cache is off): nothing is built."""
    ts = (adj_e_index, adj_e_features, col_e_idx)
    hit = _entries.get(_full_key(n_nodes, ts)) if enabled else None
    return hit[1] if hit is not None and all(a is b for a, b in zip(hit[0], ts)) else None


def put_full(n_nodes, adj_e_index, adj_e_features, col_e_idx, graph):
    """Enter a graph somebody else prepared (TilinGNN.forward_many: K layouts in one call) under the key `get_full` uses."""
    return get_full(n_nodes, adj_e_index, adj_e_features, col_e_idx, build=lambda: graph)


def get_full(n_nodes, adj_e_index, adj_e_features, col_e_idx, build=None):
    """build: what prepares the graph on a miss (default: ops.prepare_graph) -- TilinGNN.forward passes a builder that queues the
    forward's graph-independent head beside the preparation."""
    ts = (adj_e_index, adj_e_features, col_e_idx)
    return _lookup(_full_key(n_nodes, ts), ts,
                   build or (lambda: ops.prepare_graph(n_nodes, adj_e_index, adj_e_features, col_e_idx)))


def get_adj(n_nodes, adj_e_index, adj_e_features):
    """Graph with only the adjacency set prepared (stand-alone NNConv / GraphConv calls)."""
    import torch
    ts = (adj_e_index, adj_e_features)
    empty = torch.empty(2, 0, dtype=torch.int64, device=adj_e_index.device)
    return _lookup(("adj", n_nodes, ops.GROUPS and ops.runs_general_schedule(n_nodes)) + _key(*ts), ts,
                   lambda: ops.prepare_graph(n_nodes, adj_e_index, adj_e_features, empty))


def get_col(n_nodes, col_e_idx):
    """Graph with only the collision set prepared (stand-alone GINConv / CollConv calls)."""
    import torch
    ts = (col_e_idx,)
    empty_i = torch.empty(2, 0, dtype=torch.int64, device=col_e_idx.device)
    empty_f = torch.empty(0, 1, dtype=torch.float32, device=col_e_idx.device)
    return _lookup(("col", n_nodes) + _key(*ts), ts,
                   lambda: ops.prepare_graph(n_nodes, empty_i, empty_f, col_e_idx))
