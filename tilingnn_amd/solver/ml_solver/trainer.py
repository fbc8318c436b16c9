"""`Trainer` -- the training loop (/root/reference/solver/ml_solver/trainer.py:22-124).

What the reference does per epoch (:68-124): for every layout of `<data_path>/train/raw/*.pkl` (a PyG Dataset/DataLoader,
batch_size 1, inputs/config.py:44): forward in train mode, `Losses.calculate_unsupervised_loss`, `loss.backward()`,
`optimizer.step()`; then the average loss over the training and the testing split (`Losses.cal_avg_loss`), and a
checkpoint of network + optimizer when the test loss improved or every `save_model_per_epoch` epochs, which
`ml_solver.load_saved_network` reads back.

Here: the same loop with
  * the layout files read by the shapely-free loader (util/data_util.py) ONCE and kept on the GPU (a split of 20 000
    layouts of a few thousand nodes is a few GB; the reference re-reads `data_<i>.pt` from disk every step),
  * forward + backward through the adjoint kernels (tilingnn_amd/train.py; `network.autograd` is switched on around the
    steps), the loss and its gradient on the GPU (solver/ml_solver/losses.py),
  * the caller's optimizer untouched (`optimizer.step()` on the `.grad`s, as in network_train.py).
`create_data` (trainer.py:39-50, :126-165) judges its random target shapes on the GPU (csrc/region.hip) instead of with
shapely in a 16-process pool.  Not mirrored: the per-checkpoint debug plots (`ml_solver.save_debug_info`, trainer.py:113-121).  `train` takes batch_size 1, the only
value the reference configures; mini-batches -- PyG's disjoint-union batching, the `batch_size` of the reference's signature
(trainer.py:55, :60) -- are `train_batches`: per step the union of B layouts is written by one launch (`ops.batch_union`,
csrc/batch_union.hip) and goes through the same `train_step`.  The evaluation of the single-layout splits after an epoch runs one
layout at a time (`cal_avg_loss`) or, with `eval_group=G`, G layouts per forward / loss call behind one read-back per split
(`cal_avg_loss_many`: the same float).
"""
import contextlib
import glob
import os
import traceback

import numpy as np
import torch

from ... import ops
from ...util import data_util
from ...util.algorithms import DeviceLayout, PackedLayouts, _forward_many_checked
from .losses import Losses


class LayoutDataset:
    """`<root>/raw/*.pkl` (GraphDataset.raw_file_names, solver/ml_solver/data_util.py:15-17) resident on the device."""

    def __init__(self, root, device):
        self.files = sorted(glob.glob(os.path.join(root, "raw", "*.pkl")))
        self.device = device
        self._packed = None
        self.layouts = []
        for f in self.files:
            _, x, col_idx, col_feat, adj_idx, adj_feat, *_ = data_util.load_brick_layout_data(f)
            if x is None or col_idx is None or adj_idx is None or adj_feat is None:
                raise ValueError(f"{f}: a training layout file must carry its features (write_bricklayout(with_features=True))")
            self.layouts.append(DeviceLayout.upload(_Arrays(x, adj_idx, adj_feat, col_idx), device))
        from ...graph_networks import _graph_cache
        _graph_cache.reserve(len(_graph_cache._entries) + len(self.layouts))    # every layout's prepared graph stays cached

    def __len__(self):
        return len(self.layouts)

    def __getitem__(self, i):
        return self.layouts[i]

    @property
    def packed(self):
        """The resident layouts as one `PackedLayouts` (built on first use: a second copy of the arrays, concatenated): what
        `ops.batch_union` gathers mini-batches from."""
        if self._packed is None:
            self._packed = PackedLayouts(self.layouts, self.device)
        return self._packed


class _Arrays:
    def __init__(self, node_feature, align_edge_index, align_edge_features, collide_edge_index):
        self.node_feature, self.align_edge_index = node_feature, align_edge_index
        self.align_edge_features, self.collide_edge_index = align_edge_features, collide_edge_index


def cal_avg_loss(network, layouts):
    """Losses.cal_avg_loss (losses.py:14-45), first return value: the mean loss over a split."""
    losses = []
    was = network.autograd
    network.autograd = False
    try:
        for lay in layouts:
            if lay.align_edge_index.numel() == 0 or lay.collide_edge_index.numel() == 0:
                continue
            with torch.no_grad():
                probs, _ = network(lay.node_feature, lay.align_edge_index, lay.align_edge_features, lay.collide_edge_index)
                loss, _, _ = Losses.calculate_unsupervised_loss(probs, lay.node_feature, lay.collide_edge_index,
                                                                lay.align_edge_index, lay.align_edge_features)
            losses.append(float(loss))
    finally:
        network.autograd = was
    return float(np.mean(losses)) if losses else float("nan")


def eval_groups(n, group):
    """range(n) cut into contiguous groups of `group`, the short last one kept: what one `unsupervised_losses_many` call covers."""
    group = int(group)
    if group < 1:
        raise ValueError("group must be at least 1")
    return [range(i, min(i + group, int(n))) for i in range(0, int(n), group)]


def _split_layouts(split, device=None):
    """(PackedLayouts, one DeviceLayout per member) of a LayoutDataset, a PackedLayouts or a list of layouts.  A data set's own
    layouts are the ones its prepared graphs are cached under; the views of a PackedLayouts are made once and kept with it."""
    if isinstance(split, LayoutDataset):
        return split.packed, split.layouts
    if not isinstance(split, PackedLayouts):
        split = list(split)
        if not split:
            return None, []
        split = PackedLayouts(split, device if device is not None else split[0].node_feature.device)
    views = getattr(split, "_member_views", None)
    if views is None:
        views = split._member_views = [split.layout(k) for k in range(split.k)]
    return split, views


def cal_avg_loss_many(network, dataset_or_packed, group=32, union=True):
    """`cal_avg_loss` with the work of `group` layouts per call: the members of every contiguous group (file order) that have both
    edge sets are scored by `network.forward_many(..., union=union)` -- the solo forward's bits --, the persistent kernels'
    health word is polled once per group, and ONE `Losses.unsupervised_losses_many` call per group (the solo loss's bits) writes
    into one device buffer that is read back once per split.  The same float as `cal_avg_loss(network, split)`: the per-layout
    minimum cast to float32, then np.mean over Python floats; NaN for an empty split.  One difference that reaches no output: in
    train mode `forward_many` leaves the BatchNorm running statistics untouched where `cal_avg_loss` updates them once per
    layout; train-mode outputs do not read them."""
    packed, lays = _split_layouts(dataset_or_packed, getattr(dataset_or_packed, "device", None))
    n = len(lays)
    if n == 0:
        return float("nan")
    m = int(network.output_dim)
    buf, losses, terms, err = Losses.many_outputs(n, m, packed.device)
    present = [False] * n
    was = network.autograd
    network.autograd = False
    try:
        with torch.no_grad():
            for ids in eval_groups(n, group):
                keep = [k for k in ids if lays[k].align_edge_index.numel() != 0 and lays[k].collide_edge_index.numel() != 0]
                outs = _forward_many_checked(network, [lays[k] for k in keep], 3, union=bool(union)) if keep else []
                probs = [None] * len(ids)
                for k, out in zip(keep, outs):
                    probs[k - ids[0]] = out
                    present[k] = True
                rows = slice(ids[0], ids[0] + len(ids))
                Losses.unsupervised_losses_many(probs, packed, first=ids[0], count=len(ids),
                                                out=(losses[rows], terms[rows], err[rows]))
                del outs, probs
    finally:
        network.autograd = was
    if not any(present):
        return float("nan")
    results = Losses.results_many(*Losses.read_back_many(buf, n, m), present=present)      # the split's ONE read-back
    return float(np.mean([float(r[0]) for r in results if r is not None]))


def batch_chunks(order, batch_size):
    """DataLoader(batch_size=B, drop_last=False) over an index order: consecutive chunks of B, the short last one kept."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    order = [int(i) for i in order]
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def _union_is_trainable(packed, ids):
    """What `train_step` needs of a batch, from the host tables: 2 nodes (BatchNorm), both edge sets non-empty."""
    size = lambda p: sum(p[i + 1] - p[i] for i in ids)
    return size(packed.node_ptr_h) >= 2 and size(packed.adj_ptr_h) > 0 and size(packed.col_ptr_h) > 0


@contextlib.contextmanager
def _graph_cache_bypassed(network):
    """A union is a new graph every step: prepared beside the cache, so that an epoch of them does not evict the per-layout
    graphs `LayoutDataset` reserved room for (and the cache does not pin B layouts' worth of arrays per step)."""
    was = network.cache_graph
    network.cache_graph = False
    try:
        yield
    finally:
        network.cache_graph = was


def cal_avg_loss_batches(network, packed, chunks):
    """`cal_avg_loss` over disjoint-union batches (the reference evaluates `loader_train`, whose batches are unions)."""
    losses = []
    was = network.autograd
    network.autograd = False
    try:
        with _graph_cache_bypassed(network), torch.no_grad():
            for ids in chunks:
                if not _union_is_trainable(packed, ids):
                    continue
                lay = ops.batch_union(packed, ids)
                probs, _ = network(lay.node_feature, lay.align_edge_index, lay.align_edge_features, lay.collide_edge_index)
                loss, _, _ = Losses.calculate_unsupervised_loss(probs, lay.node_feature, lay.collide_edge_index,
                                                                lay.align_edge_index, lay.align_edge_features)
                losses.append(float(loss))
    finally:
        network.autograd = was
    return float(np.mean(losses)) if losses else float("nan")


class Trainer:
    def __init__(self, debugger, plotter, device, network, data_path, model_save_path=None):
        self.debugger, self.plotter, self.device, self.network = debugger, plotter, device, network
        self.data_path = data_path
        self.training_path = os.path.join(data_path, "train")
        self.testing_path = os.path.join(data_path, "test")
        if model_save_path is None:                                      # trainer.py:27, :34-35
            model_save_path = debugger.file_path("model") if debugger is not None else os.path.join(data_path, "model")
        self.model_save_path = model_save_path
        os.makedirs(self.model_save_path, exist_ok=True)

    def create_data(self, complete_graph, low=0.4, high=0.8, max_vertices=10, testing_ratio=0.2, number_of_data=20000,
                    rng=None, batch=4096):
        """trainer.py:39-50, :126-165: `number_of_data` training layouts, then int(number_of_data * testing_ratio) testing
        layouts, cut out of the complete graph by random stars (tile_factory.generate_random_inputs) and written as
        `<data_path>/{train,test}/raw/data_<i>.pkl` in the reference's schema (write_brick_layout_data, with features).

        rng: a random.Random (default: the global `random` module).  Candidates are drawn in stream order and judged on the
        GPU `batch` at a time (the predicate and the edge counts in one launch each; a candidate with no collision or no
        adjacency edge is rejected, as the reference's loop draws again); data i is the i-th accepted candidate, and its file
        is what create_brick_layout_from_super_set + write_brick_layout_data give for its tiles.  Afterwards the stream is
        where a sequential loop would leave it: at the draw of the last accepted candidate of the test split.
        The reference forks a pool of 16 workers that all inherit one random state (trainer.py:137-138), so its files depend
        on the scheduling; that is not mirrored.  The seconds spent are left in `self.create_data_times`
        (gpu = draws + predicate + counts, write = the producer and the files)."""
        import random as _random
        rng = _random if rng is None else rng
        for path in (self.data_path, self.training_path, self.testing_path):
            os.makedirs(path, exist_ok=True)
        self.create_data_times = {"gpu": 0.0, "write": 0.0}
        self._create_data(complete_graph, self.training_path, number_of_data, low, high, max_vertices, rng, batch)
        self._create_data(complete_graph, self.testing_path, int(number_of_data * testing_ratio), low, high, max_vertices,
                          rng, batch)

    def _create_data(self, graph, data_path, number_of_data, low, high, max_vertices, rng, batch):
        import time
        from ...tiling import tile_factory
        from ...tiling.region import Region
        os.makedirs(os.path.join(data_path, "raw"), exist_ok=True)
        on_device = data_util.graph_on_device(graph, self.device)
        bound = tile_factory.get_graph_bound(graph)
        done = 0
        while done < number_of_data:
            t0 = time.perf_counter()
            want = number_of_data - done
            n = min(batch, max(64, want + want // 2))
            regions, states = [], []
            for _ in range(n):
                regions.append(Region(tile_factory.draw_random_polygon(bound, max_vertices, low, high, rng), validate=False))
                states.append(rng.getstate())
            alive = on_device.tiles_in_regions(regions)
            counts = on_device.region_edge_counts(alive).cpu().numpy()
            accepted = np.flatnonzero((counts[:, 0] > 0) & (counts[:, 1] > 0))[:want]
            rows = alive[torch.from_numpy(accepted).to(alive.device)].cpu().numpy() if accepted.size else None
            t1 = time.perf_counter()
            self.create_data_times["gpu"] += t1 - t0
            for j, k in enumerate(accepted):
                out = data_util.create_brick_layout_from_super_set(graph, np.flatnonzero(rows[j]).tolist())
                data_util.write_brick_layout_data(save_path="raw/data_{}.pkl".format(done + j), node_features=out[0],
                                                  collide_edge_index=out[1], collide_edge_features=out[2],
                                                  align_edge_index=out[3], align_edge_features=out[4], re_index=out[5],
                                                  prefix=data_path, predict=None, predict_order=None, predict_probs=None)
            self.create_data_times["write"] += time.perf_counter() - t1
            done += int(accepted.size)
            if done == number_of_data and accepted.size:
                rng.setstate(states[int(accepted[-1])])      # the draws past the last accepted candidate are undone

    def train_step(self, layout, optimizer):
        """trainer.py:69-84 for one layout; returns the loss (a 0-dim tensor) or None when the layout has an empty edge
        set (the reference's forward cannot run on one either)."""
        if layout.align_edge_index.numel() == 0 or layout.collide_edge_index.numel() == 0:
            return None
        probs, _ = self.network(layout.node_feature, layout.align_edge_index, layout.align_edge_features,
                                layout.collide_edge_index)
        optimizer.zero_grad()
        loss, *_ = Losses.calculate_unsupervised_loss(probs, layout.node_feature, layout.collide_edge_index,
                                                      adj_edges_index=layout.align_edge_index,
                                                      adj_edge_features=layout.align_edge_features)
        loss.backward()
        optimizer.step()
        return loss.detach()

    def train(self, ml_solver, optimizer, batch_size=1, training_epoch=10000, save_model_per_epoch=5, shuffle_seed=None,
              log=print, eval_group=None):
        """eval_group: None = the splits are evaluated one layout at a time (`cal_avg_loss`); an integer = `eval_group` layouts
        per forward_many / loss call (`cal_avg_loss_many`: the same losses, BatchNorm running statistics left untouched)."""
        evaluate = cal_avg_loss if eval_group is None else (lambda net, split: cal_avg_loss_many(net, split, group=eval_group))
        if batch_size != 1:
            raise NotImplementedError("batch_size 1 only (inputs/config.py:44)")
        train_set = LayoutDataset(self.training_path, self.device)
        test_set = LayoutDataset(self.testing_path, self.device)
        rng = np.random.default_rng(shuffle_seed)
        log("Training Start!!!")
        min_test_loss = float("inf")
        history = []
        for epoch in range(training_epoch):
            self.network.train()
            self.network.autograd = True
            try:
                for i in rng.permutation(len(train_set)):               # DataLoader(shuffle=True), trainer.py:61
                    try:
                        self.train_step(train_set[int(i)], optimizer)
                    except Exception:                                    # trainer.py:82-84: report and go on
                        log(traceback.format_exc())
            finally:
                self.network.autograd = False
            loss_train = evaluate(self.network, train_set)
            log(f"epoch {epoch}: training loss: {loss_train}")
            loss_test = evaluate(self.network, test_set)
            log(f"epoch {epoch}: testing loss: {loss_test}")
            history.append((loss_train, loss_test))
            if loss_test < min_test_loss or epoch % save_model_per_epoch == 0:      # trainer.py:96-108
                min_test_loss = min(min_test_loss, loss_test)
                model_file = os.path.join(self.model_save_path, f"model_{epoch}_{loss_test}.pth")
                torch.save(self.network.state_dict(), model_file)
                torch.save(optimizer.state_dict(), os.path.join(self.model_save_path, f"optimizer_{epoch}_{loss_test}.pth"))
                log(f"model saved at epoch {epoch}")
                if ml_solver is not None:
                    ml_solver.load_saved_network(model_file)
        log("Training Done!!!")
        return history

    def train_batch_step(self, packed, ids, optimizer):
        """One mini-batch step: the disjoint union of the layouts `ids` of `packed` (one launch, `ops.batch_union`) through
        `train_step` -- BatchNorm statistics over all rows of the union, one loss, one optimizer step, as the reference's loop
        body on a PyG batch.  `network.autograd` must be on (as for `train_step`).  Returns the loss, or None for a batch
        `train_step` cannot run (fewer than 2 nodes, or an edge set empty over the whole batch)."""
        if not _union_is_trainable(packed, ids):
            return None
        with _graph_cache_bypassed(self.network):
            return self.train_step(ops.batch_union(packed, ids), optimizer)

    def train_batches(self, ml_solver, optimizer, batch_size=32, training_epoch=10000, save_model_per_epoch=5,
                      shuffle_seed=None, log=print, eval_group=None):
        """The loop of `train` on mini-batches (the reference's `train` with its `batch_size`, trainer.py:52-124): every epoch's
        permutation is cut into consecutive chunks of `batch_size` (the short last one kept: DataLoader's drop_last=False) and
        every chunk is one `train_batch_step`.  After the epoch the training loss is the mean over the batches of the training
        split (in file order, same `batch_size`: the reference evaluates `loader_train`), the test loss the mean over single
        layouts (`loader_test` has batch_size 1); checkpoints as in `train`.  eval_group: as in `train`, for the test split."""
        evaluate = cal_avg_loss if eval_group is None else (lambda net, split: cal_avg_loss_many(net, split, group=eval_group))
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        chunks_of = lambda order: batch_chunks(order, batch_size)
        train_set = LayoutDataset(self.training_path, self.device)
        test_set = LayoutDataset(self.testing_path, self.device)
        packed = train_set.packed
        eval_chunks = chunks_of(range(len(train_set)))
        rng = np.random.default_rng(shuffle_seed)
        log("Training Start!!!")
        min_test_loss = float("inf")
        history = []
        for epoch in range(training_epoch):
            self.network.train()
            self.network.autograd = True
            try:
                for ids in chunks_of(rng.permutation(len(train_set))):   # DataLoader(batch_size, shuffle=True), trainer.py:60
                    try:
                        self.train_batch_step(packed, ids, optimizer)
                    except Exception:                                    # trainer.py:85-87: report and go on
                        log(traceback.format_exc())
            finally:
                self.network.autograd = False
            loss_train = cal_avg_loss_batches(self.network, packed, eval_chunks)
            log(f"epoch {epoch}: training loss: {loss_train}")
            loss_test = evaluate(self.network, test_set)
            log(f"epoch {epoch}: testing loss: {loss_test}")
            history.append((loss_train, loss_test))
            if loss_test < min_test_loss or epoch % save_model_per_epoch == 0:      # trainer.py:96-108
                min_test_loss = min(min_test_loss, loss_test)
                model_file = os.path.join(self.model_save_path, f"model_{epoch}_{loss_test}.pth")
                torch.save(self.network.state_dict(), model_file)
                torch.save(optimizer.state_dict(), os.path.join(self.model_save_path, f"optimizer_{epoch}_{loss_test}.pth"))
                log(f"model saved at epoch {epoch}")
                if ml_solver is not None:
                    ml_solver.load_saved_network(model_file)
        log("Training Done!!!")
        return history
