"""`ML_Solver` -- the boundary caller of the scoring path, mirroring the part of
/root/reference/solver/ml_solver/ml_solver.py that sits on it:

    predict(brick_layout)            ml_solver.py:29-49   (empty-edge early-out, forward, best-map pick)
    get_unsupervised_losses_from_layout(layout, probs)    ml_solver.py:51-62 (losses.py on the GPU, csrc/loss.hip)
    get_predict_probs(brick_layout)  ml_solver.py:69-81
    load_saved_network(path)         ml_solver.py:129-131 (load_state_dict + network.train())

    solve(brick_layout)              ml_solver.py:64-73   (greedy assembly loop: tilingnn_amd/util/algorithms.py keeps the
                                                           layout on the GPU; `greedy_solver=` swaps in the reference's)
    solve_many(brick_layouts)        Tiling-Shape.py:60-64 (the crop loop: K device-greedy solves in one loop)
    solve_many_hole_free(layouts)    the same crop loop with the hole veto of algorithms.py:150-152 in every solve
    solve_tree(brick_layout)         algorithms.py:66-181  (the tree search; `predict_top_maps` scores its popped states)
The debug dumps stay with the reference.

`brick_layout` is duck-typed exactly as the reference uses it: `.node_feature`,
`.align_edge_index`, `.collide_edge_index` (numpy) and `.get_data_as_torch_tensor(device)`.
"""
from copy import deepcopy

import numpy as np
import torch

from ...graph_networks.network_utils import get_network_prediction


class LayoutArrays:
    """Minimal stand-in for tiling.brick_layout.BrickLayout's data side (brick_layout.py:242-246):
    the five numpy arrays and the float32/int64 conversion of util/data_util.py:110-117."""

    def __init__(self, node_feature, align_edge_index, align_edge_features, collide_edge_index,
                 collide_edge_features):
        self.node_feature = node_feature
        self.align_edge_index = align_edge_index
        self.align_edge_features = align_edge_features
        self.collide_edge_index = collide_edge_index
        self.collide_edge_features = collide_edge_features

    def get_data_as_torch_tensor(self, device):
        return (torch.from_numpy(self.node_feature).float().to(device),
                torch.from_numpy(self.align_edge_index).long().to(device),
                torch.from_numpy(self.align_edge_features).float().to(device),
                torch.from_numpy(self.collide_edge_index).long().to(device),
                torch.from_numpy(self.collide_edge_features).float().to(device))


class ML_Solver:
    def __init__(self, debugger, device, complete_graph, network, num_prob_maps, greedy_solver=None, score_fn=None):
        self.debugger = debugger
        self.device = device
        self.complete_graph = complete_graph
        self.network = network
        self.random_network = deepcopy(self.network)            # ml_solver.py:26
        self.num_prob_maps = num_prob_maps
        self._greedy_solver = greedy_solver
        self._score_fn = score_fn                               # (selection, layout) -> float; default: Losses.solution_score
        # None (default): solve() runs the reference's sweep with numpy's RNG stream (seeded parity) at every size; a node count:
        # layouts at least that large take tilingnn_amd.util.algorithms.solve_by_device_greedy (batched acceptance on the GPU)
        self.device_greedy_min_nodes = None
        self.device_greedy_seed = 0
        # solve_many / solve_many_by_device_greedy: score every round's small sub-layouts inside ONE persistent kernel launch
        # (TilinGNN.forward_many(union=True), csrc/forward_small.hip); the same results either way
        self.union_forward = False
        # ... and, with union_forward, prepare their graphs by ONE library call and one read-back per round instead of one of each per
        # sub-layout (TilinGNN.forward_many(union=True, union_prep=True), csrc/graph_prep.hip); the same graphs either way
        self.union_prep = False
        # solve_many: K hole-free solves -- solve_many_hole_free, the sequential sweep with the reference's hole veto for every layout
        # (csrc/hole_sweep.hip) -- instead of the batched acceptance, which has no hole rule
        self.check_holes_many = False

    @staticmethod
    def _no_edges(index) -> bool:
        """`len(index) == 0` of the reference (an empty edge set is `np.array([]).T` there); a device-resident
        sub-layout holds an empty [2, 0] tensor instead, and so may a caller's numpy layout."""
        return index.numel() == 0 if torch.is_tensor(index) else np.asarray(index).size == 0

    def predict(self, brick_layout):
        if self._no_edges(brick_layout.collide_edge_index) or self._no_edges(brick_layout.align_edge_index):
            # only one edge set left: select every remaining tile (ml_solver.py:31-32)
            predictions = torch.ones((brick_layout.node_feature.shape[0], self.num_prob_maps)).float().to(self.device)
        else:
            x, adj_edge_index, adj_edge_features, collide_edge_index, collide_edge_features = \
                brick_layout.get_data_as_torch_tensor(self.device)
            # the reference's call (ml_solver.py:39-43); tilingnn_amd.TilinGNN also checks the health word of its persistent
            # kernels here (forward_checked: the probabilities travel to the host below anyway)
            run = getattr(self.network, "forward_checked", None) or self.network
            predictions, *_ = run(x=x, adj_e_index=adj_edge_index, adj_e_features=adj_edge_features,
                                  col_e_idx=collide_edge_index, col_e_features=collide_edge_features)
        best_map_index = self._best_prob_map(predictions, brick_layout)
        return predictions[:, best_map_index].detach().cpu().numpy()

    def predict_on_device(self, brick_layout):
        """predict() for a layout that lives on the GPU, the probabilities staying there: [N] float32 on self.device (the loop of
        tilingnn_amd.util.algorithms.solve_by_device_greedy feeds them straight into the acceptance kernels)."""
        if self._no_edges(brick_layout.collide_edge_index) or self._no_edges(brick_layout.align_edge_index):
            return torch.ones(brick_layout.node_feature.shape[0], dtype=torch.float32, device=self.device)     # ml_solver.py:31-32
        x, adj_edge_index, adj_edge_features, collide_edge_index, collide_edge_features = \
            brick_layout.get_data_as_torch_tensor(self.device)
        run = getattr(self.network, "forward_checked", None) or self.network
        predictions, *_ = run(x=x, adj_e_index=adj_edge_index, adj_e_features=adj_edge_features,
                              col_e_idx=collide_edge_index, col_e_features=collide_edge_features)
        return predictions[:, self._best_prob_map(predictions, brick_layout)].detach().contiguous()

    def predict_many(self, sub_layouts):
        """`predict` for several device-resident layouts at once -> a list of numpy arrays, per layout the bits `predict` returns:
        the forwards side by side (`network.forward_many`, honouring `union_forward` / `union_prep`, with the checks of
        `forward_checked` once), the best-map pick of a network with several maps from ONE loss call as
        `solve_many_by_device_greedy` makes it, and ONE read-back for all layouts.  A layout with one edge set left gets ones
        without the network (ml_solver.py:31-32).  This is the seam `solve_many_hole_free` calls once per round
        (tilingnn_amd.util.algorithms.solve_many_hole_free; each sub-layout carries `.origin_index` there)."""
        from ...util import algorithms as alg
        subs = list(sub_layouts)
        out = [None] * len(subs)
        need = [i for i, s in enumerate(subs) if not (self._no_edges(s.collide_edge_index) or self._no_edges(s.align_edge_index))]
        for i, s in enumerate(subs):
            if i not in need:
                out[i] = np.ones(int(s.node_feature.shape[0]), dtype=np.float32)
        if not need:
            return out
        views = [subs[i] for i in need]
        if hasattr(self.network, "forward_many"):
            preds = alg._forward_many_checked(self.network, views, 3, bool(self.union_forward), bool(self.union_prep))
        else:
            preds = [self.predict_on_device(v).reshape(-1, 1) for v in views]
        best = {j: 0 for j in range(len(views))}
        if preds[0].shape[1] > 1:
            pk = alg.PackedLayouts(views, self.device)
            best = alg._best_prob_maps_many(pk, list(range(len(views))), preds, None, None)
        flat = torch.cat([p[:, best[j]].detach().reshape(-1) for j, p in enumerate(preds)])
        host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
        host.copy_(flat, non_blocking=True)
        torch.cuda.current_stream(flat.device).synchronize()
        host, at = host.numpy(), 0
        for j, i in enumerate(need):
            n = int(preds[j].shape[0])
            out[i] = host[at:at + n].copy()
            at += n
        return out

    def predict_top_maps(self, sub_layouts, top_k):
        """What the tree search asks per popped state (tilingnn_amd.util.algorithms.solve_by_treesearch; the repair of the
        reference's 4-argument get_best_prob_map, algorithms.py:105): for several device-resident layouts at once, per layout a
        numpy float32 [n, min(top_k, M)] array -- the probabilities of its min(top_k, M) best maps, best first, "best" being
        `np.argsort` of the per-map unsupervised loss.  The forwards side by side as in `predict_many` (honouring
        `union_forward` / `union_prep`, the checks of `forward_checked` once), the ranking of every layout from ONE
        `tgnn_unsupervised_loss_many` call, ONE read-back of the probabilities.  A layout with one edge set left gets ones
        without the network (ml_solver.py:31-32).  Column 0 is bit for bit what `predict` returns."""
        from ...util import algorithms as alg
        if top_k < 1:
            raise ValueError("predict_top_maps: top_k is at least 1")
        subs = list(sub_layouts)
        out = [None] * len(subs)
        need = [i for i, s in enumerate(subs) if not (self._no_edges(s.collide_edge_index) or self._no_edges(s.align_edge_index))]
        for i, s in enumerate(subs):
            if i not in need:
                out[i] = np.ones((int(s.node_feature.shape[0]), min(int(top_k), int(self.num_prob_maps))), dtype=np.float32)
        if not need:
            return out
        views = [subs[i] for i in need]
        if hasattr(self.network, "forward_many"):
            preds = alg._forward_many_checked(self.network, views, 3, bool(self.union_forward), bool(self.union_prep))
        else:
            run = getattr(self.network, "forward_checked", None) or self.network
            preds = [run(x=v.node_feature, adj_e_index=v.align_edge_index, adj_e_features=v.align_edge_features,
                         col_e_idx=v.collide_edge_index, col_e_features=v.collide_edge_features)[0] for v in views]
        n_maps = int(preds[0].shape[1])
        keep = min(int(top_k), n_maps)
        ranks = {j: np.arange(1) for j in range(len(views))}
        if n_maps > 1:
            ranks = alg._prob_map_ranks_many(alg.PackedLayouts(views, self.device), list(range(len(views))), preds)
        picks = [torch.from_numpy(np.ascontiguousarray(ranks[j][:keep])).to(preds[j].device) for j in range(len(views))] if n_maps > 1 else None
        flat = torch.cat([(p if picks is None else p[:, picks[j]]).detach().reshape(-1) for j, p in enumerate(preds)])
        host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
        host.copy_(flat, non_blocking=True)
        torch.cuda.current_stream(flat.device).synchronize()
        host, at = host.numpy(), 0
        for j, i in enumerate(need):
            n = int(preds[j].shape[0])
            out[i] = host[at:at + n * keep].reshape(n, keep).copy()
            at += n * keep
        return out

    def _best_prob_map(self, predictions, brick_layout):
        """get_best_prob_map (ml_solver.py:133-136): argsort of the per-map unsupervised loss.
        With one probability map -- the only configuration the reference ever constructs
        (Tiling-Shape.py:37, Tiling-GUI.py:570) -- the answer is 0 and the loss (a device round trip) is skipped."""
        if predictions.shape[1] == 1:
            return 0
        losses = self.get_unsupervised_losses_from_layout(brick_layout, predictions)
        return int(np.argsort(losses)[0])

    def get_unsupervised_losses_from_layout(self, brick_layout, probs):
        """ml_solver.py:51-62: the per-map losses of `probs` on a layout, as numpy."""
        from .losses import Losses
        x, adj_edge_index, adj_edge_features, collide_edge_index, collide_edge_features = \
            brick_layout.get_data_as_torch_tensor(self.device)
        _, _, losses = Losses.calculate_unsupervised_loss(probs, x, collide_edge_index,
                                                          adj_edges_index=adj_edge_index,
                                                          adj_edge_features=adj_edge_features)
        return losses

    def get_predict_probs(self, brick_layout):
        x, adj_edge_index, adj_edge_features, collide_edge_index, collide_edge_features = \
            brick_layout.get_data_as_torch_tensor(self.device)
        return get_network_prediction(network=self.network, x=x, adj_e_index=adj_edge_index,
                                      adj_e_features=adj_edge_features, col_e_idx=collide_edge_index,
                                      col_e_features=collide_edge_features)

    def solve(self, brick_layout, check_holes=False, device_sweep=False):
        """ml_solver.py:64-73.  Default loop: tilingnn_amd.util.algorithms.solve_by_probablistic_greedy (layout resident
        on the GPU; score = Losses.solution_score when the layout carries its complete graph and super-contour area, or
        `score_fn`, else None); `greedy_solver=` swaps in another one, e.g. the reference's own.
        check_holes: the reference's hole veto (algorithms.py:150-152) in that loop -- a tile that would enclose a gap is passed
        over, so the solution has no hole (`solve_by_probablistic_greedy(check_holes=True)`, csrc/union_hole_delta.hip).  Always
        the sequential sweep, whatever `device_greedy_min_nodes` says: the batched acceptance has no hole rule.
        device_sweep (with check_holes): that guarded sweep runs on the device, one launch and one read-back per round
        (csrc/hole_sweep.hip); the same solution and the same RNG stream."""
        if device_sweep and not check_holes:
            raise ValueError("device_sweep is an option of check_holes=True")
        if self._greedy_solver is None:
            from ...util.algorithms import solve_by_device_greedy, solve_by_probablistic_greedy
            n_nodes = int(brick_layout.node_feature.shape[0])
            if check_holes:                                      # the sequential sweep only: tiles accepted at once can close a gap jointly
                output_solution, score, predict_order = solve_by_probablistic_greedy(self, brick_layout, score_fn=self._score_fn,
                                                                                     check_holes=True, device_sweep=device_sweep)
            elif self.device_greedy_min_nodes is not None and n_nodes >= self.device_greedy_min_nodes:
                # large layouts: the acceptance batched on the device (a documented substitute of the sequential sweep)
                output_solution, score, predict_order = solve_by_device_greedy(self, brick_layout, seed=self.device_greedy_seed,
                                                                               score_fn=self._score_fn)
            else:
                output_solution, score, predict_order = solve_by_probablistic_greedy(self, brick_layout, score_fn=self._score_fn)
        elif check_holes:
            raise ValueError("check_holes is an option of the default greedy loop; hand it to the `greedy_solver` given instead")
        else:
            output_solution, score, predict_order = self._greedy_solver(self, brick_layout)
        output_layout = deepcopy(brick_layout)
        output_layout.predict_order = predict_order
        output_layout.predict = output_solution
        output_layout.predict_probs = self.predict(brick_layout)
        return output_layout, score

    def solve_many(self, brick_layouts, seed=None):
        """`solve` for K layouts at once -- the crop loop of the reference (Tiling-Shape.py:60-64) as ONE greedy loop on the GPU
        (tilingnn_amd.util.algorithms.solve_many_by_device_greedy: per round one compaction, one read-back, the sub-layouts
        scored side by side, one acceptance call).  Every layout is solved as `solve_by_device_greedy` solves it alone with the
        same seed (default: `device_greedy_seed`), whatever `device_greedy_min_nodes` says.  Returns a list of
        (output_layout, score) in input order; `predict`, `predict_order` as in `solve`; `predict_probs` = the first round's
        probabilities (the first round's sub-layout IS the layout: what `self.predict(layout)` returns, without K more forwards).
        In train mode the BatchNorm running statistics are left untouched (see `TilinGNN.forward_many`).
        `self.union_forward = True`: every round's small sub-layouts are scored inside one persistent kernel launch
        (`TilinGNN.forward_many(union=True)`): the same results, fewer launches per round.  `self.union_prep = True` beside it: the
        sub-layouts' graphs come from one library call and one read-back per round (`forward_many(..., union_prep=True)`).
        `self.check_holes_many = True` (an attribute like `union_forward`, default False): `solve_many_hole_free` instead -- K
        HOLE-FREE solves, the sequential sweep with the reference's hole veto for every layout."""
        from ...util.algorithms import solve_many_by_device_greedy
        if getattr(self, "check_holes_many", False):
            return self.solve_many_hole_free(brick_layouts, seed=seed)
        brick_layouts = list(brick_layouts)
        if not brick_layouts:
            return []
        results = solve_many_by_device_greedy(self, brick_layouts, seed=self.device_greedy_seed if seed is None else seed,
                                              score_fn=self._score_fn)
        first = solve_many_by_device_greedy.last_first_probs
        out = []
        for layout, (selection, score, order), probs in zip(brick_layouts, results, first):
            output_layout = deepcopy(layout)
            output_layout.predict_order = order
            output_layout.predict = selection
            output_layout.predict_probs = probs.cpu().numpy() if probs is not None else self.predict(layout)
            out.append((output_layout, score))
        return out

    def solve_many_hole_free(self, brick_layouts, seed=None):
        """`solve(layout, check_holes=True)` for K layouts at once (tilingnn_amd.util.algorithms.solve_many_hole_free,
        csrc/hole_sweep.hip): every layout is solved as it is solved alone after `np.random.seed(seed_k)` -- the sequential sweep
        with the reference's hole veto, a block per layout, one `predict_many`, one sweep call and one read-back per round for all
        of them -- so no solution has a hole.  `seed`: one per layout, or one number for all (default `device_greedy_seed`); the
        global `np.random` stream is not touched.  The layouts must be cut from ONE complete graph and carry it with their
        `inverse_index`.  Returns what `solve_many` returns.  What `solve_many` runs when `self.check_holes_many` is set."""
        from ...util.algorithms import solve_many_hole_free
        if self._greedy_solver is not None:
            raise ValueError("check_holes is an option of the default greedy loop; hand it to the `greedy_solver` given instead")
        brick_layouts = list(brick_layouts)
        if not brick_layouts:
            return []
        seeds = self.device_greedy_seed if seed is None else seed
        seeds = [int(s) for s in seeds] if np.ndim(seeds) else [int(seeds)] * len(brick_layouts)
        results = solve_many_hole_free(self, brick_layouts, seeds, score_fn=self._score_fn)
        out = []
        for layout, (selection, score, order), probs in zip(brick_layouts, results, solve_many_hole_free.last_first_probs):
            output_layout = deepcopy(layout)
            output_layout.predict_order = order
            output_layout.predict = selection
            output_layout.predict_probs = probs if probs is not None else self.predict(layout)
            out.append((output_layout, score))
        return out

    def solve_tree(self, brick_layout, **options):
        """The tree search of the reference (util/algorithms.py:66-181) on one layout:
        tilingnn_amd.util.algorithms.solve_by_treesearch(self, brick_layout, **options) -- top_k, check_holes, max_predictions,
        time_limit, beam, roots, seed, literal -- with the branch sweeps on the device (csrc/tree_sweep.hip).  Returns a list of
        (output_layout, score), one per distinct finished tiling, best first; `predict`, `predict_order` and `predict_probs` as
        `solve` sets them.  `last_predict_cnt`: the states the search scored."""
        from ...util.algorithms import solve_by_treesearch
        options.setdefault("score_fn", self._score_fn)
        results, self.last_predict_cnt = solve_by_treesearch(self, brick_layout, **options)
        probs = self.predict(brick_layout) if results else None
        out = []
        for selection, score, order in results:
            output_layout = deepcopy(brick_layout)
            output_layout.predict_order = order
            output_layout.predict = selection
            output_layout.predict_probs = probs
            out.append((output_layout, score))
        return out

    def load_saved_network(self, net_path):
        self.network.load_state_dict(torch.load(net_path, map_location=self.device))
        self.network.train()                                     # ml_solver.py:131: inference stays in train mode
