"""Every output and state array of tgnn_hole_sweep_many and tgnn_tree_sweep_many on the case builders of
tests/test_hole_sweep_gpu.py and tests/test_tree_sweep_gpu.py, one solve_many_hole_free over the eight ring-9 cuts of
scratch/hole_sweep_times.py (selections, orders, round counts, vetoes, final RandomState states) and the tilings of one
solve_tree(roots=8, beam=8, top_k=1, check_holes=True), written to one .npz -- to compare two trees byte for byte (integer sums,
fixed orders: equality is the expectation, not a tolerance).  Run from each tree, one process each, then compare:
    python <tree A>/scratch/sweep_accept_refactor_bytes.py a.npz
    python <tree B>/scratch/sweep_accept_refactor_bytes.py b.npz
    python scratch/sweep_accept_refactor_bytes.py --compare a.npz b.npz
Only what both trees have is used: the two harnesses, the fixtures' graphs and the public attributes of the front ends."""
import gzip
import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), (sorted(set(a.files) ^ set(b.files)))
    same = []
    for name in a.files:
        x, y = a[name], b[name]
        same.append(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())
        if not same[-1]:
            print(f"{name}: {x.dtype} {x.shape} sha256 {hashlib.sha256(x.tobytes()).hexdigest()[:16]} / "
                  f"{hashlib.sha256(y.tobytes()).hexdigest()[:16]} DIFFERENT")
    groups = sorted({name.split(".")[0] for name in a.files})
    for grp in groups:
        names = [n for n in a.files if n.split(".")[0] == grp]
        digest = hashlib.sha256(b"".join(a[n].tobytes() for n in sorted(names))).hexdigest()[:16]
        ok = all(s for n, s in zip(a.files, same) if n in names)
        print(f"{grp}: {len(names)} arrays, {sum(a[n].nbytes for n in names)} bytes, sha256 {digest}: {'identical' if ok else 'DIFFERENT'}")
    print(f"sweep entries, {sys.argv[2]} against {sys.argv[3]}: {sum(same)} of {len(same)} arrays byte-identical")
    sys.exit(0 if all(same) else 1)

import torch  # noqa: E402

from tests import hole_delta_cases as hc  # noqa: E402
from tests import hole_guard_restatement as hg  # noqa: E402
from tests import test_hole_sweep_gpu as th  # noqa: E402
from tests import test_tree_sweep_gpu as tt  # noqa: E402
from tests import tree_search_restatement as ts  # noqa: E402
from tests.golden_util import GOLDEN  # noqa: E402
from tests.test_tree_search_host import CONFIGS, restated  # noqa: E402
from tilingnn_amd import TilinGNN, _lib  # noqa: E402
from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver  # noqa: E402
from tilingnn_amd.tiling.brick_layout import BrickLayout  # noqa: E402
from tilingnn_amd.tiling.tile_graph import TileGraph  # noqa: E402
from tilingnn_amd.util import algorithms as alg  # noqa: E402
from tilingnn_amd.util import data_util as du  # noqa: E402
from tilingnn_amd.weights import make_state_dict  # noqa: E402

DEV = torch.device("cuda:0")
out = {}


def keep(prefix, res=None, state=None, **more):
    for name, a in (res or {}).items():
        out[f"{prefix}.{name}"] = np.asarray(a)
    for i, a in enumerate(state or ()):
        out[f"{prefix}.state{i}"] = np.asarray(a)
    for name, a in more.items():
        out[f"{prefix}.{name}"] = np.asarray(a)


def load(name, gz):
    g = TileGraph(2)
    if gz:
        tmp = tempfile.mkdtemp()
        path = os.path.join(tmp, "g.pkl")
        with gzip.open(os.path.join(GOLDEN, name + ".pkl.gz"), "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        g.load_graph_state(path, sidecar=False)
        shutil.rmtree(tmp)
    else:
        g.load_graph_state(os.path.join(GOLDEN, name + ".pkl"), sidecar=False)
    return g


ring9_graph, small_graph = load("complete_graph_ring9", True), load("complete_graph_small", False)
ring9, small_h, small_t = th.Fixture(ring9_graph), th.Fixture(small_graph), tt.Fixture(small_graph)

# ---------------------------------------------------------------- the hole entry (tests/test_hole_sweep_gpu.py)
# nine copies of ring 9, eight rounds, layout 4 sitting out two of them
K = 9
run = th.Harness(ring9.on_device, [(np.arange(ring9.n), ring9.col)] * K)
rng = np.random.default_rng(5)
for rnd in range(8):
    unl = run.unlabelled.cpu().numpy().reshape(K, ring9.n)
    active = np.array([int(unl[k].any() and not (k == 4 and rnd in (3, 4))) for k in range(K)], dtype=np.int32)
    visits, thr, u = [], [], []
    for k in range(K):
        ids = np.flatnonzero(unl[k]) if active[k] else np.zeros(0, dtype=np.int64)
        p = rng.random(ids.size)
        order = np.argsort(-p)
        visits.append(ids[order]); thr.append(np.exp(p[order] - 1)); u.append(rng.random(ids.size))
    keep(f"hole_ring9_round{rnd}", run.call(visits, thr, u, active=active), run.state())
# either side of the LDS limit, with a collision row so that the walk kills and breaks as well
w = 96
x, y = [c.reshape(-1) for c in np.meshgrid(np.arange(w), np.arange(64))]
cell, far = 40 * w + 50, 10 * w + 7
order = np.array([cell - 1, cell + 1, cell - w, cell + w, cell, 7, far, 9])
grids = {}
for extra in (0, 1):
    tiles = [hc.box(a, b, a + 1, b + 1) for a, b in zip(x, y)] + [hc.box(200, 0, 201, 1)] * extra
    grids[extra] = od = th._made_up_graph(tiles)
    run = th.Harness(od, [(np.arange(len(tiles)), np.array([[cell, far], [far, cell]]))])
    keep(f"hole_grid{extra}_first", run.call([order], [np.array([1.0, 1.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0])],
                                             [np.array([0.5, 0.25, 0.125, 0.0, 0.875, 0.0, 0.0, 0.0])], ws_fill=0x55), run.state())
    keep(f"hole_grid{extra}_second", run.call([[cell + w, 11]], [[1.0, 0.5]], [[0.0, 0.75]]), run.state())
# labels of a row of seven, and the killed list in row order
run = th.Harness(th._made_up_graph([hc.box(i, 0, i + 1, 1) for i in range(7)]), [(np.arange(7), np.zeros((2, 0)))])
for node in [6, 0, 3, 5, 4, 1, 2]:
    keep(f"hole_row7_node{node}", run.call([[node]], [[1.0]], [[0.0]]), run.state())
six = [hc.box(2 * i, 0, 2 * i + 1, 1) for i in range(6)]
six_col = np.array([[0, 0, 0, 0, 3, 4, 2, 5], [4, 2, 4, 5, 0, 0, 0, 0]])
run = th.Harness(th._made_up_graph(six), [(np.arange(6), six_col)])
keep("hole_six", run.call([[1, 0, 3, 2, 4]], [[0.5, 1.0, 1.0, 1.0, 1.0]], [[0.75, 0.0, 0.0, 0.0, 0.0]]), run.state())
# the recipe solve of the small graph through DeviceHoleSweep, every round
for seed in range(3):
    fx = small_h
    rs = np.random.RandomState(seed)
    dsw = alg.DeviceHoleSweep(fx.graph, [(fx.n, fx.col, np.arange(fx.n))], [rs], DEV)
    sw, rnd = dsw.sweeps[0], 0
    while sw.unlabelled.any():
        rnd += 1
        dsw.round([hg.round_probs(seed, rnd, fx.n, sw.ids())])
        v = int(dsw.visit_ptr[1])
        keep(f"hole_small_seed{seed}_round{rnd}", trace=dsw.trace[:v].copy(), visit=dsw.visit_node[:v].copy())
    keep(f"hole_small_seed{seed}", state=[t.cpu().numpy() for t in (dsw.unlabelled, dsw.tile_alive, dsw.label, dsw.chi_cache)],
         selection=sw.selection, order=np.array(sw.order), vetoes=dsw.vetoes, launches=dsw.launches, rng=rs.get_state()[1], rng_pos=rs.get_state()[2])

# ---------------------------------------------------------------- the tree entry (tests/test_tree_sweep_gpu.py)
fx = small_t
for config in range(3):
    cfg = CONFIGS[config]
    s = restated(fx.rings, fx.col, cfg, 0)
    reuse = cfg["top_k"] == 1
    run = tt.Harness(fx.on_device, np.arange(fx.n), fx.col, cfg["roots"] if reuse else cfg["roots"] + sum(len(step) for step in s.steps))
    slot_of = {uid: uid for uid in range(cfg["roots"])}
    for i, step in enumerate(s.steps):
        for br in step:
            slot_of[br.uid] = slot_of[br.parent] if reuse else br.uid
        res = run.call([slot_of[b.parent] for b in step], [slot_of[b.uid] for b in step], [b.nodes for b in step], [b.p for b in step],
                       [b.u for b in step], check_holes=int(cfg["check_holes"]))
        keep(f"tree_replay{config}_step{i}", res)
    keep(f"tree_replay{config}", state=run.state())
run = tt.Harness(fx.on_device, np.arange(fx.n), fx.col, 10)
branches = tt._a_state_and_nine_branches(fx, run)
visits, p, u = ([b[i] for b in branches] for i in range(3))
keep("tree_nine", run.call([0] * 9, list(range(1, 10)), visits, p, u, fill=0x7F), run.state())
for extra in (0, 1):
    run = tt.Harness(grids[extra], np.arange(6144 + extra), np.array([[cell, far], [far, cell]]), 2)
    keep(f"tree_grid{extra}_first", run.call([0], [1], [order], [np.zeros(8)], [np.ones(8)]), run.state())
    keep(f"tree_grid{extra}_second", run.call([1], [1], [[cell + w, 11, cell]], [[1.0, 1.0, 0.5]], [[0.75, 0.0, 0.0]]), run.state())
for geometry in (False, True):
    run = tt.Harness(tt._made_up_graph(six), np.arange(6), six_col, 3, geometry=geometry)
    keep(f"tree_six_geometry{int(geometry)}", run.call([0, 0], [1, 2], [[1, 0, 3, 2, 4, 5], [3, 0, 1]], [[1.0, 1.0, 1.0, 0.5, 0.5, 0.5], [1.0] * 3],
                                                       [[0.25, 0.75, 0, 0, 0, 0], [0.0] * 3], check_holes=0), run.state())

# ---------------------------------------------------------------- the two solves
n = len(ring9_graph.tiles)
cut = lambda tiles: BrickLayout(ring9_graph, *du.create_brick_layout_from_super_set(ring9_graph, [int(t) for t in tiles]))
cuts = [cut(np.flatnonzero(np.random.default_rng(100 + k).random(n) < 0.5)) for k in range(8)]
seeds = list(range(8))


class Stubbed(ML_Solver):
    """The recipe's probabilities for K layouts (scratch/hole_sweep_times.py)."""

    def __init__(self, layouts):
        self.device, self._greedy_solver, self._score_fn = DEV, None, (lambda s, l: None)
        self.device_greedy_min_nodes, self.device_greedy_seed = None, 0
        self.tiles = [np.array([l.inverse_index[i] for i in range(len(l.node_feature))]) for l in layouts]
        self.rounds = [0] * len(self.tiles)

    def predict_many(self, subs):
        res = []
        for sub in subs:
            k = sub.origin_index
            self.rounds[k] += 1
            res.append(hg.round_probs(seeds[k], self.rounds[k], n, self.tiles[k][sub.inverse_index.cpu().numpy()]))
        return res


got = Stubbed(cuts).solve_many_hole_free(cuts, seed=seeds)
fn = alg.solve_many_hole_free
rngs = fn.last_guard.rngs                                       # the layouts' RandomStates after the solve
keep("solve_many_hole_free", rounds=np.array(fn.last_rounds), calls=fn.last_sweep_calls, vetoes=np.array(fn.last_vetoes),
     selections=np.concatenate([np.asarray(o.predict, np.float64) for o, _ in got]),
     orders=np.concatenate([np.asarray(o.predict_order, np.int64) for o, _ in got]),
     rng=np.stack([r.get_state()[1] for r in rngs]), rng_pos=np.array([r.get_state()[2] for r in rngs]))

layout = cut(range(n))
fe, fxd = int(np.asarray(layout.align_edge_features).shape[1]), int(np.asarray(layout.node_feature).shape[1])
net = TilinGNN(adj_edge_features_dim=fe, network_depth=20, network_width=32, node_features_dim=fxd)
net.load_state_dict(make_state_dict(fe, 20, 32, 1, fxd, seed=0), strict=True)
solver = ML_Solver(None, DEV, ring9_graph, net.to(DEV).train(), num_prob_maps=1, score_fn=lambda s, l: float(np.sum(s)))
tilings = solver.solve_tree(layout, seed=0, roots=8, beam=8, top_k=1, check_holes=True, max_predictions=100000)
dsw = alg.solve_by_treesearch.last_sweep
keep("solve_tree", tilings=np.stack([np.asarray(o.predict, np.float64) for o, _ in tilings]), predictions=solver.last_predict_cnt,
     calls=dsw.calls, branches=dsw.branches, vetoes=dsw.vetoes)
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print(f"{_lib.LIB_PATH}: {len(out)} arrays -> {sys.argv[1]}")
