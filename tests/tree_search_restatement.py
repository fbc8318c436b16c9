"""The tree search restated on the host (the reference's util/algorithms.py:66-181 solve_by_treesearch, :223-234
get_nodes_order_array, :196-207 label_collision_neighbor), with the loop-tracing oracle of tests/topology_oracle.py as the hole
veto: a tile is refused when holes(selection + tile) > holes(selection).  Nothing of the package's search is imported: the loop is
written out again.

The reference's function cannot run as it stands (it calls a `predict(..., random_network=)` and a 4-argument
`get_best_prob_map` that do not exist); two repairs, everything else kept:
  * the solver hands back, per sub-layout, the probabilities of its min(top_k, M) best maps, best first (here: `maps(cnt, ids)`
    -> float32 [n_sub, m], cnt = the number of the prediction, from 1);
  * `is_random_network` is accepted and must be False.
Kept quirks: the saved value starts at 1.0 where a log-probability of 0 is meant (:285), and the test of an already labelled node
is `u < prob_m[idx]` on a value that can exceed 1 (:145).  log_prob_network keeps the dtype numpy gives it (float32 from a float32
network: no up-cast before the log).

literal=True follows the reference decision for decision: one root, one state popped per step with the `random` module, the
exponent 1 / predict_cnt of the GLOBAL count (:98, :113), `np.random.choice` and `np.random.random` of numpy's global stream, the
branches of a state swept one after another.
The default is the batched search: `roots` empty selections; per step min(beam, len(queue)) states popped one at a time with
`random.Random(seed).randint(0, len(queue) - 1)`; the exponent of a state is 1 / depth, its OWN number of predictions (the global
counter under a beam would flatten every prob_m towards 1); branch number s -- in creation order: step, pop order, map rank -- has
its own `np.random.RandomState([seed, s])` for its choice and its draws; neither global generator is touched.

The recipe the tests share: the WHOLE complete graph as the layout (node i = tile i); `recipe_maps(seed, M, top_k)`.
"""
import random
import time
from dataclasses import dataclass, field

import numpy as np

from tests import topology_oracle as to

EPS = 1e-7
ALPHA = 100.0
NOT_REACHED, BREAK, VETOED, REJECTED, ACCEPTED, SKIPPED = range(6)


def recipe_probs(seed, cnt, n, n_maps):
    """All M maps of prediction `cnt` over all n tiles, float32 as a network gives them."""
    return np.random.default_rng(1000 * seed + cnt).random((n, n_maps)).astype(np.float32)


def recipe_maps(seed, n, n_maps, top_k):
    """maps(cnt, ids): the recipe's maps on the nodes `ids`, the min(top_k, M) best first; the stub's "loss" of a map is minus
    the sum of its probabilities on the sub-layout (float64 sum of float32 values, np.argsort as the reference ranks)."""
    def maps(cnt, ids):
        prob = recipe_probs(seed, cnt, n, n_maps)[ids]
        losses = -prob.astype(np.float64).sum(axis=0)
        return prob[:, np.argsort(losses)[:top_k]]
    return maps


def softmax(x):
    x = x - np.max(x)
    exp_x = np.exp(x)
    return exp_x / np.sum(exp_x)


def sampling_probabilities(prob_m):
    """get_nodes_order_array (:228-230), the builtin `sum` included."""
    sampling_prob = np.clip(softmax(prob_m * ALPHA), a_min=1e-7, a_max=1 - 1e-7)
    return sampling_prob / sum(sampling_prob)


@dataclass
class State:
    saved: np.ndarray                         # unlabelled_nodes' values over all nodes (1.0 at the start: :285)
    unlabelled: np.ndarray
    order: list = field(default_factory=list)  # the nodes labelled 1, in labelling order
    depth: int = 0                            # predictions made on the way to this state
    uid: int = 0

    def fork(self, uid):
        return State(self.saved.copy(), self.unlabelled.copy(), list(self.order), self.depth, uid)


@dataclass
class Branch:
    """One sweep as a device call would see it."""
    parent: int
    uid: int
    nodes: np.ndarray                         # the sampled visiting order, layout nodes
    p: np.ndarray                             # prob_m at each position
    u: np.ndarray                             # the branch's next len(nodes) uniforms (the walk consumes a prefix)
    trace: list                               # per position reached: (code, node)
    accepted: list
    killed: list
    vetoes: int
    draws: int
    skipped: int
    requeued: bool
    unlabelled: np.ndarray                    # afterwards
    selected: list                            # the state's whole selection afterwards, in order


@dataclass
class Search:
    results: list                             # (selection, score, order), best first (stable)
    predict_cnt: int
    steps: list                               # per step the list of its Branches
    pops: list                                # per step the uids popped


def search(rings, colli_edges, maps, top_k=4, check_holes=False, max_predictions=None, beam=8, roots=1, seed=0, literal=False,
           is_random_network=False, time_limit=None, score_fn=None):
    assert is_random_network is False
    assert max_predictions is not None or time_limit is not None
    if literal:
        assert beam == 1 and roots == 1
    n = len(rings)
    col = np.asarray(colli_edges).reshape(2, -1)
    by_src = np.argsort(col[0], kind="stable")
    starts = np.searchsorted(col[0][by_src], np.arange(n + 1))
    nbr = col[1][by_src]
    score_fn = score_fn or (lambda selection: None)
    pop_rng = random if literal else random.Random(seed)
    uid = 0
    queue = []
    for _ in range(roots):
        queue.append(State(np.ones(n), np.ones(n, dtype=bool), uid=uid))
        uid += 1
    results, seen, steps, pops = [], {}, [], []
    predict_cnt, n_branches = 0, 0
    start = time.time()

    def running():
        return (len(queue) > 0 and (max_predictions is None or predict_cnt < max_predictions)
                and (time_limit is None or time.time() - start < time_limit))

    while running():
        popped = []
        for _ in range(min(beam, len(queue))):
            if not running():
                break
            popped.append(queue.pop(pop_rng.randint(0, len(queue) - 1)))
            predict_cnt += 1
            popped[-1].depth += 1
            popped[-1].cnt = predict_cnt
        pops.append([s.uid for s in popped])
        step = []
        for chosen in popped:
            ids = np.flatnonzero(chosen.unlabelled)
            prob = maps(chosen.cnt, ids)
            for m in range(prob.shape[1]):
                prob_network = prob[:, m]
                log_prob_network = np.log(np.clip(prob_network, EPS, 1.0))                          # (:111)
                log_prob_m = chosen.saved[ids] + log_prob_network                                  # (:112)
                prob_m = np.exp(log_prob_m / (predict_cnt if literal else chosen.depth))            # (:113)
                new = chosen.fork(uid)
                uid += 1
                new.saved[ids] = log_prob_m                                                         # (:124-125)
                rng = np.random if literal else np.random.RandomState([seed, n_branches])
                n_branches += 1
                order = rng.choice(len(ids), len(ids), replace=False, p=sampling_probabilities(prob_m))     # (:232)
                ahead = np.random.RandomState()
                ahead.set_state(rng.get_state())
                br = Branch(chosen.uid, new.uid, ids[order].copy(), prob_m[order].copy(), ahead.uniform(size=len(ids)), [], [], [],
                            0, 0, 0, False, None, None)
                tiles = [rings[i] for i in new.order]
                veto_cache = {}

                def vetoed(node):
                    if node not in veto_cache:
                        veto_cache[node] = to.topology(tiles + [rings[node]])[1] > 0
                    return veto_cache[node]

                for idx in order:                                                                   # (:138)
                    node = int(ids[idx])
                    if not new.unlabelled[node]:                                                    # (:144-148)
                        br.draws += 1
                        if rng.random_sample() < prob_m[idx]:
                            br.trace.append((SKIPPED, node))
                            br.skipped += 1
                            continue
                        br.trace.append((BREAK, node))
                        break
                    if check_holes and vetoed(node):                                                # (:151-152)
                        br.trace.append((VETOED, node))
                        br.vetoes += 1
                        continue
                    new.unlabelled[node] = False                                                    # (:155-157)
                    new.order.append(node)
                    br.trace.append((ACCEPTED, node))
                    br.accepted.append(node)
                    tiles.append(rings[node])
                    if check_holes:
                        assert to.topology(tiles)[1] == 0, "an accepted tile opened a hole"
                        veto_cache.clear()
                    for v in nbr[starts[node]:starts[node + 1]]:
                        if new.unlabelled[v]:
                            new.unlabelled[v] = False
                            br.killed.append(int(v))
                br.requeued = bool(new.unlabelled.any()) and len(br.accepted) > 0                   # (:166)
                br.unlabelled, br.selected = new.unlabelled.copy(), list(new.order)
                step.append(br)
                if br.requeued:
                    queue.append(new)
                else:
                    selection = np.zeros(n)
                    selection[new.order] = 1
                    key = "".join(str(int(s)) for s in selection)                                   # (:172)
                    if key not in seen:
                        seen[key] = 1
                        results.append((selection, score_fn(selection), list(new.order)))
        steps.append(step)
    if results and results[0][1] is not None:
        results = sorted(results, key=lambda tup: tup[1], reverse=True)                             # (:180)
    return Search(results, predict_cnt, steps, pops)
