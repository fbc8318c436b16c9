"""The kernels of the general schedule's layer loop in the block shapes they are launched with (csrc/nnconv_eg_plan.h:
kLayerFootprints): the edge-group NNConv, whose tile shares come from that header, as an op against fp64 at the layouts where the
shares degenerate; the two-stream forward of the general schedule against its single-stream form and the fp64 oracle; and the
register / LDS counts the runtime reports for the four kernels against the table.

Nothing here has a tolerance of its own: graphs, operands, reference and both gates are tests/nnconv_cases.py's (through the
helpers of tests/test_nnconv32_ops.py), the BatchNorm partial rows are held to dense_oracle.PARTIAL_RTOL, the forward to the slot
gates of tests/test_small_layout.py / tests/test_mid_layout.py."""
import ctypes as C

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import nnconv_cases as nc
from tests import test_mid_layout as tml
from tests import test_nnconv32_ops as t32
from tests.test_hip_parity import make_net
from tests.test_small_layout import _forward_with_slots, slot_tol

pytestmark = pytest.mark.gpu

NNCONV, AGGREGATE, GIN_MLP, MERGE = range(4)           # csrc/nnconv_eg_plan.h: LayerKernel
BENCH_TYPES = 13


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def footprint(kernel, n_types=BENCH_TYPES):
    """(waves per block, waves per SIMD of one block, register cap, registers the runtime reports, LDS bytes, max threads)"""
    from tilingnn_amd import _lib
    out = (C.c_int32 * 6)()
    _lib.check(_lib.lib.tgnn_kernel_footprint(kernel, n_types, out))
    return tuple(int(v) for v in out)


# ---------------------------------------------------------------------------------------------- the NNConv as an op
# fewer tiles than waves (1, 15, 16, 17, 37 rows: one to three tiles, most waves idle); one row more than 16 tiles per wave of a
# block would hold (16 * waves + 1); the row classes of nc.graph bring a row with more than 16 in-edges of ONE type (hub, from 64
# rows on), zero-in-degree rows (deg0_last from 2 rows on, a whole tile of them from 48 on) at every size
SMALL_ROWS = (1, 15, 16, 17, 37)


@pytest.mark.parametrize("leaky", [False, True], ids=["none", "leaky"])
@pytest.mark.parametrize("n", SMALL_ROWS)
def test_fewer_tiles_than_waves(dev, n, leaky):
    t32.run_and_gate(nc.problem(n), dev, "eg", leaky, f"rows {n} leaky {int(leaky)}")


@pytest.mark.parametrize("T", [13, 16])
def test_one_row_past_sixteen_tiles_per_wave_slot(dev, T):
    waves = footprint(NNCONV)[0]
    n = 16 * waves + 1
    p = nc.problem(n, T)
    assert "hub" in p.g.rows and int(p.g.deg[p.g.rows["hub"]]) > 16 and "deg0_last" in p.g.rows and "deg0_tile" in p.g.rows
    t32.run_and_gate(p, dev, "eg", True, f"rows {n} T {T}")


RAGGED_ROWS = 4099                                       # 257 tiles, the last one of 3 rows: 65 -> 64 blocks without a cap


def test_ragged_layout_at_1_8_and_9_blocks(dev, debug_hooks):
    """tgnn_debug_set_block_caps of 1, 8, 9 (-> 8) blocks: 257 tiles over 4, 32 and 32 SIMD slots -- shares of 64 / 65 and 8 / 9
    tiles split over the waves of a SIMD; then the uncapped launch.  (Under the production library the test runs once more in a
    process of its own against the debug build: conftest.py, debug_hooks.)"""
    if debug_hooks:
        return
    from tilingnn_amd._lib import lib
    p = nc.problem(RAGGED_ROWS)
    try:
        for cap in (1, 8, 9):
            lib.tgnn_debug_set_block_caps(cap, 0)
            _, _, npart = t32.run_and_gate(p, dev, "eg", True, f"rows {RAGGED_ROWS} cap {cap}", debug_cap=cap)
            assert npart == (cap if cap < 9 else 8)
    finally:
        lib.tgnn_debug_set_block_caps(0, 0)
    t32.run_and_gate(p, dev, "eg", True, f"rows {RAGGED_ROWS} no cap", blocks=64)


# ---------------------------------------------------------------------------------------------- the forward
def _forward_single_stream(net, inputs, n, dev):
    """tgnn_forward_profiled (every kernel on one stream, events around the classes) on a zeroed workspace -> (probs, slots)"""
    from tilingnn_amd import _lib, ops
    x, adj, adj_attr, col = inputs
    graph = ops.prepare_graph(n, adj, adj_attr, col)
    dims = net._dims()
    table, _ = net._param_table()
    ws_bytes = _lib.lib.tgnn_forward_workspace_bytes(C.byref(dims), n, graph.n_types)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    probs = torch.empty(n, 1, device=dev)
    ms, cnt = (C.c_float * 8)(), (C.c_int32 * 8)()
    g = graph.c_struct()
    _lib.check(_lib.lib.tgnn_forward_profiled(C.byref(dims), table, ops.ptr(x), ops.ptr(adj_attr), C.byref(g), 0, 0, ops.ptr(probs),
                                              ops.ptr(ws), ws_bytes, _lib.current_stream(dev), ms, cnt))
    torch.cuda.synchronize()
    d = net.network_depth
    slots = ws[: (d + 1) * n * 32 * 4].view(torch.float32).view(d + 1, n, 32).clone()
    return probs.cpu(), slots.cpu()


@pytest.mark.parametrize("n", [4099, 5003])
def test_general_schedule_two_streams_single_stream_and_oracle(dev, n):
    """Layouts the persistent schedules would take, forced onto the launch-per-op schedule: the two-stream forward against the
    single-stream profiled one bit for bit (same kernels, same trees), every slot against the fp64 oracle within the slot gates,
    and one BatchNorm update per module forward."""
    from tilingnn_amd import _lib
    depth = 3
    inputs, inputs64 = tml._layout(n, dev)
    before = _lib.lib.tgnn_get_small_layout_limit(), _lib.lib.tgnn_get_mid_layout_limit()
    _lib.lib.tgnn_set_small_layout_limit(0)
    _lib.lib.tgnn_set_mid_layout_limit(0)
    try:
        net, sd = make_net(dev, depth=depth)
        c0 = _lib.forward_path_counts()
        probs, slots = _forward_with_slots(net, inputs, n, dev)
        assert _lib.forward_path_counts()[0] == c0[0] + 1                  # the general schedule ran
        probs1, slots1 = _forward_single_stream(net, inputs, n, dev)
        assert torch.equal(probs, probs1) and torch.equal(slots, slots1)
        x, adj, attr, col = inputs
        net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)
        torch.cuda.synchronize()
        tracked = [int(v) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")]
        assert tracked and all(t == 1 for t in tracked), tracked
    finally:
        _lib.lib.tgnn_set_small_layout_limit(before[0])
        _lib.lib.tgnn_set_mid_layout_limit(before[1])
    cap = {}
    with torch.no_grad():
        want = orc.tilingnn_forward(orc.cast_sd(sd, torch.float64), *inputs64, capture=cap)[0]
    errs = [orc.rel_max_err(slots[0], cap["init"])] + [orc.rel_max_err(slots[k], cap[f"mid.{k}"]) for k in range(1, depth + 1)]
    pgap = float((probs.double() - want.cpu()).abs().max())
    print(f"n {n} depth {depth} general schedule: slots " + " ".join(f"{e:.1e}" for e in errs) + f"  max |p - p64| {pgap:.1e}")
    for k, e in enumerate(errs):
        assert e < slot_tol(k), (k, e, slot_tol(k))
    assert pgap < 1e-4 * 4 ** (depth - 1)


# ---------------------------------------------------------------------------------------------- the dense pair in its new shapes
def half_blocks(n, cap=224):
    """gin.hip, gin32_mlp_grid: 4-wave blocks, one per 64 rows, at most twice the CUs left to the chain and below the fold's group
    rows (496); from 8 on a multiple of 8"""
    nb = min((n + 63) // 64, 2 * cap, 496)
    return max(nb & ~7 if nb >= 8 else nb, 1)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 4099])
def test_gin_mlp_in_four_wave_blocks(dev, n):
    """gin32_mlp_kernel<4> (the forward's shape) through tgnn_gin32_fwd: the gate and the partial-row tolerances of
    tests/test_gin32_ops.py on tests/gin_cases.py's problems, and every row bit for bit what the 8-wave blocks give."""
    from tests import gin_cases as gc
    from tests import test_gin32_ops as g32
    from tilingnn_amd import _lib, ops
    graph = g32.col_graph(n, dev)
    before = _lib.lib.tgnn_set_gin_mlp_half_blocks(2)
    try:
        for with_stat in (False, True):
            p = gc.problem(n, 32, with_stat, 1.0)
            params = [t.to(dev) for t in gc.param_list(p.sd)]
            a = p.a.to(dev)
            stat = p.stat.to(dev) if with_stat else None
            for leaky in (True, False):
                want = orc.leaky_relu(p.want) if leaky else p.want
                act = ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE
                _lib.lib.tgnn_set_gin_mlp_half_blocks(2)
                part = ops.new_partials(32, dev)
                out, npart = ops.gin(a, graph, *params, act=act, in_stat=stat, partials=part, kernel=gc.VARIANTS[0])
                err = orc.rel_max_err(out.cpu(), want)
                print(f"gin32 4-wave blocks n {n} stat {int(with_stat)} leaky {int(leaky)}: rel_max_err {err:.3e}, {npart} blocks")
                assert out.shape == (n, 32) and bool(torch.isfinite(out).all()) and err < g32.GATE
                assert npart == half_blocks(n)
                g32.check_partials(part, npart, want, n, 32)
                _lib.lib.tgnn_set_gin_mlp_half_blocks(0)
                out8, npart8 = ops.gin(a, graph, *params, act=act, in_stat=stat, partials=ops.new_partials(32, dev), kernel=gc.VARIANTS[0])
                assert npart8 == gc.gin32_blocks(n) and torch.equal(out, out8)
    finally:
        _lib.lib.tgnn_set_gin_mlp_half_blocks(before)


@pytest.mark.parametrize("n", [1, 1023, 1025, 4099])
@pytest.mark.parametrize("n_partials", [129, 257, 512])
def test_wide_merge_is_finalize_then_merge_bit_for_bit(dev, n, n_partials):
    """merge_bn1_wide_kernel<512> (from 129 partial rows on; 257: its second round trip for the rows) through tgnn_merge_bn1_fwd
    against the two ops it fuses -- tgnn_bn_finalize on the same partial rows, tgnn_merge_fwd with that record: the same tree,
    the same formula, the same bits, record and rows, with a residual and without."""
    from tests import test_bn_merge_ops as bm
    from tilingnn_amd import _lib, ops
    c = 32
    g = torch.Generator().manual_seed(7 * n + n_partials)
    a1 = (torch.randn(n, c, generator=g) * 1.5 + 0.5).to(dev)
    a2 = (torch.randn(n, c, generator=g) * 0.7 - 0.25).to(dev)
    resid_t = torch.randn(n, c, generator=g).to(dev)
    st2 = bm.random_record(c, dev, 2 * c + n, -0.25)
    bn = bm.make_bn(c, dev, n)
    n_total = max(n, 2)
    _, rows = bm.split_sums(a1, n_partials, n)
    stat1 = ops.bn_finalize(rows, n_partials, n_total, bn, update_running=False)
    for resid in (None, resid_t):
        want, _ = ops.merge(a1, stat1, a2, st2, resid, want_h2=False)
        buf = torch.full((3, n, c), -7.25, device=dev)
        rec = torch.empty(4, c, device=dev)
        _lib.check(_lib.lib.tgnn_merge_bn1_fwd(ops.ptr(a1), ops.ptr(rows), n_partials, ops.ptr(bn.weight), ops.ptr(bn.bias), n_total,
                                              float(bn.eps), ops.ptr(a2), ops.ptr(st2), ops.ptr(resid), n, ops.ptr(buf[1]), ops.ptr(rec),
                                              _lib.current_stream(dev)))
        torch.cuda.synchronize()
        assert torch.equal(rec, stat1), "the record"
        assert torch.equal(buf[1], want), "rows"
        assert bool((buf[0] == -7.25).all() and (buf[2] == -7.25).all()), "a neighbouring slot changed"


# ---------------------------------------------------------------------------------------------- register and LDS counts
def test_reported_footprints_against_the_table(dev):
    """This checks the register and LDS counts the runtime reports (hipFuncGetAttributes) and nothing else -- not that blocks
    are resident together, not a time.  Every kernel stays within the cap its __launch_bounds__ pins it to and one block fits a
    CU; for the pair the general schedule shapes to share a CU -- one 4-wave block of the GIN MLP beside one 8-wave block of the
    merge (csrc/nnconv_eg_plan.h: kCoResidentPairs) -- waves per SIMD x allocated registers of both is at most 512 and the LDS sum
    at most 160 KB.  The NNConv does not fit beside either kernel of the collision chain: that is stated, not hidden."""
    fp = [footprint(k) for k in range(4)]
    alloc = [(f[3] + 7) // 8 * 8 for f in fp]
    for k, f in enumerate(fp):
        waves, per_simd, cap, regs, lds, max_threads = f
        print(f"kernel {k}: {waves} waves per block, {per_simd} per SIMD, cap {cap}, reported {regs} registers, {lds} B LDS")
        assert per_simd == (waves + 3) // 4 and waves * 64 <= max_threads
        assert 0 < regs <= cap
        assert per_simd * alloc[k] <= 512 and lds <= 160 * 1024
    assert [f[0] for f in fp] == [16, 4, 4, 8]
    for a, b in ((GIN_MLP, MERGE),):
        assert fp[a][1] * alloc[a] + fp[b][1] * alloc[b] <= 512, (fp[a], fp[b])
        assert fp[a][4] + fp[b][4] <= 160 * 1024
    assert fp[NNCONV][1] * alloc[NNCONV] + fp[AGGREGATE][1] * alloc[AGGREGATE] > 512
    assert fp[NNCONV][1] * alloc[NNCONV] + fp[GIN_MLP][1] * alloc[GIN_MLP] > 512
