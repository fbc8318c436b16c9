"""The conditions the GINConv op tests (tests/test_gin32_ops.py) rest on, checked on the CPU from the oracle alone: every kernel of
csrc/gin.hip is reached by some case and every case reaches the kernel it names (tests/gin_cases.py: dispatch); no case saturates
layer 1; and at unit scale the fp64 oracle evaluated in fp32 by torch stays within 5e-7 -- the 1e-6 gate keeps at least 2x over a
correct fp32 kernel."""
import pytest
import torch

from tests import gin_cases as gc


def test_every_kernel_is_reached_and_every_case_reaches_its_kernel():
    reached = set()
    for case in gc.CASES:
        kernels, blocks = gc.dispatch(case.c, case.n, case.lda, case.aligned, case.variant)
        assert kernels == case.kernels, case
        assert 1 <= blocks <= 512, case
        reached.update(kernels)
    assert reached == set(gc.KERNELS)
    # the block counts the row counts are there for
    want = {1: 1, 7: 1, 9: 1, 16: 1, 17: 1, 37: 1, 200: 2, 800: 7, 1000: 8, 2000: 16, 3000: 24, 1254: 8, 30000: 224, 66003: 224}
    assert set(want) == set(gc.ROW_COUNTS)
    assert {n: gc.gin32_blocks(n) for n in gc.ROW_COUNTS} == want
    assert gc.gin32_blocks(200003) == 224
    assert [gc.gin32_blocks(n) for n in gc.FORWARD_ROWS] == [1, 2, 7, 8, 16, 24]
    # the fused kernel's hand-over ring has 6 slots per team; a team's share is ceil(tiles / (4 blocks)) tiles at most
    team = lambda n: -(-((n + 15) // 16) // (4 * gc.gin32_blocks(n)))
    assert team(66003) == 5 and team(200003) == 14          # no wrap; every slot reused twice
    # what the op refuses, and the forward's default
    assert gc.dispatch(64, 37, 64, True, 0)[0] == ("refused",) and gc.dispatch(32, 37, 33, True, 0)[0] == ("refused",)
    assert gc.dispatch(32, 37, 32, False, 2)[0] == ("refused",) and gc.dispatch(32, 2 ** 24, 32, True, 0)[0] == ("refused",)
    assert gc.dispatch(32, 37, 36, True, 0)[0] == (gc.AGG, gc.MLP)
    assert gc.dispatch(32, 37, 36, True, 1)[0] == ("refused",) and gc.dispatch(32, 37, 36, True, 2)[0] == ("refused",)
    assert [gc.forward_default_variant(n) for n in (3000, 199999, 200000, 200003)] == [0, 0, 2, 2]


@pytest.mark.parametrize("n", sorted(gc.ROW_COUNTS) + sorted(gc.FUSED_ONLY_ROW_COUNTS))
def test_op_cases_are_unsaturated_and_fp32_holds_the_floor(n):
    """Every (record or none) x magnitude: at least half of layer 1's pre-activations within (-4, 4); at unit scale the fp32 torch
    evaluation of the oracle within 5e-7 of the fp64 one."""
    torch.set_num_threads(8)
    for with_stat in (False, True):
        for scale in gc.MAGNITUDES:
            p = gc.problem(n, 32, with_stat, scale)
            print(f"gin32 n {n} stat {int(with_stat)} scale {scale:g}: unsaturated share {p.share:.2f}, fp32 torch vs fp64 {p.f32_err:.2e}")
            assert p.share >= 0.5, (with_stat, scale, p.share)
            assert bool(torch.isfinite(p.want).all())
            if scale == 1.0:
                assert p.f32_err < gc.F32_FLOOR, (with_stat, p.f32_err)


@pytest.mark.parametrize("n", gc.WEIGHT_SCALE_ROWS)
def test_weight_scale_cases(n):
    """The first four scale pairs keep plain fp32 within the floor; the two scaled-up pairs are the ones whose gate follows the
    fp32 evaluation (tests/test_gin32_ops.py): printed here."""
    for w2s, w3s in gc.WEIGHT_SCALES:
        p = gc.problem(n, 32, False, 1.0, w2s, w3s)
        print(f"gin32 n {n} W2 x {w2s:g} W3 x {w3s:g}: unsaturated share {p.share:.2f}, fp32 torch vs fp64 {p.f32_err:.2e}")
        assert p.share >= 0.5
        if max(w2s, w3s) <= 1.0:
            assert p.f32_err < gc.F32_FLOOR, (w2s, w3s, p.f32_err)


@pytest.mark.parametrize("c", gc.GENERIC_WIDTHS)
def test_generic_width_cases(c):
    for n in gc.GENERIC_ROWS:
        for with_stat in (False, True):
            p = gc.problem(n, c, with_stat, 1.0)
            print(f"gin generic c {c} n {n} stat {int(with_stat)}: unsaturated share {p.share:.2f}, fp32 torch vs fp64 {p.f32_err:.2e}")
            assert p.share >= 0.5
            assert p.f32_err < gc.F32_FLOOR, (n, with_stat, p.f32_err)
