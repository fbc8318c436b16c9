"""CPU checks of the dense op's reference and gates (tests/dense_oracle.py) on the case tables of tests/dense_cases.py: nothing
of the kernels runs.

1. The reference alone stays inside both gates: torch's CPU fp32 F.linear + activation (the BatchNorm on load in fp32, as
   bn_apply1 writes it) against the fp64 reference, on every case of the tables with the row counts capped at 4 099 -- the bounds
   are not tighter than plain fp32.
2. The gates are sensitive: five corruptions of a passing fp32 result, each of a kind a kernel produces (a masked tail row, a
   clamped column, a slot read at the wrong stride, a partial row short of one row, a BatchNorm that ignores the mean's low half)
   must be rejected.
3. The tables reach what they name: `dispatch` (dense_act_impl's conditions restated) puts every case on a kernel its group
   names, and every kernel named is reached."""
import pytest
import torch

from tests import dense_cases as dc
from tests import dense_oracle as do

ROWS_CAP = 4099
F = torch.nn.functional


def fp32_op(a, w, b, act, stat=None, slot_major=False):
    x = do.flatten(a, slot_major)
    if stat is not None:
        x = ((x - stat[0]) - stat[1]) * stat[2] + stat[3]
    return act32(F.linear(x, w, b), act)


def act32(z, act):
    return F.leaky_relu(z, 0.01) if act == dc.LEAKY else torch.sigmoid(z) if act == dc.SIGMOID else z


def capped_rows(group):
    return sorted({min(n, ROWS_CAP) for n in group.rows})


@pytest.mark.parametrize("group,shape", dc.group_shapes(dc.GROUPS + [dc.ROWS_GROUP]),
                         ids=lambda v: v.name if isinstance(v, dc.Group) else dc.shape_id(v))
def test_plain_fp32_stays_inside_both_gates(group, shape):
    slot_major = group.kind in ("slots", "f16")
    f16 = group.kind == "f16"
    bad, worst = [], 0.0
    for n in capped_rows(group):
        for stat in group.stats:
            for variant in (dc.f16_variants(shape) if f16 else ("plain",)):
                a, w, b, rec = dc.make_inputs(group, shape, n, stat, variant)
                pre = do.pre_activation(a, w, b, rec, slot_major)
                for act in group.acts:
                    ref = do.reference(a, w, b, act, rec, slot_major, pre=pre)
                    got = fp32_op(a, w, b, act, rec, slot_major)
                    worst = max(worst, do.measure(got, ref, act, f16)[1])
                    bad += ["n %d stat %s %s act %d: %s" % (n, stat, variant, act, f) for f in do.gate_failures(got, ref, act, f16)]
                    if variant == "zero":
                        assert torch.equal(got, act32(b, act).expand_as(got))
    print("%s %s: plain fp32 uses %.3f of the element-wise bound" % (group.name, dc.shape_id(shape), worst))
    assert not bad, "\n".join(bad)


def passing_case(group_name, shape, n, stat=False, act=dc.LEAKY):
    group = next(g for g in dc.GROUPS if g.name == group_name)
    slot_major = group.kind in ("slots", "f16")
    a, w, b, rec = dc.make_inputs(group, shape, n, stat)
    ref = do.reference(a, w, b, act, rec, slot_major)
    got = fp32_op(a, w, b, act, rec, slot_major)
    assert not do.gate_failures(got, ref, act)
    return a, w, b, rec, ref, got


def test_gates_reject_a_repeated_last_row():
    *_, ref, got = passing_case("split11", (32, 200), 129)
    got = got.clone()
    got[-1] = got[-2]
    assert do.gate_failures(got, ref, dc.LEAKY)


def test_gates_reject_a_zeroed_last_column_of_a_ragged_width():
    *_, ref, got = passing_case("mfma-fast", (256, 17), 127)
    got = got.clone()
    got[:, -1] = 0
    assert do.gate_failures(got, ref, dc.LEAKY)


def test_elementwise_gate_rejects_swapped_slots_the_max_norm_gate_accepts():
    """Slot 2 at 2^-10 of the others' magnitude, read in slot 1's place and the other way round (a slot read at the wrong
    stride), in a layer with one large output column (a bias of 2^22): every other column is wrong by the size of its own
    values, which max|a - b| / max|b| puts at 1e-6 of that one column."""
    group = next(g for g in dc.GROUPS if g.name == "slots")
    a, w, b, _ = dc.make_inputs(group, (5, 64, 64), 129)
    a[2] *= 2.0 ** -10
    b[0] = 2.0 ** 22
    ref = do.reference(a, w, b, dc.NONE, None, True)
    assert not do.gate_failures(fp32_op(a, w, b, dc.NONE, None, True), ref, dc.NONE)
    swapped = a.clone()
    swapped[1], swapped[2] = a[2], a[1]
    got = fp32_op(swapped, w, b, dc.NONE, None, True)
    rel, ratio = do.measure(got, ref, dc.NONE)
    assert rel < do.REL_MAX_TOL, rel                # the project's metric alone would have accepted it
    assert ratio > 1.0 and do.gate_failures(got, ref, dc.NONE)


def test_partial_sum_check_rejects_one_missing_row():
    *_, got = passing_case("split11", (128, 64), 4099)
    m = got.shape[1]
    chunks = got.split(128)
    rows = torch.stack([do.column_sums(c) for c in chunks])
    assert not do.partial_failures(rows, len(chunks), got, True)
    rows[7, 5] -= float(got[7 * 128 + 127, 5])                          # the block's last row masked out of one column's sum
    assert do.partial_failures(rows, len(chunks), got, True)
    rows = torch.stack([do.column_sums(c) for c in chunks])
    rows[-1, m + 3] -= float(got[-1, 3]) ** 2
    assert do.partial_failures(rows, len(chunks), got, True)
    assert do.partial_failures(rows, 0, got, True) and do.partial_failures(rows, 513, got, True)
    assert do.partial_failures(rows, 3, got, True, out1_kernel=True) and not do.partial_failures(rows, 0, got, True, out1_kernel=True)


def test_gates_reject_a_batchnorm_on_load_without_the_means_low_half():
    v, w, b, rec = dc.near_constant_case()
    ref = do.reference(v, w, b, dc.NONE, rec)
    assert not do.gate_failures(fp32_op(v, w, b, dc.NONE, rec), ref, dc.NONE)
    dropped = rec.clone()
    dropped[1] = 0
    assert float(rec[1].abs().max()) > 2e-6                              # (the low half is there to be dropped)
    assert do.gate_failures(fp32_op(v, w, b, dc.NONE, dropped), ref, dc.NONE)


def test_every_case_lands_on_a_kernel_its_group_names_and_every_kernel_is_reached():
    for group in dc.GROUPS:
        assert dc.group_kernels(group) == group.kernels, group.name
    assert dc.group_kernels(dc.ROWS_GROUP, modes=dc.ROWS_MODES) == dc.ROWS_GROUP.kernels
    # the thresholds the row counts are chosen by
    assert dc.dispatch("plain", 256, 1, 8200) == "out1<64>" and (8200 * 64 + 255) // 256 > 2048
    assert (131372 + 255) // 256 > do.MAX_PARTIALS
    assert 1024 // 128 == 8 and 17408 // 128 == 136 and 136 % 8 == 0 and (16385 + 127) // 128 == 129
    for mode, want in ((2, "rows<8>"), (0, "rows<8>"), (3, "rows2<8>"), (6, "halves<8,4>"), (10, "halves<8,4>")):
        assert dc.dispatch("f16", 672, 256, 49152, 32, f16=True, wimg=True, rows_mode=mode) == want
    assert dc.dispatch("f16", 672, 256, 49151, 32, f16=True, wimg=True) == "split<2,2,f16>"
