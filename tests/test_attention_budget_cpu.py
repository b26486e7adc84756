"""CPU: the error budget of tests/attention_budget.py judges torch-CPU emulations of the attention kernels' arithmetic -- the correct
ones must pass with the constants the GPU tests use, and every mutant (a wrong activation, a lost product term, a lost row, a stale
block) must be rejected at 4 * M, so that neither verdict is marginal."""
import numpy as np
import pytest
import torch

import attention_budget as ab

SHAPES = [(3, 7, 19, 72), (2, 15, 200, 64), (2, 30, 32, 256), (2, 30, 50, 400), (5, 1, 3, 64), (1, 1, 1, 64), (2, 5, 7, 66)]
MUTANT_SHAPES = [(3, 7, 19, 72), (2, 30, 50, 400)]

# (mutant, arithmetic, family) combinations where a mutant does NOT reach 4 * M, and why.  Everything else is asserted.
_ACT = ("tanh_gelu", "gelu_grad_at_bf16_z")
NO_BITE = {}
for _a in ("f32", "bf16x3"):
    NO_BITE[("tanh_gelu", _a, "small")] = "tanh and erf GELU agree to 1e-9 on pre-activations of 1e-3: there is nothing to see"
for _m in _ACT:
    for _f in ("x8", "mixed"):
        # The bf16x3 yardstick is the emulation's own error, 10 .. 40 fp32 yardsticks wherever an operand has a non-zero lo part.  With
        # large inputs (x8, the loud impressions of mixed) most pre-activations sit in the saturated tails, where GELU is 0 or z
        # and GELU' is 0 or 1 whatever the formula or the rounding of z: the two activation mutants measure 11 .. 43 Y3 there, under
        # 4 * M_BF16X3 = 64.  On every other family they measure 98 .. 5200 Y3 and are asserted; in fp32 they are asserted on x8 and
        # mixed too (215 .. 1600 Y).
        NO_BITE[(_m, "bf16x3", _f)] = "saturated GELU tails: the activation error is of the order of the bf16x3 emulation's own error"
NO_BITE[("tanh_gelu", "bf16x3", "small")] = NO_BITE[("tanh_gelu", "f32", "small")]
NO_BITE[("drop_cross_term", "f32", None)] = "a mutant of the bf16x3 product only"

MUTANT_CASES = [(m, a, f) for m in ab.MUTANTS for a in ("f32", "bf16x3") for f in ab.FAMILIES
                if (m, a, f) not in NO_BITE and not (m == "drop_cross_term" and a == "f32")]


@pytest.mark.parametrize("family,B,T,H,D", [(f,) + s for f in ab.FAMILIES for s in SHAPES if not ab.family_is_degenerate(s, f)])
def test_correct_emulations_pass(family, B, T, H, D):
    case = ab.get_case((B, T, H, D), family)
    r = ab.assert_within_budget(ab.emulate(case, "f32"), case, "f32")
    # bf16x3: judged against a yardstick built from a second emulation that sums in another order (transposed operands, the
    # reduction split in two halves)
    r3 = ab.assert_within_budget(ab.emulate(case, "bf16x3", order=0), case, "bf16x3", order=1)
    print(f"{(B, T, H, D)} {family}: fp32 emulation {ab.worst(r):.2f} Y, bf16x3 emulation {ab.worst(r3):.2f} Y3")


@pytest.mark.parametrize("B,T,H,D", [(3, 7, 19, 72), (2, 30, 32, 256)])
@pytest.mark.parametrize("family", ab.FAMILIES)
def test_correct_emulations_of_the_fused_node_pass(family, B, T, H, D):
    case = ab.get_case((B, T, H, D), family, pool=True)
    ab.assert_within_budget(ab.emulate(case, "f32"), case, "f32")
    ab.assert_within_budget(ab.emulate(case, "bf16x3", order=0), case, "bf16x3", order=1)


@pytest.mark.parametrize("B,T,H,D", MUTANT_SHAPES)
@pytest.mark.parametrize("mutant,arithmetic,family", MUTANT_CASES)
def test_mutants_are_rejected(mutant, arithmetic, family, B, T, H, D):
    case = ab.get_case((B, T, H, D), family)
    got = ab.emulate(case, arithmetic, mutant=mutant)
    r = ab.ratios(got, case, arithmetic, order=1)
    (piece, norm), w, margin = ab.worst_margin(r, arithmetic)
    print(f"{mutant} / {arithmetic} / {family} {(B, T, H, D)}: {w:.0f} x the yardstick in {piece} ({norm}), M = {ab.m_of(piece, arithmetic)}")
    assert margin > 4, (piece, norm, w)
    with pytest.raises(AssertionError, match="over the .* error budget"):
        ab.assert_within_budget(got, case, arithmetic, order=1)


@pytest.mark.parametrize("B,T,H,D", MUTANT_SHAPES)
@pytest.mark.parametrize("mutant,arithmetic,family", [k for k in NO_BITE if k[2] in ("x8", "mixed")])
def test_unasserted_activation_mutants_stay_unseen(mutant, arithmetic, family, B, T, H, D):
    """Keeps NO_BITE honest: the two activation mutants in bf16x3 on saturated inputs really are below 4 * M_BF16X3 (at (2,30,50,400)
    even below M: they PASS the bf16x3 gate there -- a known limit).  If one of them rises above 4 * M the yardstick
    or the emulation has changed and the combination belongs among the asserted ones."""
    case = ab.get_case((B, T, H, D), family)
    r = ab.ratios(ab.emulate(case, arithmetic, mutant=mutant), case, arithmetic, order=1)
    _, w, margin = ab.worst_margin(r, arithmetic)
    print(f"{mutant} / {arithmetic} / {family} {(B, T, H, D)}: {w:.1f} Y3")
    assert margin <= 4, w


def test_families_say_where_they_degenerate():
    assert ab.family_is_degenerate((1, 1, 1, 64), "dup") and ab.family_is_degenerate((1, 1, 1, 64), "padded")
    for fam in ("dup", "padded"):
        a, b = ab.make_inputs(1, 1, 1, 64, fam), ab.make_inputs(1, 1, 1, 64, "normal")
        assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
        c, d = ab.make_inputs(5, 1, 3, 64, fam), ab.make_inputs(5, 1, 3, 64, "normal")
        assert not ab.family_is_degenerate((5, 1, 3, 64), fam) and not np.array_equal(c[2], d[2])


def test_mutants_confined_to_one_piece_are_seen_in_that_piece():
    """What one max-norm per tensor hides: stale_block is wrong in the W_d block of the fc1.weight gradient only, drop_row in no row
    tensor, and the quiet impression of `mixed` carries the error of a mutant that the loud one outweighs."""
    case = ab.get_case((2, 30, 50, 400), "normal")
    r = ab.ratios(ab.emulate(case, "f32", mutant="stale_block"), case, "f32")
    bad = {p for (p, n), v in r.items() if v > ab.M_F32}
    assert bad == {"d_fc1.weight[W_d]"}, bad
    r = ab.ratios(ab.emulate(case, "f32", mutant="drop_row"), case, "f32")
    bad = {p for (p, n), v in r.items() if v > ab.M_F32}
    assert bad and not bad & {"s", "d_target", "d_history"}, bad
    assert r[("d_fc2.bias", "max")] > 4 * ab.M_FC2_BIAS                     # the piece with its own constant still sees a lost row
    # a relative error of 1e-3 in the quiet last impression only (scaled 2**-6 against 2**3): one max-norm over the tensor sees a
    # fraction of it, the impression's own piece all of it
    case = ab.get_case((3, 7, 19, 72), "mixed")
    got = dict(ab.emulate(case, "f32"))
    ref = case.reference(torch.float64)
    got["d_history"] = got["d_history"].copy()
    got["d_history"][-1] *= 1.0 + 1e-3
    whole = np.abs(got["d_history"] - ref["d_history"]).max() / np.abs(ref["d_history"]).max()
    assert whole < 1e-3                                                     # ten times inside the 1e-2 gate of the whole tensor
    assert ab.ratios(got, case, "f32")[("d_history", "max")] > 4 * ab.M_F32


def test_yardstick_floor_is_one_fp32_roundoff():
    """The fc2.bias gradient is the plain sum of g.  With a small-integer g the fp32 oracle's sum is EXACT: its own error is 0, and a
    yardstick of 0 would reject any device sum that is one rounding off.  Such a piece is judged against 2**-23 instead."""
    B, T, H, D = 3, 7, 19, 72
    w, t, h, g = ab.make_inputs(B, T, H, D)
    g = (np.sign(g) * np.ceil(np.abs(g))).astype(np.float32)                # +-1, +-2, ...: non-zero everywhere
    if g.sum() == 0:
        g[0, 0, 0] += 1
    case = ab.Case(w, t, h, g)
    r64 = case.reference(torch.float64)
    raw = ab.errors(case.reference(torch.float32), r64, D)
    for norm in ("max", "l2"):
        assert raw[("d_fc2.bias", norm)] == 0.0
        assert case.yardstick("f32")[("d_fc2.bias", norm)] == ab.FLOOR
    assert min(v for k, v in case.yardstick("f32").items() if k[0] != "d_fc2.bias") > ab.FLOOR     # the others carry their own error
    got = dict(ab.emulate(case, "f32"))
    got["mlp.fc2.bias"] = r64["mlp.fc2.bias"] * (1.0 + 2.0 ** -23)          # the truth, one fp32 unit roundoff off
    r = ab.assert_within_budget(got, case, "f32")
    assert abs(r[("d_fc2.bias", "max")] - 1.0) < 1e-6
    got["mlp.fc2.bias"] = r64["mlp.fc2.bias"] * (1.0 + 8 * ab.M_FC2_BIAS * 2.0 ** -23)
    with pytest.raises(AssertionError, match="piece d_fc2.bias"):
        ab.assert_within_budget(got, case, "f32")


def test_a_zero_reference_piece_is_an_error_not_a_pass():
    w, t, h, g = ab.make_inputs(1, 1, 1, 64)
    case = ab.Case(w, t, t.copy(), g)                                       # t == h in the only pair: the W_d gradient block is exactly 0
    with pytest.raises(AssertionError, match="float64 reference is zero"):
        case.yardstick("f32")


def test_families_keep_the_upstream_gradient_non_zero_and_pad_the_history():
    for shape in SHAPES:
        for family in ab.FAMILIES:
            for pool in (False, True):
                w, t, h, g = ab.make_inputs(*shape, family=family, pool=pool)
                assert np.abs(g).min() > 0
                if family == "padded" and shape[2] >= 3:
                    assert not h[:, -1].any()


def test_forms_table_is_shared_with_the_row_containment_tests():
    import test_gpu_row_containment as rc
    assert rc.FORMS is ab.FORMS


def test_constants_follow_the_recorded_run():
    """M = the smallest power of two >= 4 x the worst ratio of that arithmetic in profiles/attention_error_budget.json."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention_error_budget.json")
    with open(path) as f:
        rec = json.load(f)
    for arith, m in (("f32", ab.M_F32), ("bf16x3", ab.M_BF16X3), ("d_fc2.bias", ab.M_FC2_BIAS)):
        worst = rec["worst_ratio"][arith]["ratio"]
        assert rec["M"][arith] == m
        assert m >= 4 * worst and m / 2 < 4 * worst, (arith, m, worst)
        assert m & (m - 1) == 0
