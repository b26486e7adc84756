"""CPU: training on compacted candidate lists -- the candidate planner against brute force over all contiguous
partitions, the candidate-group identity on the float64 oracle (loss, logits, batch statistics and every gradient of a training-mode
step; three hand-made groupings, the planner's own, and the plan combined with history groups), its three mutants, host-side validation
of the four new C-ABI entries, and the new ops' registration and fake-tensor shapes.

Gates: float64 against float64, as in test_history_train_cpu.py -- logits and loss 1e-12 relative, gradients 1e-11 of the tensor's
max-norm, batch mean and variance 1e-13 of their max-norm; delta and out_mlp.fc2.bias have an exactly zero gradient (softmax is shift
invariant) and are compared absolutely.  Each mutant (weight 1 in BatchNorm only, in the loss only, in bn_backward's column terms only)
must move the logits or a gradient by more than 1e-4 of its max-norm: seven orders of magnitude above the gate.
The two instant-interest gradients are sums that cancel: whatever the summation order, an evaluation carries an
absolute error of a few eps times the term-magnitude sum S of golden_util.instant_interest_grad_bounds, and |gradient| / S is 1e-4 .. 1e-3
for the bias.  The fp32 tests allow II_NOISE = 4e-6 (34 float32 eps) per unit of S; here the same 34 eps of float64 are allowed on top of
the relative gate (measured: 3.8e-12 of the bias's max-norm, with groups in another row order than the dense step's)."""
import ctypes

import numpy as np
import pytest
import torch

from candidate_train_util import (B_ID, COUNTS, H_ID, HAND_GROUPINGS, MUTANTS, T_ID, brute_force_rows, compact_oracle_step, dense_oracle_step,
                                  hand_plan, padded_batch)
from golden_util import II_B, II_NOISE, II_W, instant_interest_grad_bounds
from news_recommendation_model_amd import compact

ZERO_GRAD = ("delta", "out_mlp.fc2.bias")
II_NOISE64 = II_NOISE * 2.0 ** -29          # the same count of eps, float64 for float32


@pytest.fixture(scope="module")
def identity_case():
    from news_recommendation_model_amd import synth
    from news_recommendation_model_amd.config import Dims
    from oracle import user_model_oracle as orc
    dims = Dims.for_emb(64, category_label_num=50)
    batch = padded_batch(dims, COUNTS, H_ID, T_ID, seed=29)
    assert batch["x_target"].shape[:2] == (B_ID, T_ID)
    sd = synth.make_state_dict(dims, seed=1, user_num=int(batch["user_num"]))
    _bounds[id(batch)] = instant_interest_grad_bounds(sd, batch)
    return orc, sd, batch, dense_oracle_step(orc, sd, batch)


_bounds = {}


def _worst(got, want, bounds=None):
    """(worst relative difference over the logits, the loss, the statistics and the gradients, its name)"""
    (loss_g, r_g, g_g, st_g), (loss_d, r_d, g_d, st_d) = got, want
    figs = {"logits": float((r_g - r_d).abs().max() / r_d.abs().max()), "loss": abs(float(loss_g) - float(loss_d)) / abs(float(loss_d)),
            "batch mean": float((st_g[0] - st_d[0]).abs().max() / st_d[0].abs().max()),
            "batch variance": float((st_g[1] - st_d[1]).abs().max() / st_d[1].abs().max())}
    assert sorted(g_g) == sorted(g_d)
    for k in g_d:
        diff = float((g_g[k] - g_d[k]).abs().max())
        figs[k] = diff if k in ZERO_GRAD else diff / float(g_d[k].abs().max())
        if bounds is not None and k in bounds:          # the cancelling sums: what exceeds the eps-of-S allowance, in the same unit
            over = ((g_g[k] - g_d[k]).abs().numpy() - II_NOISE64 * bounds[k].reshape(tuple(g_d[k].shape))).max()
            print(f"  {k}: {figs[k]:.2e} of its max-norm before the allowance of {II_NOISE64:.1e} S")
            figs[k] = max(float(over), 0.0) / float(g_d[k].abs().max())
    return figs


def _assert_identity(figs, what):
    for k, v in sorted(figs.items()):
        print(f"  {what}: {k}: {v:.2e}")
        gate = 1e-12 if k in ("logits", "loss") else 1e-13 if k.startswith("batch") else 1e-11
        assert v <= gate, (what, k, v)


PLANNED = {"planner, 3 groups": 3, "planner, 2 groups": 2}


@pytest.mark.parametrize("grouping", sorted(HAND_GROUPINGS) + sorted(PLANNED))
def test_candidate_groups_equal_the_dense_step_in_float64(identity_case, grouping):
    orc, sd, batch, dense = identity_case
    if grouping in PLANNED:
        plan = compact.plan_candidate_groups(batch["empty_num"], T_ID, max_groups=PLANNED[grouping])
    else:
        sizes, widths = HAND_GROUPINGS[grouping]
        plan = hand_plan(COUNTS, T_ID, sizes, widths)
        best = compact.plan_candidate_groups(batch["empty_num"], T_ID, max_groups=len(sizes))
        assert best.N <= plan.N and best.perm.tolist() == plan.perm.tolist() and best.expand.shape == plan.expand.shape
    print(f"{grouping}: {plan.N} of {plan.B * plan.T} candidate rows")
    figs = _worst(compact_oracle_step(orc, sd, batch, plan), dense, _bounds[id(batch)])
    _assert_identity(figs, grouping)
    print(f"  worst: {max(figs.values()):.2e}")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_each_weight_is_needed(identity_case, mutant):
    """Teeth: the same groups with ONE of the three weights left out."""
    orc, sd, batch, dense = identity_case
    sizes, widths = HAND_GROUPINGS["3+3+3"]
    figs = _worst(compact_oracle_step(orc, sd, batch, hand_plan(COUNTS, T_ID, sizes, widths), mutant=mutant), dense)
    moved = {k: v for k, v in figs.items() if k not in ZERO_GRAD and not k.startswith("batch") and k != "loss"}
    worst = max(moved, key=moved.get)
    print(f"mutant {mutant}: moves {worst} by {moved[worst]:.2e} of its max-norm; logits {figs['logits']:.2e}")
    assert moved[worst] > 1e-4


def test_combined_history_and_candidate_groups_equal_the_dense_step(identity_case):
    """Both axes: the cuts are the history plan's, every group gets the width of its members; histories cut the way L_LIST is."""
    from history_compact_util import cut_history
    orc, sd, _batch, _dense = identity_case
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    H, lengths = 37, [0, 1, 15, 16, 17, 36, 37, 5, 16]
    batch = cut_history(padded_batch(dims, COUNTS, H, T_ID, seed=31, user_num=int(_batch["user_num"])), lengths)
    dense = dense_oracle_step(orc, sd, batch)
    hist = compact.plan_history_groups(lengths, H, max_groups=3, quantum=1)
    plan = compact.plan_candidate_groups(batch["empty_num"], T_ID, history_plan=hist)
    assert plan.perm.tolist() == hist.perm.tolist() and plan.bounds.tolist() == hist.bounds.tolist() and (plan.T_g < T_ID).any()
    kept = float((np.diff(plan.bounds) * plan.T_g * hist.H_g).sum())
    assert plan.saving == pytest.approx(1 - kept / (B_ID * T_ID * H))
    figs = _worst(compact_oracle_step(orc, sd, batch, plan, hist=hist.H_g), dense, instant_interest_grad_bounds(sd, batch))
    _assert_identity(figs, "history x candidates")


def test_planner_matches_brute_force_on_random_counts():
    rng = np.random.default_rng(5)
    for case in range(60):
        B, T = int(rng.integers(1, 11)), int(rng.integers(1, 16))
        empty = rng.integers(-2, T + 3, B)                    # out of range on both sides: clamped
        n = T - np.clip(empty, 0, T)
        for max_groups in (1, 2, 3, 4):
            plan = compact.plan_candidate_groups(empty, T, max_groups=max_groups)
            assert plan.N == brute_force_rows(n, T, max_groups), (case, empty.tolist(), T, max_groups)
            assert (plan.B, plan.T) == (B, T) and 1 <= plan.G <= max_groups and plan.count.tolist() == n.tolist()
            assert plan.perm.tolist() == sorted(range(B), key=lambda b: (n[b], b))           # stable
            assert plan.inverse[plan.perm].tolist() == list(range(B))
            assert plan.bounds[0] == 0 and plan.bounds[-1] == B and (np.diff(plan.bounds) > 0).all()
            assert plan.w_g.tolist() == (T - plan.T_g + 1).tolist()
            assert plan.row_off.tolist() == np.concatenate([[0], np.cumsum(np.diff(plan.bounds) * plan.T_g)]).tolist() and plan.N == plan.row_off[-1]
            fewer = [compact.plan_candidate_groups(empty, T, max_groups=m) for m in range(1, max_groups)]
            assert all(f.N > plan.N or f.G == plan.G for f in fewer)                         # ties go to fewer groups
            for g in range(plan.G):
                members = n[plan.perm[plan.bounds[g]:plan.bounds[g + 1]]]
                assert plan.T_g[g] == min(T, int(members.max()) + 1)
            # expand: every dense cell maps to its own arena row, a dropped cell to its group's last column; all N rows are hit
            expand = plan.expand.reshape(B, T)
            for b in range(B):
                g = int(np.searchsorted(plan.bounds, plan.inverse[b], side="right") - 1)
                first = plan.row_off[g] + (plan.inverse[b] - plan.bounds[g]) * plan.T_g[g]
                assert expand[b].tolist() == [first + min(t, plan.T_g[g] - 1) for t in range(T)]
            assert sorted(set(expand.reshape(-1).tolist())) == list(range(plan.N))
            assert plan.saving == pytest.approx(1 - plan.N / (B * T))
            bound = compact.candidate_saving_bound(empty, T)             # what no grouping exceeds: train_step asks it before it plans
            assert plan.saving <= bound + 1e-12 and bound == pytest.approx(1 - np.minimum(T, n + 1).sum() / (B * T))
            assert plan.dense == (bool((plan.T_g == T).all()) or plan.saving < compact.MIN_SAVING)
            for k in ("perm", "inverse", "bounds", "T_g", "w_g", "row_off", "count", "expand"):
                assert getattr(plan, k).dtype == np.int32


def test_planner_edge_cases_and_tables():
    assert compact.plan_candidate_groups([0] * 5, 7, max_groups=4).dense                      # all-full lists
    assert compact.candidate_saving_bound([0] * 5, 7) == 0.0 and compact.candidate_saving_bound([], 7) == 0.0
    assert compact.candidate_saving_bound(torch.tensor([7, 7]), 7) == pytest.approx(6 / 7)
    same = compact.plan_candidate_groups([4] * 6, 7, max_groups=4)                            # all-equal lists: one group of width 4
    assert (same.G, same.T_g.tolist(), same.w_g.tolist(), same.N, same.dense) == (1, [4], [4], 24, False)
    empty = compact.plan_candidate_groups([], 7)
    assert (empty.B, empty.G, empty.N, empty.dense, empty.expand.shape) == (0, 0, 0, True, (0,))
    clamped = compact.plan_candidate_groups([-3, 99], 7, max_groups=2)                        # -> counts 7 and 0
    assert clamped.count.tolist() == [7, 0] and clamped.T_g.tolist() == [1, 7]
    plan = compact.plan_candidate_groups(T_ID - np.asarray(COUNTS), T_ID, max_groups=3)
    assert not plan.dense and plan.N == brute_force_rows(COUNTS, T_ID, 3)
    tabs = plan.upload("cpu")                                    # one buffer, five views
    assert tabs["_host"].numel() == 9 + 2 * (plan.G + 1) + plan.G + 9 * T_ID
    for k in ("perm", "bounds", "row_off", "T_g", "expand"):
        assert tabs[k].dtype == torch.int32 and tabs[k].tolist() == getattr(plan, k).tolist()
    assert compact.plan_candidate_groups(torch.tensor(T_ID - np.asarray(COUNTS)), T_ID, max_groups=3).bounds.tolist() == plan.bounds.tolist()
    for bad in (dict(T=0), dict(max_groups=0), dict(max_groups=65)):
        with pytest.raises(ValueError):
            compact.plan_candidate_groups([1, 2], **{"T": 7, **bad})
    with pytest.raises(ValueError):
        compact.plan_candidate_groups([1, 2], 7, history_plan=compact.plan_history_groups([1, 2, 3], 5))
    full = compact.full_height_history_plan(plan, 37)
    assert full.cand is plan and full.H_g.tolist() == [37] * plan.G and full.w_g.tolist() == [1] * plan.G and full.R == 9 * 37
    assert full.row_off.tolist() == (plan.bounds * 37).tolist() and full.perm is plan.perm
    assert compact.plan_history_groups([1, 2, 3], 5).cand is None


def test_new_entries_validate_on_the_host(lib):
    f = ctypes.c_void_p(0x1000)
    cf = ctypes.c_float

    def gather(xt=f, lab=f, perm=f, out=f, roww=f, flag=f, ct=80, cg=3, G=3, B=9, T=7, N=45):
        return lib.nrm_candidate_gather_groups(xt, ct, 1, f, cg, 1, lab, 1, perm, f, f, f, G, B, T, N, out, f, f, roww, flag, None)
    for what, kw in {"null input": dict(xt=None), "null label": dict(lab=None), "null table": dict(perm=None), "null output": dict(out=None),
                     "null weights": dict(roww=None), "null flag": dict(flag=None), "negative B": dict(B=-1), "T = 0": dict(T=0),
                     "negative N": dict(N=-1), "N > B T": dict(N=64), "cols = 0": dict(ct=0), "global cols = 0": dict(cg=0), "G > 64": dict(G=65),
                     "negative G": dict(G=-1), "impressions without a group": dict(G=0)}.items():
        assert gather(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_candidate_gather_groups"), (what, lib.nrm_last_error())
    assert gather(B=0, N=0) == 0                                 # nothing to do: no launch

    def colred(mode=0, x=f, mean=f, w=f, s0=f, R=5, N=8, ld=8):
        return lib.nrm_colreduce_roww(mode, x, mean, w, s0, R, N, ld, None)
    for what, kw in {"null x": dict(x=None), "null weights": dict(w=None), "null sums": dict(s0=None), "mode 1 without a mean": dict(mode=1, mean=None),
                     "mode 2 has no row-weight form": dict(mode=2), "negative mode": dict(mode=-1), "N % 4": dict(N=6), "ld < N": dict(ld=4),
                     "negative R": dict(R=-1)}.items():
        assert colred(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_colreduce_roww"), (what, lib.nrm_last_error())
    assert colred(R=0) == 0

    def bwd(x=f, dy=f, w=f, dx=f, s0=f, R=5, n_rows=9, N=8, ld=8):
        return lib.nrm_bn_backward_roww(x, dy, f, f, f, s0, f, None, w, dx, R, n_rows, N, ld, None)
    for what, kw in {"null x": dict(x=None), "null dy": dict(dy=None), "null weights": dict(w=None), "null dx": dict(dx=None), "null s0": dict(s0=None),
                     "fewer batch rows than launch rows": dict(n_rows=4), "N % 4": dict(N=6), "ld % 4": dict(ld=10)}.items():
        assert bwd(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_bn_backward_roww"), (what, lib.nrm_last_error())
    assert bwd(R=0) == 0

    def loss(out=f, lab=f, uid=f, dout=f, B=3, T=5, nd=4, w=2.0, inv=1 / 21, so=1, sd=4):
        return lib.nrm_loss_fwd_bwd_wlast(out, so, lab, 1, uid, f, nd, cf(0.95), B, T, cf(w), cf(inv), f, dout, sd, f, f, None)
    for what, kw in {"null out": dict(out=None), "null label": dict(lab=None), "null ids": dict(uid=None), "null dout": dict(dout=None), "negative B": dict(B=-1),
                     "T = 0": dict(T=0), "empty delta": dict(nd=0), "w < 1": dict(w=0.5), "w NaN": dict(w=float("nan")), "inv_n = 0": dict(inv=0.0),
                     "inv_n NaN": dict(inv=float("nan")), "stride 0": dict(so=0), "unaligned dout": dict(dout=ctypes.c_void_p(0x1004))}.items():
        assert loss(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_loss_fwd_bwd_wlast"), (what, lib.nrm_last_error())
    assert loss(B=0) == 0


NEW_OPS = ("candidate_gather_groups", "attend_pool_grouped_fwd", "attend_pool_grouped_bwd", "batch_norm_stats_roww", "batch_norm_apply_roww",
           "batch_norm_bwd_roww", "gate_block_roww_fwd", "gate_block_roww_bwd", "softmax_bce_loss_grouped")


def test_new_ops_are_registered_with_fakes_and_refuse_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from news_recommendation_model_amd import ops
    for name in NEW_OPS:
        assert name in ops.OPS and hasattr(torch.ops.nrm, name)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.candidate_gather_groups(torch.zeros(2, 3, 4), torch.zeros(2, 3, 3), torch.zeros(2, 3), i32(1, 0), i32(0, 2), i32(0, 4), i32(2), 4)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.batch_norm_stats_roww(torch.zeros(4, 8), torch.zeros(8), torch.ones(8), 0.1, 1e-5, torch.ones(4), 6)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.softmax_bce_loss_grouped(torch.zeros(4), torch.zeros(3), torch.zeros(4), torch.zeros(2, dtype=torch.int64), [0, 2], [2], 3, 0.95)
    with FakeTensorMode():
        c = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")      # noqa: E731
        i = lambda n: c(n, dtype=torch.int32)                    # noqa: E731
        xt, xg, lab, w = torch.ops.nrm.candidate_gather_groups(c(9, 7, 80, dtype=torch.float64), c(9, 7, 3, dtype=torch.float64), c(9, 7, dtype=torch.float64),
                                                               i(9), i(4), i(4), i(3), 45)
        assert [(tuple(t.shape), t.dtype) for t in (xt, xg, lab, w)] == [((45, 80), torch.float64), ((45, 3), torch.float64), ((45,), torch.float64),
                                                                         ((45,), torch.float32)]
        b0, hg, tg = [0, 3, 6, 9], [6, 18, 37], [3, 5, 7]
        S = (((3 * 3 * 6 + 63) // 64 * 64 + 3 * 5 * 18 + 63) // 64 * 64 + 3 * 7 * 37 + 63) // 64 * 64
        Z = 3 * 3 * 6 + 3 * 5 * 18 + 3 * 7 * 37
        R = 3 * 6 + 3 * 18 + 3 * 37
        for save_z in (True, False):
            pooled, s, z = torch.ops.nrm.attend_pool_grouped_fwd(c(45, 16), c(R, 16), c(16, 64), c(16), c(1, 16), c(1), b0, hg, tg, 37, 7, save_z, 0)
            assert (tuple(pooled.shape), tuple(s.shape), tuple(z.shape)) == ((45, 16), (S,), (Z * 16 if save_z else 0,))
        for need_dt, need_dh in ((True, True), (False, False)):
            dt, dh, dw1, db1, acc = torch.ops.nrm.attend_pool_grouped_bwd(c(45, 16), c(45, 16), c(R, 16), c(16, 64), c(1, 16), c(S), c(Z * 16),
                                                                          b0, hg, tg, 37, 7, 0, need_dt, need_dh)
            assert tuple(dt.shape) == ((45, 16) if need_dt else (0,)) and tuple(dh.shape) == ((R, 16) if need_dh else (0,))
            assert (tuple(dw1.shape), tuple(db1.shape), tuple(acc.shape)) == ((16, 64), (16,), (20,))
        mean, rstd = torch.ops.nrm.batch_norm_stats_roww(c(45, 24), c(24), c(24), 0.1, 1e-5, c(45), 63)
        assert tuple(mean.shape) == tuple(rstd.shape) == (24,)
        assert tuple(torch.ops.nrm.batch_norm_apply_roww(c(45, 24), mean, rstd, c(24), c(24), c(45), 63).shape) == (45, 24)
        loss, dout, ddelta = torch.ops.nrm.softmax_bce_loss_grouped(c(45), c(11), c(45, dtype=torch.float64), c(9, dtype=torch.int64), b0, tg, 7, 0.95)
        assert (tuple(loss.shape), tuple(dout.shape), dout.stride(), tuple(ddelta.shape)) == ((), (45,), (4,), (11,))


def test_model_and_trainer_interfaces_without_a_gpu():
    import inspect
    from news_recommendation_model_amd import modules, trainer
    m = modules.UserModel(3).train()
    assert m.compact_candidates_applies()
    m.gate.activation = torch.nn.ReLU()
    assert not m.compact_candidates_applies()                         # a non-GELU gate: the step runs dense
    m = modules.UserModel(3)
    m.bn = torch.nn.BatchNorm1d(m.bn.num_features, affine=False)
    assert not m.compact_candidates_applies()                         # the nn.BatchNorm1d fallback has no row-weight form
    m = modules.UserModel(3)
    m.bn = torch.nn.BatchNorm1d(m.bn.num_features, momentum=None)
    assert not m.compact_candidates_applies()
    m = modules.UserModel(3)
    m.invariant_interest_model.register_forward_hook(lambda *a: None)
    assert not m.compact_candidates_applies()                         # a hooked sub-model
    for fn in (trainer.train_step, trainer.train_epochs):
        assert inspect.signature(fn).parameters["compact_candidates"].default is False
    with pytest.raises(RuntimeError, match="captured step"):
        trainer.GraphedTrainStep(None, None, None, compact_candidates=True)
    with pytest.raises(KeyError, match="empty_num"):
        trainer.train_step(m, None, {"x_history": torch.zeros(1)}, compact_candidates=True)
    assert hasattr(modules.UserModel, "loss_grouped")
