"""CPU: training on compacted histories -- the length-group identity on the float64 oracle (loss, logits and every
gradient of a training-mode step, two hand-made groupings and the trivial one), the group planner against brute force over all
contiguous partitions, host-side validation of the three new C-ABI entries, and the new ops' registration and fake-tensor shapes.

Gates: float64 against float64 -- logits 1e-12 relative, gradients 1e-11 of the tensor's max-norm (3.9e-13 was measured on the worst
tensor, instant_interest_model.out_fc.0.bias, whose entries are sums that cancel: DESIGN.md section 2); delta and out_mlp.fc2.bias have an
exactly zero gradient (softmax is shift invariant) and are compared absolutely.  The mutant with w_g = 1 must move the logits by more
than 1e-3, or the inputs do not exercise the weight."""
import ctypes

import numpy as np
import pytest
import torch

from history_train_util import H_ID, HAND_GROUPINGS, L_LIST, brute_force_rows, grouped_oracle, hand_plan, oracle_step, padded_batch, quantised_height
from news_recommendation_model_amd import compact

ZERO_GRAD = ("delta", "out_mlp.fc2.bias")


@pytest.fixture(scope="module")
def identity_case():
    from news_recommendation_model_amd import synth
    from news_recommendation_model_amd.config import Dims
    from oracle import user_model_oracle as orc
    dims = Dims.for_emb(64, category_label_num=50)
    batch = padded_batch(dims, L_LIST, H_ID, 3, seed=23)
    sd = synth.make_state_dict(dims, seed=1, user_num=int(batch["user_num"]))
    return orc, sd, batch, oracle_step(orc, sd, batch)


PLANNED_GROUPINGS = {"planner, 4 groups, quantum 1": dict(max_groups=4, quantum=1), "planner, 3 groups, quantum 16": dict(max_groups=3, quantum=16)}


@pytest.mark.parametrize("grouping", sorted(HAND_GROUPINGS) + sorted(PLANNED_GROUPINGS))
def test_length_groups_equal_the_dense_step_in_float64(identity_case, grouping):
    orc, sd, batch, (loss_d, r_d, g_d) = identity_case
    if grouping.startswith("planner"):                 # the package's own plan (the identity needs nothing but its tables)
        plan = compact.plan_history_groups(L_LIST, H_ID, **PLANNED_GROUPINGS[grouping])
    else:
        sizes, heights = HAND_GROUPINGS[grouping]
        plan = hand_plan(L_LIST, H_ID, sizes, heights)
        best = compact.plan_history_groups(L_LIST, H_ID, max_groups=len(sizes), quantum=1)
        assert best.R <= plan.R and best.perm.tolist() == plan.perm.tolist()          # the planner never keeps more rows than a hand-made grouping
    with grouped_oracle(orc, plan):
        loss_g, r_g, g_g = oracle_step(orc, sd, batch)
    assert r_g.dtype == torch.float64
    print(f"{grouping}: {plan.R} of {plan.B * plan.H} rows; loss {float(loss_g):.15g} against {float(loss_d):.15g}")
    worst = float((r_g - r_d).abs().max() / r_d.abs().max())
    print(f"  logits: worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    assert abs(float(loss_g) - float(loss_d)) <= 1e-12 * abs(float(loss_d))
    assert sorted(g_g) == sorted(g_d)
    for k in sorted(g_d):
        diff = float((g_g[k] - g_d[k]).abs().max())
        if k in ZERO_GRAD:
            print(f"  {k}: |gradient| {float(g_d[k].abs().max()):.1e} dense, absolute difference {diff:.1e}")
            assert diff <= 1e-11
            continue
        rel = diff / float(g_d[k].abs().max())
        print(f"  {k}: {rel:.2e} of its max-norm")
        assert rel <= 1e-11, k
    if plan.G > 1:                                     # teeth: the same groups without the multiplicity
        with grouped_oracle(orc, plan, use_weight=False):
            _l, r_m, _g = oracle_step(orc, sd, batch)
        moved = float((r_m - r_d).abs().max())
        print(f"  mutant w_g = 1 moves the logits by {moved:.2e}")
        assert moved > 1e-3


PLAN_CASES = {
    "the L list": (L_LIST, 37),
    "the L list, first eight": (L_LIST[:8], 37),
    "L all 0": ([0] * 6, 37),
    "L all H": ([37] * 5, 37),
    "one impression": ([12], 37),
    "entries outside [0, H] are clamped": ([-4, 99, 7, 20, 3], 24),
    "ties and a long tail": ([3, 3, 3, 3, 40, 3, 17, 3], 40),
}


@pytest.mark.parametrize("quantum", [1, 16])
@pytest.mark.parametrize("what", sorted(PLAN_CASES))
def test_planner_matches_brute_force_over_all_contiguous_partitions(what, quantum):
    lengths, H = PLAN_CASES[what]
    L = np.clip(np.asarray(lengths), 0, H)
    B = len(L)
    for max_groups in (1, 2, 3, 4):
        plan = compact.plan_history_groups(np.asarray(lengths), H, max_groups=max_groups, quantum=quantum)
        assert (plan.B, plan.H, plan.quantum) == (B, H, quantum) and 1 <= plan.G <= max_groups
        assert plan.R == brute_force_rows(lengths, H, max_groups, quantum), (what, max_groups, quantum)
        assert plan.hist_len.tolist() == L.tolist()
        assert plan.perm.tolist() == sorted(range(B), key=lambda b: (L[b], b))           # stable
        assert plan.inverse[plan.perm].tolist() == list(range(B))
        assert plan.bounds[0] == 0 and plan.bounds[-1] == B and (np.diff(plan.bounds) > 0).all()
        assert plan.w_g.tolist() == (H - plan.H_g + 1).tolist()
        assert plan.row_off.tolist() == np.concatenate([[0], np.cumsum(np.diff(plan.bounds) * plan.H_g)]).tolist() and plan.R == plan.row_off[-1]
        for g in range(plan.G):
            members = L[plan.perm[plan.bounds[g]:plan.bounds[g + 1]]]
            assert plan.H_g[g] == quantised_height(int(members.max()), H, quantum)
            assert plan.H_g[g] == H or (plan.H_g[g] >= members + 1).all()
        assert plan.saving == pytest.approx(1 - plan.R / (B * H))
        assert plan.dense == (bool((plan.H_g == H).all()) or plan.saving < compact.MIN_SAVING)
        for k in ("perm", "inverse", "bounds", "H_g", "w_g", "row_off", "hist_len"):
            assert getattr(plan, k).dtype == np.int32


def test_planner_edge_cases_and_tables():
    assert compact.plan_history_groups([37] * 5, 37, max_groups=4).dense
    empty = compact.plan_history_groups([], 37)
    assert (empty.B, empty.G, empty.R, empty.dense) == (0, 0, 0, True)
    plan = compact.plan_history_groups(L_LIST, 37, max_groups=3, quantum=1)
    assert not plan.dense and plan.H_g.tolist() == [6, 18, 37] and plan.R == 164
    tabs = plan.upload("cpu")                                    # one buffer, five views
    assert tabs["_host"].numel() == 2 * 9 + 2 * 4 + 3
    for k in ("perm", "inverse", "bounds", "row_off", "H_g"):
        assert tabs[k].dtype == torch.int32 and tabs[k].tolist() == getattr(plan, k).tolist()
    assert compact.plan_history_groups(torch.tensor(L_LIST), 37, max_groups=3, quantum=1).bounds.tolist() == plan.bounds.tolist()
    for bad in (dict(H=0), dict(quantum=0), dict(max_groups=0), dict(max_groups=65)):
        with pytest.raises(ValueError):
            compact.plan_history_groups(L_LIST, **{"H": 37, **bad})
    assert compact.MAX_GROUPS == 2 and compact.MIN_SAVING == 0.25      # the unmeasured, conservative defaults


def test_new_entries_validate_on_the_host(lib):
    f = ctypes.c_void_p(0x1000)
    assert lib.nrm_abi_version() == 7

    def gather(x=f, perm=f, out=f, cols=80, G=3, B=9, H=37, R=164):
        return lib.nrm_history_gather_groups(x, cols, 1, perm, f, f, f, G, B, H, R, out, None)
    for what, kw in {"null input": dict(x=None), "null table": dict(perm=None), "null output": dict(out=None), "negative B": dict(B=-1),
                     "negative R": dict(R=-1), "R > B H": dict(R=334), "cols = 0": dict(cols=0), "G > 64": dict(G=65), "negative G": dict(G=-1),
                     "rows without a group": dict(G=0)}.items():
        assert gather(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_history_gather_groups"), (what, lib.nrm_last_error())
    assert gather(R=0) == 0 and gather(B=0, R=0) == 0            # nothing to do: no launch

    def bmm(W=f, X=f, out=f, B=2, I=3, J=17, D=64, ldx=64, w=2.0, row=0):
        return lib.nrm_pool_bmm_wlast(W, 51, 17, 1, X, ldx, out, B, I, J, D, 0, ctypes.c_float(w), row, None)
    for what, kw in {"null W": dict(W=None), "null X": dict(X=None), "null out": dict(out=None), "negative B": dict(B=-1), "I = 0": dict(I=0),
                     "negative J": dict(J=-2), "D % 4": dict(D=66, ldx=68), "ldx < D": dict(ldx=60), "unaligned X": dict(X=ctypes.c_void_p(0x1004)),
                     "w < 1": dict(w=0.5), "w = 0": dict(w=0.0), "w NaN": dict(w=float("nan")), "unknown placement": dict(row=2)}.items():
        assert bmm(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_pool_bmm_wlast"), (what, lib.nrm_last_error())
    assert bmm(B=0) == 0

    def rowdot(g=f, h=f, ds=f, B=2, T=3, H=17, D=64, ldg=64, w=2.0, zero=f, zn=68):
        return lib.nrm_pool_rowdot_wlast(g, ldg, h, ds, B, T, H, D, zero, zn, ctypes.c_float(w), None)
    for what, kw in {"null g": dict(g=None), "null h": dict(h=None), "null ds": dict(ds=None), "negative B": dict(B=-1), "T = 0": dict(T=0),
                     "negative H": dict(H=-1), "D % 4": dict(D=66, ldg=68), "D > 1024": dict(D=1028, ldg=1028), "ldg < D": dict(ldg=32),
                     "w < 1": dict(w=0.99), "w NaN": dict(w=float("nan")), "zero_n without zero_out": dict(zero=None)}.items():
        assert rowdot(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_pool_rowdot_wlast"), (what, lib.nrm_last_error())


def test_new_ops_are_registered_with_fakes_and_refuse_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from news_recommendation_model_amd import ops
    for name in ("attend_pool_grouped_fwd", "attend_pool_grouped_bwd", "history_gather_groups"):
        assert name in ops.OPS and hasattr(torch.ops.nrm, name)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.history_gather_groups(torch.zeros(2, 3, 4), i32(1, 0), i32(0, 2), i32(0, 4), i32(2), 4)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.attend_pool_grouped_fwd(torch.zeros(6, 8), torch.zeros(4, 8), torch.zeros(8, 32), torch.zeros(8), torch.zeros(1, 8),
                                              torch.zeros(1), [0, 2], [2], [3], 5, 3, False, 0)
    with FakeTensorMode():
        c = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")      # noqa: E731
        i = lambda n: c(n, dtype=torch.int32)                    # noqa: E731
        xh = torch.ops.nrm.history_gather_groups(c(9, 37, 80, dtype=torch.float64), i(9), i(4), i(4), i(3), 164)
        assert (tuple(xh.shape), xh.dtype) == ((164, 80), torch.float64)
        b0, hg, tg = [0, 3, 7, 9], [6, 18, 37], [5, 5, 5]
        S = (((3 * 5 * 6 + 63) // 64 * 64 + 4 * 5 * 18 + 63) // 64 * 64 + 2 * 5 * 37 + 63) // 64 * 64
        for save_z in (True, False):
            pooled, s, z = torch.ops.nrm.attend_pool_grouped_fwd(c(9 * 5, 16), c(164, 16), c(16, 64), c(16), c(1, 16), c(1), b0, hg, tg, 37, 5, save_z, 0)
            assert (tuple(pooled.view(9, 5, 16).shape), tuple(s.shape), tuple(z.shape)) == ((9, 5, 16), (S,), (164 * 5 * 16 if save_z else 0,))
        for need_dt, need_dh in ((True, True), (False, False)):
            dt, dh, dw1, db1, acc = torch.ops.nrm.attend_pool_grouped_bwd(c(9 * 5, 16), c(9 * 5, 16), c(164, 16), c(16, 64), c(1, 16), c(S), c(164 * 5 * 16),
                                                                          b0, hg, tg, 37, 5, 0, need_dt, need_dh)
            assert tuple(dt.view(-1, 5, 16).shape if need_dt else dt.shape) == ((9, 5, 16) if need_dt else (0,))
            assert tuple(dh.shape) == ((164, 16) if need_dh else (0,))
            assert (tuple(dw1.shape), tuple(db1.shape), tuple(acc.shape)) == ((16, 64), (16,), (20,))


def test_merged_grouped_node_fakes_are_the_3d_forms_reshaped():
    """The one grouped attention + pool node on a uniform-T plan of 3 groups (B = 9, T = 5, H = 37, D = 16): its fake shapes are what the
    node that took t as [B, T, D] returned, reshaped -- pooled and dt [B * T, D], s [S] with every group's block on a 256-byte boundary,
    z [Z * D] with Z = R * T, dh [R, D] -- written out here without the layout helper the fakes use."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    B, T, H, D = 9, 5, 37, 16
    b0, hg = [0, 3, 7, 9], [6, 18, 37]
    n = [b0[g + 1] - b0[g] for g in range(3)]
    R = sum(n[g] * hg[g] for g in range(3))
    Z = R * T
    S = sum((n[g] * T * hg[g] + 63) // 64 * 64 for g in range(3))
    assert (R, S) == (164, 896)
    with FakeTensorMode():
        c = lambda *s: torch.empty(*s, dtype=torch.float32, device="cuda")      # noqa: E731
        w = (c(D, 4 * D), c(D), c(1, D), c(1))
        for save_z in (True, False):
            pooled, s, z = torch.ops.nrm.attend_pool_grouped_fwd(c(B * T, D), c(R, D), *w, b0, hg, [T] * 3, H, T, save_z, 0)
            assert [tuple(x.shape) for x in (pooled, s, z)] == [(B * T, D), (S,), (Z * D if save_z else 0,)]
            assert pooled.dtype == s.dtype == z.dtype == torch.float32
        for need_dt, need_dh in ((True, True), (True, False), (False, True), (False, False)):
            out = torch.ops.nrm.attend_pool_grouped_bwd(c(B * T, D), c(B * T, D), c(R, D), w[0], w[2], c(S), c(Z * D), b0, hg, [T] * 3, H, T, 0,
                                                        need_dt, need_dh)
            assert [tuple(x.shape) for x in out] == [(B * T, D) if need_dt else (0,), (R, D) if need_dh else (0,), (D, 4 * D), (D,), (D + 4,)]
        with pytest.raises(RuntimeError, match="not a partition"):       # a group_t that does not go with group_h
            torch.ops.nrm.attend_pool_grouped_fwd(c(B * T, D), c(R, D), *w, b0, hg, [T] * 2, H, T, True, 0)


def test_model_and_trainer_interfaces_without_a_gpu():
    import inspect
    from news_recommendation_model_amd import modules, trainer
    m = modules.UserModel(3).train()
    assert m.compact_history_applies()                                # the reference's default widths (64 / 400... multiples of 4)
    m.invariant_interest_model.label_attention.mlp.activation = torch.nn.ReLU()
    assert not m.compact_history_applies()                            # a non-GELU MLP: the step runs dense
    m = modules.UserModel(3)
    m.invariant_interest_model.register_forward_hook(lambda *a: None)
    assert not m.compact_history_applies()                            # a hooked sub-model
    for fn in (trainer.train_step, trainer.train_epochs):
        assert inspect.signature(fn).parameters["compact_history"].default is False
    with pytest.raises(RuntimeError, match="captured step"):
        trainer.GraphedTrainStep(None, None, None, compact_history=True)
    with pytest.raises(RuntimeError, match="inference only"):         # (unchanged: forward_compact stays an inference entry)
        modules.UserModel(3).train().forward_compact(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3), compact.build_plan([0], 2, history_len=[1], H=2))
