"""CPU: history compaction of the compact scoring path -- the identity it rests on, on the float64 oracle (the
trailing all-zero history rows of an impression all have the same score and the same history row, so one representative row weighted
by their number replaces them), the plan's history tables against a brute-force loop, host-side validation of the new C-ABI entry
points, the ops' registration and fake-tensor shapes, and what must not change (the two-argument plan, the training-mode refusal).

Gates: float64 against float64 at 1e-12 relative (summation order only: 200 addends bound it by 200 * 2^-53 ~ 2e-14); the mutant
without the factor H - L_b must miss that gate by more than 10^6 x on the label attention, or the inputs do not exercise it."""
import ctypes

import numpy as np
import pytest
import torch

from compact_util import brute_force_plan
from history_compact_util import L_LIST, brute_force_history_plan, cut_history, eval_logits_from_eu_H, weighted_eu_H
from news_recommendation_model_amd import compact

GATE = 1e-12


def _oracle_case():
    from news_recommendation_model_amd import synth
    from news_recommendation_model_amd.config import Dims
    from oracle import user_model_oracle as orc
    dims = Dims.for_emb(64, category_label_num=50)
    H, T = 37, 5
    L = L_LIST(H)
    batch = cut_history(synth.make_batch(dims, len(L), H, T, seed=17), L)
    p = orc.to_torch_params(synth.make_state_dict(dims, seed=1), requires_grad=False, dtype=torch.float64)
    tb = {k: torch.from_numpy(batch[k]) for k in ("x_history", "x_target", "x_global")}
    return orc, p, tb, L, H


def _rel(a, b):
    """worst per-impression |a - b| / max |b|"""
    return max(float((a[i] - b[i]).abs().max() / b[i].abs().max()) for i in range(a.shape[0]))


def test_weighted_formula_equals_the_dense_oracle_in_float64():
    orc, p, tb, L, H = _oracle_case()
    with orc.precision(torch.float64), torch.no_grad():
        eu_dense, _ec = orc.invariant_interest(p, tb["x_history"], tb["x_target"])
        eu_w = weighted_eu_H(orc, p, tb["x_history"], tb["x_target"], L)
        eu_mut = weighted_eu_H(orc, p, tb["x_history"], tb["x_target"], L, use_mult=False)
        assert eu_dense.dtype == torch.float64 and eu_w.dtype == torch.float64
        worst = _rel(eu_w, eu_dense)
        print(f"eu_H, weighted formula against the dense oracle, float64: worst relative difference {worst:.2e}")
        assert worst <= GATE
        # teeth: without the multiplicity the label attention's pool is far off wherever more than one padded row was dropped
        D_l = p["invariant_interest_model.label_attention.mlp.fc2.weight"].shape[1]
        short = [b for b in range(len(L)) if H - L[b] > 1]
        miss = min(float((eu_mut[b, :, :D_l] - eu_dense[b, :, :D_l]).abs().max() / eu_dense[b, :, :D_l].abs().max()) for b in short)
        print(f"mutant without the factor H - L_b: smallest relative miss on the label attention {miss:.2e}")
        assert miss > 1e6 * GATE
        # the same through the logits of the eval-mode model
        r_dense = orc.user_model_forward(p, tb["x_history"], tb["x_target"], tb["x_global"], training=False)
        r_w = eval_logits_from_eu_H(orc, p, eu_w, tb["x_target"], tb["x_global"])
        r_self = eval_logits_from_eu_H(orc, p, eu_dense, tb["x_target"], tb["x_global"])
        assert torch.equal(r_self, r_dense)                      # the helper IS the oracle's head
        worst = _rel(r_w, r_dense)
        print(f"logits, weighted formula against the dense oracle, float64: worst relative difference {worst:.2e}")
        assert worst <= GATE


HIST_PLAN_CASES = {
    # name: (empty_num, T, history_len, H)
    "L all 0": ([1, 0, 3], 5, [0, 0, 0], 20),
    "L all H": ([1, 0, 3], 5, [20, 20, 20], 20),
    "B = 0": ([], 5, [], 20),
    "K in {1, 15, 16, 17}": ([0, 2, 1, 4], 6, [0, 14, 15, 16], 40),
    "K = 16 and 17 by a full history": ([0, 2], 6, [16, 17], 17),
    "an impression with zero candidates": ([2, 7, 0, 7], 7, [3, 9, 0, 33], 33),
    "entries outside [0, H] are clamped": ([0, 1, 2], 4, [-3, 99, 7], 12),
    "H = 0": ([0, 1], 3, [0, 0], 0),
}


@pytest.mark.parametrize("what", sorted(HIST_PLAN_CASES))
def test_history_plan_matches_brute_force(what):
    empty, T, L, H = HIST_PLAN_CASES[what]
    want_c = brute_force_plan(empty, T)
    counts = np.diff(np.asarray(want_c["cand_off"], dtype=np.int64))
    want = brute_force_history_plan(counts, L, H)
    for l_in in (np.array(L, dtype=np.int32), torch.tensor(L, dtype=torch.int32), list(L)):
        plan = compact.build_plan(np.array(empty, dtype=np.int64), T, history_len=l_in, H=H)
        for k in ("cand_off", "cand_imp", "src", "pad_mult", "live"):          # today's keys keep their contents
            assert getattr(plan, k).tolist() == want_c[k], (what, k)
        for k in ("hist_len", "hist_mult", "hist_off", "hist_src", "tile_pre"):
            got = getattr(plan, k)
            assert got.dtype == np.int32 and got.tolist() == want[k], (what, k, got.tolist(), want[k])
        assert (plan.R, plan.k_max, plan.Mt, plan.history_dense, plan.H) == (want["R"], want["k_max"], want["Mt"], want["history_dense"], H), what
        assert plan.has_history
    with pytest.raises(ValueError):
        compact.build_plan(np.array(empty, dtype=np.int64), T, history_len=list(L) + [1], H=H)
    with pytest.raises(ValueError):
        compact.build_plan(np.array(empty, dtype=np.int64), T, history_len=L)          # H is required


def test_plan_without_the_keyword_is_todays_plan():
    empty, T = [4, 3, 6, 3, 5], 9
    want = brute_force_plan(empty, T)
    plan = compact.build_plan(np.array(empty), T)
    for k in ("cand_off", "cand_imp", "src", "pad_mult", "live"):
        got = getattr(plan, k)
        assert got.dtype == np.int32 and got.tolist() == want[k]
    assert (plan.B, plan.T, plan.trim, plan.Tp, plan.N, plan.max_count) == (5, 9, want["trim"], want["Tp"], want["N"], 6)
    assert not plan.has_history and plan.hist_off is None and plan.tile_pre is None and plan.history_dense is None
    tabs = plan.upload("cpu")                                    # one buffer, today's three views, nothing else
    assert sorted(k for k in tabs if not k.startswith("_")) == ["cand_imp", "cand_off", "pad_mult"]
    assert tabs["_host"].numel() == 2 * 5 + 1 + plan.N
    hp = compact.build_plan(np.array(empty), T, history_len=[1, 2, 3, 4, 5], H=5)
    tabs = hp.upload("cpu")                                      # the history tables ride behind today's in the same buffer
    assert tabs["_host"].numel() == 2 * 5 + 1 + hp.N + 3 * 5 + 2
    for k in ("cand_off", "pad_mult", "cand_imp", "hist_off", "hist_mult", "tile_pre"):
        assert tabs[k].tolist() == getattr(hp, k).tolist(), k


def test_forward_compact_still_refuses_training_mode():
    from news_recommendation_model_amd import modules
    m = modules.UserModel(3).train()
    plan = compact.build_plan([0], 2, history_len=[1], H=2)
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_compact(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3), plan)


def test_history_entries_validate_on_the_host(lib):
    f = ctypes.c_void_p(0x1000)
    assert lib.nrm_abi_version() == 7

    def fwd(B=4, N=9, mc=5, R=30, Mt=12, km=10, D=64, mma=0, null=False, tab=f):
        p = None if null else f
        return lib.nrm_pwattn_fwd_hragged(p, f, f, f, f, f, f, f, f, f, f, f, tab, B, N, mc, R, Mt, km, D, mma, None)
    for what, kw in {"D % 4": dict(D=66), "D > 1024": dict(D=1028), "negative N": dict(N=-1), "max_count > N": dict(mc=10), "k_max > R": dict(km=31),
                     "16 Mt >= 2^31": dict(Mt=1 << 27), "[R, D] >= 2^31 bytes": dict(R=1 << 23, D=64), "null pointer": dict(null=True),
                     "unknown mma": dict(mma=7), "unaligned tile table": dict(tab=ctypes.c_void_p(0x1004))}.items():
        assert fwd(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_pwattn_fwd_hragged"), (what, lib.nrm_last_error())
    for mma in (1, 2):
        assert fwd(mma=mma) != 0
        assert b"fp32 arithmetic only" in lib.nrm_last_error() and b"bf16" in lib.nrm_last_error()
    assert fwd(N=0, mc=0) == 0 and fwd(B=0, N=0, mc=0) == 0 and fwd(Mt=0) == 0 and fwd(R=0, km=0) == 0          # nothing to do: no launch

    pool = lambda s=f, B=2, N=5, mc=3, R=9, Mt=5, km=4, D=16: lib.nrm_pool_bmm_hragged(s, f, f, f, f, f, f, B, N, mc, R, Mt, km, D, None)     # noqa: E731
    assert pool(s=None) != 0 and b"null" in lib.nrm_last_error()
    assert pool(D=18) != 0 and lib.nrm_last_error().startswith(b"nrm_pool_bmm_hragged")
    assert pool(mc=6) != 0 and pool(km=10) != 0 and pool(Mt=1 << 27) != 0
    assert pool(B=0, N=0, mc=0, R=0, Mt=0, km=0) == 0
    # no B <= 65535 refusal as in the dense pool entries: neither this entry nor nrm_pwattn_fwd_hragged in front of it has a grid dimension
    # per impression (the launch is a 1-D grid of tasks and refuses a task count past 2^31 workgroups), so the values pass validation
    assert pool(B=65536, R=0, Mt=0, km=0) == 0 and fwd(B=65536, R=0, km=0) == 0

    assert lib.nrm_history_len(None, 80, 1, 3, 5, f, None) != 0 and b"null" in lib.nrm_last_error()
    assert lib.nrm_history_len(f, 0, 1, 3, 5, f, None) != 0 and lib.nrm_last_error().startswith(b"nrm_history_len")
    assert lib.nrm_history_len(f, 80, 1, 3, 5, None, None) != 0
    assert lib.nrm_history_len(ctypes.c_void_p(0x1002), 80, 0, 3, 5, f, None) != 0
    assert lib.nrm_history_len(f, 80, 1, 0, 5, f, None) == 0
    gather = lambda x=f, B=3, H=5, R=9, km=4, out=f: lib.nrm_history_gather(x, 80, 1, f, B, H, R, km, out, None)     # noqa: E731
    for what, bad in {"k_max > H": gather(km=6), "R > B H": gather(R=16), "null input": gather(x=None), "null output": gather(out=None)}.items():
        assert bad != 0, what
    assert lib.nrm_last_error().startswith(b"nrm_history_gather")
    assert gather(R=0, km=0) == 0
    tiles = lambda tab=f, Mt=5, N=4: lib.nrm_history_tiles(f, f, f, f, 2, N, 9, Mt, tab, None)     # noqa: E731
    assert tiles(tab=None) != 0 and tiles(tab=ctypes.c_void_p(0x1008)) != 0 and tiles(Mt=1 << 27) != 0 and tiles(N=-1) != 0
    assert lib.nrm_last_error().startswith(b"nrm_history_tiles")
    assert tiles(Mt=0, N=0) == 0


def test_history_ops_are_registered_with_fakes_and_refuse_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from news_recommendation_model_amd import ops
    for name in ("history_len", "history_gather", "history_tiles", "attend_pool_hragged_fwd"):
        assert name in ops.OPS and hasattr(torch.ops.nrm, name)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)          # noqa: E731
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.history_len(torch.zeros(2, 3, 4))
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.history_gather(torch.zeros(2, 3, 4), i32(3), 4, 2)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.attend_pool_hragged_fwd(torch.zeros(5, 8), torch.zeros(4, 8), torch.zeros(8, 32), torch.zeros(8), torch.zeros(1, 8), torch.zeros(1),
                                              i32(5), i32(3), i32(3), i32(2), i32(3), i32(5, 4), 3, 2, 0)
    with FakeTensorMode():
        c = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")      # noqa: E731
        ci, off, mult = c(17, dtype=torch.int32), c(6, dtype=torch.int32), c(5, dtype=torch.int32)
        ln = torch.ops.nrm.history_len(c(5, 9, 30, dtype=torch.float64))
        assert (tuple(ln.shape), ln.dtype) == ((5,), torch.int32)
        xh = torch.ops.nrm.history_gather(c(5, 9, 30, dtype=torch.float64), off, 23, 7)
        assert (tuple(xh.shape), xh.dtype) == ((23, 30), torch.float64)
        tab = torch.ops.nrm.history_tiles(ci, off, off, off, 23, 21)
        assert (tuple(tab.shape), tab.dtype) == ((21, 4), torch.int32)
        pooled, s = torch.ops.nrm.attend_pool_hragged_fwd(c(17, 16), c(23, 16), c(16, 64), c(16), c(1, 16), c(1), ci, off, off, mult, off, tab, 6, 7, 0)
        assert (tuple(pooled.shape), tuple(s.shape), pooled.dtype, s.dtype) == ((17, 16), (16 * 21,), torch.float32, torch.float32)
