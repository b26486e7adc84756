"""CPU: the compact scoring path's host side -- the plan (compact.build_plan) against a brute-force loop, the identity the path rests
on (one representative padded candidate counted e' times in the first softmax = the reference's dense model_test) on the float64
oracle, host-side argument validation of the new C-ABI entry points (never-dereferenced pointers, nothing is launched) and the
registration / fake-tensor shapes of the new ops."""
import ctypes

import numpy as np
import pytest
import torch

from compact_util import brute_force_plan, pad_batch, percentile_counts
from news_recommendation_model_amd import compact


PLAN_CASES = {
    "no padding at all": ([0, 0, 0, 0], 7),
    "every row padded": ([3, 1, 6, 2], 7),
    "a row with no live candidate": ([2, 7, 0, 7], 7),
    "trim > 0": ([4, 3, 6, 3, 5], 9),
    "trim > 0, equal padding (dense after the trim)": ([2, 2, 2], 5),
    "B = 0": ([], 5),
    "T = 1": ([0, 1, 0], 1),
    "T = 1, all padded": ([1, 1], 1),
    "entries outside [0, T] are clamped": ([-2, 9, 1], 4),
}


@pytest.mark.parametrize("what", sorted(PLAN_CASES))
def test_plan_matches_brute_force(what):
    empty, T = PLAN_CASES[what]
    want = brute_force_plan(empty, T)
    for e_in in (np.array(empty, dtype=np.int64), torch.tensor(empty, dtype=torch.int64), np.array(empty, dtype=np.float64)):
        plan = compact.build_plan(e_in, T)
        assert (plan.B, plan.T, plan.trim, plan.Tp, plan.N) == (len(empty), T, want["trim"], want["Tp"], want["N"]), what
        for k in ("cand_off", "cand_imp", "src", "pad_mult", "live"):
            got = getattr(plan, k)
            assert got.dtype == np.int32 and got.tolist() == want[k], (what, k)
        counts = np.diff(want["cand_off"]) if want["cand_off"][1:] else np.zeros(0, dtype=int)
        assert plan.max_count == (int(counts.max()) if len(counts) else 0)
        assert plan.dense == (want["N"] == len(empty) * want["Tp"])


def test_plan_of_no_padding_is_the_dense_layout():
    plan = compact.build_plan(np.zeros(5, dtype=np.int64), 6)
    assert plan.N == 30 and plan.dense and plan.src.tolist() == list(range(30)) and plan.pad_mult.tolist() == [0] * 5
    assert plan.cand_imp.tolist() == [b for b in range(5) for _ in range(6)]


def test_plan_counts_on_percentile_lists():
    rng = np.random.default_rng(3)
    n = percentile_counts(rng, 80, 40)
    plan = compact.build_plan(40 - n, 40)
    assert plan.trim == 0 and plan.N == int(n.sum() + (n < 40).sum()) and plan.N < 0.5 * 80 * 40


def test_compact_formula_equals_model_test_in_float64():
    """The semantics, independent of any kernel: on a seeded padded batch (two models, common trim 3) the compact formula over
    n live logits + ONE padded logit counted e' times equals oracle.model_test_scores, both in float64, to 1e-12 relative."""
    from news_recommendation_model_amd import synth
    from news_recommendation_model_amd.config import Dims
    from oracle import user_model_oracle as orc
    dims = Dims.for_emb(64, category_label_num=50)
    B, H, T, trim = 24, 10, 30, 3
    rng = np.random.default_rng(11)
    counts = np.minimum(percentile_counts(rng, B, T, one_long=False), T - trim)
    counts[0] = T - trim                                        # the row that fixes the common trim
    counts[1] = 1
    batch = pad_batch(synth.make_batch(dims, B, H, T, seed=5), counts)
    plan = compact.build_plan(batch["empty_num"], T)
    assert plan.trim == trim and 0 < plan.N < B * plan.Tp
    tb = {k: torch.from_numpy(batch[k]) for k in ("x_history", "x_target", "x_global", "empty_num")}
    params = [orc.to_torch_params(synth.make_state_dict(dims, seed=s), requires_grad=False, dtype=torch.float64) for s in (1, 2)]
    with orc.precision(torch.float64):
        dense = orc.model_test_scores(params, tb)
        with torch.no_grad():
            logits = [orc.user_model_forward(p, tb["x_history"], tb["x_target"], tb["x_global"], training=False).numpy().reshape(-1)[plan.src]
                      for p in params]
    assert logits[0].dtype == np.float64
    got = compact.compact_scores_reference(logits, plan)
    worst = 0.0
    for b in range(B):
        n = int(plan.live[b])
        assert len(dense[b]) == n and dense[b].dtype == np.float64
        worst = max(worst, float(np.abs(got[b, :n] - dense[b]).max() / np.abs(dense[b]).max()))
        assert not got[b, n:].any()
    print(f"compact formula against model_test_scores, float64: worst relative difference {worst:.2e}")
    assert worst <= 1e-12


def _fake(n=1):
    return ctypes.c_void_p(0x1000 * n)


def test_ragged_attention_entry_validates_on_the_host(lib):
    f = _fake()

    def call(B=4, N=9, mc=5, H=6, D=64, mma=0, null=False):
        p = None if null else f
        return lib.nrm_pwattn_fwd_ragged(p, f, f, f, f, f, f, f, f, f, B, N, mc, H, D, mma, None)
    for what, kw in {"D % 4": dict(D=66), "D > 1024": dict(D=1028), "H = 0": dict(H=0), "negative N": dict(N=-1), "max_count > N": dict(mc=10),
                     "null pointer": dict(null=True), "unknown mma": dict(mma=7)}.items():
        assert call(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_pwattn_fwd_ragged"), (what, lib.nrm_last_error())
    for mma in (1, 2):                                          # bf16 / bf16x3: refused, and the message says why
        assert call(mma=mma) != 0
        assert b"fp32 arithmetic only" in lib.nrm_last_error() and b"bf16" in lib.nrm_last_error()
    assert call(N=0, mc=0) == 0 and call(B=0, N=0, mc=0) == 0   # nothing to do: no launch


def test_ragged_pool_tail_and_gather_entries_validate_on_the_host(lib):
    f = _fake()
    assert lib.nrm_pool_bmm_ragged(None, f, f, f, 2, 5, 3, 4, 16, None) != 0 and b"null" in lib.nrm_last_error()
    assert lib.nrm_pool_bmm_ragged(f, f, f, f, 2, 5, 3, 4, 18, None) != 0 and lib.nrm_last_error().startswith(b"nrm_pool_bmm_ragged")
    assert lib.nrm_pool_bmm_ragged(f, f, f, f, 2, 5, 6, 4, 16, None) != 0          # max_count > N
    assert lib.nrm_pool_bmm_ragged(f, f, f, f, 0, 0, 0, 4, 16, None) == 0

    cap = lib.nrm_ensemble_rank_max_candidates()
    ptrs, strides = (ctypes.c_void_p * 8)(*[0x1000] * 8), (ctypes.c_long * 8)(*[1] * 8)

    def tail(logits=ptrs, M=2, B=4, T=30, N=50, label=None, metrics=None, out=f, tabs=f, cols=strides):
        return lib.nrm_ensemble_rank_ragged(logits, cols, M, tabs, tabs, N, label, B, T, out, out, out, metrics, None)
    for what, kw in {"null logits": dict(logits=None), "M = 0": dict(M=0), "M = 9": dict(M=9), "T = 0": dict(T=0), "T = cap + 1": dict(T=cap + 1),
                     "label without metrics": dict(label=f), "metrics without label": dict(metrics=f), "null outputs": dict(out=None),
                     "null tables": dict(tabs=None), "negative B": dict(B=-1), "negative N": dict(N=-1),
                     "stride 0": dict(cols=(ctypes.c_long * 8)(*[0] * 8))}.items():
        assert tail(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_ensemble_rank_ragged") and len(lib.nrm_last_error()) > 28, (what, lib.nrm_last_error())
    assert tail(logits=(ctypes.c_void_p * 8)(0x1000, None)) != 0 and b"logits[1]" in lib.nrm_last_error()
    assert tail(B=0) == 0

    def gather(B=4, T=10, trim=2, N=20, tc=30, gc=3, xt=f, out=f, flag=f):
        return lib.nrm_compact_gather(xt, tc, 1, f, gc, 1, f, f, B, T, trim, N, out, out, flag, None)
    for what, kw in {"trim > T": dict(trim=11), "negative trim": dict(trim=-1), "T = 0": dict(T=0, trim=0), "N > B (T - trim)": dict(N=33),
                     "no columns": dict(tc=0), "null input": dict(xt=None), "null output": dict(out=None), "null flag": dict(flag=None)}.items():
        assert gather(**kw) != 0, what
        assert lib.nrm_last_error().startswith(b"nrm_compact_gather"), (what, lib.nrm_last_error())
    assert gather(B=0, N=0) == 0 and gather(trim=10, N=0) == 0                  # no kept cell: no launch


def test_compact_ops_are_registered_with_fakes_and_refuse_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from news_recommendation_model_amd import evaluation, modules, ops
    for name in ("compact_gather", "attend_pool_ragged_fwd", "ensemble_rank_ragged"):
        assert name in ops.OPS and hasattr(torch.ops.nrm, name)
    assert callable(evaluation.predict_ranked_compact) and hasattr(modules.UserModel, "forward_compact")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)          # noqa: E731
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.ensemble_rank_ragged([torch.zeros(5)], i32(3), i32(2), None, 4)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.compact_gather(torch.zeros(2, 3, 4), torch.zeros(2, 3, 3), i32(3), i32(2), 0, 5)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.attend_pool_ragged_fwd(torch.zeros(5, 8), torch.zeros(2, 3, 8), torch.zeros(8, 32), torch.zeros(8), torch.zeros(1, 8),
                                             torch.zeros(1), i32(5), i32(3), 3, 0)
    with FakeTensorMode():
        c = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")      # noqa: E731
        off, mult, imp = c(6, dtype=torch.int32), c(5, dtype=torch.int32), c(17, dtype=torch.int32)
        xt, xg = torch.ops.nrm.compact_gather(c(5, 7, 30, dtype=torch.float64), c(5, 7, 3, dtype=torch.float64), off, mult, 1, 17)
        assert (tuple(xt.shape), xt.dtype, tuple(xg.shape), xg.dtype) == ((17, 30), torch.float64, (17, 3), torch.float64)
        pooled, s = torch.ops.nrm.attend_pool_ragged_fwd(c(17, 16), c(5, 9, 16), c(16, 64), c(16), c(1, 16), c(1), imp, off, 6, 0)
        assert (tuple(pooled.shape), tuple(s.shape), pooled.dtype, s.dtype) == ((17, 16), (17, 9), torch.float32, torch.float32)
        for label, rows in ((None, 0), (c(5, 6), 5)):
            score, rank, live, metrics = torch.ops.nrm.ensemble_rank_ragged([c(17), c(17)], off, mult, label, 6)
            assert (tuple(score.shape), score.dtype) == ((5, 6), torch.float32)
            assert (tuple(rank.shape), rank.dtype) == ((5, 6), torch.int32)
            assert (tuple(live.shape), live.dtype) == ((5,), torch.int32)
            assert (tuple(metrics.shape), metrics.dtype) == ((rows, 3), torch.float32)


def test_forward_compact_is_inference_only():
    from news_recommendation_model_amd import modules
    m = modules.UserModel(3).train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_compact(torch.zeros(1, 2, 3), torch.zeros(2, 3), torch.zeros(2, 3), compact.build_plan([0], 2))
