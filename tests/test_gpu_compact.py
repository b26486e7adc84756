"""GPU: the compact scoring path -- gather + padding check, ragged attention + pool, UserModel.forward_compact,
the ragged scoring tail, evaluation.predict_ranked_compact and score_dataset(compact=True).

References and gates (none of them taken from the code under test):
  * ragged attention + pool: the float64 oracle per compact candidate through tests/attention_budget.py's pieces (one per impression),
    yardstick max(err(R32 against R64), 2^-23) and the dense kernels' own constant M_F32 -- the per-row arithmetic is theirs;
  * logits: the project's forward gate (<= 1e-3 of the largest entry against the fp32 oracle) and, per impression,
    err(compact, R64) <= M_LOGIT * max(err(dense, R64), 2^-23); M_LOGIT by the rule of DESIGN section 3b from the ratios recorded in
    profiles/compact_scoring.json;
  * scores of the ragged tail from fixed logits: the compact formula in float64 (compact.compact_scores_reference, itself pinned to the
    oracle's model_test on the CPU), rtol 1e-5 / atol 1e-7, the gate of tests/test_gpu_scoring.py;
  * predict_ranked_compact against predict_ranked: rtol = 1e-5 + expm1(2 expm1(2 d)) with d the largest logit difference between
    the two paths measured in the test (softmax turns an absolute logit difference d into a relative change <= expm1(2 d), twice);
  * ranks: exact against evaluation.rank_row on the path's own scores; against the dense path only on rows whose float64 scores keep
    a relative gap >= 2e-6 between neighbours, on models (out_mlp.fc2.weight x 100) for which that filter keeps >= 90 % of the rows."""
import json
import math
import os
import zipfile

import numpy as np
import pytest
import torch

import attention_budget as ab
from compact_util import pad_batch, percentile_counts
from news_recommendation_model_amd import compact

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-7
T_GRID = (1, 2, 5, 30, 100, 257, 1024)
# profiles/compact_scoring.json, "error_budget": the worst err(compact, R64) / max(err(dense, R64), 2^-23) of any impression in the
# recorded MI355X run of test_logits_against_dense_and_float64 below is 1.000 at all three sizes -- the compact logits came out
# bitwise equal to the dense ones (largest difference 0.0: the ragged kernels do the dense kernels' arithmetic per row, and every
# other op is row-wise).  M_LOGIT = the smallest power of two >= 4 x that ratio (the rule of DESIGN.md section 3b).
M_LOGIT = 4
_RECORD = os.environ.get("NRM_COMPACT_RECORD")          # a directory: every measured ratio is appended to <dir>/compact_ratios.jsonl


def _record(kind, **kw):
    if _RECORD:
        os.makedirs(_RECORD, exist_ok=True)
        with open(os.path.join(_RECORD, "compact_ratios.jsonl"), "a") as f:
            f.write(json.dumps(dict(kind=kind, **kw)) + "\n")


def _plan_of_counts(counts, T):
    """(cand_off, cand_imp, max_count) of lists with ``counts[b]`` candidates and no padded representative (pure ragged lists)."""
    counts = np.asarray(counts, dtype=np.int64)
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    imp = np.repeat(np.arange(len(counts)), counts)
    return off.astype(np.int32), imp.astype(np.int32), int(counts.max()) if len(counts) else 0


# ------------------------------------------------------------------------------------------------ ragged attention + pool
ATTN_CASES = {
    # name: (shape (B, T, H, D), counts per impression, environment)
    "streaming, compact candidate image (NT 10)": ((4, 12, 20, 160), [12, 0, 1, 7], {}),
    "streaming, per-row image (H < 16)": ((4, 9, 7, 160), [9, 1, 0, 5], {}),
    "streaming, two N-chunks of 13 tiles (D = 400)": ((3, 8, 18, 400), [8, 3, 1], {}),
    "streaming, D = 200 (not a multiple of 16)": ((3, 6, 17, 200), [5, 0, 6], {}),
    "fp32 walk, D = 64": ((5, 14, 40, 64), [14, 0, 1, 9, 3], {}),
    "fp32 walk, D = 64, tsplit 3": ((5, 14, 40, 64), [14, 0, 1, 9, 3], {"NRM_FWD_TSPLIT": "3"}),
    "fp32 walk, D = 128": ((3, 10, 24, 128), [10, 1, 4], {"NRM_FWD_WALK_F32": "1"}),
    "resident tiles, D = 128": ((3, 10, 24, 128), [10, 1, 4], {}),
    "resident tiles, D = 72 (not a multiple of 16)": ((3, 7, 9, 72), [2, 7, 0], {}),
    "degenerate plan N = B T, streaming": ((3, 5, 20, 160), [5, 5, 5], {}),
    "degenerate plan N = B T, walk": ((3, 5, 33, 64), [5, 5, 5], {}),
}


def _gate(name, got, r64, r32, what):
    e, y = ab._piece_err(name, got, r64), ab._piece_err(name, r32, r64)
    for norm, ev, yv in zip(("max", "l2"), e, y):
        ratio = ev / max(yv, ab.FLOOR)
        print(f"{what}: {name}/{norm} err {ev:.3e} yardstick {max(yv, ab.FLOOR):.3e} ratio {ratio:.2f} (M = {ab.M_F32})")
        _record("attention", case=what, piece=name, norm=norm, ratio=ratio)
        assert ratio <= ab.M_F32, (what, name, norm, ratio)


@pytest.mark.parametrize("what", sorted(ATTN_CASES))
def test_ragged_attention_and_pool_within_the_fp32_budget(lib, what, monkeypatch):
    from news_recommendation_model_amd import ops   # noqa: F401
    shape, counts, env = ATTN_CASES[what]
    B, T, H, D = shape
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = ab.get_case(shape, "normal", pool=True)
    case_s = ab.get_case(shape, "normal", pool=False)          # same seed, same (w, t, h): the scores' own references
    assert np.array_equal(case.t, case_s.t) and np.array_equal(case.h, case_s.h)
    off, imp, max_count = _plan_of_counts(counts, T)
    N = int(off[-1])
    t_c = np.concatenate([case.t[b, :counts[b]] for b in range(B)], axis=0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    w = [dev(case.w[k]) for k in ab.WKEYS]
    pooled, s = torch.ops.nrm.attend_pool_ragged_fwd(dev(t_c), dev(case.h), *w, dev(imp), dev(off), max_count, 0)
    torch.cuda.synchronize()
    assert tuple(pooled.shape) == (N, D) and tuple(s.shape) == (N, H)
    pooled, s = pooled.cpu().numpy(), s.cpu().numpy()
    rows = [b for b in range(B) if counts[b] > 0]
    regroup = lambda a: [a[off[b]:off[b + 1]] for b in rows]               # noqa: E731  (one piece per impression, as the dense gate)
    for name, got, c in (("s", s, case_s), ("pooled", pooled, case)):
        r64, r32 = c.reference(torch.float64)[name], c.reference(torch.float32)[name]
        _gate(name, regroup(got), [r64[b, :counts[b]] for b in rows], [r32[b, :counts[b]] for b in rows], what)
    if N == B * T:                                             # the dense entry point on the same data: the same gate, the same numbers
        p_d, s_d, _z = torch.ops.nrm.attend_pool_fwd(dev(case.t), dev(case.h), *w, False, 0)
        torch.cuda.synchronize()
        for name, dense, got, c in (("s", s_d, s, case_s), ("pooled", p_d, pooled, case)):
            dense = dense.cpu().numpy().reshape(got.shape)
            r64, r32 = c.reference(torch.float64)[name], c.reference(torch.float32)[name]
            _gate(name, [dense[off[b]:off[b + 1]] for b in rows], [r64[b] for b in rows], [r32[b] for b in rows], what + " (dense entry)")
            print(f"{what}: ragged against dense {name}: max |difference| {np.abs(dense - got).max():.3e}")


def test_ragged_attention_refuses_bf16(lib):
    from news_recommendation_model_amd import ops
    case = ab.get_case((2, 3, 5, 64), "normal", pool=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    off, imp, mc = _plan_of_counts([3, 2], 3)
    args = (dev(case.t.reshape(-1, 64)[:5]), dev(case.h), *[dev(case.w[k]) for k in ab.WKEYS], dev(imp), dev(off), mc)
    for mma in ("bf16", "bf16x3"):
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            ops.attend_pool_ragged(*args, mma=mma)
    assert tuple(ops.attend_pool_ragged(*args, mma="f32").shape) == (5, 64)


# ------------------------------------------------------------------------------------------------ models and batches
def _models(dims, user_num, seeds=(1, 5), scale_out=1.0):
    from news_recommendation_model_amd import synth, trainer
    sds = []
    for s in seeds:
        sd = synth.make_state_dict(dims, seed=s, user_num=user_num)
        if scale_out != 1.0:
            sd["out_mlp.fc2.weight"] = (sd["out_mlp.fc2.weight"] * scale_out).astype(sd["out_mlp.fc2.weight"].dtype)
        sds.append(sd)
    return [trainer.build_model(dims, user_num, sd, device="cuda").eval() for sd in sds], sds


def _padded_batch(dims, B, H, T, seed, trim=0, one_empty=False):
    from news_recommendation_model_amd import synth
    rng = np.random.default_rng(seed)
    counts = np.minimum(percentile_counts(rng, B, T, one_long=False), T - trim)
    counts[0] = T - trim
    if B > 2:
        counts[1] = 1
    if one_empty and B > 3:
        counts[2] = 0
    batch = pad_batch(synth.make_batch(dims, B, H, T, seed=seed, user_num=50), counts)
    return batch, counts


def _device_batch(batch, host_empty=True):
    tb = {k: torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in ("x_history", "x_target", "x_global", "label")}
    tb["empty_num"] = torch.from_numpy(batch["empty_num"]) if host_empty else torch.from_numpy(batch["empty_num"]).cuda()
    return tb


def _compact_logits(models, tb, plan):
    from news_recommendation_model_amd import ops
    tabs = plan.upload("cuda")
    xt_c, xg_c = ops.compact_gather(tb["x_target"], tb["x_global"], tabs["cand_off"], tabs["pad_mult"], plan.trim, plan.N)
    return [m.forward_compact(tb["x_history"], xt_c, xg_c, plan) for m in models], xt_c, xg_c


def _delta_max(models, tb, plan):
    """The largest logit difference between forward_compact and the dense eval forward over the plan's cells."""
    lcs, _, _ = _compact_logits(models, tb, plan)
    cells = torch.from_numpy(plan.cand_imp.astype(np.int64) * plan.Tp + (plan.src - plan.cand_imp.astype(np.int64) * plan.T)).cuda()
    delta = 0.0
    with torch.no_grad():
        for m, lc in zip(models, lcs):
            ld = m(tb["x_history"], tb["x_target"][:, :plan.Tp], tb["x_global"][:, :plan.Tp]).reshape(-1)
            delta = max(delta, float((lc - ld[cells]).abs().max()))
    return delta


def test_gather_copies_the_plan_rows_bitwise(lib):
    from news_recommendation_model_amd import ops
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(16, category_label_num=20)
    for dtype in (np.float64, np.float32):
        batch, _ = _padded_batch(dims, 9, 4, 11, seed=3, trim=2, one_empty=True)
        batch["x_target"], batch["x_global"] = batch["x_target"].astype(dtype), batch["x_global"].astype(dtype)
        plan = compact.build_plan(batch["empty_num"], 11)
        assert plan.trim == 2 and 0 < plan.N < 9 * 9
        tb = _device_batch(batch)
        tabs = plan.upload("cuda")
        xt_c, xg_c = ops.compact_gather(tb["x_target"], tb["x_global"], tabs["cand_off"], tabs["pad_mult"], plan.trim, plan.N)
        ops.check_pad_errors("cuda")                            # a clean batch: silent
        assert xt_c.dtype == tb["x_target"].dtype and xg_c.dtype == tb["x_global"].dtype
        assert np.array_equal(xt_c.cpu().numpy(), batch["x_target"].reshape(9 * 11, -1)[plan.src])
        assert np.array_equal(xg_c.cpu().numpy(), batch["x_global"].reshape(9 * 11, -1)[plan.src])


# ------------------------------------------------------------------------------------------------ logits
LOGIT_CASES = {
    "tiny": dict(emb=16, B=9, H=6, T=12, trim=1),
    "reference default (emb 64, H = 200)": dict(emb=64, B=8, H=200, T=24, trim=0),
    "C3 (emb 400, H = 50)": dict(emb=400, B=6, H=50, T=16, trim=2),
}


@pytest.mark.parametrize("what", sorted(LOGIT_CASES))
def test_logits_against_dense_and_float64(lib, what):
    from news_recommendation_model_amd.config import Dims
    from oracle import user_model_oracle as orc
    c = LOGIT_CASES[what]
    dims = Dims.for_emb(c["emb"], category_label_num=50)
    B, H, T = c["B"], c["H"], c["T"]
    batch, counts = _padded_batch(dims, B, H, T, seed=7, trim=c["trim"])
    models, sds = _models(dims, 50, seeds=(1,))
    plan = compact.build_plan(batch["empty_num"], T)
    assert plan.trim == c["trim"] and plan.N < B * plan.Tp
    tb = _device_batch(batch)
    (lc,), _, _ = _compact_logits(models, tb, plan)
    with torch.no_grad():
        ld = models[0](tb["x_history"], tb["x_target"][:, :plan.Tp], tb["x_global"][:, :plan.Tp])
    torch.cuda.synchronize()
    lc, ld = lc.cpu().numpy().astype(np.float64), ld.cpu().numpy().astype(np.float64).reshape(-1)
    cells = (plan.cand_imp.astype(np.int64) * plan.Tp + (plan.src - plan.cand_imp.astype(np.int64) * T))     # (b, t) in the trimmed [B, T'] layout
    cpu = {k: torch.from_numpy(batch[k][:, :plan.Tp] if k != "x_history" else batch[k]) for k in ("x_history", "x_target", "x_global")}
    with torch.no_grad():
        r32 = orc.user_model_forward(orc.to_torch_params(sds[0], requires_grad=False), cpu["x_history"], cpu["x_target"], cpu["x_global"],
                                     training=False).numpy().astype(np.float64).reshape(-1)
        with orc.precision(torch.float64):
            r64 = orc.user_model_forward(orc.to_torch_params(sds[0], requires_grad=False, dtype=torch.float64), cpu["x_history"],
                                         cpu["x_target"], cpu["x_global"], training=False).numpy().reshape(-1)
    # the standing forward gate, against the fp32 oracle
    fwd = np.abs(lc - r32[cells]).max() / np.abs(r32).max()
    print(f"{what}: forward gate {fwd:.3e} (<= 1e-3), N = {plan.N} of {B * plan.Tp} cells")
    assert fwd <= 1e-3
    worst, delta = 0.0, float(np.abs(lc - ld[cells]).max())
    for b in range(B):
        sl = slice(int(plan.cand_off[b]), int(plan.cand_off[b + 1]))
        ref = r64[cells[sl]]
        den = np.abs(r64[b * plan.Tp:(b + 1) * plan.Tp]).max()
        e_c = np.abs(lc[sl] - ref).max() / den
        e_d = np.abs(ld[cells[sl]] - ref).max() / den
        worst = max(worst, e_c / max(e_d, ab.FLOOR))
    print(f"{what}: worst per-impression err(compact, R64) / max(err(dense, R64), 2^-23) = {worst:.3f} (M_LOGIT = {M_LOGIT}); "
          f"largest logit difference compact - dense {delta:.3e}")
    _record("logit", case=what, ratio=worst, delta=delta, N=plan.N, cells=B * plan.Tp)
    assert worst <= M_LOGIT


def test_forward_compact_refuses_a_bf16_model(lib):
    from news_recommendation_model_amd import evaluation, synth, trainer
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    batch, _ = _padded_batch(dims, 5, 8, 9, seed=2)
    tb = _device_batch(batch)
    for mma in ("bf16", "bf16x3"):
        model = trainer.build_model(dims, 50, synth.make_state_dict(dims, seed=1, user_num=50), device="cuda", attention_mma=mma).eval()
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            evaluation.predict_ranked_compact([model], tb)
        assert len(evaluation.predict_ranked([model], tb)) == 3          # the dense path takes it


# ------------------------------------------------------------------------------------------------ ragged tail alone
def _tail_inputs(T, M, B=11, seed=0):
    g = np.random.default_rng(1000 * T + 10 * M + seed)
    live = g.integers(1, T + 1, B)
    live[0] = T                                               # pad_mult 0
    if T > 1:
        live[1] = T - 1                                       # pad_mult 1
        live[2] = 1                                           # pad_mult T - 1 (large)
    live[3] = 0 if T > 1 else T                               # no live candidate: all zeros
    plan = compact.build_plan(T - live, T)
    assert plan.trim == 0 and plan.live.tolist() == live.tolist()
    logits = [np.clip(4 * g.standard_normal(plan.N), -10, 10).astype(np.float32) for _ in range(M)]
    return plan, logits


def _run_tail(plan, logits, label=None):
    tabs = plan.upload("cuda")
    out = torch.ops.nrm.ensemble_rank_ragged([torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x for x in logits], tabs["cand_off"],
                                             tabs["pad_mult"], label.cuda() if label is not None else None, plan.Tp)
    torch.cuda.synchronize()
    return out


def _check_tail(plan, logits, score, rank, live, what):
    from news_recommendation_model_amd import evaluation
    ref = compact.compact_scores_reference([np.asarray(x, dtype=np.float64) for x in logits], plan)
    got = score.cpu().numpy().astype(np.float64)
    assert live.dtype == torch.int32 and live.cpu().tolist() == plan.live.tolist(), what
    mask = np.arange(plan.Tp)[None, :] < plan.live[:, None]
    worst = float((np.abs(got - ref)[mask] / (ATOL + RTOL * np.abs(ref[mask]))).max()) if mask.any() else 0.0
    print(f"{what}: worst |err| / (atol + rtol |ref|) = {worst:.4f}")
    assert worst <= 1.0, (what, worst)
    assert (got[~mask] == 0).all(), what
    s, r = score.cpu(), rank.cpu()
    assert r.dtype == torch.int32
    for b in range(plan.B):
        n = int(plan.live[b])
        assert r[b, :n].tolist() == evaluation.rank_row(s[b, :n].tolist()), (what, b)
        assert bool((r[b, n:] == 0).all()), (what, b)


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("T", T_GRID)
def test_ragged_tail_scores_and_ranks_on_the_grid(lib, T, M):
    plan, logits = _tail_inputs(T, M)
    score, rank, live, metrics = _run_tail(plan, logits)
    assert tuple(metrics.shape) == (0, 3) and tuple(score.shape) == (plan.B, T)
    _check_tail(plan, logits, score, rank, live, f"T={T} M={M}")
    if T > 1:
        assert bool((score[3] == 0).all()) and bool((rank[3] == 0).all())
    # the logits where the models leave them: column 0 of a padded [N, 4] GEMM output (stride 4), nothing is copied
    padded = [torch.full((plan.N, 4), -77.0).cuda() for _ in logits]
    for p, x in zip(padded, logits):
        p[:, 0] = torch.from_numpy(x).cuda()
    strided = _run_tail(plan, [p[:, 0] for p in padded])
    assert torch.equal(strided[0], score) and torch.equal(strided[1], rank)


@pytest.mark.parametrize("T", [30, 100])
def test_ragged_tail_ties_break_by_index_and_metrics(lib, T):
    from test_gpu_scoring import _ref_metrics
    plan, logits = _tail_inputs(T, 3, seed=2)
    rows = [b for b in range(plan.B) if plan.live[b] >= 8]
    assert rows
    for x in logits:
        for b in rows:
            c0 = int(plan.cand_off[b])
            x[c0 + 7] = x[c0 + 2]                             # two live candidates with equal logits in every model
    label = torch.zeros(plan.B, T)
    for b in range(plan.B):
        if plan.live[b]:
            label[b, b % int(plan.live[b])] = 1
    score, rank, live, metrics = _run_tail(plan, logits, label)
    s, r = score.cpu(), rank.cpu()
    assert torch.equal(s[rows, 2].view(torch.int32), s[rows, 7].view(torch.int32))      # bitwise equal scores ...
    assert bool((r[rows, 7] == r[rows, 2] + 1).all())                                   # ... the lower index ranks first
    _check_tail(plan, logits, score, rank, live, f"T={T} ties")
    want = _ref_metrics(r.numpy(), label.numpy(), live.cpu().numpy())
    assert np.abs(metrics.cpu().numpy().astype(np.float64) - want).max() < 1e-6
    assert (want[3] == -1).all()


@pytest.mark.parametrize("T", [30, 100])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_ragged_tail_keeps_a_non_finite_logit_in_its_row(lib, T, poison):
    plan, logits = _tail_inputs(T, 2, seed=4)
    label = torch.zeros(plan.B, T)
    label[:, 0] = 1
    clean = [t.clone() for t in _run_tail(plan, logits, label)]
    bad = [x.copy() for x in logits]
    bad[1][int(plan.cand_off[5])] = poison
    dirty = _run_tail(plan, bad, label)
    others = [b for b in range(plan.B) if b != 5]
    for name, a, c in zip(("score", "rank", "live", "metrics"), dirty, clean):
        assert torch.equal(a[others].view(torch.int32), c[others].view(torch.int32)), name


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("host_empty", [True, False])
def test_predict_ranked_compact_against_predict_ranked(lib, host_empty):
    from news_recommendation_model_amd import evaluation, ops
    from news_recommendation_model_amd.config import Dims
    from test_gpu_scoring import _ref_metrics
    dims = Dims.for_emb(64, category_label_num=50)
    B, H, T = 40, 24, 40
    batch, counts = _padded_batch(dims, B, H, T, seed=13, trim=3, one_empty=True)
    models, _ = _models(dims, 50)
    tb = _device_batch(batch, host_empty)
    plan = compact.build_plan(batch["empty_num"], T)
    s_d, r_d, live_d, m_d = evaluation.predict_ranked(models, tb, with_metrics=True)
    s_c, r_c, live_c, m_c = evaluation.predict_ranked_compact(models, tb, with_metrics=True)
    ops.check_pad_errors("cuda")
    ops.check_index_errors("cuda")
    assert s_c.shape == s_d.shape == (B, T - 3) and torch.equal(live_c, live_d) and live_c.dtype == torch.int32
    # the largest logit difference between the two paths, measured here, fixes the gate
    delta = _delta_max(models, tb, plan)
    rtol = 1e-5 + math.expm1(2 * math.expm1(2 * delta))
    got, ref = s_c.cpu().double(), s_d.cpu().double()
    mask = torch.arange(T - 3)[None, :] < live_d.cpu()[:, None]
    worst = float(((got - ref).abs()[mask] / (ATOL + rtol * ref[mask].abs())).max())
    print(f"predict_ranked_compact against predict_ranked: delta_max {delta:.3e}, rtol {rtol:.3e}, worst |err| / (atol + rtol |ref|) = {worst:.4f}; "
          f"N = {plan.N} of {B * plan.Tp} cells")
    _record("end_to_end", delta=delta, rtol=rtol, worst=worst)
    assert worst <= 1.0
    assert bool((got[~mask] == 0).all()) and bool((s_c[2] == 0).all()) and bool((r_c[2] == 0).all())
    for b in range(B):                                        # ranks: exact on the compact path's OWN scores
        n = int(live_c[b])
        assert r_c[b, :n].tolist() == evaluation.rank_row(s_c[b, :n].tolist()), b
        assert bool((r_c[b, n:] == 0).all())
    want = _ref_metrics(r_c.cpu().numpy(), batch["label"][:, :T - 3], live_c.cpu().numpy())
    assert np.abs(m_c.cpu().numpy().astype(np.float64) - want).max() < 1e-6
    three = evaluation.predict_ranked_compact(models, tb)
    assert len(three) == 3 and torch.equal(three[0], s_c) and torch.equal(three[1], r_c)


def test_unpadded_batch_takes_the_dense_path_and_forced_compact_agrees(lib):
    from news_recommendation_model_amd import evaluation, synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    batch = synth.make_batch(dims, 7, 20, 9, seed=4, user_num=50, pad_target=2)      # every row padded alike: nothing left after the trim
    models, _ = _models(dims, 50)
    tb = _device_batch(batch)
    dense = evaluation.predict_ranked(models, tb)
    same = evaluation.predict_ranked_compact(models, tb)
    assert all(torch.equal(a, b) for a, b in zip(dense, same))               # handed to predict_ranked itself: bitwise
    forced = evaluation.predict_ranked_compact(models, tb, force_compact=True)
    plan = compact.build_plan(batch["empty_num"], 9)
    assert plan.dense and plan.trim == 2
    rtol = 1e-5 + math.expm1(2 * math.expm1(2 * _delta_max(models, tb, plan)))       # the gate of the end-to-end test above
    assert torch.equal(forced[2], dense[2]) and torch.allclose(forced[0], dense[0], rtol=rtol, atol=ATOL)


def test_ranks_agree_with_the_dense_path_where_the_reference_separates_the_scores(lib):
    from news_recommendation_model_amd import evaluation
    from news_recommendation_model_amd.config import Dims
    from oracle import user_model_oracle as orc
    dims = Dims.for_emb(64, category_label_num=50)
    B, H, T = 80, 24, 40
    batch, counts = _padded_batch(dims, B, H, T, seed=21, trim=3)
    models, sds = _models(dims, 50, scale_out=100.0)
    tb = _device_batch(batch)
    _s_d, r_d, live_d = evaluation.predict_ranked(models, tb)
    _s_c, r_c, live_c = evaluation.predict_ranked_compact(models, tb)
    cpu = {k: torch.from_numpy(batch[k]) for k in ("x_history", "x_target", "x_global", "empty_num")}
    with orc.precision(torch.float64):
        ref = orc.model_test_scores([orc.to_torch_params(sd, requires_grad=False, dtype=torch.float64) for sd in sds], cpu)
    keep = []
    for b in range(B):
        v = np.sort(ref[b])[::-1]
        gap = np.min((v[:-1] - v[1:]) / np.abs(v[:-1])) if len(v) > 1 else 1.0
        if gap >= 2e-6:
            keep.append(b)
    dropped = B - len(keep)
    print(f"rank comparison: {dropped} of {B} rows have a float64 gap below 2e-6 and are left out")
    assert dropped <= B // 10
    differ = [b for b in keep if r_c[b].tolist() != r_d[b].tolist()]
    assert not differ, differ
    assert torch.equal(live_c, live_d)


def test_non_finite_inputs_stay_in_their_impression(lib):
    from news_recommendation_model_amd import evaluation
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    B, H, T = 12, 20, 18
    batch, counts = _padded_batch(dims, B, H, T, seed=5)
    models, _ = _models(dims, 50)
    clean = [t.clone() for t in evaluation.predict_ranked_compact(models, _device_batch(batch), with_metrics=True)]
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean)
    for where in ("x_target", "x_history"):
        for poison in (float("nan"), float("inf")):
            bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
            bad[where][4, 0, 5] = poison                       # a text / image column of impression 4
            dirty = evaluation.predict_ranked_compact(models, _device_batch(bad), with_metrics=True)
            torch.cuda.synchronize()
            others = [b for b in range(B) if b != 4]
            for name, a, c in zip(("score", "rank", "live", "metrics"), dirty, clean):
                assert torch.equal(a[others].view(torch.int32), c[others].view(torch.int32)), (where, poison, name)
            assert not bool(torch.isfinite(dirty[0][4, :int(counts[4])]).all()), (where, poison)


def test_pad_check_and_index_flag(lib):
    from news_recommendation_model_amd import evaluation, ops
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    B, H, T = 10, 12, 15
    batch, counts = _padded_batch(dims, B, H, T, seed=9)
    models, _ = _models(dims, 50)
    evaluation.predict_ranked_compact(models, _device_batch(batch))
    ops.check_pad_errors("cuda")                                # clean: silent
    b = int(np.argmax((T - counts) >= 3))
    assert T - counts[b] >= 3
    for field, col in (("x_target", 6), ("x_global", 1)):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
        bad[field][b, T - 1, col] = 0.25                        # the LAST padded row of one impression is not like the others
        evaluation.predict_ranked_compact(models, _device_batch(bad))
        with pytest.raises(ValueError, match="padded candidate row differs"):
            ops.check_pad_errors("cuda")
        ops.check_pad_errors("cuda")                            # the flag was cleared
    # a difference in a TRIMMED column is never read, as the reference never reads it
    trimmed, _ = _padded_batch(dims, B, H, T, seed=9, trim=2)
    trimmed["x_target"][3, T - 1, 6] = 0.25
    evaluation.predict_ranked_compact(models, _device_batch(trimmed))
    ops.check_pad_errors("cuda")
    # an out-of-range category id in a live row still raises through the index flag
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    bad["x_target"][0, 0, 4 + dims.pca_vector] = 10 ** 6
    evaluation.predict_ranked_compact(models, _device_batch(bad))
    with pytest.raises(IndexError):
        ops.check_index_errors("cuda")


def test_score_dataset_compact_end_to_end(lib, tmp_path):
    from news_recommendation_model_amd import data_io, evaluation, synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    models, _ = _models(dims, 50)
    B, T = 13, 6
    b = synth.make_batch(dims, B, 5, T, seed=11, user_num=50)
    pad_batch(b, T - np.array([1, 3, 2, 1, 4, 0, 2, 1, 3, 0, 2, 2, 5]))
    b["impression_id"] = np.array([900 + 7 * i for i in range(B)])
    head = data_io.write_processed_dataset(data_io.records_from_batch(b), str(tmp_path / "test_set"), subvolume_item_num=6)
    out_dir = str(tmp_path / "out")
    zpath = evaluation.score_dataset(models, head, out_dir, batch_size=5, compact=True)
    lines = open(os.path.join(out_dir, "predictions.txt"), encoding="utf-8").read().splitlines(keepends=True)
    assert len(lines) == B
    loaded, _ = data_io.load_processed_dataset(head)
    want_lines = []
    for lo in range(0, B, 5):                                  # batches of 5, 5, 3: the second straddles subvolumes, the last is short
        cb = data_io.collate(loaded[lo:lo + 5])
        tb = {k: torch.from_numpy(cb[k]).cuda() for k in ("x_history", "x_target", "x_global")}
        tb["empty_num"] = torch.from_numpy(cb["empty_num"])
        s_c, rank, live = evaluation.predict_ranked_compact(models, tb)
        for i in range(s_c.shape[0]):
            n = int(live[i])
            assert n == T - int(cb["empty_num"][i])
            ranks = evaluation.rank_row(s_c[i, :n].tolist())
            assert rank[i, :n].tolist() == ranks
            want_lines.append("{} [{}]\n".format(int(cb["impression_id"][i]), ",".join(str(r) for r in ranks)))
    assert lines == want_lines
    for i, line in enumerate(lines):
        head_id, body = line.split(" ")
        assert int(head_id) == 900 + 7 * i
        assert len(body.strip()[1:-1].split(",")) == T - int(b["empty_num"][i])
    with zipfile.ZipFile(zpath) as z:
        assert z.namelist() == ["predictions.txt"] and z.read("predictions.txt").decode("utf-8") == "".join(lines)
    # a data set whose padded rows are not all alike is refused after the last batch
    b["x_global"][1, T - 2, 0] = 0.5                          # (column T - 1 is trimmed in its batch, T - 2 is kept)
    head2 = data_io.write_processed_dataset(data_io.records_from_batch(b), str(tmp_path / "bad_set"), subvolume_item_num=6)
    with pytest.raises(ValueError, match="padded candidate row differs"):
        evaluation.score_dataset(models, head2, str(tmp_path / "out2"), batch_size=5, compact=True)


def test_opcheck_compact_ops(lib):
    from news_recommendation_model_amd import ops   # noqa: F401
    plan, logits = _tail_inputs(30, 2)
    tabs = plan.upload("cuda")
    xs = [torch.from_numpy(x).cuda() for x in logits]
    label = torch.zeros(plan.B, 30, device="cuda")
    label[:, 1] = 1
    torch.library.opcheck(torch.ops.nrm.ensemble_rank_ragged.default, (xs, tabs["cand_off"], tabs["pad_mult"], None, 30))
    torch.library.opcheck(torch.ops.nrm.ensemble_rank_ragged.default, (xs[:1], tabs["cand_off"], tabs["pad_mult"], label, 30))
    xt = torch.randn(plan.B, 30, 9, device="cuda", dtype=torch.float64)
    xg = torch.randn(plan.B, 30, 3, device="cuda", dtype=torch.float64)
    torch.library.opcheck(torch.ops.nrm.compact_gather.default, (xt, xg, tabs["cand_off"], tabs["pad_mult"], 0, plan.N))
    ops.pad_error_flag("cuda").zero_()                          # (random rows are not padding: the flag is expected here)
    case = ab.get_case((2, 3, 5, 16), "normal", pool=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    off, imp, mc = _plan_of_counts([3, 2], 3)
    torch.library.opcheck(torch.ops.nrm.attend_pool_ragged_fwd.default,
                          (dev(case.t.reshape(-1, 16)[:5]), dev(case.h), *[dev(case.w[k]) for k in ab.WKEYS], dev(imp), dev(off), mc, 0))
