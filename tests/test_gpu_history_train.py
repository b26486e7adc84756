"""GPU: training on compacted histories -- the grouped gather against numpy (bitwise), the pool kernels with a
weighted last row against float64 (yardstick: today's unweighted kernel on the EXPANDED input, the last row repeated w times), the grouped
attention + pool node in the attention error budget (tests/attention_budget.py) against the float64 oracle on the dense input, the whole
training step through trainer.train_step(compact_history=True) against the float64 oracle step with the dense HIP step as the
yardstick, three lock-step optimizer steps, the dense plan (bitwise the dense step) and the refusals.

Set NRM_HISTORY_TRAIN_RECORD=<path> to write every measured ratio to a JSON file (profiles/history_train.json is such a record)."""
import json
import os

import numpy as np
import pytest
import torch

import attention_budget as ab
from golden_util import II_B, II_W, ZERO_GRAD_KEYS, grad_tolerance, oracle_step_with_bounds, rel_err
from history_train_util import H_ID, L_LIST, padded_batch

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
M_POOL = 4             # two bits: one product by w in place of w equal addends (fixed by reasoning, not measured)
# profiles/history_train.json (one MI355X run of this file): the worst err(compact step) / max(err(dense HIP step), 2^-23) of any tensor
# but the two below is 6.39 (label_attention.mlp.fc2.bias, third lock-step step; 1.54 over the single steps); M_TRAIN_HIST is the smallest power of two
# >= 4 x that figure (the rule of DESIGN.md section 3b).
M_TRAIN_HIST = 32
# The two instant-interest gradients are sums that cancel (golden_util.instant_interest_grad_bounds): their fp32 error is
# noise of a few 1e-7 .. 1e-6 of the term-magnitude sum S, a relative error anywhere up to ~1e-5, in the dense HIP step and in the compact
# one alike -- and the compact step sums the B*T rows in another (sorted) order.  Their ratio is noise over noise, so they get a constant
# of their own by the same rule, as d_fc2.bias does in section 3b: recorded worst 17.9 (second lock-step step; 1.07 over the single steps).
M_TRAIN_HIST_II = 128


def _m_step(key):
    return M_TRAIN_HIST_II if key in (II_W, II_B) else M_TRAIN_HIST
FWD_TOL, GRAD_TOL = 1e-3, 1e-2
_record = {"pool": {}, "node": {}, "step": {}}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("NRM_HISTORY_TRAIN_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({"M_POOL": M_POOL, "M_TRAIN_HIST": M_TRAIN_HIST, "M_TRAIN_HIST_II": M_TRAIN_HIST_II, "M_F32": ab.M_F32, "M_BF16X3": ab.M_BF16X3, "M_FC2_BIAS": ab.M_FC2_BIAS,
                       **{k: {kk: v[kk] for kk in sorted(v)} for k, v in _record.items()}}, f, indent=1)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cols", [80, 7])
def test_grouped_gather_is_bitwise(lib, dtype, cols):
    from news_recommendation_model_amd import compact, ops
    B, H = 9, H_ID
    rng = np.random.default_rng(cols)
    x = rng.standard_normal((B, H, cols)).astype(dtype)
    x[0, 3, 0] = -0.0
    x[1, 0, 1] = np.nan
    plan = compact.plan_history_groups(L_LIST, H, max_groups=3, quantum=1)
    assert plan.G == 3 and plan.perm.tolist() != list(range(B)) and 1 not in np.diff(plan.bounds).tolist()
    one = compact.plan_history_groups([0, 30, 31, 32, 33, 34, 35, 36, 37], H, max_groups=3, quantum=1)      # a group of one impression
    assert 1 in np.diff(one.bounds).tolist()
    shuffled = compact.plan_history_groups(L_LIST, H, max_groups=3, quantum=1)
    shuffled.perm = shuffled.perm[::-1].copy()                                                               # any permutation is copied as told
    for p in (plan, one, shuffled):
        p.device_tables = None
        tabs = p.upload("cuda")
        got = ops.history_gather_groups(_dev(x), tabs["perm"], tabs["bounds"], tabs["row_off"], tabs["H_g"], p.R).cpu().numpy()
        want = np.concatenate([x[p.perm[b], :p.H_g[g]] for g in range(p.G) for b in range(p.bounds[g], p.bounds[g + 1])])
        assert got.dtype == dtype and got.shape == (p.R, cols)
        assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ weighted pool kernels
def _call(name, *args):
    from news_recommendation_model_amd import native
    native.call(name, *args, native.stream_ptr())


def _p(t):
    from news_recommendation_model_amd import native
    return native.ptr(t)


def _bmm(W, wsb, wsi, wsj, X, out, B, I, J, D, accumulate, w=None, row=0):
    if w is None:
        _call("nrm_pool_bmm", _p(W), wsb, wsi, wsj, _p(X), D, _p(out), B, I, J, D, accumulate)
    else:
        _call("nrm_pool_bmm_wlast", _p(W), wsb, wsi, wsj, _p(X), D, _p(out), B, I, J, D, accumulate, float(w), row)
    return out


def _rowdot(g, h, B, T, H, D, w=None):
    ds = torch.empty(B, T, H, dtype=torch.float32, device="cuda")
    if w is None:
        _call("nrm_pool_rowdot", _p(g), D, _p(h), _p(ds), B, T, H, D, None, 0)
    else:
        _call("nrm_pool_rowdot_wlast", _p(g), D, _p(h), _p(ds), B, T, H, D, None, 0, float(w))
    return ds


def _expand(a, axis, w):
    """The last entry along ``axis`` repeated w times (w = 1: unchanged)."""
    last = np.take(a, [a.shape[axis] - 1], axis=axis)
    return np.concatenate([a] + [last] * (w - 1), axis=axis)


def _gate(what, key, got, yard, truth):
    e, y = rel_err(got, truth), max(rel_err(yard, truth), FLOOR)
    _record["pool"][f"{what}|{key}"] = e / y
    assert e <= M_POOL * y, (what, key, e, y, e / y)


POOL_SHAPES = [(B, T, J) for J in (1, 2, 16, 17, 37) for T in (1, 3) for B in (1, 5)]


@pytest.mark.parametrize("jsplit", [None, "1"])
@pytest.mark.parametrize("w", [1, 2, 37])
@pytest.mark.parametrize("D", [64, 72])
def test_weighted_pool_kernels_against_float64(lib, monkeypatch, D, w, jsplit):
    """The three placements of w.  B <= 5 impressions are a handful of tasks, so from J = 32 the pool runs its JSPLIT form by itself;
    NRM_POOL_JSPLIT=1 forces it at every J (and on the history gradient, whose reduction index is the T candidates)."""
    if jsplit is None:
        monkeypatch.delenv("NRM_POOL_JSPLIT", raising=False)
    else:
        monkeypatch.setenv("NRM_POOL_JSPLIT", jsplit)
    for B, T, J in POOL_SHAPES:
        rng = np.random.default_rng(1000 * D + 100 * w + 10 * J + T + B)
        s, h, g, pre = (rng.standard_normal(sh).astype(np.float32) for sh in ((B, T, J), (B, J, D), (B, T, D), (B, J, D)))
        s64, h64, g64 = s.astype(np.float64), h.astype(np.float64), g.astype(np.float64)
        wj = np.ones(J)
        wj[-1] = w
        key = f"B{B} T{T} J{J} D{D} w{w} jsplit {jsplit}"
        Je = J + w - 1
        s_e, h_e = _expand(s, 2, w), _expand(h, 1, w)
        new = lambda *sh: torch.empty(*sh, dtype=torch.float32, device="cuda")          # noqa: E731
        # forward: pooled = sum_j w_j s[., j] h[j, :], weighted where s is READ
        sd = _dev(s)
        got = _bmm(sd, T * J, J, 1, _dev(h), new(B, T, D), B, T, J, D, 0, w, 0)
        yard = _bmm(_dev(s_e), T * Je, Je, 1, _dev(h_e), new(B, T, D), B, T, Je, D, 0)
        _gate("forward", key, got.cpu().numpy(), yard.cpu().numpy(), np.einsum("btj,j,bjd->btd", s64, wj, h64))
        assert torch.equal(sd.cpu(), torch.from_numpy(s))                               # s itself stays unweighted
        # score gradient: ds[., J - 1] = w g . h[J - 1]
        got = _rowdot(_dev(g), _dev(h), B, T, J, D, w).cpu().numpy()
        yard = _rowdot(_dev(g), _dev(h_e), B, T, Je, D).cpu().numpy().astype(np.float64)
        yard = np.concatenate([yard[..., :J - 1], yard[..., J - 1:].sum(-1, keepdims=True)], axis=-1)
        _gate("score gradient", key, got, yard, np.einsum("btd,bjd,j->btj", g64, h64, wj))
        # history gradient, accumulated onto a non-zero dh: only the added term of row J - 1 carries w
        got = _bmm(sd, T * J, 1, J, _dev(g), _dev(pre), B, J, T, D, 1, w, 1).cpu().numpy()
        pre_e = np.concatenate([pre, np.zeros((B, w - 1, D), dtype=np.float32)], axis=1)
        yard = _bmm(_dev(s_e), T * Je, 1, Je, _dev(g), _dev(pre_e), B, Je, T, D, 1).cpu().numpy().astype(np.float64)
        yard = np.concatenate([yard[:, :J - 1], yard[:, J - 1:].sum(1, keepdims=True)], axis=1)
        _gate("history gradient", key, got, yard, pre.astype(np.float64) + np.einsum("btj,j,btd->bjd", s64, wj, g64))
        if w == 1:                                                                      # bitwise today's kernels
            assert torch.equal(_bmm(sd, T * J, J, 1, _dev(h), new(B, T, D), B, T, J, D, 0, 1, 0), _bmm(sd, T * J, J, 1, _dev(h), new(B, T, D), B, T, J, D, 0))
            assert torch.equal(_rowdot(_dev(g), _dev(h), B, T, J, D, 1), _rowdot(_dev(g), _dev(h), B, T, J, D))
            assert torch.equal(_bmm(sd, T * J, 1, J, _dev(g), _dev(pre), B, J, T, D, 1, 1, 1), _bmm(sd, T * J, 1, J, _dev(g), _dev(pre), B, J, T, D, 1))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the grouped node
NODE_SHAPES = {(7, 3, 37, 64): L_LIST[:7], (7, 3, 37, 72): L_LIST[:7], (4, 2, 20, 400): [3, 20, 5, 9]}
_node_cases = {}


def _node_case(shape):
    """Dense inputs whose history rows j >= L_b all equal ONE non-zero row of their impression (with zero rows a missing multiplicity
    would pool nothing and go unseen), as a budget case: float64 and fp32 oracle on the DENSE input, computed once per shape."""
    if shape not in _node_cases:
        B, T, H, D = shape
        w, t, h, g = ab.make_inputs(B, T, H, D, pool=True)
        for b, L in enumerate(NODE_SHAPES[shape]):
            if L < H:
                h[b, L:] = h[b, L]
        _node_cases[shape] = ab.Case(w, t, h, g, pool=True, tag={"shape": list(shape), "family": "equal padded rows"})
    return _node_cases[shape]


def _reduce_dh(dh, plan):
    """Dense d_history [B, H, D] (caller's order) -> per impression [H_g, D] with the last row the SUM of the dense rows it stands for."""
    out = [None] * plan.B
    for g in range(plan.G):
        H_g = int(plan.H_g[g])
        for b in plan.perm[plan.bounds[g]:plan.bounds[g + 1]]:
            out[b] = np.concatenate([dh[b, :H_g - 1], dh[b, H_g - 1:].sum(0, keepdims=True)])
    return out


def _run_grouped(case, plan, mma, rowgrads):
    from news_recommendation_model_amd import ops
    perm = torch.from_numpy(plan.perm.astype(np.int64))
    arena = np.concatenate([case.h[plan.perm[b], :plan.H_g[g]] for g in range(plan.G) for b in range(plan.bounds[g], plan.bounds[g + 1])])
    wg = {k: _dev(v).requires_grad_(True) for k, v in case.w.items()}
    t = _dev(case.t[plan.perm]).requires_grad_(rowgrads)
    h = _dev(arena).requires_grad_(rowgrads)
    out = ops.attend_and_pool_grouped(t, h, *(wg[k] for k in ab.WKEYS), plan, mma=mma)
    (out * _dev(case.g[plan.perm])).sum().backward()
    torch.cuda.synchronize()
    inv = torch.from_numpy(plan.inverse.astype(np.int64))
    got = {"pooled": out.detach().cpu()[inv].numpy()}
    got.update({k: wg[k].grad.cpu().numpy() for k in ab.WKEYS})
    rows = None
    if rowgrads:
        dh, off = h.grad.cpu().numpy(), plan.row_off
        per_imp = [None] * plan.B
        for g in range(plan.G):
            for i, b in enumerate(plan.perm[plan.bounds[g]:plan.bounds[g + 1]]):
                per_imp[b] = dh[off[g] + i * plan.H_g[g]:off[g] + (i + 1) * plan.H_g[g]]
        rows = {"d_target": list(t.grad.cpu()[inv].numpy()), "d_history": per_imp}
    return got, rows


NODE_ARMS = [(shape, G, arm, "f32") for shape in NODE_SHAPES for G in ((2,) if shape[3] == 400 else (1, 2, 3)) for arm in ("default", "dp", "weights only")]
NODE_ARMS += [((7, 3, 37, 64), G, arm, "bf16x3") for G in (1, 2, 3) for arm in ("default", "weights only")]


@pytest.mark.parametrize("shape,G,arm,arithmetic", NODE_ARMS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_grouped_node_is_within_the_attention_budget(lib, monkeypatch, shape, G, arm, arithmetic):
    from news_recommendation_model_amd import compact
    monkeypatch.delenv("NRM_BWD_DP", raising=False)
    if arm == "dp":
        monkeypatch.setenv("NRM_BWD_DP", "1")
    B, T, H, D = shape
    case = _node_case(shape)
    plan = compact.plan_history_groups(NODE_SHAPES[shape], H, max_groups=G, quantum=1)
    assert plan.G == G and (G == 1 or plan.R < B * H)
    rowgrads = arm != "weights only"
    got, rows = _run_grouped(case, plan, arithmetic, rowgrads)
    r = ab.assert_within_budget(got, case, arithmetic, rowgrads=False)
    key = f"{shape} G{G} {arm} {arithmetic}"
    _record["node"][key] = {f"{p}|{n}": float(v) for (p, n), v in r.items()}
    if not rowgrads:
        return
    r64 = case.reference(torch.float64)
    yards = [case.reference(torch.float32)] + ([ab.emulate(case, "bf16x3")] if arithmetic == "bf16x3" else [])
    form = {"d_target": list, "d_history": lambda a: _reduce_dh(np.asarray(a), plan)}
    for name in ("d_target", "d_history"):
        ref = form[name](r64[name])
        for i, norm in enumerate(("max", "l2")):
            e = ab._piece_err(name, rows[name], ref)[i]
            y = max([FLOOR] + [ab._piece_err(name, form[name](yd[name]), ref)[i] for yd in yards])
            _record["node"][key][f"{name}|{norm}"] = e / y
            assert e <= ab.M[arithmetic] * y, (name, norm, e / y)


# ------------------------------------------------------------------------------------------------ the whole training step
@pytest.fixture(scope="module")
def step_case():
    from news_recommendation_model_amd import synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    batch = padded_batch(dims, L_LIST, H_ID, 5, seed=29)
    sd = synth.make_state_dict(dims, seed=1, user_num=int(batch["user_num"]))
    return dims, batch, sd, oracle_step_with_bounds(sd, batch)          # the float64 oracle step, once


def _spied_step(dims, batch, sd, steps=1, **kw):
    """``steps`` calls of trainer.train_step with FlatAdam on a fresh model -> [(loss, logits, flat gradient as gathered)] and the model."""
    from news_recommendation_model_amd import trainer
    model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda").train()
    opt = trainer.FlatAdam(model)
    grabbed, real = [], opt.step

    def step(zero_grad=True):
        opt.collect_grads()                       # (verify_deferred_targets runs here: a copied gradient buffer raises)
        grabbed.append(opt.flat_grad.clone())
        return real(zero_grad=zero_grad)
    opt.step = step
    tb = trainer.batch_to_device(batch, "cuda")
    out = []
    for _ in range(steps):
        loss, logits = trainer.train_step(model, opt, tb, **kw)
        out.append((float(loss), logits.cpu().numpy(), grabbed[-1].cpu().numpy()))
    torch.cuda.synchronize()
    return out, model, opt


def _tensor_errs(flat, opt, model, g_ref):
    out = {}
    for (k, p), o in zip(model.named_parameters(), opt.offsets):
        out[k] = (flat[o:o + p.numel()].reshape(tuple(p.shape)), g_ref[k])
    return out


@pytest.mark.parametrize("max_groups", [1, 2, 4])
def test_compact_training_step_against_the_float64_oracle(lib, step_case, max_groups):
    dims, batch, sd, (loss_o, r_o, g_o, bounds) = step_case
    (dense,), dm, dopt = _spied_step(dims, batch, sd)
    (comp,), cm, copt = _spied_step(dims, batch, sd, compact_history=True, max_groups=max_groups)
    rec = _record["step"].setdefault(f"max_groups {max_groups}", {})
    for what, d, c, ref in (("loss", dense[0], comp[0], loss_o), ("logits", dense[1], comp[1], r_o)):
        e, y = rel_err(c, ref), max(rel_err(d, ref), FLOOR)
        rec[what] = e / y
        print(f"max_groups {max_groups}: {what}: compact {e:.2e}, dense HIP {rel_err(d, ref):.2e}, ratio {e / y:.2f}")
        assert e < FWD_TOL and e <= M_TRAIN_HIST * y, what
    gscale = max(float(np.abs(v).max()) for v in g_o.values())
    dt, ct = _tensor_errs(dense[2], dopt, dm, g_o), _tensor_errs(comp[2], copt, cm, g_o)
    for k in ct:
        got, ref = ct[k]
        if k in ZERO_GRAD_KEYS:
            assert np.abs(got).max() < 1e-5 * max(1.0, gscale), k
            continue
        assert (np.abs(got - ref) <= grad_tolerance(k, ref, GRAD_TOL, bounds)).all(), (k, float(np.abs(got - ref).max()))
        e, y = rel_err(got, ref), max(rel_err(dt[k][0], ref), FLOOR)
        rec[k] = e / y
        print(f"max_groups {max_groups}: {k}: compact {e:.2e}, dense HIP {rel_err(dt[k][0], ref):.2e}, ratio {e / y:.2f}")
        assert e <= _m_step(k) * y, (k, e / y)


def test_three_lockstep_optimizer_steps_agree_with_the_dense_step(lib, step_case):
    """FlatAdam under deferred slab reductions (train_step's default).  Before each of three steps the compact model is given the dense
    model's weights, Adam moments and BatchNorm buffers; both then step on the same batch, and the float64 oracle steps from the same
    weights.  Every parameter still has ONE gradient buffer (collect_grads' verify_deferred_targets raises otherwise) and the flat
    gradient stays within the step gate of the dense HIP step's on each step."""
    from news_recommendation_model_amd import ops, trainer
    dims, batch, sd, _ = step_case
    built = []
    for kw in ({}, dict(compact_history=True, max_groups=4)):
        model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda").train()
        opt = trainer.FlatAdam(model)
        grabbed, real = [], opt.step

        def step(zero_grad=True, opt=opt, grabbed=grabbed, real=real):
            opt.collect_grads()
            grabbed.append(opt.flat_grad.clone())
            return real(zero_grad=zero_grad)
        opt.step = step
        built.append((model, opt, grabbed, kw))
    (dm, dopt, dgrab, _), (cm, copt, cgrab, ckw) = built
    tb = trainer.batch_to_device(batch, "cuda")
    for i in range(3):
        copt.flat_param.copy_(dopt.flat_param); copt.exp_avg.copy_(dopt.exp_avg); copt.exp_avg_sq.copy_(dopt.exp_avg_sq); copt.state.copy_(dopt.state)
        cm.bn.load_state_dict(dm.bn.state_dict())
        ops.repack_persistent(copt.params)
        now = {k: v.detach().cpu().numpy() for k, v in dm.state_dict().items()}
        loss_o, r_o, g_o, bounds = oracle_step_with_bounds(now, batch)
        ld, od = trainer.train_step(dm, dopt, tb)
        lc, oc = trainer.train_step(cm, copt, tb, **ckw)
        rec = _record["step"].setdefault(f"lock-step {i}", {})
        for what, d, c, ref in (("loss", float(ld), float(lc), loss_o), ("logits", od.cpu().numpy(), oc.cpu().numpy(), r_o)):
            rec[what] = rel_err(c, ref) / max(rel_err(d, ref), FLOOR)
        gd, gc = dgrab[-1].cpu().numpy(), cgrab[-1].cpu().numpy()
        for (k, p), o in zip(dm.named_parameters(), dopt.offsets):
            if k in ZERO_GRAD_KEYS:
                continue
            ref = g_o[k]
            rec[k] = rel_err(gc[o:o + p.numel()].reshape(ref.shape), ref) / max(rel_err(gd[o:o + p.numel()].reshape(ref.shape), ref), FLOOR)
        worst = max(rec, key=lambda k: rec[k] / _m_step(k))
        print(f"lock-step {i}: worst ratio {rec[worst]:.2f} ({worst}); instant-interest {rec[II_W]:.2f} / {rec[II_B]:.2f}")
    for i in range(3):
        for k, v in _record["step"][f"lock-step {i}"].items():
            assert v <= _m_step(k), (i, k, v)
    assert copt.steps == 3 and dopt.steps == 3
    torch.cuda.synchronize()


# what only a step on compacted CANDIDATE lists launches (tests/test_gpu_candidate_train.py asserts them of that step)
WEIGHTED_ENTRIES = ("nrm_colreduce_roww", "nrm_bn_backward_roww", "nrm_loss_fwd_bwd_wlast")


def test_a_dense_plan_is_bitwise_the_dense_step(lib, step_case, monkeypatch):
    """All L_b = H: the plan is dense and the step continues as compact_history=False does.  Four dense and four dense-plan steps run
    alternately from the same state.  Every dense-plan step issues exactly the dense step's native calls, with the same integer
    arguments, around the one length measurement; loss and logits are bitwise the dense step's.  Gradients: a tensor on which all four
    dense steps agree bit for bit must come out of the dense-plan steps with those very bits.  Float atomics (slab reductions, the dz pass's
    dw2 | db2, the front end's table gradients) land in any order, so some tensors differ between two DENSE steps; only a tensor that
    this very run shows to differ from dense step to dense step is held to the dense steps' own spread instead.  Such a tensor may
    still agree over four dense steps by chance (seen on the MI355X: the one-element db2, one ulp apart in the next step), so the bitwise
    demand on an agreeing tensor is that some dense-plan step reproduces the bits and none leaves the spread gate."""
    from news_recommendation_model_amd import native, synth
    dims, _, sd, _ = step_case
    batch = synth.make_batch(dims, 6, H_ID, 5, seed=31)                   # no padded rows: every L_b = H
    sd = synth.make_state_dict(dims, seed=1, user_num=int(batch["user_num"]))
    seen, real = [], native.call

    def call(name, *args, tag=None):
        seen.append((name, tag) + tuple(a for a in args if isinstance(a, (int, float))))
        return real(name, *args, tag=tag)
    monkeypatch.setattr(native, "call", call)
    dense, plan_runs, calls = [], [], {}
    for i in range(8):
        del seen[:]
        (res,), model, opt = _spied_step(dims, batch, sd, **(dict(compact_history=True, max_groups=4) if i % 2 else {}))
        (plan_runs if i % 2 else dense).append(res)
        calls.setdefault(i % 2, []).append(list(seen))
    for c in calls[1]:
        lens = [k for k, x in enumerate(c) if x[0] == "nrm_history_len"]
        assert len(lens) == 1 and c[:lens[0]] + c[lens[0] + 1:] == calls[0][0]
    assert all(c == calls[0][0] for c in calls[0])
    names = [x[0] for x in calls[0][0]]                 # the dense step passes no row weight: the plain kernels, none of the weighted ones
    assert not [e for e in WEIGHTED_ENTRIES if e in names] and all(e in names for e in ("nrm_colreduce", "nrm_bn_backward", "nrm_loss_fwd_bwd"))
    for r in dense[1:] + plan_runs:
        assert r[0] == dense[0][0] and r[1].tobytes() == dense[0][1].tobytes()
    bitwise = spread = 0
    for (k, p), o in zip(model.named_parameters(), opt.offsets):
        d = [r[2][o:o + p.numel()] for r in dense]
        c = [r[2][o:o + p.numel()] for r in plan_runs]
        gate = 4 * max([rel_err(x, d[0]) for x in d[1:]] + [4 * FLOOR])         # a few ulps of fp32 atomics at the least
        assert all(rel_err(x, d[0]) <= gate for x in c), k
        if len({x.tobytes() for x in d}) == 1:
            bitwise += 1
            assert any(x.tobytes() == d[0].tobytes() for x in c), k
        else:
            spread += 1
    print(f"gradient tensors: {bitwise} bitwise reproducible over four dense steps (reproduced bit for bit by the dense plan), {spread} not")
    assert bitwise > 0


def test_prefetcher_measures_the_lengths_on_a_side_stream(lib, step_case, monkeypatch):
    from news_recommendation_model_amd import trainer
    dims, batch, sd, _ = step_case
    pf = trainer.BatchPrefetcher([batch, batch], "cuda", history_len=True)
    seen = 0
    for tb, slot in pf:
        host, done, ptr, version = tb["history_len_host"]
        done.synchronize()
        assert host.is_pinned() and host.tolist() == L_LIST and (ptr, version) == (tb["x_history"].data_ptr(), tb["x_history"]._version)
        pf.release(slot)
        seen += 1
    assert seen == 2
    model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda").train()
    # lengths are used only for the tensor contents they were measured on: a batch refreshed in place is measured again
    from news_recommendation_model_amd import native
    opt, seen, real = trainer.FlatAdam(model), [], native.call
    monkeypatch.setattr(native, "call", lambda name, *a, tag=None: (seen.append(name), real(name, *a, tag=tag))[1])
    tb = trainer.attach_history_len(trainer.batch_to_device(batch, "cuda"))
    trainer.train_step(model, opt, tb, compact_history=True, max_groups=4)
    assert seen.count("nrm_history_len") == 1 and seen.count("nrm_history_gather_groups") == 1
    # the history-only compacted step keeps every candidate row: unweighted BatchNorm and loss kernels, none of the weighted ones
    assert not [e for e in WEIGHTED_ENTRIES if e in seen] and all(e in seen for e in ("nrm_colreduce", "nrm_bn_backward", "nrm_loss_fwd_bwd"))
    tb["x_history"].copy_(tb["x_history"].flip(0))                       # other lengths in the same buffer
    del seen[:]
    loss_stale, _ = trainer.train_step(model, opt, tb, compact_history=True, max_groups=4)
    assert seen.count("nrm_history_len") == 1 and np.isfinite(float(loss_stale))
    monkeypatch.setattr(native, "call", real)
    hist = trainer.train_epochs(model, trainer.FlatAdam(model), lambda: [batch], 1, compact_history=True, max_groups=4)
    assert np.isfinite(hist[0]["loss_avg"]) and hist[0]["impressions"] == len(L_LIST)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(lib, step_case):
    from news_recommendation_model_amd import compact, ops, trainer
    dims, batch, sd, _ = step_case
    model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda").train()
    opt = trainer.FlatAdam(model)
    tb = trainer.batch_to_device(batch, "cuda")
    with pytest.raises(RuntimeError, match="inference only"):            # (re-asserted: forward_compact stays an inference entry)
        plan = compact.build_plan([0] * len(L_LIST), 5, history_len=L_LIST, H=H_ID)
        model.forward_compact(tb["x_history"].reshape(-1, tb["x_history"].shape[2])[:plan.R], tb["x_target"][:, 0], tb["x_global"][:, 0], plan)
    # a second backward through the grouped node
    case = _node_case((7, 3, 37, 64))
    plan = compact.plan_history_groups(NODE_SHAPES[(7, 3, 37, 64)], 37, max_groups=2, quantum=1)
    arena = np.concatenate([case.h[plan.perm[b], :plan.H_g[g]] for g in range(plan.G) for b in range(plan.bounds[g], plan.bounds[g + 1])])
    wg = [_dev(case.w[k]).requires_grad_(True) for k in ab.WKEYS]
    t, h = _dev(case.t[plan.perm]).requires_grad_(True), _dev(arena).requires_grad_(True)
    inv = torch.from_numpy(plan.inverse.astype(np.int64))
    seed = _dev(case.g[plan.perm])

    def walk(out, retain):
        """One backward -> (row gradients, result dict of the weight gradients for the attention budget)."""
        g = torch.autograd.grad(out, [t, h] + wg, seed, retain_graph=retain)
        got = {"pooled": out.detach().cpu()[inv].numpy()}
        got.update({k: x.cpu().numpy() for k, x in zip(ab.WKEYS, g[2:])})
        return g[:2], got
    out = ops.attend_and_pool_grouped(t, h, *wg, plan)
    rows_first, w_first = walk(out, True)
    with pytest.raises(RuntimeError, match="second backward"):
        torch.autograd.grad(out, wg, seed, retain_graph=True)
    prev = ops.set_retain_attention_graph(True)
    try:
        out = ops.attend_and_pool_grouped(t, h, *wg, plan)
        rows_a, w_a = walk(out, True)
        rows_b, w_b = walk(out, True)
    finally:
        ops.set_retain_attention_graph(prev)
    # the row gradients come from kernels without atomics: bit for bit on every walk (as the dense node's, tests/test_gpu_model.py);
    # the weight gradients are reduced with float atomics in any order, so each walk is held to the float64 reference instead
    for rows in (rows_a, rows_b):
        assert all(torch.equal(x, y) for x, y in zip(rows, rows_first))
    for got in (w_first, w_a, w_b):
        ab.assert_within_budget(got, case, "f32", rowgrads=False)
    # inside a stream capture (checked before anything is enqueued)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="stream capture"):
        with torch.cuda.graph(graph):
            trainer.train_step(model, opt, tb, compact_history=True)
    with pytest.raises(RuntimeError, match="captured step"):
        trainer.GraphedTrainStep(model, opt, tb, compact_history=True)
    torch.cuda.synchronize()


def test_opcheck_on_the_new_ops(lib):
    from news_recommendation_model_amd import compact
    case = _node_case((7, 3, 37, 64))
    plan = compact.plan_history_groups(NODE_SHAPES[(7, 3, 37, 64)], 37, max_groups=2, quantum=1)
    arena = np.concatenate([case.h[plan.perm[b], :plan.H_g[g]] for g in range(plan.G) for b in range(plan.bounds[g], plan.bounds[g + 1])])
    w = [_dev(case.w[k]) for k in ab.WKEYS]
    b0, hg = [int(x) for x in plan.bounds], [int(x) for x in plan.H_g]
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    tg = [3] * plan.G
    args = (_dev(case.t[plan.perm]).flatten(0, 1), _dev(arena), *w, b0, hg, tg, 37, 3, True, 0)
    torch.library.opcheck(torch.ops.nrm.attend_pool_grouped_fwd.default, args, test_utils=tests)
    pooled, s, z = torch.ops.nrm.attend_pool_grouped_fwd(*args)
    z = z.detach()
    torch.library.opcheck(torch.ops.nrm.attend_pool_grouped_bwd.default, (_dev(case.g[plan.perm]).flatten(0, 1), args[0], args[1], w[0], w[2], s, z, b0, hg, tg, 37, 3,
                                                                            0, True, True),
                          test_utils=tests)
    tabs = plan.upload("cuda")
    x = _dev(np.random.default_rng(0).standard_normal((7, 37, 12)))
    torch.library.opcheck(torch.ops.nrm.history_gather_groups.default, (x, tabs["perm"], tabs["bounds"], tabs["row_off"], tabs["H_g"], plan.R), test_utils=tests)
