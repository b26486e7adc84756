"""GPU: training on compacted candidate lists -- the candidate gather against numpy (bitwise) and its padding check,
the row-weight BatchNorm column kernels and the last-column-weighted loss against float64 (yardstick: today's kernel on the EXPANDED input,
a weighted row repeated w times), the whole training step through trainer.train_step(compact_candidates=True) against the float64 oracle
step with the dense HIP step as the yardstick, its three mutants, three lock-step optimizer steps, the dense plan (bitwise the dense step),
the refusals, opcheck and train_epochs.

Set NRM_CANDIDATE_TRAIN_RECORD=<path> to write every measured ratio to a JSON file (profiles/candidate_train.json is such a record)."""
import json
import os

import numpy as np
import pytest
import torch

from candidate_train_util import B_ID, COUNTS, H_ID, T_ID, padded_batch
from compact_util import percentile_counts
from golden_util import II_B, II_W, ZERO_GRAD_KEYS, grad_tolerance, oracle_step_with_bounds, rel_err

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
M_ROWW = 4             # two bits: one product by w in place of w equal addends (fixed by reasoning, not measured: M_POOL of section 5e)
# profiles/candidate_train.json (one MI355X run of this file): the worst err(compact step) / max(err(dense HIP step), 2^-23) of any tensor but
# the two below is 9.23 (text_img_attention.mlp.fc2.bias, third lock-step step; 6.41 over the single steps: label_attention.mlp.fc2.bias, B = 32,
# T = 15, max_groups 4); M_TRAIN_CAND is the smallest power of two >= 4 x that figure (the rule of DESIGN.md section 3b).  Two earlier runs of
# this file gave 5.69 and 4.63 (the same tensors): the two fc2 bias gradients are sums of the score gradients over every (b, t, h), reduced
# with float atomics, and the dense step's own error on them moves from run to run.  The record kept is the run with the worst figure.
M_TRAIN_CAND = 64
# The two instant-interest gradients are sums that cancel: noise over noise, a constant of their own by the same rule,
# as in section 5e: recorded worst 5.38 (both flags together; 3.87 over the lock-step steps).
M_TRAIN_CAND_II = 32
FWD_TOL, GRAD_TOL = 1e-3, 1e-2
_record = {"colreduce": {}, "bn_backward": {}, "loss": {}, "step": {}, "mutants": {}}


def _m_step(key):
    return M_TRAIN_CAND_II if key in (II_W, II_B) else M_TRAIN_CAND


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("NRM_CANDIDATE_TRAIN_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({"M_ROWW": M_ROWW, "M_TRAIN_CAND": M_TRAIN_CAND, "M_TRAIN_CAND_II": M_TRAIN_CAND_II,
                       **{k: {kk: v[kk] for kk in sorted(v)} for k, v in _record.items()}}, f, indent=1)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _call(name, *args):
    from news_recommendation_model_amd import native
    native.call(name, *args, native.stream_ptr())


def _p(t):
    from news_recommendation_model_amd import native
    return native.ptr(t) if t is not None else None


def _gate(group, key, got, yard, truth, scale=None):
    """err(got) <= M_ROWW * max(err(yardstick), 2^-23), both against the float64 truth in the max-norm (``scale``: another norm's unit)."""
    if scale is None:
        e, y = rel_err(got, truth), rel_err(yard, truth)
    else:
        e, y = (float(np.abs(np.asarray(x, dtype=np.float64) - truth).max()) / (scale + 1e-30) for x in (got, yard))
    _record[group][key] = e / max(y, FLOOR)
    print(f"{group} {key}: weighted {e:.2e}, expanded yardstick {y:.2e}, ratio {e / max(y, FLOOR):.2f}")
    assert e <= M_ROWW * max(y, FLOOR), (group, key, e, y)


# ------------------------------------------------------------------------------------------------ gather
GATHER_COUNTS = [0, 1, 7, 0, 1, 6, 1, 0, 7]           # sorted: three lists of width 1, three of width 2, three of width T


def _gather_inputs(dtype, cols):
    rng = np.random.default_rng(cols)
    B, T = len(GATHER_COUNTS), T_ID
    xt = rng.standard_normal((B, T, cols)).astype(dtype)
    xg = rng.standard_normal((B, T, 3)).astype(dtype)
    lab = rng.integers(0, 2, (B, T)).astype(dtype)
    xt[2, 3, 0] = -0.0
    xt[5, 6, 1] = np.nan                                # a padded cell: compared bit for bit, NaN == NaN
    for b, n in enumerate(GATHER_COUNTS):               # every padded candidate equals the FIRST one (non-zero: a wrong row would show)
        if n < T:
            xt[b, n:], xg[b, n:], lab[b, n:] = xt[b, n], xg[b, n], lab[b, n]
    return xt, xg, lab


def _gather(plan, xt, xg, lab):
    from news_recommendation_model_amd import ops
    plan.device_tables = None
    tabs = plan.upload("cuda")
    return ops.candidate_gather_groups(_dev(xt), _dev(xg), _dev(lab), tabs["perm"], tabs["bounds"], tabs["row_off"], tabs["T_g"], plan.N)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cols", [80, 7])
def test_candidate_gather_is_bitwise_and_checks_the_dropped_cells(lib, dtype, cols):
    from news_recommendation_model_amd import compact, ops
    B, T = len(GATHER_COUNTS), T_ID
    xt, xg, lab = _gather_inputs(dtype, cols)
    plan = compact.plan_candidate_groups(T - np.asarray(GATHER_COUNTS), T, max_groups=3)
    assert plan.T_g.tolist() == [1, 2, T] and plan.perm.tolist() != list(range(B))
    one = compact.plan_candidate_groups(T - np.asarray(GATHER_COUNTS), T, max_groups=1)
    assert one.T_g.tolist() == [T]
    ops.check_pad_errors("cuda")
    for p in (plan, one):
        got = [t.cpu().numpy() for t in _gather(p, xt, xg, lab)]
        cells = [(p.perm[b], p.T_g[g]) for g in range(p.G) for b in range(p.bounds[g], p.bounds[g + 1])]
        for a, src in zip(got[:3], (xt, xg, lab)):
            want = np.concatenate([src[b, :tg] for b, tg in cells])
            assert a.dtype == dtype and a.shape == want.shape and a.tobytes() == want.tobytes()
        want_w = np.concatenate([[1.0] * (tg - 1) + [float(T - tg + 1)] for _b, tg in cells]).astype(np.float32)
        assert got[3].dtype == np.float32 and got[3].tolist() == want_w.tolist()
        ops.check_pad_errors("cuda")                                # clean data: no flag
    # one dropped cell altered, in each of the three tensors in turn: the host's empty_num is checked, not trusted
    for which in range(3):
        bad = [a.copy() for a in (xt, xg, lab)]
        b = 3                                                       # counts 0: a group of width 1, cells 1 .. T - 1 are dropped
        bad[which][(b, T - 1) + ((cols - 1,) if which == 0 else (2,) if which == 1 else ())] += 1.0
        _gather(plan, *bad)
        with pytest.raises(ValueError, match="padded"):
            ops.check_pad_errors("cuda")
        ops.check_pad_errors("cuda")                                # cleared by the raise
    # a kept cell may hold anything
    ok = [a.copy() for a in (xt, xg, lab)]
    ok[0][2, 3] += 1.0
    _gather(plan, *ok)
    ops.check_pad_errors("cuda")


# ------------------------------------------------------------------------------------------------ weighted column kernels
def _row_weights(R, w):
    wts = np.ones(R, dtype=np.int64)
    wts[(1 if R < 3 else 2)::(2 if R < 3 else 3)] = w              # every third row (every second of two) stands for w rows
    return wts


@pytest.mark.parametrize("w", [1, 2, 14])
@pytest.mark.parametrize("N", [8, 268, 1608])
def test_row_weight_column_kernels_against_float64(lib, N, w):
    for R in (2, 5, 63, 64, 65, 257):
        rng = np.random.default_rng(10000 * N + 100 * R + w)
        wts = _row_weights(R, w)
        n = int(wts.sum())
        x = (rng.standard_normal((R, N)) + 0.5).astype(np.float32)
        g = rng.standard_normal((R, N)).astype(np.float32)            # the per-copy gradient; G = w g is what reaches the kernel
        add = rng.standard_normal((R, N)).astype(np.float32)
        gamma = (1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32)
        x64, g64 = x.astype(np.float64), g.astype(np.float64)
        wf = wts.astype(np.float64)[:, None]
        mean64 = (wf * x64).sum(0) / n
        mean = mean64.astype(np.float32)
        var64 = (wf * (x64 - mean.astype(np.float64)) ** 2).sum(0) / n
        rstd = (1.0 / np.sqrt(var64 + 1e-5)).astype(np.float32)
        x_e = np.repeat(x, wts, axis=0)
        key = f"R{R} N{N} w{w}"
        xd, xed, wd, md = _dev(x), _dev(x_e), _dev(wts.astype(np.float32)), _dev(mean)
        zeros = lambda: torch.zeros(N, dtype=torch.float32, device="cuda")          # noqa: E731
        # mode 0: sum_r w_r x
        got, yard = zeros(), zeros()
        _call("nrm_colreduce_roww", 0, _p(xd), None, _p(wd), _p(got), R, N, N)
        _call("nrm_colreduce", 0, _p(xed), None, None, None, _p(yard), None, n, N, N)
        _gate("colreduce", "sum|" + key, got.cpu().numpy(), yard.cpu().numpy(), (wf * x64).sum(0))
        # mode 1: sum_r w_r (x - mean)^2 around the SAME fp32 mean
        got1, yard1 = zeros(), zeros()
        _call("nrm_colreduce_roww", 1, _p(xd), _p(md), _p(wd), _p(got1), R, N, N)
        _call("nrm_colreduce", 1, _p(xed), None, _p(md), None, _p(yard1), None, n, N, N)
        _gate("colreduce", "centred square|" + key, got1.cpu().numpy(), yard1.cpu().numpy(), (wf * (x64 - mean.astype(np.float64)) ** 2).sum(0))
        # backward: dx_r = gamma rstd (G_r - w_r s0/n - w_r xhat_r s1/n) + add_r.  G = w g and add are what the arena row receives (the
        # sums over its copies); the expanded batch gets G / w and add / w per copy, and the yardstick is the SUM of its copies' dx.  Each
        # side is held to the float64 evaluation of its own fp32 inputs (G / w and add / w are rounded once more).
        f64 = lambda a: a.astype(np.float64)                           # noqa: E731
        G = (wf * g64).astype(np.float32)
        xhat64 = (x64 - f64(mean)) * f64(rstd)
        s0, s1 = f64(G).sum(0).astype(np.float32), (f64(G) * xhat64).sum(0).astype(np.float32)
        k64 = f64(gamma) * f64(rstd)
        truth = k64 * (f64(G) - wf * f64(s0) / n - wf * xhat64 * f64(s1) / n) + f64(add)
        rd, gd, s0d, s1d = _dev(rstd), _dev(gamma), _dev(s0), _dev(s1)
        dx = torch.empty(R, N, dtype=torch.float32, device="cuda")
        Gd, addd = _dev(G), _dev(add)                                   # (held: a pointer does not keep its tensor alive)
        _call("nrm_bn_backward_roww", _p(xd), _p(Gd), _p(md), _p(rd), _p(gd), _p(s0d), _p(s1d), _p(addd), _p(wd), _p(dx), R, n, N, N)
        Ge, add_e = (np.repeat((f64(a) / wf).astype(np.float32), wts, axis=0) for a in (G, add))
        dx_e = torch.empty(n, N, dtype=torch.float32, device="cuda")
        Ged, added = _dev(Ge), _dev(add_e)
        _call("nrm_bn_backward", _p(xed), _p(Ged), _p(md), _p(rd), _p(gd), _p(s0d), _p(s1d), _p(added), _p(dx_e), n, N, N, 1)
        torch.cuda.synchronize()
        first = np.concatenate([[0], np.cumsum(wts)[:-1]])
        truth_e = k64 * (f64(Ge) - f64(s0) / n - np.repeat(xhat64, wts, axis=0) * f64(s1) / n) + f64(add_e)
        e = rel_err(dx.cpu().numpy(), truth)
        y = rel_err(np.add.reduceat(f64(dx_e.cpu().numpy()), first, axis=0), np.add.reduceat(truth_e, first, axis=0))
        _record["bn_backward"][key] = e / max(y, FLOOR)
        print(f"bn_backward {key}: weighted {e:.2e}, expanded yardstick {y:.2e}, ratio {e / max(y, FLOOR):.2f}")
        assert e < 1e-5 and e <= M_ROWW * max(y, FLOOR), (key, e, y)
        if w == 1:                                                      # bitwise today's kernels
            assert torch.equal(got, yard) and torch.equal(got1, yard1)
            assert torch.equal(dx, dx_e)
    torch.cuda.synchronize()


def test_batch_norm_with_row_weights_is_the_expanded_batch_norm(lib):
    """ops.batch_norm / ops.gate_block with (row_weight, n_rows): output rows, running statistics and every gradient are those of the
    module on the expanded batch (float64 nn.BatchNorm1d as the truth, the unweighted ops on the expanded rows as the yardstick)."""
    from news_recommendation_model_amd import ops
    R, N, w = 65, 24, 5
    rng = np.random.default_rng(3)
    wts = _row_weights(R, w)
    n = int(wts.sum())
    x = (rng.standard_normal((R, N)) + 0.3).astype(np.float32)
    seed = rng.standard_normal((R, N)).astype(np.float32)              # per-copy output gradient
    first = np.concatenate([[0], np.cumsum(wts)[:-1]])

    def run(xa, weights, seed_rows, dtype=torch.float32, module=False):
        bn = torch.nn.BatchNorm1d(N).to("cuda", dtype).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, N)); bn.bias.copy_(torch.linspace(-1, 1, N))
        xd = _dev(xa, dtype).requires_grad_(True)
        if module:
            y = bn(xd)
        elif weights is None:
            y = ops.batch_norm(xd, bn)
        else:
            y = ops.batch_norm(xd, bn, _dev(weights.astype(np.float32)), n)
        (y * _dev(seed_rows, dtype)).sum().backward()
        return [t.detach().double().cpu().numpy() for t in (y, xd.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)]
    x_e, seed_e = np.repeat(x, wts, axis=0), np.repeat(seed, wts, axis=0)
    truth = run(x_e, None, seed_e, torch.float64, module=True)
    yard = run(x_e, None, seed_e)
    got = run(x, wts, seed * wts[:, None].astype(np.float32))          # the arena's output gradient carries the weight (the loss puts it there)
    fold = lambda a, i: a[first] if i == 0 else np.add.reduceat(a, first, axis=0) if i == 1 else a      # noqa: E731
    for i, name in enumerate(("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")):
        _gate("bn_backward", f"ops.batch_norm {name}", got[i], fold(yard[i], i), fold(truth[i], i))


# ------------------------------------------------------------------------------------------------ weighted loss
def _loss_case(rng, B, T, w, scale, label_dtype):
    out = (rng.standard_normal((B, T)) * scale).astype(np.float32)
    label = np.zeros((B, T), dtype=label_dtype)
    if T > 1 or w == 1:
        label[np.arange(B), rng.integers(0, max(T - 1, 1), B)] = 1     # a live column: the last one is padding where w > 1
    uid = rng.integers(0, 9, B)
    delta = (rng.standard_normal(9) * 0.3).astype(np.float32)
    return out, label, uid, delta


def _loss_native(out, label, uid, delta, w=None, inv_n=None):
    B, T = out.shape
    o, y, u, d = _dev(out), _dev(label), _dev(uid.astype(np.int64)), _dev(delta)
    loss = torch.zeros((), dtype=torch.float32, device="cuda")
    dout = torch.empty(B * T, 4, dtype=torch.float32, device="cuda")
    dd = torch.zeros(9, dtype=torch.float32, device="cuda")
    from news_recommendation_model_amd import ops
    err = ops.index_error_flag("cuda")
    f64 = 1 if label.dtype == np.float64 else 0
    if w is None:
        _call("nrm_loss_fwd_bwd", _p(o), 1, _p(y), f64, _p(u), _p(d), 9, 0.95, B, T, _p(loss), _p(dout), 4, _p(dd), _p(err))
    else:
        _call("nrm_loss_fwd_bwd_wlast", _p(o), 1, _p(y), f64, _p(u), _p(d), 9, 0.95, B, T, float(w), float(inv_n), _p(loss), _p(dout), 4, _p(dd), _p(err))
    torch.cuda.synchronize()
    assert float(dout[:, 1:].abs().max()) == 0.0
    return float(loss), dout[:, 0].view(B, T).cpu().numpy(), dd.cpu().numpy()


def _loss_truth(out_e, label_e, uid, delta):
    from oracle import user_model_oracle as orc
    o = torch.from_numpy(out_e.astype(np.float64)).requires_grad_(True)
    d = torch.from_numpy(delta.astype(np.float64)).requires_grad_(True)
    with orc.precision(torch.float64):
        loss = orc.user_model_loss({"delta": d}, torch.from_numpy(uid), o, torch.from_numpy(label_e.astype(np.float64)))
    loss.backward()
    return float(loss.detach()), o.grad.numpy(), d.grad.numpy()


LOSS_CASES = [(B, T, 1.0) for T in (1, 2, 15, 64, 65, 257) for B in (1, 5)] + [(5, 15, 60.0)]     # the last: the -100 clamp regime


@pytest.mark.parametrize("label_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("w", [1, 2, 14])
def test_last_column_weighted_loss_against_float64(lib, monkeypatch, w, label_dtype):
    """T <= 256: the register kernel (and, forced, the re-reading one); T = 257: the re-reading one.  The yardstick is today's kernel on the
    expanded logits (the last column repeated w times); dout of the weighted column is the sum over its copies.  dL/ddelta is zero in exact
    arithmetic (softmax is shift invariant), a residue of roundings on both sides: its error is counted in units of the impression's
    term-magnitude sum (sum_t |dout_t|), not of its own vanishing max-norm."""
    fold = lambda a, T: np.concatenate([a[:, :T - 1], a[:, T - 1:].sum(1, keepdims=True)], axis=1)      # noqa: E731
    for B, T, scale in LOSS_CASES:
        for force_long in ((None, "1") if T <= 256 and B == 5 else (None,)):
            if force_long is None:
                monkeypatch.delenv("NRM_LOSS_LONG", raising=False)
            else:
                monkeypatch.setenv("NRM_LOSS_LONG", force_long)
            rng = np.random.default_rng(1000 * T + 10 * w + B)
            out, label, uid, delta = _loss_case(rng, B, T, w, scale, label_dtype)
            out_e = np.concatenate([out] + [out[:, -1:]] * (w - 1), axis=1)
            label_e = np.concatenate([label] + [label[:, -1:]] * (w - 1), axis=1)
            Te = T + w - 1
            inv_n = float(np.float32(1.0) / (np.float32(B) * np.float32(Te)))
            got = _loss_native(out, label, uid, delta, w, inv_n)
            yard = _loss_native(out_e, label_e, uid, delta)
            truth = _loss_truth(out_e, label_e, uid, delta)
            key = f"B{B} T{T} w{w} scale {scale:g} {np.dtype(label_dtype).name} long {force_long}"
            _gate("loss", "value|" + key, got[0], yard[0], truth[0])
            _gate("loss", "dout|" + key, got[1], fold(yard[1].astype(np.float64), T), fold(truth[1], T))
            terms = np.zeros(9)
            np.add.at(terms, uid, np.abs(truth[1]).sum(1))
            _gate("loss", "ddelta|" + key, got[2], yard[2], truth[2], scale=float(terms.max()))
            if w == 1:                                                  # bitwise today's kernel: per row, no atomics
                assert got[1].tobytes() == yard[1].tobytes(), key
    monkeypatch.delenv("NRM_LOSS_LONG", raising=False)


def test_grouped_loss_op_is_the_dense_loss(lib):
    """ops.softmax_bce_loss_grouped over a three-group arena (logits as column 0 of a padded [N, 4] matrix) against the dense op on the
    expanded [B, T] logits: value and, through autograd with a non-unit seed, dout (folded) and ddelta within the kernel gate."""
    from news_recommendation_model_amd import compact, ops
    T = T_ID
    plan = compact.plan_candidate_groups(T - np.asarray(COUNTS), T, max_groups=3)
    rng = np.random.default_rng(8)
    arena = rng.standard_normal(plan.N).astype(np.float32)
    lab_dense = np.zeros((B_ID, T))
    lab_dense[np.arange(B_ID), [b % max(n, 1) for b, n in enumerate(COUNTS)]] = 1
    expand = plan.expand.reshape(B_ID, T)
    dense = arena[expand]                                               # [B, T] in the caller's order
    lab_arena = np.zeros(plan.N)
    lab_arena[expand.reshape(-1)] = lab_dense.reshape(-1)               # (padded cells all carry 0)
    uid = rng.integers(0, 9, B_ID)
    delta = (rng.standard_normal(9) * 0.3).astype(np.float32)
    truth = _loss_truth(dense, lab_dense, uid, delta)
    od = _dev(dense).requires_grad_(True)
    dd = _dev(delta).requires_grad_(True)
    (3.0 * ops.softmax_bce_loss(od, dd, _dev(lab_dense), _dev(uid), 0.95)).backward()
    buf = torch.zeros(plan.N, 4, device="cuda")
    buf[:, 0] = _dev(arena)
    buf.requires_grad_(True)
    dg = _dev(delta).requires_grad_(True)
    loss = ops.softmax_bce_loss_grouped(buf[:, 0], dg, _dev(lab_arena), _dev(uid[plan.perm]), plan, 0.95)
    (3.0 * loss).backward()
    fold = lambda a: np.bincount(expand.reshape(-1), weights=np.asarray(a, dtype=np.float64).reshape(-1), minlength=plan.N)      # noqa: E731
    _gate("loss", "op value", float(loss), float(ops.softmax_bce_loss(od.detach(), dd.detach(), _dev(lab_dense), _dev(uid), 0.95)), truth[0])
    _gate("loss", "op dout", buf.grad[:, 0].cpu().numpy() / 3.0, fold(od.grad.cpu().numpy() / 3.0), fold(truth[1]))
    terms = np.zeros(9)
    np.add.at(terms, uid, np.abs(truth[1]).sum(1))
    _gate("loss", "op ddelta", dg.grad.cpu().numpy() / 3.0, dd.grad.cpu().numpy() / 3.0, truth[2], scale=float(terms.max()))


# ------------------------------------------------------------------------------------------------ the whole training step
def _make_case(counts, H, T, seed):
    from news_recommendation_model_amd import synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    batch = padded_batch(dims, counts, H, T, seed=seed)
    sd = synth.make_state_dict(dims, seed=1, user_num=int(batch["user_num"]))
    loss_o, r_o, g_o, bounds = oracle_step_with_bounds(sd, batch)          # the float64 oracle step, once
    # the running statistics after the step, from the float64 batch statistics
    from candidate_train_util import dense_oracle_step
    from oracle import user_model_oracle as orc
    mean, var = (s.numpy() for s in dense_oracle_step(orc, sd, batch)[3])
    n = len(counts) * T
    running = {"bn.running_mean": 0.9 * sd["bn.running_mean"] + 0.1 * mean, "bn.running_var": 0.9 * sd["bn.running_var"] + 0.1 * var * n / (n - 1)}
    return dims, batch, sd, (loss_o, r_o, g_o, bounds, running)


@pytest.fixture(scope="module")
def step_cases():
    small = _make_case(COUNTS, H_ID, T_ID, seed=29)
    counts = percentile_counts(np.random.default_rng(17), 32, 15)
    return {"B9 T7": small, "B32 T15 percentile": _make_case(counts.tolist(), 6, 15, seed=37)}


def _spied_step(dims, batch, sd, steps=1, **kw):
    """``steps`` calls of trainer.train_step with FlatAdam on a fresh model -> [(loss, logits, flat gradient as gathered, running stats)]."""
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
        out.append((float(loss), logits.cpu().numpy(), grabbed[-1].cpu().numpy(),
                    {"bn.running_mean": model.bn.running_mean.cpu().numpy().copy(), "bn.running_var": model.bn.running_var.cpu().numpy().copy()}))
    torch.cuda.synchronize()
    return out, model, opt


def _step_ratios(dense, comp, dm, dopt, cm, copt, oracle, check=True):
    """{tensor: err(compact) / max(err(dense HIP), 2^-23)} against the float64 oracle, with the absolute gates of the dense step's own tests."""
    loss_o, r_o, g_o, bounds, running = oracle
    rec = {}
    pairs = [("loss", dense[0], comp[0], loss_o), ("logits", dense[1], comp[1], r_o)] + [(k, dense[3][k], comp[3][k], running[k]) for k in sorted(running)]
    for what, d, c, ref in pairs:
        e, y = rel_err(c, ref), max(rel_err(d, ref), FLOOR)
        rec[what] = e / y
        if check:
            assert e < FWD_TOL, (what, e)
    gscale = max(float(np.abs(v).max()) for v in g_o.values())
    for (k, p), o_c, o_d in zip(cm.named_parameters(), copt.offsets, dopt.offsets):
        got, ref = comp[2][o_c:o_c + p.numel()].reshape(tuple(p.shape)), g_o[k]
        if k in ZERO_GRAD_KEYS:
            if check:
                assert np.abs(got).max() < 1e-5 * max(1.0, gscale), k
            continue
        if check:
            assert (np.abs(got - ref) <= grad_tolerance(k, ref, GRAD_TOL, bounds)).all(), (k, float(np.abs(got - ref).max()))
        rec[k] = rel_err(got, ref) / max(rel_err(dense[2][o_d:o_d + p.numel()].reshape(ref.shape), ref), FLOOR)
    return rec


@pytest.mark.parametrize("max_groups", [1, 2, 4])
@pytest.mark.parametrize("case", ["B9 T7", "B32 T15 percentile"])
def test_compact_candidate_step_against_the_float64_oracle(lib, step_cases, case, max_groups, monkeypatch):
    from news_recommendation_model_amd import native
    dims, batch, sd, oracle = step_cases[case]
    (dense,), dm, dopt = _spied_step(dims, batch, sd)
    seen, real = [], native.call
    monkeypatch.setattr(native, "call", lambda name, *a, tag=None: (seen.append(name), real(name, *a, tag=tag))[1])
    (comp,), cm, copt = _spied_step(dims, batch, sd, compact_candidates=True, max_groups=max_groups)
    monkeypatch.setattr(native, "call", real)
    from news_recommendation_model_amd import compact
    plan = compact.plan_candidate_groups(batch["empty_num"], batch["x_target"].shape[1], max_groups=max_groups)
    assert max_groups < 4 or not plan.dense                 # (one group holds a full list and is the dense step; four groups save enough in both cases)
    if plan.dense:
        assert "nrm_candidate_gather_groups" not in seen and "nrm_loss_fwd_bwd" in seen
    else:                                                   # the compact path ran, and nothing of the dense head beside it
        assert seen.count("nrm_candidate_gather_groups") == 1 and "nrm_loss_fwd_bwd_wlast" in seen and "nrm_bn_backward_roww" in seen
        assert "nrm_loss_fwd_bwd" not in seen and "nrm_bn_backward" not in seen and seen.count("nrm_colreduce_roww") == 2
    assert comp[1].shape == dense[1].shape
    rec = _step_ratios(dense, comp, dm, dopt, cm, copt, oracle)
    _record["step"][f"{case} max_groups {max_groups}"] = rec
    worst = max(rec, key=lambda k: rec[k] / _m_step(k))
    print(f"{case} max_groups {max_groups}: worst ratio {rec[worst]:.2f} ({worst}); instant-interest {rec[II_W]:.2f} / {rec[II_B]:.2f}")
    for k, v in rec.items():
        assert v <= _m_step(k), (k, v)


MUTANT_ENTRIES = {"bn": "nrm_colreduce_roww", "loss": "nrm_loss_fwd_bwd_wlast", "bn_bwd": "nrm_bn_backward_roww"}


@pytest.mark.parametrize("mutant", sorted(MUTANT_ENTRIES))
def test_the_step_gate_rejects_each_missing_weight(lib, step_cases, mutant, monkeypatch):
    """The device path with ONE of the three weights replaced by 1 (a vector of ones handed to the BatchNorm statistics or to bn_backward's
    column terms, wlast = 1 handed to the loss): some tensor must leave the step gate by more than a factor 4."""
    import ctypes
    from news_recommendation_model_amd import native
    dims, batch, sd, oracle = step_cases["B9 T7"]
    (dense,), dm, dopt = _spied_step(dims, batch, sd)
    ones = torch.ones(B_ID * T_ID, dtype=torch.float32, device="cuda")
    real = native.call

    def call(name, *a, tag=None):
        a = list(a)
        if name == MUTANT_ENTRIES[mutant]:
            if mutant == "bn":
                a[3] = native.ptr(ones)
            elif mutant == "bn_bwd":
                a[8] = native.ptr(ones)
            else:
                a[10] = 1.0
        return real(name, *a, tag=tag)
    assert isinstance(native.ptr(ones), ctypes.c_void_p)
    monkeypatch.setattr(native, "call", call)
    (comp,), cm, copt = _spied_step(dims, batch, sd, compact_candidates=True, max_groups=4)
    monkeypatch.setattr(native, "call", real)
    rec = _step_ratios(dense, comp, dm, dopt, cm, copt, oracle, check=False)
    worst = max(rec, key=lambda k: rec[k] / _m_step(k))
    _record["mutants"][mutant] = {"tensor": worst, "ratio": rec[worst], "constant": _m_step(worst)}
    print(f"mutant {mutant}: {worst} at {rec[worst]:.3g} x the dense step's error (constant {_m_step(worst)})")
    assert rec[worst] > 4 * _m_step(worst)


def test_three_lockstep_optimizer_steps_agree_with_the_dense_step(lib, step_cases):
    """As in test_gpu_history_train.py: before each of three steps the compact model is given the dense model's weights, Adam moments and
    BatchNorm buffers; both step on the same batch, the float64 oracle steps from the same weights; every tensor stays within the step gate."""
    from candidate_train_util import dense_oracle_step
    from news_recommendation_model_amd import ops, trainer
    from oracle import user_model_oracle as orc
    dims, batch, sd, _ = step_cases["B9 T7"]
    built = []
    for kw in ({}, dict(compact_candidates=True, max_groups=4)):
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
    n = B_ID * T_ID
    stats = lambda m: {"bn.running_mean": m.bn.running_mean.cpu().numpy().copy(), "bn.running_var": m.bn.running_var.cpu().numpy().copy()}      # noqa: E731
    for i in range(3):
        copt.flat_param.copy_(dopt.flat_param); copt.exp_avg.copy_(dopt.exp_avg); copt.exp_avg_sq.copy_(dopt.exp_avg_sq); copt.state.copy_(dopt.state)
        cm.bn.load_state_dict(dm.bn.state_dict())
        ops.repack_persistent(copt.params)
        now = {k: v.detach().cpu().numpy() for k, v in dm.state_dict().items()}
        loss_o, r_o, g_o, bounds = oracle_step_with_bounds(now, batch)
        mean, var = (s.numpy() for s in dense_oracle_step(orc, now, batch)[3])
        running = {"bn.running_mean": 0.9 * now["bn.running_mean"] + 0.1 * mean, "bn.running_var": 0.9 * now["bn.running_var"] + 0.1 * var * n / (n - 1)}
        ld, od = trainer.train_step(dm, dopt, tb)
        lc, oc = trainer.train_step(cm, copt, tb, **ckw)
        dense = (float(ld), od.cpu().numpy(), dgrab[-1].cpu().numpy(), stats(dm))
        comp = (float(lc), oc.cpu().numpy(), cgrab[-1].cpu().numpy(), stats(cm))
        rec = _record["step"][f"lock-step {i}"] = _step_ratios(dense, comp, dm, dopt, cm, copt, (loss_o, r_o, g_o, bounds, running), check=False)
        worst = max(rec, key=lambda k: rec[k] / _m_step(k))
        print(f"lock-step {i}: worst ratio {rec[worst]:.2f} ({worst}); instant-interest {rec[II_W]:.2f} / {rec[II_B]:.2f}")
    for i in range(3):
        for k, v in _record["step"][f"lock-step {i}"].items():
            assert v <= _m_step(k), (i, k, v)
    assert copt.steps == 3 and dopt.steps == 3
    torch.cuda.synchronize()


def test_history_and_candidate_groups_together(lib, step_cases):
    """Both flags: the cuts are the history plan's, every group is trimmed in both axes; same gate."""
    from history_compact_util import cut_history
    from news_recommendation_model_amd import synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(64, category_label_num=50)
    batch = cut_history(padded_batch(dims, COUNTS, 37, T_ID, seed=31), [0, 1, 15, 16, 17, 36, 37, 5, 16])
    sd = synth.make_state_dict(dims, seed=1, user_num=int(batch["user_num"]))
    loss_o, r_o, g_o, bounds = oracle_step_with_bounds(sd, batch)
    (dense,), dm, dopt = _spied_step(dims, batch, sd)
    (comp,), cm, copt = _spied_step(dims, batch, sd, compact_candidates=True, compact_history=True, max_groups=3)
    running = {k: dense[3][k].astype(np.float64) for k in dense[3]}      # (the statistics are held to the oracle in the tests above)
    from news_recommendation_model_amd import compact
    hist = compact.plan_history_groups([0, 1, 15, 16, 17, 36, 37, 5, 16], 37, max_groups=3)
    assert not compact.plan_candidate_groups(batch["empty_num"], T_ID, history_plan=hist).dense          # both axes are trimmed
    rec = _record["step"]["history x candidates"] = _step_ratios(dense, comp, dm, dopt, cm, copt, (loss_o, r_o, g_o, bounds, running))
    for k, v in rec.items():
        if not k.startswith("bn.running"):
            assert v <= _m_step(k), (k, v)
    assert rel_err(comp[3]["bn.running_var"], dense[3]["bn.running_var"]) < 1e-5


def test_a_dense_plan_is_bitwise_the_dense_step(lib, step_cases, monkeypatch):
    """Every list full: the plan is dense and the step continues as compact_candidates=False does.  As in test_gpu_history_train.py: four
    dense and four dense-plan steps alternate from the same state; every dense-plan step issues exactly the dense step's native calls with
    the same integer arguments; a tensor (the loss, the logits, every gradient) on which the four dense steps agree bit for bit comes out of
    a dense-plan step with those bits, the others stay within the dense steps' own spread (the loss is summed with one float atomic per
    impression: on the MI355X two DENSE steps were seen one ulp apart)."""
    from news_recommendation_model_amd import native, synth
    dims = step_cases["B9 T7"][0]
    batch = synth.make_batch(dims, 6, H_ID, 5, seed=31)                   # no padded candidates: empty_num = 0
    assert batch["empty_num"].tolist() == [0] * 6
    sd = synth.make_state_dict(dims, seed=1, user_num=int(batch["user_num"]))
    seen, real = [], native.call

    def call(name, *args, tag=None):
        seen.append((name, tag) + tuple(a for a in args if isinstance(a, (int, float))))
        return real(name, *args, tag=tag)
    monkeypatch.setattr(native, "call", call)
    dense, plan_runs, calls = [], [], {}
    for i in range(8):
        del seen[:]
        (res,), model, opt = _spied_step(dims, batch, sd, **(dict(compact_candidates=True, max_groups=4) if i % 2 else {}))
        (plan_runs if i % 2 else dense).append(res)
        calls.setdefault(i % 2, []).append(list(seen))
    assert all(c == calls[0][0] for c in calls[0] + calls[1])
    bitwise = spread = 0
    # the loss is a sum of one float atomic per impression and is held like a gradient tensor; so are the logits
    tensors = [("loss", [np.float32(r[0]).reshape(1) for r in dense], [np.float32(r[0]).reshape(1) for r in plan_runs]),
               ("logits", [r[1].reshape(-1) for r in dense], [r[1].reshape(-1) for r in plan_runs])]
    for (k, p), o in zip(model.named_parameters(), opt.offsets):
        tensors.append((k, [r[2][o:o + p.numel()] for r in dense], [r[2][o:o + p.numel()] for r in plan_runs]))
    for k, d, c in tensors:
        gate = 4 * max([rel_err(x, d[0]) for x in d[1:]] + [4 * FLOOR])         # a few ulps of fp32 atomics at the least
        assert all(rel_err(x, d[0]) <= gate for x in c), k
        if len({x.tobytes() for x in d}) == 1:
            bitwise += 1
            assert any(x.tobytes() == d[0].tobytes() for x in c), k
        else:
            spread += 1
    print(f"gradient tensors: {bitwise} bitwise reproducible over four dense steps (reproduced bit for bit by the dense plan), {spread} not")
    assert bitwise > 0


# ------------------------------------------------------------------------------------------------ housekeeping
def test_refusals_and_fallbacks(lib, step_cases, monkeypatch):
    from news_recommendation_model_amd import native, trainer
    dims, batch, sd, _ = step_cases["B9 T7"]
    model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda").train()
    opt = trainer.FlatAdam(model)
    tb = trainer.batch_to_device(batch, "cuda")
    with pytest.raises(KeyError, match="empty_num"):
        trainer.train_step(model, opt, {k: v for k, v in tb.items() if k != "empty_num"}, compact_candidates=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="stream capture"):
        with torch.cuda.graph(graph):
            trainer.train_step(model, opt, tb, compact_candidates=True)
    with pytest.raises(RuntimeError, match="captured step"):
        trainer.GraphedTrainStep(model, opt, tb, compact_candidates=True)
    torch.cuda.synchronize()
    # models the row-weight head does not take run the dense step: a BatchNorm the column kernels refuse, a non-GELU gate, a hooked sub-model
    seen, real = [], native.call
    monkeypatch.setattr(native, "call", lambda name, *a, tag=None: (seen.append(name), real(name, *a, tag=tag))[1])
    for what in ("bn", "gate", "hook"):
        m = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda").train()
        if what == "bn":
            m.bn = torch.nn.BatchNorm1d(m.bn.num_features, momentum=None).cuda()
        elif what == "gate":
            m.gate.activation = torch.nn.GELU(approximate="tanh")
        else:
            m.invariant_interest_model.register_forward_hook(lambda *a: None)
        assert not m.compact_candidates_applies()
        del seen[:]
        loss, out = trainer.train_step(m, trainer.FlatAdam(m), tb, compact_candidates=True)
        assert "nrm_candidate_gather_groups" not in seen and tuple(out.shape) == (B_ID, T_ID) and np.isfinite(float(loss)), what
    # the prefetcher's host copy is used while empty_num is the tensor it was staged from; a device-only tensor is read back
    monkeypatch.setattr(native, "call", real)
    pf = trainer.BatchPrefetcher([batch], "cuda", empty_num=True)
    for staged, slot in pf:
        host, ptr, version = staged["empty_num_host"]
        assert host.tolist() == batch["empty_num"].tolist() and (ptr, version) == (staged["empty_num"].data_ptr(), staged["empty_num"]._version)
        loss, out = trainer.train_step(model, opt, staged, compact_candidates=True)
        pf.release(slot)
        assert np.isfinite(float(loss))
    # a batch whose empty_num overstates the padding: the gather's check raises at the next compacted step
    lying = dict(tb, empty_num=tb["empty_num"] + 1)
    trainer.train_step(model, opt, lying, compact_candidates=True, max_groups=4)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="padded"):
        trainer.train_step(model, opt, tb, compact_candidates=True, max_groups=4)
    trainer.train_step(model, opt, tb, compact_candidates=True, max_groups=4)      # the flag was cleared
    torch.cuda.synchronize()


def test_opcheck_on_the_new_ops(lib):
    from news_recommendation_model_amd import compact
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)          # noqa: E731
    T = T_ID
    plan = compact.plan_candidate_groups(T - np.asarray(COUNTS), T, max_groups=3)
    tabs = plan.upload("cuda")
    xt, xg, lab = (np.nan_to_num(a) for a in _gather_inputs(np.float64, 12))      # (opcheck compares inputs before and after: no NaN)
    for b, n in enumerate(COUNTS):
        if n < T:
            xt[b, n:], xg[b, n:], lab[b, n:] = xt[b, n], xg[b, n], lab[b, n]
    torch.library.opcheck(torch.ops.nrm.candidate_gather_groups.default,
                          (_dev(xt), _dev(xg), _dev(lab), tabs["perm"], tabs["bounds"], tabs["row_off"], tabs["T_g"], plan.N), test_utils=tests)
    # BatchNorm and the gate block with row weights
    N = plan.N
    w = _dev(np.where(np.arange(N) % 3 == 2, 4.0, 1.0).astype(np.float32))
    n_rows = int(w.sum())
    x = r(N, 24).requires_grad_(True)
    rm, rv = torch.zeros(24, device="cuda"), torch.ones(24, device="cuda")
    torch.library.opcheck(torch.ops.nrm.batch_norm_stats_roww.default, (x.detach(), rm, rv, 0.1, 1e-5, w, n_rows))
    mean, rstd = torch.ops.nrm.batch_norm_stats_roww(x.detach(), rm, rv, 0.1, 1e-5, w, n_rows)
    gamma, beta = r(24).requires_grad_(True), r(24).requires_grad_(True)
    torch.library.opcheck(torch.ops.nrm.batch_norm_apply_roww.default, (x, mean, rstd, gamma, beta, w, n_rows))
    torch.library.opcheck(torch.ops.nrm.batch_norm_bwd_roww.default, (r(N, 24), x.detach(), mean, rstd, gamma.detach(), w, n_rows))
    wg1, bg1 = (0.2 * r(6, 24)).requires_grad_(True), r(6).requires_grad_(True)
    wg2, bg2 = (0.2 * r(24, 6)).requires_grad_(True), r(24).requires_grad_(True)
    torch.library.opcheck(torch.ops.nrm.gate_block_roww_fwd.default, (x, mean, rstd, gamma, beta, wg1, bg1, wg2, bg2, w, n_rows))
    # the grouped loss
    out = r(N).requires_grad_(True)
    delta = (0.1 * r(11)).requires_grad_(True)
    label = torch.zeros(N, device="cuda", dtype=torch.float64)
    uid = torch.arange(B_ID, device="cuda") % 11
    b0, tg = [int(v) for v in plan.bounds], [int(v) for v in plan.T_g]
    torch.library.opcheck(torch.ops.nrm.softmax_bce_loss_grouped.default, (out, delta, label, uid, b0, tg, T, 0.95))
    # the attention + pool node on groups trimmed in both axes (its backward consumes z in place: no AOT dispatch check, as for the others)
    D, H, hg = 16, 9, [3, 9, 9]
    R = sum((b0[i + 1] - b0[i]) * hg[i] for i in range(3))
    args = (r(N, D), r(R, D), 0.1 * r(D, 4 * D), 0.1 * r(D), r(1, D), r(1), b0, hg, tg, H, T, True, 0)
    torch.library.opcheck(torch.ops.nrm.attend_pool_grouped_fwd.default, args, test_utils=tests)
    pooled, s, z = torch.ops.nrm.attend_pool_grouped_fwd(*args)
    torch.library.opcheck(torch.ops.nrm.attend_pool_grouped_bwd.default,
                          (r(N, D), args[0], args[1], args[2], args[4], s, z.detach(), b0, hg, tg, H, T, 0, True, True), test_utils=tests)


def test_train_epochs_returns_the_dense_run(lib, step_cases):
    """Two batches of one epoch, dense and compact, against the float64 oracle's two steps: loss_avg and auc_avg within the step gate."""
    from news_recommendation_model_amd import trainer
    from oracle import user_model_oracle as orc
    dims, batch, sd, _ = step_cases["B32 T15 percentile"]
    p = orc.to_torch_params(sd, dtype=torch.float64)
    tb = {k: torch.from_numpy(v) for k, v in batch.items() if isinstance(v, np.ndarray) and v.ndim > 0}
    state, losses, aucs = {"step": 0, "m": {}, "v": {}}, [], []
    with orc.precision(torch.float64):
        for _ in range(2):
            loss, r, _g = orc.train_step(p, state, tb)
            losses.append(float(loss))
            aucs.append(float(orc.batch_auc(batch["label"], r.numpy()).mean()))
    truth = {"loss_avg": float(np.mean(losses)), "auc_avg": float(np.mean(aucs))}
    runs = []
    for kw in ({}, dict(compact_candidates=True, max_groups=4)):
        model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda").train()
        seen = []
        hist = trainer.train_epochs(model, trainer.FlatAdam(model), lambda: [batch, batch], 1, on_batch=lambda e, i, loss, auc: seen.append(tuple(auc.shape)), **kw)
        assert seen == [(32,), (32,)] and hist[0]["impressions"] == 64
        runs.append(hist[0])
    for k in ("loss_avg", "auc_avg"):
        e, y = (abs(r[k] - truth[k]) / abs(truth[k]) for r in (runs[1], runs[0]))
        _record["step"].setdefault("train_epochs", {})[k] = e / max(y, FLOOR)
        print(f"train_epochs {k}: oracle {truth[k]:.9g}, dense {runs[0][k]:.9g}, compact {runs[1][k]:.9g}")
        assert e <= M_TRAIN_CAND * max(y, FLOOR), (k, runs, truth)
