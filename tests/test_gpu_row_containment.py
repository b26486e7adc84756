"""GPU: a NaN or Inf in one row must stay in that row's outputs.

PyTorch's Linear and the oracle's concat-form attention are row-independent: a non-finite value in one candidate, history row or
upstream-gradient entry can only reach the outputs that depend on that row.  The kernels read whole 16-column K-chunks of
row-major rows, so where the width is not a multiple of 16 the last chunk of a row also reads the first columns of the NEXT row
(or the hidden padding of a caller's view); multiplying those by the zero padding of the packed weights is not enough, since
NaN * 0 and Inf * 0 are NaN.  Every case plants a value, runs the same poisoned inputs through the reference (the CPU oracle,
or float64 PyTorch for the dense ops) and requires, elementwise on every output and input gradient:
  * no non-finite entry where the reference is finite;
  * the same finite pattern the other way round (see _allow_extra_finite for the one exception);
  * the existing tolerances on the entries finite in both.
Weight gradients are legitimately non-finite after most plants; the pattern check covers them, the content is the row gradients."""
import numpy as np
import pytest
import torch

import dense_forms_util as dfu
from attention_budget import FORMS, form_skip_reason
from golden_util import masked_rel_err
from oracle import user_model_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {"f32": (1e-3, 1e-2), "bf16x3": (1e-4, 1e-3), "bf16": (1e-2, 3e-2)}      # (forward, gradient): the gates of test_gpu_attention.py
DENSE_TOL = {"f32": 1e-5, "bf16x3": 1e-4, "bf16": 3e-2}
VALUES = {"nan": float("nan"), "inf": float("inf")}


def _allow_extra_finite(value, gelu):
    # Only where a GELU lies between the plant and the output: a +Inf input entry becomes +-Inf in the pre-activation (its sign
    # follows the weight it meets).  The reference's exact GELU x * Phi(x) is NaN at x = -Inf (-Inf * 0) while a GELU that saturates
    # returns 0 there, so the entries computed from that value may be finite in the kernel and NaN in the reference.  A NaN input has
    # no such freedom (NaN stays NaN everywhere), and neither has an Inf that meets no GELU (weighted_pool, linear without GELU, ...).
    return value == "inf" and gelu


def _check(tag, got, ref, tol, value, gelu=False):
    problems, err = masked_rel_err(got, ref, allow_finite_where_ref_not=_allow_extra_finite(value, gelu))
    assert not problems, (tag, problems)
    assert err < tol, (tag, err)


def _plant_row(arr, idx, value):
    """NaN: the whole row; Inf: its first column (the one a ragged chunk of the previous row reads)."""
    if value == "nan":
        arr[idx] = np.nan
    else:
        arr[idx + (0,)] = np.inf


# ------------------------------------------------------------------------------------------------ attention
def _weights(rng, D):
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    return {"mlp.fc1.weight": rng.uniform(-k1, k1, (D, 4 * D)).astype(np.float32),
            "mlp.fc1.bias": rng.uniform(-k1, k1, (D,)).astype(np.float32),
            "mlp.fc2.weight": rng.uniform(-k2, k2, (1, D)).astype(np.float32),
            "mlp.fc2.bias": rng.uniform(-k2, k2, (1,)).astype(np.float32)}


def _plants(B, T, H):
    """(kind, index) of every planted row: the first and the last row of impression 1, the first row of impression 2, and the rows
    that hold flattened row m = 16 and m = 64 (m = (b T + t) H + h: just after a 16-row and a 64-row tile boundary)."""
    M = B * T * H
    out = [("history", (1, 0)), ("history", (1, H - 1)), ("history", (2, 0)),
           ("target", (1, 0)), ("target", (1, T - 1)), ("target", (2, 0)),
           ("grad", (1, 0, 0)), ("grad", (1, T - 1, H - 1)), ("grad", (2, 0, 0))]
    for m in (16, 64):
        if m < M:
            bt, h = divmod(m, H)
            b, t = divmod(bt, T)
            out += [("history", (b, h)), ("target", (b, t)), ("grad", (b, t, h))]
    return list(dict.fromkeys(out))


_oracle_cache = {}


def _oracle(key, w, tgt, his, gs, pool):
    if key not in _oracle_cache:
        p = {"a." + k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in w.items()}
        t_c = torch.from_numpy(tgt).clone().requires_grad_(True)
        h_c = torch.from_numpy(his).clone().requires_grad_(True)
        s = orc.pointwise_attention_scores(p, "a", t_c, h_c)[..., 0]
        out = torch.einsum("bth,bhd->btd", s, h_c) if pool else s
        (out * torch.from_numpy(gs)).sum().backward()
        ref = {"out": out.detach().numpy(), "target": t_c.grad.numpy(), "history": h_c.grad.numpy()}
        ref.update({k: p["a." + k].grad.numpy() for k in w})
        _oracle_cache[key] = ref
    return _oracle_cache[key]


def _attn_case(entry, mma, B, T, H, D, rowgrads=True):
    """Every plant of _plants x every value through `entry` ('scores' | 'attend_and_pool'), against the oracle."""
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D)
    w = _weights(rng, D)
    tgt0 = rng.standard_normal((B, T, D)).astype(np.float32)
    his0 = rng.standard_normal((B, H, D)).astype(np.float32)
    pool = entry == "attend_and_pool"
    gs0 = rng.standard_normal((B, T, D) if pool else (B, T, H)).astype(np.float32)
    fwd_tol, grad_tol = TOL[mma]
    for value in VALUES:
        for kind, idx in _plants(B, T, H):
            tgt, his, gs = tgt0.copy(), his0.copy(), gs0.copy()
            if kind == "grad":
                if pool:                                 # a dz row comes from one (b, t, h) score: plant in d_pooled[b, t] instead
                    idx = idx[:2]
                _plant_row(gs, idx, value) if pool else gs.__setitem__(idx, VALUES[value])
            else:
                _plant_row(tgt if kind == "target" else his, idx, value)
            ref = _oracle((entry, B, T, H, D, kind, idx, value), w, tgt, his, gs, pool)
            wg = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in w.items()}
            t_g = torch.from_numpy(tgt).cuda().requires_grad_(rowgrads)
            h_g = torch.from_numpy(his).cuda().requires_grad_(rowgrads)
            args = (t_g, h_g, wg["mlp.fc1.weight"], wg["mlp.fc1.bias"], wg["mlp.fc2.weight"], wg["mlp.fc2.bias"])
            out = ops.attend_and_pool(*args, mma=mma) if pool else ops.pointwise_attention_scores(*args, mma=mma)
            (out * torch.from_numpy(gs).cuda()).sum().backward()
            torch.cuda.synchronize()
            tag = (kind, idx, value)
            _check(tag + ("out",), out.detach().cpu().numpy(), ref["out"], fwd_tol, value, gelu=True)
            if rowgrads:
                _check(tag + ("d_target",), t_g.grad.cpu().numpy(), ref["target"], grad_tol, value, gelu=True)
                _check(tag + ("d_history",), h_g.grad.cpu().numpy(), ref["history"], grad_tol, value, gelu=True)
            for k in w:
                _check(tag + (k,), wg[k].grad.cpu().numpy(), ref[k], grad_tol, value, gelu=True)


# (B, T, H, D): B >= 3 (impression 1 has neighbours on both sides); ragged D the dP walk takes (72, 100, 132, 388, 420), exact controls
# (64, 256, 400), D = 66 (padded by the wrapper); H < 16 and H % 16 != 0 (a 16-row fragment spans impressions).  fp32 chunk-streaming
# forward plans (D > 128; D <= 128 takes the resident-W forms): 132 -> 10 tiles, 188 -> 12, 196 -> 13, 256 -> 16, 300 -> 20,
# 388 / 400 -> 2 x 13, 420 -> 2 x 14.  There are no narrower plans (a width of at most 8 tiles takes the resident-W forward, a wider
# one is split into chunks of more than 8 tiles) and no wider one (21..26 tiles are two chunks of 12 or 13).
ATTN_SHAPES = [(3, 3, 20, 72), (3, 2, 17, 100), (3, 2, 18, 132), (3, 2, 17, 388), (3, 2, 16, 420), (3, 2, 20, 64), (3, 2, 16, 256),
               (3, 2, 20, 400), (3, 3, 7, 66), (4, 3, 6, 132), (3, 2, 5, 196), (3, 2, 19, 300), (3, 2, 17, 128), (3, 2, 17, 188)]

# per-launch knobs (read at every launch): forward image / walk forms and every backward form -- the table and its skip rules are
# shared with the error-budget tests (tests/attention_budget.py)
@pytest.mark.parametrize("B,T,H,D", ATTN_SHAPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_attention_f32_keeps_rows_apart(lib, monkeypatch, form, B, T, H, D):
    why = form_skip_reason(form, D, H, lib)
    if why:
        pytest.skip(why)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    _attn_case("scores", "f32", B, T, H, D)


# plain bf16 above D = 256 (no resident-W backward): the serial contraction for dW_p alone from fp32 dz, ragged and exact width
WEIGHT_ONLY_CASES = [(3, 3, 20, 72, "f32"), (3, 2, 17, 388, "f32"), (3, 2, 20, 400, "f32"), (3, 2, 20, 64, "f32"),
                     (3, 2, 17, 388, "bf16"), (3, 2, 20, 320, "bf16")]


@pytest.mark.parametrize("B,T,H,D,mma", WEIGHT_ONLY_CASES, ids=["-".join(map(str, c[:4] if c[4] == "f32" else c)) for c in WEIGHT_ONLY_CASES])
@pytest.mark.parametrize("direct", ["0", "1"])
@pytest.mark.parametrize("interleave", ["0", "1"])
def test_attention_weight_only_backward_keeps_rows_apart(lib, monkeypatch, direct, interleave, B, T, H, D, mma):
    """The text+image attention's backward (no row gradients): the direct dW_p pass and the E-form, both group walks."""
    monkeypatch.setenv("NRM_DW_DIRECT", direct)
    monkeypatch.setenv("NRM_BT_INTERLEAVE", interleave)
    _attn_case("scores", mma, B, T, H, D, rowgrads=False)


@pytest.mark.parametrize("B,T,H,D", [(3, 3, 20, 72), (3, 2, 20, 64), (3, 2, 17, 128), (3, 2, 16, 256), (3, 2, 17, 388), (3, 2, 20, 400),
                                     (3, 3, 7, 66), (4, 3, 6, 132)])
@pytest.mark.parametrize("mma", ["bf16x3", "bf16"])
def test_attention_bf16_keeps_rows_apart(lib, monkeypatch, mma, B, T, H, D):
    """Resident-W forward (walk at D = 64 / 128 / 256, tile form elsewhere) and the bf16 resident-W backward."""
    _attn_case("scores", mma, B, T, H, D)


@pytest.mark.parametrize("B,T,H,D", [(3, 3, 20, 72), (3, 2, 17, 388), (3, 2, 20, 400), (3, 3, 7, 66)])
@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
def test_attend_and_pool_keeps_rows_apart(lib, mma, B, T, H, D):
    _attn_case("attend_and_pool", mma, B, T, H, D)


@pytest.mark.parametrize("B,T,H,D", [(3, 3, 20, 72), (3, 2, 17, 400), (3, 3, 7, 66)])
def test_weighted_pool_keeps_rows_apart(lib, B, T, H, D):
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(B + T + H + D)
    s0 = rng.standard_normal((B, T, H)).astype(np.float32)
    h0 = rng.standard_normal((B, H, D)).astype(np.float32)
    g0 = rng.standard_normal((B, T, D)).astype(np.float32)
    for value in VALUES:
        for kind, idx in [("history", (1, 0)), ("history", (1, H - 1)), ("scores", (1, 0)), ("scores", (2, T - 1)), ("grad", (1, 0))]:
            s, h, g = s0.copy(), h0.copy(), g0.copy()
            _plant_row({"history": h, "scores": s, "grad": g}[kind], idx, value)
            sr, hr = (torch.from_numpy(a).double().requires_grad_(True) for a in (s, h))
            out_r = torch.einsum("bth,bhd->btd", sr, hr)
            (out_r * torch.from_numpy(g).double()).sum().backward()
            sg, hg = (torch.from_numpy(a).cuda().requires_grad_(True) for a in (s, h))
            out = ops.weighted_pool(sg, hg)
            (out * torch.from_numpy(g).cuda()).sum().backward()
            tag = (kind, idx, value)
            _check(tag + ("out",), out.detach().cpu().numpy(), out_r.detach().numpy(), 1e-5, value)
            _check(tag + ("d_scores",), sg.grad.cpu().numpy(), sr.grad.numpy(), 1e-5, value)
            _check(tag + ("d_history",), hg.grad.cpu().numpy(), hr.grad.numpy(), 1e-5, value)


# ------------------------------------------------------------------------------------------------ dense layers
# production widths {402, 1608, 1032, 258, 66, 264} and K % 16 in {4, 8, 12}; M small but over several 64-row blocks
DENSE_SHAPES = [(150, 402, 1608), (150, 1608, 402), (150, 1032, 258), (150, 258, 1032), (150, 66, 264), (150, 264, 66),
                (150, 100, 40), (150, 72, 24), (150, 140, 12)]


def _dense_rows(M):
    return [0, 15, 16, 63, 64, M - 1]


@pytest.mark.parametrize("M,K,N", DENSE_SHAPES)
@pytest.mark.parametrize("mma", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("gelu", [False, True])
def test_linear_keeps_rows_apart(lib, mma, gelu, M, K, N):
    from news_recommendation_model_amd import ops
    g = torch.Generator(device="cpu").manual_seed(M + K + N)
    x0 = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    gy0 = torch.randn(M, N, generator=g)
    tol = DENSE_TOL[mma]
    ops.set_dense_arithmetic(mma)
    try:
        for value in VALUES:
            for where in ("x", "dy"):
                for r in _dense_rows(M):
                    x, gy = x0.clone().numpy(), gy0.clone().numpy()
                    _plant_row(x if where == "x" else gy, (r,), value)
                    xr = torch.from_numpy(x).double().requires_grad_(True)
                    y_ref = torch.nn.functional.linear(xr, w.double(), b.double())
                    if gelu:
                        y_ref = torch.nn.functional.gelu(y_ref)
                    y_ref.backward(torch.from_numpy(gy).double())
                    xg = torch.from_numpy(x).cuda().requires_grad_(True)
                    y = ops.linear(xg, w.cuda(), b.cuda(), gelu=gelu)
                    y.backward(torch.from_numpy(gy).cuda())
                    tag = (where, r, value)
                    _check(tag + ("y",), y.detach().cpu().numpy(), y_ref.detach().numpy(), tol, value, gelu=gelu)
                    _check(tag + ("dx",), xg.grad.cpu().numpy(), xr.grad.numpy(), tol, value, gelu=gelu)
    finally:
        ops.set_dense_arithmetic(None)


@pytest.mark.parametrize("mma,M,K,N", dfu.CONTAINMENT_CASES, ids=["-".join(map(str, c)) for c in dfu.CONTAINMENT_CASES])
def test_linear_keeps_rows_apart_in_the_multi_tile_forms(lib, monkeypatch, mma, M, K, N):
    """The forms in which a wave owns several interleaved 16-row tiles (fp32 gemm_nt_kernel<NT, MT > 1>: 64 * MT rows per workgroup,
    taken only by grids of 512 or more workgroups) or a workgroup holds 64 / 128 resident rows (gemm_nt_rx_kernel<RT = 4 | 8>): NaN
    rows planted all at once around the tile and block boundaries -- 0, 15, 16, BM - 1, BM, M - 1, BM the block height of the form the
    launch takes (nrm_gemm_nt_form) -- first in x, checked on y, then in dy, checked on dx; GELU on.  The non-finite output rows must
    be exactly the planted ones and every other row must hold the float64 value."""
    from news_recommendation_model_amd import ops
    for k in dfu.KNOBS:
        monkeypatch.delenv(k, raising=False)
    code = dfu.MMA_BY_NAME[mma]
    fwd, bwd = dfu.dense_form(lib, M, N, K, code), dfu.dense_form(lib, M, K, N, code)      # y = x W^T; dx = dy' W
    # several row tiles in the forward launch (the 42-wide dX of the fp32 cases is a narrower grid: whatever form it takes, its block
    # height places the rows), in the arithmetic asked for
    assert fwd[2] > 1 and all((form[0] == "nt") == (mma == "f32") for form in (fwd, bwd)), (fwd, bwd)
    g = torch.Generator(device="cpu").manual_seed(M + K + N)
    x0 = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    gy0 = torch.randn(M, N, generator=g)
    tol = DENSE_TOL[mma]
    ops.set_dense_arithmetic(mma)
    try:
        for where, form in (("x", fwd), ("dy", bwd)):
            BM = dfu.block_rows(form)
            rows = sorted({0, 15, 16, BM - 1, BM, M - 1})
            x, gy = x0.clone().numpy(), gy0.clone().numpy()
            for r in rows:
                _plant_row(x if where == "x" else gy, (r,), "nan")
            xr = torch.from_numpy(x).double().requires_grad_(where == "dy")
            y_ref = torch.nn.functional.gelu(torch.nn.functional.linear(xr, w.double(), b.double()))
            xg = torch.from_numpy(x).cuda().requires_grad_(where == "dy")
            if where == "x":
                with torch.no_grad():
                    got, ref = ops.linear(xg, w.cuda(), b.cuda(), gelu=True).cpu().numpy(), y_ref.detach().numpy()
            else:
                y_ref.backward(torch.from_numpy(gy).double())
                ops.linear(xg, w.cuda(), b.cuda(), gelu=True).backward(torch.from_numpy(gy).cuda())
                got, ref = xg.grad.cpu().numpy(), xr.grad.numpy()
            bad_rows = np.flatnonzero(~np.isfinite(got).all(axis=1)).tolist()
            assert bad_rows == rows, (where, form, bad_rows)
            assert not np.isfinite(got[rows]).any(), (where, form)
            _check((where, form), got, ref, tol, "nan", gelu=True)
    finally:
        ops.set_dense_arithmetic(None)


@pytest.mark.parametrize("M,K,Hd,N", [(150, 1608, 402, 1608), (150, 264, 66, 264), (150, 258, 1032, 258), (150, 100, 72, 44)])
@pytest.mark.parametrize("mma", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("mul", [False, True])
def test_mlp_gelu_keeps_rows_apart(lib, mma, mul, M, K, Hd, N):
    from news_recommendation_model_amd import ops
    g = torch.Generator(device="cpu").manual_seed(M + 3 * K + 5 * Hd + 7 * N)
    x0 = torch.randn(M, K, generator=g)
    w1 = torch.randn(Hd, K, generator=g) / np.sqrt(K)
    b1 = torch.randn(Hd, generator=g) * 0.1
    w2 = torch.randn(N, Hd, generator=g) / np.sqrt(Hd)
    b2 = torch.randn(N, generator=g) * 0.1
    m0 = torch.randn(M, N, generator=g)
    gy0 = torch.randn(M, N, generator=g)
    tol = DENSE_TOL[mma]
    ops.set_dense_arithmetic(mma)
    try:
        for value in VALUES:
            for where in ("x", "dy"):
                for r in _dense_rows(M):
                    x, gy = x0.clone().numpy(), gy0.clone().numpy()
                    _plant_row(x if where == "x" else gy, (r,), value)
                    xr = torch.from_numpy(x).double().requires_grad_(True)
                    y_ref = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(xr, w1.double(), b1.double())),
                                                       w2.double(), b2.double())
                    if mul:
                        y_ref = y_ref * m0.double()
                    y_ref.backward(torch.from_numpy(gy).double())
                    xg = torch.from_numpy(x).cuda().requires_grad_(True)
                    y = ops.mlp_gelu(xg, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), mul=m0.cuda() if mul else None)
                    y.backward(torch.from_numpy(gy).cuda())
                    tag = (where, r, value)
                    _check(tag + ("y",), y.detach().cpu().numpy(), y_ref.detach().numpy(), tol, value, gelu=True)
                    _check(tag + ("dx",), xg.grad.cpu().numpy(), xr.grad.numpy(), tol, value, gelu=True)
    finally:
        ops.set_dense_arithmetic(None)


# ------------------------------------------------------------------------------------------------ padding views
@pytest.mark.parametrize("K,N", [(402, 1608), (258, 1032), (66, 264), (100, 40), (264, 66)])
@pytest.mark.parametrize("extra", ["pad4", "plus12"])
@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
def test_padding_views_with_nan_give_contiguous_results(lib, mma, extra, K, N):
    """x = buf[:, :K] whose hidden columns are NaN (row stride pad4(K) or K + 12) must give what the same data gives contiguous:
    linear (+GELU), mlp_gelu, gate_block, eval batch_norm and concat_last, forward and input gradient."""
    from news_recommendation_model_amd import ops
    M = 150
    g = torch.Generator(device="cpu").manual_seed(K * 3 + N)
    x = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / np.sqrt(K)).cuda()
    b = (torch.randn(N, generator=g) * 0.1).cuda()
    w2 = (torch.randn(K, N, generator=g) / np.sqrt(N)).cuda()
    b2 = (torch.randn(K, generator=g) * 0.1).cuda()
    gy = torch.randn(M, N, generator=g).cuda()
    gz = torch.randn(M, K, generator=g).cuda()
    ld = (K + 3) // 4 * 4 if extra == "pad4" else K + 12
    buf = torch.full((M, ld), float("nan"), device="cuda")
    buf[:, :K] = x
    ops.set_dense_arithmetic(mma)
    try:
        bn = _eval_bn(K, g)
        res = {}
        for name, xin in (("view", buf[:, :K]), ("contiguous", x.clone())):
            xin = xin.detach().requires_grad_(True)
            y = ops.linear(xin, w, b, gelu=True)
            z = ops.mlp_gelu(xin, w, b, w2, b2)
            gb = ops.gate_block(xin, bn, w, b, w2, b2)
            nb = ops.batch_norm(xin, bn)
            cat = ops.concat_last([xin, y])
            (y * gy).sum().backward(retain_graph=True)
            (z * gz).sum().backward()
            ((gb + nb) * gz).sum().backward()
            cat.sum().backward()
            res[name] = [y.detach(), z.detach(), gb.detach(), nb.detach(), cat.detach(), xin.grad]
        torch.cuda.synchronize()
        # the same data in both runs; some of these paths reduce with float atomics, so the comparison allows their run-to-run
        # spread -- a leak of the hidden NaN shows as a non-finite entry
        for i, (a, r) in enumerate(zip(res["view"], res["contiguous"])):
            assert bool(torch.isfinite(a).all()), i
            assert float((a - r).abs().max() / r.abs().max()) < 1e-5, i
    finally:
        ops.set_dense_arithmetic(None)


def _eval_bn(K, g):
    bn = torch.nn.BatchNorm1d(K).cuda().eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(K, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(K, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(K, generator=g) * 0.1)
    return bn


@pytest.mark.parametrize("B,T,H,D", [(3, 3, 20, 72), (3, 2, 17, 400), (3, 3, 7, 66)])
@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
def test_attention_padding_views_with_nan_give_contiguous_results(lib, mma, B, T, H, D):
    """target / history as views t[..., :D] of buffers whose hidden columns are NaN (row stride pad4(D) and D + 12):
    pointwise_attention_scores, attend_and_pool and weighted_pool must return what the same data gives contiguous."""
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(B + T + H + D)
    w = {k: torch.from_numpy(v).cuda() for k, v in _weights(rng, D).items()}
    tgt = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).cuda()
    his = torch.from_numpy(rng.standard_normal((B, H, D)).astype(np.float32)).cuda()
    sc = torch.from_numpy(rng.standard_normal((B, T, H)).astype(np.float32)).cuda()
    for ld in ((D + 3) // 4 * 4, D + 12):
        def view(a):
            buf = torch.full(a.shape[:-1] + (ld,), float("nan"), device="cuda")
            buf[..., :D] = a
            return buf[..., :D]
        res = {}
        for name, (t_in, h_in) in (("view", (view(tgt), view(his))), ("contiguous", (tgt.clone(), his.clone()))):
            t_in, h_in = t_in.detach().requires_grad_(True), h_in.detach().requires_grad_(True)
            args = (t_in, h_in, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"], w["mlp.fc2.bias"])
            s = ops.pointwise_attention_scores(*args, mma=mma)
            pooled = ops.attend_and_pool(*args, mma=mma)
            wp = ops.weighted_pool(sc, h_in)
            (s.sum() + pooled.sum() + wp.sum()).backward()
            res[name] = [s.detach(), pooled.detach(), wp.detach(), t_in.grad, h_in.grad]
        torch.cuda.synchronize()
        # the same data in both runs; scores and gradients may go through float-atomic reductions (resident-W forward of bf16x3,
        # the backward's row gradients), so the comparison allows their run-to-run spread -- a leak shows as a non-finite entry
        for i, (a, r) in enumerate(zip(res["view"], res["contiguous"])):
            assert bool(torch.isfinite(a).all()), (ld, i)
            assert float((a - r).abs().max() / r.abs().max()) < 1e-5, (ld, i)


# ------------------------------------------------------------------------------------------------ the other dense ops
@pytest.mark.parametrize("M,K,Hd", [(150, 1608, 402), (150, 264, 66), (150, 100, 28)])
@pytest.mark.parametrize("mma", ["f32", "bf16x3", "bf16"])
def test_gate_block_and_eval_batch_norm_keep_rows_apart(lib, mma, M, K, Hd):
    """gate(bn(x)) * x and bn(x) with BatchNorm in eval mode (running statistics): row-independent, against float64 torch."""
    from news_recommendation_model_amd import ops
    F = torch.nn.functional
    g = torch.Generator(device="cpu").manual_seed(M + K + Hd)
    x0 = torch.randn(M, K, generator=g)
    w1 = torch.randn(Hd, K, generator=g) / np.sqrt(K)
    b1 = torch.randn(Hd, generator=g) * 0.1
    w2 = torch.randn(K, Hd, generator=g) / np.sqrt(Hd)
    b2 = torch.randn(K, generator=g) * 0.1
    gy0 = torch.randn(M, K, generator=g)
    bn = _eval_bn(K, g)
    bnd = [t.detach().cpu().double() for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias)]
    tol = DENSE_TOL[mma]
    ops.set_dense_arithmetic(mma)
    try:
        for value in VALUES:
            for where in ("x", "dy"):
                for r in _dense_rows(M):
                    x, gy = x0.clone().numpy(), gy0.clone().numpy()
                    _plant_row(x if where == "x" else gy, (r,), value)
                    for op in ("gate_block", "batch_norm"):
                        xr = torch.from_numpy(x).double().requires_grad_(True)
                        nr = F.batch_norm(xr, bnd[0], bnd[1], bnd[2], bnd[3], False, 0.0, bn.eps)
                        y_ref = F.linear(F.gelu(F.linear(nr, w1.double(), b1.double())), w2.double(), b2.double()) * xr \
                            if op == "gate_block" else nr
                        y_ref.backward(torch.from_numpy(gy).double())
                        xg = torch.from_numpy(x).cuda().requires_grad_(True)
                        y = ops.gate_block(xg, bn, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda()) if op == "gate_block" \
                            else ops.batch_norm(xg, bn)
                        y.backward(torch.from_numpy(gy).cuda())
                        tag = (op, where, r, value)
                        gelu = op == "gate_block"
                        # (batch_norm is elementwise: fp32 against float64, whatever the dense arithmetic)
                        t_op = tol if gelu else 1e-5
                        _check(tag + ("y",), y.detach().cpu().numpy(), y_ref.detach().numpy(), t_op, value, gelu=gelu)
                        _check(tag + ("dx",), xg.grad.cpu().numpy(), xr.grad.numpy(), t_op, value, gelu=gelu)
    finally:
        ops.set_dense_arithmetic(None)


@pytest.mark.parametrize("R,K,N", [(150, 3, 8), (150, 4, 5), (70, 1, 8)])
def test_small_linear_relu_keeps_rows_apart(lib, R, K, N):
    from news_recommendation_model_amd import ops
    g = torch.Generator(device="cpu").manual_seed(R + K + N)
    x0 = torch.randn(R, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g) * 0.1
    for value in VALUES:
        for r in _dense_rows(R):
            x = x0.clone().numpy()
            _plant_row(x, (r,), value)
            y_ref = torch.relu(torch.nn.functional.linear(torch.from_numpy(x).double(), w.double(), b.double()))
            y = ops.small_linear_relu(torch.from_numpy(x).cuda(), w.cuda(), b.cuda())
            _check(("x", r, value, "y"), y.cpu().numpy(), y_ref.numpy(), 1e-5, value)


@pytest.mark.parametrize("widths", [(402, 1608), (66, 258, 1032), (264, 12, 6), (100, 3)])
def test_concat_last_keeps_rows_apart(lib, widths):
    from news_recommendation_model_amd import ops
    g = torch.Generator(device="cpu").manual_seed(sum(widths))
    M = 150
    parts0 = [torch.randn(M, w, generator=g) for w in widths]
    gy0 = torch.randn(M, sum(widths), generator=g)
    for value in VALUES:
        for which in ("part", "dy"):
            for r in _dense_rows(M):
                parts = [p.clone().numpy() for p in parts0]
                gy = gy0.clone().numpy()
                _plant_row(parts[len(parts) - 1] if which == "part" else gy, (r,), value)
                pr = [torch.from_numpy(p).double().requires_grad_(True) for p in parts]
                y_ref = torch.cat(pr, dim=-1)
                y_ref.backward(torch.from_numpy(gy).double())
                pg = [torch.from_numpy(p).cuda().requires_grad_(True) for p in parts]
                y = ops.concat_last(pg)
                y.backward(torch.from_numpy(gy).cuda())
                tag = (which, r, value)
                _check(tag + ("y",), y.detach().cpu().numpy(), y_ref.detach().numpy(), 1e-12, value)
                for i, (a, b) in enumerate(zip(pg, pr)):
                    _check(tag + ("d_part", i), a.grad.cpu().numpy(), b.grad.numpy(), 1e-12, value)


@pytest.mark.parametrize("emb", [64, 256])
def test_frontend_keeps_rows_apart(lib, emb):
    """A NaN in one row's float feature (a PCA entry, the sentiment value, scroll / read time) reaches that row's outputs only:
    every other row's label and text/image rows equal the clean run bit for bit."""
    from news_recommendation_model_amd import ops, synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(emb, category_label_num=50)
    batch = synth.make_batch(dims, 4, 20, 5, seed=7)
    sd = synth.make_state_dict(dims, seed=8, user_num=int(batch["user_num"]))
    pre = "invariant_interest_model."
    names = ("category_embedding.0.weight", "sentiment_embedding.0.weight", "sentiment_embedding.0.bias", "type_embedding.0.weight",
             "year_embedding.0.weight", "month_embedding.0.weight", "day_embedding.0.weight", "hour_embedding.0.weight")
    tabs = [torch.from_numpy(np.asarray(sd[pre + n], dtype=np.float32)).cuda() for n in names]
    for key, behaviour in (("x_history", True), ("x_target", False)):
        x = torch.from_numpy(batch[key]).cuda()
        lab0, ti0 = ops.frontend(x, behaviour, dims.n_subcat, dims.pca_vector, *tabs)
        ncol = x.shape[-1]
        c_sent = 4 + dims.pca_vector + 1 + dims.n_subcat
        cols = [4, 4 + dims.pca_vector - 1, c_sent, c_sent + dims.n_sentiment - 1] + ([ncol - 2, ncol - 1] if behaviour else [])
        for col in cols:
            for b, n in ((1, 0), (1, x.shape[1] - 1), (2, 0)):
                xb = x.clone()
                xb[b, n, col] = float("nan")
                lab, ti = ops.frontend(xb, behaviour, dims.n_subcat, dims.pca_vector, *tabs)
                keep = torch.ones(x.shape[:2], dtype=torch.bool, device="cuda")
                keep[b, n] = False
                assert torch.equal(lab[keep], lab0[keep]), (key, col, b, n)
                assert torch.equal(ti[keep], ti0[keep]), (key, col, b, n)


def test_softmax_bce_loss_keeps_rows_apart(lib):
    """Per-row logit gradient: a NaN / Inf logit in impression b makes the (mean) loss non-finite, but the gradient of every other
    impression's logits depends on that impression alone (against the oracle's gradient, the gate of test_gpu_model.py)."""
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(11)
    for B, T in ((5, 7), (4, 100)):
        out0 = rng.standard_normal((B, T)).astype(np.float32)
        label = np.zeros((B, T), dtype=np.float64)
        label[np.arange(B), rng.integers(0, T, B)] = 1
        uid = rng.integers(0, 9, B)
        delta = (rng.standard_normal(9) * 0.3).astype(np.float32)
        # the oracle's BCE refuses non-finite probabilities, so the reference is derived: the mean's gradient with respect to row b'
        # is that row's own term over B T, the same as in the clean batch; row b is NaN (a softmax over a row holding NaN, or +Inf:
        # exp(Inf - Inf), is NaN throughout)
        o_c = torch.from_numpy(out0).requires_grad_(True)
        d_c = torch.from_numpy(delta).requires_grad_(True)
        orc.user_model_loss({"delta": d_c}, torch.from_numpy(uid), o_c, torch.from_numpy(label)).backward()
        for value in VALUES:
            for b, t in ((1, 0), (1, T - 1), (2, 0)):
                out = out0.copy()
                out[b, t] = VALUES[value]
                ref = o_c.grad.numpy().copy()
                ref[b] = np.nan
                o_g = torch.from_numpy(out).cuda().requires_grad_(True)
                d_g = torch.from_numpy(delta).cuda().requires_grad_(True)
                ops.softmax_bce_loss(o_g, d_g, torch.from_numpy(label).cuda(), torch.from_numpy(uid).cuda(), 0.95).backward()
                _check((b, t, value, "d_out"), o_g.grad.cpu().numpy(), ref, 1e-4, value)


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
@pytest.mark.parametrize("emb,H,T", [(64, 20, 6), (256, 32, 6)])
def test_nan_history_feature_stays_in_its_impression(lib, mma, emb, H, T):
    """Eval mode: BatchNorm uses running statistics, so an impression's scores depend on that impression alone.  A NaN in one
    history row of impression 1 must leave every other impression's eval forward and predict() scores exactly as they were."""
    from news_recommendation_model_amd import evaluation, ops, synth, trainer
    from news_recommendation_model_amd.config import Dims
    B = 5
    dims = Dims.for_emb(emb, category_label_num=50)
    batch = synth.make_batch(dims, B, H, T, seed=3)
    sd = synth.make_state_dict(dims, seed=4, user_num=int(batch["user_num"]))
    ops.set_dense_arithmetic(mma)
    try:
        model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda:0", attention_mma=mma).eval()
        tb = trainer.batch_to_device(batch, "cuda:0")
        others = [b for b in range(B) if b != 1]
        with torch.no_grad():
            clean = model(tb["x_history"], tb["x_target"], tb["x_global"]).clone()
            clean_p, _ = evaluation.predict([model], tb)
            clean_p = clean_p.clone()
            assert bool(torch.isfinite(clean).all())
            ncol = tb["x_history"].shape[-1]
            # float features only (ids index tables): a PCA entry, the last PCA entry, the two behaviour values (scroll, read time)
            for col in (4, 4 + dims.pca_vector - 1, ncol - 2, ncol - 1):
                xh = tb["x_history"].clone()
                for h in (0, H - 1):
                    xh[1, h, col] = float("nan")
                bad = dict(tb, x_history=xh)
                out = model(bad["x_history"], bad["x_target"], bad["x_global"])
                p, _ = evaluation.predict([model], bad)
                assert torch.equal(out[others], clean[others]), (col, float((out[others] - clean[others]).abs().max()))
                assert torch.equal(p[others], clean_p[others]), col
    finally:
        ops.set_dense_arithmetic(None)


# ------------------------------------------------------------------------------------------------ uninitialised memory
def _fill_allocator(value, nbytes):
    """Return blocks of assorted sizes, about `nbytes` in all, to the caching allocator holding `value`: what a later torch.empty
    (every kernel output, with its pad4 columns) is then handed."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    sizes = [1 << 12, 3 << 14, 1 << 16, 5 << 16, 1 << 19, 3 << 19, 1 << 21, 3 << 21]
    held, total, i = [], 0, 0
    while total < nbytes:
        n = sizes[i % len(sizes)]
        held.append(torch.full((n // 4,), value, dtype=torch.float32, device="cuda"))
        total += n
        i += 1
    torch.cuda.synchronize()
    del held


def _model_run(dims, sd, batch, mma, fill, nbytes):
    """eval forward, predict() and one eager train step of a fresh model, each after the allocator was filled with `fill`."""
    from news_recommendation_model_amd import evaluation, ops, trainer
    ops.invalidate_packed_weights()
    model = trainer.build_model(dims, int(batch["user_num"]), sd, device="cuda:0", attention_mma=mma).eval()
    tb = trainer.batch_to_device(batch, "cuda:0")
    res = {}
    with torch.no_grad():
        _fill_allocator(fill, nbytes)
        res["forward"] = model(tb["x_history"], tb["x_target"], tb["x_global"]).clone()
        _fill_allocator(fill, nbytes)
        res["predict"] = evaluation.predict([model], tb)[0].clone()
    model.train()
    opt = trainer.make_optimizer(model)
    _fill_allocator(fill, nbytes)
    loss, out = trainer.train_step(model, opt, tb)
    torch.cuda.synchronize()
    res["loss"], res["train_out"] = loss.reshape(1).clone(), out.clone()
    res["params"] = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    return res


@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
@pytest.mark.parametrize("emb,B,H,T", [(64, 8, 40, 15), (256, 8, 32, 30)])       # reference-default-like, C2-like
def test_nan_filled_allocator_changes_nothing(lib, mma, emb, B, H, T):
    """Every intermediate is a torch.empty buffer; its padding columns hold whatever the caching allocator had there.  With the
    allocator filled with NaN before each run, the eval forward, predict() and an eager train step must be finite and equal to
    the same runs after a fill with zeros: bit for bit where the path has no float atomics (eval in fp32), otherwise within the
    run-to-run spread of the atomic reductions."""
    from news_recommendation_model_amd import ops, synth
    from news_recommendation_model_amd.config import Dims
    dims = Dims.for_emb(emb, category_label_num=50)
    batch = synth.make_batch(dims, B, H, T, seed=5)
    sd = synth.make_state_dict(dims, seed=6, user_num=int(batch["user_num"]))
    ops.set_dense_arithmetic(mma)
    try:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        _model_run(dims, sd, batch, mma, 0.0, 0)
        nbytes = 2 * torch.cuda.max_memory_allocated()
        zero = _model_run(dims, sd, batch, mma, 0.0, nbytes)
        nan = _model_run(dims, sd, batch, mma, float("nan"), nbytes)
    finally:
        ops.set_dense_arithmetic(None)
    for k in zero:
        assert bool(torch.isfinite(nan[k]).all()), k
        if mma == "f32" and k in ("forward", "predict"):
            assert torch.equal(nan[k], zero[k]), (k, float((nan[k] - zero[k]).abs().max()))
        else:
            err = float((nan[k] - zero[k]).abs().max() / (zero[k].abs().max() + 1e-30))
            assert err < 1e-5, (k, err)
