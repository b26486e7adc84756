"""GPU: the head's column kernels (head.hip) through their C entries -- nrm_colreduce, nrm_bn_finalize, nrm_bn_apply, nrm_bn_backward,
nrm_mul_bwd, nrm_concat_cols -- element by element against the float64 statements of head_columns_util, each entry judged on what it
was given (the chain feeds every entry the previous entry's fp32 result).  The bounds are derived in head_columns_util's docstring from
the kernels' operations; tests/test_head_columns_cpu.py shows that this very check rejects ten one-line mutants of the kernels.  Cases:
R in 1 .. 513 around blockDim.y = 8 and 256 rows per block, N in 4 .. 264 around the 128-column slab, ld = N and N + 4, three input
families, the sums also onto non-zero content, one case that sends the elementwise kernels round their grid-stride loop a second time,
the finalisation at R up to 30720 with and without running statistics, and the concatenation's vector and scalar paths.  Every output
carries sentinels behind its rows and columns.  ops.batch_norm and ops.gate_block run on a column slice of a wider matrix (ld > N) and
are judged per column against float64 nn.BatchNorm1d with the chained bounds.

No test of this file creates a stream or captures a graph.  Set NRM_HEAD_POOL_RECORD=<path> to merge the worst error / bound per entry
into a JSON file (profiles/head_pool_bounds.json is such a record; no gate is derived from it)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_columns_util as hu  # noqa: E402
from news_recommendation_model_amd import native  # noqa: E402

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("NRM_HEAD_POOL_RECORD")
    if path:
        data = {}
        if os.path.exists(path):
            with open(path) as f:
                data = json.load(f)
        data["head_columns"] = {k: round(WORST[k], 4) for k in sorted(WORST)}
        with open(path, "w") as f:
            json.dump(data, f, indent=1)


def _p(t):
    return native.ptr(t) if t is not None else None


class Native:
    """head_columns_util's backend over the C ABI: numpy in, numpy out; every tensor lives until the call has been waited for"""

    def _d(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def _run(self, name, *args):
        native.call(name, *args, native.stream_ptr())
        torch.cuda.synchronize()

    def colreduce(self, mode, x, dy, mean, rstd, s0, s1, R, N, ld):
        t = [self._d(a) for a in (x, dy, mean, rstd, s0, s1)]
        self._run("nrm_colreduce", mode, *[_p(a) for a in t], R, N, ld)
        return t[4].cpu().numpy(), None if s1 is None else t[5].cpu().numpy()

    def finalize(self, stage, s, out, running, R, N, momentum, eps):
        t = [self._d(a) for a in (s, out, running)]
        self._run("nrm_bn_finalize", stage, *[_p(a) for a in t], R, N, momentum, eps)
        return t[1].cpu().numpy(), None if running is None else t[2].cpu().numpy()

    def apply(self, x, mean, rstd, gamma, beta, y, R, N, ld):
        t = [self._d(a) for a in (x, mean, rstd, gamma, beta, y)]
        self._run("nrm_bn_apply", *[_p(a) for a in t], R, N, ld)
        return t[5].cpu().numpy()

    def backward(self, x, dy, mean, rstd, gamma, s0, s1, add, dx, R, N, ld, training):
        t = [self._d(a) for a in (x, dy, mean, rstd, gamma, s0, s1, add, dx)]
        self._run("nrm_bn_backward", *[_p(a) for a in t], R, N, ld, training)
        return t[8].cpu().numpy()

    def mul_bwd(self, dy, lddy, g, ldg, e, lde, dg, de, ldo, R, N):
        t = [self._d(a) for a in (dy, g, e, dg, de)]
        self._run("nrm_mul_bwd", _p(t[0]), lddy, _p(t[1]), ldg, _p(t[2]), lde, _p(t[3]), _p(t[4]), ldo, R, N)
        return t[3].cpu().numpy(), t[4].cpu().numpy()

    def concat(self, parts, out, ldo, R):
        n = len(parts)
        bufs = [self._d(p["buf"]) for p in parts]
        o = self._d(out)
        srcs = (ctypes.c_void_p * n)(*[b.data_ptr() + 4 * p["off"] for b, p in zip(bufs, parts)])
        lds = (ctypes.c_long * n)(*[p["ld"] for p in parts])
        widths = (ctypes.c_int * n)(*[p["width"] for p in parts])
        self._run("nrm_concat_cols", srcs, lds, widths, n, _p(o), ldo, R)
        return o.cpu().numpy()


def _hold(tag, res):
    for k, v in res.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(tag, {k: round(v, 3) for k, v in res.items()})
    for k, v in res.items():
        assert v <= 1.0, (tag, k, v)


ALL_ENTRIES = set(hu.SUMS + hu.SUMS_PRIOR + hu.ELEMENTWISE + ("finalize0.mean", "finalize0.running", "finalize1.rstd", "finalize1.running"))


@pytest.mark.parametrize("family", hu.FAMILIES)
@pytest.mark.parametrize("N", hu.COLS)
def test_column_kernels_per_element(lib, N, family):
    """every R and both leading dimensions at this width and family: every entry, per element"""
    be = Native()
    for R in hu.ROWS:
        for extra in hu.LD_EXTRA:
            res = hu.check_case(be, hu.make_case(R, N, N + extra, family))
            assert set(res) == ALL_ENTRIES
            _hold((R, N, N + extra, family), res)


def test_second_trip_of_the_grid_stride_loops(lib):
    """R N / 4 = 1 053 700 float4s against the 4096 x 256 threads ew_blocks allows: bn_apply, bn_backward and mul_bwd take a second trip"""
    R, N = hu.SECOND_TRIP
    assert R * (N // 4) > hu.EW_MAX_THREADS
    res = hu.check_case(Native(), hu.make_case(R, N, N + 4, "b"), elementwise_only=True)
    assert set(res) == set(hu.ELEMENTWISE)
    _hold(("second trip", R, N), res)


def test_finalize_per_element(lib):
    """R in 1 .. 30720, N around one block of 256 threads, running statistics present and null, momentum 0.1 and 1"""
    be = Native()
    for R, N, running, m in hu.finalize_cases():
        res = hu.check_finalize(be, R, N, running, m)
        assert len(res) == (4 if running else 2)
        _hold(("finalize", R, N, running, m), res)


def test_concat_cols_is_a_bitwise_copy(lib):
    """1, 3 and 8 parts; the float4 path (every width, leading dimension and base a multiple of 4 floats), and the scalar path by a
    width of 3, by a source 4 bytes off alignment, and with leading dimensions above the widths"""
    be = Native()
    for name, spec in hu.CONCAT_SPECS.items():
        for R in hu.CONCAT_ROWS:
            for extra in (0, 4):
                _hold(("concat", name, R, extra), hu.check_concat(be, spec, R, extra))


# ------------------------------------------------------------------------------------------------ the ops on a column slice
SLICE_R, SLICE_N, SLICE_WIDE, SLICE_AT = 257, 132, 140, 4


def _slice_case():
    c = hu.make_case(SLICE_R, SLICE_N, SLICE_WIDE, "b")
    wide = np.full((SLICE_R, SLICE_WIDE), np.nan, dtype=np.float32)
    wide[:, SLICE_AT:SLICE_AT + SLICE_N] = c["x"]
    return c, wide


def _module(c, training):
    bn = torch.nn.BatchNorm1d(SLICE_N, eps=hu.EPS, momentum=0.1).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c["gamma"])); bn.bias.copy_(torch.from_numpy(c["beta"]))
        bn.running_mean.copy_(torch.from_numpy(c["run_mean"])); bn.running_var.copy_(torch.from_numpy(c["run_var"]))
    return bn.train(training)


def _judge(tag, got, cb, names):
    res = {}
    for name in names:
        ref, b = cb[name]
        res["ops." + name] = hu.ratio(got[name], ref, b)
        per_col = np.abs(hu.f64(got[name]) - ref) / np.maximum(b, 1e-300)
        print(tag, name, "worst error / chained bound %.3f" % res["ops." + name], "(worst column %d)" % int(np.argmax(per_col.max(0) if per_col.ndim == 2 else per_col)))
    _hold(tag, res)


def _check_slice_grad(wide_t, dx):
    g = wide_t.grad.cpu().numpy()
    assert np.array_equal(hu.bits(g[:, SLICE_AT:SLICE_AT + SLICE_N]), hu.bits(dx))
    outside = np.concatenate([g[:, :SLICE_AT], g[:, SLICE_AT + SLICE_N:]], axis=1)
    assert not hu.bits(outside).any(), "the columns outside the slice receive +0.0"


@pytest.mark.parametrize("training", [True, False])
def test_batch_norm_on_a_column_slice_per_column(lib, training):
    """ops.batch_norm(x, bn) with x = 132 columns inside a [257, 140] matrix (ld > N; NaN outside): y, dx, d gamma, d beta and the running
    statistics per column against float64 nn.BatchNorm1d within the chained bounds"""
    from news_recommendation_model_amd import ops
    c, wide = _slice_case()
    bn = _module(c, training)
    wide_t = torch.from_numpy(wide).cuda().requires_grad_(True)
    x = wide_t[:, SLICE_AT:SLICE_AT + SLICE_N]
    assert x.stride(0) == SLICE_WIDE and x.data_ptr() % 16 == 0
    gy = torch.from_numpy(c["dy"]).cuda()
    y = ops.batch_norm(x, bn)
    y.backward(gy)
    torch.cuda.synchronize()
    cb = hu.chain_bounds(c["x"], c["dy"], None, c["gamma"], c["beta"], c["run_mean"], c["run_var"], 0.1, hu.EPS, training)
    dx = wide_t.grad[:, SLICE_AT:SLICE_AT + SLICE_N].cpu().numpy()
    got = dict(y=y.detach().cpu().numpy(), dx=dx, dgamma=bn.weight.grad.cpu().numpy(), dbeta=bn.bias.grad.cpu().numpy(),
               running_mean=bn.running_mean.cpu().numpy(), running_var=bn.running_var.cpu().numpy())
    _judge(("batch_norm", training), got, cb, ["y", "dx", "dgamma", "dbeta"] + (["running_mean", "running_var"] if training else []))
    _check_slice_grad(wide_t, dx)
    if not training:
        assert np.array_equal(hu.bits(got["running_mean"]), hu.bits(c["run_mean"])) and np.array_equal(hu.bits(got["running_var"]), hu.bits(c["run_var"]))
    assert int(bn.num_batches_tracked) == (1 if training else 0)


@pytest.mark.parametrize("training", [True, False])
def test_gate_block_on_a_column_slice_per_column(lib, monkeypatch, training):
    """ops.gate_block on the same slice.  The node's BatchNorm output c and the (dc, dmul) its gate MLP hands the BatchNorm backward are
    read where the node passes them on; c, and dx, d gamma, d beta for that fp32 dc and add = dmul, are judged per column against float64
    nn.BatchNorm1d within the chained bounds; what autograd returns is bitwise what the BatchNorm backward returned."""
    from news_recommendation_model_amd import ops
    c, wide = _slice_case()
    bn = _module(c, training)
    rng = np.random.default_rng(7)
    hid = 16
    w1 = torch.from_numpy(hu.f32(0.1 * rng.standard_normal((hid, SLICE_N)))).cuda().requires_grad_(True)
    b1 = torch.from_numpy(hu.f32(0.1 * rng.standard_normal(hid))).cuda().requires_grad_(True)
    w2 = torch.from_numpy(hu.f32(0.3 * rng.standard_normal((SLICE_N, hid)))).cuda().requires_grad_(True)
    b2 = torch.from_numpy(hu.f32(1.0 + 0.1 * rng.standard_normal(SLICE_N))).cuda().requires_grad_(True)
    seen = {}
    real_apply, real_bwd = ops._bn_apply_impl, ops._bn_bwd_impl

    def apply(x, mean, rstd, weight, bias, batch_stats):
        seen["c"] = real_apply(x, mean, rstd, weight, bias, batch_stats)
        seen["ld"] = x.stride(0)
        return seen["c"]

    def bwd(dy, x, mean, rstd, weight, training, add=None, row_weight=None, n_rows=0):
        seen["dc"], seen["add"] = dy.detach().cpu().numpy().copy(), add.detach().cpu().numpy().copy()
        seen["out"] = real_bwd(dy, x, mean, rstd, weight, training, add=add, row_weight=row_weight, n_rows=n_rows)
        return seen["out"]

    monkeypatch.setattr(ops, "_bn_apply_impl", apply)
    monkeypatch.setattr(ops, "_bn_bwd_impl", bwd)
    wide_t = torch.from_numpy(wide).cuda().requires_grad_(True)
    x = wide_t[:, SLICE_AT:SLICE_AT + SLICE_N]
    y = ops.gate_block(x, bn, w1, b1, w2, b2)
    y.backward(torch.from_numpy(c["dy"]).cuda())
    torch.cuda.synchronize()
    assert seen["ld"] == SLICE_WIDE and set(seen) == {"c", "ld", "dc", "add", "out"}
    assert np.isfinite(y.detach().cpu().numpy()).all()
    cb = hu.chain_bounds(c["x"], seen["dc"], seen["add"], c["gamma"], c["beta"], c["run_mean"], c["run_var"], 0.1, hu.EPS, training)
    dx, dgamma, dbeta = (t.detach().cpu().numpy() for t in seen["out"])
    got = dict(y=seen["c"].detach().cpu().numpy(), dx=dx, dgamma=dgamma, dbeta=dbeta,
               running_mean=bn.running_mean.cpu().numpy(), running_var=bn.running_var.cpu().numpy())
    _judge(("gate_block", training), got, cb, ["y", "dx", "dgamma", "dbeta"] + (["running_mean", "running_var"] if training else []))
    _check_slice_grad(wide_t, dx)
    assert np.array_equal(hu.bits(bn.weight.grad.cpu().numpy()), hu.bits(dgamma)) and np.array_equal(hu.bits(bn.bias.grad.cpu().numpy()), hu.bits(dbeta))
    assert int(bn.num_batches_tracked) == (1 if training else 0)


def test_zz_worst_ratios():
    print("worst error / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert WORST and all(v <= 1.0 for v in WORST.values())
