"""GPU: the dense pool pair (pool_loss.hip) through nrm_pool_bmm and nrm_pool_rowdot, element by element against the float64 statements
of pool_util.  Bounds (derived in pool_util's docstring from the fp32 MFMA being a chain of fused multiply-adds): J U sum_j |W X| for the
batched product in either form (plus U (|prior| + |ref|) with `accumulate`), D U sum_d |g h| for the row dots; one-hot W / g must give
the selected row of X / column of h BITWISE.  tests/test_pool_cpu.py shows that this very check rejects six one-line mutants.

nrm_pool_bmm: the full product of I in 1 .. 65 and J in 1 .. 130 at D = 68, B = 3, D in 4 .. 132 at (17, 33), B = 1; each shape with W = s
and W = s^T (wsi = 1), ldx = D and D + 4 (NaN in the padding), accumulate 0 and 1, three families, and in the three settings of
NRM_POOL_JSPLIT (the launcher reads it at every launch).  nrm_pool_rowdot: T x H x D x ldg x B as listed in pool_util, zero_n in {0, 3, 300}
on a NaN-filled zero_out.  Sentinels behind every output.

No test of this file creates a stream or captures a graph.  Set NRM_HEAD_POOL_RECORD=<path> to merge the worst error / bound per entry
into a JSON file (profiles/head_pool_bounds.json is such a record; no gate is derived from it)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pool_util as pu  # noqa: E402
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
        data["pool"] = {k: round(WORST[k], 4) for k in sorted(WORST)}
        with open(path, "w") as f:
            json.dump(data, f, indent=1)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Native:
    """pool_util's backend over the C ABI; every tensor lives until the call has been waited for.  ``form`` is the environment's."""

    def bmm(self, wmem, wsb, wsi, wsj, xmem, ldx, out, B, I, J, D, accumulate, form):
        assert os.environ.get("NRM_POOL_JSPLIT") == form
        w, x, o = _d(wmem), _d(xmem), _d(out)
        native.call("nrm_pool_bmm", native.ptr(w), wsb, wsi, wsj, native.ptr(x), ldx, native.ptr(o), B, I, J, D, accumulate, native.stream_ptr())
        torch.cuda.synchronize()
        return o.cpu().numpy()

    def rowdot(self, gmem, ldg, hmem, ds, B, T, H, D, zero_out, zero_n):
        g, h, o, z = _d(gmem), _d(hmem), _d(ds), _d(zero_out)
        native.call("nrm_pool_rowdot", native.ptr(g), ldg, native.ptr(h), native.ptr(o), B, T, H, D, native.ptr(z), zero_n, native.stream_ptr())
        torch.cuda.synchronize()
        return o.cpu().numpy(), z.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _bmm_case(B, I, J, D, layout, ldx, family):
    """made once, shared by the three forms, never changed (the backends copy what they write)"""
    return pu.make_bmm(B, I, J, D, layout, ldx, family)


def _hold(tag, res):
    for k, v in res.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= 1.0, (tag, k, v)


@pytest.mark.parametrize("layout", pu.LAYOUTS)
@pytest.mark.parametrize("jsplit", pu.FORMS)
def test_pool_bmm_per_element(lib, monkeypatch, jsplit, layout):
    if jsplit is None:
        monkeypatch.delenv("NRM_POOL_JSPLIT", raising=False)
    else:
        monkeypatch.setenv("NRM_POOL_JSPLIT", jsplit)
    be, ran, worst = Native(), 0, 0.0
    for B, I, J, D in pu.bmm_shapes():
        for ldx in (D, D + 4):
            for family in pu.BMM_FAMILIES:
                c = _bmm_case(B, I, J, D, layout, ldx, family)
                for accumulate in (0, 1):
                    res = pu.check_bmm(be, c, accumulate, jsplit)
                    assert ("pool_bmm.onehot" in res) == (family == "onehot" and not accumulate)
                    _hold((jsplit, layout, B, I, J, D, ldx, family, accumulate), res)
                    worst = max(worst, res["pool_bmm"])
                    ran += 1
    print(f"NRM_POOL_JSPLIT={jsplit} W={layout}: {ran} launches, worst error / bound {worst:.3f}")
    assert ran == len(pu.bmm_shapes()) * 2 * len(pu.BMM_FAMILIES) * 2


@pytest.mark.parametrize("D", pu.ROWDOT_D)
def test_pool_rowdot_per_element(lib, D):
    be, ran, worst = Native(), 0, 0.0
    for B, T, H, d in pu.rowdot_shapes():
        if d != D:
            continue
        for ldg in (D, D + 4):
            for family in pu.ROWDOT_FAMILIES:
                c = pu.make_rowdot(B, T, H, D, ldg, family)
                for zero_n in (pu.ZERO_N if family == "normal" else pu.ZERO_N[ran % 3:][:1]):
                    res = pu.check_rowdot(be, c, zero_n)
                    assert ("pool_rowdot.onehot" in res) == (family == "onehot")
                    _hold((B, T, H, D, ldg, family, zero_n), res)
                    worst = max(worst, res["pool_rowdot"])
                    ran += 1
    print(f"D={D}: {ran} launches, worst error / bound {worst:.3f}")
    assert ran == len(pu.ROWDOT_B) * len(pu.ROWDOT_T) * len(pu.ROWDOT_H) * 2 * 4


def test_zz_worst_ratios():
    print("worst error / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert WORST and all(v <= 1.0 for v in WORST.values())
