"""GPU: the fp32 dense kernels of csrc/gemm.hip through their C entries -- nrm_gemm_pack / nrm_gemm_pack_multi + nrm_gemm_nt (every
gemm_nt_kernel<NT, MT, EPI, WPE> the selector returns, four epilogues), nrm_gemm_tn (all six wave tiles, 1 .. 8 row splits, colsum, zero_out)
and nrm_slab_reduce / nrm_slab_reduce_multi -- element by element against the float64 statements of dense_elements_util.  Bounds (derived in
the util's docstring): K U sum |x w| for the accumulator (+ U |ref| for the bias, one more rounding per term for a src + sign2 src2 pack),
G |z| = (0.75e-7 + 16 U) |z| for gelu of the device's own z, |gelu'| K U sum |x w| + |acc| G' + U |ref| with G' = 0.75e-7 + 19 U for the
GELU' epilogue, nrows_s U sum |a b| per slab of gemm_tn, (spc - 1 + nchunk) U sum |ws| + nchunk U |prior| for the slab reduction; one-hot
operands must come out BITWISE.  NaN in every byte the kernels promise not to read (x, A, B and slab padding, the floats behind every
input), sentinels in every float they promise not to write (rows >= M, columns past the last tile, around the column block of `out`, four
floats behind every output), zeros of the stated sign in the padding columns of y and z.  tests/test_dense_elements_cpu.py shows that this very
check rejects twenty-two one-line mutants.

The four forms with several row tiles per wave run in ONE child process (tests/dense_knob_worker.py elements_planned_mt, NRM_NT_SMALLM=0 is
latched per process); the gate on its ratios is here.  No test of this file creates a stream or captures a graph.  Set
NRM_DENSE_RECORD=<path> to merge the worst error / bound per key into a JSON file (profiles/dense_element_bounds.json is such a record; no gate
is derived from it)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dense_elements_util as du  # noqa: E402
import dense_forms_util as dfu  # noqa: E402
from news_recommendation_model_amd import native  # noqa: E402

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("NRM_DENSE_RECORD")
    if path:
        data = {}
        if os.path.exists(path):
            with open(path) as f:
                data = json.load(f)
        for k in sorted(WORST):
            data[k] = round(max(WORST[k], data.get(k, 0.0)), 4)
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset)


def _h(t):
    return None if t is None else t.cpu().numpy()


class Native:
    """dense_elements_util's backend over the C ABI; every tensor lives until the call has been waited for"""

    def __init__(self):
        self.lib = native.load()

    def tn_plan(self, ni, nj, R, waves):
        assert os.environ.get("NRM_TN_WAVES") == waves
        return du.lib_tn_plan(self.lib, ni, nj, R)

    def gemm_nt(self, xmem, ldx, M, w, w2, sign2, N, K, bias, ymem, ldy, zmem, ldz, mmem, ldm, epi, form):
        assert du.lib_nt_form(self.lib, M, N, K) == tuple(form), (M, N, K, form)      # the launch below is the form the case is for
        st = native.stream_ptr()
        x, ws, ws2, b, y, z, m = _d(xmem), _d(w), _d(w2), _d(bias), _d(ymem), _d(zmem), _d(mmem)
        packed = torch.full((self.lib.nrm_gemm_packed_floats(N, K, 0),), float("nan"), device="cuda")
        if w2 is None:
            native.call("nrm_gemm_pack", native.ptr(ws), K, 1, N, K, native.ptr(packed), st)
        else:
            descs = (native.PackDesc * 1)()
            d = descs[0]
            d.src, d.src2, d.sign2, d.row_stride, d.col_stride = ws.data_ptr(), ws2.data_ptr(), sign2, K, 1
            d.nrows, d.ncols, d.packed, d.mma = N, K, packed.data_ptr(), 0
            native.call("nrm_gemm_pack_multi", descs, 1, st)
        native.call("nrm_gemm_nt", _p(x), ldx, M, _p(packed), N, K, _p(b), _p(y), ldy, _p(z), ldz, _p(m), ldm, epi, 0, st)
        torch.cuda.synchronize()
        return _h(y), _h(z)

    def gemm_tn(self, amem, lda, ni, bmem, ldb, nj, R, ws, ldws, colsum, zero_out, zero_n, waves, plan):
        assert os.environ.get("NRM_TN_WAVES") == waves
        a, b, w, cs, zo = _d(amem), _d(bmem), _d(ws), _d(colsum), _d(zero_out)
        native.call("nrm_gemm_tn", _p(a), lda, ni, _p(b), ldb, nj, R, _p(w), ldws, _p(cs), _p(zo), zero_n, 0, native.stream_ptr())
        torch.cuda.synchronize()
        return _h(w), _h(cs), _h(zo)

    def slab_reduce(self, sets, multi):
        keep, descs = [], (native.SlabDesc * len(sets))()
        for d, s in zip(descs, sets):
            w, o, o2, v = _d(s["wsmem"]), _d(s["outmem"]), _d(s["out2mem"]), _d(s["vecmem"])
            vo = None if v is None else torch.full((s["ni"] + du.TAIL,), float(du.SENTINEL), device="cuda")
            keep.append((w, o, o2, v, vo))
            args = (s["nsplit"], s["nj"], s["ldws"], s["ni"])
            if multi:
                d.ws, (d.nsplit, d.nj, d.ldws, d.ni) = w.data_ptr(), args
                d.out, d.out_istride, d.out_jstride = o.data_ptr() + 4 * s["off"], s["wide"], 1
                d.out2, d.out2_istride, d.out2_jstride, d.sign2 = (None if o2 is None else o2.data_ptr()), 1, s["ni"] + 3, -1.0
                d.vec, d.vec_out = (None if v is None else v.data_ptr()), (None if vo is None else vo.data_ptr())
            else:
                native.call("nrm_slab_reduce", _p(w), *args, _p(o, s["off"]), s["wide"], 1, _p(o2), 1, s["ni"] + 3, -1.0, _p(v), _p(vo), native.stream_ptr())
        if multi:
            native.call("nrm_slab_reduce_multi", descs, len(sets), native.stream_ptr())
        torch.cuda.synchronize()
        return [(_h(o), _h(o2), _h(vo)) for _, o, o2, _, vo in keep]


def _hold(tag, res):
    for k, v in res.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= 1.0, (tag, k, v)


def run_nt(be, launches, form_of, hold):
    """every launch of a list through check_nt; returns how many ran"""
    ran = 0
    for M, K, N, epi, family, variant in launches:
        res = du.check_nt(be, du.nt_case(M, K, N, family), epi, variant, form_of(M, N))
        assert ("nt.onehot" in res) == (epi == "bias" and family == "onehot" and not variant[3])
        hold((M, K, N, epi, family, variant), res)
        ran += 1
    return ran


@pytest.mark.parametrize("NT", sorted(du.NT_WIDTHS))
def test_gemm_nt_per_element(lib, monkeypatch, NT):
    """gemm_nt_kernel<NT, 1, EPI, 4>: M around the 16-row tile and the 64-row workgroup, K around the 16-wide chunk, the widths of the util"""
    for k in dfu.KNOBS:
        monkeypatch.delenv(k, raising=False)
    launches = du.nt_launches(du.nt_shapes(NT))
    ran = run_nt(Native(), launches, du.nt_form, _hold)
    print(f"NT = {NT}: {ran} launches, worst error / bound", {k: round(v, 3) for k, v in WORST.items() if k.startswith("nt.%dx" % NT)})
    assert ran == len(du.nt_shapes(NT)) * 14 == len(launches)


def test_gemm_nt_planned_forms_in_a_child_process(lib):
    """<4,4,2>, <5,4,2>, <8,3,2> and <9,2,3> at M around one and two workgroups: taken at small M only under NRM_NT_SMALLM=0"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in dfu.KNOBS and k not in ("NRM_TN_SHAPES", "NRM_TN_WAVES")}
    env["NRM_NT_SMALLM"] = "0"
    pr = subprocess.run([sys.executable, os.path.join(here, "dense_knob_worker.py"), "elements_planned_mt"], env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, (pr.returncode, pr.stderr.decode(errors="replace")[-3000:])
    res = json.loads(pr.stdout.decode().strip().splitlines()[-1])
    assert res["which"] == "elements_planned_mt" and res["forms_ok"] is True, res
    assert res["ran"] == res["expected"] == 5 * 5 * 12
    print(res["ratios"])
    assert {k for k in res["ratios"] if k.startswith("nt.") and k != "nt.onehot"} == {"nt.%dx%d.%s" % (NT, du.NT_PLANNED[NT][0], e) for NT in du.MT_WIDTHS
                                                                                      for e in du.EPILOGUES}
    _hold("elements_planned_mt", {k: (v if v is not None else du.INF) for k, v in res["ratios"].items()})


@pytest.mark.parametrize("waves", du.TN_WAVES)
def test_gemm_tn_per_element(lib, monkeypatch, waves):
    """every wave tile, R from one row to eight splits; NRM_TN_WAVES (read at every call) = 1 keeps a launch at four splits"""
    if waves is None:
        monkeypatch.delenv("NRM_TN_WAVES", raising=False)
    else:
        monkeypatch.setenv("NRM_TN_WAVES", waves)
    be, ran, shapes = Native(), 0, set()
    launches = [t for t in du.tn_launches() if t[3] == waves]
    for n, (ni, nj, R, w, family, dpad, colsum, zero_n) in enumerate(launches):
        res = du.check_tn(be, du.tn_case(ni, nj, R, w, family, dpad), colsum, zero_n, dws=4 * (n % 2))
        assert ("tn.colsum" in res) == colsum
        _hold((ni, nj, R, w, family, dpad, colsum, zero_n), res)
        shapes |= {k for k in res if k != "tn.colsum"}
        ran += 1
    print(f"NRM_TN_WAVES={waves}: {ran} launches, worst error / bound", {k: round(v, 3) for k, v in WORST.items() if k.startswith("tn.")})
    assert ran == len(launches) >= 24 and (waves is not None or shapes == {"tn.%dx%d" % s for s in du.TN_SHAPES})


def test_slab_reduce_per_element(lib):
    """nrm_slab_reduce set by set, nrm_slab_reduce_multi with one set and with more sets than one table of the launch holds"""
    be, ran = Native(), 0
    cases = du.slab_cases()
    for c in cases:
        res = du.check_slab(be, c)
        _hold(([(s["nsplit"], s["ni"], s["nj"]) for s in c["sets"]][:3], c["multi"]), res)
        ran += len(c["sets"])
    print(f"{ran} slab sets in {len(cases)} launches, worst error / bound", {k: round(v, 3) for k, v in WORST.items() if k.startswith("slab")})
    assert ran == 2 * len(du.SLAB_SETS) + 3 + 3 * len(du.SLAB_SETS)
    assert sum(1 for c in cases if not c["multi"]) == 2 * len(du.SLAB_SETS) and cases[-1]["multi"] and len(cases[-1]["sets"]) == 3 * len(du.SLAB_SETS)
