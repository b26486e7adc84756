"""Child process of tests/test_gpu_dense.py::test_latched_gemm_knobs_in_a_child_process: the gemm_nt forms behind knobs that are read once
per process.  The parent sets the environment; this script checks with nrm_gemm_nt_form that the knobs select the forms they are
for, runs the dense ops against float64 PyTorch and prints ONE JSON line {"which", "forms_ok", "expected", "rel_err": {case: value}}.
The gates are the parent's.

    python tests/dense_knob_worker.py planned_mt    (NRM_NT_SMALLM=0 NRM_NT_NARROW=0 NRM_TN_SHAPES=0)

Child process of tests/test_gpu_dense_elements.py::test_gemm_nt_planned_forms_in_a_child_process as well: the four forms with several row
tiles per wave, element by element against float64 (dense_elements_util.check_nt over the C ABI) at M around one and two workgroups; prints
ONE JSON line {"which", "forms_ok", "expected", "ran", "ratios": {key: worst error / bound}}.

    python tests/dense_knob_worker.py elements_planned_mt    (NRM_NT_SMALLM=0, NRM_NT_NARROW unset)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np          # noqa: E402
import torch                # noqa: E402

import dense_forms_util as dfu                                   # noqa: E402
from golden_util import rel_err                                  # noqa: E402
from news_recommendation_model_amd import native, ops           # noqa: E402

F = torch.nn.functional


def linear_case(out, M, K, N):
    for gelu in (False, True):
        g = torch.Generator(device="cpu").manual_seed(M * 7 + K + N)
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / np.sqrt(K)
        b = torch.randn(N, generator=g) * 0.1
        gy = torch.randn(M, N, generator=g)
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        y_ref = F.linear(xr, wr, br)
        if gelu:
            y_ref = F.gelu(y_ref)
        y_ref.backward(gy.double())
        xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
        y = ops.linear(xg, wg, bg, gelu=gelu)
        y.backward(gy.cuda())
        tag = f"linear{(M, K, N)}{'+gelu' if gelu else ''}."
        out[tag + "y"] = rel_err(y.detach().cpu().numpy(), y_ref.detach().numpy())
        for name, a, r in (("dx", xg, xr), ("dw", wg, wr), ("db", bg, br)):
            out[tag + name] = rel_err(a.grad.cpu().numpy(), r.grad.numpy())
    return 8


def mlp_case(out, M, K, Hd, N):
    g = torch.Generator(device="cpu").manual_seed(M + 3 * K + 5 * Hd + 7 * N)
    x = torch.randn(M, K, generator=g)
    w1 = torch.randn(Hd, K, generator=g) / np.sqrt(K)
    b1 = torch.randn(Hd, generator=g) * 0.1
    w2 = torch.randn(N, Hd, generator=g) / np.sqrt(Hd)
    b2 = torch.randn(N, generator=g) * 0.1
    gy = torch.randn(M, N, generator=g)
    ref = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y_ref = F.linear(F.gelu(F.linear(ref[0], ref[1], ref[2])), ref[3], ref[4])
    y_ref.backward(gy.double())
    dev = [t.cuda().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = ops.mlp_gelu(*dev)
    y.backward(gy.cuda())
    tag = f"mlp_gelu{(M, K, Hd, N)}."
    out[tag + "y"] = rel_err(y.detach().cpu().numpy(), y_ref.detach().numpy())
    for a, r, name in zip(dev, ref, ("dx", "dw1", "db1", "dw2", "db2")):
        out[tag + name] = rel_err(a.grad.cpu().numpy(), r.grad.numpy())
    return 6


def gemm_tn_case(out, R, ni, nj):
    g = torch.Generator(device="cpu").manual_seed(R + 3 * ni + 5 * nj)
    a = ops._rows(torch.randn(R, ni, generator=g).cuda())
    b = ops._rows(torch.randn(R, nj, generator=g).cuda())
    c, cs = ops._gemm_tn(a, b, True)
    torch.cuda.synchronize()
    assert tuple(c.shape) == (ni, nj)
    out[f"gemm_tn{(R, ni, nj)}.c"] = rel_err(c.cpu().numpy(), (a.double().t() @ b.double()).cpu().numpy())
    out[f"gemm_tn{(R, ni, nj)}.colsum"] = rel_err(cs.cpu().numpy(), a.double().sum(0).cpu().numpy())
    return 2


def elements_planned_mt(lib):
    import dense_elements_util as du
    from test_gpu_dense_elements import Native, run_nt
    planned = lambda M, N: du.nt_form(M, N, small_m=False)          # noqa: E731
    want = {4: (4, 4, 2, 1), 5: (5, 4, 2, 1), 8: (8, 3, 2, 1), 9: (9, 2, 3, 1)}
    forms_ok = all(du.lib_nt_form(lib, M, N, K) == planned(M, N) == want[NT] for NT in du.MT_WIDTHS for M, K, N in du.mt_shapes(NT))
    worst, ran, expected = {}, 0, 0

    def hold(tag, res):
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    be = Native()
    for NT in du.MT_WIDTHS:
        launches = du.nt_launches(du.mt_shapes(NT), families=("normal", "scaled", "onehot"))
        expected += len(launches)
        ran += run_nt(be, launches, planned, hold)
    torch.cuda.synchronize()
    print(json.dumps({"which": "elements_planned_mt", "forms_ok": bool(forms_ok), "expected": expected, "ran": ran, "ratios": worst}), flush=True)


def main(which):
    lib = native.load()
    if which == "elements_planned_mt":
        return elements_planned_mt(lib)
    nt = lambda M, N, K: dfu.nt_form(lib, M, N, K)               # noqa: E731
    out, n = {}, 0
    if which == "planned_mt":
        linears = [(300, 1032, 258), (300, 264, 66), (33, 66, 64)]
        forms_ok = (all(nt(M, 64, 66) == (4, 4, 2, 1) for M in (33, 300)) and all(nt(M, N, 264) == (8, 3, 2, 1) for N in (258, 66) for M in (33, 64, 300))
                    and nt(300, 1032, 258) == (13, 1, 4, 1) and nt(300, 264, 66) == (8, 3, 2, 1))
        for shape in linears:
            n += linear_case(out, *shape)
        n += mlp_case(out, 64, 264, 66, 264)
        for shape in [(640, 400, 402), (130, 2, 1608)]:          # gemm_tn on the plain 4x4 / 5x5 wave tiles (NRM_TN_SHAPES=0)
            n += gemm_tn_case(out, *shape)
    else:
        raise SystemExit(f"unknown knob set {which!r}")
    torch.cuda.synchronize()
    print(json.dumps({"which": which, "forms_ok": bool(forms_ok), "expected": n, "rel_err": out}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
