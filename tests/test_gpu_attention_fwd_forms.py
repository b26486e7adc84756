"""GPU: every forward form of the pointwise attention the selector can return (csrc/pwattn_fwd.hip pwattn_fwd_select) is launched, is
the form the query nrm_pwattn_fwd_form says it is at this device's own compute-unit count, and is compared with float64.

The cases live in tests/attention_fwd_forms_util.py; tests/test_attention_fwd_forms_cpu.py holds the set of forms they reach equal to
the set the selector returns.  Gates are those of tests/attention_budget.py, unchanged: M_F32, M_BF16X3 times what the fp32 oracle
(bf16x3: or the CPU emulation of bf16x3) loses against float64 on the same case, per impression; plain bf16 is characterised with the
1e-2 bound of tests/test_gpu_attention.py, not gated.
  1. test_small_forms: default latched knobs, one round.  The dense variants run forward with z and the whole backward under the error
     budget (a wrong saved z shows in the gradients); the launch without a z store must give the same scores bit for bit (one or two
     column slices: exact float adds; more slices add in any order, so there the scores of that launch are gated against float64
     instead); the ragged and history-ragged variants are gated against float64 on their lists.
  2. test_second_round: the smallest shape for which every variant's busiest wave goes round its persistent loop twice, with a partial
     last round, computed from the compute-unit count.  Scores per impression against float64, the saved z of the first and the last two
     impressions (the second round's rows are the last ones), and a NaN planted in the first row of the wave that takes the first
     second-round tile / task.
  3. test_latched_knobs_in_a_child_process: NRM_FWD_WALK=0 in a fresh python child (tests/attention_fwd_knob_worker.py); the child
     prints its figures, the gates are applied here.
  4. test_slices_add_b2_once_into_a_cleared_buffer: the several-slice launch path (bf16x3 at D = 132 and 400) adds b2 in one slice only
     and clears the score buffer its slices add into."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_budget as ab
import attention_fwd_forms_util as afu
from attention_fwd_forms_util import BF16, BF16X3, F32

pytestmark = pytest.mark.gpu
_record = []


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("NRM_FWD_FORMS_RECORD")          # a file: every measured figure of this module, for profiles/
    if path:
        with open(path, "w") as f:
            json.dump({"M": {"f32": ab.M_F32, "bf16x3": ab.M_BF16X3}, "bf16_bound": afu.BF16_BOUND, "runs": _record}, f, indent=1)


@pytest.fixture
def cus(lib, monkeypatch):
    for k in afu.PER_LAUNCH:
        monkeypatch.delenv(k, raising=False)
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    # the latched knobs were read at the first query or launch of this process: these tests describe the default dispatch
    probe = [afu.dense_query(lib, (3, 5, 17, D), mma, 1, n) for D, mma in ((64, F32), (400, F32), (64, BF16))]
    assert [(f["family"], afu.template(f)) for f in probe] == [("walk_f32", (4,)), ("stream", (13, 1, 4, 1, 4)), ("walk_bf16", (4, 2))], \
        "run without NRM_FWD_WALK"
    return n


def _id(case):
    shape, settings = case
    return "-".join(map(str, shape)) + "".join(f"-{k[8:].lower()}{v}" for k, v in sorted(settings.items()))


@pytest.mark.parametrize("case", afu.SMALL_CASES, ids=_id)
def test_small_forms(lib, cus, case):
    shape, settings = case
    data = afu.Data(shape)
    bcase = ab.get_case(shape)
    assert np.array_equal(bcase.t, data.t) and np.array_equal(bcase.h, data.h)
    variants = afu.variants_of(lib, shape, settings, cus=cus)
    # the forms this case is in the lists for do not depend on the device: one round at any compute-unit count
    assert [afu.key(f) for _v, f in variants] == [afu.key(f) for _v, f in afu.variants_of(lib, shape, settings, cus=256)]
    with afu.env(settings):
        saved = {}
        for (kind, mma, z), f in variants:
            what = f"{_id(case)} {kind} {afu.NAME_OF_MMA[mma]} z={z} {f['family']}{afu.template(f)} slices {f['nsplit']} parts {f['tsplit']}"
            if kind == "dense" and z:
                got = ab.run_device(bcase, afu.NAME_OF_MMA[mma])                # forward with z and the whole backward
                if mma == BF16:
                    figure = afu.check_scores(data, (kind, mma, z), list(got["s"]), what)
                else:
                    r = ab.assert_within_budget(got, bcase, afu.NAME_OF_MMA[mma], record=None)
                    figure = {f"{p}|{n}": float(v) for (p, n), v in r.items()}
                    print(f"{what}: worst budget ratio {ab.worst(r):.2f}")
                s, _zz = afu.launch(data, (kind, mma, 1))
                if f["nsplit"] <= 2:                          # the training node and the bare op launch the same kernel
                    assert np.array_equal(np.stack(s), got["s"]), what
                saved[mma] = np.stack(s)
            elif kind == "dense":
                s, _zz = afu.launch(data, (kind, mma, 0))
                if f["nsplit"] <= 2:
                    assert np.array_equal(np.stack(s), saved[mma]), what + ": the z store changes the scores"
                    figure = {"equal_to_saving_launch": True}
                else:
                    figure = afu.check_scores(data, (kind, mma, z), s, what)
            else:
                s, _zz = afu.launch(data, (kind, mma, z))
                figure = afu.check_scores(data, (kind, mma, z), s, what)
            _record.append({"test": "small", "case": _id(case), "variant": [kind, afu.NAME_OF_MMA[mma], z], "form": afu._jsonable(afu.key(f)),
                            "figure": figure})


@pytest.mark.parametrize("case", afu.ROUND2_CASES, ids=lambda c: c[0])
def test_second_round(lib, cus, case):
    shape, runs = afu.run_second_round(lib, case, cus)
    for (kind, mma, z), f, figure in runs:
        _record.append({"test": "round2", "case": case[0], "shape": list(shape), "variant": [kind, afu.NAME_OF_MMA[mma], z],
                        "form": afu._jsonable(afu.key(f)), "rounds": f["rounds"], "figure": figure})


def _direct_launch(data, mma, b2=None, prefill=None):
    """nrm_pwattn_fwd (no z) as ops calls it, into a score buffer of this module's own -> s [B, T, H] on the host."""
    from news_recommendation_model_amd import native, ops
    B, T, H, D = data.shape
    w1, b1, w2, b2_w = data.wd
    if b2 is not None:
        b2_w = torch.full_like(b2_w, b2)
    t, h, u, v, packed, w2v, b2v = ops._attn_operands(data.dev(data.t), data.dev(data.h), w1, b1, w2, b2_w, mma)
    s = torch.full((B * T * H,), float(prefill), device="cuda") if prefill is not None else torch.empty(B * T * H, device="cuda")
    native.call("nrm_pwattn_fwd", native.ptr(t), native.ptr(h), native.ptr(u), native.ptr(v), native.ptr(packed), native.ptr(w2v),
                native.ptr(b2v), None, native.ptr(s), B, T, H, D, mma, native.stream_ptr())
    torch.cuda.synchronize()
    return s.cpu().numpy().reshape(B, T, H)


@pytest.mark.parametrize("shape", [(3, 5, 17, 132), (3, 5, 17, 400)], ids=lambda s: f"D{s[3]}")
def test_slices_add_b2_once_into_a_cleared_buffer(lib, cus, shape):
    """Several column slices (bf16x3: two at D = 132, five at D = 400) add their partial scores with float atomics.  b2 is added by ONE
    slice: the scores move by exactly the change of b2 (to fp32 rounding of sums of this size, the products being identical and only the
    order of the atomic adds free); and the launch clears the buffer its slices add into: what was there before is not part of the scores."""
    f = afu.dense_query(lib, shape, BF16X3, 0, cus)
    assert f["valid"] and f["family"] == "rw_tile" and f["nsplit"] > 1, f
    assert f["nsplit"] == {132: 2, 400: 5}[shape[3]]
    data = afu.Data(shape)
    s0, s1 = _direct_launch(data, BF16X3, b2=0.0), _direct_launch(data, BF16X3, b2=0.75)
    tol = 64 * 2.0 ** -24 * max(1.0, float(np.abs(s1).max()))
    s2 = _direct_launch(data, BF16X3, b2=0.75, prefill=1000.0)
    print(f"{shape} slices {f['nsplit']}: |s1 - s0 - 0.75| {np.abs(s1 - s0 - 0.75).max():.3e}, |s2 - s1| {np.abs(s2 - s1).max():.3e} (tolerance {tol:.3e})")
    assert np.abs(s1 - s0 - 0.75).max() <= tol, "b2 does not enter the scores exactly once"
    assert np.abs(s2 - s1).max() <= tol, "a pre-filled score buffer is added to"


@pytest.mark.parametrize("which", sorted(afu.LATCHED_SETTINGS))
def test_latched_knobs_in_a_child_process(lib, cus, tmp_path, which):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in afu.KNOBS}
    env.update(afu.LATCHED_SETTINGS[which])
    args = [sys.executable, os.path.join(here, "attention_fwd_knob_worker.py"), which]
    if which == "walk0":                                          # the walk's scores of the same cases, from this process
        walk = {}
        for shape, variants in afu.KNOB_WIDTH_CASES[which]:
            data = afu.Data(shape)
            for v, f in afu.variants_of(lib, shape, {}, variants, cus):
                assert f["family"] == "walk_bf16", (shape, v, f)
                walk[f"{shape}{v}"] = [a.tolist() for a in afu.launch(data, v)[0]]
        path = str(tmp_path / "walk_scores.json")
        with open(path, "w") as fh:
            json.dump(walk, fh)
        args.append(path)
    pr = subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, (pr.returncode, pr.stderr.decode(errors="replace")[-3000:])
    res = json.loads(pr.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(res, indent=1))
    assert res["which"] == which and res["forms_ok"] is True, res
    assert len(res["figures"]) == res["expected"] > 0
    for what, fig in res["figures"].items():
        arith = fig["arithmetic"]
        for k, v in fig["values"].items():
            if k.endswith("bf16"):
                assert v < afu.BF16_BOUND, (what, k, v)
            elif k.startswith("equal"):
                assert v is True, (what, k)
            elif k.startswith("budget|"):
                assert v <= ab.m_of(k.split("|")[1], arith), (what, k, v)
            elif k.startswith("against_walk|"):              # two fp32 accumulations of the same products: each within M_F32 yardsticks of their exact sum
                assert v <= 2 * ab.M_F32, (what, k, v)
            else:
                assert arith != "bf16" and v <= ab.M[arith], (what, k, v)
    _record.append({"test": "knob", "which": which, "figures": res["figures"]})
