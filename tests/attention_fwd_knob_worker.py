"""Child process of tests/test_gpu_attention_fwd_forms.py::test_latched_knobs_in_a_child_process: the forward forms behind knobs that are
read once per process.  The parent sets the environment; this script checks with nrm_pwattn_fwd_form that the knob selects the forms it is
for, runs the cases of tests/attention_fwd_forms_util.py KNOB_CASES against float64 and prints ONE JSON line
{"which", "forms_ok", "expected", "figures": {launch: {"arithmetic", "values": {name: figure}}}}.  The gates are the parent's.

    python tests/attention_fwd_knob_worker.py rw0           (NRM_FWD_RW=0: the streaming kernel <4,4>, <6,4>, <8,3> at D <= 128)
    python tests/attention_fwd_knob_worker.py rw2           (NRM_FWD_RW=2: the fp32 resident tiles in several slices)
    python tests/attention_fwd_knob_worker.py 13x1_0        (NRM_FWD_13X1=0: one chunk of 25 tiles)
    python tests/attention_fwd_knob_worker.py walk0 FILE    (NRM_FWD_WALK=0: the tile-by-tile kernel where the bf16 walks are the default;
                                                             FILE: the walk's scores of the same cases, from the parent)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np          # noqa: E402
import torch                # noqa: E402

import attention_budget as ab                                    # noqa: E402
import attention_fwd_forms_util as afu                           # noqa: E402
from attention_fwd_forms_util import BF16, F32                   # noqa: E402
from news_recommendation_model_amd import native, ops           # noqa: E402

# what each setting is for: (family, template parameters, column slices) by width, dense or ragged alike
EXPECTED = {
    "rw0": {64: ("stream", (4, 4, 2, 0, 4), 1), 68: ("stream", (6, 4, 2, 0, 4), 1), 100: ("stream", (8, 3, 2, 0, 4), 1)},
    "rw2": {400: ("rw_tile", (5,), 5), 132: ("rw_tile", (5,), 2), 164: ("rw_tile", (6,), 2), 196: ("rw_tile", (8,), 2), 500: ("rw_tile", (4,), 8),
            628: ("rw_tile", (3,), 14), 1024: ("rw_tile", (2,), 32)},
    "13x1_0": {388: ("stream", (25, 1, 2, 0, 4), 1), 400: ("stream", (25, 1, 2, 0, 4), 1)},
    "walk0": {64: ("rw_tile", (4,), 1), 128: ("rw_tile", (8,), 1), 256: ("rw_tile", (8,), 2)},
}


def direct_launch(data, b2=None, prefill=None):
    """nrm_pwattn_fwd (fp32, no z) as ops calls it, into a score buffer of this script's own -> s [B, T, H] on the host."""
    B, T, H, D = data.shape
    w1, b1, w2, b2_w = data.wd
    if b2 is not None:
        b2_w = torch.full_like(b2_w, b2)
    t, h, u, v, packed, w2v, b2v = ops._attn_operands(data.dev(data.t), data.dev(data.h), w1, b1, w2, b2_w, F32)
    s = torch.full((B * T * H,), float(prefill), device="cuda") if prefill is not None else torch.empty(B * T * H, device="cuda")
    native.call("nrm_pwattn_fwd", native.ptr(t), native.ptr(h), native.ptr(u), native.ptr(v), native.ptr(packed), native.ptr(w2v),
                native.ptr(b2v), None, native.ptr(s), B, T, H, D, F32, native.stream_ptr())
    torch.cuda.synchronize()
    return s.cpu().numpy().reshape(B, T, H)


def main(which, walk_file=None):
    lib = native.load()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    walk = json.load(open(walk_file)) if walk_file else None
    figures, forms_ok, n = {}, True, 0
    for shape, variants in afu.KNOB_CASES[which] + afu.KNOB_WIDTH_CASES.get(which, []):
        D = shape[3]
        data = afu.Data(shape)
        bcase = ab.get_case(shape)
        assert np.array_equal(bcase.t, data.t) and np.array_equal(bcase.h, data.h)
        fs = afu.variants_of(lib, shape, {}, variants, cus)
        forms_ok = forms_ok and len(fs) == len(variants)
        saved = {}
        for variant, f in fs:
            kind, mma, z = variant
            forms_ok = forms_ok and (f["family"], afu.template(f), f["nsplit"]) == EXPECTED[which][D] and f["rounds"] == 1
            arith = afu.NAME_OF_MMA[mma]
            what = f"{shape} {kind} {arith} z={z} {f['family']}{afu.template(f)} slices {f['nsplit']}"
            vals = {}
            if kind == "dense" and z:
                got = ab.run_device(bcase, arith)                # forward with z and the whole backward
                if mma == BF16:
                    vals.update(afu.check_scores(data, variant, list(got["s"]), what))
                else:
                    vals.update({f"budget|{p}|{nm}": float(v) for (p, nm), v in ab.ratios(got, bcase, arith).items()})
                saved[mma] = got["s"]
            s, _zz = afu.launch(data, variant)
            if kind == "dense" and not z and f["nsplit"] <= 2:
                vals["equal_to_saving_launch"] = bool(np.array_equal(np.stack(s), saved[mma]))
            if not (kind == "dense" and z and mma != BF16):
                vals.update({"s|" + k: v for k, v in afu.check_scores(data, variant, s, what).items()})
            if not z:
                vals.update(afu.check_row_plants(data, variant, what))
            if walk is not None:                                  # against the walk kernel's scores: the same products, another association
                r64 = data.reference(torch.float64)[0]
                y = ab._piece_err("s", list(data.reference(torch.float32)[0]), list(r64))[0]
                w = [np.asarray(a) for a in walk[f"{shape}{variant}"]]
                d = max(np.abs(s[b] - w[b]).max() / np.abs(r64[b]).max() for b in range(shape[0]))
                vals["against_walk|max"] = float(d / max(y, ab.FLOOR))
            figures[what] = {"arithmetic": arith, "values": vals}
            n += 1
        if which == "rw2" and D in (132, 400):
            # b2 is added by ONE slice: the scores move by exactly the change of b2 (to fp32 rounding of sums of this size) ...
            s0, s1 = direct_launch(data, b2=0.0), direct_launch(data, b2=0.75)
            tol = 64 * 2.0 ** -24 * max(1.0, float(np.abs(s1).max()))
            # ... and the launch clears the buffer its slices add into: what was there before is not part of the scores
            s2 = direct_launch(data, b2=0.75, prefill=1000.0)
            figures[f"{shape} b2 and memset"] = {"arithmetic": "f32", "values": {
                "equal_b2_once": bool(np.abs(s1 - s0 - 0.75).max() <= tol), "equal_buffer_cleared": bool(np.abs(s2 - s1).max() <= tol)}}
            n += 1
    for case in afu.KNOB_ROUND2.get(which, []):
        shape, runs = afu.run_second_round(lib, case, cus)
        for (kind, mma, z), f, figure in runs:
            forms_ok = forms_ok and (f["family"], afu.template(f), f["nsplit"]) == EXPECTED[which][shape[3]]
            figures[f"{case[0]} {shape} {kind} {afu.NAME_OF_MMA[mma]} z={z}"] = {"arithmetic": afu.NAME_OF_MMA[mma], "values": figure}
            n += 1
    print(json.dumps({"which": which, "forms_ok": bool(forms_ok), "expected": n, "figures": figures}), flush=True)


if __name__ == "__main__":
    main(*sys.argv[1:3])
