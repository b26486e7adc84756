"""Child process of tests/test_gpu_attention_fwd_forms.py::test_latched_knobs_in_a_child_process: the forward forms behind the knob that is
read once per process.  The parent sets the environment; this script checks with nrm_pwattn_fwd_form that the knob selects the forms it is
for, runs the cases of tests/attention_fwd_forms_util.py KNOB_CASES against float64 and prints ONE JSON line
{"which", "forms_ok", "expected", "figures": {launch: {"arithmetic", "values": {name: figure}}}}.  The gates are the parent's.

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
from attention_fwd_forms_util import BF16                        # noqa: E402
from news_recommendation_model_amd import native                # noqa: E402

# what each setting is for: (family, template parameters, column slices) by width, dense or ragged alike
EXPECTED = {
    "walk0": {64: ("rw_tile", (4,), 1), 128: ("rw_tile", (8,), 1), 256: ("rw_tile", (8,), 2)},
}


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
    for case in afu.KNOB_ROUND2.get(which, []):
        shape, runs = afu.run_second_round(lib, case, cus)
        for (kind, mma, z), f, figure in runs:
            forms_ok = forms_ok and (f["family"], afu.template(f), f["nsplit"]) == EXPECTED[which][shape[3]]
            figures[f"{case[0]} {shape} {kind} {afu.NAME_OF_MMA[mma]} z={z}"] = {"arithmetic": afu.NAME_OF_MMA[mma], "values": figure}
            n += 1
    print(json.dumps({"which": which, "forms_ok": bool(forms_ok), "expected": n, "figures": figures}), flush=True)


if __name__ == "__main__":
    main(*sys.argv[1:3])
