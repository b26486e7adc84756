"""Child process of tests/test_gpu_attention_bwd_forms.py::test_latched_knobs_in_a_child_process: the backward forms behind knobs that are
read once per process.  The parent sets the environment; this script checks with nrm_pwattn_bwd_plan that the knob selects the forms it is
for, runs the cases of tests/attention_bwd_forms_util.py KNOB_CASES and KNOB_WIDTH_CASES exactly as the parent runs its own (float64
budget, the default plan of the same process) and prints ONE JSON line {"which", "forms_ok", "runs": [record line per case]}.  A case over
a gate ends the script with its assertion.

    python tests/attention_bwd_knob_worker.py rw0        (NRM_BWD_RW=0: the bf16 arithmetics at D <= 256 through the E-form passes 1 and 2)
    python tests/attention_bwd_knob_worker.py narrow0    (NRM_DZ_NARROW=0: the dz slabs keep their width for long histories)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch                # noqa: E402

import attention_bwd_forms_util as abu                           # noqa: E402
from news_recommendation_model_amd import native                 # noqa: E402


def expected(which, case, forms):
    """What the setting is for, at this case."""
    con = [f for f in forms if f["launch"] == abu.CONTRACT]
    if which == "rw0":           # no resident-W backward, fp32 dz, the dt and the dh pass on the serial kernel
        return (not [f for f in forms if f["launch"] == abu.RW] and forms[0]["dz_format"] == abu.DZ_F32
                and [(f["pass"], f["family"], f["with_dt"], f["hl4"]) for f in con] == [(1, "serial", 1, 0), (2, "serial", 1, 0)])
    return forms[0]["family"] == 0 and forms[0]["narrowed"] == 0


def main(which):
    lib = native.load()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    forms_ok, runs = True, []
    for case in abu.KNOB_CASES[which] + abu.KNOB_WIDTH_CASES[which]:
        forms_ok = forms_ok and bool(expected(which, case, abu.case_forms(lib, case, cus)))
        runs.append(abu.summary(case, abu.run_case(lib, case, cus)))
    print(json.dumps({"which": which, "forms_ok": forms_ok, "runs": runs}), flush=True)


if __name__ == "__main__":
    for k in abu.PER_LAUNCH:
        os.environ.pop(k, None)
    main(sys.argv[1])
