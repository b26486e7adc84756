"""GPU: every form the launches of the pointwise attention's backward can take (csrc/pwattn_bwd.hip bwd_dz_select / bwd_e_select with the
plan of csrc/capi.hip, csrc/pwattn_bwd_dp.hip pwattn_bwd_dp_select, csrc/pwattn_bwd_rw.hip pwattn_bwd_rw_select) is launched, is the form
the query nrm_pwattn_bwd_plan says it is at this device's own compute-unit count, and every gradient it contributes to is compared with
float64.

The cases live in tests/attention_bwd_forms_util.py; tests/test_attention_bwd_forms_cpu.py holds the set of forms they reach equal to
the set the selectors return, and the walks of several groups per wave reached at their edges.  Each case runs one backward through
ops.pointwise_attention_scores under its knobs and once more under the default plan (small launches: one group per wave, one trip):
  * against float64 under the error budget of tests/attention_budget.py, gates unchanged (plain bf16: the 1e-2 / 3e-2 bounds of
    tests/test_gpu_attention.py);
  * against the default plan, "the same products in another summation order": 2e-5 (fp32), 1e-4 (bf16x3), and for bf16 four times
    what two runs of the default plan differ by (attention_bwd_forms_util.WALK_TOL).
test_latched_knobs_in_a_child_process: NRM_BWD_RW=0 and NRM_DZ_NARROW=0, one fresh python child each (tests/attention_bwd_knob_worker.py)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import attention_budget as ab
import attention_bwd_forms_util as abu

pytestmark = pytest.mark.gpu
_record = []


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("NRM_BWD_FORMS_RECORD")          # a file: the worst budget ratio of every case of this module, for profiles/
    if path:
        head = {"M": dict(ab.M, **ab.PIECE_M), "bf16_bounds": [abu.BF16_FWD_TOL, abu.BF16_GRAD_TOL],
                "walk_tol": {abu.NAME_OF_MMA[k]: v for k, v in abu.WALK_TOL.items()},
                "default_spread": {a: max([r.get("default_spread", 0.0) for r in _record if f"-{a}-" in r["case"]], default=0.0) for a in abu.MMA_BY_NAME}}
        with open(path, "w") as f:                             # one case per line: a later recording diffs case by case
            f.write(json.dumps(head, indent=1)[:-2] + ',\n "runs": [\n')
            f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in _record))
            f.write("\n ]\n}\n")


@pytest.fixture
def cus(lib, monkeypatch):
    for k in abu.PER_LAUNCH:
        monkeypatch.delenv(k, raising=False)
    # the latched knobs were read at the first query or launch of this process: these tests describe the default dispatch
    assert abu.query(lib, abu.RW, 3, 5, 17, 64, 0, abu.BF16)["valid"] == 1 and abu.query(lib, abu.DZ, 2, 15, 200, 64)["narrowed"] == 1, \
        "run without NRM_BWD_RW / NRM_DZ_NARROW"
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.mark.parametrize("case", abu.CASES + abu.EXTRA_CASES, ids=abu.case_id)
def test_backward_form(lib, cus, case):
    _record.append(abu.summary(case, abu.run_case(lib, case, cus, measure_default_spread=bool(os.environ.get("NRM_BWD_FORMS_RECORD")))))


@pytest.mark.parametrize("which", sorted(abu.LATCHED_SETTINGS))
def test_latched_knobs_in_a_child_process(lib, cus, which):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in abu.KNOBS}
    env.update(abu.LATCHED_SETTINGS[which])
    pr = subprocess.run([sys.executable, os.path.join(here, "attention_bwd_knob_worker.py"), which], env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, (pr.returncode, pr.stdout.decode(errors="replace")[-2000:], pr.stderr.decode(errors="replace")[-3000:])
    res = json.loads(pr.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(res, indent=1))
    assert res["which"] == which and res["forms_ok"] is True, res
    assert len(res["runs"]) == len(abu.KNOB_CASES[which]) + len(abu.KNOB_WIDTH_CASES[which]) > 0
    _record.extend(dict(r, knob=which) for r in res["runs"])
