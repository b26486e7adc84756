"""CPU: nrm_pwattn_bwd_plan reports, without a kernel launch, what each launch of the pointwise attention's backward runs -- the dz pass,
a contraction pass with its plan and walk, the fp32 dP walk, the resident-W backward of the bf16 arithmetics -- with the host function the
launch itself switches on.  The production answers are pinned, bad arguments refused, and the set of forms the selectors can return --
under the default latched knobs and under each latched setting, one device-free child process each -- is held equal to the set the GPU
cases reach: the older lists of tests/test_gpu_attention.py and tests/test_gpu_dw_pack.py counted through the query, and the new lists of
tests/attention_bwd_forms_util.py.  Every walk of several groups per wave must be reached at its edges, and every new case must be needed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_bwd_forms_util as abu
from attention_bwd_forms_util import BF16, BF16X3, CONTRACT, DP, DZ, F32, RW

CUS = 256          # the closure is taken at the MI355X's compute-unit count; the GPU tests ask at the device's own


@pytest.fixture
def plans(lib, monkeypatch):
    for k in abu.PER_LAUNCH:
        monkeypatch.delenv(k, raising=False)
    # the latched knobs were read at the first query of this process: these tests describe the default dispatch
    assert abu.query(lib, RW, 3, 5, 17, 64, 0, BF16)["valid"] == 1 and abu.query(lib, DZ, 2, 15, 200, 64)["narrowed"] == 1, \
        "run without NRM_BWD_RW / NRM_DZ_NARROW"
    return lib


def _pick(f, *names):
    return tuple(f[n] for n in names)


def test_production_configurations(plans):
    """BASELINE configurations at 256 compute units: the launches of one backward, in order."""
    # C3 (fp32, D = 400): full-row dz pass, the dP walk in two N-chunks of 13 tiles over 3072 workgroups of 7 or 8 steps (a workgroup crosses
    # from one (row block, N-chunk) item into the next), then the packed one-accumulator dW_p pass: 80 splits of 192 groups on 5x5 tiles
    dz, dp, dw = abu.launches(plans, (512, 30, 50, 400), F32, True, CUS)
    assert _pick(dz, "family", "threads", "rows_class", "dz_format") == (1, 1024, 2, 0)
    assert _pick(dp, "NT", "nchunks", "kchunks", "steps", "grid", "max_steps", "max_items") == (13, 2, 25, 24000, 3072, 8, 2)
    assert _pick(dw, "family", "tile", "exact", "with_dw", "with_dt", "pack", "interleave", "nkw", "ndcol", "nsplit", "gps", "last_groups", "last_live") \
        == ("dw_direct", 5, 1, 1, 0, 2, 0, 5, 5, 80, 192, 192, 4)
    # ... the text+image attention (no row gradient wanted): the dz pass and the same dW_p pass
    assert [abu.key(f) for f in abu.launches(plans, (512, 30, 50, 400), F32, False, CUS)] == [abu.key(dz), abu.key(dw)]
    # C2 (bf16x3, D = 256): dz in the hl4 format, the resident-W backward in two reduction slices of 128 workgroups x 8 waves, 2048 tasks:
    # two trips; the 32-row dW_p pass, 128 splits of 120 groups
    dz, rw, dw = abu.launches(plans, (512, 30, 32, 256), BF16X3, True, CUS)
    assert _pick(dz, "family", "threads", "rows_class", "dz_format") == (1, 512, 2, 1)
    assert _pick(rw, "NG", "mma", "exact", "nks", "workgroups", "waves", "tsplit", "tasks", "rounds", "plain_dh") == (2, 2, 1, 2, 256, 8, 1, 2048, 2, 0)
    assert _pick(dw, "family", "tile", "exact", "mma", "hl4", "nsplit", "gps", "last_groups", "last_live") == ("dw_r32", 4, 1, 2, 1, 128, 120, 120, 4)
    # reference default (fp32, D = 64, 49 M z elements: the E-form): both serial passes on one exact 4x4 tile; the (b,h) pass has a short
    # last split and two live waves in its last workgroup
    dz, bt, bh = abu.launches(plans, (512, 15, 200, 64), F32, True, CUS)
    assert _pick(dz, "family", "threads", "rows_class") == (1, 1024, 2)
    assert _pick(bt, "family", "with_dw", "with_dt", "nsplit", "gps", "last_groups", "last_live", "G") == ("serial", 1, 1, 1920, 4, 4, 4, 7680)
    assert _pick(bh, "family", "with_dw", "with_dt", "nsplit", "gps", "last_groups", "last_live", "G") == ("serial", 0, 1, 11378, 9, 7, 2, 102400)
    # C5 (fp32, D = 768): narrowed dz slabs of 32 columns, the dP walk in four chunks of 12 tiles, the interleaved one-accumulator dW_p pass
    dz, dp, dw = abu.launches(plans, (64, 64, 128, 768), F32, True, CUS)
    assert _pick(dz, "family", "slab_cols", "slabs", "hchunk", "nhc", "big_lds", "narrowed") == (0, 32, 24, 128, 1, 0, 1)
    assert _pick(dp, "NT", "nchunks", "kchunks", "steps", "grid", "max_steps", "max_items") == (12, 4, 48, 32768, 3072, 11, 1)
    assert _pick(dw, "family", "tile", "pack", "interleave", "nkw", "ndcol", "nsplit", "gps", "last_groups", "last_live") == ("dw_direct", 4, 1, 1, 12, 12, 40, 103, 79, 4)
    assert abu.DP_MIN_ELEMS == __import__("news_recommendation_model_amd.ops", fromlist=["ops"]).DP_MIN_ELEMS


def test_the_plan_entry_agrees_with_the_older_entries(plans):
    for (T, H, D) in ((30, 50, 400), (7, 19, 72), (29, 7, 72), (15, 200, 64), (5, 33, 100), (5, 20, 64)):
        for mma in (F32, BF16, BF16X3):
            for p, fmt in ((1, 0), (2, 0), (4, 0), (4, 1)):
                old = plans.nrm_pwattn_bwd_form(T, H, D, p, mma, fmt)
                f = abu.query(plans, CONTRACT, 1, T, H, D, p, mma, fmt, CUS)
                if old == -1:
                    assert f is None or not f["valid"], (T, H, D, p, mma, fmt)
                    continue
                bits = (abu.E_FAMILIES.index(f["family"]) | (4 if f["exact"] else 0) | (8 if f["tile"] == 5 else 0) | (16 if f["with_dw"] else 0)
                        | (32 if f["with_dt"] else 0) | (64 if f["hl4"] else 0))
                assert bits == old, (T, H, D, p, mma, fmt)
    for B, T, H, D in ((3, 7, 18, 80), (3, 6, 17, 64), (2, 3, 13, 80)):
        for waves in (None, str(4 * abu.tiles(D))):
            with abu.env({"NRM_BT_WAVES": waves} if waves else {}):
                f = abu.query(plans, CONTRACT, B, T, H, D, 4, F32, 0, CUS)
                assert f["pack"] == plans.nrm_pwattn_bwd_dw_pack(B, T, H, D, 0) and f["nsplit"] == plans.nrm_pwattn_bwd_nsplit(B, T, H, D, 0)


def test_bad_arguments(plans):
    import ctypes
    out = (ctypes.c_int * abu.PLAN_LEN)()
    ask = plans.nrm_pwattn_bwd_plan
    good = dict(launch=CONTRACT, B=3, T=5, H=17, D=64, p=1, mma=0, fmt=0, cus=256)
    order = ("launch", "B", "T", "H", "D", "p", "mma", "fmt", "cus")
    assert ask(*[good[k] for k in order], out) == 0
    bad = [dict(launch=-1), dict(launch=4), dict(B=-1), dict(T=0), dict(H=0), dict(D=0), dict(D=66), dict(D=1028), dict(cus=-1),
           dict(B=1 << 20, T=1 << 10, H=1 << 10), dict(mma=3), dict(mma=-1), dict(p=0), dict(p=3), dict(p=5), dict(fmt=2),
           dict(p=1, mma=1, fmt=1), dict(p=4, mma=0, fmt=1), dict(p=2, mma=2, fmt=1),
           dict(launch=DZ, fmt=2), dict(launch=DZ, B=65536, T=1, H=1), dict(launch=RW, mma=3), dict(launch=RW, T=4096, H=4096, D=64, B=1),
           dict(launch=DP, T=4096, H=4096, D=64, B=1)]
    for change in bad:
        args = dict(good, **change)
        assert ask(*[args[k] for k in order], out) == -1, change
        assert plans.nrm_last_error().decode().startswith("nrm_pwattn_bwd_plan: "), (change, plans.nrm_last_error())
    assert ask(*[good[k] for k in order], None) == -1 and plans.nrm_last_error().decode().startswith("nrm_pwattn_bwd_plan: ")
    # a shape a launch does not take is no bad argument: valid = 0, as the _supported entries say
    assert abu.query(plans, RW, 3, 5, 17, 64, 0, F32)["valid"] == 0 and abu.query(plans, RW, 3, 5, 17, 260, 0, BF16)["valid"] == 0
    assert abu.query(plans, DP, 3, 5, 15, 64)["valid"] == 0 and abu.query(plans, DP, 3, 5, 16, 64)["valid"] == 1
    assert abu.query(plans, CONTRACT, 3, 5, 17, 64, 2, BF16, 0)["valid"] == 1 and abu.query(plans, CONTRACT, 0, 5, 17, 64, 1)["valid"] == 0
    # cus = 0: the current device's count, 256 where there is none
    import torch
    if not torch.cuda.is_available():
        assert abu.raw(plans, RW, 40, 9, 100, 64, 0, BF16, 0, 0) == abu.raw(plans, RW, 40, 9, 100, 64, 0, BF16, 0, 256)


def test_per_launch_knobs_are_read_at_every_call(plans, monkeypatch):
    fam = lambda *a: abu.query(plans, CONTRACT, *a, cus=CUS)["family"]          # noqa: E731
    assert fam(3, 29, 9, 80, 2) == "pipe" and fam(3, 7, 18, 80, 4) == "dw_direct" and fam(3, 7, 20, 64, 4, BF16, 1) == "dw_r32"
    for knob in ("NRM_BH_PIPE", "NRM_DW_DIRECT", "NRM_DW_R32"):
        monkeypatch.setenv(knob, "0")
    assert fam(3, 29, 9, 80, 2) == "serial" and fam(3, 7, 18, 80, 4) == "serial" and fam(3, 7, 20, 64, 4, BF16, 1) == "serial"
    f = abu.query(plans, CONTRACT, 3, 7, 18, 80, 1, cus=CUS)
    assert _pick(f, "nsplit", "gps", "interleave", "order") == (21, 1, 0, 0)
    monkeypatch.setenv("NRM_BT_WAVES", "8")
    monkeypatch.setenv("NRM_BT_INTERLEAVE", "1")
    monkeypatch.setenv("NRM_BT_ORDER", "1")
    f = abu.query(plans, CONTRACT, 3, 7, 18, 80, 1, cus=CUS)
    assert _pick(f, "nsplit", "gps", "last_groups", "last_live", "interleave", "order") == (7, 3, 3, 3, 1, 1)
    assert _pick(abu.query(plans, CONTRACT, 3, 7, 18, 80, 2, cus=CUS), "nsplit", "gps") == (54, 1)          # NRM_BH_WAVES is the (b,h) pass's
    monkeypatch.setenv("NRM_BH_WAVES", "4")
    monkeypatch.delenv("NRM_BH_PIPE")
    f = abu.query(plans, CONTRACT, 1, 29, 10, 72, 2, cus=CUS)              # the pipelined kernel honours neither the walk nor the order
    assert _pick(f, "family", "nsplit", "gps", "last_groups", "last_live", "interleave", "order") == ("pipe", 4, 3, 1, 4, 0, 0)
    assert abu.query(plans, DZ, 40, 5, 17, 256)["family"] == 1 and abu.query(plans, DZ, 3, 5, 17, 256)["family"] == 0
    monkeypatch.setenv("NRM_DZ_ROWS", "0")
    assert abu.query(plans, DZ, 40, 5, 17, 256)["family"] == 0
    monkeypatch.setenv("NRM_DZ_ROWS", "1")
    assert _pick(abu.query(plans, DZ, 3, 5, 17, 256), "family", "threads", "rows_class") == (1, 512, 1)
    assert _pick(abu.query(plans, DP, 2, 6, 50, 400), "grid", "max_steps", "max_items") == (6, 4, 2)      # 24 steps, four per workgroup, items of 6
    monkeypatch.setenv("NRM_DP_GRID", "1")
    assert _pick(abu.query(plans, DP, 2, 6, 50, 400), "grid", "max_steps", "max_items") == (1, 24, 4)
    f = abu.query(plans, RW, 5, 24, 100, 64, 0, BF16X3)                     # 35 tasks: cut while a part keeps eight candidates
    assert _pick(f, "workgroups", "waves", "tsplit", "tasks", "rounds", "plain_dh") == (14, 8, 3, 105, 1, 0)
    monkeypatch.setenv("NRM_BRW_WAVES", "1")
    monkeypatch.setenv("NRM_BRW_TSPLIT", "8")
    assert _pick(abu.query(plans, RW, 5, 24, 100, 64, 0, BF16X3), "workgroups", "waves", "tsplit", "tasks", "rounds") == (256, 1, 8, 280, 2)
    assert _pick(abu.query(plans, RW, 5, 24, 100, 64, 0, BF16X3, cus=304), "workgroups", "rounds") == (280, 1)
    monkeypatch.setenv("NRM_BRW_TSPLIT", "6")
    assert _pick(abu.query(plans, RW, 3, 24, 50, 256, 0, BF16), "nks", "workgroups", "tsplit", "tasks", "rounds") == (2, 256, 6, 144, 2)
    monkeypatch.setenv("NRM_BRW_TSPLIT", "99")
    assert abu.query(plans, RW, 3, 9, 17, 64, 0, BF16)["tsplit"] == 9                                         # at most T parts


def _lists(lib):
    """The case lists of the older GPU tests, taken from their modules."""
    import test_gpu_attention as tga
    import test_gpu_dw_pack as tdp
    fuzz_dp = []
    for s in tga._fuzz_shapes_dp():                          # (the test draws its NRM_DP_GRID from the shape's generator)
        B, T, H, D = s
        fuzz_dp.append((s, int(np.random.default_rng(B * 100003 + T * 1009 + H * 31 + D).integers(1, 40))))
    par = lambda fn: {m.args[0]: m.args[1] for m in fn.pytestmark if m.name == "parametrize"}["B,T,H,D"]          # noqa: E731
    assert par(tga.test_scores_and_grads_match_oracle) == tga.SHAPES + tga.PIPE_RAGGED_SHAPES
    assert par(tga.test_random_shapes_match_oracle) == tga._fuzz_shapes() and par(tga.test_random_shapes_match_oracle_bf16x3) == tga._fuzz_shapes(16, 7)
    assert par(tga.test_interleaved_group_walk_matches_oracle) == tga.INTERLEAVED_SHAPES
    return dict(SHAPES=tga.SHAPES, PIPE_RAGGED_SHAPES=tga.PIPE_RAGGED_SHAPES, FUZZ=tga._fuzz_shapes(), BF16_SHAPES=tga.BF16_SHAPES,
                BF16_E_EXACT_SHAPES=tga.BF16_E_EXACT_SHAPES, FUZZ_BF16X3=tga._fuzz_shapes(n=16, seed=7), DZ_ROWS_SHAPES=tga.DZ_ROWS_SHAPES,
                DP_SHAPES=tga.DP_SHAPES, FUZZ_DP=fuzz_dp, DIRECT_DW_SHAPES=par(tga.test_direct_dw_pass_matches_oracle_and_e_form),
                BATCH32_SHAPES=par(tga.test_default_dispatch_at_batch_32_matches_oracle), DW_PACK_SHAPES=tdp.SHAPES,
                INTERLEAVED_SHAPES=tga.INTERLEAVED_SHAPES, INTERLEAVED_FORCED=tga.INTERLEAVED_FORCED,
                dp_supported=lambda s: bool(lib.nrm_pwattn_bwd_dp_supported((s[3] + 3) // 4 * 4, s[2])))


def test_what_the_older_lists_left_untested(plans):
    """The gap this file's GPU cases close, recorded: over SHAPES, PIPE_RAGGED_SHAPES, BF16_SHAPES, BF16_E_EXACT_SHAPES, DP_SHAPES,
    DZ_ROWS_SHAPES and the fuzz lists of tests/test_gpu_attention.py the fp32 contraction passes walk more than one group per wave at two
    shapes only, never on 5x5 tiles; the bf16 arithmetics reach two groups at three; the pipelined kernel has two groups in flight at one,
    and no resident-W backward makes a second trip.  (The batch-32 test adds 2 and 3 groups per wave on the serial passes at (32, 6, 16, 400) and
    (33, 5, 50, 256); tests/test_gpu_dw_pack.py forces four splits on the dW_p-only pass.)"""
    lists = _lists(plans)
    before = [c for c in abu.older_cases(lists) if c[0].split()[0] in ("scores_and_grads", "bf16", "fuzz_bf16x3", "dz_rows", "dp", "fuzz_dp")]
    seen = {}
    for case in before:
        for f in abu.case_forms(plans, case, CUS):
            if f["launch"] == CONTRACT and f["gps"] > 1 and f["mma"] == F32:
                seen.setdefault(case[1], set()).add((f["pass"], f["tile"], f["gps"]))
            assert f["launch"] != RW or f["rounds"] == 1, case[0]
    assert seen == {(1, 64, 128, 768): {(1, 4, 6), (4, 4, 6), (2, 4, 2)}, (4, 3, 6, 1024): {(1, 4, 2)}}
    bf = {case[1] for case in before if case[2] != F32 for f in abu.case_forms(plans, case, CUS) if f["launch"] == CONTRACT and f["gps"] > 1}
    assert bf == {(2, 30, 50, 400), (1, 64, 128, 768), (4, 3, 6, 1024)} and all(          # ((8, 2, 43, 400) would: its fuzz test is fp32 only)
       
        f["gps"] == 2 for case in before if case[2] != F32 and case[1] != (1, 64, 128, 768)
        for f in abu.case_forms(plans, case, CUS) if f["launch"] == CONTRACT and f["gps"] > 1)
    # the pipelined kernel had two groups in flight at one shape only: even ranges of 2 on exact 4x4 tiles -- never its odd tail, never 5x5
    pipe = {(c[1], f["tile"], f["exact"], f["gps"], f["last_groups"]) for c in before for f in abu.case_forms(plans, c, CUS)
            if f["launch"] == CONTRACT and f["family"] == "pipe" and f["gps"] > 1}
    assert pipe == {((1, 64, 128, 768), 4, 1, 2, 2)}


SWEEP_SHARES = 4          # device-free child processes the default sweep is dealt to (they run beside the two latched ones)


def _start(args, settings):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in abu.KNOBS}
    env.update(settings)
    return subprocess.Popen([sys.executable, os.path.join(here, "attention_bwd_forms_util.py"), *args], env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)


def _join(pr, which):
    out, err = pr.communicate(timeout=600)
    assert pr.returncode == 0, (pr.returncode, err.decode(errors="replace")[-3000:])
    res = json.loads(out.decode().strip().splitlines()[-1])
    assert res["which"] == which
    return res


@pytest.fixture(scope="module")
def children(lib):
    """The sweeps, each in a device-free child process (ctypes only), all at once: SWEEP_SHARES shares of the default sweep and one child per
    latched setting.  -> (forms of the default sweep, {setting: (forms its sweep finds, {i: forms its cases reach without case i; -1: all
    cases}, forms of its width cases)})"""
    shares = [_start(["sweep", str(i), str(SWEEP_SHARES)], {}) for i in range(SWEEP_SHARES)]
    knobs = {which: _start([which], abu.LATCHED_SETTINGS[which]) for which in abu.LATCHED_SETTINGS}
    possible = set()
    for pr in shares:
        possible |= {abu._key_of_json(k) for k in _join(pr, "sweep")["possible"]}
    latched = {}
    for which, pr in knobs.items():
        res = _join(pr, which)
        latched[which] = ({abu._key_of_json(k) for k in res["possible"]}, {int(i): {abu._key_of_json(k) for k in ks} for i, ks in res["reached"].items()},
                          [[abu._key_of_json(k) for k in ks] for ks in res["width"]])
    return possible, latched


@pytest.fixture(scope="module")
def latched(children):
    return children[1]


@pytest.fixture(scope="module")
def default_side(lib, children):
    """(forms the sweep finds, (forms, walk edges) the older tests reach) under the default latched knobs: computed once."""
    for k in abu.PER_LAUNCH:
        assert k not in os.environ, k
    lists = _lists(lib)
    older = abu.older_cases(lists) + abu.interleaved_cases(lib, lists["INTERLEAVED_FORCED"])
    return children[0], abu.reached(lib, older, CUS)


def _closure(lib, default_side, latched, skip=None, skip_knob=(None, -1)):
    """(possible, reached forms, reached walk edges); ``skip``: a case of CASES left out, ``skip_knob``: (setting, index into KNOB_CASES)."""
    possible, (older_keys, older_edges) = default_side
    possible = set(possible)
    keys, edges = abu.reached(lib, abu.CASES, CUS, skip=skip)
    keys, edges = set(keys) | set(older_keys), set(edges) | set(older_edges)
    for which, (poss_l, reached_l, _width) in latched.items():
        possible |= poss_l
        keys |= reached_l[skip_knob[1] if which == skip_knob[0] else -1]
    return possible, keys, edges


def test_latched_settings_select_what_they_are_for(plans, default_side, latched):
    # NRM_BWD_RW=0: no resident-W backward and no hl4 dz; the bf16 arithmetics' row gradients come from the E-form passes at every width
    poss, _r, width = latched["rw0"]
    assert not [k for k in poss if k[0] == "rw" or (k[0] == "contract" and k[7]) or (k[0] == "dz" and k[4])]
    assert all([k[1:8] for k in ks if k[0] == "contract"] == [("serial", 4, e, m, 1, 1, 0), ("serial", 4, e, m, 0, 1, 0)]
               for ks, (e, m) in zip(width, ((1, 2), (0, 2), (1, 1), (0, 1))))
    assert all(k[-1] for ks in width for k in ks if k[0] == "contract")                   # ... over several groups per wave
    # NRM_DZ_NARROW=0: no narrowed slab; a wide slab of a long history needs more than 64 KB
    poss, _r, width = latched["narrow0"]
    big = ("dz", 0, 256, 0, 0, False, 1, 0)                   # one history chunk, more than 64 KB, not narrowed
    assert not [k for k in poss if k[7]] and big in poss and big not in default_side[0]
    assert width == [[("dz", 0, 256, 0, 0, False, 0, 0), ("contract", "serial", 4, 1, 0, 1, 1, 0, 1, 0, False),
                      ("contract", "serial", 4, 1, 0, 0, 1, 0, 1, 0, False)]]
    assert abu.key(abu.query(plans, DZ, 2, 15, 200, 64)) == ("dz", 0, 256, 0, 0, False, 0, 1)


def test_every_form_the_selectors_return_has_a_gpu_case(plans, default_side, latched):
    possible, keys, edges = _closure(plans, default_side, latched)
    not_run = set(abu.NOT_RUN)
    assert not_run <= possible and not (not_run & keys) and len(not_run) <= 0.05 * len(possible)
    assert all(isinstance(why, str) and why for why in abu.NOT_RUN.values())
    assert possible - keys - not_run == set(), "forms without a GPU case"
    assert keys - possible == set(), "forms the sweep does not find: widen the sweep"
    # every walk of several groups per wave is reached with a short last split and with a last workgroup of fewer than four live waves; the
    # pipelined kernel, which takes two groups per trip, with ranges of an odd and of an even number of groups, on both tile shapes
    missing = abu.required_walk_features(possible - not_run) - edges
    assert missing == set(), "walk edges without a GPU case"
    pipe = {k for k in possible if k[0] == "contract" and k[1] == "pipe" and k[-1]}
    assert {k[2] for k in pipe} == {4, 5} and {k[3] for k in pipe} == {0, 1}
    # what the set is today
    count = lambda kind: len({k for k in possible if k[0] == kind})          # noqa: E731
    assert (count("contract"), count("dz"), count("dp"), count("rw"), len(default_side[0])) == (152, 17, 14, 40, 222), \
        [count(k) for k in ("contract", "dz", "dp", "rw")]
    # the extra cases add nothing the closure counts: they pin the walks at further shapes
    extra_keys, extra_edges = abu.reached(plans, abu.EXTRA_CASES, CUS)
    assert set(extra_keys) <= keys and set(extra_edges) <= edges


def test_every_case_reaches_what_its_tag_promises(plans):
    ids = [abu.case_id(c) for c in abu.CASES + abu.EXTRA_CASES]
    assert len(set(ids)) == len(ids)
    for case in abu.CASES + abu.EXTRA_CASES:
        assert abu.promise(case, abu.case_forms(plans, case, CUS)) is None, abu.case_id(case)
    # the shapes the rounds of the resident-W backward are built on, at 256 compute units
    with abu.env(abu.resolve(abu.E(BRW_WAVES="1", TSPLIT="r2"), (5, 24, 100, 64), BF16X3, plans, CUS)):
        assert os.environ["NRM_BRW_TSPLIT"] == "8" and abu.query(plans, RW, 5, 24, 100, 64, 0, BF16X3)["tasks"] == 280
    with abu.env(abu.resolve(abu.E(BRW_WAVES="1", TSPLIT="r2"), (3, 24, 50, 256), BF16, plans, CUS)):
        assert os.environ["NRM_BRW_TSPLIT"] == "6" and _pick(abu.query(plans, RW, 3, 24, 50, 256, 0, BF16), "tasks", "workgroups") == (144, 256)


def test_every_new_gpu_case_is_needed(plans, default_side, latched):
    """Sensitivity of the closure: with any ONE case taken out of CASES / KNOB_CASES a form, or an edge of a walk, is left without a case."""
    def complete(**skip):
        possible, keys, edges = _closure(plans, default_side, latched, **skip)
        return possible - keys - set(abu.NOT_RUN) == set() and abu.required_walk_features(possible) - edges == set()

    assert complete()
    for case in abu.CASES:
        assert not complete(skip=case), ("the closure does not need", abu.case_id(case))
    for which in abu.LATCHED_SETTINGS:
        for i, case in enumerate(abu.KNOB_CASES[which]):
            assert not complete(skip_knob=(which, i)), ("the closure does not need", which, abu.case_id(case))
