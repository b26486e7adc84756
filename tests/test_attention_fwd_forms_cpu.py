"""CPU: nrm_pwattn_fwd_form reports, without a kernel launch, which forward kernel of the pointwise attention a launch of nrm_pwattn_fwd /
_fwd_ragged / _fwd_hragged takes -- the selector the launches themselves switch on (csrc/pwattn_fwd.hip pwattn_fwd_select,
csrc/pwattn_fwd_rw.hip pwattn_fwd_rw_select).  The production answers are pinned, bad arguments refused, the per-launch knobs honoured
at every call, and the set of forms the selector can return -- under the default latched knob and under its other setting, in a
device-free child process -- is held equal to the set the GPU cases of tests/attention_fwd_forms_util.py reach."""
import json
import os
import subprocess
import sys

import pytest

import attention_fwd_forms_util as afu
from attention_fwd_forms_util import BF16, BF16X3, F32

CUS = 256          # the closure is taken at the MI355X's compute-unit count; the GPU tests ask at the device's own


@pytest.fixture
def forms(lib, monkeypatch):
    for k in afu.PER_LAUNCH:
        monkeypatch.delenv(k, raising=False)
    # the latched knobs were read at the first query of this process: these tests describe the default dispatch
    probe = [afu.dense_query(lib, (3, 5, 17, D), mma, 1, CUS) for D, mma in ((64, F32), (400, F32), (64, BF16))]
    assert [(f["family"], afu.template(f)) for f in probe] == [("walk_f32", (4,)), ("stream", (13, 1, 4, 1, 4)), ("walk_bf16", (4, 2))], \
        "run without NRM_FWD_WALK"
    return lib


def _pick(f, *names):
    return tuple(f[n] for n in names)


def test_production_configurations(forms):
    """BASELINE configurations at 256 compute units."""
    q = lambda *a, **k: afu.query(forms, *a, cus=CUS, **k)          # noqa: E731
    # C3: D = 400 fp32 -> two chunks of <13,1>, four waves per SIMD, the compact candidate image; 64-row workgroups
    f = q(512, 30, 50, 400, F32, 1)
    assert f["valid"] and f["family"] == "stream" and afu.template(f) == (13, 1, 4, 1, 4) and f["nchunks"] == 2
    assert _pick(f, "tasks", "workgroups", "rounds", "nsplit", "tsplit") == (12000, 12000, 1, 1, 1)
    # C2: D = 256 bf16x3 -> the walk <8,8> in two slices of 128 persistent workgroups; 512 x 2 tasks fill two rounds without a cut
    f = q(512, 30, 32, 256, BF16X3, 1)
    assert f["family"] == "walk_bf16" and afu.template(f) == (8, 8) and _pick(f, "nsplit", "workgroups", "tsplit", "tasks", "rounds") == (2, 256, 2, 2048, 2)
    # reference default: D = 64 fp32 -> the fp32 walk <4>, two 8-wave workgroups per compute unit; 512 x 13 tasks are cut in two to fill two
    # rounds of 4096 (a part keeps 7 >= 4 candidates): the production launch goes round four times
    f = q(512, 15, 200, 64, F32, 1)
    assert f["family"] == "walk_f32" and afu.template(f) == (4,) and _pick(f, "nsplit", "workgroups", "tsplit", "tasks", "rounds") == (1, 512, 2, 13312, 4)
    # C5: D = 768 fp32 -> three chunks of <16,1>, the per-row image
    f = q(64, 64, 128, 768, F32, 1)
    assert f["family"] == "stream" and afu.template(f) == (16, 1, 2, 0, 4) and f["nchunks"] == 3 and f["tasks"] == 64 * 64 * 128 // 64
    # compact scoring at C3: ragged lists and ragged histories keep the dense plan; at D = 64 they walk
    for ragged, T_or_Mt in ((1, 0), (2, 9000 * 4)):
        f = q(512, T_or_Mt, 50, 400, F32, 0, ragged, N=9000, max_count=30, k_max=50)
        assert f["valid"] and f["family"] == "stream" and afu.template(f) == (13, 1, 4, 1, 4) and f["ragged"] == ragged
        f = q(512, T_or_Mt, 200, 64, F32, 0, ragged, N=9000, max_count=30, k_max=200)
        assert f["valid"] and f["family"] == "walk_f32" and afu.template(f) == (4,) and f["tasks"] == 512 * 13 * 2 and f["tsplit"] == 2      # (mean list: 18)
    assert q(512, 0, 50, 400, F32, 0, 1, N=9000, max_count=30)["tasks"] == (9000 * 50 + 63) // 64
    assert q(512, 36000, 0, 400, F32, 0, 2, N=9000, max_count=30, k_max=50)["tasks"] == 36000 * 16 // 64
    # a history plan whose longest kept history is shorter than a tile keeps the per-row image
    assert afu.template(q(512, 9000, 0, 400, F32, 0, 2, N=9000, max_count=30, k_max=15)) == (13, 1, 3, 0, 4)


def test_selections_without_a_kernel(forms):
    q = lambda *a, **k: afu.query(forms, *a, cus=CUS, **k)          # noqa: E731
    for ragged, T in ((1, 0), (2, 40)):
        assert q(3, T, 17, 64, F32, 0, ragged, N=10, max_count=5, k_max=17)["valid"] == 1
        for mma in (BF16, BF16X3):                               # the ragged forms have fp32 arithmetic only
            for D in (64, 400):
                assert q(3, T, 17, D, mma, 0, ragged, N=10, max_count=5, k_max=17)["valid"] == 0
        for D in (64, 400):                                       # ... and store no z
            assert q(3, T, 17, D, F32, 1, ragged, N=10, max_count=5, k_max=17)["valid"] == 0
    # every width the entries accept has a bf16 and a bf16x3 forward (one 16-column slice of W_p fits the LDS up to D = 1024)
    assert all(q(3, 5, 17, D, mma, 1)["valid"] == 1 for D in afu.SWEEP_D if D <= 1024 for mma in (BF16, BF16X3))


def test_every_history_ragged_selection_has_a_kernel(forms):
    """A history-ragged workgroup of the streaming kernel holds NW * MT <= 16 row tiles (its compact image has 16 rows): 8 at <14,2>, 4
    otherwise -- every plan passes, so no width and no k_max reaches a selection without a kernel
    from ops.attend_pool_hragged.  Pinned over every width the entry accepts, both sides of k_max = 16, both candidate images."""
    for ct in (None, "0", "1"):
        with afu.env({} if ct is None else {"NRM_FWD_CT": ct}):
            for D in range(4, 1025, 4):
                for k_max in (1, 15, 16, 17, 200):
                    f = afu.query(forms, 3, 15 * ((k_max + 15) // 16), 0, D, F32, 0, 2, N=15, max_count=5, k_max=k_max, cus=CUS)
                    assert f is not None and f["valid"] == 1, (D, k_max, ct)
                    assert f["family"] != "stream" or f["NW"] * f["MT"] <= 16, (D, k_max, f)
    got = {D: afu.template(afu.query(forms, 3, 30, 0, D, F32, 0, 2, N=15, max_count=5, k_max=17, cus=CUS)) for D in (212, 224, 420, 448)}
    assert got == {D: (14, 2, 2, 0, 4) for D in got}          # (the 14 x 2 plan: 209..224 and 417..448)


def test_bad_arguments(forms):
    import ctypes
    out = (ctypes.c_int * len(afu.FIELDS))()
    ask = forms.nrm_pwattn_fwd_form
    good = dict(B=3, T=5, H=17, D=64, mma=0, save_z=1, ragged=0, N=0, max_count=0, k_max=0, cus=256)
    order = ("B", "T", "H", "D", "mma", "save_z", "ragged", "N", "max_count", "k_max", "cus")
    assert ask(*[good[k] for k in order], out) == 0
    bad = [dict(B=-1), dict(T=0), dict(H=0), dict(D=0), dict(D=66), dict(D=1028), dict(mma=3), dict(mma=-1), dict(save_z=2), dict(ragged=3),
           dict(ragged=-1), dict(cus=-1), dict(B=1 << 20, T=1 << 10, H=1 << 10),
           dict(ragged=1, N=-1), dict(ragged=1, N=5, max_count=6), dict(ragged=1, N=5, max_count=-1), dict(ragged=1, H=0), dict(ragged=1, D=6),
           dict(ragged=2, T=-1, N=5, max_count=5), dict(ragged=2, N=5, max_count=5, k_max=-1), dict(ragged=2, T=1 << 27, N=5, max_count=5)]
    for change in bad:
        args = dict(good, **change)
        assert ask(*[args[k] for k in order], out) == -1, change
        assert forms.nrm_last_error().decode().startswith("nrm_pwattn_fwd_form: "), (change, forms.nrm_last_error())
    assert ask(*[good[k] for k in order], None) == -1 and forms.nrm_last_error().decode().startswith("nrm_pwattn_fwd_form: ")
    # nothing to launch is no error: tasks = 0
    assert afu.query(forms, 0, 5, 17, 64)["tasks"] == 0
    assert afu.query(forms, 3, 0, 17, 64, F32, 0, 1, N=0, max_count=0)["tasks"] == 0
    # cus = 0: the current device's count, 256 where there is none -- the same answer as cus = 256 on a machine without a GPU
    import torch
    if not torch.cuda.is_available():
        assert afu.query(forms, 17, 31, 125, 124, cus=0) == afu.query(forms, 17, 31, 125, 124, cus=256)


def test_per_launch_knobs_are_read_at_every_call(forms, monkeypatch):
    t = lambda *a, **k: (lambda f: (f["family"], afu.template(f)))(afu.query(forms, *a, cus=CUS, **k))          # noqa: E731
    assert t(3, 5, 17, 400) == ("stream", (13, 1, 4, 1, 4)) and t(3, 5, 7, 400) == ("stream", (13, 1, 3, 0, 4))
    monkeypatch.setenv("NRM_FWD_CT", "0")
    assert t(3, 5, 17, 400) == ("stream", (13, 1, 3, 0, 4))
    monkeypatch.setenv("NRM_FWD_CT", "1")
    assert t(3, 5, 7, 400) == ("stream", (13, 1, 4, 1, 4)) and t(3, 5, 4, 400) == ("stream", (13, 1, 3, 0, 4))      # (63 / 4 + 2 > 16 image rows)
    assert t(3, 5, 17, 768) == ("stream", (16, 1, 2, 0, 4))                                                        # no compact image on 16 tiles
    monkeypatch.delenv("NRM_FWD_CT")
    assert t(3, 5, 17, 64) == ("walk_f32", (4,)) and t(3, 5, 17, 128) == ("rw_tile", (8,))
    monkeypatch.setenv("NRM_FWD_WALK_F32", "0")
    assert t(3, 5, 17, 64) == ("rw_tile", (4,))
    monkeypatch.setenv("NRM_FWD_WALK_F32", "1")
    assert t(3, 5, 17, 64) == ("walk_f32", (4,)) and t(3, 5, 17, 128) == ("walk_f32", (8,)) and t(3, 5, 17, 124) == ("rw_tile", (8,))
    monkeypatch.delenv("NRM_FWD_WALK_F32")
    f = afu.query(forms, 3, 30, 17, 64, cus=CUS)
    assert (f["tsplit"], f["tasks"]) == (7, 42)                   # six tasks: cut while a part keeps four candidates (30 / 7 = 4, 30 / 8 = 3 < 4)
    for v, want in (("15", 15), ("64", 30), ("0", 1), ("-3", 1)):
        monkeypatch.setenv("NRM_FWD_TSPLIT", v)
        f = afu.query(forms, 3, 30, 17, 64, cus=CUS)
        assert (f["tsplit"], f["tasks"]) == (want, 6 * want), v
        assert afu.query(forms, 3, 30, 17, 64, BF16, cus=CUS)["tsplit"] == want
        assert afu.query(forms, 3, 30, 17, 400, cus=CUS)["tsplit"] == 1          # not a walk
    monkeypatch.setenv("NRM_FWD_TSPLIT", "9")                     # a ragged walk is cut into at most max_count parts
    assert afu.query(forms, 3, 0, 17, 64, F32, 0, 1, N=12, max_count=5, cus=CUS)["tsplit"] == 5


def test_rounds_follow_the_compute_unit_count(forms):
    """rounds = ceil(tasks / (workgroups per slice x waves)): the table of DESIGN.md ('one round holds')."""
    rounds = lambda cus, *a, **k: afu.query(forms, *a, cus=cus, **k)["rounds"]          # noqa: E731
    assert rounds(256, 1, 1, 65536, 124) == 1 and rounds(256, 1, 1, 65537, 124) == 2          # fp32 tiles: 256 x 16 tiles of 16 rows
    assert rounds(256, 1, 1, 13056, 400, BF16X3) == 1 and rounds(256, 1, 1, 13057, 400, BF16X3) == 2      # 5 slices, 51 workgroups
    assert rounds(256, 128, 1, 256, 64, BF16) == 1 and rounds(256, 129, 1, 256, 64, BF16) == 2             # 2048 walk tasks
    assert rounds(256, 64, 1, 256, 256, BF16X3) == 1 and rounds(256, 65, 1, 256, 256, BF16X3) == 2         # 2 slices: 1024
    assert rounds(256, 256, 1, 256, 64) == 1 and rounds(256, 257, 1, 256, 64) == 2                         # fp32 walk: 4096
    assert rounds(64, 1, 1, 16385, 124) == 2 and rounds(304, 1, 1, 65537, 124) == 1
    assert rounds(256, 512, 30, 50, 400) == 1                                                               # the streaming kernel does not loop


def test_older_case_lists_are_those_of_their_modules(forms):
    import test_gpu_attention as tga
    import test_gpu_attention_budget as tgb
    import test_gpu_compact as tgc
    import test_gpu_history_compact as tgh
    assert afu.OLD_F32_SHAPES == list(dict.fromkeys(tga.SHAPES + tga.PIPE_RAGGED_SHAPES + tga.DP_SHAPES))
    assert set(afu.OLD_F32_SHAPES) == set(tgb.ALL_F32_SHAPES + tga.PIPE_RAGGED_SHAPES)
    assert [f for f in tgb.F32_FORMS.values() if any(k in afu.PER_LAUNCH for k in f)] == afu.OLD_F32_ENVS[1:]
    assert afu.OLD_BF16_SHAPES == list(dict.fromkeys(tga.BF16_SHAPES + tga.BF16_E_EXACT_SHAPES + tgb.ALL_BF16X3_SHAPES))
    walk = [m.args[1] for m in tga.test_fp32_walk_forward_matches_oracle_and_tile_form.pytestmark if m.name == "parametrize"]
    ct = [m.args[1] for m in tga.test_compact_candidate_image_is_bit_identical.pytestmark if m.name == "parametrize"]
    assert walk == [afu.OLD_WALK_SHAPES] and ct == [afu.OLD_CT_SHAPES]
    assert sorted(afu.OLD_RAGGED_CASES, key=repr) == sorted(tgc.ATTN_CASES.values(), key=repr)
    assert sorted(afu.OLD_HRAGGED_CASES, key=repr) == sorted(tgh.ATTN_CASES.values(), key=repr)


def _child(which):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in afu.KNOBS}
    env.update(afu.LATCHED_SETTINGS[which])
    pr = subprocess.run([sys.executable, os.path.join(here, "attention_fwd_forms_util.py"), which], env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode == 0, (pr.returncode, pr.stderr.decode(errors="replace")[-3000:])
    res = json.loads(pr.stdout.decode().strip().splitlines()[-1])
    assert res["which"] == which
    return ({afu._key_of_json(k) for k in res["possible"]}, {int(i): {afu._key_of_json(k) for k in ks} for i, ks in res["reached"].items()})


@pytest.fixture(scope="module")
def latched(lib):
    """{setting: (forms the sweep finds, {i: forms its cases reach without case i; -1: all cases})} from one device-free child process each."""
    return {which: _child(which) for which in afu.LATCHED_SETTINGS}


@pytest.fixture(scope="module")
def default_side(lib):
    """(forms the sweep finds, forms the older tests reach) under the default latched knobs: computed once."""
    for k in afu.PER_LAUNCH:
        assert k not in os.environ, k
    return set(afu.sweep(lib, CUS)), set(afu.reached_by_older_tests(lib, CUS))


def _closure(forms, default_side, latched, skip=None, skip_knob=(None, -1)):
    """(possible, reached) over the default dispatch and the latched setting; ``skip``: a case of SMALL_CASES / ROUND2_CASES left out,
    ``skip_knob``: (setting, index into its KNOB_CASES + KNOB_ROUND2) left out."""
    possible, older = default_side
    possible = set(possible)
    reached = older | set(afu.reached_by_new_tests(forms, CUS, skip=skip))
    for which, (poss_l, reached_l) in latched.items():
        possible |= poss_l
        reached |= reached_l[skip_knob[1] if which == skip_knob[0] else -1]
    return possible, reached


def test_latched_settings_select_what_they_are_for(default_side, latched):
    fam = lambda which, name, mma=F32: {k[1] for k in latched[which][0] if k[0] == name and k[2] == mma}          # noqa: E731
    assert not fam("walk0", "walk_bf16", BF16) and not fam("walk0", "walk_bf16", BF16X3) and fam("walk0", "walk_f32") == {(4,), (8,)}


def test_every_form_the_selector_returns_has_a_gpu_case(forms, default_side, latched):
    possible, reached = _closure(forms, default_side, latched)
    not_run = set(afu.NOT_RUN)
    assert not_run <= possible and not (not_run & reached) and len(not_run) <= 0.05 * len(possible)
    assert all(isinstance(why, str) and why for why in afu.NOT_RUN.values())
    assert possible - reached - not_run == set(), "forms without a GPU case"
    assert reached - possible == set(), "forms the sweep does not find: widen the sweep"
    # what the set is today
    fam = lambda name: {k for k in possible if k[0] == name}          # noqa: E731
    assert {k[1] for k in fam("stream")} == {(10, 1, 3, 0, 4), (10, 1, 4, 1, 4), (12, 1, 3, 0, 4), (12, 1, 4, 1, 4), (13, 1, 3, 0, 4), (13, 1, 4, 1, 4),
                                             (14, 2, 2, 0, 4), (16, 1, 2, 0, 4), (20, 1, 2, 0, 4)}
    assert {k[1] for k in fam("rw_tile")} == {(n,) for n in (1, 2, 3, 4, 5, 6, 8)}
    assert {k[1] for k in fam("walk_bf16")} == {(4, 2), (8, 4), (8, 8)} and {k[1] for k in fam("walk_f32")} == {(4,), (8,)}
    assert all(not k[7] for k in fam("stream")) and all(k[2] == F32 for k in fam("stream") | fam("walk_f32"))
    assert len(default_side[0]) == 268 and len(possible) == 268          # NRM_FWD_WALK=0 selects forms that also run by default at other widths


def test_every_new_gpu_case_is_needed(forms, default_side, latched):
    """Sensitivity of the closure: with any ONE new case taken out of the helper's lists a form is left without a case.  (KNOB_WIDTH_CASES pin
    a knob at a width, not a form: the closure does not count them.)"""
    def complete(**skip):
        possible, reached = _closure(forms, default_side, latched, **skip)
        return possible - reached - set(afu.NOT_RUN) == set()

    assert complete()
    for case in afu.SMALL_CASES + afu.ROUND2_CASES:
        assert not complete(skip=case), ("the closure does not need", case[:4])
    for which in afu.LATCHED_SETTINGS:
        for i, case in enumerate(afu.KNOB_CASES[which] + afu.KNOB_ROUND2.get(which, [])):
            assert not complete(skip_knob=(which, i)), ("the closure does not need", which, case[:4])
