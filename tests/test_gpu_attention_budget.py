"""GPU: every form of the pointwise attention held to the fp32 error budget of tests/attention_budget.py -- float64 truth, the fp32
reference's own loss on the same case as the yardstick, judged per impression / per fc1 block in two norms.

With NRM_BUDGET_RECORD=<path> every measured ratio is written there as JSON when the module finishes (the committed
profiles/attention_error_budget.json is one such run); without it nothing is written."""
import pytest

import attention_budget as ab
from test_gpu_attention import BF16_SHAPES, DP_SHAPES, SHAPES

pytestmark = pytest.mark.gpu

_record = []


@pytest.fixture(scope="module", autouse=True)
def _budget_record():
    yield
    path = ab.record_path()
    if path:
        ab.write_record(path, _record)


# (the dW_p-only pass that NRM_DW_DIRECT switches runs beside the dP walk, or when no row gradient is wanted: see the weight-only test)
F32_FORMS = dict(ab.FORMS, dp_dw_direct0={"NRM_BWD_DP": "1", "NRM_DW_DIRECT": "0"}, dp_dw_direct1={"NRM_BWD_DP": "1", "NRM_DW_DIRECT": "1"},
                 bt_interleave0={"NRM_BT_INTERLEAVE": "0"}, bt_interleave1={"NRM_BT_INTERLEAVE": "1"})
BF16X3_FORMS = {"default": {}, "dz_rows0": {"NRM_DZ_ROWS": "0"}, "dz_rows1": {"NRM_DZ_ROWS": "1"}}
ALL_F32_SHAPES = list(dict.fromkeys(SHAPES + DP_SHAPES))
# every form on every shape: the cases of one shape share their cached references, so a form costs a device launch.  Measured on one
# MI355X, alternating three times: this module 8.6 .. 9.0 s, tests/test_gpu_attention.py at the parent commit 8.9 .. 9.7 s
F32_FORM_CASES = [(f, s) for f in F32_FORMS for s in ALL_F32_SHAPES]
ALL_BF16X3_SHAPES = list(dict.fromkeys(BF16_SHAPES + [(4, 6, 50, 256), (3, 5, 130, 208)]))
FAMILY_SHAPES = [(3, 7, 19, 72), (2, 30, 50, 400), (2, 15, 200, 64), (2, 30, 32, 256), (1, 5, 17, 388), (5, 1, 3, 64)]
FAMILY_CONFIGS = {"f32-default": ("f32", "default"), "f32-dp_walk": ("f32", "dp_walk"), "f32-e_form": ("f32", "e_form"),
                  "bf16x3-default": ("bf16x3", "default")}
OTHER_FAMILIES = [f for f in ab.FAMILIES if f != "normal"]
KNOBS = ("NRM_FWD_CT", "NRM_FWD_WALK_F32", "NRM_FWD_WALK", "NRM_BWD_DP", "NRM_DP_GRID", "NRM_DZ_ROWS", "NRM_DW_DIRECT",
         "NRM_BT_INTERLEAVE", "NRM_BT_ORDER", "NRM_BWD_RW", "NRM_DW_R32")


def _set_form(monkeypatch, lib, forms, form, shape):
    why = ab.form_skip_reason(form, shape[3], shape[2], lib)
    if why:
        pytest.skip(why)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in forms[form].items():
        monkeypatch.setenv(k, v)


def _judge(case, mma, form, rowgrads=True):
    got = ab.run_device(case, mma, rowgrads=rowgrads)
    return ab.assert_within_budget(got, case, mma, rowgrads=rowgrads, record=_record, form=form, rowgrads_wanted=rowgrads)


@pytest.mark.parametrize("form,shape", F32_FORM_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_f32_forms_within_budget(lib, monkeypatch, form, shape):
    B, T, H, D = shape
    _set_form(monkeypatch, lib, F32_FORMS, form, (B, T, H, D))
    _judge(ab.get_case((B, T, H, D)), "f32", form)


@pytest.mark.parametrize("B,T,H,D", ALL_BF16X3_SHAPES)
@pytest.mark.parametrize("form", list(BF16X3_FORMS))
def test_bf16x3_forms_within_budget(lib, monkeypatch, form, B, T, H, D):
    _set_form(monkeypatch, lib, BF16X3_FORMS, form, (B, T, H, D))
    _judge(ab.get_case((B, T, H, D)), "bf16x3", form)


@pytest.mark.parametrize("B,T,H,D", FAMILY_SHAPES)
@pytest.mark.parametrize("config", list(FAMILY_CONFIGS))
@pytest.mark.parametrize("family", OTHER_FAMILIES)
def test_input_families_within_budget(lib, monkeypatch, family, config, B, T, H, D):
    mma, form = FAMILY_CONFIGS[config]
    _set_form(monkeypatch, lib, F32_FORMS, form, (B, T, H, D))
    _judge(ab.get_case((B, T, H, D), family), mma, form)


@pytest.mark.parametrize("B,T,H,D", [(3, 7, 19, 72), (2, 30, 32, 256)])
@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
@pytest.mark.parametrize("family", list(ab.FAMILIES))
def test_attend_and_pool_within_budget(lib, monkeypatch, family, mma, B, T, H, D):
    """The fused attention + pool node (pooled output, the pool's history gradient added by the attention's last launch)."""
    _set_form(monkeypatch, lib, F32_FORMS, "default", (B, T, H, D))
    _judge(ab.get_case((B, T, H, D), family, pool=True), mma, "default")


# (3, 7, 5, 320): an exact width above 256 -- bf16x3 takes the EXACT serial contraction for dW_p alone, from fp32 dz
@pytest.mark.parametrize("B,T,H,D", [(2, 30, 50, 400), (3, 7, 19, 72), (2, 15, 200, 64), (3, 7, 5, 320)])
@pytest.mark.parametrize("mma,direct", [("f32", "0"), ("f32", "1"), ("bf16x3", None)])
def test_weight_only_backward_within_budget(lib, monkeypatch, mma, direct, B, T, H, D):
    """t and h without requires_grad (the text+image attention's path): no row gradients are formed, every weight piece is judged.
    fp32: the one-set dW_p pass (NRM_DW_DIRECT=1, the default) and the two-set E-form."""
    _set_form(monkeypatch, lib, F32_FORMS, "default", (B, T, H, D))
    if direct is not None:
        monkeypatch.setenv("NRM_DW_DIRECT", direct)
    _judge(ab.get_case((B, T, H, D)), mma, "weight_only" + ("" if direct is None else "_dw_direct" + direct), rowgrads=False)


@pytest.mark.parametrize("B,T,H,D", [(32, 6, 16, 400), (33, 5, 50, 256), (40, 4, 24, 64)])
@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
def test_default_dispatch_at_batch_32_within_budget(lib, monkeypatch, mma, B, T, H, D):
    """What the library picks by itself for B >= 32 (full-row dz pass, compact candidate image): no knob in the environment."""
    _set_form(monkeypatch, lib, F32_FORMS, "default", (B, T, H, D))
    _judge(ab.get_case((B, T, H, D)), mma, "default")


@pytest.mark.parametrize("B,T,H,D", [s for s in ALL_BF16X3_SHAPES if s[3] >= 64 and s[0] * s[1] * s[2] >= 64])
def test_plain_bf16_fails_the_bf16x3_budget(lib, monkeypatch, B, T, H, D):
    """On-device sensitivity: plain bf16 (one product instead of three) judged as if it were bf16x3 must be rejected, and not
    marginally -- its scores sit above 4 * M_BF16X3 yardsticks.  If plain bf16 passed, the bf16x3 gate would be too wide."""
    _set_form(monkeypatch, lib, F32_FORMS, "default", (B, T, H, D))
    case = ab.get_case((B, T, H, D))
    r = ab.ratios(ab.run_device(case, "bf16"), case, "bf16x3")
    meta = dict(case.tag, entry="scores", arithmetic="bf16 (judged as bf16x3, not gated)", form="default", rowgrads_wanted=True)
    _record.extend(dict(meta, piece=p, norm=n, ratio=float(v)) for (p, n), v in r.items())
    for norm in ("max", "l2"):
        assert r[("s", norm)] > 4 * ab.M_BF16X3, (norm, r[("s", norm)])
