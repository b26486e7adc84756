"""GPU: which native calls one attention backward issues, in which order, with which bench.py tag, `passes` and dz format -- for the
three forms of ops._attn_bwd_core (resident-W, dP walk, E-form) and every combination of wanted row gradients -- and the rule that
orders the two attentions' contractions across streams (ops._chain).  The expectations were read off _attn_bwd_core as it stood with
one hand-written branch per form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, H, D = 2, 4, 16, 64          # the smallest shape that has the dP walk (H >= 16); the bf16 arithmetics have the resident-W backward at D = 64
F32, HL4 = 0, 1
KNOBS = ("NRM_BWD_DP", "NRM_BWD_RW", "NRM_DW_LAST", "NRM_DW_DIRECT", "NRM_BH_PIPE", "NRM_DW_R32", "NRM_DZ_ROWS")


@pytest.fixture
def calls(monkeypatch):
    """Every native call of the attention backward as (entry without its prefix, tag, passes, dz format), None where an entry has no
    such argument; stream waits appear in the same list as ("wait_event", stream, event)."""
    from news_recommendation_model_amd import native
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    seen, real_call, real_wait = [], native.call, torch.cuda.Stream.wait_event

    def call(name, *args, tag=None):
        if name.startswith("nrm_pwattn_bwd"):
            passes, fmt = (args[12], args[14]) if name.endswith("_contract") else (None, args[11]) if name.endswith("_dz") else (None, None)
            seen.append((name[len("nrm_pwattn_bwd_"):], tag, passes, fmt))
        return real_call(name, *args, tag=tag)

    def wait_event(self, event):
        seen.append(("wait_event", self, event))
        return real_wait(self, event)

    monkeypatch.setattr(native, "call", call)
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
    return seen


def _attention(rng, need_dt, need_dh, mma):
    """-> a function that runs the backward of one freshly run forward."""
    from news_recommendation_model_amd import ops
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    dev = torch.device("cuda", torch.cuda.current_device())
    w = [torch.from_numpy(rng.uniform(-k, k, shape).astype(np.float32)).to(dev).requires_grad_(True)
         for k, shape in ((k1, (D, 4 * D)), (k1, (D,)), (k2, (1, D)), (k2, (1,)))]
    t = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).to(dev).requires_grad_(need_dt)
    h = torch.from_numpy(rng.standard_normal((B, H, D)).astype(np.float32)).to(dev).requires_grad_(need_dh)
    g = torch.from_numpy(rng.standard_normal((B, T, H)).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    loss = (ops.pointwise_attention_scores(t, h, *w, mma=mma) * g).sum()
    return loss.backward


def _sequence(calls, need_dt, need_dh, mma):
    back = _attention(np.random.default_rng(11), need_dt, need_dh, mma)
    del calls[:]
    back()
    torch.cuda.synchronize()
    return list(calls)


E_BT, E_BH, E_DW = "pwattn_bwd_e_bt", "pwattn_bwd_e_bh", "pwattn_bwd_e_dw"
E_FORM = {(True, True): [("contract", E_BT, 1, F32), ("contract", E_BH, 2, F32)],
          (True, False): [("contract", E_BT, 1, F32)],
          (False, True): [("contract", E_DW, 4, F32), ("contract", E_BH, 2, F32)],
          (False, False): [("contract", E_DW, 4, F32)]}
DP_WALK = dict(E_FORM)
DP_WALK[(True, True)] = [("dp_pack", None, None, None), ("dp_dtdh", "pwattn_bwd_dp_dtdh", None, None), ("contract", E_DW, 4, F32)]
RW_ROWS = [("rw_pack", None, None, None), ("rw_dtdh", "pwattn_bwd_rw_dtdh", None, None), ("contract", E_BT, 4, HL4)]
RESIDENT_W = {(True, True): RW_ROWS, (True, False): RW_ROWS, (False, True): RW_ROWS, (False, False): [("contract", E_BT, 4, HL4)]}


@pytest.mark.parametrize("need_dt,need_dh", [(True, True), (True, False), (False, True), (False, False)])
def test_backward_launch_order_of_every_form(lib, calls, monkeypatch, need_dt, need_dh):
    for dp, want in (("0", E_FORM), ("1", DP_WALK)):
        monkeypatch.setenv("NRM_BWD_DP", dp)
        assert _sequence(calls, need_dt, need_dh, "f32") == [("dz", None, None, F32)] + want[need_dt, need_dh], dp
    monkeypatch.delenv("NRM_BWD_DP")
    assert _sequence(calls, need_dt, need_dh, "bf16x3") == [("dz", None, None, HL4)] + RESIDENT_W[need_dt, need_dh]


def test_weight_only_contraction_waits_for_a_full_chain_on_another_stream(lib, calls, monkeypatch):
    """ops._chain: a backward that produced a row gradient notes the end of its chain; a contraction that serves no row gradient, issued
    later in the same step on ANOTHER stream, waits for that end before it is launched -- and leaves it where it is."""
    from news_recommendation_model_amd import ops
    monkeypatch.setenv("NRM_DW_LAST", "1")            # (the default switches the wait on by size: hundreds of millions of z elements)
    monkeypatch.setenv("NRM_BWD_DP", "0")
    rng = np.random.default_rng(12)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ops.begin_step()
    assert ops._chain["end"] is None
    with torch.cuda.stream(sa):
        full = _attention(rng, True, True, "f32")
    with torch.cuda.stream(sb):
        weights_only = _attention(rng, False, False, "f32")
        same_stream = _attention(rng, False, False, "f32")
    with torch.cuda.stream(sa):
        same_stream_a = _attention(rng, False, False, "f32")
    assert ops._chain["end"] is None                  # (a training forward clears it)
    del calls[:]
    full()
    end = ops._chain["end"]
    assert end is not None and end[0] == ops._chain["token"] and end[2] == sa
    assert not [c for c in calls if c[0] == "wait_event"]
    del calls[:]
    weights_only()
    assert calls == [("dz", None, None, F32), ("wait_event", sb, end[1]), ("contract", E_DW, 4, F32)]
    assert ops._chain["end"] is end                   # a chain without a row gradient notes nothing
    del calls[:]
    same_stream_a()                                   # on the chain's own stream: stream order already holds
    assert calls == [("dz", None, None, F32), ("contract", E_DW, 4, F32)]
    monkeypatch.setenv("NRM_DW_LAST", "0")
    del calls[:]
    same_stream()
    assert calls == [("dz", None, None, F32), ("contract", E_DW, 4, F32)]
    ops.begin_step()
    assert ops._chain["end"] is None
    torch.cuda.synchronize()
