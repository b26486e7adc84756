"""GPU: which native calls the attention nodes issue, in which order, with which bench.py tag, block dimensions, `passes`, dz format and
pool arguments.  The backward of the scores-only node for the three contraction forms of ops._attn_bwd_contract (resident-W, dP walk,
E-form) and every combination of wanted row gradients, and the rule that orders the two attentions' contractions across streams
(ops._chain): these expectations were read off the dense backward when it had one hand-written branch per form.  The forward and backward
of the fused nodes: the dense node is the one-group case of the grouped one (ops._attn_blocks_fwd, ops._attn_blocks_bwd), a full-height
group launches the plain pool kernels, a trimmed one the weighted ones, and each group's contraction form follows its own shape."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, H, D = 2, 4, 16, 64          # the smallest shape that has the dP walk (H >= 16); the bf16 arithmetics have the resident-W backward at D = 64
F32, HL4 = 0, 1
KNOBS = ("NRM_BWD_DP", "NRM_BWD_RW", "NRM_DW_LAST", "NRM_DW_DIRECT", "NRM_BH_PIPE", "NRM_DW_R32", "NRM_DZ_ROWS")


# entry -> (index of the first of its three block dimensions, {argument name: index}) in the positional arguments of native.call
ARGS = {"nrm_pwattn_fwd": (9, {}),
        "nrm_pwattn_bwd_dz": (7, {"dz": 11}),
        "nrm_pwattn_bwd_contract": (8, {"passes": 12, "dz": 14}),
        "nrm_pwattn_bwd_dp_dtdh": (6, {}),
        "nrm_pwattn_bwd_rw_dtdh": (6, {}),
        "nrm_pool_bmm": (7, {"accumulate": 11}),
        "nrm_pool_bmm_wlast": (7, {"accumulate": 11, "wlast": 12, "wlast_row": 13}),
        "nrm_pool_rowdot": (4, {"zero_n": 9}),
        "nrm_pool_rowdot_wlast": (4, {"zero_n": 9, "wlast": 10})}


class _Calls(list):
    """The backward entries in the short form the first tests compare; ``launches``: every nrm_pwattn* / nrm_pool* call in full."""

    def __init__(self):
        super().__init__()
        self.launches = []


def launch(entry, dims=None, tag=None, **args):
    """One element of ``calls.launches``: (entry without nrm_, tag, block dimensions, {passes, dz, accumulate, zero_n, wlast, wlast_row}
    as far as the entry has them)."""
    return (entry, tag, dims, args)


@pytest.fixture
def calls(monkeypatch):
    """Every native call of the attention backward as (entry without its prefix, tag, passes, dz format), None where an entry has no
    such argument; stream waits appear in the same list as ("wait_event", stream, event).  ``calls.launches``: every attention and pool
    call, forward and backward, as ``launch`` builds it."""
    from news_recommendation_model_amd import native
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    seen, real_call, real_wait = _Calls(), native.call, torch.cuda.Stream.wait_event

    def call(name, *args, tag=None):
        if name.startswith("nrm_pwattn_bwd"):
            passes, fmt = (args[12], args[14]) if name.endswith("_contract") else (None, args[11]) if name.endswith("_dz") else (None, None)
            seen.append((name[len("nrm_pwattn_bwd_"):], tag, passes, fmt))
        if name.startswith(("nrm_pwattn", "nrm_pool")):
            first, named = ARGS.get(name, (None, {}))
            seen.launches.append(launch(name[len("nrm_"):], tuple(args[first:first + 3]) if first is not None else None, tag,
                                        **{k: args[i] for k, i in named.items()}))
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


# ---- the fused nodes: dense [B, T, H] and a grouped one over 3 impressions, a full-height group of 2 and one of H_g = 5 < 16 (too short for
# the dP walk), whose last row stands for 16 - 5 + 1 = 12 equal rows
GROUP_B0, GROUP_H, W_LAST = [0, 2, 3], [16, 5], 12.0
FULL, SHORT = (2, T, 16), (1, T, 5)


def _fused(rng, need_dt, need_dh, grouped):
    """-> a function that runs the forward of one fused node (fp32) and returns the function that runs its backward."""
    from news_recommendation_model_amd import ops
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    dev = torch.device("cuda", torch.cuda.current_device())
    dev_t = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)      # noqa: E731
    w = [dev_t(rng.uniform(-k, k, shape)).requires_grad_(True) for k, shape in ((k1, (D, 4 * D)), (k1, (D,)), (k2, (1, D)), (k2, (1,)))]
    n = GROUP_B0[-1] if grouped else B
    t = dev_t(rng.standard_normal((n, T, D))).requires_grad_(need_dt)
    h = dev_t(rng.standard_normal((2 * 16 + 1 * 5, D) if grouped else (B, H, D))).requires_grad_(need_dh)
    g = dev_t(rng.standard_normal((n, T, D)))
    torch.cuda.synchronize()

    def forward():
        if grouped:
            pooled = ops.attend_pool_grouped_fwd(t.flatten(0, 1), h, *w, GROUP_B0, GROUP_H, [T] * len(GROUP_H), H, T, True, ops.MMA_F32)[0].view_as(g)
        else:
            pooled = ops.attend_and_pool(t, h, *w, mma="f32")
        return (pooled * g).sum().backward
    return forward


def _fused_sequences(calls, need_dt, need_dh, grouped):
    forward = _fused(np.random.default_rng(13), need_dt, need_dh, grouped)
    del calls.launches[:]
    back = forward()
    fwd = list(calls.launches)
    del calls.launches[:]
    back()
    torch.cuda.synchronize()
    return fwd, list(calls.launches)


def _contractions(dims, dp):
    """The contraction launches of one block with both row gradients wanted: the dP walk where it is forced and the block can take it."""
    if dp == "1" and dims[2] >= 16:
        return [launch("pwattn_bwd_dp_pack"), launch("pwattn_bwd_dp_dtdh", dims, "pwattn_bwd_dp_dtdh"),
                launch("pwattn_bwd_contract", dims, E_DW, passes=4, dz=F32)]
    return [launch("pwattn_bwd_contract", dims, E_BT, passes=1, dz=F32), launch("pwattn_bwd_contract", dims, E_BH, passes=2, dz=F32)]


@pytest.mark.parametrize("dp", ["0", "1"])
def test_dense_fused_node_launches(lib, calls, monkeypatch, dp):
    monkeypatch.setenv("NRM_BWD_DP", dp)
    fwd, bwd = _fused_sequences(calls, True, True, False)
    assert fwd == [launch("pwattn_pack_wp"), launch("pwattn_fwd", FULL), launch("pool_bmm", (2, T, 16), accumulate=0)]
    assert bwd == ([launch("pool_rowdot", FULL, zero_n=D + 4), launch("pwattn_bwd_dz", FULL, dz=F32)] + _contractions(FULL, dp)
                   + [launch("pool_bmm", (2, 16, T), accumulate=1)])


def test_dense_fused_node_launches_without_row_gradients(lib, calls, monkeypatch):
    monkeypatch.setenv("NRM_BWD_DP", "0")
    _, bwd = _fused_sequences(calls, False, False, False)
    assert bwd == [launch("pool_rowdot", FULL, zero_n=D + 4), launch("pwattn_bwd_dz", FULL, dz=F32),
                   launch("pwattn_bwd_contract", FULL, E_DW, passes=4, dz=F32)]


@pytest.mark.parametrize("dp", ["0", "1"])
def test_grouped_node_launches(lib, calls, monkeypatch, dp):
    """A full-height group goes through the plain pool kernels, the trimmed one through the weighted ones (the forward's last column, the
    backward's last row); only the first rowdot clears dw2 | db2; the form of the contractions follows each group's own shape."""
    monkeypatch.setenv("NRM_BWD_DP", dp)
    fwd, bwd = _fused_sequences(calls, True, True, True)
    assert fwd == [launch("pwattn_pack_wp"),
                   launch("pwattn_fwd", FULL), launch("pool_bmm", (2, T, 16), accumulate=0),
                   launch("pwattn_fwd", SHORT), launch("pool_bmm_wlast", (1, T, 5), accumulate=0, wlast=W_LAST, wlast_row=0)]
    assert bwd == ([launch("pool_rowdot", FULL, zero_n=D + 4), launch("pwattn_bwd_dz", FULL, dz=F32),
                    launch("pool_rowdot_wlast", SHORT, zero_n=0, wlast=W_LAST), launch("pwattn_bwd_dz", SHORT, dz=F32)]
                   + _contractions(FULL, dp) + _contractions(SHORT, dp)
                   + [launch("pool_bmm", (2, 16, T), accumulate=1),
                      launch("pool_bmm_wlast", (1, 5, T), accumulate=1, wlast=W_LAST, wlast_row=1)])


def test_one_full_height_group_is_bitwise_the_dense_forward(lib):
    """torch.ops.nrm.attend_pool_grouped_fwd over the one group [0, B] x [H] against torch.ops.nrm.attend_pool_fwd: the same launches on
    the same operands, no atomics -- pooled, s and z bit for bit."""
    rng = np.random.default_rng(14)
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    dev = torch.device("cuda", torch.cuda.current_device())
    w = [torch.from_numpy(rng.uniform(-k, k, shape).astype(np.float32)).to(dev)
         for k, shape in ((k1, (D, 4 * D)), (k1, (D,)), (k2, (1, D)), (k2, (1,)))]
    t = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).to(dev)
    h = torch.from_numpy(rng.standard_normal((B, H, D)).astype(np.float32)).to(dev)
    pooled, s, z = torch.ops.nrm.attend_pool_fwd(t, h, *w, True, 0)
    pooled_g, s_g, z_g = torch.ops.nrm.attend_pool_grouped_fwd(t.reshape(B * T, D), h.reshape(B * H, D), *w, [0, B], [H], [T], H, T, True, 0)
    torch.cuda.synchronize()
    assert tuple(s.shape) == (B, T, H) and tuple(z.shape) == (B, T, H, D) and z_g.numel() == z.numel() and s_g.numel() >= s.numel()
    bits = lambda x: x.contiguous().view(torch.int32)                      # noqa: E731
    assert torch.equal(bits(pooled_g.reshape(B, T, D)), bits(pooled))
    assert torch.equal(bits(s_g[:s.numel()].reshape(B, T, H)), bits(s)) and torch.equal(bits(z_g.reshape(B, T, H, D)), bits(z))
    assert float(pooled.abs().max()) > 0 and float(z.abs().max()) > 0
