"""GPU: the packed dW_p-only pass (bwd_dw_pack_kernel: P = 4 / gcd(H, 4) consecutive (b,t) groups reduced together in whole 4-row steps,
NRM_DW_PACK=1) against the per-group pass (NRM_DW_PACK=0), the two-set E-form (NRM_DW_DIRECT=0) and the oracle.  Every shape runs under
the default plan (small launches: one group per split, so the launch stays unpacked) and with four splits (super-groups and the tails
behind them); nrm_pwattn_bwd_dw_pack says which kernel each launch takes, so no case passes by never running the new one."""
import functools

import numpy as np
import pytest
import torch

from golden_util import rel_err
from oracle import user_model_oracle as orc

pytestmark = pytest.mark.gpu
GRAD_TOL = 1e-2
KNOBS = ("NRM_DW_PACK", "NRM_DW_DIRECT", "NRM_BT_WAVES", "NRM_BT_INTERLEAVE", "NRM_BT_ORDER", "NRM_BWD_DP")

# (B, T, H, D): the smallest shapes at which each thing can go wrong
SHAPES = [
    (3, 7, 18, 80),     # P = 2; T odd: pairs straddle impressions; ranges of 6, 6, 6, 3 groups (an odd tail); one exact 5x5 tile
    (3, 6, 17, 64),     # P = 4; ranges of 5 (one quad and a tail); an exact 4x4 tile
    (2, 3, 13, 80),     # the shortest R the direct kernel takes; S = 13 (2 groups per split: stays unpacked)
    (6, 3, 13, 80),     # ... and with ranges of 5, where it is packed
    (2, 5, 14, 80),     # R = 2 mod 4 at the minimum S
    (2, 5, 15, 80),     # R = 3 mod 4 (3 groups per split: stays unpacked)
    (4, 5, 15, 80),     # ... packed
    (1, 9, 19, 72),     # ragged width on 5x5 (unpacked at 3 groups per split)
    (2, 9, 19, 72),     # ... packed
    (2, 6, 50, 400),    # C3's group shape; all 25 tiles; a pair and a tail
    (5, 1, 17, 64),     # T = 1 (2 groups per split: unpacked)
    (17, 1, 17, 64),    # T = 1: the four groups of a quad are four impressions; ranges 5, 5, 5, 2
    (3, 6, 18, 64),     # P = 2 on an exact 4x4 tile
    (2, 9, 18, 72),     # P = 2 on the ragged 5x5 tile
    (2, 9, 17, 100),    # P = 4 on ragged 4x4 tiles (four of them)
    (2, 9, 18, 100),    # P = 2 on ragged 4x4 tiles
    (2, 4, 16, 80),     # R % 4 == 0: the entry reports 1 and the gradient equals that of NRM_DW_PACK=0 exactly
]


def _tiles(D):
    n16 = (D + 15) // 16
    tile = 5 if (n16 + 4) // 5 * 5 < (n16 + 3) // 4 * 4 else 4
    return ((n16 + tile - 1) // tile) ** 2


def _expected_pack(B, T, H, four_splits):
    """bwd_e_select's rule restated for these small launches: the default plan gives them one group per split, NRM_BT_WAVES = 4 tiles
    gives four splits of ceil(G / 4) groups.  (All shapes here are below the 256 KB per group of the interleaved walk.)"""
    P = 1 if H % 4 == 0 else 2 if H % 2 == 0 else 4
    gps = -(-B * T // 4) if four_splits else 1
    return P if P > 1 and gps >= P and (H + 3) // 4 >= 4 and P * H // 4 >= 4 else 1


def _weights(rng, D):
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    return {"mlp.fc1.weight": rng.uniform(-k1, k1, (D, 4 * D)).astype(np.float32),
            "mlp.fc1.bias": rng.uniform(-k1, k1, (D,)).astype(np.float32),
            "mlp.fc2.weight": rng.uniform(-k2, k2, (1, D)).astype(np.float32),
            "mlp.fc2.bias": rng.uniform(-k2, k2, (1,)).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def _case(B, T, H, D):
    """inputs and the oracle's fc1 gradient: computed once per shape, shared by both plans, never written to"""
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D + 23)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    p = {"a." + k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in w.items()}
    s_c = orc.pointwise_attention_scores(p, "a", torch.from_numpy(tgt), torch.from_numpy(his))[..., 0]
    (s_c * torch.from_numpy(gs)).sum().backward()
    ref = p["a.mlp.fc1.weight"].grad.numpy()
    for arr in (tgt, his, gs, ref, *w.values()):
        arr.setflags(write=False)
    return w, tgt, his, gs, ref


def _fc1_grad(w, tgt, his, gs, rowgrads):
    from news_recommendation_model_amd import ops
    wg = {k: torch.from_numpy(v.copy()).cuda().requires_grad_(True) for k, v in w.items()}
    t_g = torch.from_numpy(tgt.copy()).cuda().requires_grad_(rowgrads)
    h_g = torch.from_numpy(his.copy()).cuda().requires_grad_(rowgrads)
    s = ops.pointwise_attention_scores(t_g, h_g, wg["mlp.fc1.weight"], wg["mlp.fc1.bias"], wg["mlp.fc2.weight"], wg["mlp.fc2.bias"])
    (s * torch.from_numpy(gs.copy()).cuda()).sum().backward()
    torch.cuda.synchronize()
    return wg["mlp.fc1.weight"].grad.cpu().numpy()


def _check(lib, monkeypatch, B, T, H, D, four_splits, rowgrads):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if four_splits:
        monkeypatch.setenv("NRM_BT_WAVES", str(4 * _tiles(D)))
        gps = -(-B * T // 4)
        assert lib.nrm_pwattn_bwd_nsplit(B, T, H, D, 0) == -(-B * T // gps)   # four splits, or as many as ceil(G / 4) groups each leave
    if rowgrads:
        monkeypatch.setenv("NRM_BWD_DP", "1")
    w, tgt, his, gs, ref = _case(B, T, H, D)
    want = _expected_pack(B, T, H, four_splits)

    monkeypatch.setenv("NRM_DW_PACK", "1")
    assert lib.nrm_pwattn_bwd_dw_pack(B, T, H, D, 0) == want           # the launch below is (is not) the packed kernel
    g_p = _fc1_grad(w, tgt, his, gs, rowgrads)
    monkeypatch.setenv("NRM_DW_PACK", "0")
    assert lib.nrm_pwattn_bwd_dw_pack(B, T, H, D, 0) == 1
    g_u = _fc1_grad(w, tgt, his, gs, rowgrads)
    monkeypatch.setenv("NRM_DW_DIRECT", "0")
    g_e = _fc1_grad(w, tgt, his, gs, rowgrads)

    errs = (rel_err(g_p, ref), rel_err(g_p[:, 3 * D:], ref[:, 3 * D:]), rel_err(g_p, g_u), rel_err(g_p, g_e))
    print(f"dw_pack {(B, T, H, D)} four_splits={four_splits} rowgrads={rowgrads} pack={want}: oracle {errs[0]:.3e} dW_p {errs[1]:.3e} "
          f"vs unpacked {errs[2]:.3e} vs E-form {errs[3]:.3e}")
    assert errs[0] < GRAD_TOL
    assert errs[1] < 1e-4                                               # the dW_p block itself
    assert errs[2] < 2e-5                                               # the same products, another summation order
    if H % 4 == 0:
        assert np.array_equal(g_p, g_u)                                 # nothing to pack: the same kernel, the same bits
    assert errs[3] < 2e-5


@pytest.mark.parametrize("four_splits", [False, True])
@pytest.mark.parametrize("B,T,H,D", SHAPES)
def test_packed_dw_pass_matches_unpacked_e_form_and_oracle(lib, monkeypatch, B, T, H, D, four_splits):
    _check(lib, monkeypatch, B, T, H, D, four_splits, rowgrads=False)


def test_packed_dw_pass_beside_the_dp_walk(lib, monkeypatch):
    B, T, H, D = 2, 6, 50, 400
    assert lib.nrm_pwattn_bwd_dp_supported(D, H)
    _check(lib, monkeypatch, B, T, H, D, four_splits=True, rowgrads=True)


def test_every_shape_family_is_packed_somewhere():
    """the table above must reach the new kernel for P = 2 and P = 4, on 5x5 and 4x4 tiles, exact and ragged"""
    seen = {(_expected_pack(B, T, H, True), D) for B, T, H, D in SHAPES}
    assert {(2, 80), (2, 400), (2, 64), (2, 72), (2, 100), (4, 64), (4, 80), (4, 72), (4, 100)} <= seen
