"""GPU: the HIP pointwise-attention op (through the C ABI) against the oracle's literal
[B,T,H,4D]-concat implementation, forward and every gradient.
Tolerances (BASELINE.json north_star): forward <= 1e-3 relative, gradients <= 1e-2 relative -- and, where _budget is called, the fp32
error budget of tests/attention_budget.py: a float64 oracle, judged per impression / per fc1 block at a small multiple of what the
fp32 oracle itself loses on the same case."""
import os

import numpy as np
import pytest
import torch

import attention_budget as ab
from golden_util import GOLDEN, rel_err
from oracle import user_model_oracle as orc

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 1e-3, 1e-2


def _weights(rng, D):
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    return {"mlp.fc1.weight": rng.uniform(-k1, k1, (D, 4 * D)).astype(np.float32),
            "mlp.fc1.bias": rng.uniform(-k1, k1, (D,)).astype(np.float32),
            "mlp.fc2.weight": rng.uniform(-k2, k2, (1, D)).astype(np.float32),
            "mlp.fc2.bias": rng.uniform(-k2, k2, (1,)).astype(np.float32)}


def _run_both(w, tgt, his, gs, mma=None):
    """-> (scores, grads) of the HIP op and of the oracle; grads = dict incl. target/history."""
    from news_recommendation_model_amd import ops
    # oracle on CPU
    p = {"a." + k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in w.items()}
    t_c = torch.from_numpy(tgt).clone().requires_grad_(True)
    h_c = torch.from_numpy(his).clone().requires_grad_(True)
    s_c = orc.pointwise_attention_scores(p, "a", t_c, h_c)[..., 0]
    (s_c * torch.from_numpy(gs)).sum().backward()
    ref = {"target": t_c.grad.numpy(), "history": h_c.grad.numpy()}
    ref.update({k: p["a." + k].grad.numpy() for k in w})
    # HIP op
    dev = "cuda"
    wg = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in w.items()}
    t_g = torch.from_numpy(tgt).to(dev).requires_grad_(True)
    h_g = torch.from_numpy(his).to(dev).requires_grad_(True)
    s_g = ops.pointwise_attention_scores(t_g, h_g, wg["mlp.fc1.weight"], wg["mlp.fc1.bias"],
                                         wg["mlp.fc2.weight"], wg["mlp.fc2.bias"], mma=mma)
    (s_g * torch.from_numpy(gs).to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = {"target": t_g.grad.cpu().numpy(), "history": h_g.grad.cpu().numpy()}
    got.update({k: wg[k].grad.cpu().numpy() for k in w})
    return s_g.detach().cpu().numpy(), got, s_c.detach().numpy(), ref


def _budget(w, tgt, his, gs, s, got, arithmetic="f32"):
    """The result of _run_both under the float64 error budget; w / tgt / his / gs as given to _run_both."""
    return ab.assert_within_budget(ab.from_run_both(s, got), ab.Case(w, tgt, his, gs), arithmetic)


def _budget_spot(arithmetic, w4, t, h, g, s, dt, dh, gw):
    """Oracle spot check of a full-size launch under the error budget: ``t, h, g, s, dt, dh`` are the chosen impressions' slices of
    the FULL launch, ``gw`` the four weight gradients of a launch over those impressions alone (weight gradients sum over the batch)."""
    w = {k: v.detach().cpu().numpy() for k, v in zip(ab.WKEYS, w4)}
    case = ab.Case(w, t.detach().cpu().numpy(), h.detach().cpu().numpy(), g.detach().cpu().numpy())
    got = {"s": s.detach().cpu().numpy(), "d_target": dt.cpu().numpy(), "d_history": dh.cpu().numpy()}
    got.update({k: v.cpu().numpy() for k, v in zip(ab.WKEYS, gw)})
    return ab.assert_within_budget(got, case, arithmetic)


# (B, T, H, D): BASELINE shapes at reduced B, reference default, ragged / tiny / non-multiple-of-16 cases
SHAPES = [
    (2, 30, 50, 400),     # C3 large: 25x1 forward tiles (one N-chunk), 5x5 E tiles with 3+2 sub-passes
    (2, 30, 32, 256),     # C2 small: 16x2 tiles
    (2, 15, 200, 64),     # reference default H/T/D
    (2, 20, 10, 256),     # C1 demo
    (1, 64, 128, 768),    # C5 long: three N-chunks
    (3, 7, 19, 72),       # nothing is a multiple of 16
    (1, 1, 1, 64),        # single pair
    (5, 1, 3, 64),        # H < 4 (one partial reduction step)
    (1, 3, 1, 128),       # H = 1
    (7, 5, 37, 100),      # D multiple of 4 only
    (2, 9, 21, 320),      # 20 column tiles in one N-chunk (20x1 wave tile)
    (1, 5, 17, 388),      # 24.25 -> 25 column tiles with a ragged last tile
    (1, 4, 9, 420),       # 27 tiles -> two N-chunks of 14
    (2, 5, 7, 66),        # D not a multiple of 4: zero-padded to 68 inside the wrapper
    (3, 2, 4, 5),         # tiny odd width
    (1, 3, 300, 64),      # history longer than one LDS du slab (256 rows): two chunks in bwd_dz
    (2, 2, 520, 8),       # three history chunks, dv accumulated across them
]


# the pipelined dh kernel (T >= 21 on 4x4 tiles, T >= 29 on 5x5) at widths that fill no whole wave tile, with a group count that is no
# multiple of 4 (a last workgroup with fewer than four live waves): the two instantiations no other shape of this file reaches
PIPE_RAGGED_SHAPES = [(3, 21, 5, 100), (3, 29, 7, 72)]


@pytest.mark.parametrize("B,T,H,D", SHAPES + PIPE_RAGGED_SHAPES)
def test_scores_and_grads_match_oracle(lib, B, T, H, D):
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    s, got, s_ref, ref = _run_both(w, tgt, his, gs)
    assert s.shape == (B, T, H)
    assert rel_err(s, s_ref) < FWD_TOL
    for k in ref:
        assert rel_err(got[k], ref[k]) < GRAD_TOL, k
    _budget(w, tgt, his, gs, s, got)


# fp32 "walk" form of the resident-W forward (pwattn_fwd_walk_f32_kernel, round 5; the default at D = 64, NRM_FWD_WALK_F32=1 at D = 128):
# a wave keeps its 16 history rows, its u tile and the fc2 weights in registers and walks the candidates.  Against the oracle and
# against the tile-by-tile resident-W kernel (NRM_FWD_WALK_F32=0) -- scores and the saved pre-activation; the two start their
# accumulators at u and at u + v, one fp32 rounding apart -- with and without the z store, ragged last history tile, a candidate
# walk split over workgroups (few impressions), T = 1, H = 1
@pytest.mark.parametrize("B,T,H,D", [(2, 15, 200, 64), (256, 15, 200, 64), (3, 7, 19, 64), (1, 1, 1, 64), (5, 1, 3, 64), (2, 33, 16, 64),
                                     (1, 40, 17, 64), (2, 15, 50, 128), (3, 5, 9, 128)])
def test_fp32_walk_forward_matches_oracle_and_tile_form(lib, monkeypatch, B, T, H, D):
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D + 3)
    w = {k: torch.from_numpy(v).cuda() for k, v in _weights(rng, D).items()}
    t = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).cuda()
    h = torch.from_numpy(rng.standard_normal((B, H, D)).astype(np.float32)).cuda()
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("NRM_FWD_WALK_F32", mode)
        s, z = ops.pwattn_fwd(t, h, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"], w["mlp.fc2.bias"], True, ops.MMA_F32)
        s2, _ = ops.pwattn_fwd(t, h, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"], w["mlp.fc2.bias"], False, ops.MMA_F32)
        torch.cuda.synchronize()
        out[mode] = (s.clone(), z.clone(), s2.clone())
    assert torch.equal(out["1"][0], out["1"][2])                      # the z store does not change the scores
    assert torch.allclose(out["1"][1], out["0"][1], rtol=1e-5, atol=1e-5)      # z: (u + P W^T) + v against (u + v) + P W^T
    assert torch.allclose(out["1"][0], out["0"][0], rtol=1e-4, atol=1e-5)
    if B <= 8:
        p = {"a." + k: v.cpu() for k, v in w.items()}
        ref = orc.pointwise_attention_scores(p, "a", t.cpu(), h.cpu())[..., 0]
        assert rel_err(out["1"][0].cpu().numpy(), ref.numpy()) < FWD_TOL
        assert rel_err(out["0"][0].cpu().numpy(), ref.numpy()) < FWD_TOL
    # the default dispatch: the walk at D = 64, the tile form at D = 128
    monkeypatch.delenv("NRM_FWD_WALK_F32", raising=False)
    s, _ = ops.pwattn_fwd(t, h, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"], w["mlp.fc2.bias"], True, ops.MMA_F32)
    assert torch.equal(s, out["1" if D == 64 else "0"][0])


# compact candidate image of the forward kernel (template parameter CT, csrc/pwattn_fwd.hip; default for H >= 16 on the 10 / 12 / 13-tile
# plans -- the 16-tile plan of D = 768 keeps the per-row image, pwattn_fwd_launch measured it slower there): forced on from H = 5 and off, the scores and the saved pre-activation must be BIT-identical (same arithmetic, only
# the LDS staging of the candidate rows differs) -- ragged row counts, blocks that span many candidates, D of every such plan
@pytest.mark.parametrize("B,T,H,D", [(2, 30, 50, 400), (3, 7, 19, 388), (1, 64, 128, 768), (5, 3, 5, 160), (4, 9, 7, 192), (2, 11, 16, 400),
                                     (3, 5, 130, 208), (1, 1, 5, 400), (7, 2, 21, 176), (2, 13, 63, 768)])
def test_compact_candidate_image_is_bit_identical(lib, monkeypatch, B, T, H, D):
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D + 7)
    w = {k: torch.from_numpy(v).cuda() for k, v in _weights(rng, D).items()}
    t = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).cuda()
    h = torch.from_numpy(rng.standard_normal((B, H, D)).astype(np.float32)).cuda()
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("NRM_FWD_CT", mode)
        s, z = ops.pwattn_fwd(t, h, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"], w["mlp.fc2.bias"], True, ops.MMA_F32)
        s2, _ = ops.pwattn_fwd(t, h, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"], w["mlp.fc2.bias"], False, ops.MMA_F32)
        torch.cuda.synchronize()
        out[mode] = (s.clone(), z.clone(), s2.clone())
    assert torch.equal(out["0"][1], out["1"][1])                      # z
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][2], out["1"][2])
    p = {"a." + k: v.cpu() for k, v in w.items()}
    ref = orc.pointwise_attention_scores(p, "a", t.cpu(), h.cpu())[..., 0]
    assert rel_err(out["1"][0].cpu().numpy(), ref.numpy()) < FWD_TOL


# full-row form of the dz pass (bwd_dz_rows_kernel: one workgroup owns all D columns of an impression; the default from B >= 32 when
# >= 85 % of the lanes own a column and a thread owns <= 6 rows, dz_rows_threads in csrc/pwattn_bwd.hip): forced here on every small
# shape it can take -- (D, H) -> 512 threads with <= 6 rows per thread, else 1024 threads; shapes it cannot take (D = 768 / H = 128:
# 26 rows per thread) silently stay on the slab form.  The DEFAULT dispatch (no NRM_DZ_ROWS / NRM_FWD_CT in the environment) is
# asserted against the oracle by test_default_dispatch_at_batch_32_matches_oracle below
DZ_ROWS_SHAPES = [(2, 30, 50, 400), (2, 30, 32, 256), (2, 15, 200, 64), (2, 20, 10, 256), (3, 7, 19, 72), (1, 1, 1, 64), (5, 1, 3, 64),
                  (7, 5, 37, 100), (1, 5, 17, 388), (1, 4, 9, 420), (2, 5, 7, 66), (3, 2, 4, 5), (1, 3, 300, 64), (2, 2, 520, 8),
                  (1, 64, 128, 768), (4, 3, 6, 1024), (2, 31, 5, 16)]


@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
@pytest.mark.parametrize("B,T,H,D", DZ_ROWS_SHAPES)
def test_full_row_dz_pass_matches_oracle_and_slab_form(lib, monkeypatch, mma, B, T, H, D):
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    monkeypatch.setenv("NRM_DZ_ROWS", "0")
    _, slab, _, _ = _run_both(w, tgt, his, gs, mma=mma)
    monkeypatch.setenv("NRM_DZ_ROWS", "1")
    s, got, s_ref, ref = _run_both(w, tgt, his, gs, mma=mma)
    fwd_tol, grad_tol = (FWD_TOL, GRAD_TOL) if mma == "f32" else (1e-4, 1e-3)
    assert rel_err(s, s_ref) < fwd_tol
    for k in ref:
        assert rel_err(got[k], ref[k]) < grad_tol, (k, rel_err(got[k], ref[k]))
        # same arithmetic per element; only the order of the dv / dw2 partial sums (and of float atomics downstream) differs
        assert rel_err(got[k], slab[k]) < 2e-5, (k, rel_err(got[k], slab[k]))


# dP walk form of the fp32 backward (csrc/pwattn_bwd_dp.hip, round 5: dt and dh from ONE contraction dP = dz W_p, dW_p from the (b,t)
# pass without its epilogue), forced on (NRM_BWD_DP=1) against the oracle and against the E-form (NRM_BWD_DP=0): histories that are not
# a multiple of 16 (a wave's 16 flattened rows reach into the next impression), row counts that are not a multiple of 64, H = 16,
# every N-chunk plan (4 / 8 / 12 / 13 tiles; one, two and four chunks), D that is not a multiple of 16, one candidate, more
# workgroups than steps / 4 (NRM_DP_GRID) and a single workgroup walking everything
DP_SHAPES = [(2, 30, 50, 400), (3, 7, 19, 72), (2, 15, 200, 64), (1, 64, 128, 768), (7, 5, 37, 100), (2, 9, 21, 320), (1, 5, 17, 388),
             (1, 4, 16, 420), (5, 1, 16, 64), (9, 3, 23, 132), (2, 11, 16, 400), (33, 2, 17, 208), (4, 6, 50, 256), (1, 3, 300, 64)]


@pytest.mark.parametrize("B,T,H,D", DP_SHAPES)
def test_dp_walk_backward_matches_oracle_and_e_form(lib, monkeypatch, B, T, H, D):
    assert lib.nrm_pwattn_bwd_dp_supported(D, H) == 1
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D + 5)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    monkeypatch.setenv("NRM_BWD_DP", "0")
    _, eform, _, _ = _run_both(w, tgt, his, gs)
    monkeypatch.setenv("NRM_BWD_DP", "1")
    for grid in (None, "1", "7"):
        if grid is None:
            monkeypatch.delenv("NRM_DP_GRID", raising=False)
        else:
            monkeypatch.setenv("NRM_DP_GRID", grid)
        s, got, s_ref, ref = _run_both(w, tgt, his, gs)
        assert rel_err(s, s_ref) < FWD_TOL
        for k in ref:
            assert rel_err(got[k], ref[k]) < GRAD_TOL, (grid, k, rel_err(got[k], ref[k]))
            # the same products in another summation order
            assert rel_err(got[k], eform[k]) < 2e-5, (grid, k, rel_err(got[k], eform[k]))


# the dW_p-only pass with ONE accumulator set (bwd_dw_direct_kernel, round 5: the scale row t[b,t,:] folded into the h operand, one long
# reduction over (group, row)) against the two-set E-form (NRM_DW_DIRECT=0) and the oracle: as the text+image attention runs it (no row
# gradient wanted) and beside the dP walk; 5x5 and 4x4 tiles, exact and ragged widths, odd step counts, H <= 4 (one reduction step per
# group: the launcher keeps the E-form), the interleaved group walk of big groups
@pytest.mark.parametrize("rowgrads", [False, True])
@pytest.mark.parametrize("B,T,H,D", [(2, 30, 50, 400), (3, 7, 19, 72), (2, 15, 200, 64), (1, 64, 128, 768), (7, 5, 37, 100), (5, 1, 3, 64),
                                     (1, 3, 1, 128), (2, 9, 21, 320), (1, 5, 17, 388), (4, 6, 5, 256), (2, 3, 8, 160), (33, 2, 17, 208)])
def test_direct_dw_pass_matches_oracle_and_e_form(lib, monkeypatch, rowgrads, B, T, H, D):
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D + 9)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    if rowgrads:
        if not lib.nrm_pwattn_bwd_dp_supported(D, H):
            pytest.skip("no dP walk for this shape: the dW_p-only pass never runs beside it")
        monkeypatch.setenv("NRM_BWD_DP", "1")

    def run():
        wg = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in w.items()}
        t_g = torch.from_numpy(tgt).cuda().requires_grad_(rowgrads)
        h_g = torch.from_numpy(his).cuda().requires_grad_(rowgrads)
        s = ops.pointwise_attention_scores(t_g, h_g, wg["mlp.fc1.weight"], wg["mlp.fc1.bias"], wg["mlp.fc2.weight"], wg["mlp.fc2.bias"])
        (s * torch.from_numpy(gs).cuda()).sum().backward()
        torch.cuda.synchronize()
        return wg["mlp.fc1.weight"].grad.cpu().numpy()

    monkeypatch.setenv("NRM_DW_DIRECT", "0")
    g_e = run()
    monkeypatch.setenv("NRM_DW_DIRECT", "1")
    g_d = run()
    for il in ("0", "1"):
        monkeypatch.setenv("NRM_BT_INTERLEAVE", il)
        g_i = run()
        assert rel_err(g_i, g_e) < 2e-5, il
    p = {"a." + k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in w.items()}
    s_c = orc.pointwise_attention_scores(p, "a", torch.from_numpy(tgt), torch.from_numpy(his))[..., 0]
    (s_c * torch.from_numpy(gs)).sum().backward()
    ref = p["a.mlp.fc1.weight"].grad.numpy()
    assert rel_err(g_d, ref) < GRAD_TOL
    assert rel_err(g_d[:, 3 * D:], ref[:, 3 * D:]) < 1e-4                   # the dW_p block itself
    assert rel_err(g_d, g_e) < 2e-5                                        # the same products, another summation order


def test_dp_walk_is_not_offered_where_it_cannot_run(lib):
    assert lib.nrm_pwattn_bwd_dp_supported(400, 15) == 0              # a wave's 16 rows could span three impressions
    assert lib.nrm_pwattn_bwd_dp_supported(66, 50) == 0               # rows that are not 16-byte multiples
    assert lib.nrm_pwattn_bwd_dp_packed_floats(400, 50) == 25 * 2 * 13 * 16 * 16


@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
@pytest.mark.parametrize("B,T,H,D", [(32, 6, 16, 400), (33, 5, 50, 256), (40, 4, 24, 64)])
def test_default_dispatch_at_batch_32_matches_oracle(lib, monkeypatch, mma, B, T, H, D):
    """What the library picks BY ITSELF for B >= 32, H >= 16 (every other small test forces a form): the full-row dz pass
    and, in fp32 at D = 400, the compact candidate image of the forward -- no NRM_DZ_ROWS / NRM_FWD_CT in the environment."""
    for e in ("NRM_DZ_ROWS", "NRM_FWD_CT", "NRM_FWD_WALK", "NRM_BWD_RW", "NRM_DW_R32"):
        monkeypatch.delenv(e, raising=False)
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D + 1)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    s, got, s_ref, ref = _run_both(w, tgt, his, gs, mma=mma)
    fwd_tol, grad_tol = (FWD_TOL, GRAD_TOL) if mma == "f32" else (1e-4, 1e-3)
    assert rel_err(s, s_ref) < fwd_tol
    for k in ref:
        assert rel_err(got[k], ref[k]) < grad_tol, (k, rel_err(got[k], ref[k]))
    _budget(w, tgt, his, gs, s, got, mma)


# bf16 MFMA operands, fp32 accumulation (BASELINE config 2).  Gates are the same as for the fp32 path and are taken against
# the SAME fp32 oracle: forward <= 1e-3, gradients <= 1e-2 (max-abs difference over max-abs reference, per tensor).
BF16_SHAPES = [
    (2, 30, 32, 256),     # C2 small (4x4 E tiles, 16x1 forward tiles, one 32-row reduction step)
    (2, 30, 50, 400),     # C3 dimensions: 5x5 E tiles, two N-chunks, D % 32 = 16 (half-empty last K-chunk)
    (2, 15, 200, 64),     # reference default: 7 reduction super-steps, the last one ragged
    (2, 20, 10, 256),     # C1 demo: fewer rows than one super-step
    (3, 7, 19, 72),       # nothing is a multiple of 16
    (1, 1, 1, 64), (5, 1, 3, 64), (7, 5, 37, 100), (1, 4, 9, 420), (2, 5, 7, 66), (3, 2, 4, 5), (1, 3, 300, 64),
]


# an exact width above 256 (no resident-W backward there) with 21 groups: the bf16 arithmetics on the EXACT serial contraction, both passes
BF16_E_EXACT_SHAPES = [(3, 7, 5, 320)]


@pytest.mark.parametrize("B,T,H,D", BF16_SHAPES + BF16_E_EXACT_SHAPES)
@pytest.mark.parametrize("mma", ["bf16x3", "bf16"])
def test_bf16_mfma_scores_and_grads_match_fp32_oracle(lib, mma, B, T, H, D):
    """bf16x3 (hi/lo split operands, three MFMAs per product) must meet the fp32 gates with a wide margin: it is the
    arithmetic BASELINE config 2 runs with.  Plain bf16 (one rounding of each operand, relative error 2^-9 per product)
    is measured at ~1.1e-3 on the raw scores of N(0,1) inputs at D = 256 -- just outside the 1e-3 gate -- and at 8e-3 on a
    single (b,t,h) pair (no max-norm averaging); it is characterised here with bounds of 1e-2 / 3e-2, not gated."""
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    s, got, s_ref, ref = _run_both(w, tgt, his, gs, mma=mma)
    fwd_tol, grad_tol = (1e-4, 1e-3) if mma == "bf16x3" else (1e-2, 3e-2)
    assert rel_err(s, s_ref) < fwd_tol, rel_err(s, s_ref)
    for k in ref:
        assert rel_err(got[k], ref[k]) < grad_tol, (k, rel_err(got[k], ref[k]))
    if mma == "bf16x3":
        _budget(w, tgt, his, gs, s, got, "bf16x3")
    # and it really is a different arithmetic from the fp32 path (unless the contraction is degenerate)
    s32, _, _, _ = _run_both(w, tgt, his, gs, mma="f32")
    if D >= 64 and H * T > 1:
        assert np.abs(s - s32).max() > 0


def test_padding_rows_are_scored_not_masked(lib):
    # all-zero history rows still produce fc2(GELU(bias + t W_t-part)) != 0 (SURVEY.md §7 "padding is not masked")
    rng = np.random.default_rng(5)
    B, T, H, D = 2, 4, 9, 64
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    his[:, 5:] = 0.0
    gs = np.ones((B, T, H), dtype=np.float32)
    s, got, s_ref, ref = _run_both(w, tgt, his, gs)
    assert np.abs(s[:, :, 5:]).min() > 0
    assert rel_err(s, s_ref) < FWD_TOL
    assert rel_err(got["history"], ref["history"]) < GRAD_TOL


def test_module_2d_target_golden(lib):
    """PointwiseAttentionExpanded with a [B,D] target against the REFERENCE's own output
    (tests/golden/attention_2d.npz, generated by importing models/attention_model.py)."""
    import news_recommendation_model_amd as nrm
    fx = np.load(os.path.join(GOLDEN, "attention_2d.npz"))
    att = nrm.PointwiseAttentionExpanded(64)
    att.load_state_dict({k[2:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("w/")})
    att = att.cuda()
    tgt = torch.from_numpy(fx["target"]).cuda().requires_grad_(True)
    his = torch.from_numpy(fx["history"]).cuda().requires_grad_(True)
    s = att(tgt, his)
    assert tuple(s.shape) == tuple(fx["scores"].shape)            # [B,1,H,1]
    (s * torch.from_numpy(fx["grad_scores"]).cuda()).sum().backward()
    assert rel_err(s.detach().cpu().numpy(), fx["scores"]) < FWD_TOL
    assert rel_err(tgt.grad.cpu().numpy(), fx["grad_target"]) < GRAD_TOL
    assert rel_err(his.grad.cpu().numpy(), fx["grad_history"]) < GRAD_TOL
    for k, v in att.named_parameters():
        assert rel_err(v.grad.cpu().numpy(), fx["grad/" + k]) < GRAD_TOL, k
    # stand-alone MLP and the non-broadcast PointwiseAttention variant
    m = nrm.MLP(264, 264)
    m.load_state_dict({k[6:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("mlp_w/")})
    y = m.cuda()(torch.from_numpy(fx["mlp_x"]).cuda())
    assert rel_err(y.detach().cpu().numpy(), fx["mlp_y"]) < FWD_TOL
    pa = nrm.PointwiseAttention(64).cuda()
    pa.load_state_dict(att.state_dict())
    one = pa(tgt.detach(), his.detach()[:, 0])
    assert rel_err(one.detach().cpu().numpy(), fx["scores"][:, 0, 0]) < FWD_TOL


def test_inference_path_saves_no_activations(lib):
    from news_recommendation_model_amd import ops
    rng = np.random.default_rng(3)
    D = 64
    w = {k: torch.from_numpy(v).cuda() for k, v in _weights(rng, D).items()}
    t = torch.randn(2, 3, D, device="cuda")
    h = torch.randn(2, 5, D, device="cuda")
    with torch.no_grad():
        s = ops.pointwise_attention_scores(t, h, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"],
                                           w["mlp.fc2.bias"])
    t2 = t.clone().requires_grad_(True)
    s2 = ops.pointwise_attention_scores(t2, h, w["mlp.fc1.weight"], w["mlp.fc1.bias"], w["mlp.fc2.weight"],
                                        w["mlp.fc2.bias"])
    # the two template variants (with / without the z store) may schedule the fc2 dot differently: rounding only
    assert torch.allclose(s, s2.detach(), rtol=1e-5, atol=1e-6)


def test_full_size_linearity_property(lib):
    """BASELINE C3 at full size (B=1024,H=50,T=30,D=400) is too big for the CPU oracle; use properties the
    math offers: the gradient wrt the upstream weight is linear, and scores of a batch equal scores of
    its halves (impressions are independent)."""
    from news_recommendation_model_amd import ops
    torch.manual_seed(0)
    B, T, H, D = 1024, 30, 50, 400
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    w1 = (torch.rand(D, 4 * D, device="cuda") * 2 - 1) * k1
    b1 = (torch.rand(D, device="cuda") * 2 - 1) * k1
    w2 = (torch.rand(1, D, device="cuda") * 2 - 1) * k2
    b2 = (torch.rand(1, device="cuda") * 2 - 1) * k2
    t = torch.randn(B, T, D, device="cuda")
    h = torch.randn(B, H, D, device="cuda", requires_grad=True)
    s = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2)
    with torch.no_grad():
        whole = ops.pointwise_attention_scores(t, h.detach(), w1, b1, w2, b2)
        lo = ops.pointwise_attention_scores(t[:512], h[:512].detach(), w1, b1, w2, b2)
        hi = ops.pointwise_attention_scores(t[512:], h[512:].detach(), w1, b1, w2, b2)
    # same kernel variant: a row's result does not depend on which other rows are in the launch
    assert torch.equal(whole[:512], lo) and torch.equal(whole[512:], hi)
    assert torch.allclose(s.detach(), whole, rtol=1e-5, atol=1e-6)
    g = torch.randn_like(s)
    (gh1,) = torch.autograd.grad(s, h, g, retain_graph=False)
    s = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2)
    (gh2,) = torch.autograd.grad(s, h, 2.0 * g)
    assert rel_err((gh2 / 2).cpu().numpy(), gh1.cpu().numpy()) < 1e-4     # float atomics: order noise only
    # spot check 2 impressions against the oracle
    idx = [3, 777]
    p = {"a.mlp.fc1.weight": w1.cpu(), "a.mlp.fc1.bias": b1.cpu(), "a.mlp.fc2.weight": w2.cpu(), "a.mlp.fc2.bias": b2.cpu()}
    ref = orc.pointwise_attention_scores(p, "a", t[idx].cpu(), h[idx].detach().cpu())[..., 0]
    assert rel_err(s.detach()[idx].cpu().numpy(), ref.numpy()) < FWD_TOL
    # ... and the BACKWARD of the full-size launch against the oracle: the gradients w.r.t. the target and
    # history rows of an impression depend on that impression only, so the oracle runs on the same 2 impressions
    tq = t.clone().requires_grad_(True)
    s = ops.pointwise_attention_scores(tq, h, w1, b1, w2, b2)
    gt_full, gh_full = torch.autograd.grad(s, [tq, h], g)
    t_c, h_c = t[idx].cpu().clone().requires_grad_(True), h[idx].detach().cpu().clone().requires_grad_(True)
    s_c = orc.pointwise_attention_scores(p, "a", t_c, h_c)[..., 0]
    (s_c * g[idx].cpu()).sum().backward()
    assert rel_err(gt_full[idx].cpu().numpy(), t_c.grad.numpy()) < GRAD_TOL
    assert rel_err(gh_full[idx].cpu().numpy(), h_c.grad.numpy()) < GRAD_TOL
    # the weight gradients sum over impressions: full launch == sum of the launches over its two halves, and the oracle's
    # weight gradients of 2 impressions == the HIP weight gradients of a launch over just those 2
    wq = [x.clone().requires_grad_(True) for x in (w1, b1, w2, b2)]
    gw_full = torch.autograd.grad(ops.pointwise_attention_scores(t, h.detach(), *wq), wq, g)
    gw_lo = torch.autograd.grad(ops.pointwise_attention_scores(t[:512], h[:512].detach(), *wq), wq, g[:512])
    gw_hi = torch.autograd.grad(ops.pointwise_attention_scores(t[512:], h[512:].detach(), *wq), wq, g[512:])
    for a, lo_, hi_ in zip(gw_full, gw_lo, gw_hi):
        assert rel_err(a.cpu().numpy(), (lo_ + hi_).cpu().numpy()) < 1e-4
    gw_two = torch.autograd.grad(ops.pointwise_attention_scores(t[idx], h[idx].detach(), *wq), wq, g[idx])
    pc = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    s_c = orc.pointwise_attention_scores(pc, "a", t[idx].cpu(), h[idx].detach().cpu())[..., 0]
    (s_c * g[idx].cpu()).sum().backward()
    for a, k in zip(gw_two, ("a.mlp.fc1.weight", "a.mlp.fc1.bias", "a.mlp.fc2.weight", "a.mlp.fc2.bias")):
        assert rel_err(a.cpu().numpy().reshape(-1), pc[k].grad.numpy().reshape(-1)) < GRAD_TOL, k
    # the same spot check under the error budget (dP walk, full-row dz pass and two streams are this size's default dispatch)
    _budget_spot("f32", (w1, b1, w2, b2), t[idx], h[idx], g[idx], s[idx], gt_full[idx], gh_full[idx], gw_two)


def test_full_size_c2_bf16x3_properties(lib):
    """BASELINE config 2 at FULL size (B=512, H=32, T=30, D=256) on the bf16x3 arithmetic: the persistent resident-W forward
    and the bf16 E-form backward against properties the math offers (too big for the CPU oracle): rows are independent of
    the rest of the launch (up to the order of the two float atomics per score, which commute exactly), the backward is
    linear in the upstream gradient, agrees with the fp32-MFMA path of the same kernels' inputs to 1e-4 / 1e-3, and two
    impressions match the fp32 oracle to the fp32 gate."""
    from news_recommendation_model_amd import ops
    torch.manual_seed(1)
    B, T, H, D = 512, 30, 32, 256
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    w1 = ((torch.rand(D, 4 * D, device="cuda") * 2 - 1) * k1).requires_grad_(True)
    b1 = (torch.rand(D, device="cuda") * 2 - 1) * k1
    w2 = (torch.rand(1, D, device="cuda") * 2 - 1) * k2
    b2 = (torch.rand(1, device="cuda") * 2 - 1) * k2
    t = torch.randn(B, T, D, device="cuda")
    h = torch.randn(B, H, D, device="cuda", requires_grad=True)
    with torch.no_grad():
        whole = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2, mma="bf16x3")
        lo = ops.pointwise_attention_scores(t[:200], h[:200], w1, b1, w2, b2, mma="bf16x3")
        f32 = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2, mma="f32")
    assert torch.equal(whole[:200], lo)
    assert rel_err(whole.cpu().numpy(), f32.cpu().numpy()) < 1e-4
    g = torch.randn_like(whole)
    s = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2, mma="bf16x3")
    gh1, gw1 = torch.autograd.grad(s, [h, w1], g)
    s = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2, mma="bf16x3")
    gh2, gw2 = torch.autograd.grad(s, [h, w1], 2.0 * g)
    assert rel_err((gh2 / 2).cpu().numpy(), gh1.cpu().numpy()) < 1e-4 and rel_err((gw2 / 2).cpu().numpy(), gw1.cpu().numpy()) < 1e-4
    s = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2, mma="f32")
    gh32, gw32 = torch.autograd.grad(s, [h, w1], g)
    assert rel_err(gh1.cpu().numpy(), gh32.cpu().numpy()) < 1e-3 and rel_err(gw1.cpu().numpy(), gw32.cpu().numpy()) < 1e-3
    idx = [5, 400]
    p = {"a.mlp.fc1.weight": w1.detach().cpu(), "a.mlp.fc1.bias": b1.cpu(), "a.mlp.fc2.weight": w2.cpu(), "a.mlp.fc2.bias": b2.cpu()}
    ref = orc.pointwise_attention_scores(p, "a", t[idx].cpu(), h[idx].detach().cpu())[..., 0]
    assert rel_err(whole[idx].cpu().numpy(), ref.numpy()) < FWD_TOL
    # the two impressions under the bf16x3 error budget: scores and row gradients of the FULL launch, weight gradients of a launch
    # over those two alone
    tq = t.clone().requires_grad_(True)
    s = ops.pointwise_attention_scores(tq, h, w1, b1, w2, b2, mma="bf16x3")
    gt_full, gh_full = torch.autograd.grad(s, [tq, h], g)
    wq = [x.detach().clone().requires_grad_(True) for x in (w1, b1, w2, b2)]
    gw_two = torch.autograd.grad(ops.pointwise_attention_scores(t[idx], h[idx].detach(), *wq, mma="bf16x3"), wq, g[idx])
    _budget_spot("bf16x3", (w1, b1, w2, b2), t[idx], h[idx], g[idx], s[idx], gt_full[idx], gh_full[idx], gw_two)


def _fuzz_shapes(n=48, seed=20260101):
    rng = np.random.default_rng(seed)
    shapes = []
    for i in range(n):
        B = int(rng.integers(1, 4))
        T = int(rng.integers(1, 45))            # both sides of the pipelined dh kernel's threshold (T >= 21 / 29)
        H = int(rng.integers(1, 75))
        D = int(rng.choice([4, 8, 12, 20, 36, 52, 64, 68, 76, 80, 84, 96, 100, 124, 128, 132, 160, 164, 200, 7, 33, 90]))
        shapes.append((B, T, H, D))
    return shapes


@pytest.mark.parametrize("B,T,H,D", _fuzz_shapes(n=16, seed=7))
def test_random_shapes_match_oracle_bf16x3(lib, B, T, H, D):
    """The fuzz list on the bf16x3 arithmetic (resident-W forward: slice counts 1..n, ragged last slices, widths that are not
    multiples of 32; E-form backward with ragged 32-row super-steps), held to the fp32 gates."""
    rng = np.random.default_rng(B * 100003 + T * 1009 + H * 31 + D)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    s, got, s_ref, ref = _run_both(w, tgt, his, gs, mma="bf16x3")
    assert rel_err(s, s_ref) < FWD_TOL
    for k in ref:
        assert rel_err(got[k], ref[k]) < GRAD_TOL, k
    _budget(w, tgt, his, gs, s, got, "bf16x3")


def _fuzz_shapes_dp(n=24, seed=20261005):
    rng = np.random.default_rng(seed)
    shapes = []
    for i in range(n):
        B = int(rng.integers(1, 9))              # row counts B*H on both sides of whole 64-row blocks, impressions inside a wave's 16 rows
        T = int(rng.integers(1, 12))
        H = int(rng.integers(16, 90))
        D = int(rng.choice([16, 36, 64, 68, 100, 128, 132, 192, 208, 212, 256, 320, 400, 404, 420, 33, 90]))
        shapes.append((B, T, H, D))
    return shapes


@pytest.mark.parametrize("B,T,H,D", _fuzz_shapes_dp())
def test_random_shapes_match_oracle_dp_walk(lib, monkeypatch, B, T, H, D):
    """Random shapes through the dP walk + one-set dW_p pass (forced: they are the default only from 100 M z elements): every N-chunk
    plan, ragged last chunks and tiles, widths the wrapper pads to a multiple of 4, with a random workgroup count."""
    monkeypatch.setenv("NRM_BWD_DP", "1")
    rng = np.random.default_rng(B * 100003 + T * 1009 + H * 31 + D)
    monkeypatch.setenv("NRM_DP_GRID", str(int(rng.integers(1, 40))))
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    s, got, s_ref, ref = _run_both(w, tgt, his, gs)
    assert rel_err(s, s_ref) < FWD_TOL
    for k in ref:
        assert rel_err(got[k], ref[k]) < GRAD_TOL, (k, rel_err(got[k], ref[k]))
        assert rel_err(got[k], ref[k]) < 1e-4, (k, rel_err(got[k], ref[k]))          # (measured: 1e-6; a wrong segment or tail shows as 1e-1)
    _budget(w, tgt, his, gs, s, got)


@pytest.mark.parametrize("B,T,H,D", _fuzz_shapes())
def test_random_shapes_match_oracle(lib, B, T, H, D):
    """Seeded random (B, T, H, D): every tile-edge / step-count / padding combination the hand-picked list may miss
    (tile counts 1..13, widths that are not multiples of 16 or 4, T and H on both sides of every kernel-variant
    threshold)."""
    rng = np.random.default_rng(B * 100003 + T * 1009 + H * 31 + D)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    s, got, s_ref, ref = _run_both(w, tgt, his, gs)
    assert rel_err(s, s_ref) < FWD_TOL
    for k in ref:
        assert rel_err(got[k], ref[k]) < GRAD_TOL, k
    _budget(w, tgt, his, gs, s, got)


# The dt/dW pass has two group walks (csrc/capi.hip): blocked (every wave its own run of groups) and interleaved (the four
# waves of a workgroup share one run round-robin; default for groups above 256 KB, i.e. C5).  Both must give the same
# gradients for any number of groups / splits, including a last workgroup with fewer than four active waves.
# Under the default plan a launch of few groups gets one group per wave, where the two walks are the same walk: every shape with
# enough groups therefore runs a second time under a plan forced with NRM_BT_WAVES to at least three groups per split and a split
# count that is no multiple of 4 (attention_bwd_forms_util.interleave_waves asks nrm_pwattn_bwd_plan), asserted through the query.
# The last four shapes are there for that plan: 9 groups in 3 splits; 21 in 7 on 5x5 tiles; H = 33 (the bf16 arithmetics on the
# serial hl4 kernel, which honours the walk; at H <= 32 their 32-row kernel always walks blocked); D = 320 (their dt pass).
INTERLEAVED_SHAPES = [(2, 30, 50, 400), (3, 7, 19, 72), (5, 1, 3, 64), (1, 4, 9, 420), (7, 5, 37, 100), (1, 1, 1, 64), (2, 3, 130, 768),
                      (3, 3, 5, 64), (3, 7, 5, 80), (3, 7, 33, 100), (3, 7, 5, 320)]
INTERLEAVED_FORCED = INTERLEAVED_SHAPES[:3] + INTERLEAVED_SHAPES[4:5] + INTERLEAVED_SHAPES[7:]      # the others have fewer than 5 groups


@pytest.mark.parametrize("mma", ["f32", "bf16x3"])
@pytest.mark.parametrize("B,T,H,D", INTERLEAVED_SHAPES)
def test_interleaved_group_walk_matches_oracle(lib, monkeypatch, mma, B, T, H, D):
    import attention_bwd_forms_util as abu
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D + 1)
    w = _weights(rng, D)
    tgt = rng.standard_normal((B, T, D)).astype(np.float32)
    his = rng.standard_normal((B, H, D)).astype(np.float32)
    gs = rng.standard_normal((B, T, H)).astype(np.float32)
    for k in abu.PER_LAUNCH:
        monkeypatch.delenv(k, raising=False)
    plans = [None]
    if (B, T, H, D) in INTERLEAVED_FORCED:
        waves = abu.interleave_waves(lib, (B, T, H, D), abu.MMA_BY_NAME[mma])
        assert waves is not None, "no NRM_BT_WAVES gives this shape several groups per split"
        plans.append(waves)
    for waves in plans:
        if waves is not None:
            monkeypatch.setenv("NRM_BT_WAVES", waves)
            monkeypatch.setenv("NRM_BWD_DP", "0")
        out = {}
        for walk in ("0", "1"):
            monkeypatch.setenv("NRM_BT_INTERLEAVE", walk)
            if waves is not None:                                        # the launch below walks several groups per wave, in this walk
                f = [f for f in abu.launches(lib, (B, T, H, D), abu.MMA_BY_NAME[mma]) if f["launch"] == abu.CONTRACT and f["pass"] != 2][0]
                assert f["gps"] > 1 and (f["gps"] >= 3 and f["nsplit"] % 4 != 0 or B * T < 9), f
                assert f["interleave"] == int(walk) or f["family"] == "dw_r32", f
            s, got, s_ref, ref = _run_both(w, tgt, his, gs, mma=mma)
            assert rel_err(s, s_ref) < FWD_TOL
            for k in ref:
                assert rel_err(got[k], ref[k]) < GRAD_TOL, (waves, walk, k, rel_err(got[k], ref[k]))
            out[walk] = got
        # the two walks differ only in the order in which float atomics and slab sums meet
        for k in out["0"]:
            assert rel_err(out["1"][k], out["0"][k]) < 1e-4, (waves, k)
        # ... and so does the k-range-major block order of the pass (NRM_BT_ORDER=1: a measured no-go for C5's over-fetch, kept as a
        # tuning knob -- which workgroup owns which tile must not matter)
        monkeypatch.setenv("NRM_BT_ORDER", "1")
        _, got, _, _ = _run_both(w, tgt, his, gs, mma=mma)
        for k in out["0"]:
            assert rel_err(got[k], out["1"][k]) < 1e-4, (waves, k)
        monkeypatch.delenv("NRM_BT_ORDER")


def test_full_size_c5_properties(lib):
    """BASELINE config 5 at FULL size (B=256, H=128, T=64, D=768; z = 6.4 GB): the launch geometry the fuzz lists never reach --
    three N-chunks of 16 column tiles in the forward, 32-column dz slabs, 4x4 E tiles with the INTERLEAVED group walk of the
    dt/dW pass (groups of 393 KB) and a grid that exceeds one XCD's L2.  Too big for the CPU oracle as a whole, so: rows are
    independent of the rest of the launch, the backward is linear in the upstream gradient, weight gradients add over halves of
    the batch, and one impression matches the oracle (forward and every gradient)."""
    from news_recommendation_model_amd import ops
    torch.manual_seed(5)
    B, T, H, D = 256, 64, 128, 768
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    w1 = (torch.rand(D, 4 * D, device="cuda") * 2 - 1) * k1
    b1 = (torch.rand(D, device="cuda") * 2 - 1) * k1
    w2 = (torch.rand(1, D, device="cuda") * 2 - 1) * k2
    b2 = (torch.rand(1, device="cuda") * 2 - 1) * k2
    t = torch.randn(B, T, D, device="cuda")
    h = torch.randn(B, H, D, device="cuda")
    g = torch.randn(B, T, H, device="cuda")
    with torch.no_grad():
        whole = ops.pointwise_attention_scores(t, h, w1, b1, w2, b2)
        lo = ops.pointwise_attention_scores(t[:100], h[:100], w1, b1, w2, b2)
        hi = ops.pointwise_attention_scores(t[100:], h[100:], w1, b1, w2, b2)
    assert torch.equal(whole[:100], lo) and torch.equal(whole[100:], hi)
    # backward of the full launch: linear in the upstream gradient
    tq, hq = t.clone().requires_grad_(True), h.clone().requires_grad_(True)
    wq = [x.clone().requires_grad_(True) for x in (w1, b1, w2, b2)]
    s = ops.pointwise_attention_scores(tq, hq, *wq)
    assert torch.allclose(s.detach(), whole, rtol=1e-5, atol=1e-6)            # with / without the z store
    grads1 = torch.autograd.grad(s, [tq, hq] + wq, g)
    s = ops.pointwise_attention_scores(tq, hq, *wq)
    grads2 = torch.autograd.grad(s, [tq, hq] + wq, -0.5 * g)
    for a, b_ in zip(grads1, grads2):
        assert rel_err((b_ * -2.0).cpu().numpy().reshape(-1), a.cpu().numpy().reshape(-1)) < 1e-4
    # weight gradients add over the two halves of the batch; row gradients of a half equal those of the full launch
    half = B // 2
    parts = []
    for sl in (slice(0, half), slice(half, B)):
        tp, hp = t[sl].clone().requires_grad_(True), h[sl].clone().requires_grad_(True)
        parts.append(torch.autograd.grad(ops.pointwise_attention_scores(tp, hp, *wq), [tp, hp] + wq, g[sl]))
    for i in range(2, 6):
        assert rel_err(grads1[i].cpu().numpy().reshape(-1), (parts[0][i] + parts[1][i]).cpu().numpy().reshape(-1)) < 1e-4
    assert rel_err(grads1[0][:half].cpu().numpy(), parts[0][0].cpu().numpy()) < 1e-4
    assert rel_err(grads1[1][half:].cpu().numpy(), parts[1][1].cpu().numpy()) < 1e-4
    del parts, grads2
    # one impression against the oracle: scores, target / history gradients (of the FULL launch) and the weight gradients of a
    # launch over that impression alone
    i = 77
    p = {"a.mlp.fc1.weight": w1.cpu(), "a.mlp.fc1.bias": b1.cpu(), "a.mlp.fc2.weight": w2.cpu(), "a.mlp.fc2.bias": b2.cpu()}
    pc = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    t_c, h_c = t[i:i + 1].cpu().clone().requires_grad_(True), h[i:i + 1].cpu().clone().requires_grad_(True)
    s_c = orc.pointwise_attention_scores(pc, "a", t_c, h_c)[..., 0]
    (s_c * g[i:i + 1].cpu()).sum().backward()
    assert rel_err(whole[i:i + 1].cpu().numpy(), s_c.detach().numpy()) < FWD_TOL
    assert rel_err(grads1[0][i:i + 1].cpu().numpy(), t_c.grad.numpy()) < GRAD_TOL
    assert rel_err(grads1[1][i:i + 1].cpu().numpy(), h_c.grad.numpy()) < GRAD_TOL
    gw_one = torch.autograd.grad(ops.pointwise_attention_scores(t[i:i + 1], h[i:i + 1], *wq), wq, g[i:i + 1])
    for a, k in zip(gw_one, ("a.mlp.fc1.weight", "a.mlp.fc1.bias", "a.mlp.fc2.weight", "a.mlp.fc2.bias")):
        assert rel_err(a.cpu().numpy().reshape(-1), pc[k].grad.numpy().reshape(-1)) < GRAD_TOL, k
    _budget_spot("f32", (w1, b1, w2, b2), t[i:i + 1], h[i:i + 1], g[i:i + 1], whole[i:i + 1], grads1[0][i:i + 1], grads1[1][i:i + 1], gw_one)
