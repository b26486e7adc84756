"""Shared by the history-compaction tests: histories cut to given lengths the way the reference's ETL pads them
(rows past the user's own all-zero), the plan's history tables by explicit loops, and the weighted formula on the float64 oracle."""
import numpy as np
import torch

L_LIST = lambda H: [0, 1, 15, 16, 17, H - 1, H]          # noqa: E731  (the lengths the issue names)


def cut_history(batch, lengths):
    """In place: rows ``lengths[b]:`` of impression b's history zeroed."""
    for b, n in enumerate(lengths):
        batch["x_history"][b, int(n):] = 0.0
    return batch


def brute_force_history_plan(counts, hist_len, H):
    """The history tables by explicit loops (what compact.build_plan(..., history_len=, H=) is checked against).  ``counts[b]``: compact
    candidate rows of impression b."""
    L = [min(max(int(x), 0), H) for x in hist_len]
    hist_off, hist_src, hist_mult, tile_pre = [0], [], [], [0]
    k_max = 0
    for b, l in enumerate(L):
        k = l + (1 if l < H else 0)
        for j in range(k):
            hist_src.append(b * H + j)
        hist_off.append(len(hist_src))
        hist_mult.append(H - l)
        tile_pre.append(tile_pre[-1] + int(counts[b]) * ((k + 15) // 16))
        k_max = max(k_max, k)
    return dict(hist_len=L, hist_mult=hist_mult, hist_off=hist_off, hist_src=hist_src, R=len(hist_src), k_max=k_max, tile_pre=tile_pre,
                Mt=tile_pre[-1], history_dense=all(l == H for l in L))


def weighted_eu_H(orc, p, x_history, x_target, hist_len, use_mult=True):
    """eu_H [B, T, D_l + P] by the formula of section 5d on the oracle: impression b's first K_b history rows scored as the reference
    scores them, pooled with weight 1 except H - L_b on row L_b (``use_mult=False``: weight 1 there too -- the mutant the tests must catch)."""
    B, H = x_history.shape[:2]
    P = p["invariant_interest_model.text_img_attention.mlp.fc2.weight"].shape[1]
    rows = []
    for b in range(B):
        l = int(hist_len[b])
        k = l + (1 if l < H else 0)
        _eu, _ec, aux = orc.invariant_interest(p, x_history[b:b + 1, :k], x_target[b:b + 1], return_aux=True)
        w = torch.ones(k, dtype=aux["label_h"].dtype)
        if l < H and use_mult:
            w[l] = H - l
        ti_h = x_history[b:b + 1, :k, 4:4 + P].to(aux["label_h"].dtype)
        lab = torch.sum(aux["score_label"] * w[None, None, :, None] * aux["label_h"][:, None], dim=2)
        ti = torch.sum(aux["score_text_img"] * w[None, None, :, None] * ti_h[:, None], dim=2)
        rows.append(torch.cat([lab, ti], dim=2))
    return torch.cat(rows, dim=0)


def eval_logits_from_eu_H(orc, p, eu_H, x_target, x_global, eps=1e-5):
    """The eval-mode head of the oracle's user_model_forward (models/user_model.py:31-34) on a given eu_H."""
    _e, ec = orc.invariant_interest(p, torch.zeros(x_target.shape[0], 1, x_target.shape[2] + 2, dtype=x_target.dtype), x_target)
    e = torch.cat([eu_H, orc.instant_interest(p, x_global), ec], dim=2)
    B, T, N = e.shape
    e2 = e.reshape(B * T, N)
    c = (e2 - p["bn.running_mean"]) / torch.sqrt(p["bn.running_var"] + eps) * p["bn.weight"] + p["bn.bias"]
    x = orc.mlp(p, "gate", c) * e2
    return orc.mlp(p, "out_mlp", orc.mlp(p, "mlp", x)).reshape(B, T)
