"""Shared by the tests of the step that trains on compacted candidate lists: the counts the checks name, batches
padded the way the reference's training ETL pads a candidate list (all-zero x_target / x_global rows, label 0), the candidate-group
identity on the float64 oracle -- the oracle's own functions per group on the trimmed columns, BatchNorm and the loss with a row weight,
both written out here -- its three mutants, and a brute-force planner."""
import itertools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from compact_util import pad_batch

T_ID, H_ID, B_ID = 7, 5, 9
COUNTS = [1, 2, 3, 3, 6, 7, 7, 4, 2]
# sizes of the contiguous groups of the sorted batch and the columns each keeps
HAND_GROUPINGS = {"3+3+3": ((3, 3, 3), (3, 5, 7)), "5+4": ((5, 4), (4, 7)), "one group": ((9,), (7,))}
MUTANTS = ("bn", "loss", "bn_bwd")          # weight 1 in BatchNorm only / in the loss only / in bn_backward's column terms only


def padded_batch(dims, counts, H, T, seed, user_num=None):
    """synth.make_batch with candidates ``counts[b]:`` of impression b padded (numpy dict; ``empty_num`` = T - counts)."""
    from news_recommendation_model_amd import synth
    return pad_batch(synth.make_batch(dims, len(counts), H, T, seed=seed, user_num=user_num), counts)


def hand_plan(counts, T, sizes, widths, order=None):
    """A CandidateGroupPlan-like record for given group sizes and widths (``order``: the sorted order, default by count)."""
    n = np.clip(np.asarray(counts, dtype=np.int64), 0, T)
    perm = np.argsort(n, kind="stable") if order is None else np.asarray(order, dtype=np.int64)
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(n))
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    T_g = np.asarray(widths, dtype=np.int64)
    for g in range(len(sizes)):                     # what makes the identity hold: column T_g - 1 of every member is padding, or the group is untrimmed
        assert T_g[g] == T or (n[perm[bounds[g]:bounds[g + 1]]] + 1 <= T_g[g]).all()
    row_off = np.concatenate([[0], np.cumsum(np.asarray(sizes) * T_g)]).astype(np.int64)
    expand = np.empty((len(n), T), dtype=np.int64)
    for g in range(len(sizes)):
        for i in range(bounds[g], bounds[g + 1]):
            expand[perm[i]] = row_off[g] + (i - bounds[g]) * T_g[g] + np.minimum(np.arange(T), T_g[g] - 1)
    return SimpleNamespace(B=len(n), T=T, G=len(sizes), count=n, perm=perm, inverse=inverse, bounds=bounds, T_g=T_g, w_g=T - T_g + 1, row_off=row_off,
                           N=int(row_off[-1]), expand=expand.reshape(-1))


def row_weights(plan, dtype=torch.float64):
    w = torch.ones(plan.N, dtype=dtype)
    for g in range(plan.G):
        n, tg = int(plan.bounds[g + 1] - plan.bounds[g]), int(plan.T_g[g])
        w[int(plan.row_off[g]):int(plan.row_off[g + 1])].view(n, tg)[:, tg - 1] = float(plan.w_g[g])
    return w


class WeightedBatchNorm(torch.autograd.Function):
    """Training-mode BatchNorm over rows x [N, width] that stand for n rows, with the backward of the issue's identity written out:
        mean = (1/n) sum_r w_r x_r     var = (1/n) sum_r w_r (x_r - mean)^2
        dx_r = gamma rstd [G_r - wb_r s0 / n - wb_r xhat_r s1 / n],  s0 = sum_r G_r,  s1 = sum_r G_r xhat_r        (G carries the weight already)
    ``w`` weights the statistics, ``wb`` the two column terms of the backward (the mutants set one of them to ones)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, wb, n, eps):
        mean = (w[:, None] * x).sum(0) / n
        var = (w[:, None] * (x - mean) ** 2).sum(0) / n
        rstd = 1.0 / torch.sqrt(var + eps)
        xhat = (x - mean) * rstd
        ctx.save_for_backward(xhat, gamma, rstd, wb)
        ctx.n = n
        ctx.stats = (mean.detach(), var.detach())
        return xhat * gamma + beta

    @staticmethod
    def backward(ctx, G):
        xhat, gamma, rstd, wb = ctx.saved_tensors
        s0, s1 = G.sum(0), (G * xhat).sum(0)
        dx = gamma * rstd * (G - wb[:, None] * s0 / ctx.n - wb[:, None] * xhat * s1 / ctx.n)
        return dx, s1, s0, None, None, None, None


def weighted_loss(orc, p, user_id_sorted, r_arena, label_arena, plan, w_loss, alpha=0.95):
    """(1/n) sum_b sum_t w_t bce(p_t, y_t) for both terms, p_t = exp(r_t) / sum_t' w_t' exp(r_t'), nn.BCELoss's clamp per entry."""
    n = plan.B * plan.T
    total = 0.0
    for g in range(plan.G):
        lo, hi, tg = int(plan.row_off[g]), int(plan.row_off[g + 1]), int(plan.T_g[g])
        r = r_arena[lo:hi].view(-1, tg)
        y = label_arena[lo:hi].view(-1, tg).to(r.dtype)
        w = w_loss[lo:hi].view(-1, tg)
        d = p["delta"][user_id_sorted[int(plan.bounds[g]):int(plan.bounds[g + 1])].long()][:, None]
        for shift, wt in ((torch.zeros_like(d), 1 - alpha), (d, alpha)):
            o = r + shift
            e = torch.exp(o - o.max(dim=1, keepdim=True).values)
            prob = e / (w * e).sum(dim=1, keepdim=True)
            total = total + wt * (w * F.binary_cross_entropy(prob, y, reduction="none")).sum() / n
    return total


def compact_oracle_step(orc, sd, batch, plan, mutant=None, hist=None, dtype=torch.float64, eps=1e-5):
    """One training-mode forward + loss + gradients of the oracle on the candidate groups of ``plan`` -> (loss, logits [B, T] expanded in
    the caller's order, {name: gradient}, (batch mean, biased batch variance)).  ``hist`` = (H_g per group): the groups are trimmed in the
    history too, their last kept row weighted H - H_g + 1 in the two pools (the identity of section 5e, per group)."""
    p = orc.to_torch_params(sd, dtype=dtype)
    tb = {k: torch.from_numpy(v) for k, v in batch.items() if isinstance(v, np.ndarray) and v.ndim > 0}
    perm = torch.as_tensor(np.asarray(plan.perm).astype(np.int64))
    H = tb["x_history"].shape[1]
    with orc.precision(dtype):
        rows, labels = [], []
        for g in range(plan.G):
            idx, tg = perm[int(plan.bounds[g]):int(plan.bounds[g + 1])], int(plan.T_g[g])
            xt, xg = tb["x_target"][idx, :tg], tb["x_global"][idx, :tg]
            if hist is None:
                eu_H, ec = orc.invariant_interest(p, tb["x_history"][idx], xt)
            else:
                hg = int(hist[g])
                P = p["invariant_interest_model.text_img_attention.mlp.fc2.weight"].shape[1]
                _e, ec, aux = orc.invariant_interest(p, tb["x_history"][idx, :hg], xt, return_aux=True)
                wh = torch.ones(hg, dtype=dtype)
                wh[-1] = float(H - hg + 1)
                ti_h = tb["x_history"][idx, :hg, 4:4 + P].to(dtype)
                eu_H = torch.cat([torch.sum(aux["score_label"] * wh[None, None, :, None] * aux["label_h"][:, None], dim=2),
                                  torch.sum(aux["score_text_img"] * wh[None, None, :, None] * ti_h[:, None], dim=2)], dim=2)
            e = torch.cat([eu_H, orc.instant_interest(p, xg), ec], dim=2)
            rows.append(e.reshape(-1, e.shape[2]))
            labels.append(tb["label"][idx, :tg].reshape(-1))
        e2, label_arena = torch.cat(rows, dim=0), torch.cat(labels)
        w = row_weights(plan, dtype)
        ones = torch.ones_like(w)
        n = plan.B * plan.T
        c = WeightedBatchNorm.apply(e2, p["bn.weight"], p["bn.bias"], ones if mutant == "bn" else w, ones if mutant in ("bn", "bn_bwd") else w, n, eps)
        stats = weighted_batch_stats(e2, ones if mutant == "bn" else w, n)
        x = orc.mlp(p, "gate", c) * e2
        r = orc.mlp(p, "out_mlp", orc.mlp(p, "mlp", x)).reshape(-1)
        loss = weighted_loss(orc, p, tb["user_id"][perm], r, label_arena, plan, ones if mutant == "loss" else w)
        names = [k for k in p if k not in orc.BUFFER_KEYS]
        grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    out = r.detach()[torch.as_tensor(np.asarray(plan.expand).astype(np.int64))].view(plan.B, plan.T)
    return loss.detach(), out, {k: (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(names, grads)}, stats


def weighted_batch_stats(x, w, n):
    """(mean, biased variance) of the n rows the weighted rows x stand for."""
    with torch.no_grad():
        mean = (w[:, None] * x).sum(0) / n
        return mean, (w[:, None] * (x - mean) ** 2).sum(0) / n


def dense_oracle_step(orc, sd, batch, dtype=torch.float64):
    """The dense oracle step -> (loss, logits, gradients, (batch mean, biased batch variance))."""
    p = orc.to_torch_params(sd, dtype=dtype)
    tb = {k: torch.from_numpy(v) for k, v in batch.items() if isinstance(v, np.ndarray) and v.ndim > 0}
    with orc.precision(dtype):
        r, aux = orc.user_model_forward(p, tb["x_history"], tb["x_target"], tb["x_global"], training=True, return_aux=True)
        loss = orc.user_model_loss(p, tb["user_id"], r, tb["label"])
        names = [k for k in p if k not in orc.BUFFER_KEYS]
        grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    stats = (aux["e2"].detach().mean(0), aux["bn_var"].detach())
    return loss.detach(), r.detach(), {k: (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(names, grads)}, stats


def brute_force_rows(counts, T, max_groups):
    """Fewest kept candidate rows over ALL partitions of the sorted counts into at most ``max_groups`` contiguous groups."""
    n = sorted(min(max(int(x), 0), T) for x in counts)
    B = len(n)
    if B == 0:
        return 0
    best = None
    for k in range(min(max_groups, B)):
        for cuts in itertools.combinations(range(1, B), k):
            edges = (0,) + cuts + (B,)
            rows = sum((edges[i + 1] - edges[i]) * min(T, n[edges[i + 1] - 1] + 1) for i in range(len(edges) - 1))
            best = rows if best is None else min(best, rows)
    return best
