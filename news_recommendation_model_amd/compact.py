"""Host-side plan of the compact scoring path (inference only).

A processed test set pads every impression's candidate list with all-zero rows to the longest list of the whole data set, and
the reference's ``model_test`` trims only the padding common to a batch (test.py:48-56).  All padded candidates of one
impression have the same inputs, hence the same logit, so impression ``b`` with ``n_b`` live candidates and
``e'_b = empty_b - trim`` padded columns left after the trim needs ``n_b + [e'_b > 0]`` forward rows -- its live candidates
and ONE representative padded candidate (column ``n_b``) whose ``exp`` enters the first softmax ``e'_b`` times -- instead of
``T' = n_b + e'_b``.  ``build_plan`` turns the host ``empty_num`` into the index tables the ragged kernels read.  Plain numpy:
no device work, testable on the CPU.
"""
from __future__ import annotations

import numpy as np


class CompactPlan:
    """Tables of one batch (all int32 numpy arrays on the host; ``upload`` puts them on a device with ONE pinned copy).

      B, T, trim, Tp     batch rows, columns of the input, common trim, columns kept (``T' = T - trim``)
      N                  compact candidate rows, ``sum_b (n_b + [e'_b > 0])``
      live [B]           ``n_b``
      pad_mult [B]       ``e'_b``
      cand_off [B + 1]   prefix sums of the rows per impression
      cand_imp [N]       impression of each compact row
      src [N]            source cell ``b * T + t`` of each compact row in the flattened [B * T] input rows
      max_count          longest list, ``max_b (cand_off[b + 1] - cand_off[b])`` (0 for an empty plan)
    """

    __slots__ = ("B", "T", "trim", "Tp", "N", "live", "pad_mult", "cand_off", "cand_imp", "src", "max_count", "device_tables")

    @property
    def dense(self):
        """No row keeps padding after the trim (``N = B * T'``): the compact path has nothing to drop."""
        return self.N == self.B * self.Tp

    def upload(self, device):
        """-> dict of int32 device views (cand_off, pad_mult, cand_imp) of ONE buffer copied from pinned host memory
        (non-blocking: no synchronisation).  Cached on the plan.  ``src`` stays on the host: the gather kernel derives a row's
        source cell from cand_off, the table is the plan's own record (and what the tests check the kernel against)."""
        import torch
        if self.device_tables is not None and self.device_tables["cand_off"].device == torch.device(device):
            return self.device_tables
        B, N = self.B, self.N
        host = torch.empty(2 * B + 1 + N, dtype=torch.int32)
        if torch.cuda.is_available():
            host = host.pin_memory()
        host.numpy()[:] = np.concatenate([self.cand_off, self.pad_mult, self.cand_imp])
        dev = host.to(device, non_blocking=True)
        self.device_tables = {"cand_off": dev[:B + 1], "pad_mult": dev[B + 1:2 * B + 1], "cand_imp": dev[2 * B + 1:],
                              "_host": host}        # (the pinned source lives as long as the copy may run)
        return self.device_tables


def build_plan(empty_num, T):
    """``empty_num`` [B]: trailing all-padding candidates per row (the DataLoader's HOST tensor or array: no device work;
    a device-resident tensor is read with ``.cpu()``, which costs one synchronise per batch); ``T``: candidate columns of the
    batch.  Entries are clamped to [0, T], as the scoring tail clamps them."""
    if hasattr(empty_num, "detach"):
        empty_num = empty_num.detach().cpu().numpy()
    empty = np.clip(np.asarray(empty_num).reshape(-1).astype(np.int64), 0, int(T))
    B, T = int(empty.shape[0]), int(T)
    if T < 0:
        raise ValueError(f"build_plan: T={T}")
    trim = int(empty.min()) if B else 0                          # test.py:48-56
    Tp = T - trim
    pad = empty - trim                                           # e'_b
    live = Tp - pad                                              # n_b
    count = live + (pad > 0)
    cand_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(count, out=cand_off[1:])
    N = int(cand_off[B])
    if N >= 2 ** 31 or B * T >= 2 ** 31:
        raise ValueError("build_plan: more than 2^31 candidate rows")
    cand_imp = np.repeat(np.arange(B, dtype=np.int64), count)
    within = np.arange(N, dtype=np.int64) - cand_off[cand_imp]   # column of the compact row in its impression: 0 .. n_b (n_b = the pad)
    plan = CompactPlan()
    plan.B, plan.T, plan.trim, plan.Tp, plan.N = B, T, trim, Tp, N
    plan.live, plan.pad_mult = live.astype(np.int32), pad.astype(np.int32)
    plan.cand_off, plan.cand_imp = cand_off.astype(np.int32), cand_imp.astype(np.int32)
    plan.src = (cand_imp * T + within).astype(np.int32)
    plan.max_count = int(count.max()) if B else 0
    plan.device_tables = None
    return plan


def compact_scores_reference(logits, plan, dtype=np.float64):
    """The compact formula in numpy (the semantics the ragged scoring tail implements; tests compare it with the oracle's dense
    ``model_test_scores``): ``logits`` = list (one per model) of [N] compact logits -> scores [B, T'] with 0 on padding columns.

        p_i = exp(l_i - m) / (sum_{j < n} exp(l_j - m) + e' exp(l_pad - m)),  m = max over the live and the pad logit
        mean over the models, then (only where e' > 0) softmax over the n live values                      (test.py:58-70)
    """
    out = np.zeros((plan.B, plan.Tp), dtype=dtype)
    for b in range(plan.B):
        c0, n, e = int(plan.cand_off[b]), int(plan.live[b]), int(plan.pad_mult[b])
        if n == 0:
            continue
        acc = np.zeros(n, dtype=dtype)
        for lg in logits:
            x = np.asarray(lg, dtype=dtype)[c0:int(plan.cand_off[b + 1])]
            m = x.max()
            ex = np.exp(x - m)
            acc += ex[:n] / (ex[:n].sum() + (e * ex[n] if e > 0 else 0.0))
        acc /= len(logits)
        if e > 0:
            ex = np.exp(acc - acc.max())
            acc = ex / ex.sum()
        out[b, :n] = acc
    return out
