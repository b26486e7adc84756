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

    With ``build_plan(..., history_len=, H=)`` the plan also drops the trailing all-zero history rows; without it
    these fields are None:
      H                  history rows of the input
      hist_len [B]       ``L_b``: 1 + the last live history row, clamped to [0, H]
      hist_mult [B]      ``H - L_b``: how many equal rows the representative padded row (row ``L_b``) stands for
      hist_off [B + 1]   prefix sums of ``K_b = L_b + [L_b < H]``, the rows kept per impression
      R                  kept history rows, ``sum_b K_b``
      hist_src [R]       source row ``b * H + j`` of each kept row in the flattened [B * H] history rows
      k_max              longest kept history
      tile_pre [B + 1]   prefix sums of ``count_b * ceil(K_b / 16)``: the scores of a compact candidate are whole 16-row tiles
      Mt                 ``tile_pre[B]``: 16-row score tiles of the batch
      history_dense      every ``L_b = H``: nothing to drop
    """

    __slots__ = ("B", "T", "trim", "Tp", "N", "live", "pad_mult", "cand_off", "cand_imp", "src", "max_count", "device_tables",
                 "H", "hist_len", "hist_mult", "hist_off", "R", "hist_src", "k_max", "tile_pre", "Mt", "history_dense")

    @property
    def has_history(self):
        return self.hist_off is not None

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
        parts = [self.cand_off, self.pad_mult, self.cand_imp]
        if self.has_history:                        # the [B]-sized history tables ride in the same copy, behind today's
            parts += [self.hist_off, self.hist_mult, self.tile_pre]
        host = torch.empty(sum(len(p) for p in parts), dtype=torch.int32)
        if torch.cuda.is_available():
            host = host.pin_memory()
        host.numpy()[:] = np.concatenate(parts)
        dev = host.to(device, non_blocking=True)
        self.device_tables = {"cand_off": dev[:B + 1], "pad_mult": dev[B + 1:2 * B + 1], "cand_imp": dev[2 * B + 1:2 * B + 1 + N],
                              "_host": host}        # (the pinned source lives as long as the copy may run)
        if self.has_history:
            o = 2 * B + 1 + N
            t = self.device_tables
            t.update(hist_off=dev[o:o + B + 1], hist_mult=dev[o + B + 1:o + 2 * B + 1], tile_pre=dev[o + 2 * B + 1:o + 3 * B + 2])
            if dev.is_cuda:                         # the per-tile table (Mt x 16 bytes) is built ON the device from the [B + 1] tables
                from . import ops
                t["tile_tab"] = ops.history_tiles(t["cand_imp"], t["cand_off"], t["hist_off"], t["tile_pre"], self.R, self.Mt)
        return self.device_tables


def build_plan(empty_num, T, history_len=None, H=None):
    """``empty_num`` [B]: trailing all-padding candidates per row (the DataLoader's HOST tensor or array: no device work;
    a device-resident tensor is read with ``.cpu()``, which costs one synchronise per batch); ``T``: candidate columns of the
    batch.  Entries are clamped to [0, T], as the scoring tail clamps them.
    ``history_len`` [B] (with ``H``, the history rows of the batch): ``L_b`` as ``ops.history_len`` measures it on the device, a host
    array (entries clamped to [0, H]); the plan then carries the history tables as well."""
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
    for k in ("H", "hist_len", "hist_mult", "hist_off", "R", "hist_src", "k_max", "tile_pre", "Mt", "history_dense"):
        setattr(plan, k, None)
    if history_len is not None:
        if H is None or int(H) < 0:
            raise ValueError(f"build_plan: history_len needs H >= 0, got H={H}")
        if hasattr(history_len, "detach"):
            history_len = history_len.detach().cpu().numpy()
        H = int(H)
        L = np.clip(np.asarray(history_len).reshape(-1).astype(np.int64), 0, H)
        if L.shape[0] != B:
            raise ValueError(f"build_plan: history_len has {L.shape[0]} entries for {B} impressions")
        K = L + (L < H)                                          # the live rows and ONE representative padded row
        hist_off = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(K, out=hist_off[1:])
        tile_pre = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(count * ((K + 15) // 16), out=tile_pre[1:])
        R, Mt = int(hist_off[B]), int(tile_pre[B])
        if B * H >= 2 ** 31 or 16 * Mt >= 2 ** 31:
            raise ValueError("build_plan: more than 2^31 history or score rows")
        imp = np.repeat(np.arange(B, dtype=np.int64), K)
        plan.H, plan.R, plan.Mt = H, R, Mt
        plan.hist_len, plan.hist_mult = L.astype(np.int32), (H - L).astype(np.int32)
        plan.hist_off, plan.tile_pre = hist_off.astype(np.int32), tile_pre.astype(np.int32)
        plan.hist_src = (imp * H + np.arange(R, dtype=np.int64) - hist_off[imp]).astype(np.int32)
        plan.k_max = int(K.max()) if B else 0
        plan.history_dense = bool((L == H).all())
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


# ------------------------------------------------------------------------------------------------ training: history length groups
#   The compacted TRAINING step sorts the batch by history length and cuts it into a few contiguous groups, each
# trimmed to its own height H_g and run through the dense kernels; only the pool sees that the last kept row of a trimmed group
# stands for w_g = H - H_g + 1 equal padded rows.
MAX_GROUPS = 2          # default of plan_history_groups / train_step.  Speed: not measured on an MI355X -- the conservative value
MIN_SAVING = 0.25       # a plan that drops less than this share of the B * H history rows runs dense.  Not measured either.
GROUPS_CAP = 64         # csrc/compact.hpp HISTORY_GROUPS_MAX


class HistoryGroupPlan:
    """Length groups of one batch (host numpy; ``upload`` puts the tables on a device with ONE pinned copy).

      B, H, G, quantum   impressions, history rows of the input, groups, the multiple every trimmed height is rounded up to
      hist_len [B]       ``L_b`` clamped to [0, H], in the CALLER's order
      perm [B]           stable argsort of hist_len: sorted impression i is impression perm[i] of the batch
      inverse [B]        ``inverse[perm] == arange(B)``: row of the sorted order that holds impression b
      bounds [G + 1]     group g = sorted impressions bounds[g] .. bounds[g + 1] - 1
      H_g [G]            rows kept per impression of the group: min(H, quantum * ceil((max L_b + 1) / quantum))
      w_g [G]            ``H - H_g + 1``: how many equal rows row H_g - 1 stands for (1 where H_g == H: the dense computation)
      row_off [G + 1]    first row of each group in the grouped history arena, ``row_off[g + 1] - row_off[g] = B_g * H_g``
      R                  ``row_off[G]``: history rows the step computes instead of B * H
      saving             ``1 - R / (B * H)``
      dense              nothing worth dropping: every H_g == H, or saving < MIN_SAVING
    """

    __slots__ = ("B", "H", "G", "quantum", "hist_len", "perm", "inverse", "bounds", "H_g", "w_g", "row_off", "R", "saving", "dense",
                 "device_tables")

    def upload(self, device):
        """-> dict of int32 device views (perm, inverse, bounds, row_off, H_g) of ONE buffer copied from pinned host memory
        (non-blocking).  Cached on the plan."""
        import torch
        if self.device_tables is not None and self.device_tables["perm"].device == torch.device(device):
            return self.device_tables
        parts = [("perm", self.perm), ("inverse", self.inverse), ("bounds", self.bounds), ("row_off", self.row_off), ("H_g", self.H_g)]
        host = torch.empty(sum(len(p) for _, p in parts), dtype=torch.int32)
        if torch.cuda.is_available():
            host = host.pin_memory()
        host.numpy()[:] = np.concatenate([p for _, p in parts])
        dev = host.to(device, non_blocking=True)
        tabs, o = {"_host": host}, 0
        for name, p in parts:
            tabs[name] = dev[o:o + len(p)]
            o += len(p)
        self.device_tables = tabs
        return tabs


def plan_history_groups(hist_len, H, max_groups=None, quantum=16):
    """``hist_len`` [B]: ``L_b`` as ``ops.history_len`` measures it (host array or tensor; entries are clamped to [0, H]).  Sorts the
    impressions by length (stable) and cuts the sorted order into at most ``max_groups`` contiguous groups that minimise the kept rows
    ``sum_g B_g * H_g`` -- contiguous groups of the sorted order are optimal (a group's height is set by its longest member), and the
    dynamic programme over the cut points is exact.  A group only ever ends where the quantised height changes: a cut inside a run
    of equal heights saves nothing.  Ties go to fewer groups (every group multiplies the launches)."""
    if hasattr(hist_len, "detach"):
        hist_len = hist_len.detach().cpu().numpy()
    H, q = int(H), int(quantum)
    max_groups = MAX_GROUPS if max_groups is None else int(max_groups)
    if H < 1 or q < 1 or not 1 <= max_groups <= GROUPS_CAP:
        raise ValueError(f"plan_history_groups: H={H} quantum={q} max_groups={max_groups} (H, quantum >= 1, 1 <= max_groups <= {GROUPS_CAP})")
    L = np.clip(np.asarray(hist_len).reshape(-1).astype(np.int64), 0, H)
    B = int(L.shape[0])
    if B * H >= 2 ** 31:
        raise ValueError("plan_history_groups: more than 2^31 history rows")
    perm = np.argsort(L, kind="stable")
    inverse = np.empty(B, dtype=np.int64)
    inverse[perm] = np.arange(B)
    height = np.minimum(H, q * ((L[perm] + q) // q))                 # q * ceil((L + 1) / q) of each sorted impression: non-decreasing
    ends = (np.flatnonzero(np.diff(height)) + 1).tolist() + [B] if B else []      # where a group may end
    K = len(ends)
    h_end = [int(height[e - 1]) for e in ends]
    INF = float("inf")
    # cost[g][k]: fewest rows of the first ends[k] impressions in exactly g + 1 groups, the last of which ends at ends[k]
    cost = [[INF] * K for _ in range(min(max_groups, K))]
    back = [[-1] * K for _ in range(min(max_groups, K))]
    for k in range(K):
        cost[0][k] = ends[k] * h_end[k]
    for g in range(1, len(cost)):
        for k in range(g, K):
            for i in range(g - 1, k):
                c = cost[g - 1][i] + (ends[k] - ends[i]) * h_end[k]
                if c < cost[g][k]:
                    cost[g][k], back[g][k] = c, i
    cuts = []
    if K:
        g = min(range(len(cost)), key=lambda gg: (cost[gg][K - 1], gg))
        k = K - 1
        while k >= 0 and g >= 0:
            cuts.append(ends[k])
            k, g = back[g][k], g - 1
    bounds = np.array([0] + cuts[::-1], dtype=np.int64)
    G = len(bounds) - 1
    H_g = np.array([int(height[bounds[g + 1] - 1]) for g in range(G)], dtype=np.int64)
    row_off = np.zeros(G + 1, dtype=np.int64)
    np.cumsum(np.diff(bounds) * H_g, out=row_off[1:])
    plan = HistoryGroupPlan()
    plan.B, plan.H, plan.G, plan.quantum = B, H, G, q
    plan.hist_len, plan.perm, plan.inverse = L.astype(np.int32), perm.astype(np.int32), inverse.astype(np.int32)
    plan.bounds, plan.H_g, plan.w_g, plan.row_off = bounds.astype(np.int32), H_g.astype(np.int32), (H - H_g + 1).astype(np.int32), row_off.astype(np.int32)
    plan.R = int(row_off[G])
    plan.saving = 1.0 - plan.R / (B * H) if B else 0.0
    plan.dense = bool((H_g == H).all()) or plan.saving < MIN_SAVING
    plan.device_tables = None
    return plan
