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


def _upload(plan, parts, device):
    """The group plans' ``upload``: the int32 host arrays ``parts`` (attribute names) of ``plan`` as device views of ONE buffer copied from
    pinned host memory (non-blocking).  Cached on the plan."""
    import torch
    if plan.device_tables is not None and plan.device_tables[parts[0]].device == torch.device(device):
        return plan.device_tables
    arrays = [getattr(plan, name) for name in parts]
    host = torch.empty(sum(len(a) for a in arrays), dtype=torch.int32)
    if torch.cuda.is_available():
        host = host.pin_memory()
    host.numpy()[:] = np.concatenate(arrays)
    dev = host.to(device, non_blocking=True)
    tabs, o = {"_host": host}, 0                # (the pinned source lives as long as the copy may run)
    for name, a in zip(parts, arrays):
        tabs[name] = dev[o:o + len(a)]
        o += len(a)
    plan.device_tables = tabs
    return tabs


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
      cand               None, or the ``CandidateGroupPlan`` cut along these groups (``plan_candidate_groups(..., history_plan=)``,
                         DESIGN.md section 5f): the step then trims every group in the candidate axis as well
    """

    __slots__ = ("B", "H", "G", "quantum", "hist_len", "perm", "inverse", "bounds", "H_g", "w_g", "row_off", "R", "saving", "dense",
                 "device_tables", "cand")

    def upload(self, device):
        """-> dict of int32 device views (perm, inverse, bounds, row_off, H_g) of ONE buffer copied from pinned host memory
        (non-blocking).  Cached on the plan."""
        return _upload(self, ("perm", "inverse", "bounds", "row_off", "H_g"), device)


def _cut_sorted(height, max_groups):
    """The dynamic programme both group planners share.  ``height`` [B]: the non-decreasing kept height of each sorted impression; -> the
    ascending end points of at most ``max_groups`` contiguous groups that minimise ``sum_g B_g * height of the group's last member``.  A
    group only ever ends where the height changes; ties go to fewer groups."""
    B = len(height)
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
    return cuts[::-1]


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
    cuts = _cut_sorted(height, max_groups)
    bounds = np.array([0] + cuts, dtype=np.int64)
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
    plan.cand = None
    return plan


# ------------------------------------------------------------------------------------------------ training: candidate count groups
#   The training ETL pads every candidate list with all-zero rows to T columns; all padded candidates of one impression
# have the same inputs and the same label.  The batch is sorted by n_b = T - empty_b and cut into a few contiguous groups, each trimmed to
# T_g = min(T, max n_b + 1) columns: where T_g < T the group's last column is a padded candidate that stands for w_g = T - T_g + 1 equal ones,
# which BatchNorm's batch statistics and the loss see as a row weight.  MAX_GROUPS and MIN_SAVING are the defaults here too: both unmeasured.
class CandidateGroupPlan:
    """Candidate count groups of one batch (host numpy; ``upload`` puts the tables on a device with ONE pinned copy).

      B, T, G            impressions, candidate columns of the input, groups
      count [B]          ``n_b = T - empty_b`` with empty_b clamped to [0, T], in the CALLER's order
      perm [B]           stable argsort of count: sorted impression i is impression perm[i] of the batch
      inverse [B]        ``inverse[perm] == arange(B)``
      bounds [G + 1]     group g = sorted impressions bounds[g] .. bounds[g + 1] - 1
      T_g [G]            columns kept per impression of the group: min(T, max n_b + 1)
      w_g [G]            ``T - T_g + 1``: how many equal candidates column T_g - 1 stands for (1 where T_g == T: the dense computation)
      row_off [G + 1]    first row of each group in the candidate arena, ``row_off[g + 1] - row_off[g] = B_g * T_g``
      N                  ``row_off[G]``: candidate rows the step computes instead of B * T
      expand [B * T]     arena row of dense cell ``b * T + t`` in the caller's order (a dropped cell maps to its group's last column)
      saving             ``1 - N / (B * T)``
      dense              nothing worth dropping: every T_g == T, or saving < MIN_SAVING
    """

    __slots__ = ("B", "T", "G", "count", "perm", "inverse", "bounds", "T_g", "w_g", "row_off", "N", "expand", "saving", "dense", "device_tables")

    def upload(self, device):
        """-> dict of int32 device views (perm, bounds, row_off, T_g, expand) of ONE buffer copied from pinned host memory (non-blocking)."""
        return _upload(self, ("perm", "bounds", "row_off", "T_g", "expand"), device)


def plan_candidate_groups(empty_num, T, max_groups=None, history_plan=None):
    """``empty_num`` [B]: trailing all-padding candidates per impression (the DataLoader's HOST tensor or array; a device tensor costs one
    ``.cpu()``); entries are clamped to [0, T].  Sorts the impressions by ``n_b = T - empty_b`` (stable) and cuts the sorted order with the
    dynamic programme of ``plan_history_groups`` (cost ``sum_g B_g * T_g``, quantum 1, cuts only where n_b changes, ties to fewer groups).
    ``history_plan`` (a ``HistoryGroupPlan`` of the same batch): no joint planner -- order and cuts stay the history plan's, every group
    additionally gets ``T_g = min(T, max n_b + 1)`` of its members, and ``saving`` is ``1 - sum_g B_g T_g H_g / (B T H)``."""
    if hasattr(empty_num, "detach"):
        empty_num = empty_num.detach().cpu().numpy()
    T = int(T)
    max_groups = MAX_GROUPS if max_groups is None else int(max_groups)
    if T < 1 or not 1 <= max_groups <= GROUPS_CAP:
        raise ValueError(f"plan_candidate_groups: T={T} max_groups={max_groups} (T >= 1, 1 <= max_groups <= {GROUPS_CAP})")
    count = T - np.clip(np.asarray(empty_num).reshape(-1).astype(np.int64), 0, T)
    B = int(count.shape[0])
    if B * T >= 2 ** 31:
        raise ValueError("plan_candidate_groups: more than 2^31 candidate rows")
    if history_plan is not None:
        if history_plan.B != B:
            raise ValueError(f"plan_candidate_groups: empty_num has {B} entries for a history plan of {history_plan.B} impressions")
        perm, inverse, bounds = (np.asarray(a).astype(np.int64) for a in (history_plan.perm, history_plan.inverse, history_plan.bounds))
        width = np.minimum(T, count[perm] + 1)
        G = len(bounds) - 1
        T_g = np.array([int(width[bounds[g]:bounds[g + 1]].max()) for g in range(G)], dtype=np.int64)
    else:
        perm = np.argsort(count, kind="stable")
        inverse = np.empty(B, dtype=np.int64)
        inverse[perm] = np.arange(B)
        width = np.minimum(T, count[perm] + 1)                       # the live candidates and ONE representative padded one
        bounds = np.array([0] + _cut_sorted(width, max_groups), dtype=np.int64)
        G = len(bounds) - 1
        T_g = np.array([int(width[bounds[g + 1] - 1]) for g in range(G)], dtype=np.int64)
    row_off = np.zeros(G + 1, dtype=np.int64)
    np.cumsum(np.diff(bounds) * T_g, out=row_off[1:])
    group = np.repeat(np.arange(G, dtype=np.int64), np.diff(bounds))[inverse] if B else np.zeros(0, dtype=np.int64)     # group of impression b
    first = (row_off[group] + (inverse - bounds[group]) * T_g[group]) if B else group
    expand = first[:, None] + np.minimum(np.arange(T, dtype=np.int64)[None, :], (T_g[group] - 1)[:, None]) if B else np.zeros((0, T), dtype=np.int64)
    plan = CandidateGroupPlan()
    plan.B, plan.T, plan.G = B, T, G
    plan.count, plan.perm, plan.inverse = count.astype(np.int32), perm.astype(np.int32), inverse.astype(np.int32)
    plan.bounds, plan.T_g, plan.w_g, plan.row_off = bounds.astype(np.int32), T_g.astype(np.int32), (T - T_g + 1).astype(np.int32), row_off.astype(np.int32)
    plan.N = int(row_off[G])
    plan.expand = expand.reshape(-1).astype(np.int32)
    plan.saving = 1.0 - plan.N / (B * T) if B else 0.0
    if history_plan is not None and B:
        plan.saving = 1.0 - float((np.diff(bounds) * T_g * np.asarray(history_plan.H_g).astype(np.int64)).sum()) / (B * T * history_plan.H)
    plan.dense = bool((T_g == T).all()) or plan.saving < MIN_SAVING
    plan.device_tables = None
    return plan


def candidate_saving_bound(empty_num, T):
    """The share of the B * T candidate rows NO grouping can drop more than: every impression its own group, ``1 - sum_b min(T, n_b + 1) /
    (B T)``.  One pass over the counts: ``train_step`` asks this first, so a batch with nothing worth dropping pays neither the sort nor the
    dynamic programme nor the tables (at launch-bound sizes the plan's host time is a measurable part of a step)."""
    if hasattr(empty_num, "detach"):
        empty_num = empty_num.detach().cpu().numpy()
    T = int(T)
    empty = np.asarray(empty_num).reshape(-1)
    B = empty.shape[0]
    if B == 0 or T < 1:
        return 0.0
    # min(T, n_b + 1) = T + 1 - clip(empty_b, 1, T)
    return 1.0 - (B * (T + 1) - float(np.clip(empty, 1, T).sum())) / (B * T)


def full_height_history_plan(cand, H):
    """The ``HistoryGroupPlan`` of a step that compacts the candidate lists only: ``cand``'s order and cuts, every group at the full height H
    (``w_g = 1``: the dense pool), carrying ``cand``."""
    H = int(H)
    if H < 1 or cand.B * H >= 2 ** 31:
        raise ValueError(f"full_height_history_plan: H={H} for {cand.B} impressions")
    plan = HistoryGroupPlan()
    plan.B, plan.H, plan.G, plan.quantum = cand.B, H, cand.G, 1
    plan.hist_len = np.full(cand.B, H, dtype=np.int32)
    plan.perm, plan.inverse, plan.bounds = cand.perm, cand.inverse, cand.bounds
    plan.H_g, plan.w_g = np.full(cand.G, H, dtype=np.int32), np.ones(cand.G, dtype=np.int32)
    plan.row_off = (cand.bounds.astype(np.int64) * H).astype(np.int32)
    plan.R, plan.saving, plan.dense = cand.B * H, 0.0, True
    plan.device_tables = None
    plan.cand = cand
    return plan


# ------------------------------------------------------------------------------------------------ training: one group plan per epoch
#   A table-fed epoch knows every impression's history length and empty_num on the host before it starts, and the order
# INSIDE a batch is free (loss, BatchNorm statistics and the tally do not depend on it).  Every full batch's slice of the epoch's order is
# sorted by length on the host, and ONE plan is cut that every full batch fits: the height of sorted position i is the maximum over the
# batches.  The plan is static and the batch arrives sorted (perm = identity), so the grouped step is one fixed sequence of launches.
def _epoch_lengths(hist_len, empty_num, H, T):
    L = np.clip(np.asarray(hist_len).reshape(-1).astype(np.int64), 0, int(H))
    n = int(T) - np.clip(np.asarray(empty_num).reshape(-1).astype(np.int64), 0, int(T))
    if L.shape != n.shape:
        raise ValueError(f"epoch plan: {L.shape[0]} history lengths and {n.shape[0]} empty_num entries")
    return L, n


def sort_epoch_order(hist_len, empty_num, order, B, H, T, compact_history):
    """``order`` with every full batch's slice [i * B, (i + 1) * B) stably sorted ascending by history length (``compact_history``) or by
    ``n_b = T - empty_b``; the trailing partial batch is left as it is.  Batch membership does not change."""
    L, n = _epoch_lengths(hist_len, empty_num, H, T)
    order = np.array(order, dtype=np.int64).reshape(-1)
    B = int(B)
    nb = order.shape[0] // B if B > 0 else 0
    if order.size and (order.min() < 0 or order.max() >= L.shape[0]):
        raise IndexError(f"epoch plan: order holds an impression outside [0, {L.shape[0]})")
    if nb:
        full = order[:nb * B].reshape(nb, B)
        key = (L if compact_history else n)[full]
        order[:nb * B] = np.take_along_axis(full, np.argsort(key, axis=1, kind="stable"), axis=1).reshape(-1)
    return order


class EpochGroupPlan:
    """One static group plan for all full batches of an epoch (host numpy; ``upload`` puts the tables on a device with ONE pinned copy).

      B, H, T, G, quantum   impressions of a full batch, history rows, candidate columns, groups, the multiple a trimmed height is rounded to
      n_batches             full batches the plan was cut for
      order [N]             the epoch's order with every full batch sorted (``sort_epoch_order``)
      hist                  ``HistoryGroupPlan`` with ``perm = inverse = arange(B)`` (the batch arrives sorted); ``hist.cand`` is ``cand``
      cand                  None, or the ``CandidateGroupPlan`` along the same order and cuts (identity ``perm``, static ``expand``)
      bounds [G + 1], H_g [G], hist_row_off [G + 1], T_g [G], cand_row_off [G + 1], expand [B * T]
                            what the grouped assemble kernel and the step read (T_g = T, cand_row_off = bounds * T without ``cand``)
      R, N                  rows of the history and of the candidate arena
      saving                ``1 - R / (B H)``, with candidate groups ``1 - sum_g B_g T_g H_g / (B T H)``
      dense                 nothing trimmed, no full batch, or ``saving`` below ``min_saving`` (None: ``MIN_SAVING``)
    """

    __slots__ = ("B", "H", "T", "G", "quantum", "n_batches", "order", "hist", "cand", "compact_history", "compact_candidates", "bounds", "H_g",
                 "hist_row_off", "T_g", "cand_row_off", "expand", "R", "N", "saving", "dense", "device_tables")

    def upload(self, device):
        """-> dict of int32 device views (bounds, H_g, hist_row_off, T_g, cand_row_off, expand) of ONE buffer copied from pinned host memory."""
        return _upload(self, ("bounds", "H_g", "hist_row_off", "T_g", "cand_row_off", "expand"), device)

    def fits(self, hist_len, empty_num, order):
        """Whether every full batch of ANOTHER epoch (its lengths and order; sorted here the way the plan's own order was) fits this plan:
        every member of group g has ``L < H_g`` or ``H_g == H``, and ``n_b < T_g`` or ``T_g == T``."""
        L, n = _epoch_lengths(hist_len, empty_num, self.H, self.T)
        order = sort_epoch_order(L, self.T - n, order, self.B, self.H, self.T, self.compact_history)
        nb = order.shape[0] // self.B
        if nb == 0:
            return True
        full = order[:nb * self.B].reshape(nb, self.B)
        size = np.diff(self.bounds)
        h_pos, t_pos = np.repeat(self.H_g, size).astype(np.int64), np.repeat(self.T_g, size).astype(np.int64)
        return bool((((L[full] < h_pos) | (h_pos == self.H)) & ((n[full] < t_pos) | (t_pos == self.T))).all())


def plan_epoch_groups(hist_len, empty_num, order, B, H, T, compact_history, compact_candidates, max_groups=None, quantum=16, min_saving=None):
    """``hist_len`` / ``empty_num`` [N]: every impression's history length and trailing padded candidates (host arrays:
    ``tables.history_len`` / ``tables.empty_num_all``), ``order`` the epoch's impression order.  Sorts every full batch of ``order`` by
    length and cuts ONE plan for all of them with the dynamic programme of ``plan_history_groups`` over the ENVELOPE: the position-wise
    maximum over the full batches of ``min(H, q * ceil((L + 1) / q))`` -- or, with ``compact_candidates`` alone, of ``min(T, n_b + 1)``.
    There is no joint planner: with both flags the cuts are the history's and every group additionally gets
    ``T_g = min(T, 1 + max n_b)`` over its positions in all full batches."""
    B, H, T, q = int(B), int(H), int(T), int(quantum)
    max_groups = MAX_GROUPS if max_groups is None else int(max_groups)
    if B < 1 or H < 1 or T < 1 or q < 1 or not 1 <= max_groups <= GROUPS_CAP:
        raise ValueError(f"plan_epoch_groups: B={B} H={H} T={T} quantum={q} max_groups={max_groups} (B, H, T, quantum >= 1, 1 <= max_groups <= "
                         f"{GROUPS_CAP})")
    if not (compact_history or compact_candidates):
        raise ValueError("plan_epoch_groups: neither compact_history nor compact_candidates")
    if B * H >= 2 ** 31 or B * T >= 2 ** 31:
        raise ValueError("plan_epoch_groups: more than 2^31 history or candidate rows")
    L, n = _epoch_lengths(hist_len, empty_num, H, T)
    order = sort_epoch_order(L, T - n, order, B, H, T, compact_history)
    nb = order.shape[0] // B
    full = order[:nb * B].reshape(nb, B)
    height = np.minimum(H, q * ((L[full] + q) // q)).max(axis=0) if nb else np.full(B, H, dtype=np.int64)        # the envelope, per position
    width = np.minimum(T, n[full] + 1).max(axis=0) if nb else np.full(B, T, dtype=np.int64)
    if compact_history:                                          # rows sorted by L: the position-wise maximum is non-decreasing as well
        bounds = np.array([0] + _cut_sorted(height, max_groups), dtype=np.int64)
    else:
        height = np.full(B, H, dtype=np.int64)
        bounds = np.array([0] + _cut_sorted(width, max_groups), dtype=np.int64)
    G = len(bounds) - 1
    size = np.diff(bounds)
    H_g = np.array([int(height[bounds[g + 1] - 1]) for g in range(G)], dtype=np.int64)
    T_g = (np.array([int(width[bounds[g]:bounds[g + 1]].max()) for g in range(G)], dtype=np.int64) if compact_candidates
           else np.full(G, T, dtype=np.int64))
    with_cand = bool(compact_candidates and (T_g < T).any())
    hist_row_off, cand_row_off = np.zeros(G + 1, dtype=np.int64), np.zeros(G + 1, dtype=np.int64)
    np.cumsum(size * H_g, out=hist_row_off[1:])
    np.cumsum(size * T_g, out=cand_row_off[1:])
    ident = np.arange(B, dtype=np.int32)
    hist = HistoryGroupPlan()
    hist.B, hist.H, hist.G, hist.quantum = B, H, G, q if compact_history else 1
    hist.hist_len = ((L[full].max(axis=0) if nb else np.zeros(B)) if compact_history else np.full(B, H)).astype(np.int32)
    hist.perm, hist.inverse = ident, ident.copy()
    hist.bounds, hist.H_g, hist.w_g, hist.row_off = bounds.astype(np.int32), H_g.astype(np.int32), (H - H_g + 1).astype(np.int32), hist_row_off.astype(np.int32)
    hist.R = int(hist_row_off[G])
    hist.saving = 1.0 - hist.R / (B * H)
    hist.device_tables, hist.cand = None, None
    group = np.repeat(np.arange(G, dtype=np.int64), size)        # group of sorted position b
    first = cand_row_off[group] + (np.arange(B) - bounds[group]) * T_g[group]
    expand = first[:, None] + np.minimum(np.arange(T, dtype=np.int64)[None, :], (T_g[group] - 1)[:, None])
    saving = 1.0 - float((size * T_g * H_g).sum()) / (B * T * H)
    cand = None
    if with_cand:
        cand = CandidateGroupPlan()
        cand.B, cand.T, cand.G = B, T, G
        cand.count = (n[full].max(axis=0) if nb else np.zeros(B)).astype(np.int32)
        cand.perm, cand.inverse = ident, ident.copy()
        cand.bounds, cand.T_g, cand.w_g, cand.row_off = bounds.astype(np.int32), T_g.astype(np.int32), (T - T_g + 1).astype(np.int32), cand_row_off.astype(np.int32)
        cand.N = int(cand_row_off[G])
        cand.expand = expand.reshape(-1).astype(np.int32)
        cand.saving = saving
        cand.device_tables = None
        hist.cand = cand
    floor = MIN_SAVING if min_saving is None else float(min_saving)
    hist.dense = bool((H_g == H).all()) or hist.saving < floor
    if cand is not None:
        cand.dense = saving < floor
    plan = EpochGroupPlan()
    plan.B, plan.H, plan.T, plan.G, plan.quantum, plan.n_batches = B, H, T, G, q, nb
    plan.order, plan.hist, plan.cand = order, hist, cand
    plan.compact_history, plan.compact_candidates = bool(compact_history), bool(compact_candidates)
    plan.bounds, plan.H_g, plan.hist_row_off = hist.bounds, hist.H_g, hist.row_off
    plan.T_g, plan.cand_row_off, plan.expand = T_g.astype(np.int32), cand_row_off.astype(np.int32), expand.reshape(-1).astype(np.int32)
    plan.R, plan.N = hist.R, int(cand_row_off[G])
    plan.saving = saving
    plan.dense = nb == 0 or bool((H_g == H).all() and (T_g == T).all()) or saving < floor
    plan.device_tables = None
    return plan
