"""Helpers of the table-fed evaluation tests: the seeded data set both the host plan test and the GPU runner test
use, and ``tally_reference``, the numpy float64 restatement of ``nrm_eval_tally``."""
import numpy as np

from news_recommendation_model_amd import synth, tables
from news_recommendation_model_amd.config import Dims

B, H, N = 8, 17, 5 * 8 + 3                     # five full batches and a tail of 3
# The lists hold 2 .. 9 entries (a list of one would be a row with a single class, on which validation raises) and the target is always in
# its list, so with keep_target_slot=False and T = the longest list every row has both classes and empty_num = T - its length.
# RECORD_SEED is chosen so that the full batches take more than one width, one of them T itself (test_table_scoring_cpu.py asserts it).
RECORD_SEED = 6
MAX_LIST = 9
GUARD = 0x5A5A5A5A5A5A5A5A


def scoring_records(seed=RECORD_SEED, n=N, labelled=True):
    dims = Dims()
    lens = np.random.default_rng(1000 + seed).integers(2, MAX_LIST + 1, n)
    return dims, synth.make_records(dims, 40, 12, n, seed=seed, max_history=25, list_lens=lens, labelled=labelled)


def scoring_tables(seed=RECORD_SEED, n=N, labelled=True):
    """-> (dims, host tables, T = the longest list)"""
    dims, recs = scoring_records(seed, n, labelled)
    t = tables.ImpressionTables.from_records(*recs, dims, history_max=30, dtype=np.float32)
    assert t.n_impressions == n
    return dims, t, int(np.diff(t.imp_off).max())


def tally_reference(calls, T, n_order, cap, cursor=0, state=None):
    """``nrm_eval_tally`` restated: ``calls`` is a list of steps, each a dict with rank [B, Tp] int32, live [B] int32, impression_id [B] int64
    and (or None) auc [B] float32, top1 [B] int32, metrics [B, 3] float32.  -> dict(cursor, sums [5] float64, counts [4] int64, rec_rank
    [cap, T], rec_live [cap], rec_id [cap]) after all steps; ``state``: the dict of an earlier call to go on from (record buffers start as
    the GUARD pattern so that an unwritten row is told from a zero one).  The sums are plain float64 numpy sums: the device's differ by
    association only."""
    if state is None:
        state = {"cursor": int(cursor), "sums": np.zeros(5, dtype=np.float64), "counts": np.zeros(4, dtype=np.int64),
                 "rec_rank": np.full((cap, T), GUARD & 0x7FFFFFFF, dtype=np.int32), "rec_live": np.full(cap, GUARD & 0x7FFFFFFF, dtype=np.int32),
                 "rec_id": np.full(cap, GUARD, dtype=np.int64)}
    for step in calls:
        rank = step["rank"]
        n, tp = rank.shape
        p = state["cursor"] + np.arange(n, dtype=np.int64)
        inside = (p >= 0) & (p < n_order)
        if step.get("auc") is not None:
            auc, top1 = step["auc"], step["top1"]
            ok = inside & (auc >= 0)
            state["sums"][0] += np.sum(auc[ok].astype(np.float64))
            state["sums"][1] += np.float64(int(top1[inside].sum()))
            state["counts"][0] += int((inside & ~(auc >= 0)).sum())
        if step.get("metrics") is not None:
            m = step["metrics"]
            ok = inside & (m[:, 0] >= 0)
            for k in range(3):
                state["sums"][2 + k] += np.sum(m[ok, k].astype(np.float64))
            state["counts"][1] += int((inside & ~(m[:, 0] >= 0)).sum())
        state["counts"][2] += 1
        state["counts"][3] += int(inside.sum())
        if cap:
            rows = p[inside] % cap
            state["rec_rank"][rows, :tp] = rank[inside]
            state["rec_rank"][rows, tp:] = 0
            state["rec_live"][rows] = step["live"][inside]
            state["rec_id"][rows] = step["impression_id"][inside]
        state["cursor"] += n
    return state


def plan_reference(empty_num, n, b, T):
    """(impressions, T - min over the batch of empty_num) per batch, restated"""
    e = np.asarray(empty_num)
    return [(int(e[lo:lo + b].shape[0]), int(T - np.min(e[lo:lo + b]))) for lo in range(0, n, b)]
