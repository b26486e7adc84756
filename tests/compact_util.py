"""Shared by the compact-scoring tests: padded batches as the reference's ETL writes a processed test set (every candidate list
padded with all-zero rows to one length, ``empty_num`` = the padding per row), list lengths drawn from the percentiles the
reference records (configs/model_config.py:32: 70 % of the lists have at most 12 candidates, 80 % at most 15, 90 % at most 20)."""
import numpy as np


def percentile_counts(rng, B, T, one_long=True):
    """Live candidates per row, in [1, T]: 70 % uniform in [1, 12], 10 % in [13, 15], 10 % in [16, 20], 10 % in [21, T]
    (clipped to T); ``one_long`` makes row 0 a full-length list (the row that keeps the common trim at 0)."""
    u = rng.random(B)
    lo = np.where(u < 0.7, 1, np.where(u < 0.8, 13, np.where(u < 0.9, 16, 21)))
    hi = np.where(u < 0.7, 12, np.where(u < 0.8, 15, np.where(u < 0.9, 20, max(T, 21))))
    n = np.minimum(rng.integers(lo, hi + 1), T)
    if one_long and B:
        n[0] = T
    return np.maximum(n, 1).astype(np.int64)


def pad_batch(batch, counts):
    """In place: rows ``counts[b]:`` of x_target / x_global zeroed, empty_num = T - counts, the one-hot label moved into the live part."""
    B, T = batch["x_target"].shape[:2]
    counts = np.asarray(counts).astype(np.int64)
    for b in range(B):
        n = int(counts[b])
        batch["x_target"][b, n:] = 0.0
        batch["x_global"][b, n:] = 0.0
        batch["label"][b] = 0.0
        if n > 0:
            batch["label"][b, b % n] = 1.0
    batch["empty_num"] = (T - counts).astype(np.int64)
    return batch


def brute_force_plan(empty, T):
    """The plan's tables by explicit loops (what compact.build_plan is checked against)."""
    empty = [min(max(int(e), 0), T) for e in empty]
    B = len(empty)
    trim = min(empty) if B else 0
    Tp = T - trim
    cand_off, cand_imp, src, pad_mult, live = [0], [], [], [], []
    for b in range(B):
        e = empty[b] - trim
        n = Tp - e
        for t in range(n):
            cand_imp.append(b)
            src.append(b * T + t)
        if e > 0:
            cand_imp.append(b)
            src.append(b * T + n)                     # the first padded column stands for all e of them
        cand_off.append(len(cand_imp))
        pad_mult.append(e)
        live.append(n)
    return dict(trim=trim, Tp=Tp, N=len(cand_imp), cand_off=cand_off, cand_imp=cand_imp, src=src, pad_mult=pad_mult, live=live)
