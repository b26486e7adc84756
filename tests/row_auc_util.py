"""Shared by the tests of the per-impression AUC / top-1 kernel (pool_loss.hip: row_auc_kernel, C ABI nrm_row_auc): the cases and the
reference, which is oracle.user_model_oracle.row_auc (pinned to sklearn's roc_auc_score) on the candidates that count, -1 where
sklearn raises, and numpy.argmax for the top-1 hit.  ``MUTANTS`` names the copy of the AUC that the CPU test must tell from the
oracle on these very cases.

A lane of the kernel strides the candidates by 64 and a workgroup holds 4 impressions: T = 63, 64, 65 sit around one candidate per
lane, 130 and 257 leave a ragged last trip, 1024 gives every lane 16; B = 1, 3, 4, 5, 9 sit around one workgroup.
"""
from collections import namedtuple

import numpy as np

from oracle import user_model_oracle as orc

U = 2.0 ** -24
T_VALUES = (1, 2, 63, 64, 65, 130, 257, 1024)
B_VALUES = (1, 3, 4, 5, 9)
MUTANTS = ("ge",)                                # `>=` for `>`: a tie counts 1 + 1/2 instead of 1/2

Case = namedtuple("Case", "name score label length")     # score, label [B, T] float32; length [B] int32 or None


def mutant_row_auc(label_row, score_row, mutant):
    assert mutant == "ge"
    y = np.asarray(label_row, dtype=np.float64) > 0.5
    s = np.asarray(score_row, dtype=np.float64)
    pos, neg = s[y], s[~y]
    return float((pos[:, None] >= neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / float(len(pos) * len(neg))


def reference(case, mutant=None):
    """-> (auc [B] float64, -1 where the counting candidates hold one class or none; top1 [B] int; n_pos * n_neg [B])"""
    B, T = case.score.shape
    auc, top1, pairs = np.full(B, -1.0), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = T if case.length is None else min(int(case.length[b]), T)
        if n <= 0:
            continue
        s, y = case.score[b, :n], case.label[b, :n]
        top1[b] = int(np.argmax(s) == np.argmax(y))
        n_pos = int((y > 0.5).sum())
        pairs[b] = n_pos * (n - n_pos)
        if pairs[b]:
            auc[b] = orc.row_auc(y, s) if mutant is None else mutant_row_auc(y, s, mutant)
    return auc, top1, pairs


def _rows(rng, B, T, n_pos_of_row):
    """scores on four levels (ties everywhere), negatives labelled 0, 0.25 or exactly 0.5, positives 0.75 or 1"""
    score = (rng.integers(0, 4, (B, T)) / 4.0).astype(np.float32)
    label = rng.choice(np.array([0.0, 0.25, 0.5], dtype=np.float32), (B, T))
    for b in range(B):
        k = int(np.clip(n_pos_of_row(b), 0, T))
        at = rng.choice(T, k, replace=False)
        label[b, at] = rng.choice(np.array([0.75, 1.0], dtype=np.float32), k)
    return score, label


def grid_cases():
    """Every T with a B: full rows with 1, 3, T - 1, no and only positives, then the same rows under per-row lengths 0, 1, T, T + 5
    (clamped) and a negative one, the padding behind a length filled with a larger score and a positive label."""
    out = []
    for i, T in enumerate(T_VALUES):
        B = B_VALUES[i % len(B_VALUES)]
        rng = np.random.default_rng(50 + i)
        counts = (1, 3, T - 1, 0, T)
        score, label = _rows(rng, B, T, lambda b: counts[(b + i) % 5])
        out.append(Case(f"T{T}-B{B}-full", score, label, None))
        B2 = 9
        score, label = _rows(rng, B2, T, lambda b: (1, 3, T - 1)[b % 3])
        length = np.array([(0, 1, T, T + 5, -3, max(T // 2, 1), max(T - 1, 1), T, 1)[b] for b in range(B2)], dtype=np.int32)
        for b in range(B2):
            n = int(np.clip(length[b], 0, T))
            score[b, n:], label[b, n:] = 9.0, 1.0
        out.append(Case(f"T{T}-B{B2}-lengths", score, label, length))
    return out


def tie_cases():
    """Equal maximal scores (then labels) at 5 and 70 -- lanes 5 and 6 -- and at 5 and 69 -- both lane 5: the first index wins, so
    the hit depends on which of the two the other array points at."""
    out = []
    for other in (70, 69):
        for tied in ("score", "label"):
            rows_s, rows_y = [], []
            for pointed in (5, other):                                   # the untied array's maximum: hit for 5, miss for the other
                rng = np.random.default_rng(other + pointed)
                s = (rng.integers(0, 4, 130) / 4.0).astype(np.float32)
                y = rng.choice(np.array([0.0, 0.25, 0.5, 0.75], dtype=np.float32), 130)
                a, b = (s, y) if tied == "score" else (y, s)
                a[5] = a[other] = 2.0
                b[pointed] = 3.0
                rows_s.append(s)
                rows_y.append(y)
            out.append(Case(f"tie-{tied}-5-{other}", np.stack(rows_s), np.stack(rows_y), None))
    return out


def all_cases():
    return grid_cases() + tie_cases()
