"""Shared by the tests of the embedding front end's forward (frontend.hip: frontend_fwd_kernel, C ABI nrm_frontend_fwd): a numpy
float64 statement of the label row and the text/image row written from the header comment of nrm_frontend_fwd, the rule each kind
of column is held to, the case lists, and the mutants the CPU test must tell from the oracle.

The reference reads what the kernel reads: the tables are float32 values promoted to float64, an id is ``trunc`` of the stored
value (C's float -> int conversion, ``.long()`` in the reference model), a sentiment scalar and every copied column is the stored
value rounded to float32 (exact for fp32 rows).  An id outside its table is clamped to the nearest row and raises the flag.

Column rules (U = 2^-24, S = the sum of the absolute values of the terms the reference added for that element):
  type, behaviour, text/image     bitwise float32(x) / the table entry: a copy, no arithmetic
  padding [width, ldlab), [P, ldti)   bitwise +0.0
  category    |got - ref| <= (n_sub + 2) U S   n_sub - 1 additions of the slot sum (the first adds to 0, exact), the rounding of
                                               1 / n_sub, the product with it and the addition of the category's own entry
  time        |got - ref| <= 3 U S             three additions
  sentiment   |got - ref| <= 6 U S             three products and three additions; ReLU is 1-Lipschitz, so the bound on the
                                               pre-activation holds for the output, and an element whose float64 pre-activation
                                               lies within the bound of 0 may come out as 0 or as anything up to the bound
Fused multiply-adds only remove roundings from these counts.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
MAXSUB = 16                                     # FE_MAXSUB of frontend.hip
ROWS = (1, 7, 8, 9, 17, 2049)                   # FWD_ROWS = 8 rows per workgroup: partial, full, full + 1, several, many
MUTANTS = ("border", "mean")                    # the category block one column short / the slot mean over n_sub - 1

Spec = namedtuple("Spec", "e P n_sub behaviour n_cat n_type n_time")
Case = namedtuple("Case", "spec rows f64 ldlab_extra ldti_extra xcols_extra seed")

TABLE_NAMES = ("cat", "sen_w", "sen_b", "type", "year", "month", "day", "hour")


def spec(e, P=4, n_sub=5, behaviour=1, n_cat=11, n_type=5, n_time=(7, 13, 6, 4)):
    return Spec(tuple(e), P, n_sub, int(bool(behaviour)), n_cat, n_type, tuple(n_time))


def pad4(n):
    return (n + 3) // 4 * 4


def width(s):
    return sum(s.e) + (2 if s.behaviour else 0)


def need_cols(s):
    return 4 + s.P + 1 + s.n_sub + 3 + 1 + (2 if s.behaviour else 0)


def id_cols(s):
    """(column, limit) of every id of a packed row: year, month, day, hour, category, the sub-category slots, type."""
    c_cat = 4 + s.P
    return ([(k, s.n_time[k]) for k in range(4)] + [(c_cat + k, s.n_cat) for k in range(1 + s.n_sub)]
            + [(c_cat + 1 + s.n_sub + 3, s.n_type)])


def make_tables(s, seed):
    """The eight float32 tables.  The sentiment bias stays 0.05 away from 0, so a row of zero scalars is not a near-zero ReLU."""
    rng = np.random.default_rng(seed)
    e0, e1, e2, e3 = s.e
    shapes = [(s.n_cat, e0), (e1, 3), (e1,), (s.n_type, e2)] + [(n, e3) for n in s.n_time]
    tabs = [rng.standard_normal(sh).astype(np.float32) for sh in shapes]
    tabs[2] = (np.sign(tabs[2]) * (np.abs(tabs[2]) + 0.05)).astype(np.float32)
    return dict(zip(TABLE_NAMES, tabs))


def make_rows(s, rows, f64, seed, xcols_extra=0):
    """Packed rows [rows, need + xcols_extra] with every id in range and NaN in the unused trailing columns.  fp64 rows carry
    doubles that float32 does not hold in the copied columns and the sentiment scalars, so the kernel's conversion is seen."""
    rng = np.random.default_rng(seed)
    need = need_cols(s)
    x = rng.standard_normal((rows, need + xcols_extra))
    if not f64:
        x = x.astype(np.float32)
    for c, lim in id_cols(s):
        x[:, c] = rng.integers(0, lim, rows)
    x[:, need:] = np.nan
    return x


def reference(s, tabs, x, mutant=None):
    """-> dict(lab [R, width] float64, S [R, width] float64, kind [width] of 'cat' | 'sen' | 'type' | 'time' | 'beh',
    ti [R, P] float32, pre [R, e1] float64 sentiment pre-activations, flag: an id was out of range)."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64) and 1 <= s.n_sub
    e0, e1, e2, e3 = s.e
    t = {k: np.asarray(v, dtype=np.float32).astype(np.float64) for k, v in tabs.items()}
    flag = False
    ids = []
    for c, lim in id_cols(s):
        i = np.trunc(x[:, c].astype(np.float64)).astype(np.int64)
        flag = flag or bool(((i < 0) | (i >= lim)).any())
        ids.append(np.clip(i, 0, lim - 1))
    year, month, day, hour, cat = ids[:5]
    sub, typ = np.stack(ids[5:5 + s.n_sub], axis=1), ids[5 + s.n_sub]              # [R, n_sub]
    n_mean = s.n_sub - 1 if mutant == "mean" else s.n_sub
    sub_rows = t["cat"][sub]                                                        # [R, n_sub, e0]
    cat_v = t["cat"][cat] + sub_rows.sum(axis=1) / n_mean
    cat_S = np.abs(t["cat"][cat]) + np.abs(sub_rows).sum(axis=1) / n_mean
    c_sen = 4 + s.P + 1 + s.n_sub
    sen = x[:, c_sen:c_sen + 3].astype(np.float32).astype(np.float64)               # [R, 3]
    terms = t["sen_w"][None, :, :] * sen[:, None, :]                                # [R, e1, 3]
    pre = t["sen_b"][None, :] + terms.sum(axis=2)
    sen_v = np.maximum(pre, 0.0)
    sen_S = np.abs(t["sen_b"])[None, :] + np.abs(terms).sum(axis=2)
    typ_v = t["type"][typ]
    time_terms = [t["year"][year], t["month"][month], t["day"][day], t["hour"][hour]]
    time_v = time_terms[0] + time_terms[1] + time_terms[2] + time_terms[3]
    time_S = sum(np.abs(a) for a in time_terms)
    blocks = [cat_v, sen_v, typ_v, time_v]
    mags = [cat_S, sen_S, np.abs(typ_v), time_S]
    kind = ["cat"] * e0 + ["sen"] * e1 + ["type"] * e2 + ["time"] * e3
    if s.behaviour:
        c_beh = c_sen + 3 + 1
        beh = x[:, c_beh:c_beh + 2].astype(np.float32).astype(np.float64)
        blocks.append(beh)
        mags.append(np.abs(beh))
        kind += ["beh"] * 2
    lab, S = np.concatenate(blocks, axis=1), np.concatenate(mags, axis=1)
    if mutant == "border":                      # `c < e0 - 1`: the last category column already holds the first sentiment unit
        lab[:, e0 - 1], S[:, e0 - 1] = sen_v[:, 0], sen_S[:, 0]
    return dict(lab=lab, S=S, kind=np.array(kind), ti=x[:, 4:4 + s.P].astype(np.float32), pre=pre, flag=flag)


def roundings(s):
    """kind -> k of the module docstring (0: a copy)."""
    return {"cat": s.n_sub + 2, "sen": 6, "type": 0, "time": 3, "beh": 0}


def bound(s, ref):
    k = roundings(s)
    return np.array([k[n] for n in ref["kind"]], dtype=np.float64)[None, :] * U * ref["S"]


def near_zero_share(s, ref):
    """share of the sentiment elements whose float64 pre-activation lies within the bound of 0"""
    sen = ref["kind"] == "sen"
    return float((np.abs(ref["pre"]) <= bound(s, ref)[:, sen]).mean())


# e settings: width % 4 = 0, 1, 2, 3 without the behaviour columns and 2, 3, 0, 1 with them
E_SETTINGS = ((5, 1, 1, 1), (6, 1, 1, 1), (4, 3, 2, 1), (3, 2, 3, 3))
P_VALUES = (1, 4, 65)
NSUB_VALUES = (1, 5, 16)


def sweep_cases(e, behaviour):
    """One case per row count for an e setting; P, n_sub, the input type, the two leading dimensions and the row width cycle with
    periods 3, 3, 2, 2, 2 and 2 against each other and against the six row counts and eight settings, so every value of each
    meets every row-count class."""
    n = E_SETTINGS.index(tuple(e)) * 2 + int(bool(behaviour))
    out = []
    for i, rows in enumerate(ROWS):
        j = i + n
        s = spec(e, P=P_VALUES[j % 3], n_sub=NSUB_VALUES[(j // 3 + i) % 3], behaviour=behaviour)
        out.append(Case(s, rows, bool(j % 2), 8 * ((j // 2) % 2), 4 * ((j // 4 + i) % 2), 3 * ((j // 3) % 2), 1000 + 16 * n + i))
    return out


def all_sweep_cases():
    return [c for e in E_SETTINGS for b in (0, 1) for c in sweep_cases(e, b)]
