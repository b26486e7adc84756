"""Helpers of the table tests: an independent, literal per-impression statement of the ETL loop (python floats and lists, no closed form),
the seeded record sets, and the slot-rule cases."""
import os

import numpy as np

from news_recommendation_model_amd import synth, tables
from news_recommendation_model_amd.config import Dims

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLOT_KINDS = ("first", "at", "later", "absent", "dup")


def literal_buckets(delta_us):
    """sec_norm in python floats and ints, one value at a time"""
    sec = max(0, int(delta_us) / 1e6)
    out = []
    for standard, cap in ((60 * 60 * 24 * 365, 3000), (60 * 60 * 24 * 30, 12), (60 * 60 * 24, 30), (60 * 60, 23)):
        out.append(min(int(sec / standard), cap))
        sec -= standard * out[-1]
    return out


def literal_slots(inview, target, T, keep_target_slot):
    """The candidate loop as the ETL walks it: entries are taken in order; while the last slot is next and no target has been placed, only
    the target is taken.  -> list of in-view positions per slot (None = empty)."""
    slots, placed = [], False
    for pos, a in enumerate(inview):
        if keep_target_slot and len(slots) == T - 1 and not placed:
            if target is not None and a == target:
                slots.append(pos)
                placed = True
        else:
            slots.append(pos)
            placed = placed or (target is not None and a == target)
        if len(slots) >= T:
            break
    return slots + [None] * (T - len(slots))


def literal_assemble(t, sel, H, T, keep_target_slot=True):
    """assemble_host's dict, one impression, one row, one column group at a time"""
    Sw = t.static_cols
    out = {"x_history": [], "x_target": [], "x_global": [], "label": [], "label_id": [], "empty_num": [], "user_id": [], "impression_id": [],
           "history_len": []}
    for n in sel:
        n = int(n)
        u, when = int(t.imp_user[n]), int(t.imp_time_us[n])
        rows = np.zeros((H, 4 + Sw + 2))
        events = list(range(int(t.user_off[u]), int(t.user_off[u + 1])))[:H]
        for j, e in enumerate(events):
            rows[j] = literal_buckets(when - int(t.ev_time_us[e])) + [float(v) for v in t.art_static[t.ev_art[e], :Sw]] + [float(t.ev_read[e]), float(t.ev_scroll[e])]
        inview = [int(a) for a in t.imp_inview[int(t.imp_off[n]):int(t.imp_off[n + 1])]]
        target = int(t.imp_target[n]) if t.imp_target[n] >= 0 else None
        xt, xg, lab, lid = np.zeros((T, 4 + Sw)), np.zeros((T, 3)), np.zeros(T), -np.ones(T, dtype=np.int64)
        for s, pos in enumerate(literal_slots(inview, target, T, keep_target_slot)):
            if pos is None:
                continue
            a = inview[pos]
            xt[s] = literal_buckets(when - int(t.art_pub_us[a])) + [float(v) for v in t.art_static[a, :Sw]]
            xg[s] = [float(v) for v in t.art_global[a]]
            lab[s] = 1.0 if a == target else 0.0
            lid[s] = int(t.art_id[a])
        for k, v in (("x_history", rows), ("x_target", xt), ("x_global", xg), ("label", lab), ("label_id", lid), ("empty_num", int((lid == -1).sum())),
                     ("user_id", int(t.user_id[u])), ("impression_id", int(t.imp_id[n])), ("history_len", len(events))):
            out[k].append(v)
    return {k: np.asarray(v) for k, v in out.items()}


def seeded_tables(dims=None, dtype=np.float64, seed=3, n_articles=60, n_users=24, n_impressions=48, history_max=30, max_list=24, **kw):
    dims = Dims() if dims is None else dims
    recs = synth.make_records(dims, n_articles, n_users, n_impressions, seed=seed, absent_target_frac=0.2, multi_click_frac=0.1, max_history=40,
                              max_list=max_list, **kw)
    return tables.ImpressionTables.from_records(*recs, dims, history_max=history_max, dtype=dtype)


def history_tables(H, dims=None, dtype=np.float64, seed=5):
    """users with 0, 1, H-1, H and H+5 events (cut at H+5 by the builder), one impression each and two more on the longest"""
    lens = [0, 1, max(H - 1, 0), H, H + 5]
    dims = Dims() if dims is None else dims
    recs = synth.make_records(dims, 30, len(lens), 7, seed=seed, history_lens=lens, max_list=6)
    recs[2]["user_id"] = recs[1]["user_id"][[0, 1, 2, 3, 4, 4, 0]]
    return tables.ImpressionTables.from_records(*recs, dims, history_max=H + 5, dtype=dtype)


def slot_tables(T, dims=None, dtype=np.float64, labelled=True, seed=9):
    """One impression per (list length, where the target is): lengths 0, 1, T-1, T, T+1, 3T; target among the first T-1 ('first'), at
    position T-1 ('at'), behind it ('later'), not in the list ('absent'), twice in the list ('dup': at the front where there is one and
    again at the end); ``labelled=False``: the same lists with no target.  -> (tables, [(length, kind)])"""
    dims = Dims() if dims is None else dims
    lengths = sorted({0, 1, max(T - 1, 0), T, T + 1, 3 * T})
    A = 3 * T + 8
    articles, histories, _ = synth.make_records(dims, A, 4, 1, seed=seed, max_history=12)
    ids = articles["article_id"]
    rng = np.random.default_rng(seed)
    beh = {"impression_id": [], "user_id": [], "impression_time_us": [], "article_ids_inview": [], "article_ids_clicked": []}
    cases = []
    for L in lengths:
        for kind in SLOT_KINDS:
            perm = ids[rng.permutation(A)]
            inview, outside = perm[:L].copy(), perm[L]
            if kind == "first":
                if L < 1 or T < 2:
                    continue
                click = inview[min(L, T - 1) - 1]
            elif kind == "at":
                if L < T:
                    continue
                click = inview[T - 1]
            elif kind == "later":
                if L <= T:
                    continue
                click = inview[L - 1]
            elif kind == "absent":
                click = outside
            else:
                if L < 2:
                    continue
                click = inview[0]
                inview[L - 1] = click
            cases.append((L, kind))
            beh["impression_id"].append(1000 + len(cases))
            beh["user_id"].append(histories["user_id"][len(cases) % 4])
            beh["impression_time_us"].append(1_684_000_000_000_000 + 3_600_000_000 * len(cases))
            beh["article_ids_inview"].append(inview)
            beh["article_ids_clicked"].append(np.array([click]))
    if not labelled:
        del beh["article_ids_clicked"]
    return tables.ImpressionTables.from_records(articles, histories, beh, dims, history_max=12, dtype=dtype), cases


def border_tables(dims=None, dtype=np.float64, count=256):
    """Impressions whose one event and one candidate lie exactly a fixture time difference back: the bucket borders of etl_norm.npz, the
    inputs on which integer arithmetic differs first.  -> (tables, delta_us [n])"""
    dims = Dims() if dims is None else dims
    g = np.load(os.path.join(GOLDEN, "etl_norm.npz"))
    ok = np.abs(g["delta_us"]) < 2 ** 61                                # (time stamps stay inside int64)
    d, differs = g["delta_us"][ok], g["integer_differs"][ok]
    pick = np.concatenate([d[differs][:count // 2], d[::max(1, d.shape[0] // (count // 2))]])[:count]
    n = pick.shape[0]
    articles, histories, _ = synth.make_records(dims, n, n, 1, seed=2, history_lens=np.ones(n, dtype=np.int64))
    now = 1_684_000_000_000_000
    when = np.where(pick > now, pick, now)                           # differences beyond the epoch: the impression moves forward, not the event back
    articles["published_time_us"] = when - pick
    histories["impression_time_us"] = [np.array([w - p]) for w, p in zip(when.tolist(), pick.tolist())]
    beh = {"impression_id": np.arange(n), "user_id": histories["user_id"], "impression_time_us": when,
           "article_ids_inview": [articles["article_id"][i:i + 1] for i in range(n)],
           "article_ids_clicked": [articles["article_id"][i:i + 1] for i in range(n)]}
    return tables.ImpressionTables.from_records(articles, histories, beh, dims, dtype=dtype), pick
