"""Training batches assembled on the device from resident tables.

The reference's ETL (tool/process_data.py:190-252) writes one processed record per impression -- x_history [200, 80], x_target [15, 78],
x_global [15, 3] in float64, about 138 KB -- by copying an article's row into every impression that mentions it.  What a batch is made
of is far smaller: an article table, at most ``history_max`` events per user, and per impression a user, a time, an in-view list and a
target.  ``ImpressionTables`` holds exactly that, index-based and structure-of-arrays, so that it can live in HBM; ``assemble_batch``
(one HIP kernel, ``csrc/assemble.hip``) writes a step's tensors from a list of impression indices, and ``assemble_host`` is the numpy
statement of the same rows -- the reference's loop body for ``batch_type`` 0 and 2 -- that the kernel is tested against bit for bit.

Reading parquet and the PCA of the text and image vectors stay outside: ``from_records`` takes plain numpy / Python records.
"""
from __future__ import annotations

from dataclasses import dataclass, fields

import numpy as np

from .config import Dims, model_config

# reference configs/model_config.py:24-27
READ_TIME_NORM = 60.0
SCROLL_NORM = 100.0
TOTAL_VIEWS_NORM = 1e7
TOTAL_READ_TIME_NORM = 1e9
# reference tool/normalization.py:32 -- (seconds, cap) of the year, month, day and hour buckets
TIME_STANDARDS = ((60 * 60 * 24 * 365, 3000), (60 * 60 * 24 * 30, 12), (60 * 60 * 24, 30), (60 * 60, 23))


def value_norm(value, standard):
    """reference tool/normalization.py value_norm, vectorised: value / standard, 0 where value is NaN."""
    v = np.asarray(value, dtype=np.float64)
    return np.where(np.isnan(v), 0.0, v / standard)


def time_buckets(delta_us):
    """reference tool/normalization.py sec_norm on ``delta_us / 1e6`` seconds, vectorised -> int64 [..., 4] (year, month, day, hour).
    The arithmetic is the reference's float64 one: ``k = min(int(sec / standard), cap); sec -= standard * k``.  Integer arithmetic on the
    microseconds is NOT the same function: the float subtraction leaves a residue that the next division sees at bucket borders."""
    sec = np.maximum(0.0, np.asarray(delta_us, dtype=np.int64).astype(np.float64) / 1e6)
    out = np.empty(sec.shape + (4,), dtype=np.int64)
    for i, (standard, cap) in enumerate(TIME_STANDARDS):
        k = np.minimum(np.floor(sec / standard), float(cap))
        sec = sec - float(standard) * k
        out[..., i] = k.astype(np.int64)
    return out


# the order in which the tables travel to torch.ops.nrm.assemble_batch
TABLE_FIELDS = ("art_static", "art_global", "art_pub_us", "art_id", "user_off", "ev_art", "ev_time_us", "ev_read", "ev_scroll", "user_id",
                "imp_user", "imp_time_us", "imp_off", "imp_inview", "imp_target", "imp_id")


def _seq(x, what):
    if x is None:
        raise ValueError(f"{what}: missing")
    return list(x)


@dataclass
class ImpressionTables:
    """The data set as index-based tables (numpy on the host, torch tensors after ``.to(device)``).

    art_static [A, S]   text+image vector P | category | sub-categories | sentiment slots | type, zero-padded to S (a multiple of 4)
    art_pub_us [A] int64 (microseconds since the epoch), art_global [A, 3] normalised inviews, pageviews, read time, art_id [A] int64
    user_off [U + 1] int64, ev_art [E] int32, ev_time_us [E] int64, ev_read [E], ev_scroll [E], user_id [U] int64: the events of user u
        are user_off[u] .. user_off[u + 1] - 1, most recent first, at most ``history_max``
    imp_user [N] int32, imp_time_us [N] int64, imp_off [N + 1] int64, imp_inview [sum L] int32, imp_target [N] int32 (-1 = none),
        imp_id [N] int64
    """
    art_static: object
    art_global: object
    art_pub_us: object
    art_id: object
    user_off: object
    ev_art: object
    ev_time_us: object
    ev_read: object
    ev_scroll: object
    user_id: object
    imp_user: object
    imp_time_us: object
    imp_off: object
    imp_inview: object
    imp_target: object
    imp_id: object
    static_cols: int
    max_user_id: int
    dims: Dims

    # ------------------------------------------------------------------------------------------------ construction
    @staticmethod
    def from_records(articles, histories, behaviors, dims: Dims | None = None, history_max: int = 200, dtype=np.float32,
                     type_dict=None, sentiment_dict=None):
        """articles: dict of per-article columns -- article_id, text_img [A, P], category, subcategory (lists), sentiment_score,
        sentiment_label, article_type, published_time_us, total_inviews, total_pageviews, total_read_time.
        histories: dict of per-user columns -- user_id, article_id, impression_time_us, read_time, scroll_percentage (lists per user,
        oldest first, as the data set stores them).
        behaviors: dict of per-impression columns -- impression_id, user_id, impression_time_us, article_ids_inview and, for labelled
        data, article_ids_clicked.

        What reference process_articles_data / process_history_data / process_behaviors_data do to these inputs: the three counters
        divided by their standard with NaN -> 0; sub-categories padded with 0 or cut to ``n_subcat``; the sentiment score in its label's
        slot; the type looked up in the type dictionary; histories reversed to most recent first and cut at ``history_max``, read time
        / 60 and scroll / 100 with NaN -> 0; with clicks present only the impressions with exactly one click are kept, without clicks
        every impression with target = none.  Every id is resolved to an index here, once; an id that resolves to nothing raises
        ValueError naming the record."""
        dims = Dims.from_config() if dims is None else dims
        if dtype not in (np.float32, np.float64):
            raise ValueError(f"dtype {dtype}: the floating tables are float32 or float64")
        type_dict = model_config["article_type_dict"] if type_dict is None else type_dict
        sentiment_dict = model_config["sentiment_label_dict"] if sentiment_dict is None else sentiment_dict
        P, ns, nsent = dims.pca_vector, dims.n_subcat, dims.n_sentiment
        # ---- articles
        aid = np.asarray(_seq(articles.get("article_id"), "articles.article_id"), dtype=np.int64)
        A = aid.shape[0]
        ti = np.asarray(articles.get("text_img"), dtype=np.float64)
        if ti.shape != (A, P):
            raise ValueError(f"articles.text_img: shape {ti.shape}, expected ({A}, {P})")
        if len(set(aid.tolist())) != A:
            raise ValueError("articles.article_id: duplicate ids")
        if A and aid.min() < 0:
            raise ValueError("articles.article_id: negative id (-1 marks an empty slot in label_id)")
        Sw = P + 1 + ns + nsent + 1
        S = (Sw + 3) // 4 * 4
        static = np.zeros((A, S), dtype=np.float64)
        static[:, :P] = ti
        static[:, P] = np.asarray(_seq(articles.get("category"), "articles.category"), dtype=np.float64)
        sub = _seq(articles.get("subcategory"), "articles.subcategory")
        score = np.asarray(_seq(articles.get("sentiment_score"), "articles.sentiment_score"), dtype=np.float64)
        slabel = _seq(articles.get("sentiment_label"), "articles.sentiment_label")
        atype = _seq(articles.get("article_type"), "articles.article_type")
        for i in range(A):
            row = list(sub[i])[:ns]
            static[i, P + 1:P + 1 + len(row)] = row
            if slabel[i] not in sentiment_dict:
                raise ValueError(f"article {int(aid[i])}: unknown sentiment label {slabel[i]!r}")
            k = sentiment_dict[slabel[i]]
            if not 0 <= k < nsent:
                raise ValueError(f"article {int(aid[i])}: sentiment slot {k} outside [0, {nsent})")
            static[i, P + 1 + ns + k] = score[i]
            if atype[i] not in type_dict:
                raise ValueError(f"article {int(aid[i])}: unknown article type {atype[i]!r}")
            static[i, P + 1 + ns + nsent] = type_dict[atype[i]]
        glob = np.stack([value_norm(_seq(articles.get("total_inviews"), "articles.total_inviews"), TOTAL_VIEWS_NORM),
                         value_norm(_seq(articles.get("total_pageviews"), "articles.total_pageviews"), TOTAL_VIEWS_NORM),
                         value_norm(_seq(articles.get("total_read_time"), "articles.total_read_time"), TOTAL_READ_TIME_NORM)], axis=1) \
            if A else np.zeros((0, 3))
        pub = np.asarray(_seq(articles.get("published_time_us"), "articles.published_time_us"), dtype=np.int64)
        if pub.shape != (A,):
            raise ValueError(f"articles.published_time_us: {pub.shape[0]} entries for {A} articles")
        index_of = {int(a): i for i, a in enumerate(aid.tolist())}
        # ---- histories: reversed to most recent first, cut at history_max
        uid = np.asarray(_seq(histories.get("user_id"), "histories.user_id"), dtype=np.int64)
        U = uid.shape[0]
        if len(set(uid.tolist())) != U:
            raise ValueError("histories.user_id: duplicate ids")
        h_art, h_time = _seq(histories.get("article_id"), "histories.article_id"), _seq(histories.get("impression_time_us"), "histories.impression_time_us")
        h_read, h_scroll = _seq(histories.get("read_time"), "histories.read_time"), _seq(histories.get("scroll_percentage"), "histories.scroll_percentage")
        user_off = np.zeros(U + 1, dtype=np.int64)
        ev_art, ev_time, ev_read, ev_scroll = [], [], [], []
        for u in range(U):
            n = len(h_art[u])
            if not (len(h_time[u]) == len(h_read[u]) == len(h_scroll[u]) == n):
                raise ValueError(f"history of user {int(uid[u])}: the four lists differ in length")
            keep = slice(None, None, -1)
            arts = list(h_art[u])[keep][:history_max]
            try:
                ev_art.append(np.asarray([index_of[int(a)] for a in arts], dtype=np.int32))
            except KeyError as e:
                raise ValueError(f"history of user {int(uid[u])}: article {e.args[0]} is not in the article table") from None
            ev_time.append(np.asarray(list(h_time[u])[keep][:history_max], dtype=np.int64))
            ev_read.append(value_norm(np.asarray(list(h_read[u])[keep][:history_max], dtype=np.float64), READ_TIME_NORM))
            ev_scroll.append(value_norm(np.asarray(list(h_scroll[u])[keep][:history_max], dtype=np.float64), SCROLL_NORM))
            user_off[u + 1] = user_off[u] + len(arts)
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)      # noqa: E731
        user_index = {int(x): i for i, x in enumerate(uid.tolist())}
        # ---- behaviors: with clicks, exactly one click; without, target = none
        b_id = _seq(behaviors.get("impression_id"), "behaviors.impression_id")
        b_user, b_time = _seq(behaviors.get("user_id"), "behaviors.user_id"), _seq(behaviors.get("impression_time_us"), "behaviors.impression_time_us")
        b_inview = _seq(behaviors.get("article_ids_inview"), "behaviors.article_ids_inview")
        b_click = behaviors.get("article_ids_clicked")
        imp_user, imp_time, imp_id, imp_target, lists = [], [], [], [], []
        max_user_id = 0
        for i in range(len(b_id)):
            target = -1
            if b_click is not None:
                if len(b_click[i]) != 1:
                    continue
                c = int(b_click[i][0])
                if c not in index_of:
                    raise ValueError(f"impression {int(b_id[i])}: clicked article {c} is not in the article table")
                target = index_of[c]
            if int(b_user[i]) not in user_index:
                raise ValueError(f"impression {int(b_id[i])}: user {int(b_user[i])} has no history record")
            try:
                lists.append(np.asarray([index_of[int(a)] for a in b_inview[i]], dtype=np.int32))
            except KeyError as e:
                raise ValueError(f"impression {int(b_id[i])}: in-view article {e.args[0]} is not in the article table") from None
            imp_user.append(user_index[int(b_user[i])])
            imp_time.append(int(b_time[i]))
            imp_id.append(int(b_id[i]))
            imp_target.append(target)
            max_user_id = max(max_user_id, int(b_user[i]))
        imp_off = np.zeros(len(lists) + 1, dtype=np.int64)
        if lists:
            imp_off[1:] = np.cumsum([len(x) for x in lists])
        return ImpressionTables(
            art_static=static.astype(dtype), art_global=np.ascontiguousarray(glob, dtype=dtype), art_pub_us=pub, art_id=aid,
            user_off=user_off, ev_art=cat(ev_art, np.int32), ev_time_us=cat(ev_time, np.int64), ev_read=cat(ev_read, dtype),
            ev_scroll=cat(ev_scroll, dtype), user_id=uid,
            imp_user=np.asarray(imp_user, dtype=np.int32), imp_time_us=np.asarray(imp_time, dtype=np.int64), imp_off=imp_off,
            imp_inview=cat(lists, np.int32), imp_target=np.asarray(imp_target, dtype=np.int32), imp_id=np.asarray(imp_id, dtype=np.int64),
            static_cols=Sw, max_user_id=max_user_id, dims=dims).validate()

    def validate(self):
        """Every index against the array it points into (host tables only), once: ValueError naming the first offending record."""
        if self.is_device:
            return self
        A, U, E = self.art_static.shape[0], self.user_id.shape[0], self.ev_art.shape[0]

        def monotone(off, n, what):
            if off.shape[0] < 1 or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 0):
                raise ValueError(f"{what}: not a prefix sum ending at {n}")
        monotone(self.user_off, E, "user_off")
        monotone(self.imp_off, self.imp_inview.shape[0], "imp_off")
        for name, arr, hi, lo in (("ev_art", self.ev_art, A, 0), ("imp_inview", self.imp_inview, A, 0), ("imp_target", self.imp_target, A, -1),
                                  ("imp_user", self.imp_user, U, 0)):
            bad = np.nonzero((arr < lo) | (arr >= hi))[0]
            if bad.size:
                raise ValueError(f"{name}[{int(bad[0])}] = {int(arr[bad[0]])} is outside [{lo}, {hi})")
        if self.art_static.shape[1] != (self.static_cols + 3) // 4 * 4 or self.art_static.shape[1] % 4:
            raise ValueError(f"art_static: {self.art_static.shape[1]} columns for static width {self.static_cols}")
        for name in ("art_pub_us", "art_id"):
            if getattr(self, name).shape != (A,):
                raise ValueError(f"{name}: shape {getattr(self, name).shape} for {A} articles")
        for name in ("ev_time_us", "ev_read", "ev_scroll"):
            if getattr(self, name).shape != (E,):
                raise ValueError(f"{name}: shape {getattr(self, name).shape} for {E} events")
        return self

    # ------------------------------------------------------------------------------------------------ properties
    @property
    def is_device(self):
        return not isinstance(self.art_static, np.ndarray)

    @property
    def n_impressions(self):
        return int(self.imp_user.shape[0])

    @property
    def history_cols(self):
        return 4 + self.static_cols + 2

    @property
    def target_cols(self):
        return 4 + self.static_cols

    @property
    def nbytes(self):
        """bytes of all tables (what is resident on the device after ``.to``)"""
        total = 0
        for name in TABLE_FIELDS:
            a = getattr(self, name)
            total += int(a.nbytes) if isinstance(a, np.ndarray) else int(a.numel() * a.element_size())
        return total

    def to(self, device):
        """The tables as torch tensors on ``device`` (one upload; the host object is unchanged).  The host copies of the offsets and
        targets that ``history_len`` / ``empty_num`` read stay with the result."""
        import torch
        if self.is_device:
            raise ValueError("ImpressionTables.to: already device tables; keep the host object and call .to(device) on it")
        kw = {f.name: getattr(self, f.name) for f in fields(self)}
        for name in TABLE_FIELDS:
            kw[name] = torch.from_numpy(np.ascontiguousarray(getattr(self, name))).to(device)
        out = ImpressionTables(**kw)
        out._host = self
        return out

    @property
    def host(self):
        return getattr(self, "_host", self)

    # ------------------------------------------------------------------------------------------------ what the producer knows
    def history_len(self, sel, H):
        """min(events of the impression's user, H) for the impressions ``sel`` -- host numpy int32, touches no device."""
        t = self.host
        u = t.imp_user[np.asarray(sel, dtype=np.int64)]
        return np.minimum(t.user_off[u + 1] - t.user_off[u], H).astype(np.int32)

    def empty_num_all(self, T, keep_target_slot=True):
        """``empty_num`` of EVERY impression at ``T`` slots -- host numpy int64 [N], the closed form of the slot rule."""
        t = self.host
        N = t.n_impressions
        L = np.diff(t.imp_off)
        front = np.minimum(L, T - 1)
        if not keep_target_slot:
            return (T - front - (L > T - 1)).astype(np.int64)
        imp = np.repeat(np.arange(N), L)
        pos = np.arange(t.imp_inview.shape[0]) - np.repeat(t.imp_off[:-1], L)
        hit = (t.imp_inview == np.repeat(t.imp_target, L)) & (np.repeat(t.imp_target, L) >= 0)
        early = np.bincount(imp[hit & (pos < T - 1)], minlength=N) > 0
        late = np.bincount(imp[hit & (pos >= T - 1)], minlength=N) > 0
        last = np.where(early, L > T - 1, late)
        return (T - front - last).astype(np.int64)


_RAGGED = {"articles": ("subcategory",), "histories": ("article_id", "impression_time_us", "read_time", "scroll_percentage"),
           "behaviors": ("article_ids_inview", "article_ids_clicked")}


def pack_records(articles, histories, behaviors):
    """The raw records as a flat dict of plain numpy arrays (a ragged column becomes ``name`` + ``name.off``): what an ``.npz`` fixture holds."""
    out = {}
    for group, rec in (("articles", articles), ("histories", histories), ("behaviors", behaviors)):
        for key, col in rec.items():
            if key in _RAGGED[group]:
                parts = [np.asarray(x) for x in col]
                out[f"{group}.{key}.off"] = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
                out[f"{group}.{key}"] = np.concatenate(parts) if parts and sum(len(x) for x in parts) else np.zeros(0, dtype=np.int64)
            else:
                out[f"{group}.{key}"] = np.asarray(col)
    return out


def unpack_records(flat):
    """``pack_records`` undone -> (articles, histories, behaviors)."""
    recs = {"articles": {}, "histories": {}, "behaviors": {}}
    for name in flat:
        if name.split(".")[0] not in recs or name.endswith(".off"):
            continue
        group, key = name.split(".")[:2]
        if key in _RAGGED[group]:
            off, data = flat[name + ".off"], flat[name]
            recs[group][key] = [data[off[i]:off[i + 1]] for i in range(off.shape[0] - 1)]
        else:
            recs[group][key] = flat[name]
    return recs["articles"], recs["histories"], recs["behaviors"]


def slot_positions(inview, target, T, keep_target_slot=True):
    """The in-view position every one of the T candidate slots takes, -1 for an empty slot (closed form of the reference's loop,
    tool/process_data.py:224-250): slots 0 .. T-2 are the first T-1 entries; slot T-1 is entry T-1 if one of the first T-1 is the target,
    else the first entry at position >= T-1 that is the target, else empty.  ``keep_target_slot=False``: the first T entries."""
    inview = np.asarray(inview)
    L = inview.shape[0]
    pos = np.full(T, -1, dtype=np.int64)
    n = min(L, T - 1)
    pos[:n] = np.arange(n)
    last = T - 1
    if keep_target_slot:
        if target is None or target < 0:
            last = -1
        elif not np.any(inview[:T - 1] == target):
            later = np.nonzero(inview[T - 1:] == target)[0]
            last = T - 1 + int(later[0]) if later.size else -1
    if 0 <= last < L:
        pos[T - 1] = last
    return pos


def assemble_host(tables: ImpressionTables, sel, H, T, keep_target_slot=True):
    """The processed records of the impressions ``sel`` as the reference's ``process_dataset`` builds them (loop body of
    tool/process_data.py:190-252) for ``batch_type`` 0 (``keep_target_slot=True``, T = ``inview_max_num``) and 2 (``False``, T = the
    longest list): the dict ``assemble_batch`` returns, as numpy with float64 rows."""
    t = tables.host
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    if sel.size and (sel.min() < 0 or sel.max() >= t.n_impressions):
        raise IndexError(f"sel: impression index outside [0, {t.n_impressions})")
    B, Sw = sel.shape[0], t.static_cols
    hc, tc = 4 + Sw + 2, 4 + Sw
    xh = np.zeros((B, H, hc), dtype=np.float64)
    xt = np.zeros((B, T, tc), dtype=np.float64)
    xg = np.zeros((B, T, 3), dtype=np.float64)
    label = np.zeros((B, T), dtype=np.float64)
    label_id = np.full((B, T), -1, dtype=np.int64)
    hist_len = np.zeros(B, dtype=np.int32)
    for b, n in enumerate(sel.tolist()):
        u, when = int(t.imp_user[n]), int(t.imp_time_us[n])
        lo = int(t.user_off[u])
        k = min(int(t.user_off[u + 1]) - lo, H)
        hist_len[b] = k
        if k:
            ev = slice(lo, lo + k)
            xh[b, :k, :4] = time_buckets(when - t.ev_time_us[ev])
            xh[b, :k, 4:4 + Sw] = t.art_static[t.ev_art[ev], :Sw]
            xh[b, :k, 4 + Sw] = t.ev_read[ev]
            xh[b, :k, 5 + Sw] = t.ev_scroll[ev]
        inview = t.imp_inview[int(t.imp_off[n]):int(t.imp_off[n + 1])]
        target = int(t.imp_target[n])
        pos = slot_positions(inview, target, T, keep_target_slot)
        live = np.nonzero(pos >= 0)[0]
        if live.size:
            art = inview[pos[live]]
            xt[b, live, :4] = time_buckets(when - t.art_pub_us[art])
            xt[b, live, 4:] = t.art_static[art, :Sw]
            xg[b, live] = t.art_global[art]
            label[b, live] = (art == target) & (target >= 0)
            label_id[b, live] = t.art_id[art]
    return {"x_history": xh, "x_target": xt, "x_global": xg, "label": label, "label_id": label_id,
            "empty_num": (label_id == -1).sum(axis=1).astype(np.int64), "user_id": t.user_id[t.imp_user[sel]].astype(np.int64),
            "impression_id": t.imp_id[sel].astype(np.int64), "history_len": hist_len}


BATCH_KEYS = ("x_history", "x_target", "x_global", "label", "label_id", "empty_num", "user_id", "impression_id", "history_len")


def assemble_batch(tables: ImpressionTables, sel, H, T, keep_target_slot=True):
    """The same dict on the device: ONE launch of the assemble kernel on the current stream, from device-resident tables
    (``tables.to('cuda')``) and ``sel`` (an int64 device tensor of impression indices; repeats and any order are fine).  The three x
    tensors have the tables' floating type.  An index of ``sel`` outside the table is clamped and raises the device index flag
    (``ops.check_index_errors``).  ``sel`` is read by the launch, not by a replay: the form that can be captured is ``assemble_batch_at``."""
    from . import ops
    if not tables.is_device:
        raise RuntimeError("assemble_batch: the tables are host arrays; upload them once with tables.to('cuda') "
                           "(the host statement of the same rows is assemble_host)")
    out = ops.assemble_batch([getattr(tables, name) for name in TABLE_FIELDS], sel, int(H), int(T), bool(keep_target_slot), int(tables.static_cols))
    return dict(zip(BATCH_KEYS, out))


def assemble_batch_at(tables: ImpressionTables, order, cursor, B, H, T, keep_target_slot=True):
    """``assemble_batch`` for the ``B`` impressions ``order[cursor[0] : cursor[0] + B]``, with ``order`` (int64 [n]) AND ``cursor`` (one int64)
    on the device: the launch reads no host data, so it may sit inside a stream capture -- the returned tensors are then the graph's
    static batch, rewritten by every replay for wherever the cursor stands (``trainer.GraphedTableEpoch``).  A position outside ``order`` is
    clamped into it and raises the device index flag like an index outside the table."""
    from . import ops
    if not tables.is_device:
        raise RuntimeError("assemble_batch_at: the tables are host arrays; upload them once with tables.to('cuda') "
                           "(the host statement of the same rows is assemble_host)")
    out = ops.assemble_batch_at([getattr(tables, name) for name in TABLE_FIELDS], order, cursor, int(B), int(H), int(T), bool(keep_target_slot),
                                int(tables.static_cols))
    return dict(zip(BATCH_KEYS, out))


GROUP_KEYS = ("x_history_arena", "x_target_arena", "x_global_arena", "label_arena", "row_weight", "label", "label_id", "empty_num", "user_id",
              "impression_id", "history_len")


def assemble_groups_at(tables: ImpressionTables, order, cursor, B, H, T, plan, keep_target_slot=True):
    """``assemble_batch_at`` writing straight into the grouped arenas of ``plan`` (a ``compact.EpochGroupPlan``, or anything with its
    ``upload``, ``R`` and ``N``): the ``B`` impressions ``order[cursor[0] : cursor[0] + B]`` must arrive sorted the way
    the plan was cut (``plan.order``).  -> dict of ``GROUP_KEYS``: the history arena [R, hc], the candidate arenas [N, tc] / [N, 3] / label
    [N] / row weight [N] -- the bits ``ops.history_gather_groups`` / ``ops.candidate_gather_groups`` give on the dense batch, which is never
    written -- and the dense kernel's label [B, T], label_id, empty_num, user_id, impression_id and history_len.  An impression that does
    not fit its group raises the device flag ``ops.check_group_fit`` reads.  No host data is read: the launch may be captured."""
    from . import ops
    if not tables.is_device:
        raise RuntimeError("assemble_groups_at: the tables are host arrays; upload them once with tables.to('cuda') "
                           "(the host statement of the same rows is assemble_host)")
    tabs = plan.upload(order.device)
    out = ops.assemble_groups_at([getattr(tables, name) for name in TABLE_FIELDS], order, cursor, int(B), int(H), int(T), bool(keep_target_slot),
                                 int(tables.static_cols), tabs["bounds"], tabs["H_g"], tabs["hist_row_off"], tabs["T_g"], tabs["cand_row_off"],
                                 int(plan.R), int(plan.N))
    return dict(zip(GROUP_KEYS, out))


class TableLoader:
    """Batches of a data set that lives on the device as ``ImpressionTables``: the epoch's permutation is drawn on the host (numpy, seeded),
    ``sel`` -- a few KB -- is uploaded per batch, and the batch is written by ``assemble_batch`` on the current stream.  Yields the device
    dicts ``train_step``, ``evaluation.validate``, ``predict_ranked`` and the writers of ``score_dataset`` read, with the producer's own
    history lengths and ``empty_num`` attached on the host (``trainer.attach_known_lengths``): a compacted step plans from them without a
    measuring kernel, a copy or a synchronise.  ``order()`` is the impression order of the coming epoch (for a host path to follow)."""

    def __init__(self, tables: ImpressionTables, batch_size, H, T, shuffle=True, seed=0, keep_target_slot=True, device="cuda",
                 drop_last=False):
        self.host = tables.host
        self.tables = tables if tables.is_device else tables.to(device)
        self.batch_size, self.H, self.T = int(batch_size), int(H), int(T)
        self.shuffle, self.keep_target_slot, self.drop_last = shuffle, keep_target_slot, drop_last
        self.rng = np.random.default_rng(seed)
        self.empty_all = self.host.empty_num_all(self.T, keep_target_slot)
        self._next_order = None

    def __len__(self):
        n = self.host.n_impressions
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def order(self):
        if self._next_order is None:
            n = self.host.n_impressions
            self._next_order = self.rng.permutation(n) if self.shuffle else np.arange(n)
        return self._next_order

    def take_order(self):
        """The coming epoch's order, consumed: the next call draws the next permutation (what ``__iter__`` starts with)."""
        order, self._next_order = self.order(), None
        return order

    def __iter__(self):
        import torch
        from . import trainer
        order = self.take_order()
        dev = self.tables.art_static.device
        for i in range(len(self)):
            sel = np.ascontiguousarray(order[i * self.batch_size:(i + 1) * self.batch_size], dtype=np.int64)
            sel_dev = torch.from_numpy(sel).pin_memory().to(dev, non_blocking=True)
            batch = assemble_batch(self.tables, sel_dev, self.H, self.T, self.keep_target_slot)
            yield trainer.attach_known_lengths(batch, self.host.history_len(sel, self.H), self.empty_all[sel])
