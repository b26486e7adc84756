"""Reference pins of the ETL arithmetic and loop (data only): writes tests/golden/etl_norm.npz and tests/golden/etl_tiny.npz.

    python scripts/make_etl_golden.py --reference /path/to/News_Recommendation_Model

Run where the reference project is checked out; it is imported at run time and nothing of it is written here -- the fixtures hold inputs
and the numbers its functions returned.

(a) etl_norm.npz: tool/normalization.sec_norm on time differences (microseconds, passed as us / 1e6 seconds -- what pandas' total_seconds()
    gives) at every bucket border +- {1 us, 1 s}, negative differences, differences beyond 3000 years, random ones, and the inputs found
    on which integer arithmetic on the microseconds gives other buckets; value_norm on values that include NaN.
(b) etl_tiny.npz: the reference's process_dataset (batch_type 0 and 2) driven on a synthetic raw data set of a dozen impressions: parquet
    inputs written with pyarrow to a temporary folder, load_text_img_data replaced by the given vectors, history_max_num / inview_max_num
    lowered in its config dict, a stand-in ``zstandard`` module whose compressor is the identity (the module is not needed to build rows),
    and the history pass run in this process (process_history_data itself, without the worker pool around it).  Stored: the raw records
    (tables.pack_records) and the processed rows.
"""
import argparse
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from news_recommendation_model_amd import synth, tables          # noqa: E402
from news_recommendation_model_amd.config import Dims          # noqa: E402

STANDARDS = [(60 * 60 * 24 * 365, 3000), (60 * 60 * 24 * 30, 12), (60 * 60 * 24, 30), (60 * 60, 23)]


def integer_buckets(us):
    """the integer restatement that is NOT the reference's function (kept to find the inputs on which the two differ)"""
    rem, out = max(0, int(us)), []
    for standard, cap in STANDARDS:
        k = min(rem // (standard * 1_000_000), cap)
        rem -= k * standard * 1_000_000
        out.append(k)
    return out


def norm_fixture(normalization):
    rng = np.random.default_rng(7)
    us = set()
    Y, M, D, Hh = (s * 1_000_000 for s, _ in STANDARDS)
    for y in (0, 1, 2, 5, 99, 100, 2999, 3000, 3001):
        for m in (0, 1, 11, 12, 13):
            for d in (0, 1, 4, 29, 30, 31):
                for h in (0, 1, 22, 23, 24):
                    border = y * Y + m * M + d * D + h * Hh
                    for eps in (0, 1, -1, 1_000_000, -1_000_000):
                        us.add(border + eps)
    us.update(int(x) for x in (-1, -10**6, -10**15, 3001 * Y + 12 * M, 5000 * Y, 2**62, 10**18))
    us.update(int(x) for x in rng.integers(0, 6 * Y, 2000))
    # inputs on which integer arithmetic differs: search near multiples of the standards
    found = []
    for _ in range(400000):
        k = int(rng.integers(1, 3000)) * Y + int(rng.integers(0, 13)) * M + int(rng.integers(0, 31)) * D + int(rng.integers(0, 25)) * Hh
        x = k + int(rng.integers(-3, 4))
        if list(normalization.sec_norm(x / 1e6)) != integer_buckets(x):
            found.append(x)
            if len(found) >= 64:
                break
    us.update(found)
    us = np.array(sorted(us), dtype=np.int64)
    buckets = np.array([normalization.sec_norm(int(x) / 1e6) for x in us], dtype=np.int64)
    differs = np.array([list(b) != integer_buckets(x) for x, b in zip(us.tolist(), buckets.tolist())])
    vals = np.concatenate([rng.random(200) * 1e7, [np.nan, 0.0, -3.5, 1e12, np.nan]])
    stds = np.concatenate([rng.choice([60.0, 100.0, 1e7, 1e9], 200), [60.0, 100.0, 1e7, 1e9, 1e9]])
    vn = np.array([normalization.value_norm(float(v), float(s)) for v, s in zip(vals, stds)], dtype=np.float64)
    return {"delta_us": us, "buckets": buckets, "integer_differs": differs, "value": vals, "standard": stds, "value_norm": vn}


def tiny_fixture(ref_root, H=6, T=4):
    import pandas as pd
    zs = types.ModuleType("zstandard")

    class _Identity:
        def __init__(self, *a, **k):
            pass

        def compress(self, b):
            return b

        def decompress(self, b):
            return b
    zs.ZstdCompressor = zs.ZstdDecompressor = _Identity
    sys.modules.setdefault("zstandard", zs)
    from tool import process_data                                   # the reference's module
    from configs.model_config import config as ref_model
    from configs.run_config import config as ref_run
    dims = Dims()
    lists = [0, 1, 3, 4, 5, 12, 2, 7, 4, 3, 9, 6]
    recs = synth.make_records(dims, n_articles=14, n_users=5, n_impressions=len(lists), seed=11, history_lens=[0, 1, 5, 6, 11], list_lens=lists,
                              absent_target_frac=0.25, multi_click_frac=0.1, max_history=11)
    articles, histories, behaviors = recs
    ts = lambda us: pd.to_datetime(np.asarray(us, dtype=np.int64), unit="us")      # noqa: E731
    tmp = tempfile.mkdtemp()
    folder = os.path.join(tmp, "tiny")
    os.makedirs(os.path.join(folder, "train"))
    pd.DataFrame({"article_id": articles["article_id"], "article_type": articles["article_type"], "category": articles["category"],
                  "subcategory": [list(map(int, x)) for x in articles["subcategory"]], "sentiment_score": articles["sentiment_score"],
                  "sentiment_label": articles["sentiment_label"], "published_time": ts(articles["published_time_us"]),
                  "total_inviews": articles["total_inviews"], "total_pageviews": articles["total_pageviews"],
                  "total_read_time": articles["total_read_time"]}).to_parquet(os.path.join(folder, "articles.parquet"))
    pd.DataFrame({"user_id": histories["user_id"], "article_id_fixed": [list(map(int, x)) for x in histories["article_id"]],
                  "impression_time_fixed": [list(ts(x)) for x in histories["impression_time_us"]],
                  "read_time_fixed": [list(map(float, x)) for x in histories["read_time"]],
                  "scroll_percentage_fixed": [list(map(float, x)) for x in histories["scroll_percentage"]]}
                 ).to_parquet(os.path.join(folder, "train", "history.parquet"))
    pd.DataFrame({"impression_id": behaviors["impression_id"], "user_id": behaviors["user_id"],
                  "impression_time": ts(behaviors["impression_time_us"]),
                  "article_ids_inview": [list(map(int, x)) for x in behaviors["article_ids_inview"]],
                  "article_ids_clicked": [list(map(int, x)) for x in behaviors["article_ids_clicked"]]}
                 ).to_parquet(os.path.join(folder, "train", "behaviors.parquet"))
    vec = {int(a): np.asarray(v, dtype=np.float64) for a, v in zip(articles["article_id"], articles["text_img"])}
    process_data.load_text_img_data = lambda *a, **k: vec
    process_data.process_history_data_in_thread = lambda data, thread_num=None: process_data.process_history_data(data, {})
    ref_model["history_max_num"], ref_model["inview_max_num"] = H, T
    ref_run["processed_data_path"] = tmp + "/"
    out = dict(tables.pack_records(*recs))
    out["H"], out["T"] = np.int64(H), np.int64(T)
    for bt in (0, 2):
        head = process_data.process_dataset(folder, type_i=0, batch_type=bt)
        with open(head + ".subvolume0", "rb") as f:
            rows = pickle.loads(f.read())
        with open(head, "rb") as f:
            meta = pickle.loads(f.read())
        k = f"b{bt}."
        out[k + "impression_id"] = np.array([r[0] for r in rows], dtype=np.int64)
        out[k + "user_id"] = np.array([r[1] for r in rows], dtype=np.int64)
        out[k + "x_history"] = np.stack([r[2] for r in rows])
        out[k + "x_target"] = np.stack([r[3] for r in rows])
        out[k + "x_global"] = np.stack([r[4] for r in rows])
        out[k + "label"] = np.stack([r[5] for r in rows])
        out[k + "label_id"] = np.stack([r[6] for r in rows]).astype(np.int64)
        out[k + "empty_num"] = np.array([r[7] for r in rows], dtype=np.int64)
        out[k + "max_user_id"] = np.int64(meta[2])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--skip-tiny", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    os.chdir(tempfile.mkdtemp())
    from tool import normalization
    gold = os.path.join(ROOT, "tests", "golden")
    a = norm_fixture(normalization)
    np.savez_compressed(os.path.join(gold, "etl_norm.npz"), **a)
    print("etl_norm.npz:", a["delta_us"].shape[0], "time differences,", int(a["integer_differs"].sum()), "on which integer arithmetic differs")
    if not args.skip_tiny:
        b = tiny_fixture(args.reference)
        np.savez_compressed(os.path.join(gold, "etl_tiny.npz"), **b)
        print("etl_tiny.npz:", b["b0.x_history"].shape, b["b0.x_target"].shape, b["b2.x_target"].shape)
