#!/usr/bin/env python3
"""The reference's test driver (test.py: model_test + write_submission_file) on synthetic data, through this package: a small
processed test set is written the way the reference's ETL leaves it (head file + zstd/pickle subvolumes), scored with an
ensemble of two seeded models -- forwards, then ONE launch for softmax / mean / second softmax / rank -- and zipped.

    python examples/score_synthetic.py --impressions 200 --batch 80
    python examples/score_synthetic.py --compact      (no forward work on padded candidates: evaluation.predict_ranked_compact)
    python examples/score_synthetic.py --compact-history      (nor on padded history rows: predict_ranked_compact(history=True))
"""
import argparse
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from news_recommendation_model_amd import data_io, evaluation, synth, trainer  # noqa: E402
from news_recommendation_model_amd.config import Dims                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impressions", type=int, default=200)
    ap.add_argument("--batch", type=int, default=80, help="test.py:46's batch size")
    ap.add_argument("--history", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=12)
    ap.add_argument("--emb", type=int, default=64)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--compact", action="store_true", help="score ragged lists: live candidates + one representative padded candidate per impression")
    ap.add_argument("--compact-history", action="store_true",
                    help="--compact, and drop the trailing all-zero history rows as well (one representative padded history row per impression)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: the Modules have no CPU path")
    dims = Dims.for_emb(args.emb, category_label_num=50)
    N, T = args.impressions, args.candidates
    user_num = max(10, N // 4)
    out_dir = args.out_dir or tempfile.mkdtemp(prefix="nrm_score_")
    # a processed test set: impressions with 0 .. T/2 trailing padding candidates (all-zero rows, counted in empty_num)
    batch = synth.make_batch(dims, N, args.history, T, seed=0, user_num=user_num)
    rng = np.random.default_rng(1)
    batch["empty_num"] = rng.integers(0, T // 2 + 1, N).astype(np.int64)
    for b, z in enumerate(batch["empty_num"]):
        if z:
            batch["x_target"][b, T - z:] = 0
            batch["x_global"][b, T - z:] = 0
    batch["impression_id"] = 100000 + np.arange(N)
    head = data_io.write_processed_dataset(data_io.records_from_batch(batch), os.path.join(out_dir, "test_set"),
                                           subvolume_item_num=max(1, N // 3))
    models = [trainer.build_model(dims, user_num, synth.make_state_dict(dims, seed=s, user_num=user_num)) for s in (1, 5)]
    # the one-line replacement of test.py's model_test + write_submission_file:
    zip_path = evaluation.score_dataset(models, head, out_dir, batch_size=args.batch, compact=args.compact, compact_history=args.compact_history)
    with zipfile.ZipFile(zip_path) as z:
        lines = z.read("predictions.txt").decode("utf-8").splitlines()
    assert len(lines) == N
    print(f"{zip_path}: {len(lines)} impressions; first lines of predictions.txt:")
    for line in lines[:5]:
        print("   ", line)


if __name__ == "__main__":
    main()
