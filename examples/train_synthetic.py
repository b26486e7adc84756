#!/usr/bin/env python3
"""The reference's training driver (train.py:52-100) on synthetic EBNeRD-shaped data, through this package's drop-in
Modules: model = UserModel(max_user_id) re-dimensioned as BASELINE's configs do, FlatAdam (= Adam(lr, wd=1e-5) as one
launch), host float64 batches staged one ahead, per-impression AUC on the device, a checkpoint without `delta` per epoch.

    python examples/train_synthetic.py --workload C1-demo --batches 20 --epochs 2
    python examples/train_synthetic.py --workload ref-default --compact-history --history-lengths uniform      
    python examples/train_synthetic.py --workload ref-default --compact-candidates --candidate-counts percentile    (section 5f)
    python examples/train_synthetic.py --workload ref-default --from-tables --compact-history --compact-candidates    (section 5g)
    python examples/train_synthetic.py --workload ref-default --from-tables --graph --batches 100     (section 5g: one graph replay per step)
    python examples/train_synthetic.py --workload ref-default --from-tables --graph-grouped --compact-history --batches 100     (section 5i)
    python examples/train_synthetic.py --workload ref-default --from-tables --graph --validate     (section 5h: validation after every epoch)
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from news_recommendation_model_amd import data_io, evaluation, synth, tables, trainer  # noqa: E402
from news_recommendation_model_amd.config import Dims, WORKLOADS               # noqa: E402
sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from compact_util import pad_batch, percentile_counts                          # noqa: E402  (the count distribution the tests use)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C1-demo", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--batches", type=int, default=20, help="batches per epoch (distinct seeds, re-used every epoch)")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt-dir", default=None)
    ap.add_argument("--compact-history", action="store_true", help="do not compute the padded history rows (train_step(compact_history=True))")
    ap.add_argument("--history-lengths", default="full", choices=["full", "uniform", "tenth"],
                    help="cut the synthetic histories the way the ETL pads them: rows past a user's own are all-zero (uniform in [1, H] / all H/10)")
    ap.add_argument("--compact-candidates", action="store_true",
                    help="do not compute the padded candidates (train_step(compact_candidates=True)); reads every batch's empty_num")
    ap.add_argument("--candidate-counts", default="full", choices=["full", "percentile"],
                    help="pad the synthetic candidate lists the way the ETL does: all-zero rows past a list's own candidates, label 0 (percentile: "
                         "list lengths drawn from the percentiles the reference records, 70 %% of the lists at most 12 candidates)")
    ap.add_argument("--from-tables", action="store_true",
                    help="keep the data set on the device as index-based tables (raw synthetic records through tables.ImpressionTables) and write "
                         "every batch there with the assemble kernel (trainer.train_epochs_tables) instead of uploading processed records")
    ap.add_argument("--graph", action="store_true",
                    help="with --from-tables: after three eager steps every full batch is ONE replay of a captured step that assembles its own "
                         "batch at a device-side cursor (trainer.GraphedTableEpoch); the host reads the device once per epoch.  With --ckpt-dir "
                         "the per-step losses of every epoch are written as the reference writes them (train.py:93-94)")
    ap.add_argument("--graph-grouped", action="store_true",
                    help="with --from-tables and --compact-history and / or --compact-candidates: the captured epoch on compacted batches "
                         "(trainer.GroupedTableEpoch, DESIGN.md section 5i) -- one group plan per epoch, every batch sorted by length on the host")
    ap.add_argument("--validate", action="store_true",
                    help="with --from-tables: a second set of synthetic records is kept on the device as validation tables and scored after "
                         "every epoch in batches of 80 (train.py:107-110), through one captured pass where --graph is given "
                         "(evaluation.GraphedTableScoring); the epoch line is then the reference's")
    args = ap.parse_args()
    if args.graph_grouped:
        if not (args.compact_history or args.compact_candidates):
            raise SystemExit("--graph-grouped captures the COMPACTED step: give --compact-history and / or --compact-candidates")
        args.graph = "grouped"
    if args.graph and not args.from_tables:
        raise SystemExit("--graph / --graph-grouped capture the table-fed epoch: use them with --from-tables")
    if args.validate and not args.from_tables:
        raise SystemExit("--validate scores validation TABLES: use it with --from-tables")
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: the Modules have no CPU path")
    wl = WORKLOADS[args.workload]
    B = args.batch or wl["B"]
    dims = Dims.for_emb(wl["emb"])
    if args.from_tables:
        return main_from_tables(args, wl, B, dims)
    user_num = 10 * B
    torch.manual_seed(args.seed)                                           # train.py:42-43
    model = trainer.build_model(dims, user_num, synth.make_state_dict(dims, seed=args.seed + 1, user_num=user_num))
    opt = trainer.FlatAdam(model, lr=args.lr)                              # train.py:48
    ckpt_dir = args.ckpt_dir or tempfile.mkdtemp(prefix="nrm_ckpt_")
    # the data takes the reference's route: records in zstd+pickle subvolumes behind a head file (process_data.py:252-291),
    # read back with load_processed_dataset (:92-145) and batched as DataLoader(shuffle=True) does (train.py:40)
    records = []
    rng = np.random.default_rng(args.seed)
    for i in range(args.batches):
        batch = synth.make_batch(dims, B, wl["H"], wl["T"], seed=1000 + i, user_num=user_num)
        if args.history_lengths != "full":
            lengths = rng.integers(1, wl["H"] + 1, B) if args.history_lengths == "uniform" else np.full(B, max(wl["H"] // 10, 1))
            for b in range(B):
                batch["x_history"][b, int(lengths[b]):] = 0.0
        if args.candidate_counts == "percentile":
            # (at least two live candidates: the validation below depads a list before its AUC, and one candidate has none)
            pad_batch(batch, np.maximum(percentile_counts(rng, B, wl["T"], one_long=False), 2))
        records += data_io.records_from_batch(batch)
    head = data_io.write_processed_dataset(records, os.path.join(ckpt_dir, "synthetic_train_processed"), subvolume_item_num=4 * B)
    records, max_user_id = data_io.load_processed_dataset(head)
    epoch_no = [0]

    def loader():
        epoch_no[0] += 1
        return (b for b in data_io.iter_batches(records, B, shuffle=True, seed=args.seed + epoch_no[0]) if len(b["user_id"]) == B)
    hosts = list(data_io.iter_batches(records, B, shuffle=False))
    hist = trainer.train_epochs(model, opt, loader, args.epochs,
                                ckpt_path=os.path.join(ckpt_dir, "ckpt_synthetic_epoch_{epoch}.pth"), compact_history=args.compact_history,
                                compact_candidates=args.compact_candidates)
    for rec in hist:
        print("[epoch]:{epoch} [lr]:{lr:.3e} loss_avg={loss_avg:.4f} auc_avg={auc_avg:.4f} impressions={impressions}".format(**rec))
    # the checkpoint round-trips into a fresh model (test.py:159-160) and validates (verify.py:19-43)
    fresh = trainer.build_model(dims, user_num)
    evaluation.load_checkpoint(fresh, os.path.join(ckpt_dir, f"ckpt_synthetic_epoch_{args.epochs - 1}.pth"))
    auc, hit = evaluation.validate([fresh], (trainer.batch_to_device(h, "cuda") for h in hosts[:4]))
    # eval mode = BatchNorm running statistics (momentum 0.1): on this synthetic data (N(0,1) text/image vectors, un-normalised
    # history pooling) activations grow quickly while the model memorises, so after long runs the running statistics lag
    # the batch statistics and the eval-mode AUC can fall back to chance although the train-mode AUC keeps rising -- the
    # reference model behaves the same way (oracle/user_model_oracle.py reproduces it on the CPU)
    print(f"validation (eval mode) on 4 training batches: auc={auc:.4f} top1={hit:.4f}  checkpoints in {ckpt_dir}")


def main_from_tables(args, wl, B, dims):
    """The same driver with the data resident on the device: raw records -> tables (once) -> one assemble launch per step."""
    rng = np.random.default_rng(args.seed)
    n = args.batches * B
    n_val = max(n // 5, 80) if args.validate else 0                         # the validation set: further impressions of the same users
    n_users = max(n // 4, 8)
    recs = synth.make_records(dims, 4096, n_users, n + n_val, seed=args.seed, history_lens=rng.integers(0, wl["H"] + 20, n_users),
                              list_lens=np.clip(rng.geometric(1.0 / (0.7 * wl["T"]), n + n_val), 2, 3 * wl["T"]))
    part = lambda lo, hi: {k: v[lo:hi] for k, v in recs[2].items()}      # noqa: E731
    host = tables.ImpressionTables.from_records(recs[0], recs[1], part(0, n), dims, history_max=wl["H"])
    dev = host.to("cuda")
    validation = tables.ImpressionTables.from_records(recs[0], recs[1], part(n, n + n_val), dims, history_max=wl["H"]).to("cuda") if n_val else None
    user_num = host.max_user_id + 1
    torch.manual_seed(args.seed)
    model = trainer.build_model(dims, user_num, synth.make_state_dict(dims, seed=args.seed + 1, user_num=user_num))
    opt = trainer.FlatAdam(model, lr=args.lr)
    ckpt_dir = args.ckpt_dir or tempfile.mkdtemp(prefix="nrm_ckpt_")
    os.makedirs(ckpt_dir, exist_ok=True)
    print(f"{host.n_impressions} impressions, {host.nbytes / 1e6:.1f} MB of tables on the device; a step uploads {8 * B} bytes of indices "
          f"instead of {B * (wl['H'] * dims.history_cols + wl['T'] * (dims.target_cols + 4)) * 8 / 1e6:.1f} MB of float64 rows")
    hist = trainer.train_epochs_tables(model, opt, dev, args.epochs, B, wl["H"], wl["T"], seed=args.seed, drop_last=True,
                                       ckpt_path=os.path.join(ckpt_dir, "ckpt_synthetic_epoch_{epoch}.pth"),
                                       compact_history=args.compact_history, compact_candidates=args.compact_candidates, graph=args.graph,
                                       validation=validation)
    for rec in hist:
        if args.validate:                                                   # train.py:110
            print("[epoch]:{epoch} [avg_loss]:{loss_avg:.3e} [auc_score_t]:{auc_avg:.4f} [TPR_v]:{val_top1:.4f} [auc_score_v]:{val_auc:.4f}"
                  .format(**rec))
        print("[epoch]:{epoch} [lr]:{lr:.3e} loss_avg={loss_avg:.4f} auc_avg={auc_avg:.4f} impressions={impressions}".format(**rec)
              + (" top1_avg={top1_avg:.4f} steps={n}".format(n=len(rec["step_loss"]), **rec) if args.graph else ""))
        if args.graph and args.ckpt_dir:                                    # train.py:93-94: the epoch's per-step losses, one per line
            with open(os.path.join(ckpt_dir, f"epoch_{rec['epoch']}.txt"), "w") as f:
                f.writelines("{:.8f}\n".format(x) for x in rec["step_loss"])
    fresh = trainer.build_model(dims, user_num)
    evaluation.load_checkpoint(fresh, os.path.join(ckpt_dir, f"ckpt_synthetic_epoch_{args.epochs - 1}.pth"))
    batches = (b for i, b in enumerate(tables.TableLoader(dev, B, wl["H"], wl["T"], shuffle=False, drop_last=True)) if i < 4)
    auc, hit = evaluation.validate([fresh], batches)
    print(f"validation (eval mode) on 4 assembled batches: auc={auc:.4f} top1={hit:.4f}  checkpoints in {ckpt_dir}")


if __name__ == "__main__":
    main()
