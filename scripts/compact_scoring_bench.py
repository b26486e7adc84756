#!/usr/bin/env python3
"""Dense against compact scoring of padded candidate lists, on one GPU, in one process, the two arms
alternating; writes profiles/compact_scoring.json stamped with the kernel-source digest.

Arms: evaluation.predict_ranked (the parent's path: every (impression, column) cell the common trim leaves goes through the
forwards) against evaluation.predict_ranked_compact (live candidates + one representative padded candidate per impression), two
models.  Workloads: reference dimensions (emb 64, H = 200) and C3 dimensions (emb 400, H = 50), batches of 80 (the reference's
test batch) and 1 024, candidate lists padded to PAD_TO = 100 columns with live counts drawn from the percentiles of the reference's
configs/model_config.py:32 (70 % at most 12, 80 % at most 15, 90 % at most 20; one full-length row per batch keeps the common trim
at 0).  PAD_TO = 100 is an ASSUMPTION: the true maximum list length of the data set is not in this repository.  Plus one workload
without any padding, where predict_ranked_compact hands the batch to predict_ranked itself (must measure equal within the spread)
and where the forced compact forms (gather, table lookups on N = B T rows) are timed beside it.

Every arm is warmed up, then timed ROUNDS times over REPS calls with a device-event pair around work that ends in a synchronise;
the figure is the median of the rounds, the spread is (max - min) / median of the same arm's rounds.

    python scripts/compact_scoring_bench.py [--workloads NAME,...] [--out profiles/compact_scoring.json]
    python scripts/compact_scoring_bench.py --trace NAME --arm dense|compact      a few calls of one arm, for
        NRM_BRANCH_STREAMS=0 rocprofv3 --kernel-trace --stats -- python scripts/compact_scoring_bench.py --trace ...   (per-kernel times; a
        run of its own, with one attention stream: the dense arm otherwise overlaps its two attentions and each reports the sum)
    python scripts/compact_scoring_bench.py --kernel-stats NAME dense.csv compact.csv      fold two kernel_stats.csv into the JSON
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from compact_util import pad_batch, percentile_counts                                       # noqa: E402
from news_recommendation_model_amd import build, compact, evaluation, native, ops, synth, trainer   # noqa: E402
from news_recommendation_model_amd.config import Dims                                        # noqa: E402

PAD_TO = 100
ROUNDS = 5
TRACE_CALLS = 3
WORKLOADS = {
    # name: emb, H, B, T, padded, calls per round
    "ref_B80": dict(emb=64, H=200, B=80, T=PAD_TO, padded=True, reps=10),
    "ref_B1024": dict(emb=64, H=200, B=1024, T=PAD_TO, padded=True, reps=4),
    "c3_B80": dict(emb=400, H=50, B=80, T=PAD_TO, padded=True, reps=6),
    "c3_B1024": dict(emb=400, H=50, B=1024, T=PAD_TO, padded=True, reps=2),
    "c3_B1024_unpadded": dict(emb=400, H=50, B=1024, T=30, padded=False, reps=3),
}


def make(name):
    w = WORKLOADS[name]
    dims = Dims.for_emb(w["emb"])
    B, H, T = w["B"], w["H"], w["T"]
    batch = synth.make_batch(dims, B, H, T, seed=3, user_num=10 * B, dtype=np.float32)
    if w["padded"]:
        pad_batch(batch, percentile_counts(np.random.default_rng(B + w["emb"]), B, T, one_long=True))
    models = [trainer.build_model(dims, 10 * B, synth.make_state_dict(dims, seed=s, user_num=10 * B), device="cuda").eval() for s in (1, 2)]
    tb = {k: torch.from_numpy(batch[k]).cuda() for k in ("x_history", "x_target", "x_global")}
    tb["empty_num"] = torch.from_numpy(batch["empty_num"])                                   # host tensor, as a DataLoader hands it over
    plan = compact.build_plan(batch["empty_num"], T)
    return w, models, tb, plan


def rate(fn, B, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return B * reps / (e0.elapsed_time(e1) * 1e-3)


def summarise(dense, comp):
    md, mc = statistics.median(dense), statistics.median(comp)
    sd, sc = (max(dense) - min(dense)) / md, (max(comp) - min(comp)) / mc
    return {"dense_impressions_per_s": md, "compact_impressions_per_s": mc, "dense_rounds": dense, "compact_rounds": comp,
            "spread_dense": sd, "spread_compact": sc, "compact_over_dense": mc / md,
            "equal_within_spread": bool(abs(mc - md) <= max(sd, sc) * md)}


def measure(name):
    w, models, tb, plan = make(name)
    arms = {"dense": lambda: evaluation.predict_ranked(models, tb), "compact": lambda: evaluation.predict_ranked_compact(models, tb)}
    if not w["padded"]:
        arms["forced"] = lambda: evaluation.predict_ranked_compact(models, tb, force_compact=True)
    for fn in arms.values():
        for _ in range(3):
            fn()
    rounds = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            rounds[k].append(rate(fn, w["B"], w["reps"]))
    ops.check_index_errors("cuda")
    ops.check_pad_errors("cuda")
    out = summarise(rounds["dense"], rounds["compact"])
    out.update(B=w["B"], H=w["H"], T_kept=plan.Tp, emb=w["emb"], N=plan.N, cells=plan.B * plan.Tp, N_over_cells=plan.N / (plan.B * plan.Tp),
               calls_per_round=w["reps"], rounds=ROUNDS)
    if "forced" in rounds:
        f = summarise(rounds["dense"], rounds["forced"])
        out["forced_compact_forms"] = {k.replace("compact", "forced"): v for k, v in f.items() if k.startswith(("compact", "spread_compact"))}
    return out


def fold_kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    fwd = [r for r in rows if "pwattn_fwd" in r["Name"] and "pack" not in r["Name"]]
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]
    return {"attention_forward_ms_per_call": sum(float(r["TotalDurationNs"]) for r in fwd) / 1e6 / TRACE_CALLS,
            "all_kernels_ms_per_call": sum(float(r["TotalDurationNs"]) for r in rows) / 1e6 / TRACE_CALLS,
            "top": [{"name": r["Name"][:100], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6} for r in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_scoring.json"))
    ap.add_argument("--trace")
    ap.add_argument("--arm", default="compact", choices=["dense", "compact"])
    ap.add_argument("--kernel-stats", nargs=3, metavar=("WORKLOAD", "DENSE_CSV", "COMPACT_CSV"))
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    digest = build.sources_digest()
    if doc.get("kernel_sources_sha256") != digest:
        doc = {k: doc[k] for k in ("error_budget",) if k in doc}                             # timings of other sources are not mixed in
    if args.kernel_stats:
        name, d_csv, c_csv = args.kernel_stats
        d, c = fold_kernel_stats(d_csv), fold_kernel_stats(c_csv)
        doc.setdefault("kernel_trace", {})[name] = {
            "dense": d, "compact": c, "calls_traced": TRACE_CALLS,
            "attention_forward_compact_over_dense": c["attention_forward_ms_per_call"] / d["attention_forward_ms_per_call"]}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("needs an MI355X: a timing taken elsewhere says nothing")
        native.load()
        if args.trace:
            w, models, tb, plan = make(args.trace)
            fn = evaluation.predict_ranked if args.arm == "dense" else evaluation.predict_ranked_compact
            for _ in range(TRACE_CALLS):
                fn(models, tb)
            torch.cuda.synchronize()
            return
        doc.update({"kernel_sources_sha256": digest, "device": torch.cuda.get_device_name(0), "pad_to_columns_ASSUMED": PAD_TO,
                    "what": "impressions/s of predict_ranked (dense) against predict_ranked_compact, two models, eager; lists padded to "
                            "pad_to_columns_ASSUMED with live counts from the percentiles of the reference's model_config.py:32"})
        for name in args.workloads.split(","):
            doc.setdefault("workloads", {})[name] = r = measure(name)
            print(f"{name}: dense {r['dense_impressions_per_s']:.4g}/s  compact {r['compact_impressions_per_s']:.4g}/s  compact/dense "
                  f"{r['compact_over_dense']:.2f}  N/cells {r['N_over_cells']:.3f}  spread {max(r['spread_dense'], r['spread_compact']):.3f}", flush=True)
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
