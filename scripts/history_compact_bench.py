#!/usr/bin/env python3
"""Compact scoring with and without history compaction, on one GPU, in one process, the two arms alternating;
writes profiles/history_compact.json stamped with the kernel-source digest.

Arms: evaluation.predict_ranked_compact (today's compact path, which is also the parent commit's: every one of the B H history rows
goes through the front end, w1, the u GEMM and both attentions) against predict_ranked_compact(history=True) on the same batches
(length kernel, one device-to-host copy of B integers, live history rows + one representative padded row per impression), two models.
Workloads: the ones of scripts/compact_scoring_bench.py -- reference dimensions (emb 64, H = 200) and C3 dimensions (emb 400, H = 50),
batches of 80 and 1 024, candidate lists padded to 100 columns with live counts from the percentiles of the reference's
configs/model_config.py:32 -- each under three history-length distributions: uniform in [1, H], all H / 10, all H.  The
distributions are ASSUMPTIONS: the history lengths of the real data are in neither this repository nor the reference.  The all-H
control hands the batch to the history=False path after the length kernel and the copy: it shows what those two cost.

Every arm is warmed up, then timed ROUNDS times over REPS calls with a device-event pair around work that ends in a synchronise; the
figure is the median of the rounds, the spread is (max - min) / median of the same arm's rounds.

    python scripts/history_compact_bench.py [--workloads NAME,...] [--lengths uniform,tenth,full] [--out profiles/history_compact.json]
    python scripts/history_compact_bench.py --trace NAME --lengths uniform --arm compact|history      a few calls of one arm, for
        NRM_BRANCH_STREAMS=0 rocprofv3 --kernel-trace --stats -- python scripts/history_compact_bench.py --trace ...
    python scripts/history_compact_bench.py --kernel-stats NAME LENGTHS compact.csv history.csv      fold two kernel_stats.csv into the JSON
    python scripts/history_compact_bench.py --error-budget DIR      fold the ratios the tests recorded (NRM_COMPACT_RECORD=DIR) into the JSON
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
    # name: emb, H, B, T, calls per round
    "ref_B80": dict(emb=64, H=200, B=80, T=PAD_TO, reps=10),
    "ref_B1024": dict(emb=64, H=200, B=1024, T=PAD_TO, reps=4),
    "c3_B80": dict(emb=400, H=50, B=80, T=PAD_TO, reps=6),
    "c3_B1024": dict(emb=400, H=50, B=1024, T=PAD_TO, reps=2),
}
LENGTHS = {
    "uniform": lambda rng, B, H: rng.integers(1, H + 1, B),
    "tenth": lambda rng, B, H: np.full(B, max(H // 10, 1)),
    "full": lambda rng, B, H: np.full(B, H),
}


def make(name, lengths):
    w = WORKLOADS[name]
    dims = Dims.for_emb(w["emb"])
    B, H, T = w["B"], w["H"], w["T"]
    batch = synth.make_batch(dims, B, H, T, seed=3, user_num=10 * B, dtype=np.float32)
    pad_batch(batch, percentile_counts(np.random.default_rng(B + w["emb"]), B, T, one_long=True))
    L = LENGTHS[lengths](np.random.default_rng(7 * B + w["emb"]), B, H)
    for b in range(B):
        batch["x_history"][b, int(L[b]):] = 0.0
    models = [trainer.build_model(dims, 10 * B, synth.make_state_dict(dims, seed=s, user_num=10 * B), device="cuda").eval() for s in (1, 2)]
    tb = {k: torch.from_numpy(batch[k]).cuda() for k in ("x_history", "x_target", "x_global")}
    tb["empty_num"] = torch.from_numpy(batch["empty_num"])                                   # host tensor, as a DataLoader hands it over
    plan = compact.build_plan(batch["empty_num"], T, history_len=ops.history_len(tb["x_history"]).cpu().numpy(), H=H)
    assert plan.hist_len.tolist() == [int(x) for x in L]
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


def measure(name, lengths):
    w, models, tb, plan = make(name, lengths)
    arms = {"compact": lambda: evaluation.predict_ranked_compact(models, tb),
            "history": lambda: evaluation.predict_ranked_compact(models, tb, history=True)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    rounds = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            rounds[k].append(rate(fn, w["B"], w["reps"]))
    ops.check_index_errors("cuda")
    ops.check_pad_errors("cuda")
    mc, mh = statistics.median(rounds["compact"]), statistics.median(rounds["history"])
    sc, sh = (max(rounds["compact"]) - min(rounds["compact"])) / mc, (max(rounds["history"]) - min(rounds["history"])) / mh
    return {"compact_impressions_per_s": mc, "history_impressions_per_s": mh, "compact_rounds": rounds["compact"], "history_rounds": rounds["history"],
            "spread_compact": sc, "spread_history": sh, "history_over_compact": mh / mc, "equal_within_spread": bool(abs(mh - mc) <= max(sc, sh) * mc),
            "B": w["B"], "H": w["H"], "emb": w["emb"], "N": plan.N, "R": plan.R, "history_rows": plan.B * plan.H,
            "R_over_history_rows": plan.R / (plan.B * plan.H), "score_rows": 16 * plan.Mt, "dense_score_rows": plan.N * plan.H,
            "score_rows_ratio": 16 * plan.Mt / (plan.N * plan.H), "k_max": plan.k_max, "history_dense": plan.history_dense,
            "calls_per_round": w["reps"], "rounds": ROUNDS}


def fold_kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    fwd = [r for r in rows if "pwattn_fwd" in r["Name"] and "pack" not in r["Name"]]
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]
    return {"attention_forward_ms_per_call": sum(float(r["TotalDurationNs"]) for r in fwd) / 1e6 / TRACE_CALLS,
            "all_kernels_ms_per_call": sum(float(r["TotalDurationNs"]) for r in rows) / 1e6 / TRACE_CALLS,
            "top": [{"name": r["Name"][:100], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6} for r in top]}


def fold_error_budget(directory):
    """The ratios tests/test_gpu_history_compact.py recorded: worst per kind, and the logit constant by the rule of DESIGN section 3b."""
    rows = [json.loads(ln) for ln in open(os.path.join(directory, "history_compact_ratios.jsonl"))]
    logit = {r["case"]: {"ratio": r["ratio"], "largest_logit_difference": r["delta"], "N": r["N"], "R": r["R"], "history_rows": r["history_rows"]}
             for r in rows if r["kind"] == "logit"}
    worst = max(v["ratio"] for v in logit.values())
    m = 1
    while m < 4 * worst:
        m *= 2
    att = {}
    for r in rows:
        if r["kind"] == "attention":
            key = f"{r['case']} / {r['piece']} / {r['norm']}"
            att[key] = max(att.get(key, 0.0), r["ratio"])
    return {"what": "err(history-compact, R64) / max(err(dense, R64), 2^-23), worst impression, from test_logits_against_dense_and_float64; attention: "
                    "err(kernel, R64) / max(err(R32, R64), 2^-23) per piece against the float64 oracle on the DENSE input, gate M_F32 = 32",
            "logit": logit, "worst_logit_ratio": worst, "M_LOGIT_HIST": m, "attention_worst_ratio": max(att.values()) if att else None, "attention": att,
            "end_to_end": [r for r in rows if r["kind"] == "end_to_end"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--lengths", default=",".join(LENGTHS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_compact.json"))
    ap.add_argument("--trace")
    ap.add_argument("--arm", default="history", choices=["compact", "history"])
    ap.add_argument("--kernel-stats", nargs=4, metavar=("WORKLOAD", "LENGTHS", "COMPACT_CSV", "HISTORY_CSV"))
    ap.add_argument("--error-budget", metavar="DIR")
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    digest = build.sources_digest()
    if doc.get("kernel_sources_sha256") != digest:
        doc = {k: doc[k] for k in ("error_budget",) if k in doc}                             # timings of other sources are not mixed in
    if args.error_budget:
        doc["error_budget"] = fold_error_budget(args.error_budget)
        doc["error_budget"]["kernel_sources_sha256"] = digest
    elif args.kernel_stats:
        name, lengths, c_csv, h_csv = args.kernel_stats
        c, h = fold_kernel_stats(c_csv), fold_kernel_stats(h_csv)
        doc.setdefault("kernel_trace", {})[f"{name}/{lengths}"] = {
            "compact": c, "history": h, "calls_traced": TRACE_CALLS,
            "attention_forward_history_over_compact": h["attention_forward_ms_per_call"] / c["attention_forward_ms_per_call"]}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("needs an MI355X: a timing taken elsewhere says nothing")
        native.load()
        if args.trace:
            w, models, tb, plan = make(args.trace, args.lengths.split(",")[0])
            for _ in range(TRACE_CALLS):
                evaluation.predict_ranked_compact(models, tb, history=args.arm == "history")
            torch.cuda.synchronize()
            return
        doc.update({"kernel_sources_sha256": digest, "device": torch.cuda.get_device_name(0), "pad_to_columns_ASSUMED": PAD_TO,
                    "history_length_distributions_ASSUMED": {"uniform": "uniform in [1, H]", "tenth": "all H / 10", "full": "all H (control)"},
                    "what": "impressions/s of predict_ranked_compact (compact: the parent's path) against predict_ranked_compact(history=True), two "
                            "models, eager; candidate lists as in compact_scoring.json; the history lengths of real data are NOT known, the three "
                            "distributions are assumptions"})
        for name in args.workloads.split(","):
            for lengths in args.lengths.split(","):
                doc.setdefault("workloads", {})[f"{name}/{lengths}"] = r = measure(name, lengths)
                print(f"{name}/{lengths}: compact {r['compact_impressions_per_s']:.4g}/s  history {r['history_impressions_per_s']:.4g}/s  history/compact "
                      f"{r['history_over_compact']:.2f}  R/(B H) {r['R_over_history_rows']:.3f}  score rows {r['score_rows_ratio']:.3f}  "
                      f"spread {max(r['spread_compact'], r['spread_history']):.3f}", flush=True)
                with open(args.out, "w") as f:
                    json.dump(doc, f, indent=1)
                    f.write("\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
