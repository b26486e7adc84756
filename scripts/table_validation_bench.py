"""Measurement of a validation pass over device-resident tables -> profiles/table_validation.json.

    python scripts/table_validation_bench.py [--out profiles/table_validation.json] [--rounds 3] [--quick]

(1) the pass: milliseconds per batch of 80 impressions (reference train.py:107) at the reference's default sizes and at the C3 shape, in three
    forms on the same tables and weights -- the parent commit's way (evaluation.validate_ranked over a tables.TableLoader),
    validate_tables(graph=False) (the same call behind the new entry point) and validate_tables(graph=True) through ONE GraphedTableScoring
    kept across passes, as train_epochs_tables(validation=...) and sweep_checkpoints keep it; legs alternating, a host clock around a pass
    (every pass ends in a host read), best of the rounds; host reads per pass are counted, not timed;
(2) nrm_eval_tally alone: device events around a run of launches queued behind large copies (the method of table_loader_bench.py), with
    labels and a record, at the widths of the two shapes.
A run without a GPU fails: nothing here falls back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from news_recommendation_model_amd import build, evaluation, ops, synth, tables, trainer          # noqa: E402
from news_recommendation_model_amd.config import Dims          # noqa: E402

VAL_BATCH = 80
PASSES = 3                                                             # passes inside one timed window
CONFIGS = {"ref-default": dict(H=200, T=15, dims=Dims()), "C3-large": dict(H=50, T=30, dims=Dims.for_emb(400))}


def make_tables(cfg, n_impressions, seed=0):
    """labelled records whose every list holds at least two entries (a list of one is a single-class row, on which validation raises)"""
    H, T, dims = cfg["H"], cfg["T"], cfg["dims"]
    rng = np.random.default_rng(seed)
    n_users = max(64, n_impressions // 4)
    lens = np.minimum(rng.geometric(1.0 / (0.6 * H), n_users), H + 20)
    lists = np.clip(rng.geometric(1.0 / (0.7 * T), n_impressions), 2, 3 * T)
    recs = synth.make_records(dims, 4096, n_users, n_impressions, seed=seed, history_lens=lens, list_lens=lists)
    return tables.ImpressionTables.from_records(*recs, dims, history_max=H)


def pass_leg(cfg, rounds, batches):
    H, T, dims = cfg["H"], cfg["T"], cfg["dims"]
    t = make_tables(cfg, batches * VAL_BATCH, seed=2)
    dt = t.to("cuda")
    n = t.n_impressions
    steps = (n + VAL_BATCH - 1) // VAL_BATCH
    user_num = t.max_user_id + 1
    model = trainer.build_model(dims, user_num, synth.make_state_dict(dims, seed=1, user_num=user_num), device="cuda")
    runner = evaluation.GraphedTableScoring([model], dt, VAL_BATCH, H, T, True)
    legs = {"validate_ranked_over_TableLoader": lambda: evaluation.validate_ranked([model], tables.TableLoader(dt, VAL_BATCH, H, T, shuffle=False)),
            "validate_tables_eager": lambda: evaluation.validate_tables([model], dt, VAL_BATCH, H=H, T=T, graph=False),
            "validate_tables_captured": lambda: evaluation.validate_tables([model], dt, VAL_BATCH, H=H, T=T, graph=True, runner=runner)}
    got = {k: fn() for k, fn in legs.items()}                          # warm-up pass of every leg (the captured one captures here)
    ref = got["validate_ranked_over_TableLoader"]
    assert all(abs(got[k][m] - ref[m]) <= n * 2.0 ** -52 * abs(ref[m]) for k in got for m in ref), got
    reads0 = runner.host_reads
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(PASSES):
                fn()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / (PASSES * steps))
    best = {k: min(v) for k, v in times.items()}
    widths = sorted({tp for _n, tp in evaluation.scoring_plan(runner.empty_all, n, VAL_BATCH, T)})
    return {"batch": VAL_BATCH, "H": H, "T": T, "impressions": n, "batches_per_pass": steps, "passes_per_window": PASSES, "widths_in_the_pass": widths,
            "graphs_captured": runner.captures, "ms_per_batch": times, "best_ms_per_batch": best,
            "captured_over_eager": best["validate_tables_eager"] / best["validate_tables_captured"],
            "host_reads_per_pass": {"validate_ranked_over_TableLoader": steps + 1, "validate_tables_eager": steps + 1,
                                    "validate_tables_captured": (runner.host_reads - reads0) // (rounds * PASSES)},
            "means": ref,
            "note": "the eager legs read the device once per batch (the common trim is int(empty_num.min()) of a device tensor) and once at the "
                    "end; the captured leg plans every width on the host from the producer's empty_num and reads the state buffer once"}


def tally_leg(cfg, rounds, iters):
    B, T = VAL_BATCH, cfg["T"]
    cap = 4 * B
    state = torch.zeros(10, dtype=torch.int64, device="cuda")
    cursor, sums, counts = state[0:1], state[1:6].view(torch.float64), state[6:10]
    rec = (torch.zeros(cap, T, dtype=torch.int32, device="cuda"), torch.zeros(cap, dtype=torch.int32, device="cuda"),
           torch.zeros(cap, dtype=torch.int64, device="cuda"))
    auc, top1 = torch.rand(B, device="cuda"), torch.randint(0, 2, (B,), device="cuda", dtype=torch.int32)
    metrics, rank = torch.rand(B, 3, device="cuda"), torch.randint(0, T + 1, (B, T), device="cuda", dtype=torch.int32)
    live, ids = torch.full((B,), T, dtype=torch.int32, device="cuda"), torch.arange(B, device="cuda")
    fn = lambda: ops.eval_tally(auc, top1, metrics, rank, live, ids, cursor, sums, counts, *rec, 1 << 40)      # noqa: E731
    big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)

    def run():
        for _ in range(40):
            big2.copy_(big)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters
    run()
    times = [run() for _ in range(rounds)]
    return {"B": B, "T": T, "record_rows": cap, "iters_per_run": iters, "us_per_call": times, "best_us": min(times)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_validation.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small pass lengths (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("table_validation_bench: no GPU; this measurement does not fall back")
    result = {"kernel_sources_sha256": build.sources_digest(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "pass": {}, "tally": {}}
    for name, cfg in CONFIGS.items():
        result["tally"][name] = tally_leg(cfg, args.rounds, 20 if args.quick else 200)
        print(name, "tally", result["tally"][name]["best_us"], "us", flush=True)
    for name, cfg in CONFIGS.items():
        result["pass"][name] = pass_leg(cfg, args.rounds, (4 if args.quick else 100) if name == "ref-default" else (3 if args.quick else 40))
        print(name, "pass", json.dumps(result["pass"][name]["best_ms_per_batch"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
