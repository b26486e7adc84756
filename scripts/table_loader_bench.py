"""Measurement of batch assembly from device-resident tables -> profiles/table_loader.json.

    python scripts/table_loader_bench.py [--out profiles/table_loader.json] [--rounds 3] [--quick]

(1) the kernel: nrm_assemble_batch at (B, H, T, dims) = (256, 200, 15, default) and (1024, 50, 30, for_emb(400)) against a device-to-device
    copy_ of one tensor of the same output bytes, on the same device in the same run, legs alternating, device events around runs of launches;
(2) the feed: impressions per second of trainer.train_epochs (host float64 batches, already collated in host memory, through BatchPrefetcher)
    against trainer.train_epochs_tables on the same synthetic data, at the reference's default sizes and at C3, epochs alternating, a host clock
    around an epoch (which ends in a synchronise); a third leg runs the same epochs through trainer.GraphedTableEpoch (one graph replay per
    step; the object, and with it the captured graph, is kept across epochs as train_epochs_tables(graph=True) keeps it);
(3) the two kernels of the captured step that the eager one does not have: nrm_epoch_tally, and the cursor form of the assemble kernel against
    the sel form, with the event bracketing of (1).
--only captured: (2) and (3) alone, merged into the existing file under the key "captured_epoch".
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
from news_recommendation_model_amd import synth, tables, trainer          # noqa: E402
from news_recommendation_model_amd.config import Dims          # noqa: E402

CONFIGS = {"ref-default": dict(B=256, H=200, T=15, dims=Dims()), "C3-large": dict(B=1024, H=50, T=30, dims=Dims.for_emb(400))}
# the captured legs also run on data WITHOUT padding (every history at least H events, every list at least T entries): the data of bench.py's
# resident batches, on which the default sizes are launch-bound
CAPTURED_CONFIGS = dict(CONFIGS, **{"ref-default-full": dict(B=256, H=200, T=15, dims=Dims(), full=True)})


def make_tables(cfg, n_impressions, seed=0):
    B, H, T, dims = cfg["B"], cfg["H"], cfg["T"], cfg["dims"]
    rng = np.random.default_rng(seed)
    n_users = max(64, n_impressions // 4)
    lens = np.minimum(rng.geometric(1.0 / (0.6 * H), n_users), H + 20)              # many full histories, a tail of short ones
    lists = np.clip(rng.geometric(1.0 / (0.7 * T), n_impressions), 1, 3 * T)
    if cfg.get("full"):
        lens, lists = np.full(n_users, H + 5), np.clip(lists, T, 3 * T)
    recs = synth.make_records(dims, 4096, n_users, n_impressions, seed=seed, history_lens=lens, list_lens=lists)
    return tables.ImpressionTables.from_records(*recs, dims, history_max=H)


def out_bytes(batch):
    return sum(int(v.numel() * v.element_size()) for v in batch.values())


def kernel_leg(cfg, rounds, iters):
    B, H, T = cfg["B"], cfg["H"], cfg["T"]
    t = make_tables(cfg, 4 * B)
    dt = t.to("cuda")
    sel = torch.from_numpy(np.random.default_rng(1).permutation(t.n_impressions)[:B].astype(np.int64)).cuda()
    batch = tables.assemble_batch(dt, sel, H, T)
    nbytes = out_bytes(batch)
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty_like(src)
    legs = {"assemble": lambda: tables.assemble_batch(dt, sel, H, T), "copy": lambda: dst.copy_(src)}
    big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)

    def run(fn):
        # the host needs tens of microseconds per call, more than either kernel runs at the default sizes: a run of large copies goes first,
        # so that all timed launches are queued before the device reaches them and the events bracket device time, not the enqueue rate
        for _ in range(40):
            big2.copy_(big)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters              # microseconds per call
    for fn in legs.values():
        run(fn)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(run(fn))
    best = {k: min(v) for k, v in times.items()}
    return {"B": B, "H": H, "T": T, "history_cols": t.history_cols, "output_bytes": nbytes, "table_bytes": t.nbytes, "iters_per_run": iters,
            "us_per_call": times, "best_us": best, "assemble_over_copy": best["assemble"] / best["copy"],
            "assemble_GBps_written": nbytes / best["assemble"] / 1e3, "copy_GBps_written": nbytes / best["copy"] / 1e3,
            "note": "device time of back-to-back launches queued behind a run of large copies (the host enqueues slower than either kernel runs); "
                    "the copy reads and writes the bytes once; the large copies leave neither leg's data in the last-level cache at the start"}


def captured_kernel_leg(cfg, rounds, iters):
    """device time of the tally kernel and of the assemble kernel in its cursor form against its sel form (method of kernel_leg)"""
    from news_recommendation_model_amd import ops
    B, H, T = cfg["B"], cfg["H"], cfg["T"]
    t = make_tables(cfg, 4 * B)
    dt = t.to("cuda")
    order = torch.from_numpy(np.random.default_rng(1).permutation(t.n_impressions).astype(np.int64)).cuda()
    sel, cursor = order[:B].clone(), torch.zeros(1, dtype=torch.int64, device="cuda")
    state = torch.zeros(6 + 64, dtype=torch.int64, device="cuda")
    tcur, sums, counts, log = state[0:1], state[1:4].view(torch.float64), state[4:6], state[6:].view(torch.float32).view(64, 2)
    loss = torch.tensor(0.7, device="cuda")
    auc, top1 = torch.rand(B, device="cuda"), torch.randint(0, 2, (B,), device="cuda", dtype=torch.int32)
    legs = {"assemble_sel": lambda: tables.assemble_batch(dt, sel, H, T), "assemble_cursor": lambda: tables.assemble_batch_at(dt, order, cursor, B, H, T),
            "tally": lambda: ops.epoch_tally(loss, auc, top1, tcur, sums, counts, log)}
    big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)

    def run(fn):
        for _ in range(40):
            big2.copy_(big)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters
    for fn in legs.values():
        run(fn)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(run(fn))
    return {"B": B, "H": H, "T": T, "iters_per_run": iters, "us_per_call": times, "best_us": {k: min(v) for k, v in times.items()}}


def feed_leg(cfg, rounds, steps, host_batches, only_tables=False):
    B, H, T, dims = cfg["B"], cfg["H"], cfg["T"], cfg["dims"]
    t = make_tables(cfg, steps * B, seed=2)
    steps = t.n_impressions // B
    dt = t.to("cuda")
    user_num = t.max_user_id + 1
    sd = synth.make_state_dict(dims, seed=1, user_num=user_num)
    order = np.arange(t.n_impressions)
    hosts = [tables.assemble_host(t, order[i * B:(i + 1) * B], H, T) for i in range(min(host_batches, steps))]
    hosts = [{k: v for k, v in h.items() if k in ("user_id", "x_history", "x_target", "x_global", "label", "empty_num")} for h in hosts]
    host_step_bytes = sum(int(v.nbytes) for v in hosts[0].values())

    def host_epoch(model, opt):
        return trainer.train_epochs(model, opt, lambda: (hosts[i % len(hosts)] for i in range(steps)), 1)

    def table_epoch(model, opt):
        return trainer.train_epochs_tables(model, opt, dt, 1, B, H, T, drop_last=True)
    runners = {}

    def captured_epoch(model, opt):
        if "r" not in runners:                                     # (its first epoch holds the eager warm-up steps and the capture)
            runners["r"] = trainer.GraphedTableEpoch(model, opt, dt, B, H, T)
            runners["order"] = tables.TableLoader(dt, B, H, T, drop_last=True)
        return [runners["r"].run_epoch(runners["order"].take_order(), drop_last=True)]
    legs = {"host_prefetcher": host_epoch, "tables": table_epoch, "tables_captured": captured_epoch}
    if only_tables:
        del legs["host_prefetcher"]
    state = {}
    for k in legs:
        model = trainer.build_model(dims, user_num, sd, device="cuda")
        state[k] = (model, trainer.FlatAdam(model))
        legs[k](*state[k])                                         # warm-up epoch
    rates = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = fn(*state[k])
            torch.cuda.synchronize()
            rates[k].append(rec[0]["impressions"] / (time.perf_counter() - t0))
    best = {k: max(v) for k, v in rates.items()}
    return {"B": B, "H": H, "T": T, "steps_per_epoch": steps, "impressions_per_s": rates, "best_impressions_per_s": best,
            "ms_per_step": {k: 1e3 * B / v for k, v in best.items()},
            "tables_over_host": best["tables"] / best["host_prefetcher"] if "host_prefetcher" in best else None,
            "captured_over_eager_tables": best["tables_captured"] / best["tables"],
            "table_bytes_resident": t.nbytes, "host_bytes_per_step": {"host_prefetcher": host_step_bytes, "tables": 8 * B},
            "distinct_host_batches": len(hosts),
            "note": "the host leg cycles batches that are already collated float64 arrays in host memory (no ETL, no DataLoader workers): "
                    "it measures pinning and the upload through BatchPrefetcher, the most the host path can deliver"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_loader.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small step counts (a rehearsal, not a measurement)")
    ap.add_argument("--only", default=None, choices=["captured"],
                    help="captured: the table-fed legs (eager and captured) and the captured step's own kernels, merged into --out under 'captured_epoch'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("table_loader_bench: no GPU; this measurement does not fall back")
    if args.only == "captured":
        part = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "kernel": {}, "feed": {}}
        for name, cfg in CONFIGS.items():
            part["kernel"][name] = captured_kernel_leg(cfg, args.rounds, 20 if args.quick else 200)
            print(name, "kernel", json.dumps(part["kernel"][name]["best_us"]), flush=True)
        for name, cfg in CAPTURED_CONFIGS.items():
            steps = (6 if args.quick else 96) if name.startswith("ref-default") else (5 if args.quick else 24)
            part["feed"][name] = feed_leg(cfg, args.rounds, steps, host_batches=1, only_tables=True)
            print(name, "feed", json.dumps(part["feed"][name]["ms_per_step"]), flush=True)
        result = json.load(open(args.out)) if os.path.exists(args.out) else {}
        result["captured_epoch"] = part
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
        print("wrote", args.out)
        sys.exit(0)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "kernel": {}, "feed": {}}
    for name, cfg in CONFIGS.items():
        result["kernel"][name] = kernel_leg(cfg, args.rounds, 20 if args.quick else 200)
        print(name, "kernel", json.dumps(result["kernel"][name]["best_us"]), result["kernel"][name]["assemble_over_copy"], flush=True)
    for name, cfg in CONFIGS.items():
        steps = (4 if args.quick else 96) if name == "ref-default" else (3 if args.quick else 24)
        result["feed"][name] = feed_leg(cfg, args.rounds, steps, host_batches=8 if name == "ref-default" else 4)
        print(name, "feed", json.dumps(result["feed"][name]["best_impressions_per_s"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
