"""Measurement of the captured table epoch on compacted batches -> profiles/grouped_epoch.json.

    python scripts/grouped_epoch_bench.py [--out profiles/grouped_epoch.json] [--rounds 3] [--quick]

Data: the feed legs' tables of scripts/table_loader_bench.py (histories and lists with padding) at the reference's default sizes and at C3.
Legs, alternating in one process, a host clock around whole epochs between two synchronises, every leg on its own seeded model:
    dense_eager        trainer.train_epochs_tables
    dense_captured     trainer.GraphedTableEpoch (kept across epochs, as train_epochs_tables(graph=True) keeps it)
    eager_compacted    trainer.train_epochs_tables(compact_history=True, compact_candidates=True, max_groups=4): a plan per batch
    grouped_g2 / _g4   trainer.GroupedTableEpoch(compact_history=True, compact_candidates=True, max_groups=2 / 4): a plan per epoch
    grouped_hist_g4    the same with history groups only
    grouped_g4_same_order   grouped_g4 given the same order every epoch: no epoch plans or captures again (the steady state of a long epoch)
Every epoch draws a new permutation, so a grouped leg plans (and captures) again wherever the new epoch does not fit the plan it holds: the
captures per epoch are part of the result.  The front-end backward's device time per step (event pairs around nrm_frontend_bwd,
nrm_frontend_bwd_tables and nrm_frontend_cat_grad) is taken in one further epoch per leg kind that runs the leg's own launches EAGERLY
(events cannot be recorded inside a capture); its share is that time over the leg's measured step.  A run without a GPU fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from news_recommendation_model_amd import compact, native, synth, tables, trainer          # noqa: E402
from table_loader_bench import CONFIGS, make_tables          # noqa: E402

FRONTEND_BWD = {"nrm_frontend_bwd", "nrm_frontend_bwd_tables", "nrm_frontend_cat_grad"}
GROUPED = {"grouped_g2": dict(max_groups=2, compact_candidates=True), "grouped_g4": dict(max_groups=4, compact_candidates=True),
           "grouped_hist_g4": dict(max_groups=4, compact_candidates=False)}
FIXED = "grouped_g4_same_order"       # grouped_g4 on ONE order for all epochs: the plan always fits, so this is the replayed step alone


def bench(cfg, rounds, steps):
    B, H, T, dims = cfg["B"], cfg["H"], cfg["T"], cfg["dims"]
    t = make_tables(cfg, steps * B, seed=2)
    steps = t.n_impressions // B
    dt = t.to("cuda")
    user_num = t.max_user_id + 1
    sd = synth.make_state_dict(dims, seed=1, user_num=user_num)
    L, empty = t.history_len(np.arange(t.n_impressions), H), t.empty_num_all(T)
    grouped = dict(GROUPED, **{FIXED: GROUPED["grouped_g4"]})
    fixed_order = np.random.default_rng(5).permutation(t.n_impressions)
    runners, info = {}, {k: {"captures": [], "saving": []} for k in grouped}

    def fresh():
        model = trainer.build_model(dims, user_num, sd, device="cuda")
        return model, trainer.FlatAdam(model)

    def dense_eager(model, opt):
        return trainer.train_epochs_tables(model, opt, dt, 1, B, H, T, drop_last=True)

    def eager_compacted(model, opt):
        return trainer.train_epochs_tables(model, opt, dt, 1, B, H, T, drop_last=True, compact_history=True, compact_candidates=True, max_groups=4)

    def captured(name, make):
        def run(model, opt):
            if name not in runners:
                runners[name] = (make(model, opt), tables.TableLoader(dt, B, H, T, drop_last=True, seed=3))
            r, loader = runners[name]
            before = r.captures
            rec = r.run_epoch(fixed_order if name == FIXED else loader.take_order(), drop_last=True)
            if name in info:
                info[name]["captures"].append(r.captures - before)
                info[name]["saving"].append(r.plan.saving)
            return [rec]
        return run
    legs = {"dense_eager": dense_eager, "dense_captured": captured("dense_captured", lambda m, o: trainer.GraphedTableEpoch(m, o, dt, B, H, T)),
            "eager_compacted": eager_compacted}
    for name, kw in grouped.items():
        legs[name] = captured(name, lambda m, o, kw=kw: trainer.GroupedTableEpoch(m, o, dt, B, H, T, compact_history=True, **kw))
    state = {}
    for k in legs:
        state[k] = fresh()
        legs[k](*state[k])                                         # warm-up epoch (the captured legs' eager steps and first capture)
    for k in grouped:
        info[k] = {"captures": [], "saving": [], "warmup_epoch_saving": runners[k][0].plan.saving}
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = fn(*state[k])
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / (rec[0]["impressions"] / B))
    best = {k: min(v) for k, v in ms.items()}

    # the front-end backward's device time per step: the leg's launches, eagerly, with event pairs around the three entry points
    def frontend_ms(run_epoch):
        native.kernel_events, native.kernel_event_tags = [], FRONTEND_BWD
        try:
            n = run_epoch()
            torch.cuda.synchronize()
            per = {}
            for tag, e0, e1 in native.kernel_events:
                per[tag] = per.get(tag, 0.0) + e0.elapsed_time(e1)
        finally:
            native.kernel_events, native.kernel_event_tags = None, None
        return {tag: v / n for tag, v in per.items()}, sum(per.values()) / n
    fe = {}
    model, opt = fresh()
    dense_eager(model, opt)
    fe["dense"] = frontend_ms(lambda: dense_eager(model, opt)[0]["impressions"] // B)
    for name, kw in GROUPED.items():
        model, opt = fresh()
        r = trainer.GroupedTableEpoch(model, opt, dt, B, H, T, compact_history=True, warmup=10 ** 9, **kw)      # never captures
        order = tables.TableLoader(dt, B, H, T, drop_last=True, seed=3)
        r.run_epoch(order.take_order(), drop_last=True)
        fe[name] = frontend_ms(lambda: r.run_epoch(order.take_order(), drop_last=True)["steps"])
    share = {"dense_eager": fe["dense"][1] / best["dense_eager"], "dense_captured": fe["dense"][1] / best["dense_captured"]}
    share.update({k: fe[k][1] / best[k] for k in GROUPED})
    share[FIXED] = fe["grouped_g4"][1] / best[FIXED]
    per_batch = float(np.mean([compact.plan_history_groups(L[i * B:(i + 1) * B], H, max_groups=4).saving for i in range(steps)]))
    return {"B": B, "H": H, "T": T, "steps_per_epoch": steps, "mean_history_len": float(L.mean()), "mean_empty_num": float(empty.mean()),
            "ms_per_step": ms, "best_ms_per_step": best, "grouped": info,
            "frontend_bwd_ms_per_step": {k: {"by_entry": v[0], "total": v[1]} for k, v in fe.items()}, "frontend_bwd_share_of_step": share,
            "per_batch_history_saving_g4": per_batch,
            "grouped_g4_over_dense_captured": best["grouped_g4"] / best["dense_captured"],
            "grouped_g4_same_order_over_dense_captured": best[FIXED] / best["dense_captured"],
            "note": "ms per step = wall time of a whole epoch between two synchronises over its steps; a grouped leg's epochs include its host "
                    "planning, and any warm-up steps and capture a new plan costs (captures per epoch are listed)"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_epoch.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small step counts (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grouped_epoch_bench: no GPU; this measurement does not fall back")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "configs": {}}
    for name, cfg in CONFIGS.items():
        steps = (8 if args.quick else 96) if name == "ref-default" else (6 if args.quick else 24)
        result["configs"][name] = bench(cfg, args.rounds, steps)
        print(name, json.dumps(result["configs"][name]["best_ms_per_step"]), json.dumps(result["configs"][name]["grouped"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
