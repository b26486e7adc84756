#!/usr/bin/env python3
"""The training step with and without history compaction, on one GPU, in one process, the arms alternating;
writes profiles/history_train.json stamped with the kernel-source digest.

Arms: trainer.train_step dense (which is also the parent commit's path) against train_step(compact_history=True) for several values of
``max_groups``, FlatAdam, eager stepping in every arm, each arm with its own model and optimizer started from the same state.  The
compact arms measure the history lengths inside the timed region the way BatchPrefetcher(history_len=True) does at staging time
(trainer.attach_history_len behind an event recorded once after the upload: a side stream that does not wait for the previous step's
kernels, one device-to-host copy of B integers), so the length kernel, the copy, the plan, the
permutations and the gather are all in the figure.
Workloads: the reference's default sizes (B = 256, H = 200, T = 15, emb 64) and C3 (B = 1024, H = 50, T = 30, emb 400), each under
three history-length distributions: uniform in [1, H], all H / 10, all H.  The distributions are ASSUMPTIONS: the history lengths of
the real data are in neither this repository nor the reference.  The all-H control plans a dense step: it shows what the length
kernel, the copy and the plan cost.  ``--saving-sweep``: the reference's default sizes with every history cut to a fixed share of H and
MIN_SAVING switched off, to find the smallest saving at which the compact step is not slower than the dense one beyond the spread.

Every arm is warmed up, then timed ROUNDS times over REPS steps with a device-event pair around work that ends in a synchronise; the
figure is the median of the rounds, the spread is (max - min) / median of the same arm's rounds.

    python scripts/history_train_bench.py [--workloads ref-default,C3-large] [--lengths uniform,tenth,full] [--groups 2,3,4,6,8] [--saving-sweep]
    python scripts/history_train_bench.py --error-budget RECORD.json      fold the ratios tests/test_gpu_history_train.py recorded into the JSON
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from news_recommendation_model_amd import build, compact, native, ops, synth, trainer   # noqa: E402
from news_recommendation_model_amd.config import Dims, WORKLOADS                         # noqa: E402

ROUNDS = 5
REPS = {"ref-default": 20, "C3-large": 4}
LENGTHS = {
    "uniform": lambda rng, B, H: rng.integers(1, H + 1, B),
    "tenth": lambda rng, B, H: np.full(B, max(H // 10, 1)),
    "full": lambda rng, B, H: np.full(B, H),
}


def make(name, L_of):
    w = WORKLOADS[name]
    dims = Dims.for_emb(w["emb"])
    B, H, T = w["B"], w["H"], w["T"]
    batch = synth.make_batch(dims, B, H, T, seed=3, user_num=10 * B, dtype=np.float32)
    L = L_of(np.random.default_rng(7 * B + w["emb"]), B, H)
    for b in range(B):
        batch["x_history"][b, int(L[b]):] = 0.0
    sd = synth.make_state_dict(dims, seed=1, user_num=10 * B)
    return w, dims, sd, trainer.batch_to_device(batch, "cuda"), L


def ms_per_step(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(name, L_of, groups):
    w, dims, sd, tb, L = make(name, L_of)
    B, H = w["B"], w["H"]
    uploaded = torch.cuda.Event()
    uploaded.record()                                            # the batch is resident from here on

    def arm(max_groups):
        model = trainer.build_model(dims, 10 * B, sd, device="cuda").train()
        opt = trainer.FlatAdam(model)
        if max_groups is None:
            return lambda: trainer.train_step(model, opt, tb)

        def step():                                              # (the side stream waits for the upload alone, as in the prefetcher)
            trainer.train_step(model, opt, trainer.attach_history_len(tb, after=uploaded), compact_history=True, max_groups=max_groups)
        return step
    arms = {"dense": arm(None), **{f"compact_g{g}": arm(g) for g in groups}}
    reps = REPS.get(name, 8)
    for fn in arms.values():
        for _ in range(3):
            fn()
    rounds = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            rounds[k].append(ms_per_step(fn, reps))
    ops.check_index_errors("cuda")
    out = {"B": B, "H": H, "T": w["T"], "emb": w["emb"], "history_rows": B * H, "steps_per_round": reps, "rounds": ROUNDS, "arms": {}}
    md = statistics.median(rounds["dense"])
    for k, r in rounds.items():
        m = statistics.median(r)
        rec = {"ms_per_step": m, "rounds_ms": r, "spread": (max(r) - min(r)) / m, "over_dense": m / md}
        if k != "dense":
            plan = compact.plan_history_groups(L, H, max_groups=int(k.split("_g")[1]))
            rec.update(G=plan.G, H_g=plan.H_g.tolist(), R=plan.R, R_over_history_rows=plan.R / (B * H), plan_dense=plan.dense)
        out["arms"][k] = rec
    return out


def fold_error_budget(path):
    """The ratios tests/test_gpu_history_train.py recorded, and M_TRAIN_HIST by the rule of DESIGN.md section 3b."""
    rec = json.load(open(path))
    ii = ("instant_interest_model.out_fc.0.weight", "instant_interest_model.out_fc.0.bias")      # sums that cancel: a constant of their own

    def pow2(worst):
        m = 1
        while m < 4 * worst:
            m *= 2
        return m
    worst_step = max(v for run in rec["step"].values() for k, v in run.items() if k not in ii)
    worst_ii = max(v for run in rec["step"].values() for k, v in run.items() if k in ii)
    return {"what": "step: err(compact step, R64) / max(err(dense HIP step, R64), 2^-23) per tensor, trainer.train_step(compact_history=True) against "
                    "the float64 oracle step (max_groups 1, 2, 4 and three lock-step optimizer steps); pool: err(weighted kernel, float64) / "
                    "max(err(unweighted kernel on the expanded input, float64), 2^-23), gate M_POOL = 4; node: err(grouped node, R64) / yardstick per "
                    "piece of tests/attention_budget.py against the float64 oracle on the DENSE input, gates M_F32 = 32, M_BF16X3 = 16, M_FC2_BIAS = 64",
            "worst_step_ratio": worst_step, "M_TRAIN_HIST": pow2(worst_step), "worst_step_ratio_instant_interest": worst_ii,
            "M_TRAIN_HIST_II": pow2(worst_ii), "step": rec["step"],
            "worst_pool_ratio": max(rec["pool"].values()), "worst_pool_ratio_by_placement": {
                p: max(v for k, v in rec["pool"].items() if k.startswith(p)) for p in ("forward", "score gradient", "history gradient")},
            "worst_node_ratio_over_its_constant": max(v / (64 if k.startswith("d_fc2.bias") else 16 if "bf16x3" in run else 32)
                                                      for run, d in rec["node"].items() for k, v in d.items()),
            "node": {run: max(d.values()) for run, d in rec["node"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ref-default,C3-large")
    ap.add_argument("--lengths", default=",".join(LENGTHS))
    ap.add_argument("--groups", default="2,3,4,6,8")
    ap.add_argument("--saving-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_train.json"))
    ap.add_argument("--error-budget", metavar="RECORD")
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    digest = build.sources_digest()
    if doc.get("kernel_sources_sha256") not in (None, digest):
        doc = {}                                                                               # figures of other sources are not mixed in
    doc["kernel_sources_sha256"] = digest

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if args.error_budget:
        doc["error_budget"] = fold_error_budget(args.error_budget)
        return save()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a timing taken elsewhere says nothing")
    native.load()
    groups = [int(g) for g in args.groups.split(",")]
    doc.update({"device": torch.cuda.get_device_name(0),
                "history_length_distributions_ASSUMED": {"uniform": "uniform in [1, H]", "tenth": "all H / 10", "full": "all H (control)"},
                "what": "ms per eager trainer.train_step (FlatAdam): dense (the parent's path) against compact_history=True with max_groups = g; "
                        "the history lengths of real data are NOT known, the distributions are assumptions"})
    if args.saving_sweep:
        prev, compact.MIN_SAVING = compact.MIN_SAVING, 0.0
        try:
            for share in (0.95, 0.9, 0.8, 0.7, 0.6, 0.5):
                r = measure("ref-default", lambda rng, B, H, s=share: np.full(B, max(int(round(s * H)) - 1, 0)), [1])
                doc.setdefault("saving_sweep", {})[f"ref-default/all {share} H"] = r
                a = r["arms"]["compact_g1"]
                print(f"saving sweep {share}: saving {1 - a['R_over_history_rows']:.3f}  compact/dense {a['over_dense']:.3f}  spread "
                      f"{max(a['spread'], r['arms']['dense']['spread']):.3f}", flush=True)
                save()
        finally:
            compact.MIN_SAVING = prev
        return
    for name in args.workloads.split(","):
        for lengths in args.lengths.split(","):
            doc.setdefault("workloads", {})[f"{name}/{lengths}"] = r = measure(name, LENGTHS[lengths], groups)
            print(f"{name}/{lengths}: " + "  ".join(f"{k} {v['ms_per_step']:.3f} ms (x{v['over_dense']:.3f}, R/(B H) {v.get('R_over_history_rows', 1.0):.3f}, "
                                                    f"spread {v['spread']:.3f})" for k, v in r["arms"].items()), flush=True)
            save()


if __name__ == "__main__":
    main()
