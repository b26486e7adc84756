"""Inference and validation semantics of the reference's test.py / verify.py on top of the HIP forward.

  predict(models, batch)        test.py:31-74  model_test: eval-mode forward, trailing padding common to the batch
                                trimmed before the forward (:48-56), softmax over candidates averaged over the
                                model list (:58-64), and -- for rows that still carry their own padding -- a SECOND
                                softmax over the already-softmaxed, de-padded slice (:68).  Kept as is, not "fixed".
  row_auc_top1(scores, labels)  train.py:77-80 / verify.py:25-36: per-impression ROC-AUC and top-1 hit, on device
                                (C ABI nrm_row_auc) instead of one sklearn call per row on the host.
  validate(models, batches)     verify.py:19-43 model_validation: [mean AUC, top-1 rate].
  rank_row(scores)              test.py:118-126: 1-based rank of every candidate, highest score first.
  predict_ranked(models, batch) test.py:58-70 + :118-126 with the whole tail after the forwards -- softmax per model, mean,
                                second softmax, rank, optionally MRR / nDCG -- as ONE launch (C ABI nrm_ensemble_rank).
  predict_ranked_compact(models, batch)  predict_ranked() without the padding: each impression's live candidates and ONE representative
                                padded candidate go through the forwards (ragged kernels), the tail counts the representative e' times.
  validate_ranked(models, batches)   validate() plus MRR, nDCG@5, nDCG@10.
  write_predictions / zip_predictions   test.py:76-132: one "<impression id> [r1,r2,...]" line per impression, zipped.
  score_dataset(models, head_path, out_dir)   test.py's model_test + write_submission_file over a processed test set.
  save_checkpoint / load_checkpoint   train.py:95-97 (state_dict minus 'delta'), test.py:160 (strict=False).
  GraphedTableScoring / validate_tables / score_tables / sweep_checkpoints   train.py:107-110, test.py and verify.py:53-75 over a data
                                set that lives on the device as tables: one graph replay per batch, one host read per pass.
"""
from __future__ import annotations

import torch

from . import ops


@torch.no_grad()
def predict(models, batch):
    """-> (scores [B, T'] on device, live [B] number of real candidates per row).  ``batch`` holds x_history,
    x_target, x_global and empty_num (trailing all-padding candidates per row)."""
    xh, xt, xg = batch["x_history"], batch["x_target"], batch["x_global"]
    ops._require_gpu(xh, xt, xg)
    # the common-padding trim is a HOST decision (it changes T): taken from the tensor where it lives, so a DataLoader's CPU
    # tensor costs no device synchronisation and the host keeps launching ahead of the GPU (a device tensor forces one per batch)
    e_in = batch["empty_num"]
    trim = int(e_in.min()) if e_in.numel() else 0
    empty = e_in.to(xt.device, non_blocking=True).to(torch.int64)
    if trim > 0:                                              # test.py:48-56
        xt, xg = xt[:, :-trim], xg[:, :-trim]
        empty = empty - trim
    out = None
    for m in models:                                          # test.py:58-64
        m.eval()
        p = torch.softmax(m(xh, xt, xg), dim=1)
        out = p if out is None else out + p
    out = out / len(models)
    T = out.shape[1]
    live = T - empty
    # rows with remaining padding: softmax AGAIN over the de-padded slice of the softmaxed scores (test.py:68)
    cols = torch.arange(T, device=out.device)[None, :]
    mask = cols < live[:, None]
    padded = (empty > 0)[:, None]
    again = torch.softmax(out.masked_fill(~mask, float("-inf")), dim=1)
    scores = torch.where(padded, again, out)
    return scores, live


class _WeightsWatch:
    """What a captured forward has to know about its models' weights before a replay (the rule in GraphedPredict's docstring, shared with
    GraphedTableScoring): ``check(have_graphs)`` -> True where an ADDRESS of a parameter or buffer, or the generation of the packed-weight
    cache, has changed since the last look -- the caller drops its graphs; where only version counters have moved and graphs exist, the
    packed images are refreshed in place by one eager ``ops.repack_persistent`` launch.  ``refresh()`` takes the present state as seen
    (after a capture, whose warm-up may have created the images)."""

    def __init__(self, models):
        self.models = models
        self.addresses = self.versions = None

    def state(self):
        tensors = [t for m in self.models for t in list(m.parameters()) + list(m.buffers())]
        return (tuple(t.data_ptr() for t in tensors) + (ops.packed_weights_generation(),)), tuple(t._version for t in tensors)

    def check(self, have_graphs):
        addresses, versions = self.state()
        dropped = addresses != self.addresses
        if dropped:
            self.addresses = addresses
        elif versions != self.versions and have_graphs:
            ops.repack_persistent([p for m in self.models for p in m.parameters()])      # same buffers the graphs read
        self.versions = versions
        return dropped

    def refresh(self):
        self.addresses, self.versions = self.state()


class GraphedPredict:
    """predict() captured into one HIP graph per (input shapes, common-padding trim) and replayed: the reference's test batches
    (80 impressions, test.py:46) are launch-bound when stepped eagerly -- ~0.9 ms of host work for ~0.35 ms of kernels.  Inputs
    are copied into static device buffers (from host or device tensors), the graph is replayed, and the returned ``scores`` /
    ``live`` are the graph's static outputs: valid until the next call with the same key (clone them to keep them).
    At most ``max_graphs`` graphs are kept (least recently used first out).

    Weights may change between calls (validation after every epoch, another checkpoint loaded into the same model).  A graph
    bakes in ADDRESSES: parameters and buffers are read where they live, and the dense / side-projection GEMMs read the packed
    weight images of ``ops._pack``, which were filled during the warm-up calls BEFORE the capture (no pack launch is recorded).
    So every call compares (a) the addresses of all parameters and buffers and the generation of the packed-weight cache --
    a change (``.to()``, ``FlatAdam`` re-seating the parameters, ``ops.invalidate_packed_weights()``) drops every graph -- and
    (b) their autograd version counters: a change (``load_state_dict``, ``torch.optim`` steps, any in-place op) re-packs the
    images IN PLACE with one eager launch (``ops.repack_persistent``) before the replay.  ``trainer.FlatAdam.step()`` updates
    weights through a raw pointer but refreshes the same images itself."""

    def __init__(self, models, max_graphs=16):
        self.models = list(models)
        self.max_graphs = max_graphs
        self.graphs = {}
        self._weights = _WeightsWatch(self.models)

    @torch.no_grad()
    def __call__(self, batch):
        from . import native
        if native.kernel_events is not None:
            raise RuntimeError("per-kernel event timing cannot be recorded inside a graph capture")
        dev = next(self.models[0].parameters()).device
        if self._weights.check(bool(self.graphs)):
            self.graphs.clear()                                       # captured addresses are gone: capture again
        e_in = batch["empty_num"]
        trim = int(e_in.min()) if e_in.numel() else 0                 # host decision, as in predict()
        names = ("x_history", "x_target", "x_global", "empty_num")
        key = tuple((tuple(batch[k].shape), batch[k].dtype) for k in names) + (trim,)
        ent = self.graphs.pop(key, None)
        if ent is None:
            static = {k: torch.empty(batch[k].shape, dtype=batch[k].dtype, device=dev) for k in names}
            for k in names:
                static[k].copy_(batch[k], non_blocking=True)
            host_empty = torch.full_like(e_in, trim, device="cpu")   # what predict() reads on the host: only its minimum matters
            feed = dict(static, empty_num=_HostMin(static["empty_num"], host_empty))
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):                             # allocator / packed-weight warm-up outside the capture
                for _ in range(2):
                    predict(self.models, feed)
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                scores, live = predict(self.models, feed)
            ent = (graph, static, scores, live)
            while len(self.graphs) >= self.max_graphs:
                self.graphs.pop(next(iter(self.graphs)))
            self._weights.refresh()                                   # (the warm-up may have created the packed images)
        else:
            for k in names:
                ent[1][k].copy_(batch[k], non_blocking=True)
        self.graphs[key] = ent                                        # (re-inserted last: most recently used)
        ent[0].replay()
        return ent[2], ent[3]


class _HostMin:
    """empty_num for a captured predict(): .min() / .numel() answer from a host tensor (no synchronisation, nothing captured),
    .to(device) hands over the static device buffer."""

    def __init__(self, device_tensor, host_tensor):
        self.dev, self.host = device_tensor, host_tensor

    def numel(self):
        return self.host.numel()

    def min(self):
        return self.host.min()

    def to(self, *args, **kwargs):
        return self.dev


def row_auc_top1(scores, labels, live=None):
    """Per-row AUC [B] (fp32, -1 where a row has one class) and top-1 hit [B] (int32) on the device."""
    ops._require_gpu(scores, labels)
    return ops.row_auc(scores, labels, live)                    # torch.ops.nrm.row_auc -> C ABI nrm_row_auc


@torch.no_grad()
def validate(models, batches):
    """verify.py:19-43: mean per-impression AUC and top-1 rate over an iterable of device batches (with labels)."""
    auc_sum = torch.zeros((), dtype=torch.float64, device="cuda")
    hit_sum = torch.zeros((), dtype=torch.float64, device="cuda")
    n = 0
    for batch in batches:
        scores, live = predict(models, batch)
        label = batch["label"][:, :scores.shape[1]].to(scores.device)
        auc, top1 = row_auc_top1(scores, label, live)
        if bool((auc < 0).any()):
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        auc_sum += auc.double().sum()
        hit_sum += top1.double().sum()
        n += scores.shape[0]
    # an out-of-range table index in any batch (the reference raises IndexError); the flag of the MODELS' device
    ops.check_index_errors(next(models[0].parameters()).device)
    return [float(auc_sum / n), float(hit_sum / n)]


def rank_row(scores_row):
    """test.py:118-126: rank string items -- candidate with the highest score gets rank 1 (stable for ties)."""
    order = sorted(range(len(scores_row)), key=lambda i: scores_row[i], reverse=True)
    rank = [0] * len(scores_row)
    for r, i in enumerate(order):
        rank[i] = r + 1
    return rank


@torch.no_grad()
def predict_ranked(models, batch, with_metrics=False):
    """-> (scores [B, T'] fp32, rank [B, T'] int32, live [B] int32[, metrics [B, 3] fp32 = (rr, ndcg5, ndcg10)]), all on the device.

    predict() with its tail fused: the same host-side trim decision (taken from ``empty_num`` where it lives: a host tensor
    costs no device synchronisation), the models' eval-mode forwards, then one ``ops.ensemble_rank`` launch that reads every
    model's logits where the last GEMM left them.  ``rank`` is what ``rank_row`` gives for the row's live scores (1 = highest,
    ties by index), 0 on padding columns.  Differences from predict(): padding columns of rows that keep their own padding
    hold score 0 either way, but a row with NO live candidate is all zeros here (NaN there), and ``live`` is int32.
    ``with_metrics`` needs ``batch["label"]``; rows without a live positive get -1 in all three metrics.
    Capturable into a graph (``torch.cuda.graph``) when ``empty_num`` answers ``.min()`` on the host, as GraphedPredict's
    ``_HostMin`` does, and the label (if any) is a float32 device tensor."""
    xh, xt, xg = batch["x_history"], batch["x_target"], batch["x_global"]
    ops._require_gpu(xh, xt, xg)
    e_in = batch["empty_num"]
    trim = int(e_in.min()) if e_in.numel() else 0             # host decision (it changes T), as in predict()
    if isinstance(e_in, torch.Tensor) and not e_in.is_cuda:   # a DataLoader's host tensor: subtract and narrow before the one copy
        empty = (e_in - trim).to(torch.int32).to(xt.device, non_blocking=True)
    else:
        empty = e_in.to(xt.device, non_blocking=True)
        empty = empty - trim if trim > 0 else empty
    if trim > 0:                                              # test.py:48-56
        xt, xg = xt[:, :-trim], xg[:, :-trim]
    logits = [m.eval()(xh, xt, xg) for m in models]           # test.py:58-64; the softmaxes happen inside the kernel
    label = None
    if with_metrics:
        label = batch["label"][:, :xt.shape[1]].to(xt.device, non_blocking=True)
    scores, rank, live, metrics = ops.ensemble_rank(logits, empty, label)
    return (scores, rank, live, metrics) if with_metrics else (scores, rank, live)


@torch.no_grad()
def predict_ranked_compact(models, batch, with_metrics=False, force_compact=False, history=False):
    """predict_ranked() on ragged candidate lists, same return contract: (scores [B, T'] fp32, rank [B, T'] int32, live [B] int32
    [, metrics [B, 3]]).  The padded candidates of one impression all have the same inputs and therefore the same logit, so each
    impression sends its ``n_b`` live candidates plus -- where it keeps ``e'_b > 0`` padded columns after the common trim -- ONE
    representative padded candidate through the models (``N = sum_b (n_b + [e'_b > 0])`` rows instead of ``B * T'``), and the
    ragged scoring tail lets that candidate's ``exp`` enter the first softmax ``e'_b`` times (``compact.compact_scores_reference``).
    The scores agree with predict_ranked's to fp32 rounding of the logits, not bitwise; ranks of nearly tied scores may differ.

    The plan is built on the host from ``empty_num`` where it lives: a DataLoader's CPU tensor costs no device synchronisation and
    one pinned upload of the index tables; a device-resident ``empty_num`` costs ONE synchronise (its copy to the host).
    A batch in which no row keeps padding after the trim (``N = B * T'``) is handed to predict_ranked itself -- the choice is
    made from the input; ``force_compact`` keeps the ragged kernels even then (tests, measurements).  The gather launch checks
    that the kept padded rows of every impression are bitwise alike and raises ``ops.pad_error_flag`` otherwise:
    ``ops.check_pad_errors(device)`` turns it into a ValueError (score_dataset does after its last batch).
    Inference only; a model whose attention arithmetic is bf16 / bf16x3 is refused (RuntimeError).

    ``history=True`` drops the trailing all-zero history rows as well: one kernel measures every impression's
    history length ``L_b`` on the device, ONE device-to-host copy of those ``B`` integers (the one synchronisation per batch this
    costs) feeds ``build_plan(..., history_len=, H=)``, and the models see ``L_b + [L_b < H]`` history rows per impression -- the
    live ones and one representative padded row that the pool counts ``H - L_b`` times.  The scores agree with ``history=False``
    to fp32 rounding of the logits.  A batch whose histories are all full (``plan.history_dense``) continues exactly as
    ``history=False`` would, the hand-over of an unpadded batch to predict_ranked included: the caller has then paid the length
    kernel and the synchronise for nothing.  A batch with full candidate lists but short histories stays on the ragged path."""
    from . import compact
    xh, xt, xg = batch["x_history"], batch["x_target"], batch["x_global"]
    ops._require_gpu(xh, xt, xg)
    hist_len = None
    if history and xh.dim() == 3 and xh.shape[0] * xh.shape[1] > 0:
        hist_len = ops.history_len(xh).cpu().numpy()             # the one device-to-host copy (and synchronise) of the history path
        if bool((hist_len >= xh.shape[1]).all()):
            hist_len = None                                      # history_dense: exactly the history=False call from here on
    plan = compact.build_plan(batch["empty_num"], xt.shape[1], history_len=hist_len, H=xh.shape[1] if hist_len is not None else None)
    if plan.B != xt.shape[0]:
        raise ValueError(f"predict_ranked_compact: empty_num has {plan.B} entries for {xt.shape[0]} impressions")
    if plan.N == 0 or (plan.dense and not force_compact and hist_len is None):
        return predict_ranked(models, batch, with_metrics=with_metrics)
    tabs = plan.upload(xt.device)
    xt_c, xg_c = ops.compact_gather(xt, xg, tabs["cand_off"], tabs["pad_mult"], plan.trim, plan.N)
    if hist_len is not None:
        xh = ops.history_gather(xh, tabs["hist_off"], plan.R, plan.k_max)
    logits = [m.eval().forward_compact(xh, xt_c, xg_c, plan) for m in models]
    label = None
    if with_metrics:
        label = batch["label"][:, :plan.Tp].to(xt.device, non_blocking=True)
    scores, rank, live, metrics = ops.ensemble_rank_ragged(logits, tabs["cand_off"], tabs["pad_mult"], label, plan.Tp)
    return (scores, rank, live, metrics) if with_metrics else (scores, rank, live)


@torch.no_grad()
def validate_ranked(models, batches, compact=False, compact_history=False):
    """``compact`` / ``compact_history``: score through predict_ranked_compact (``history=compact_history``; the latter implies the
    former) -- the per-epoch validation scores the same padded layout as the test set.  Defaults: the dense path, as before.
    validate() with the ranking metrics: {"auc", "top1", "mrr", "ndcg5", "ndcg10"}, means over the impressions of an iterable
    of device batches (with labels).  AUC and top-1 come from ``row_auc`` on predict_ranked's scores; the sums are kept on the
    device in float64 and read once at the end (one synchronise), where a single-class row raises validate()'s ValueError."""
    dev = next(models[0].parameters()).device
    sums = torch.zeros(6, dtype=torch.float64, device=dev)   # auc, top1, rr, ndcg5, ndcg10, rows with a single class
    n = 0
    for batch in batches:
        if compact or compact_history:
            scores, _rank, live, metrics = predict_ranked_compact(models, batch, with_metrics=True, history=compact_history)
        else:
            scores, _rank, live, metrics = predict_ranked(models, batch, with_metrics=True)
        label = batch["label"][:, :scores.shape[1]].to(scores.device)
        auc, top1 = row_auc_top1(scores, label, live)
        per_row = torch.cat([auc[:, None].double(), top1[:, None].double(), metrics.double(), (auc < 0)[:, None].double()], dim=1)
        sums += per_row.sum(0)
        n += scores.shape[0]
    ops.check_index_errors(dev)                               # (the one synchronise; the flag of the MODELS' device)
    out = sums.tolist()
    if out[5] > 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return {k: v / max(n, 1) for k, v in zip(("auc", "top1", "mrr", "ndcg5", "ndcg10"), out)}


def prediction_lines(impression_ids, rank, live):
    """The text of test.py:124-130 for a batch: ``"{int(impression_id)} [{r1},{r2},...]\\n"`` per row with the row's first
    ``live[b]`` ranks, no spaces.  Host arrays or device tensors; ranks, live counts and ids on a device are gathered into ONE
    device-to-host copy."""
    import numpy as np
    if isinstance(rank, torch.Tensor) and rank.is_cuda:
        B, T = rank.shape
        parts = [rank.reshape(-1).to(torch.int64), torch.as_tensor(live).to(rank.device, torch.int64).reshape(-1)]
        ids_on_device = isinstance(impression_ids, torch.Tensor) and impression_ids.is_cuda
        if ids_on_device:
            parts.append(impression_ids.to(torch.int64).reshape(-1))
        host = torch.cat(parts).cpu().numpy()                 # the one D2H copy
        rank, live = host[:B * T].reshape(B, T), host[B * T:B * T + B]
        if ids_on_device:
            impression_ids = host[B * T + B:]
    rank = np.asarray(rank.cpu() if isinstance(rank, torch.Tensor) else rank)
    live = np.asarray(live.cpu() if isinstance(live, torch.Tensor) else live).astype(np.int64).reshape(-1)
    ids = np.asarray(impression_ids.cpu() if isinstance(impression_ids, torch.Tensor) else impression_ids).reshape(-1)
    if rank.ndim != 2 or len(live) != rank.shape[0] or len(ids) != rank.shape[0]:
        raise ValueError(f"prediction_lines: {len(ids)} ids, rank {rank.shape}, {len(live)} live counts do not agree")
    if len(live) and (live.min() < 0 or live.max() > rank.shape[1]):
        raise ValueError("prediction_lines: a live count lies outside [0, T]")
    rows = rank.tolist()
    return "".join(f"{int(i)} [{','.join(map(str, r[:k]))}]\n" for i, r, k in zip(ids.tolist(), rows, live.tolist()))


def write_predictions(path, impression_ids, rank, live, append=False):
    """test.py:106-110,124-130: write (or append) one line per impression to ``path``; returns the number of lines."""
    text = prediction_lines(impression_ids, rank, live)
    with open(path, "a" if append else "w", encoding="utf-8") as f:
        f.write(text)
    return text.count("\n")


def zip_predictions(txt_path, zip_path):
    """test.py:113-115: one deflated member named by the text file's base name."""
    import os
    import zipfile
    with zipfile.ZipFile(zip_path, "w", zipfile.ZIP_DEFLATED) as z:
        z.write(txt_path, arcname=os.path.basename(txt_path))
    return zip_path


def iter_dataset_batches(head_path, batch_size):
    """Batches of a processed test set in FILE order (DataLoader(shuffle=False), test.py:33), streamed: one subvolume is held
    at a time, a batch may straddle two of them, the last one may be short."""
    from . import data_io
    n_sub, total = data_io.import_processed_data(head_path)[:2]
    pending, seen = [], 0
    for rec in data_io._iter_subvolumes(head_path, n_sub):
        if seen >= total:
            break
        pending.append(rec)
        seen += 1
        if len(pending) == batch_size:
            yield data_io.collate(pending)
            pending = []
    if pending:
        yield data_io.collate(pending)


def score_dataset(models, head_path, out_dir, batch_size=80, name="predictions", compact=False, compact_history=False):
    """test.py's ``model_test`` + ``write_submission_file`` for a processed test set: -> path of ``<out_dir>/<name>.zip`` holding
    ``predictions.txt``.  Every batch goes through predict_ranked (ranks computed on the device) and write_predictions (one
    device-to-host copy); nothing but the current batch and subvolume is held.
    ``compact=True`` scores through predict_ranked_compact (no forward work on padded candidates); a batch whose padded rows are not
    all alike raises ValueError after the last batch.  The default stays the dense path: the two are two correct fp32 evaluations
    whose nearly tied scores may rank differently, so which one writes a submission is the caller's decision.
    ``compact_history=True`` implies the compact path and drops the padded history rows as well (predict_ranked_compact's
    ``history=True``: one more synchronise per batch)."""
    compact = compact or compact_history
    import os
    dev = next(models[0].parameters()).device
    os.makedirs(out_dir, exist_ok=True)
    txt_path = os.path.join(out_dir, "predictions.txt")
    open(txt_path, "w").close()
    for batch in iter_dataset_batches(head_path, batch_size):
        tb = {k: torch.from_numpy(batch[k]).to(dev, non_blocking=True) for k in ("x_history", "x_target", "x_global")}
        tb["empty_num"] = torch.from_numpy(batch["empty_num"])         # stays on the host: the trim costs no synchronisation
        if compact:
            _scores, rank, live = predict_ranked_compact(models, tb, history=compact_history)
        else:
            _scores, rank, live = predict_ranked(models, tb)
        write_predictions(txt_path, batch["impression_id"], rank, live, append=True)
    ops.check_index_errors(dev)
    if compact:
        ops.check_pad_errors(dev)
    return zip_predictions(txt_path, os.path.join(out_dir, f"{name}.zip"))


def save_checkpoint(model, path):
    """train.py:95-97: the state_dict without the per-user bias ``delta``."""
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k != "delta"}
    torch.save(sd, path)


def load_checkpoint(model, path):
    """test.py:160: load_state_dict(strict=False); only tensors are read from the file (weights_only)."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return model.load_state_dict(sd, strict=False)


# ------------------------------------------------------------------------------------------------ table-fed evaluation
def scoring_plan(empty_num, N, B, T):
    """The steps of a pass over ``N`` impressions in batches of ``B``, from the producer's ``empty_num`` IN PASS ORDER (host, [N]) ->
    [(n, Tp)] per step: n = impressions of the step, Tp = T - min over the step of empty_num -- the width the reference's common trim
    leaves (test.py:48-56), which decides the batch's scores.  Pure host arithmetic; no device."""
    import numpy as np
    e = np.asarray(empty_num, dtype=np.int64).reshape(-1)
    N, B, T = int(N), int(B), int(T)
    if e.shape[0] != N or B < 1 or T < 1:
        raise ValueError(f"scoring_plan: {e.shape[0]} entries of empty_num for N={N}, B={B}, T={T}")
    plan = []
    for lo in range(0, N, B):
        part = e[lo:lo + B]
        tp = T - int(part.min())
        if not 1 <= tp <= T:
            raise ValueError(f"scoring_plan: the batch at impression {lo} would be trimmed to {tp} of {T} candidate columns "
                             "(empty_num lies outside [0, T) for every one of its impressions)")
        plan.append((int(part.shape[0]), tp))
    return plan


class GraphedTableScoring:
    """A validation or scoring pass over device-resident tables whose steady state is ONE graph replay per batch: no
    upload, no other launch from the host and no host read until the pass ends (or the record is drained).

    The captured step is ``assemble_batch_at`` -> the slice to ``Tp`` columns -> every model's eval-mode forward -> ``ensemble_rank`` ->
    ``row_auc`` (with labels) -> ``eval_tally``.  The reference trims the padding common to a batch BEFORE the first softmax
    (test.py:48-56), so a batch's width ``Tp`` changes its scores; the producer knows ``empty_num`` of every impression on the host and a
    pass runs in a fixed order, so every batch's ``Tp`` is known before the pass starts (``scoring_plan``) and there is one graph per
    distinct ``Tp`` -- at most ``max_graphs``, least recently used first out, all in one memory pool, all reading the one cursor, the one
    ``order`` buffer and the one state buffer.  Inside a graph the shapes are the eager call's (``predict_ranked`` over a ``TableLoader``
    batch), so the logits are the eager path's.  A last partial batch runs eagerly through the same ops at its own size.

    Weights may change between passes; the rule is GraphedPredict's (``_WeightsWatch``): new addresses or a new packed-weight generation
    drop the graphs, new version counters re-pack the images in place before the first replay.

    The tally keeps the five metric sums, the counts and a ring of ``record_rows`` rows (ranks, live counts, impression ids) in ONE state
    buffer.  ``record_rows`` None: the whole pass, read once at its end; lower: the host drains the ring every ``record_rows``
    impressions -- one read per drain.  The partial batch has a record of its own size behind the ring (a step's rows divide the ring it
    writes), read with the last read."""

    def __init__(self, models, tables, batch_size, H, T, keep_target_slot, with_labels=True, record_rows=None, max_graphs=16, compact=False,
                 compact_history=False):
        import torch.distributed as dist
        from . import native
        from .tables import TABLE_FIELDS
        if compact or compact_history:
            raise RuntimeError("GraphedTableScoring(compact=True / compact_history=True): the ragged forms are planned on the host for every batch; "
                               "a captured step replays one fixed sequence of launches.  Capture the dense pass, or run the eager one "
                               "(validate_ranked(..., compact=True) over a TableLoader)")
        if native.kernel_events is not None:
            raise RuntimeError("per-kernel event timing cannot be recorded inside a graph capture")
        if dist.is_available() and dist.is_initialized():
            raise RuntimeError("GraphedTableScoring: a process group is initialised; sharding the tables' impressions over ranks is not built "
                               "(every rank would score the whole pass).  Run it in a process without a group")
        self.models = list(models)
        if not 1 <= len(self.models) <= 8:
            raise RuntimeError(f"GraphedTableScoring: {len(self.models)} models; the scoring tail (ensemble_rank) takes 1 .. 8")
        if int(batch_size) < 1 or int(max_graphs) < 1:
            raise ValueError(f"GraphedTableScoring(batch_size={batch_size}, max_graphs={max_graphs})")
        self.batch_size, self.H, self.T, self.keep_target_slot = int(batch_size), int(H), int(T), bool(keep_target_slot)
        self.with_labels, self.max_graphs = bool(with_labels), int(max_graphs)
        self.N = tables.n_impressions
        if self.N < 1:
            raise ValueError("GraphedTableScoring: the tables hold no impression")
        B = self.batch_size
        whole = (self.N + B - 1) // B * B
        cap = whole if record_rows is None else int(record_rows)
        if cap < B or cap % B:
            raise ValueError(f"GraphedTableScoring(record_rows={record_rows}): a positive multiple of batch_size={B}")
        self.cap, self.tail = min(cap, whole), self.N % B
        dev = next(self.models[0].parameters()).device
        self.tables = tables if tables.is_device else tables.to(dev)
        self._tabs = [getattr(self.tables, name) for name in TABLE_FIELDS]
        self.empty_all = self.tables.host.empty_num_all(self.T, self.keep_target_slot)
        self.order = torch.zeros(self.N, dtype=torch.int64, device=dev)
        self._order_host = torch.zeros(self.N, dtype=torch.int64).pin_memory()
        # ONE buffer of 8-byte words: cursor | sums [5] float64 | counts [4] | ring: id [cap], live [cap] int32, rank [cap, T] int32 | the
        # same three for the partial batch
        words = lambda n_int32: (n_int32 + 1) // 2      # noqa: E731
        at, self._at = 10, {}
        for name, rows in (("ring", self.cap), ("tail", self.tail)):
            self._at[name] = (at, at + rows, at + rows + words(rows))
            at += rows + words(rows) + words(rows * self.T)
        self.state = torch.zeros(at, dtype=torch.int64, device=dev)
        self.cursor, self.counts = self.state[0:1], self.state[6:10]
        self.sums = self.state[1:6].view(torch.float64)
        self._rec = {name: self._views(self.state, name) for name in ("ring", "tail") if self._rows(name)}
        ops.index_error_flag(dev)                               # (pinned: allocated before any capture)
        self.graphs, self._pool = {}, None
        self._weights = _WeightsWatch(self.models)
        self.replays = self.eager_steps = self.captures = self.host_reads = 0

    def _rows(self, name):
        return self.cap if name == "ring" else self.tail

    def _views(self, state, name):
        """(rank [rows, T] int32, live [rows] int32, id [rows] int64) of the ring or the partial batch's record inside a state buffer"""
        rows, (a_id, a_live, a_rank) = self._rows(name), self._at[name]
        as32 = state.view(torch.int32) if isinstance(state, torch.Tensor) else state.view("int32")
        return (as32[2 * a_rank:2 * a_rank + rows * self.T].reshape(rows, self.T), as32[2 * a_live:2 * a_live + rows], state[a_id:a_id + rows])

    def _step_ops(self, n, Tp, rec):
        """one step of ``n`` impressions at the cursor, scored at ``Tp`` columns: the SAME ops eagerly and inside a capture"""
        from .tables import BATCH_KEYS
        batch = dict(zip(BATCH_KEYS, ops.assemble_batch_at(self._tabs, self.order, self.cursor, n, self.H, self.T, self.keep_target_slot,
                                                           int(self.tables.static_cols))))
        xh, xt, xg, empty = batch["x_history"], batch["x_target"], batch["x_global"], batch["empty_num"]
        trim = self.T - Tp
        if trim > 0:                                            # test.py:48-56, decided by the plan instead of a device read
            xt, xg, empty = xt[:, :-trim], xg[:, :-trim], empty - trim
        logits = [m(xh, xt, xg) for m in self.models]
        label = batch["label"][:, :Tp] if self.with_labels else None
        scores, rank, live, metrics = ops.ensemble_rank(logits, empty, label)
        auc = top1 = None
        if self.with_labels:
            auc, top1 = ops.row_auc(scores, label, live)
        ops.eval_tally(auc, top1, metrics if self.with_labels else None, rank, live, batch["impression_id"], self.cursor, self.sums,
                       self.counts, rec[0], rec[1], rec[2], self.N)

    def _capture(self, Tp):
        """the graph of a full batch at width ``Tp``, built as GraphedPredict builds its own: two warm-up steps on a side stream (allocator,
        packed weight images) -- which move the cursor and the sums, so the head of the state is put back -- then the capture"""
        dev = self.order.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            head = self.state[:10].clone()
            for _ in range(2):
                self._step_ops(self.batch_size, Tp, self._rec["ring"])
                self.state[:10].copy_(head)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=self._pool):
            self._step_ops(self.batch_size, Tp, self._rec["ring"])
        if self._pool is None:
            self._pool = graph.pool()
        while len(self.graphs) >= self.max_graphs:
            self.graphs.pop(next(iter(self.graphs)))
        self._weights.refresh()                                 # (the warm-up may have created the packed images)
        self.captures += 1
        return graph

    def _read(self):
        self.host_reads += 1
        return self.state.cpu().numpy()                         # (waits for the stream)

    @torch.no_grad()
    def run(self, order=None):
        """One pass in ``order`` (host, [N]; None: file order) -> dict(auc, top1, mrr, ndcg5, ndcg10 -- means over the pass, absent without
        labels --, impressions, steps, one_class_rows, no_positive_rows, impression_id [N], rank [N, T], live [N]: host arrays in pass
        order).  A single-class row raises validate_ranked's ValueError, an out-of-range index IndexError, both at the last read."""
        import numpy as np
        from . import native
        if native.kernel_events is not None:
            raise RuntimeError("per-kernel event timing cannot be recorded inside a graph capture")
        N, B, T, cap = self.N, self.batch_size, self.T, self.cap
        order = np.arange(N, dtype=np.int64) if order is None else np.ascontiguousarray(order, dtype=np.int64)
        if order.shape != (N,):
            raise ValueError(f"GraphedTableScoring.run: order {order.shape} for {N} impressions")
        plan = scoring_plan(self.empty_all[order], N, B, T)
        for m in self.models:
            m.eval()
        if self._weights.check(bool(self.graphs)):
            self.graphs.clear()                                 # captured addresses are gone: capture again
            self._pool = None
        self._order_host.copy_(torch.from_numpy(order))
        self.order.copy_(self._order_host, non_blocking=True)
        self.state.zero_()
        ids, rank, live = np.zeros(N, dtype=np.int64), np.zeros((N, T), dtype=np.int32), np.zeros(N, dtype=np.int32)

        def take(host, name, lo, hi):
            r_rank, r_live, r_id = self._views(host, name)
            at = np.arange(lo, hi) % self._rows(name)
            ids[lo:hi], rank[lo:hi], live[lo:hi] = r_id[at], r_rank[at], r_live[at]

        done = drained = 0
        for i, (n, Tp) in enumerate(plan):
            if n == B:
                graph = self.graphs.pop(Tp, None)
                if graph is None:
                    graph = self._capture(Tp)
                self.graphs[Tp] = graph                         # (re-inserted last: most recently used)
                graph.replay()
                self.replays += 1
            else:
                self._step_ops(n, Tp, self._rec["tail"])
                self.eager_steps += 1
            done += n
            if n == B and done - drained == cap and i + 1 < len(plan) and plan[i + 1][0] == B:
                take(self._read(), "ring", drained, done)      # the ring is full and another full batch follows: drain it
                drained = done
        host = self._read()
        ops.check_index_errors(self.order.device)
        full = N - self.tail
        take(host, "ring", drained, full)
        if self.tail:
            take(host, "tail", full, N)
        sums, counts = host[1:6].view(np.float64), host[6:10]
        if int(host[0]) != N or int(counts[3]) != N or int(counts[2]) != len(plan):
            raise RuntimeError(f"GraphedTableScoring.run: the device record holds {int(counts[3])} impressions in {int(counts[2])} steps, cursor "
                               f"{int(host[0])}; the pass has {N} in {len(plan)}")
        out = {"impressions": N, "steps": len(plan), "one_class_rows": int(counts[0]), "no_positive_rows": int(counts[1]),
               "impression_id": ids, "rank": rank, "live": live}
        if self.with_labels:
            if counts[0] > 0:
                raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
            out.update({k: float(v) / N for k, v in zip(("auc", "top1", "mrr", "ndcg5", "ndcg10"), sums.tolist())})
        return out


def validate_tables(models, tables, batch_size=80, *, H, T, keep_target_slot=True, graph=True, runner=None):
    """reference train.py:107-110 / verify.py:19-43 over a validation set that lives on the device as ``ImpressionTables``, in file order
    -> validate_ranked's dict {"auc", "top1", "mrr", "ndcg5", "ndcg10"}.  ``graph=True``: one ``GraphedTableScoring`` pass (``runner``: one
    built earlier for these models and tables, whose graphs are then reused); ``graph=False``: ``validate_ranked`` over a ``TableLoader``."""
    if not graph:
        from .tables import TableLoader
        dev = next(models[0].parameters()).device
        return validate_ranked(models, TableLoader(tables, batch_size, H, T, shuffle=False, keep_target_slot=keep_target_slot, device=dev))
    if runner is None:
        runner = GraphedTableScoring(models, tables, batch_size, H, T, keep_target_slot)
    got = runner.run()
    return {k: got[k] for k in ("auc", "top1", "mrr", "ndcg5", "ndcg10")}


def score_tables(models, tables, out_dir, batch_size=80, *, H, T, keep_target_slot=False, name="predictions", graph=True, record_rows=None):
    """test.py's ``model_test`` + ``write_submission_file`` for a test set that lives on the device as ``ImpressionTables`` (no labels needed)
    -> path of ``<out_dir>/<name>.zip`` holding ``predictions.txt``, in file order.  ``graph=True``: a ``GraphedTableScoring`` pass without
    labels whose ranks stay in the device record until it is drained (``record_rows``: impressions per drain; None: the whole pass, one
    host read); ``graph=False``: predict_ranked + write_predictions per ``TableLoader`` batch (one device-to-host copy each)."""
    import os
    os.makedirs(out_dir, exist_ok=True)
    txt_path = os.path.join(out_dir, "predictions.txt")
    if graph:
        got = GraphedTableScoring(models, tables, batch_size, H, T, keep_target_slot, with_labels=False, record_rows=record_rows).run()
        write_predictions(txt_path, got["impression_id"], got["rank"], got["live"])
    else:
        from .tables import TableLoader
        dev = next(models[0].parameters()).device
        open(txt_path, "w").close()
        for batch in TableLoader(tables, batch_size, H, T, shuffle=False, keep_target_slot=keep_target_slot, device=dev):
            _scores, rank, live = predict_ranked(models, batch)
            write_predictions(txt_path, batch["impression_id"], rank, live, append=True)
        ops.check_index_errors(dev)
    return zip_predictions(txt_path, os.path.join(out_dir, f"{name}.zip"))


def sweep_checkpoints(paths, model, tables, batch_size=80, *, H, T, keep_target_slot=True, graph=True):
    """reference verify.py:53-75: every checkpoint of ``paths`` loaded into the SAME ``model`` (``load_checkpoint``) and validated over the
    tables -- through ONE ``GraphedTableScoring`` where ``graph``, so the graphs captured for the first checkpoint serve them all and only
    the packed weight images are refreshed -> {"results": [validate_tables' dict per path], "best": the path with the highest AUC, "best_auc"}.
    Ties go to the later path: the reference compares with ``>=``."""
    runner = GraphedTableScoring([model], tables, batch_size, H, T, keep_target_slot) if graph else None
    results, best, best_auc = [], None, -1.0
    for path in paths:
        load_checkpoint(model, path)
        got = validate_tables([model], tables, batch_size, H=H, T=T, keep_target_slot=keep_target_slot, graph=graph, runner=runner)
        results.append(got)
        if got["auc"] >= best_auc:
            best, best_auc = path, got["auc"]
    return {"results": results, "best": best, "best_auc": best_auc}
