"""The training step of reference train.py:66-75 and its data-parallel extension.

    out  = model(x_history, x_inview, x_global)          train.py:69
    loss = model.loss(user_id, out, label)               train.py:71
    loss.backward(); optimizer.step(); optimizer.zero_grad()      train.py:73-75

Data parallel (new): one process per GPU, every rank takes B/N impressions, and ONE
all-reduce (RCCL over xGMI; gloo in the CPU tests) of a single flat fp32 gradient buffer sits between
backward and the Adam step.  BatchNorm statistics stay per replica.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from .config import Dims, model_config


def build_model(dims: Dims, user_num: int, state_dict=None, device="cuda", attention_mma=None):
    """Construct a UserModel with the given dims (re-dimensions ``model_config`` the way the
    reference is re-dimensioned: dims are read at construction).  ``attention_mma`` ('f32' | 'bf16') pins the
    arithmetic of both attentions' contraction on this model (None: the process default, fp32)."""
    from .modules import UserInvariantInterestModel, UserModel
    saved = dict(model_config)
    saved_defaults = UserInvariantInterestModel.__init__.__defaults__
    try:
        model_config["pca_vector"] = dims.pca_vector
        model_config["category_label_num"] = dims.category_label_num
        UserInvariantInterestModel.__init__.__defaults__ = (list(dims.embed_setting),)
        model = UserModel(user_num)
    finally:
        model_config.update(saved)
        UserInvariantInterestModel.__init__.__defaults__ = saved_defaults
    if state_dict is not None:
        model.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict.items()}, strict=False)
    if attention_mma is not None:
        from . import ops
        ops.resolve_mma(attention_mma)                        # validates the name
        model.invariant_interest_model.label_attention.mma = attention_mma
        model.invariant_interest_model.text_img_attention.mma = attention_mma
    return model.to(device)


def make_optimizer(model, lr=1e-3):
    """train.py:48 -- Adam(lr, weight_decay=1e-5), L2 folded into the gradient."""
    return torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-5)


class FlatAdam:
    """train.py:48's Adam(lr, weight_decay=1e-5) over ONE flat fp32 buffer.

    Parameters are re-seated as views into one flat buffer (values are preserved, the Module's ``state_dict`` keeps
    working).  ``loss.backward()`` leaves every parameter's gradient where autograd produced it (``p.grad`` starts as
    None, so AccumulateGrad adopts the tensor instead of launching an ``add_`` per parameter); ``collect_grads()`` then
    gathers all of them into ``flat_grad`` with ONE launch (C ABI ``nrm_gather_flat``), the data-parallel all-reduce runs on
    that buffer without a copy, and ``step()`` is one fused Adam launch over all weights."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5):
        import ctypes
        from . import native
        native.load()
        self.params = [p for p in model.parameters() if p.requires_grad]
        if not self.params or not self.params[0].is_cuda:
            raise RuntimeError("FlatAdam needs the model on an MI355X device (no CPU path)")
        dev = self.params[0].device
        offs, n = [], 0
        for p in self.params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4                      # every parameter starts 16-byte aligned
        self.n = n
        self.offsets = offs
        self.flat_param = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, offs):
            view = self.flat_param[o:o + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad = None
        k = len(self.params)
        self._srcs = (ctypes.c_void_p * k)()
        self._offs = (ctypes.c_long * k)(*offs)
        self._cnts = (ctypes.c_long * k)(*[p.numel() for p in self.params])
        self._collected = False
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        # {step, 1-b1^step, sqrt(1-b2^step), -} lives on the device: the step is graph-capturable
        self.state = torch.zeros(4, dtype=torch.float32, device=dev)
        self.param_groups = [{"lr": lr}]                       # what train.py:57 reads
        self.collective_events = None                          # a list: all_reduce_grads appends an event pair per call (bench.py)

    @property
    def nbytes(self):
        return self.n * 4

    @property
    def steps(self):
        return int(self.state[0].item())

    def grad_view(self, p_index):
        """The slot of parameter ``p_index`` in ``flat_grad`` (valid after ``collect_grads()``)."""
        p, o = self.params[p_index], self.offsets[p_index]
        return self.flat_grad[o:o + p.numel()].view_as(p)

    def collect_grads(self):
        """All ``p.grad`` -> ``flat_grad`` (a parameter without a gradient contributes zeros), one launch; the per-parameter
        gradient tensors are released.  Idempotent until the next ``step()`` / ``zero_grad()``."""
        if self._collected:
            return
        from . import native, ops
        ops.verify_deferred_targets(self.params)   # a deferred reduction whose buffer autograd copied away would be lost: raise
        ops.flush_slab_reductions()                # weight gradients whose slab reduction train_step deferred become valid here
        keep = []
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                self._srcs[i] = None
                continue
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.to(torch.float32).contiguous()
            keep.append(g)
            self._srcs[i] = g.data_ptr()
        native.call("nrm_gather_flat", self._srcs, self._offs, self._cnts, len(self.params), native.ptr(self.flat_grad), self.n,
                    native.stream_ptr())
        for p in self.params:
            p.grad = None
        self._collected = True

    def step(self, zero_grad=True):
        from . import ops
        self.collect_grads()
        ops.adam_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.state,
                      float(self.param_groups[0]["lr"]), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                      float(self.weight_decay), bool(zero_grad))          # torch.ops.nrm.adam_step -> nrm_adam_step_dev
        # the weights moved (through a raw pointer: no autograd version bump): every cached packed GEMM operand is
        # refreshed by ONE launch instead of one per GEMM call of the next step
        ops.repack_persistent(self.params)
        self._collected = False

    def zero_grad(self, set_to_none=False):
        for p in self.params:
            p.grad = None
        self.flat_grad.zero_()
        self._collected = False

    def all_reduce_grads(self, group=None):
        """The ONE collective of a data-parallel step: sum the flat gradient over ranks, then average."""
        self.collect_grads()
        if not dist.is_initialized():
            return
        # issued whenever a process group exists, also for a group of one (bench.py's NRM_DIST_WORLD1 rehearsal of RCCL)
        world = dist.get_world_size(group)
        timed = self.collective_events is not None and not torch.cuda.is_current_stream_capturing()
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if dist.get_backend(group) == "nccl":
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.AVG, group=group)      # RCCL averages in the collective
        else:
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=group)
            if world > 1:
                self.flat_grad.mul_(1.0 / world)
        if timed:
            e1.record()
            self.collective_events.append((e0, e1))


class FlatGradReducer:
    """Averages the gradients of ``params`` across ranks with ONE all-reduce of a flat fp32 buffer."""

    def __init__(self, params, group=None):
        self.params = [p for p in params if p.requires_grad]
        self.group = group
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device if self.params else "cpu"
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.views, off = [], 0
        for p in self.params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            off += p.numel()

    @property
    def nbytes(self):
        return self.flat.numel() * 4

    def reduce(self):
        world = dist.get_world_size(self.group) if dist.is_initialized() else 1
        if world == 1:
            return
        for p, v in zip(self.params, self.views):
            if p.grad is None:
                v.zero_()
            else:
                v.copy_(p.grad)
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        self.flat.mul_(1.0 / world)
        for p, v in zip(self.params, self.views):
            if p.grad is None:
                p.grad = v.clone()
            else:
                p.grad.copy_(v)


class IndexErrorWatch:
    """Out-of-range ids without a host sync.  The kernels clamp a bad table index / user id and set a flag (the reference raises
    IndexError at the offending batch: F.embedding at models/user_invariant_interest_model.py:59, delta[id] at
    models/user_model.py:40).  The flag lives in pinned host memory the device writes directly (ops.index_error_flag), so
    ``before_step()`` just reads it: the error surfaces at the start of the step after the offending batch when the device keeps
    up with the host, and ``max_lag`` + 1 steps after it at the latest (``after_step()`` records an event per step and
    ``before_step()`` waits for the one that is ``max_lag`` steps old) -- not at the epoch's end, and at no cost per step beyond
    one event record.

    What this is NOT: the reference raises BEFORE any update; here the offending batch's step (computed with the clamped ids) and
    up to ``max_lag`` following steps have already been applied to the weights, both Adam moments and ``delta`` when the
    exception arrives -- the exception says so.  A caller that must not train on a bad batch uses the strict mode instead
    (``train_step(..., strict_ids=True)`` / ``validate_batch_ids``: ids checked on the device before the step is enqueued, one
    host synchronisation per step).  When the flag is found raised, every step still in flight is waited for BEFORE the flag is
    cleared, so a step enqueued earlier cannot raise it again for an unrelated later batch."""

    def __init__(self, device, max_lag=2):
        from . import ops
        self.flag = ops.index_error_flag(device)
        self.device = torch.device(device)
        self.max_lag = max_lag
        self.pending = []                                   # one event per enqueued step, oldest first

    def after_step(self):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.pending.append(ev)

    def before_step(self):
        while self.pending and (len(self.pending) > self.max_lag or self.pending[0].query()):
            self.pending.pop(0).synchronize()
        if int(self.flag[0]):
            in_flight = len(self.pending)
            while self.pending:                             # drain: steps still in flight may set the flag again
                self.pending.pop(0).synchronize()
            self.flag.zero_()
            raise IndexError("index out of range (a category / type / time table index of a packed feature row, or a user "
                             f"id outside delta) in a batch of one of the last {in_flight + 1} steps; those steps ran with the "
                             "offending ids clamped and HAVE ALREADY UPDATED the weights, the Adam moments and delta (the "
                             "reference raises before any update: use train_step(..., strict_ids=True) for that behaviour)")


def validate_batch_ids(model, batch):
    """The reference's IndexError BEFORE anything is enqueued (strict mode of train_step): every table index of the packed rows
    (time4 | text_img[P] | category | sub-categories | sentiment | type ...: models/user_invariant_interest_model.py:14-22,58-71)
    and every user id (models/user_model.py:40; negative ids count from the end, as torch indexing does) is range-checked on the
    device; ONE host synchronisation.  The asynchronous default is IndexErrorWatch."""
    if torch.cuda.is_current_stream_capturing():
        # the check ends in ONE host read of a device flag: inside a stream capture that is an error that can take the process
        # down (global capture mode).  A captured step cannot raise per replay anyway: validate before capturing / replaying.
        raise RuntimeError("validate_batch_ids / train_step(strict_ids=True) synchronises with the host and cannot run inside a "
                           "stream capture; validate the batch before the capture (or rely on IndexErrorWatch around replays)")
    inv = model.invariant_interest_model
    d = inv._dims
    P, ns = d.pca_vector, d.n_subcat
    dev = batch["x_history"].device
    tables = torch.tensor([inv.year_embedding[0].num_embeddings, inv.month_embedding[0].num_embeddings,
                           inv.day_embedding[0].num_embeddings, inv.hour_embedding[0].num_embeddings], device=dev)
    n_cat, n_type = inv.category_embedding[0].num_embeddings, inv.type_embedding[0].num_embeddings
    flags = []
    for x in (batch["x_history"], batch["x_target"]):
        if x.numel() == 0:
            continue
        t4 = x[..., :4].long()                                           # the four time-table indices of a row, one comparison
        flags.append(((t4 < 0) | (t4 >= tables)).any())                  # (F.embedding refuses negative indices too)
        ids = x[..., 4 + P:4 + P + 1 + ns].long()                     # category and its sub-category slots share one table
        flags.append(((ids < 0) | (ids >= n_cat)).any())
        typ = x[..., 4 + P + 1 + ns + d.n_sentiment].long()
        flags.append(((typ < 0) | (typ >= n_type)).any())
    n = model.delta.numel()
    uid = batch["user_id"].long()
    flags.append(((uid < -n) | (uid >= n)).any())
    if bool(torch.stack(flags).any()):                                 # the one synchronisation
        raise IndexError("index out of range in self (a category / type / time table index of a packed feature row, or a user id "
                         "outside delta); nothing was enqueued, no weight was updated")


_watches = {}


def _index_watch(device):
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    w = _watches.get(key)
    if w is None:
        w = _watches[key] = IndexErrorWatch(device)
    return w


_len_streams = {}


def history_len_host(x_history, after=None):
    """``L_b`` of a device-resident ``x_history`` [B, H, cols] as a HOST int32 tensor (pinned), measured by ``ops.history_len`` on a side
    stream that waits for ``after`` (an event: the batch's own upload) or, without one, for what the current stream holds now.  Returns
    (host tensor, event): the lengths are valid once the event has completed -- the compute stream is never drained for them."""
    from . import ops
    dev = x_history.device
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    side = _len_streams.get(key)
    if side is None:
        side = _len_streams[key] = torch.cuda.Stream(device=dev)
    if after is not None:
        side.wait_event(after)
    else:
        side.wait_stream(torch.cuda.current_stream(dev))
    host = torch.empty(x_history.shape[0], dtype=torch.int32).pin_memory()
    with torch.cuda.stream(side):
        lens = ops.history_len(x_history)
        host.copy_(lens, non_blocking=True)
        done = torch.cuda.Event()
        done.record(side)
    x_history.record_stream(side)
    return host, done


def attach_history_len(batch, after=None):
    """-> ``batch`` with ``"history_len_host"`` = (host lengths, event, address and version counter of ``x_history``), measured now by
    ``history_len_host``.  The entry is PRIVATE to this module: the lengths describe exactly the tensor contents they were measured on, and
    ``train_step`` uses them only while ``x_history`` still has that address and version counter -- a batch refreshed in place (a
    ``copy_`` into the same buffers) is measured again instead of being planned with stale lengths.  A length anybody else supplies is not
    trusted."""
    xh = batch["x_history"]
    host, done = history_len_host(xh, after)
    return dict(batch, history_len_host=(host, done, xh.data_ptr(), xh._version))


def attach_empty_num(batch, host):
    """-> ``batch`` with ``"empty_num_host"`` = (the HOST copy of ``empty_num`` the batch was staged from, address and version counter of the
    device tensor): ``train_step(compact_candidates=True)`` plans from it without a synchronise, while ``empty_num`` is still that tensor.
    The counts are not trusted either way: the gather kernel checks every dropped cell."""
    dev = batch["empty_num"]
    return dict(batch, empty_num_host=(host, dev.data_ptr(), dev._version))


def attach_known_history_len(batch, lengths):
    """-> ``batch`` with ``"history_len_host"`` filled from HOST lengths the batch's own producer knows (``tables.TableLoader``: the number of
    events it wrote rows for) instead of a measuring kernel and a copy; the entry has the form ``attach_history_len`` gives it and is dropped
    the same way once ``x_history`` is another tensor or has been written to.  A known length can only be >= the measured one (a row the
    producer wrote may be all-zero; a row behind its length never holds a bit), so the rows a plan drops are all-zero and compaction stays
    exact."""
    xh = batch["x_history"]
    host = torch.as_tensor(np.ascontiguousarray(lengths, dtype=np.int32))
    if tuple(host.shape) != (xh.shape[0],) or (host.numel() and (int(host.min()) < 0 or int(host.max()) > xh.shape[1])):
        raise ValueError(f"attach_known_history_len: lengths {tuple(host.shape)} for x_history {tuple(xh.shape)} (one per impression, 0 .. H)")
    return dict(batch, history_len_host=(host, torch.cuda.Event(), xh.data_ptr(), xh._version))     # (an event never recorded: complete)


def attach_known_lengths(batch, history_len, empty_num):
    """``attach_known_history_len`` and ``attach_empty_num`` from the producer's host arrays in one call."""
    return attach_empty_num(attach_known_history_len(batch, history_len), np.ascontiguousarray(empty_num, dtype=np.int64))


def _empty_num_host(batch):
    """``empty_num`` of the batch on the host: the prefetcher's copy where it describes this very tensor, else one ``.cpu()`` (a synchronise)."""
    e = batch["empty_num"]
    pre = batch.get("empty_num_host")
    if pre is not None and hasattr(e, "data_ptr") and (pre[1], pre[2]) == (e.data_ptr(), e._version):
        return pre[0].numpy() if hasattr(pre[0], "numpy") else pre[0]
    return e.detach().cpu().numpy() if hasattr(e, "detach") else e


def _history_plan(batch, max_groups):
    """The length groups of the batch's histories (``compact.plan_history_groups``), from the lengths the prefetcher measured or ones
    measured now."""
    from . import compact
    xh = batch["x_history"]
    pre = batch.get("history_len_host")                      # attach_history_len's entry: valid for the tensor it was measured on only
    if pre is None or (pre[2], pre[3]) != (xh.data_ptr(), xh._version):
        pre = history_len_host(xh)                           # nobody measured THESE rows: measure now, at the cost of a synchronise
    host, done = pre[0], pre[1]
    done.synchronize()                                       # the side stream's copy only -- not the compute stream
    return compact.plan_history_groups(host.numpy(), xh.shape[1], max_groups=max_groups)


def _compact_candidates_forward(model, batch, alpha, max_groups, compact_history):
    """forward + loss of train_step(compact_candidates=True) -> (loss, out [B, T] in the caller's order), or None where the candidate axis
    has nothing worth dropping or the model does not take the row-weight head (the caller then tries compact_history alone, then dense)."""
    from . import compact, ops
    xh, xt = batch["x_history"], batch["x_target"]
    empty = _empty_num_host(batch)
    # first, and before anything that costs host time: can ANY grouping save enough?  (a launch-bound step feels every 10 us spent here)
    if not compact_history and compact.candidate_saving_bound(empty, xt.shape[1]) < compact.MIN_SAVING:
        return None
    if not (hasattr(model, "compact_candidates_applies") and model.compact_candidates_applies()):
        return None
    flag = ops.pad_error_flag(xh.device)
    if int(flag[0]):                                         # raised by an EARLIER step's gather: that step has been applied
        torch.cuda.synchronize(xh.device)
        flag.zero_()
        raise ValueError("train_step(compact_candidates=True): a candidate that empty_num counts as padding differs from the other padded "
                         "candidates of its impression in x_target, x_global or label, in a batch of an earlier step (which ran on the "
                         "compacted rows and HAS BEEN APPLIED); train this data with the dense step")
    hist = _history_plan(batch, max_groups) if compact_history else None
    cand = compact.plan_candidate_groups(empty, xt.shape[1], max_groups=max_groups, history_plan=hist)
    if cand.dense or cand.B == 0:
        return None
    plan = hist if hist is not None else compact.full_height_history_plan(cand, xh.shape[1])
    plan.cand = cand
    tabs, ctabs = plan.upload(xh.device), cand.upload(xh.device)
    perm = tabs["perm"]
    arena = ops.history_gather_groups(xh, perm, tabs["bounds"], tabs["row_off"], tabs["H_g"], plan.R)
    xt_a, xg_a, label_a, roww = ops.candidate_gather_groups(xt, batch["x_global"], batch["label"], perm, tabs["bounds"], ctabs["row_off"],
                                                            ctabs["T_g"], cand.N)
    out_arena = model.forward_grouped(arena, xt_a, xg_a, plan, row_weight=roww)
    loss = model.loss_grouped(batch["user_id"].index_select(0, perm), out_arena, label_a, cand, alpha)
    return loss, out_arena.detach().index_select(0, ctabs["expand"]).view(cand.B, cand.T)


def _compact_forward(model, batch, alpha, max_groups):
    """forward + loss of train_step(compact_history=True) -> (loss, out in the caller's order), or None where the step runs dense: a
    model whose attentions do not take the fused node, or a plan with nothing worth dropping."""
    from . import ops
    if not (hasattr(model, "compact_history_applies") and model.compact_history_applies()):
        return None
    xh = batch["x_history"]
    plan = _history_plan(batch, max_groups)
    if plan.dense or plan.B == 0:
        return None
    tabs = plan.upload(xh.device)
    arena = ops.history_gather_groups(xh, tabs["perm"], tabs["bounds"], tabs["row_off"], tabs["H_g"], plan.R)
    perm = tabs["perm"]
    out_sorted = model.forward_grouped(arena, batch["x_target"].index_select(0, perm), batch["x_global"].index_select(0, perm), plan)
    loss = model.loss(batch["user_id"].index_select(0, perm), out_sorted, batch["label"].index_select(0, perm), alpha)
    return loss, out_sorted.detach().index_select(0, tabs["inverse"])


def _backward_and_step(loss, optimizer, reducer=None, defer_reductions=True):
    """The backward half of a step (train.py:73-75): backward, the gradient collective, the optimizer step, zero_grad."""
    if isinstance(optimizer, FlatAdam):
        from . import ops
        ops.begin_step()                              # (stream ordering of the two attentions' backward contractions: ops._chain)
        # nobody reads a weight gradient between backward() and collect_grads(): the step's slab reductions (one per weight
        # gradient) are recorded during backward and run as ONE launch when FlatAdam gathers the gradients.  A gradient that
        # exists already would be accumulated into before its reduction ran: then (and on request) reductions run at once.
        defer = defer_reductions and all(p.grad is None for p in optimizer.params)
        seed = ops.unit_grad(loss) if loss.dim() == 0 and loss.dtype == torch.float32 else None     # (see ops.unit_grad)
        if defer:
            with ops.deferred_slab_reductions():
                loss.backward(seed)
        else:
            loss.backward(seed)
        optimizer.all_reduce_grads()
        optimizer.step(zero_grad=True)                # Adam + zero_grad fused in one launch
    else:
        loss.backward()
        if reducer is not None:
            reducer.reduce()
        optimizer.step()
        optimizer.zero_grad(set_to_none=False)


def train_step(model, optimizer, batch, reducer: FlatGradReducer | None = None, alpha=0.95, defer_reductions=True,
               strict_ids=False, compact_history=False, max_groups=None, compact_candidates=False):
    """One step of train.py:69-75 on device-resident tensors; returns (loss, out) detached.  An out-of-range id of an EARLIER
    step raises IndexError here, before this step's work is enqueued (IndexErrorWatch: asynchronous, the offending step has
    been applied by then).  ``strict_ids=True``: the ids of THIS batch are checked first (validate_batch_ids, one host
    synchronisation) and the IndexError is raised before anything is enqueued -- the reference's behaviour.
    ``compact_history=True``: the trailing all-zero history rows the ETL pads with are not computed -- the batch is
    sorted by history length, cut into at most ``max_groups`` groups (None: ``compact.MAX_GROUPS``) and every group runs through the dense
    kernels at its own height; loss, BatchNorm statistics and every gradient are the dense step's to fp32 rounding, ``out`` is in the
    caller's order.  The plan needs the lengths on the HOST: what ``BatchPrefetcher(..., history_len=True)`` measured while staging the
    batch (``attach_history_len``; used only while ``x_history`` is the very tensor contents it was measured on) costs nothing here;
    without it the lengths are measured now and this call waits for everything enqueued before it (one synchronise per step).  A plan with nothing worth dropping, and a model whose attentions do not take the fused node, run the dense
    step unchanged.  Not inside a stream capture.
    ``compact_candidates=True``: the padded candidates the ETL fills every list with are not computed either -- the
    batch is sorted by ``T - batch["empty_num"]`` and cut into at most ``max_groups`` groups, each trimmed to its live candidates plus ONE
    padded one whose weight BatchNorm's batch statistics and the loss take; with ``compact_history`` as well the groups are the history
    plan's.  ``empty_num`` is read on the host (``BatchPrefetcher(..., empty_num=True)`` keeps its copy: no synchronise; a device-only
    tensor costs one ``.cpu()``) and CHECKED on the device: a dropped candidate that differs from its impression's padded one raises
    ValueError at the next compacted step.  ``out`` is the full [B, T] in the caller's order.  A plan with nothing worth dropping and a
    model with a BatchNorm or gate the row-weight kernels do not take run as without the flag."""
    if compact_history and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("train_step(compact_history=True) plans the length groups on the host and cannot run inside a stream capture "
                           "(GraphedTrainStep captures the dense step)")
    if compact_candidates:
        if "empty_num" not in batch:
            raise KeyError("empty_num: train_step(compact_candidates=True) needs batch['empty_num'], the trailing padded candidates per "
                           "impression")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("train_step(compact_candidates=True) plans the candidate groups on the host and cannot run inside a stream "
                               "capture (GraphedTrainStep captures the dense step)")
    watch = _index_watch(batch["x_history"].device) if not torch.cuda.is_current_stream_capturing() else None
    if watch is not None:
        watch.before_step()
    if strict_ids:
        validate_batch_ids(model, batch)
    compacted = _compact_candidates_forward(model, batch, alpha, max_groups, compact_history) if compact_candidates else None
    if compacted is None:
        compacted = _compact_forward(model, batch, alpha, max_groups) if compact_history else None
    if compacted is not None:
        loss, out = compacted
    else:
        out = model(batch["x_history"], batch["x_target"], batch["x_global"])
        loss = model.loss(batch["user_id"], out, batch["label"], alpha)
    _backward_and_step(loss, optimizer, reducer, defer_reductions)
    if watch is not None:
        watch.after_step()
    return loss.detach(), out.detach()


class GraphedTrainStep:
    """The whole train.py:69-75 step captured once into a HIP graph and replayed (static shapes, static input
    buffers).  A replay is a single launch instead of ~600: 2-13 % faster than the eager step depending on the shape
    (reference default dimensions: 3.1 -> 2.7 ms).  New data is copied INTO the tensors
    of ``batch`` before ``replay()``; ``loss`` / ``out`` are overwritten in place by every replay."""

    def __init__(self, model, optimizer, batch, alpha=0.95, warmup=3, pool=None, compact_history=False, compact_candidates=False):
        """``pool``: the memory pool of another GraphedTrainStep (``other.graph.pool()``) -- several captured steps, e.g. one per
        resident input batch, then share their intermediates' memory (they must be replayed one at a time, in any order)."""
        if compact_history:
            raise RuntimeError("GraphedTrainStep(compact_history=True): the length groups are planned on the host for every batch; a "
                               "captured step replays one fixed sequence of launches.  Capture the dense step")
        if compact_candidates:
            raise RuntimeError("GraphedTrainStep(compact_candidates=True): the candidate groups are planned on the host for every batch; a "
                               "captured step replays one fixed sequence of launches.  Capture the dense step")
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("GraphedTrainStep needs trainer.FlatAdam (its step counter lives on the device)")
        from . import native
        if native.kernel_events is not None:
            raise RuntimeError("per-kernel event timing cannot be recorded inside a graph capture")
        self.batch = batch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # allocator / lazy-init warm-up outside the capture
            for _ in range(warmup):
                train_step(model, optimizer, batch, None, alpha)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # With a process group the captured step contains the RCCL all-reduce, and ProcessGroupNCCL's watchdog THREAD keeps
        # polling events (hipEventQuery) of earlier collectives: under the default "global" capture mode any such call from
        # another thread while this one captures is an error that takes the process down ("operation not permitted when stream
        # is capturing" -- seen once in five runs of the one-rank RCCL rehearsal).  Thread-local capture mode restricts only the
        # capturing thread; the device is drained first so that no collective of the warm-up steps is still in flight.
        mode = "global"
        if dist.is_available() and dist.is_initialized():
            torch.cuda.synchronize()
            mode = "thread_local"
        with torch.cuda.graph(self.graph, pool=pool, capture_error_mode=mode):
            self.loss, self.out = train_step(model, optimizer, batch, None, alpha)

    def replay(self):
        watch = _index_watch(self.batch["x_history"].device)
        watch.before_step()                                  # an out-of-range id of an earlier replay raises IndexError here
        self.graph.replay()
        watch.after_step()
        return self.loss, self.out


class GraphedTableEpoch:
    """A table-fed epoch whose steady state is ONE graph replay per step: no upload, no other launch from the host
    and no host synchronisation until the epoch ends.

    The captured step is ``assemble_batch_at`` -> ``train_step`` -> ``row_auc`` -> ``epoch_tally``.  The assemble kernel reads its
    impressions at a cursor that lives on the device and the tally moves that cursor by B at the end of the step, so a replay knows which
    batch it is on without the host telling it; the tally also keeps what the eager epoch loops accumulate with ATen launches per step --
    loss * B, the row AUCs, the one-class rows, the per-step loss list of reference train.py:82-94 -- in one packed state buffer that
    the host reads ONCE per epoch.  ``order`` ([N] int64) stays at one address and is refilled in place by ``begin_epoch``.

    Every impression is consumed exactly once and an epoch applies exactly ceil(N / B) optimizer steps (floor with ``drop_last``): the
    allocator warm-up ``GraphedTrainStep`` spends three throwaway steps on is here the first ``warmup`` batches of the FIRST epoch, run
    eagerly through the same ops (cursor and tally stay consistent); then the step is captured -- a capture executes nothing -- and every
    further full batch is a replay.  A last partial batch runs eagerly through the same ops at its own size, so BatchNorm sees the batch
    the eager loop sees.  The learning rate and ``alpha`` are kernel arguments baked into a capture: ``begin_epoch`` re-reads
    ``param_groups[0]['lr']`` as train.py:57 does, and a step whose rate or ``alpha`` differs from the captured one captures again (no
    warm-up steps then: the allocator is warm).  ``warmup >= 1``: capturing a model that has never run would put every lazy
    initialisation of a first step inside the capture."""

    def __init__(self, model, optimizer, tables, batch_size, H, T, keep_target_slot=True, alpha=0.95, warmup=3, compact_history=False,
                 compact_candidates=False):
        if compact_history:
            raise RuntimeError("GraphedTableEpoch(compact_history=True): the length groups are planned on the host for every batch; a "
                               "captured step replays one fixed sequence of launches.  Capture the dense step, or run the eager loop "
                               "(train_epochs_tables(graph=False))")
        if compact_candidates:
            raise RuntimeError("GraphedTableEpoch(compact_candidates=True): the candidate groups are planned on the host for every batch; a "
                               "captured step replays one fixed sequence of launches.  Capture the dense step, or run the eager loop "
                               "(train_epochs_tables(graph=False))")
        who = type(self).__name__
        if not isinstance(optimizer, FlatAdam):
            raise TypeError(f"{who} needs trainer.FlatAdam (its step counter lives on the device)")
        from . import native, ops
        if native.kernel_events is not None:
            raise RuntimeError("per-kernel event timing cannot be recorded inside a graph capture")
        if dist.is_available() and dist.is_initialized():
            raise RuntimeError(f"{who}: a process group is initialised; sharding the tables' impressions over ranks is not built "
                               "(every rank would train the whole epoch).  Run it in a process without a group")
        if int(warmup) < 1:
            raise ValueError(f"{who}(warmup={warmup}): at least one eager step comes before the capture (a model that has never "
                             "run would do its lazy initialisation inside the capture)")
        if int(batch_size) < 1:
            raise ValueError(f"{who}(batch_size={batch_size})")
        from .tables import TABLE_FIELDS
        dev = optimizer.flat_param.device
        self.model, self.optimizer = model, optimizer
        self.tables = tables if tables.is_device else tables.to(dev)
        self._tabs = [getattr(self.tables, name) for name in TABLE_FIELDS]
        self.batch_size, self.H, self.T, self.keep_target_slot = int(batch_size), int(H), int(T), bool(keep_target_slot)
        self.alpha, self.warmup = float(alpha), int(warmup)
        self.N = self.tables.n_impressions
        if self.N < 1:
            raise ValueError(f"{who}: the tables hold no impression")
        self.order = torch.zeros(self.N, dtype=torch.int64, device=dev)
        self._order_host = torch.zeros(self.N, dtype=torch.int64).pin_memory()
        # ONE buffer of 8-byte words, read once per epoch: cursor | sums [3] float64 | counts [2] | step log [log_cap, 2] float32
        self.log_cap = (self.N + self.batch_size - 1) // self.batch_size
        self.state = torch.zeros(6 + self.log_cap, dtype=torch.int64, device=dev)
        self.cursor, self.counts = self.state[0:1], self.state[4:6]
        self.sums = self.state[1:4].view(torch.float64)
        self.step_log = self.state[6:].view(torch.float32).view(self.log_cap, 2)
        ops.index_error_flag(dev)                           # (pinned: allocated before any capture)
        self.graph, self.captured = None, None              # captured: the (lr, alpha) inside the graph
        self.batch = self.loss = self.out = None            # of the latest step; after a replay: the graph's static tensors
        self.lr = float(optimizer.param_groups[0]["lr"])
        self.steps_in_epoch = self.eager_steps = self.replays = self.captures = 0
        self._warm = 0

    def begin_epoch(self, order):
        """``order``: this epoch's impression order (host, [N]); copied into the device buffer in place, state zeroed, rate re-read."""
        order = np.ascontiguousarray(order, dtype=np.int64)
        if order.shape != (self.N,):
            raise ValueError(f"{type(self).__name__}.begin_epoch: order {order.shape} for {self.N} impressions")
        self.model.train()
        self.lr = float(self.optimizer.param_groups[0]["lr"])
        self._order_host.copy_(torch.from_numpy(order))
        self.order.copy_(self._order_host, non_blocking=True)
        self.state.zero_()
        self.steps_in_epoch = 0

    def _step_ops(self, n):
        """one step of ``n`` impressions at the cursor: the SAME four ops eagerly and inside the capture"""
        from . import ops
        from .tables import BATCH_KEYS
        batch = dict(zip(BATCH_KEYS, ops.assemble_batch_at(self._tabs, self.order, self.cursor, n, self.H, self.T, self.keep_target_slot,
                                                           int(self.tables.static_cols))))
        loss, out = train_step(self.model, self.optimizer, batch, None, self.alpha)
        auc, top1 = ops.row_auc(out, batch["label"], None)
        ops.epoch_tally(loss, auc, top1, self.cursor, self.sums, self.counts, self.step_log)
        return batch, loss, out

    def _capture(self):
        self.graph = self._static = None                    # a stale graph and its pool go first
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._static = self._step_ops(self.batch_size)
        self.graph, self.captured = graph, (self.lr, self.alpha)
        self.captures += 1

    def step(self, n=None):
        """The epoch's next step (``n`` impressions; None: a full batch, or what is left of the epoch) -> (loss, out) of it, device tensors
        that the next step may overwrite."""
        left = self.N - self.steps_in_epoch * self.batch_size
        n = min(self.batch_size, left) if n is None else int(n)
        if n < 1 or n > min(left, self.batch_size):
            raise RuntimeError(f"{type(self).__name__}.step: {n} impressions asked for, {max(left, 0)} left in the epoch and at most {self.batch_size} "
                               "in a step (begin_epoch starts the next epoch)")
        if n < self.batch_size or self._warm < self.warmup:
            self.batch, self.loss, self.out = self._step_ops(n)            # (train_step watches the index flag itself)
            self._warm += n == self.batch_size
            self.eager_steps += 1
        else:
            if self.graph is None or self.captured != (self.lr, self.alpha):
                self._capture()
            watch = _index_watch(self.order.device)
            watch.before_step()                              # an out-of-range id of an earlier replay raises IndexError here
            self.graph.replay()
            watch.after_step()
            self.batch, self.loss, self.out = self._static
            self.replays += 1
        self.steps_in_epoch += 1
        return self.loss, self.out

    def end_epoch(self):
        """The epoch's ONE host read -> dict(impressions, steps, loss_sum, auc_sum, top1_sum, one_class_rows, step_loss, step_auc); an
        out-of-range index of any step raises IndexError here at the latest."""
        from . import ops
        host = self.state.cpu()                              # (waits for the stream)
        ops.check_index_errors(self.order.device)
        sums, steps = host[1:4].view(torch.float64), int(host[5])
        log = host[6:].view(torch.float32).view(self.log_cap, 2)[:min(steps, self.log_cap)]
        return {"impressions": int(host[0]), "steps": steps, "loss_sum": float(sums[0]), "auc_sum": float(sums[1]), "top1_sum": float(sums[2]),
                "one_class_rows": int(host[4]), "step_loss": log[:, 0].tolist(), "step_auc": log[:, 1].tolist()}

    def run_epoch(self, order, drop_last=False):
        """``begin_epoch``, every step, ``end_epoch``."""
        self.begin_epoch(order)
        for _ in range(self.N // self.batch_size):
            self.step()
        if self.N % self.batch_size and not drop_last:
            self.step()
        return self.end_epoch()


class GroupedTableEpoch(GraphedTableEpoch):
    """``GraphedTableEpoch`` on compacted batches: the captured step computes neither the trailing all-zero history
    rows nor (``compact_candidates``) the padded candidates, the rows the eager ``train_step(compact_history=True, ...)`` drops with a plan
    made on the host for every batch.

    Here the host plans ONCE PER EPOCH.  The tables give every impression's history length and ``empty_num`` before the epoch starts, and
    the order inside a batch is free, so ``begin_epoch`` sorts every full batch's slice of the order by length and cuts one static plan that
    every full batch fits (``compact.plan_epoch_groups``: the height of sorted position i is the maximum over the batches).  The captured
    step is ``assemble_groups_at`` -- the assemble kernel writing straight into the grouped arenas -- -> ``model.forward_grouped`` ->
    ``model.loss_grouped`` (``model.loss`` without candidate groups) -> backward -> FlatAdam -> ``out`` [B, T] through the plan's static
    ``expand`` -> ``row_auc`` -> ``epoch_tally``; ``out``, ``label`` and the step's batch are in the SORTED order of the batch.  The graph is
    kept over epochs while the new epoch's batches fit the plan and rate and ``alpha`` are unchanged; else the epoch is planned again and the
    step captured again after ``warmup`` eager steps on the new shapes (``captures`` counts, ``replans`` says how many were for a plan).
    Warm-up steps run the same grouped ops eagerly, the trailing partial batch runs the dense eager step, and under a plan with nothing worth
    dropping (``plan.dense``) every step is ``GraphedTableEpoch``'s.  The kernel checks every impression against its group: a misfit (a plan
    that is not this order's) raises ValueError in ``end_epoch``, after the epoch's steps have been applied."""

    def __init__(self, model, optimizer, tables, batch_size, H, T, keep_target_slot=True, alpha=0.95, warmup=3, compact_history=True,
                 compact_candidates=False, max_groups=None, quantum=16, min_saving=None):
        if not (compact_history or compact_candidates):
            raise ValueError("GroupedTableEpoch: neither compact_history nor compact_candidates (the dense captured epoch is GraphedTableEpoch)")
        if not (hasattr(model, "compact_history_applies") and model.compact_history_applies()):
            raise RuntimeError("GroupedTableEpoch: the model does not take forward_grouped (an attention without the fused attention + pool "
                               "node, a feature width that is no multiple of 4, a substituted invariant-interest model or a forward hook); "
                               "capture the dense step (GraphedTableEpoch)")
        if compact_candidates and not model.compact_candidates_applies():
            raise RuntimeError("GroupedTableEpoch(compact_candidates=True): the model's BatchNorm or gate has no row-weight form (not the "
                               "column kernels' nn.BatchNorm1d, or no exact-GELU gate MLP); use compact_history alone or capture the dense step")
        super().__init__(model, optimizer, tables, batch_size, H, T, keep_target_slot=keep_target_slot, alpha=alpha, warmup=warmup)
        from . import ops
        self.compact_history, self.compact_candidates = bool(compact_history), bool(compact_candidates)
        self.max_groups, self.quantum, self.min_saving = max_groups, int(quantum), min_saving
        host = self.tables.host
        self._hist_len = host.history_len(np.arange(self.N), self.H)          # what the producer knows, once
        self._empty = host.empty_num_all(self.T, self.keep_target_slot)
        ops.group_fit_flag(self.order.device)                                 # (pinned: allocated before any capture)
        self.plan, self._plan_tabs, self.replans = None, None, 0

    def begin_epoch(self, order):
        """``order``: this epoch's impression order (host, [N]).  Every full batch's slice is sorted by length before the upload; the plan
        and the graph are kept where the sorted batches fit them."""
        from . import compact
        order = np.ascontiguousarray(order, dtype=np.int64)
        if order.shape != (self.N,):
            raise ValueError(f"GroupedTableEpoch.begin_epoch: order {order.shape} for {self.N} impressions")
        args = (self._hist_len, self._empty, order, self.batch_size, self.H, self.T, self.compact_history)
        if self.plan is not None and self.plan.fits(self._hist_len, self._empty, order):
            order = compact.sort_epoch_order(*args)
        else:
            self.plan = compact.plan_epoch_groups(*args, self.compact_candidates, max_groups=self.max_groups, quantum=self.quantum,
                                                  min_saving=self.min_saving)
            order = self.plan.order
            self._plan_tabs = None if self.plan.dense else self.plan.upload(self.order.device)      # uploaded before any capture
            self.graph = self._static = None                                  # the old plan's launches
            self._warm = 0                                                    # the new shapes run eagerly first
            self.replans += 1
        super().begin_epoch(order)

    def _step_ops(self, n):
        """a full batch under a plan worth having: the grouped step, the same ops eagerly and inside the capture; else the dense step"""
        if n != self.batch_size or self.plan is None or self.plan.dense:
            return super()._step_ops(n)
        from . import ops
        from . import tables as _tables
        capturing = torch.cuda.is_current_stream_capturing()
        watch = None if capturing else _index_watch(self.order.device)
        if watch is not None:
            watch.before_step()
        plan, tabs, B, T = self.plan, self._plan_tabs, self.batch_size, self.T
        batch = _tables.assemble_groups_at(self.tables, self.order, self.cursor, B, self.H, T, plan, self.keep_target_slot)
        xh, xt, xg = batch["x_history_arena"], batch["x_target_arena"], batch["x_global_arena"]
        if plan.cand is not None:
            out_arena = self.model.forward_grouped(xh, xt, xg, plan.hist, row_weight=batch["row_weight"])
            loss = self.model.loss_grouped(batch["user_id"], out_arena, batch["label_arena"], plan.cand, self.alpha)
            out = out_arena.detach().index_select(0, tabs["expand"]).view(B, T)
        else:                                                                 # every group keeps all T slots: the arenas ARE the sorted batch
            out = self.model.forward_grouped(xh, xt.view(B, T, -1), xg.view(B, T, -1), plan.hist)
            loss = self.model.loss(batch["user_id"], out, batch["label"], self.alpha)
        _backward_and_step(loss, self.optimizer)
        if watch is not None:
            watch.after_step()
        loss, out = loss.detach(), out.detach()
        auc, top1 = ops.row_auc(out, batch["label"], None)
        ops.epoch_tally(loss, auc, top1, self.cursor, self.sums, self.counts, self.step_log)
        return batch, loss, out

    def end_epoch(self):
        """``GraphedTableEpoch.end_epoch``; an impression that did not fit its group in any step of the epoch raises ValueError here."""
        from . import ops
        rec = super().end_epoch()                            # (waits for the stream)
        ops.check_group_fit(self.order.device)
        return rec


def shard_batch(batch, rank, world):
    """Rank ``rank`` of ``world`` takes a contiguous 1/world slice of the impressions."""
    B = batch["user_id"].shape[0]
    if B % world:
        raise ValueError(f"batch {B} does not divide over {world} ranks")
    lo, hi = rank * (B // world), (rank + 1) * (B // world)
    return {k: (v[lo:hi] if hasattr(v, "shape") and v.ndim > 0 and v.shape[0] == B else v) for k, v in batch.items()}


def batch_to_device(batch_np, device="cuda", dtype=None):
    out = {}
    for k, v in batch_np.items():
        if k in ("user_num",):
            continue
        t = torch.as_tensor(v)
        if dtype is not None and t.is_floating_point():
            t = t.to(dtype)
        out[k] = t.to(device)
    return out


class BatchPrefetcher:
    """Host -> HBM staging of DataLoader batches on a side stream, one batch ahead of the step.

    The reference moves every field with ``.to(device)`` inside the step (train.py:66-68), float64 as the DataLoader
    yields it; at C3 that is 272 MB per step.  Here the next batch is copied from pinned host memory into one of two
    preallocated device buffer sets on a copy stream while the current step runs; the compute stream waits on the
    copy's event, and a buffer is only overwritten after the step that read it has been enqueued (its event)."""

    def __init__(self, batches, device="cuda", pin=True, history_len=False, empty_num=False):
        """``history_len=True``: the history lengths of every staged batch are measured on a side stream that waits only for the batch's
        own upload, copied to the host and attached as ``batch["history_len_host"]`` (what ``train_step(compact_history=True)`` plans
        from, without draining the compute stream).  ``empty_num=True``: the host copy of ``empty_num`` every batch is staged from is
        kept with it as ``batch["empty_num_host"]`` (what ``train_step(compact_candidates=True)`` plans from)."""
        self.history_len = history_len
        self.empty_num = empty_num
        self.device = torch.device(device)
        self.batches = iter(batches)
        self.pin = pin
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.bufs = [None, None]
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]      # copy finished
        self.free = [None, None]                                    # step that consumed the buffer enqueued
        self.slot = 0
        self._pending = None
        self._stage()

    def _host(self, batch):
        out = {}
        for k, v in batch.items():
            if k == "user_num":
                continue
            t = torch.as_tensor(v)
            out[k] = t.pin_memory() if self.pin and not t.is_pinned() else t
        return out

    def _stage(self):
        try:
            host = self._host(next(self.batches))
        except StopIteration:
            self._pending = None
            return
        i = self.slot
        if self.bufs[i] is None or any(k not in self.bufs[i] or self.bufs[i][k].shape != v.shape or self.bufs[i][k].dtype != v.dtype
                                       for k, v in host.items()):
            self.bufs[i] = {k: torch.empty(v.shape, dtype=v.dtype, device=self.device) for k, v in host.items()}
            self.free[i] = None
        with torch.cuda.stream(self.copy_stream):
            if self.free[i] is not None:
                self.copy_stream.wait_event(self.free[i])
            if self.bufs[i].get("history_len_host") is not None:        # the length kernel of the batch this buffer held reads x_history
                self.copy_stream.wait_event(self.bufs[i]["history_len_host"][1])
            for k, v in host.items():
                self.bufs[i][k].copy_(v, non_blocking=True)
            self.ready[i].record(self.copy_stream)
        if self.history_len:
            self.bufs[i] = attach_history_len(self.bufs[i], after=self.ready[i])
        if self.empty_num and "empty_num" in host:
            self.bufs[i] = attach_empty_num(self.bufs[i], host["empty_num"])
        self._pending = (i, host)                                   # keep the pinned tensors alive until consumed

    def __iter__(self):
        return self

    def __next__(self):
        if self._pending is None:
            raise StopIteration
        i, _host = self._pending
        torch.cuda.current_stream(self.device).wait_event(self.ready[i])
        batch = self.bufs[i]
        self.slot = 1 - i
        self._stage()                                               # next copy overlaps the step about to be enqueued
        return batch, i

    def release(self, slot):
        """Call after the step that read buffer set ``slot`` has been enqueued on the current stream."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.free[slot] = ev


def train_epochs(model, optimizer, make_loader, epochs, device="cuda", ckpt_path=None, on_batch=None, compact_history=False,
                 max_groups=None, compact_candidates=False):
    """The epoch loop of reference train.py:52-100 around ``train_step``: every epoch re-reads ``param_groups[0]['lr']``
    (:57), steps through ``make_loader()`` (an iterable of host batches, dict fields as in ``synth.make_batch``), keeps
    the running loss and per-impression AUC averages the reference prints (:77-88, AUC on the device instead of a
    host sklearn loop), and saves the state_dict without ``delta`` (:95-97).  The reference never steps its scheduler
    (:99-100), so none is taken here.  Batches are staged through ``BatchPrefetcher``.  ``compact_history`` / ``max_groups``: as in
    ``train_step``; the prefetcher then measures the history lengths while it stages a batch.  ``compact_candidates``: as in ``train_step``;
    the prefetcher keeps the host ``empty_num`` of every batch, and a padding error of the epoch's last batches raises at its end.
    Returns one dict per epoch: lr, loss_avg, auc_avg, impressions."""
    from . import evaluation, ops
    history = []
    for epoch in range(epochs):
        model.train()                                                  # :56
        lr = optimizer.param_groups[0]["lr"]
        loss_sum = torch.zeros((), dtype=torch.float64, device=device)
        auc_sum = torch.zeros((), dtype=torch.float64, device=device)
        bad_rows = torch.zeros((), dtype=torch.int64, device=device)
        seen = 0
        pf = BatchPrefetcher(make_loader(), device, history_len=compact_history, empty_num=compact_candidates)
        for i, (batch, slot) in enumerate(pf):
            if compact_candidates:
                loss, out = train_step(model, optimizer, batch, compact_history=compact_history, max_groups=max_groups, compact_candidates=True)
            else:
                loss, out = train_step(model, optimizer, batch, compact_history=compact_history, max_groups=max_groups)
            auc, _hit = evaluation.row_auc_top1(out, batch["label"])
            pf.release(slot)
            n = out.shape[0]
            loss_sum += loss.double() * n                               # :82 total_loss += loss.item() * B
            auc_sum += auc.double().sum()
            bad_rows += (auc < 0).sum()                                 # one class in a row: roc_auc_score raises (:79)
            seen += n
            if on_batch is not None:
                on_batch(epoch, i, loss, auc)
        if int(bad_rows):                                               # checked once per epoch: no per-batch host sync
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        # an out-of-range table index / user id: the reference raises IndexError at the offending batch (F.embedding, delta[id]);
        # the kernels clamp and flag, train_step raises at the start of the NEXT step (IndexErrorWatch, no host sync); the last
        # batches of the epoch are covered here, at the epoch's one host sync
        ops.check_index_errors(next(model.parameters()).device)
        if compact_candidates:
            ops.check_pad_errors(next(model.parameters()).device)
        rec = {"epoch": epoch, "lr": lr, "impressions": seen,
               "loss_avg": float(loss_sum / max(seen, 1)), "auc_avg": float(auc_sum / max(seen, 1))}
        history.append(rec)
        if ckpt_path is not None:
            evaluation.save_checkpoint(model, ckpt_path.format(epoch=epoch))
    return history


def train_epochs_tables(model, optimizer, tables, epochs, batch_size, H, T, shuffle=True, seed=0, keep_target_slot=True, device="cuda",
                        ckpt_path=None, on_batch=None, compact_history=False, max_groups=None, compact_candidates=False, drop_last=False,
                        graph=False, graph_warmup=3, validation=None, validation_batch=80, validation_graph=None):
    """``train_epochs`` over a data set that lives on the device as ``tables.ImpressionTables``: every batch is
    written by the assemble kernel from a few KB of impression indices instead of being uploaded, on the current stream, and carries its
    producer's history lengths and ``empty_num`` on the host, so ``compact_history`` / ``compact_candidates`` plan without a measuring
    kernel or a synchronise.  The per-epoch record, the checkpoints and the index and padding checks are ``train_epochs``'s.  ``tables``:
    host tables (uploaded once) or device tables.
    ``graph=True``: the epochs run through a ``GraphedTableEpoch`` -- after ``graph_warmup`` eager steps every full batch is one graph
    replay, and the host reads the device once per epoch.  The permutations are the eager loop's (the same ``TableLoader`` generator: one
    seed, the same impressions in the same order).  The record gains ``step_loss`` / ``step_auc`` (per step, from the device log) and
    ``top1_avg``; ``on_batch`` is refused (a call per step would need a synchronise per step), and so is everything a captured step
    cannot do (``GraphedTableEpoch``).
    ``graph="grouped"`` (with ``compact_history`` and / or ``compact_candidates``): the captured epoch on compacted
    batches, a ``GroupedTableEpoch`` -- one group plan per epoch instead of one per batch, every full batch sorted by length on the host;
    the record is ``graph=True``'s.
    ``validation``: a second set of tables (labelled) -- after every epoch's checkpoint the model is validated over it in batches of
    ``validation_batch`` as reference train.py:107-110 does, the record gains ``val_auc``, ``val_top1``, ``val_mrr``, ``val_ndcg5`` and
    ``val_ndcg10``, and the model is put back into train mode.  ``validation_graph`` (None: as ``graph``): through one
    ``evaluation.GraphedTableScoring`` kept for all epochs, else ``validate_ranked`` over a ``TableLoader``.  None: nothing changes."""
    from . import evaluation, ops
    from .tables import TableLoader
    validate_epoch = None
    if validation is not None:
        val_graph = bool(graph if validation_graph is None else validation_graph)
        val_runner = evaluation.GraphedTableScoring([model], validation, validation_batch, H, T, keep_target_slot) if val_graph else None
        val_tables = val_runner.tables if val_graph else (validation if validation.is_device else validation.to(device))

        def validate_epoch(rec):
            got = evaluation.validate_tables([model], val_tables, validation_batch, H=H, T=T, keep_target_slot=keep_target_slot, graph=val_graph,
                                             runner=val_runner)
            model.train()
            rec.update({"val_" + k: v for k, v in got.items()})
    grouped = isinstance(graph, str) and graph == "grouped"
    if grouped and not (compact_history or compact_candidates):
        raise ValueError("train_epochs_tables(graph='grouped') needs compact_history=True and / or compact_candidates=True: it is the captured "
                         "epoch on compacted batches (the dense captured epoch is graph=True)")
    if graph:
        if on_batch is not None:
            raise RuntimeError("train_epochs_tables(graph=True, on_batch=...): a call per step would need a host synchronise per step, which is "
                               "what the captured epoch removes; the per-step figures are in the record as step_loss and step_auc")
        if grouped:
            runner = GroupedTableEpoch(model, optimizer, tables, batch_size, H, T, keep_target_slot=keep_target_slot, warmup=graph_warmup,
                                       compact_history=compact_history, compact_candidates=compact_candidates, max_groups=max_groups)
        else:
            runner = GraphedTableEpoch(model, optimizer, tables, batch_size, H, T, keep_target_slot=keep_target_slot, warmup=graph_warmup,
                                       compact_history=compact_history, compact_candidates=compact_candidates)
        loader = TableLoader(runner.tables, batch_size, H, T, shuffle=shuffle, seed=seed, keep_target_slot=keep_target_slot, device=device,
                             drop_last=drop_last)
        history = []
        for epoch in range(epochs):
            lr = optimizer.param_groups[0]["lr"]
            got = runner.run_epoch(loader.take_order(), drop_last=drop_last)
            if got["one_class_rows"]:
                raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
            seen = got["impressions"]
            history.append({"epoch": epoch, "lr": lr, "impressions": seen, "loss_avg": got["loss_sum"] / max(seen, 1),
                            "auc_avg": got["auc_sum"] / max(seen, 1), "top1_avg": got["top1_sum"] / max(seen, 1),
                            "step_loss": got["step_loss"], "step_auc": got["step_auc"]})
            if ckpt_path is not None:
                evaluation.save_checkpoint(model, ckpt_path.format(epoch=epoch))
            if validate_epoch is not None:
                validate_epoch(history[-1])
        return history
    loader = TableLoader(tables, batch_size, H, T, shuffle=shuffle, seed=seed, keep_target_slot=keep_target_slot, device=device, drop_last=drop_last)
    history = []
    for epoch in range(epochs):
        model.train()
        lr = optimizer.param_groups[0]["lr"]
        loss_sum = torch.zeros((), dtype=torch.float64, device=device)
        auc_sum = torch.zeros((), dtype=torch.float64, device=device)
        bad_rows = torch.zeros((), dtype=torch.int64, device=device)
        seen = 0
        for i, batch in enumerate(loader):
            loss, out = train_step(model, optimizer, batch, compact_history=compact_history, max_groups=max_groups,
                                   compact_candidates=compact_candidates)
            auc, _hit = evaluation.row_auc_top1(out, batch["label"])
            n = out.shape[0]
            loss_sum += loss.double() * n
            auc_sum += auc.double().sum()
            bad_rows += (auc < 0).sum()
            seen += n
            if on_batch is not None:
                on_batch(epoch, i, loss, auc)
        if int(bad_rows):
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        ops.check_index_errors(next(model.parameters()).device)
        if compact_candidates:
            ops.check_pad_errors(next(model.parameters()).device)
        history.append({"epoch": epoch, "lr": lr, "impressions": seen,
                        "loss_avg": float(loss_sum / max(seen, 1)), "auc_avg": float(auc_sum / max(seen, 1))})
        if ckpt_path is not None:
            evaluation.save_checkpoint(model, ckpt_path.format(epoch=epoch))
        if validate_epoch is not None:
            validate_epoch(history[-1])
    return history
