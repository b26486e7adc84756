"""nn.Module mirror of the reference model interface.

Same class names, constructor arguments, forward signatures, reachable attributes and
``state_dict`` keys as the reference's ``models/`` package, so its checkpoints load and its
train/test drivers can call these classes unchanged:

  MLP(input_dim, output_dim, activation_type='gelu')                 models/attention_model.py:10-32
  PointwiseAttention(input_dim)                                      models/attention_model.py:34-44
  PointwiseAttentionExpanded(input_dim)                              models/attention_model.py:47-97
  UserInvariantInterestModel(embed_setting=[32,16,8,8])              models/user_invariant_interest_model.py:10-89
  UserInstantInterestModel(output_dim)                               models/user_instant_interest_model.py:10-23
  UserModel(user_num=0)  .forward(x_history, x_target, x_global), .loss(id, out, label, alpha)
                                                                     models/user_model.py:12-43

Modules can be built, pickled and (de)serialised on the CPU; ``forward`` needs an MI355X: the hot
ops go through the C-ABI HIP kernels (ops.py) and raise on CPU tensors.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .config import Dims, TIME_TABLE_ROWS, model_config

_ACTIVATIONS = {
    "relu": nn.ReLU, "gelu": nn.GELU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid,
    "leaky_relu": nn.LeakyReLU, "elu": nn.ELU,
}


class MLP(nn.Module):
    """Linear(d, d//4) -> activation -> Linear(d//4, out); unknown activation names mean GELU."""

    def __init__(self, input_dim, output_dim, activation_type="gelu"):
        super().__init__()
        self.fc1 = nn.Linear(input_dim, input_dim // 4)
        self.fc2 = nn.Linear(input_dim // 4, output_dim)
        self.activation_type = activation_type
        self.activation = _ACTIVATIONS.get(str(activation_type).lower(), nn.GELU)()

    def forward(self, x):
        return self.forward_times(x, None)

    def forward_times(self, x, mul):
        """forward(x) [* mul]: the product (the gate of models/user_model.py:33) rides in fc2's GEMM epilogue."""
        ops._require_gpu(x)
        if isinstance(self.activation, nn.GELU) and self.activation.approximate == "none":
            # one autograd node: bias + exact GELU fused into fc1's GEMM, GELU' fused into the backward GEMM of fc2
            return ops.mlp_gelu(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, mul=mul)
        hidden = self.activation(ops.linear(x, self.fc1.weight, self.fc1.bias))
        y = ops.linear(hidden, self.fc2.weight, self.fc2.bias)
        return y if mul is None else y * mul


def _scores(mlp: MLP, target, history, mma=None):
    if not isinstance(mlp.activation, nn.GELU):
        raise RuntimeError("the HIP attention kernel implements the reference default (exact GELU) only")
    return ops.pointwise_attention_scores(target, history, mlp.fc1.weight, mlp.fc1.bias,
                                          mlp.fc2.weight, mlp.fc2.bias, mma=mma)


class PointwiseAttentionExpanded(nn.Module):
    """score[b,t,h] = MLP(cat[h, t, t-h, t*h]) for every (candidate, history) pair -> [B,T,H,1]."""

    mma = None          # arithmetic of the contraction: None = ops.set_attention_arithmetic default, 'f32' or 'bf16'

    def __init__(self, input_dim):
        super().__init__()
        self.mlp = MLP(input_dim * 4, 1)

    def forward(self, target, history):
        if target.dim() == 2:                      # a single target per impression
            target = target.unsqueeze(1)
        return _scores(self.mlp, target, history, self.mma).unsqueeze(-1)


class PointwiseAttention(nn.Module):
    """Non-broadcast variant (unused by UserModel): target and history have the same [N, D] shape,
    one score per row.  Runs the same kernel with T = H = 1."""

    def __init__(self, input_dim):
        super().__init__()
        self.mlp = MLP(input_dim * 4, 1)

    def forward(self, target, history):
        lead = target.shape[:-1]
        d = target.shape[-1]
        history = history.expand_as(target)
        s = _scores(self.mlp, target.reshape(-1, 1, d), history.reshape(-1, 1, d))
        return s.reshape(*lead, 1)


class UserInvariantInterestModel(nn.Module):
    """Embeds the packed history / candidate rows and pools the history with two pointwise
    attentions (label features, text+image vector) -> (eu_H, ec)."""

    def __init__(self, embed_setting=[32, 16, 8, 8]):
        super().__init__()
        self.embed_setting = embed_setting
        dims = Dims.from_config(embed_setting, model_config)
        self._dims = dims
        e0, e1, e2, e3 = dims.embed_setting
        # column widths of a packed row: time4 | text_img | category | sub-categories | sentiment | type | read | scroll
        self.slice_len_list = [4, dims.pca_vector, 1, dims.n_subcat, dims.n_sentiment, 1, 1, 1]
        self.category_embedding = nn.Sequential(nn.Embedding(dims.category_label_num, e0))
        self.sentiment_embedding = nn.Sequential(nn.Linear(dims.n_sentiment, e1), nn.ReLU())
        self.type_embedding = nn.Sequential(nn.Embedding(dims.n_type, e2))
        self.w1 = nn.Linear(dims.label_dim + 2, dims.label_dim)
        self.year_embedding = nn.Sequential(nn.Embedding(TIME_TABLE_ROWS[0], e3))
        self.month_embedding = nn.Sequential(nn.Embedding(TIME_TABLE_ROWS[1], e3))
        self.day_embedding = nn.Sequential(nn.Embedding(TIME_TABLE_ROWS[2], e3))
        self.hour_embedding = nn.Sequential(nn.Embedding(TIME_TABLE_ROWS[3], e3))
        self.label_attention = PointwiseAttentionExpanded(dims.label_dim)
        self.text_img_attention = PointwiseAttentionExpanded(dims.pca_vector)

    # -- helpers ---------------------------------------------------------------------------
    def slice_x(self, x, n):
        return list(torch.split(x[:, :, :sum(self.slice_len_list[:n])], self.slice_len_list[:n], dim=2))

    def feature_embedding(self, category, sub_category, sentiment, type):
        table = self.category_embedding[0].weight
        cat = F.embedding(category[..., 0].long(), table)
        sub = F.embedding(sub_category.long(), table).mean(dim=2)       # mean includes padding id 0
        sen = self.sentiment_embedding(sentiment)
        typ = F.embedding(type[..., 0].long(), self.type_embedding[0].weight)
        return torch.cat((cat + sub, sen, typ), dim=2)

    def time_embedding(self, time):
        idx = time.long()
        return (self.year_embedding[0](idx[..., 0]) + self.month_embedding[0](idx[..., 1])
                + self.day_embedding[0](idx[..., 2]) + self.hour_embedding[0](idx[..., 3]))

    def _embed(self, x, behaviour):
        """Fused front end (slice_x + feature_embedding + time_embedding [+ read_time, scroll]) on packed rows."""
        sen = self.sentiment_embedding[0]
        return ops.frontend(x, behaviour, self._dims.n_subcat, self._dims.pca_vector,
                            self.category_embedding[0].weight, sen.weight, sen.bias, self.type_embedding[0].weight,
                            self.year_embedding[0].weight, self.month_embedding[0].weight,
                            self.day_embedding[0].weight, self.hour_embedding[0].weight)

    def forward(self, x_history, x_target):
        pooled_lab, pooled_ti, lab_t, ti_t = self.forward_parts(x_history, x_target)
        return ops.concat_last((pooled_lab, pooled_ti)), ops.concat_last((lab_t, ti_t))       # (eu_H, ec): :81,:88

    def forward_parts(self, x_history, x_target):
        """The four column blocks of forward()'s two results -- eu_H = [pooled_lab | pooled_ti], ec = [lab_t | ti_t] -- before their
        concatenation: UserModel.forward writes them into the head's [eu_H | eu_L | ec] rows with ONE launch instead of three
        (two here, one there: 0.14 ms of a 31 ms step at C3, 50 us of 3.2 ms at C2)."""
        ops._require_gpu(x_history, x_target)
        if x_history.shape[0] * x_history.shape[1] == 0 or x_target.shape[1] == 0:
            # same error as the reference, whose feature_embedding reshapes with a -1 dimension (:59); the ops below
            # would accept empty inputs (ops._degenerate), the drop-in keeps the reference's behaviour
            raise RuntimeError("cannot reshape tensor of 0 elements (empty batch / history / candidate list)")
        # [B,H,D_l+2], [B,H,P], [B,T,D_l], [B,T,P]: both row sets through one autograd node (their table gradients share one arena)
        sen = self.sentiment_embedding[0]
        lab_h, ti_h, lab_t, ti_t = ops.frontend_pair(
            x_history, x_target, self._dims.n_subcat, self._dims.pca_vector, self.category_embedding[0].weight, sen.weight, sen.bias,
            self.type_embedding[0].weight, self.year_embedding[0].weight, self.month_embedding[0].weight,
            self.day_embedding[0].weight, self.hour_embedding[0].weight)
        lab_h = ops.linear(lab_h, self.w1.weight, self.w1.bias)

        # The two attentions (label features / text+image vector) share no data until the concat, so the second one is issued on
        # a side stream and overlaps the first -- in eager mode and as two parallel branches of the captured HIP graph; autograd
        # runs every backward node on the stream of its forward and joins the streams at the end of backward().  On small
        # shapes (C1, C2, the reference's default sizes) neither attention fills the chip; on full-size batches the HBM-bound
        # and the MFMA-bound kernels of the two branches overlap (ops.BRANCH_STREAMS_MAX_ELEMS).
        side = ops.branch_stream(lab_t) if self._two_streams(lab_t, lab_h) else None
        if side is not None:
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            ti_t.record_stream(side)            # allocated on the main stream, read by side-stream kernels (forward and backward)
            ti_h.record_stream(side)
            with torch.cuda.stream(side):
                pooled_ti = self._attend_and_pool(self.text_img_attention, ti_t, ti_h)
            pooled_lab = self._attend_and_pool(self.label_attention, lab_t, lab_h)
            main.wait_stream(side)
            pooled_ti.record_stream(main)
        else:
            pooled_lab = self._attend_and_pool(self.label_attention, lab_t, lab_h)
            pooled_ti = self._attend_and_pool(self.text_img_attention, ti_t, ti_h)
        return pooled_lab, pooled_ti, lab_t, ti_t

    def forward_parts_grouped(self, x_history_arena, x_target, plan):
        """forward_parts on length groups: ``x_history_arena`` [R, cols] are the plan's kept history rows
        (``ops.history_gather_groups``), ``x_target`` [B, T, cols] is in the plan's SORTED order; -> the same four blocks in sorted order.
        The front end and w1 are row-wise and run on the R history rows and the candidate rows unchanged; only the two attention + pool
        nodes know about the groups.  A plan that carries candidate groups (``plan.cand``) takes ``x_target`` as the
        candidate arena [N, cols] (``ops.candidate_gather_groups``) and returns the four blocks as arena rows [N, width]."""
        ops._require_gpu(x_history_arena, x_target)
        cand = getattr(plan, "cand", None)
        if cand is None:
            B, T = x_target.shape[0], x_target.shape[1]
            if x_history_arena.dim() != 2 or x_history_arena.shape[0] != plan.R or B != plan.B or B * T == 0 or plan.R == 0:
                raise RuntimeError(f"forward_grouped: plan for {plan.B} impressions / {plan.R} kept history rows, got a history arena "
                                   f"{tuple(x_history_arena.shape)} and targets {tuple(x_target.shape)}")
            x_target = x_target.reshape(B * T, x_target.shape[2])                               # the rows of the sorted batch
        else:
            if (x_history_arena.dim() != 2 or x_history_arena.shape[0] != plan.R or x_target.dim() != 2 or x_target.shape[0] != cand.N
                    or cand.B != plan.B or cand.N == 0 or plan.R == 0):
                raise RuntimeError(f"forward_grouped: plan for {plan.R} kept history rows / {cand.N} candidate rows, got a history arena "
                                   f"{tuple(x_history_arena.shape)} and a candidate arena {tuple(x_target.shape)}")
        if not self.grouped_attention_applies():
            raise RuntimeError("forward_grouped: an attention of this model does not take the fused attention + pool node (feature width "
                               "not a multiple of 4, a non-GELU MLP or a substituted module): run the dense forward")
        sen = self.sentiment_embedding[0]
        lab_h, ti_h, lab_t, ti_t = ops.frontend_pair_fwd(
            x_history_arena, x_target, int(self._dims.n_subcat), int(self._dims.pca_vector),
            self.category_embedding[0].weight, sen.weight, sen.bias, self.type_embedding[0].weight, self.year_embedding[0].weight,
            self.month_embedding[0].weight, self.day_embedding[0].weight, self.hour_embedding[0].weight)
        ti_h, ti_t = ti_h.detach(), ti_t.detach()
        lab_h = ops.linear(lab_h, self.w1.weight, self.w1.bias)                                       # [R, D_l]
        if cand is None:                        # the attention node and the caller take the sorted batch as [B, T, width]
            ti_t = ti_t.unflatten(0, (B, T))
            lab_t = lab_t.reshape(B, T, -1) if lab_t.is_contiguous() else lab_t.unflatten(0, (B, T))

        def attend(att, t, h):
            m = att.mlp
            return ops.attend_and_pool_grouped(t, h, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, plan, mma=att.mma)

        # two streams as in forward_parts; the choice goes by the z elements the groups really have
        z_rows = plan.R * T if cand is None else sum(int(n) * int(tg) * int(hg) for n, tg, hg in
                                                     zip(plan.bounds[1:] - plan.bounds[:-1], cand.T_g, plan.H_g))
        side = ops.branch_stream(lab_t) if self.uses_two_streams(z_rows * lab_h.shape[1]) else None
        if side is not None:
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            ti_t.record_stream(side)
            ti_h.record_stream(side)
            with torch.cuda.stream(side):
                pooled_ti = attend(self.text_img_attention, ti_t, ti_h)
            pooled_lab = attend(self.label_attention, lab_t, lab_h)
            main.wait_stream(side)
            pooled_ti.record_stream(main)
        else:
            pooled_lab = attend(self.label_attention, lab_t, lab_h)
            pooled_ti = attend(self.text_img_attention, ti_t, ti_h)
        return pooled_lab, pooled_ti, lab_t, ti_t

    def grouped_attention_applies(self):
        """Whether both attentions take the fused attention + pool node on feature widths the grouped node accepts (multiples of 4)."""
        for att, width in ((self.label_attention, self._dims.label_dim), (self.text_img_attention, self._dims.pca_vector)):
            if not self._fused_node_applies(att) or width % 4 or att._forward_hooks or att._forward_pre_hooks:
                return False
        return True

    @staticmethod
    def _fused_node_applies(attention):
        mlp = getattr(attention, "mlp", None)
        return (type(attention) is PointwiseAttentionExpanded and isinstance(mlp, MLP) and isinstance(mlp.activation, nn.GELU)
                and mlp.activation.approximate == "none")

    @staticmethod
    def _attend_and_pool(attention, t, h):
        # un-normalised weighted pool: sum_h score * history  (no softmax, padding not masked)
        if UserInvariantInterestModel._fused_node_applies(attention) and t.dim() == 3:
            mlp = attention.mlp
            # scores + pool as one autograd node (the backward chains their kernels: ops._attend_pool_bwd_impl)
            return ops.attend_and_pool(t, h, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, mma=attention.mma)
        s = attention(t, h)                                            # [B,T,H,1]
        return ops.weighted_pool(s.squeeze(-1), h)

    two_streams = None          # None: by size; True / False force it (env NRM_BRANCH_STREAMS=0|1 overrides both)

    def _two_streams(self, t, h):
        return self.uses_two_streams(t.shape[0] * t.shape[1] * h.shape[1] * h.shape[2])

    def uses_two_streams(self, z_elems):
        """Whether forward() issues its second attention on the side stream for attentions of ``z_elems`` = B*T*H*D."""
        forced = os.environ.get("NRM_BRANCH_STREAMS")
        if forced is not None:
            return forced == "1"
        if self.two_streams is not None:
            return bool(self.two_streams)
        return z_elems <= ops.BRANCH_STREAMS_MAX_ELEMS


class UserInstantInterestModel(nn.Module):
    """ReLU(Linear(3 -> output_dim)) on the per-candidate popularity scalars."""

    def __init__(self, output_dim):
        super().__init__()
        self.output_dim = output_dim
        self.out_fc = nn.Sequential(nn.Linear(3, output_dim), nn.ReLU())

    def forward(self, x_global):
        ops._require_gpu(x_global)
        fc = self.out_fc[0]
        # 3 -> 8 columns: one thread per row forward, a register reduction over the rows backward (ops.small_linear_relu; reads
        # the DataLoader's float64 rows directly)
        return ops.small_linear_relu(x_global, fc.weight, fc.bias)


class UserModel(nn.Module):
    """cat[eu_H, eu_L, ec] -> BatchNorm gate -> MLP -> MLP -> one logit per candidate."""

    def __init__(self, user_num=0):
        super().__init__()
        self.invariant_interest_model = UserInvariantInterestModel()
        self.instant_interest_model = UserInstantInterestModel(8)
        width = (sum(self.invariant_interest_model.embed_setting) + model_config["pca_vector"]) * 2 \
            + self.instant_interest_model.output_dim
        self.bn = nn.BatchNorm1d(width)
        self.gate = MLP(width, width)
        self.mlp = MLP(width, width)
        self.out_mlp = MLP(width, 1)
        self.delta = nn.Parameter(torch.zeros(user_num + 1))
        self.bce_loss = nn.BCELoss()
        self.softmax = nn.Softmax(dim=1)

    def _tail(self, gated):
        """out_mlp(mlp(gated)) (:34).  mlp.fc2 feeds out_mlp.fc1 with no nonlinearity in between: where the folded node applies
        (ops.head_tail) the rows are never widened to mlp's output width and narrowed again."""
        if gated.dim() == 2 and gated.shape[0] > 0 and self.head_fold_applies(gated.shape[1]):
            m, o = self.mlp, self.out_mlp
            return ops.head_tail(gated, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, o.fc1.weight, o.fc1.bias,
                                 o.fc2.weight, o.fc2.bias)
        return self.out_mlp(self.mlp(gated))

    def head_fold_applies(self, width):
        """Whether rows of ``width`` columns take the folded tail: fp32 dense arithmetic (and not NRM_HEAD_FOLD=0), both MLPs plain
        ``MLP`` with exact GELU over plain ``nn.Linear`` layers, no forward or backward hook on either MLP or its layers, widths
        the kernels take.  Never a matter of the row count: two runs of one model take the same path whatever their batch sizes."""
        if not ops.head_fold_enabled():
            return False
        for mod in (self.mlp, self.out_mlp):
            if type(mod) is not MLP or type(mod.fc1) is not nn.Linear or type(mod.fc2) is not nn.Linear:
                return False
            if not isinstance(mod.activation, nn.GELU) or mod.activation.approximate != "none":
                return False
            for layer in (mod, mod.fc1, mod.fc2, mod.activation):
                if layer._forward_hooks or layer._forward_pre_hooks or layer._backward_hooks or layer._backward_pre_hooks:
                    return False
        m, o = self.mlp, self.out_mlp
        return ops.head_fold_shapes_ok(width, m.fc1.weight, m.fc2.weight, m.fc2.bias, o.fc1.weight, o.fc1.bias, o.fc2.weight)

    def forward(self, x_history, x_target, x_global):
        inv = self.invariant_interest_model
        if type(inv) is UserInvariantInterestModel and not (inv._forward_hooks or inv._forward_pre_hooks):
            # e = cat[eu_H, eu_L, ec] (:31) with eu_H and ec never materialised on their own: one concat launch of five blocks
            pooled_lab, pooled_ti, lab_t, ti_t = inv.forward_parts(x_history, x_target)
            eu_L = self.instant_interest_model(x_global)
            e = ops.concat_last((pooled_lab, pooled_ti, eu_L, lab_t, ti_t))
        else:                                   # a hooked / substituted sub-model is called as the reference calls it (:28)
            eu_H, ec = inv(x_history, x_target)
            eu_L = self.instant_interest_model(x_global)
            e = ops.concat_last((eu_H, eu_L, ec))
        return self._head(e)

    def _head(self, e, row_weight=None, n_rows=None):
        """BatchNorm gate -> MLP -> MLP on the concatenated rows e [B, T, width] -> logits [B, T] (:32-34).  With ``row_weight`` [N] (DESIGN.md
        section 5f) e is the [N, width] rows of a candidate arena that stand for ``n_rows`` = B * T rows; -> logits [N]."""
        rows = e.reshape(-1, e.shape[-1])
        g = self.gate
        if isinstance(g.activation, nn.GELU) and g.activation.approximate == "none":
            # BatchNorm -> gate MLP -> product with the RAW concat as one autograd node
            gated = ops.gate_block(rows, self.bn, g.fc1.weight, g.fc1.bias, g.fc2.weight, g.fc2.bias, row_weight, n_rows)
        else:
            gated = g.forward_times(ops.batch_norm(rows, self.bn, row_weight, n_rows), rows)     # the gate multiplies the RAW concat
        return self._tail(gated).reshape(e.shape[:-1])

    def compact_history_applies(self):
        """Whether ``forward_grouped`` can stand in for ``forward``: the plain invariant-interest model (not hooked, not substituted)
        whose two attentions take the fused node, and no forward hook on the model itself."""
        inv = self.invariant_interest_model
        if self._forward_hooks or self._forward_pre_hooks:          # forward_grouped is not forward(): hooks on the model would not run
            return False
        return (type(inv) is UserInvariantInterestModel and not (inv._forward_hooks or inv._forward_pre_hooks)
                and inv.grouped_attention_applies())

    def compact_candidates_applies(self):
        """Whether ``forward_grouped`` with a plan that carries candidate groups can stand in for a training ``forward`` (DESIGN.md section
        5f): what ``compact_history_applies`` asks, a BatchNorm configuration and width the column kernels take (the ``nn.BatchNorm1d``
        fallback has no row-weight form), and the exact-GELU gate."""
        g = self.gate
        return (self.compact_history_applies() and type(self.bn) is nn.BatchNorm1d and ops.bn_column_kernels_apply(self.bn, self.bn.num_features)
                and not (self.bn._forward_hooks or self.bn._forward_pre_hooks)
                and isinstance(g, MLP) and isinstance(g.activation, nn.GELU) and g.activation.approximate == "none"
                and g.fc2.weight.shape[0] == self.bn.num_features)

    def loss_grouped(self, id_sorted, out_arena, label_arena, cand, alpha=0.95):
        """``loss`` of the dense [B, T] batch from the arena logits of ``forward_grouped`` (``cand``: the plan's ``CandidateGroupPlan``;
        ``id_sorted`` [B] in its sorted order, ``label_arena`` [N] from ``ops.candidate_gather_groups``)."""
        return ops.softmax_bce_loss_grouped(out_arena, self.delta, label_arena, id_sorted, cand, alpha)

    def forward_grouped(self, x_history_arena, x_target_sorted, x_global_sorted, plan, row_weight=None):
        """forward() on histories cut into length groups, training or eval mode.  ``plan`` is a
        ``compact.HistoryGroupPlan``; ``x_history_arena`` [R, cols] its kept history rows (``ops.history_gather_groups``), ``x_target_sorted``
        / ``x_global_sorted`` the batch's rows in the plan's sorted order (``index_select`` with ``plan.perm``).  -> logits [B, T] in SORTED
        order (the caller un-permutes them with ``plan.inverse``).  Every candidate row is there, so training-mode BatchNorm sees the
        B * T rows the dense forward sees, in another order.  Agrees with forward() on the dense batch to fp32 rounding (one product by
        w_g in place of w_g equal addends in the pool)."""
        pooled_lab, pooled_ti, lab_t, ti_t = self.invariant_interest_model.forward_parts_grouped(x_history_arena, x_target_sorted, plan)
        eu_L = self.instant_interest_model(x_global_sorted)
        cand = getattr(plan, "cand", None)
        if cand is None:
            return self._head(ops.concat_last((pooled_lab, pooled_ti, eu_L, lab_t, ti_t)))
        # candidate groups (section 5f): x_target_sorted / x_global_sorted are the candidate ARENAS [N, cols], row_weight [N] their row
        # weights (ops.candidate_gather_groups); -> logits [N] in arena order.  Training-mode BatchNorm takes its statistics with the
        # weights over the cand.B * cand.T rows the dense forward sees; eval mode is row-wise and ignores them.
        if row_weight is None or row_weight.shape[0] != cand.N:
            raise RuntimeError(f"forward_grouped: a plan with candidate groups needs the arena's row weights [{cand.N}]")
        return self._head(ops.concat_last((pooled_lab, pooled_ti, eu_L, lab_t, ti_t)), row_weight, cand.B * cand.T)

    def forward_compact(self, x_history, xt_compact, xg_compact, plan):
        """Inference on ragged candidate lists (compact scoring path): ``xt_compact`` [N, cols] and
        ``xg_compact`` [N, 3] are the plan's rows of x_target / x_global (``ops.compact_gather``), ``plan`` a
        ``compact.CompactPlan``; -> logits [N] fp32 (a strided view of the last GEMM's output).  A plan that carries history tables
        (``build_plan(..., history_len=, H=)``) takes ``x_history`` as the gathered [R, cols] rows
        (``ops.history_gather``) and runs the attention that is ragged in the history too; its logits agree with forward()'s to fp32
        rounding (one product by ``H - L_b`` in place of as many equal addends), not bitwise.  The logit of a compact candidate
        is the one forward() gives its source cell: everything but the two attentions and the pool is row-wise and runs on the N
        rows unchanged, and eval-mode BatchNorm uses the running statistics.  Eval mode only: in training mode BatchNorm's
        batch statistics would see N rows where the reference sees B * T.  fp32 attention arithmetic only."""
        if self.training:
            raise RuntimeError("UserModel.forward_compact is inference only: call .eval() first (training-mode BatchNorm takes its "
                               "statistics over the rows of the launch, and the compact path drops the padded ones)")
        inv = self.invariant_interest_model
        ops._require_gpu(x_history, xt_compact, xg_compact)
        hist = getattr(plan, "hist_off", None) is not None
        if hist:
            if x_history.dim() != 2 or x_history.shape[0] != plan.R or plan.N != xt_compact.shape[0] or xg_compact.shape[0] != plan.N:
                raise RuntimeError(f"forward_compact: plan for {plan.R} kept history rows / {plan.N} candidate rows, got x_history "
                                   f"{tuple(x_history.shape)}, {xt_compact.shape[0]} target and {xg_compact.shape[0]} global rows")
            B, H, N = plan.B, plan.H, plan.N
            x_history = x_history.unsqueeze(0)                           # [1, R, cols]: the front end is row-wise
        else:
            B, H, N = x_history.shape[0], x_history.shape[1], xt_compact.shape[0]
        if not hist and (plan.B != B or plan.N != N or xg_compact.shape[0] != N):
            raise RuntimeError(f"forward_compact: plan for {plan.B} impressions / {plan.N} rows, got {B} / {N} target and {xg_compact.shape[0]} global rows")
        if B * H == 0 or N == 0:
            raise RuntimeError("cannot reshape tensor of 0 elements (empty batch / history / candidate list)")
        if not (inv._fused_node_applies(inv.label_attention) and inv._fused_node_applies(inv.text_img_attention)):
            raise RuntimeError("forward_compact: the ragged attention implements the reference default (PointwiseAttentionExpanded, exact GELU) only")
        tabs = plan.upload(x_history.device)
        with torch.no_grad():
            sen = inv.sentiment_embedding[0]
            tables = (inv.category_embedding[0].weight, sen.weight, sen.bias, inv.type_embedding[0].weight, inv.year_embedding[0].weight,
                      inv.month_embedding[0].weight, inv.day_embedding[0].weight, inv.hour_embedding[0].weight)
            d = inv._dims
            lab_h, ti_h = ops.frontend(x_history, True, d.n_subcat, d.pca_vector, *tables)             # [B,H,D_l+2], [B,H,P]
            lab_t, ti_t = ops.frontend(xt_compact.unsqueeze(0), False, d.n_subcat, d.pca_vector, *tables)      # [1,N,D_l], [1,N,P]
            lab_h = ops.linear(lab_h, inv.w1.weight, inv.w1.bias)
            pooled = []
            for att, t, h in ((inv.label_attention, lab_t[0], lab_h), (inv.text_img_attention, ti_t[0], ti_h)):
                m = att.mlp
                if hist:
                    pooled.append(ops.attend_pool_hragged(t, h[0], m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, tabs, plan.max_count,
                                                          plan.k_max, mma=att.mma))
                    continue
                pooled.append(ops.attend_pool_ragged(t, h, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, tabs["cand_imp"],
                                                     tabs["cand_off"], plan.max_count, mma=att.mma))
            eu_L = self.instant_interest_model(xg_compact)
            return self._head(ops.concat_last((pooled[0], pooled[1], eu_L, lab_t[0], ti_t[0])))     # rows [N, width] -> logits [N]

    def loss(self, id, out, label, alpha=0.95):
        # any number of candidates: one wave per impression, in registers up to T = 256, re-reading the row beyond (csrc/pool_loss.hip)
        return ops.softmax_bce_loss(out, self.delta, label, id, alpha)
