"""GPU: the captured epoch on compacted batches.  The grouped assemble kernel against the composition it replaces --
assemble_batch_at, then history_gather_groups and candidate_gather_groups with the identity permutation -- bit for bit; its fit check; and
trainer.GroupedTableEpoch / train_epochs_tables(graph="grouped") against the dense eager table-fed loop on the same impressions.

The gates of the epoch tests are those of tests/test_gpu_table_epoch.py; what was measured before relying on them is at GATES."""
import numpy as np
import pytest
import torch

from news_recommendation_model_amd import compact, tables
from news_recommendation_model_amd.config import Dims
from test_gpu_table_epoch import FORMS, FWD_TOL, PARAM_ATOL, STEP_TOL, _bits, _load_state, _rel, _save_state

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- the kernel, bit for bit
# the five impressions of the batch, in the order the plan wants them (by history length): 0 events; exactly H_g - 1 = 15 events; exactly
# H_g - 1 = 31; 35; 45 (cut at H).  Their lists: 1 and 2 candidates (< T_g = 3), 4 (< 5), 10 with the target LAST (a late target: slot T - 1
# under keep_target_slot), 7.  Four more impressions surround them in ``order``: the cursor stands in mid-order.
HIST_LENS = [0, 15, 31, 35, 45, 5, 20]
LIST_LENS = [1, 2, 4, 10, 7, 3, 9, 6, 2]
USERS = [0, 1, 2, 3, 4, 5, 6, 5, 6]
ORDER = np.array([6, 7, 0, 1, 2, 3, 4, 8, 5], dtype=np.int64)
CURSOR = 2
# (B, H, T, bounds, H_g, T_g)
SHAPES = {
    "three_groups": (5, 40, 6, [0, 2, 3, 5], [16, 32, 40], [3, 5, 6]),
    "one_of_each": (1, 1, 1, [0, 1], [1], [1]),
    "H16_one_group": (5, 16, 6, [0, 5], [16], [6]),
    "two_candidate_waves": (5, 40, 20, [0, 2, 3, 5], [16, 32, 40], [3, 17, 20]),
}


def _kernel_tables(dims, dtype):
    from news_recommendation_model_amd import synth
    recs = synth.make_records(dims, 30, len(HIST_LENS), len(LIST_LENS), seed=13, history_lens=HIST_LENS, list_lens=LIST_LENS)
    recs[2]["user_id"] = recs[1]["user_id"][USERS]
    recs[2]["article_ids_clicked"][3] = recs[2]["article_ids_inview"][3][-1:]                # the late target
    return tables.ImpressionTables.from_records(*recs, dims, history_max=50, dtype=dtype)


def _i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device="cuda")


def _plan_tabs(B, H, T, bounds, H_g, T_g):
    size = np.diff(bounds)
    hro, cro = np.concatenate([[0], np.cumsum(size * np.asarray(H_g))]), np.concatenate([[0], np.cumsum(size * np.asarray(T_g))])
    return [_i32(x) for x in (bounds, H_g, hro, T_g, cro)], int(hro[-1]), int(cro[-1])


def _grouped(dt, order_dev, cursor, B, H, T, tabs, R, N, keep=True):
    from news_recommendation_model_amd import ops
    out = ops.assemble_groups_at([getattr(dt, n) for n in tables.TABLE_FIELDS], order_dev, torch.tensor([cursor], dtype=torch.int64, device="cuda"),
                                 B, H, T, keep, int(dt.static_cols), *tabs, R, N)
    return dict(zip(tables.GROUP_KEYS, out))


def _composition(dt, order_dev, cursor, B, H, T, tabs, R, N, keep=True):
    """what the kernel replaces: the dense batch, then the two gather kernels with the identity permutation"""
    from news_recommendation_model_amd import ops
    dense = tables.assemble_batch_at(dt, order_dev, torch.tensor([cursor], dtype=torch.int64, device="cuda"), B, H, T, keep)
    bounds, H_g, hro, T_g, cro = tabs
    perm = _i32(np.arange(B))
    want = {"x_history_arena": ops.history_gather_groups(dense["x_history"], perm, bounds, hro, H_g, R)}
    xt, xg, lab, roww = ops.candidate_gather_groups(dense["x_target"], dense["x_global"], dense["label"], perm, bounds, cro, T_g, N)
    want.update(x_target_arena=xt, x_global_arena=xg, label_arena=lab, row_weight=roww)
    for k in ("label", "label_id", "empty_num", "user_id", "impression_id", "history_len"):
        want[k] = dense[k]
    return want


def _same(got, want, rows_h=None, rows_c=None):
    assert set(got) == set(tables.GROUP_KEYS) == set(want)
    for k in tables.GROUP_KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if k == "x_history_arena" and rows_h is not None:
            g, w = g[rows_h], w[rows_h]
        if k in ("x_target_arena", "x_global_arena", "label_arena", "row_weight") and rows_c is not None:
            g, w = g[rows_c], w[rows_c]
        assert torch.equal(_bits(g), _bits(w)), k


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_grouped_assembly_is_bitwise_the_composition(lib, shape, form, dtype):
    from news_recommendation_model_amd import ops
    t = _kernel_tables(FORMS[form], dtype)
    assert lib.nrm_assemble_form(t.static_cols, t.art_static.shape[1]) == (4 if form == "units" else 1)
    B, H, T, bounds, H_g, T_g = SHAPES[shape]
    host = tables.assemble_host(t, ORDER[CURSOR:CURSOR + 5], 40, 6)      # the cases are what they are said to be
    assert host["history_len"].tolist() == [0, 15, 31, 35, 40] and (6 - host["empty_num"]).tolist() == [1, 2, 4, 6, 6]
    assert host["label"][3].tolist() == [0, 0, 0, 0, 0, 1]             # the late target took the last slot
    dt = t.to("cuda")
    order_dev = torch.from_numpy(ORDER).cuda()
    tabs, R, N = _plan_tabs(B, H, T, bounds, H_g, T_g)
    ops.check_group_fit("cuda")
    ops.check_pad_errors("cuda")
    for keep in (True, False):
        got = _grouped(dt, order_dev, CURSOR, B, H, T, tabs, R, N, keep)
        _same(got, _composition(dt, order_dev, CURSOR, B, H, T, tabs, R, N, keep))
        # the last kept slot of a trimmed group carries the weight of the slots it stands for
        w = got["row_weight"].cpu().numpy()
        size = np.diff(bounds)
        want_w = np.concatenate([np.tile([1.0] * (tg - 1) + [float(T - tg + 1)], n) for n, tg in zip(size, T_g)])
        assert np.array_equal(w, want_w.astype(np.float32))
    ops.check_group_fit("cuda")                                        # nothing misfits, and the composition's own check agrees
    ops.check_pad_errors("cuda")
    ops.check_index_errors("cuda")


@pytest.mark.parametrize("axis", ["history", "candidates"])
def test_a_plan_too_tight_for_one_impression_raises_the_flag(lib, axis):
    """place 2 (31 events, 4 live candidates) under a group one quantum too low / one slot too narrow: the flag is raised, and every arena
    row outside that impression is what the composition under the same plan gives"""
    from news_recommendation_model_amd import ops
    t = _kernel_tables(Dims(), np.float32)
    dt = t.to("cuda")
    order_dev = torch.from_numpy(ORDER).cuda()
    B, H, T = 5, 40, 6
    bounds, H_g, T_g = ([0, 2, 3, 5], [16, 16, 40], [3, 5, 6]) if axis == "history" else ([0, 2, 3, 5], [16, 32, 40], [3, 4, 6])
    tabs, R, N = _plan_tabs(B, H, T, bounds, H_g, T_g)
    ops.check_group_fit("cuda")
    got = _grouped(dt, order_dev, CURSOR, B, H, T, tabs, R, N)
    with pytest.raises(ValueError, match="HAS BEEN APPLIED"):
        ops.check_group_fit("cuda")
    ops.check_group_fit("cuda")                                        # raised once, clear afterwards
    want = _composition(dt, order_dev, CURSOR, B, H, T, tabs, R, N)
    if axis == "candidates":                                           # the composition's own check sees the dropped live candidate too
        with pytest.raises(ValueError):
            ops.check_pad_errors("cuda")
    hro, cro = tabs[2].cpu().numpy(), tabs[4].cpu().numpy()
    rows_h = torch.tensor([r for r in range(R) if not hro[1] <= r < hro[2]], device="cuda")
    rows_c = torch.tensor([r for r in range(N) if not cro[1] <= r < cro[2]], device="cuda")
    assert 0 < rows_h.numel() < R and 0 < rows_c.numel() < N
    _same(got, want, rows_h, rows_c)
    # tables that do not add up (row offsets beyond the arenas): nothing is written outside, the flag says so
    bad = [tabs[0], tabs[1], _i32(hro + 17), tabs[3], _i32(cro + 5)]
    got = _grouped(dt, order_dev, CURSOR, B, H, T, bad, R, N)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.check_group_fit("cuda")
    ops.check_index_errors("cuda")


def test_opcheck_assemble_groups_at(lib):
    from news_recommendation_model_amd import ops
    t = _kernel_tables(Dims(), np.float32).to("cuda")
    B, H, T, bounds, H_g, T_g = SHAPES["three_groups"]
    tabs, R, N = _plan_tabs(B, H, T, bounds, H_g, T_g)
    args = ([getattr(t, n) for n in tables.TABLE_FIELDS], torch.from_numpy(ORDER).cuda(), torch.tensor([CURSOR], dtype=torch.int64, device="cuda"),
            B, H, T, True, int(t.static_cols), *tabs, R, N)
    torch.library.opcheck(torch.ops.nrm.assemble_groups_at.default, args)
    ops.check_group_fit("cuda")


# ---------------------------------------------------------------------------------------------------- the epoch
EB, EH, ET, EN = 8, 40, 6, 9 * 8 + 4
STEPS = 10                                                             # per epoch: nine full batches and a tail of 4
WARMUP = 3
MAX_GROUPS = 4
LR1 = 3e-4
PARAM_STEPS = 3
RECORD_SEED = 21
# impression i is of class i % 8: 0..2 a short history (at most 10 events) and at most 3 candidates, 3..4 a medium one (17..30) and at most
# 4 candidates, 5..7 a long one (at least 40).  In the table's own order every batch holds 3 + 2 + 3 of them, so the epoch plan is
# H_g = [16, 32, 40] over [3, 2, 3] places: 232 of 320 history rows.
# MEASURED on an MI355X before these gates were relied on: the existing eager compacted epoch (train_epochs_tables(compact_history=True,
# compact_candidates=True, max_groups=4)) against the dense eager epoch on this data and protocol -- both runs take over the dense run's
# states after the warm-up steps and after epoch 0, as the fixtures below do -- differs by 4.5e-8 relative in the record, 6.9e-8 relative in
# a step's loss and 1.4e-5 absolute in the parameters (history groups alone: 1.4e-8, 3.1e-7, 1.4e-5); the dense eager epoch against itself by
# 1.8e-8, 1.1e-7 and 2.3e-6.  None exceeds a third of its gate, so the gates are table_epoch's own.
GATES = {"record": FWD_TOL, "step": STEP_TOL, "param": PARAM_ATOL}


def make_data():
    from news_recommendation_model_amd import synth
    dims = Dims()
    rng = np.random.default_rng(RECORD_SEED)
    lens = np.concatenate([rng.integers(0, 11, 8), rng.integers(17, 31, 8), rng.integers(40, 61, 8)])
    cls = np.array([0, 0, 0, 1, 1, 2, 2, 2])[np.arange(EN) % 8]
    lists = np.where(cls == 0, rng.integers(1, 4, EN), np.where(cls == 1, rng.integers(2, 5, EN), rng.integers(2, 10, EN)))
    recs = synth.make_records(dims, 40, 24, EN, seed=RECORD_SEED, history_lens=lens, list_lens=lists)
    recs[2]["user_id"] = recs[1]["user_id"][8 * cls + rng.integers(0, 8, EN)]
    t = tables.ImpressionTables.from_records(*recs, dims, history_max=60)
    assert t.n_impressions == EN == 76
    L = t.history_len(np.arange(EN), EH)
    assert (L[cls == 0] <= 10).all() and ((L[cls == 1] >= 17) & (L[cls == 1] <= 30)).all() and (L[cls == 2] == EH).all()
    user_num = t.max_user_id + 1
    return dims, t, t.to("cuda"), synth.make_state_dict(dims, seed=1, user_num=user_num), user_num


@pytest.fixture(scope="module")
def data():
    return make_data()


def _plan(t, order, compact_candidates):
    return compact.plan_epoch_groups(t.history_len(np.arange(EN), EH), t.empty_num_all(ET), order, EB, EH, ET, True, compact_candidates,
                                     max_groups=MAX_GROUPS)


def test_the_epoch_plan_on_the_host(data):
    t = data[1]
    for cc in (False, True):
        plan = _plan(t, np.arange(EN), cc)
        assert not plan.dense                                          # (on the host, before any device run relies on it)
        assert plan.bounds.tolist() == [0, 3, 5, 8] and plan.H_g.tolist() == [16, 32, 40] and plan.R == 232 and plan.hist.saving == 1 - 232 / 320
        assert (plan.cand is not None) == cc
    assert plan.T_g.tolist() == [4, 5, 6] and plan.N == 12 + 10 + 18


def _fresh(data):
    from news_recommendation_model_amd import trainer
    dims, _t, _dt, sd, user_num = data
    model = trainer.build_model(dims, user_num, sd, device="cuda")
    return model, trainer.FlatAdam(model)


def eager_two_epochs(data, first=None, **compact_flags):
    """the eager table-fed loop over the tables' own order: epoch 0 at the default rate, epoch 1 at LR1 -- records, per-step losses, the
    state after the WARMUP steps of epoch 0 and after epoch 0, the parameters one step after the former and PARAM_STEPS steps after the
    latter.  ``first``: an earlier run whose two states this one takes over where that run saved them"""
    from news_recommendation_model_amd import trainer
    model, opt = _fresh(data)
    out = {"rec": [], "steps": [], "params": []}
    for e in range(2):
        if e == 1:
            opt.param_groups[0]["lr"] = LR1
            if first is not None:
                _load_state(model, opt, first["state0"])
        losses = []

        def on_batch(ep, i, loss, auc):
            losses.append(loss)
            if (e, i) == (0, WARMUP - 1):
                if first is not None:
                    _load_state(model, opt, first["state_w"])
                out["state_w"] = _save_state(model, opt)
            if (e, i) in ((0, WARMUP), (1, PARAM_STEPS - 1)):
                out["params"].append(opt.flat_param.detach().clone())
        out["rec"] += trainer.train_epochs_tables(model, opt, data[2], 1, EB, EH, ET, shuffle=False, on_batch=on_batch, **compact_flags)
        out["steps"].append([float(x) for x in losses])
        if e == 0:
            out["state0"] = _save_state(model, opt)
    assert opt.steps == 2 * STEPS and len(out["params"]) == 2
    return out


def differences(got, ref):
    """the three quantities the gates are on: record (relative), per-step loss of epoch 0 behind the warm-up (relative), parameters (absolute)"""
    rec = max(_rel(g[k], r[k]) for g, r in zip(got["rec"], ref["rec"]) for k in ("loss_avg", "auc_avg"))
    step = max(_rel(got["steps"][0][k], ref["steps"][0][k]) for k in range(WARMUP, STEPS - 1))
    par = max(float((x - y).abs().max()) for x, y in zip(got["params"], ref["params"]))
    return {"record": rec, "step": step, "param": par}


@pytest.fixture(scope="module")
def eager(data):
    return eager_two_epochs(data)


@pytest.fixture(scope="module", params=["history", "history_candidates"])
def grouped(request, data, eager):
    """a GroupedTableEpoch driven by hand over the same two epochs, looked at after every step; it takes over the dense eager run's states
    after the warm-up steps and after epoch 0"""
    from news_recommendation_model_amd import trainer
    _dims, t, dt, _sd, _ = data
    cc = request.param == "history_candidates"
    model, opt = _fresh(data)
    runner = trainer.GroupedTableEpoch(model, opt, dt, EB, EH, ET, warmup=WARMUP, compact_history=True, compact_candidates=cc, max_groups=MAX_GROUPS)
    out = {"rec": [], "params": [], "ids": [], "orders": [], "counters": [], "cc": cc, "steps": []}
    for e in range(2):
        if e == 1:
            opt.param_groups[0]["lr"] = LR1
            _load_state(model, opt, eager["state0"])
        runner.begin_epoch(np.arange(EN))
        assert not runner.plan.dense and (runner.plan.cand is not None) == cc
        ids = []
        for k in range(STEPS):
            runner.step()
            ids.append(runner.batch["impression_id"].cpu().numpy().copy())
            if (e, k) == (0, WARMUP - 1):
                _load_state(model, opt, eager["state_w"])
            if (e, k) in ((0, WARMUP), (1, PARAM_STEPS - 1)):
                out["params"].append(opt.flat_param.detach().clone())
        rec = runner.end_epoch()
        out["rec"].append(dict(rec, loss_avg=rec["loss_sum"] / EN, auc_avg=rec["auc_sum"] / EN))
        out["steps"].append(rec["step_loss"])
        out["ids"].append(ids)
        out["orders"].append(runner.plan.order.copy())
        out["counters"].append((runner.eager_steps, runner.replays, runner.captures, runner.replans))
    out["opt_steps"] = opt.steps
    return out


def test_every_impression_once_in_sorted_batches(lib, data, grouped):
    _dims, t, _dt, _sd, _ = data
    L = t.history_len(np.arange(EN), EH)
    for e in range(2):
        order = grouped["orders"][e]
        assert sorted(order.tolist()) == list(range(EN))
        for k in range(STEPS):
            sel = order[k * EB:(k + 1) * EB]
            assert np.array_equal(grouped["ids"][e][k], t.imp_id[sel]), (e, k)
            assert sorted(sel.tolist()) == list(range(k * EB, min((k + 1) * EB, EN)))        # batch membership is the caller's
            if k < STEPS - 1:
                assert (np.diff(L[sel]) >= 0).all()
        assert sorted(np.concatenate(grouped["ids"][e]).tolist()) == sorted(t.imp_id.tolist())
        rec = grouped["rec"][e]
        assert rec["impressions"] == EN and rec["steps"] == STEPS and rec["one_class_rows"] == 0
    assert grouped["opt_steps"] == 2 * STEPS
    # epoch 0: WARMUP grouped eager steps, one capture, six replays, the dense eager tail.  Epoch 1: the same order fits the plan, so the
    # second capture is the learning rate's alone (one plan in all) and every full batch is a replay
    assert grouped["counters"] == [(WARMUP + 1, 9 - WARMUP, 1, 1), (WARMUP + 2, 2 * 9 - WARMUP, 2, 1)]
    assert grouped["counters"][0][1] >= 5


def test_grouped_epochs_land_where_the_dense_eager_loop_lands(lib, eager, grouped):
    diff = differences(grouped, eager)
    print(f"grouped captured ({'history + candidate' if grouped['cc'] else 'history'} groups) against dense eager: record {diff['record']:.3g} "
          f"relative, step loss {diff['step']:.3g} relative, parameters {diff['param']:.3g} absolute")
    for e in range(2):
        for k in ("loss_avg", "auc_avg"):
            assert _rel(grouped["rec"][e][k], eager["rec"][e][k]) <= GATES["record"], (e, k)
        assert torch.allclose(grouped["params"][e], eager["params"][e], rtol=0, atol=GATES["param"]), e
    for k in range(WARMUP, STEPS - 1):                                 # the replays of epoch 0 against the dense eager steps
        assert _rel(grouped["steps"][0][k], eager["steps"][0][k]) <= GATES["step"], k
    # both checks can fail: the first replay moved some weight by more than the tolerance, and the steps of epoch 1 at the first capture's
    # rate would have moved some weight further than the tolerance allows
    assert float((eager["params"][0] - eager["state_w"]["opt"][0]).abs().max()) > 1.5 * GATES["param"]
    moved = float((eager["params"][1] - eager["state0"]["opt"][0]).abs().max())
    assert moved * (1e-3 / LR1 - 1) > 2 * GATES["param"], moved


def test_train_epochs_tables_grouped_record(lib, data, eager):
    from news_recommendation_model_amd import trainer
    model, opt = _fresh(data)
    got = trainer.train_epochs_tables(model, opt, data[2], 1, EB, EH, ET, shuffle=False, graph="grouped", graph_warmup=WARMUP, compact_history=True,
                                      compact_candidates=True, max_groups=MAX_GROUPS)
    assert opt.steps == STEPS and len(got) == 1
    g, w = got[0], eager["rec"][0]
    assert set(g) == {"epoch", "lr", "impressions", "loss_avg", "auc_avg", "top1_avg", "step_loss", "step_auc"}
    assert g["impressions"] == EN and g["lr"] == 1e-3 and len(g["step_loss"]) == STEPS
    # epoch 0 of the eager fixture took over no state: the same weights, the same impressions, batch by batch
    for k in ("loss_avg", "auc_avg"):
        assert _rel(g[k], w[k]) <= GATES["record"], (k, g[k], w[k])


def test_a_second_epoch_that_does_not_fit_is_planned_again(lib, data):
    """an order that gives batch 0 a fourth long history in place of a short one does not fit the first epoch's plan: a new plan, the
    warm-up step again on the new shapes, a new capture -- and the epoch still consumes every impression once"""
    from news_recommendation_model_amd import trainer
    _dims, t, dt, _sd, _ = data
    model, opt = _fresh(data)
    runner = trainer.GroupedTableEpoch(model, opt, dt, EB, EH, ET, warmup=1, max_groups=MAX_GROUPS, min_saving=0.1)
    rec = runner.run_epoch(np.arange(EN))
    assert (runner.replans, runner.captures, runner.replays, runner.eager_steps) == (1, 1, 8, 2) and rec["impressions"] == EN
    order = np.arange(EN)
    order[[0, 13]] = order[[13, 0]]                                    # a long history of batch 1 for a short one of batch 0
    assert not runner.plan.fits(runner._hist_len, runner._empty, order)
    rec = runner.run_epoch(order)
    assert (runner.replans, runner.captures, runner.replays, runner.eager_steps) == (2, 2, 16, 4)
    assert rec["impressions"] == EN and rec["steps"] == STEPS and rec["one_class_rows"] == 0
    assert runner.plan.H_g.tolist() == [16, 32, 40] and runner.plan.bounds.tolist() == [0, 2, 4, 8] and not runner.plan.dense
