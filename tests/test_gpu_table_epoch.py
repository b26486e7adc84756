"""GPU: the captured table-fed epoch.  The assemble kernel at a device-side cursor against tables.assemble_host, bit
for bit, clamping at both ends of ``order`` included; the epoch tally against the host's float64 arithmetic; and trainer.GraphedTableEpoch /
train_epochs_tables(graph=True) against the eager table-fed loop on the same impressions in the same order."""
import numpy as np
import pytest
import torch

from tables_util import seeded_tables, slot_tables
from news_recommendation_model_amd import tables
from news_recommendation_model_amd.config import Dims

pytestmark = pytest.mark.gpu

FLOATS = ("x_history", "x_target", "x_global")
FORMS = {"units": Dims(), "elements": Dims(pca_vector=6)}             # 80 / 78 columns in 16-byte units, 22 / 20 element by element


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t


def _check(dev, host, ft, rows=None):
    """EXACT equality of a device batch with assemble_host's dict (floats as bits), on all rows or on ``rows``"""
    assert set(dev) == set(tables.BATCH_KEYS)
    for k in tables.BATCH_KEYS:
        want = torch.from_numpy(np.ascontiguousarray(host[k]))
        if k in FLOATS:
            want = want.to(ft)
        got = dev[k].cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, want.dtype, got.shape, want.shape)
        if rows is not None:
            got, want = got[rows], want[rows]
        assert torch.equal(_bits(got), _bits(want)), k


def _order(n, seed=11):
    """a seeded permutation of all n impressions with one repeat"""
    perm = np.random.default_rng(seed).permutation(n)
    return np.concatenate([perm, perm[3:4]]).astype(np.int64)


def _at(dt, order_dev, c, B, H, T, keep=True):
    return tables.assemble_batch_at(dt, order_dev, torch.tensor([c], dtype=torch.int64, device="cuda"), B, H, T, keep)


# ---------------------------------------------------------------------------------------------------- assembly at a cursor (eager)
B, H, T = 5, 17, 5


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_cursor_assembly_is_bitwise_the_host_rows(lib, form, dtype):
    from news_recommendation_model_amd import ops
    t = seeded_tables(FORMS[form], dtype)
    assert lib.nrm_assemble_form(t.static_cols, t.art_static.shape[1]) == (4 if form == "units" else 1)
    dt, ft = t.to("cuda"), torch.float32 if dtype == np.float32 else torch.float64
    order = _order(t.n_impressions)
    n = order.shape[0]
    assert n > 3 * B
    order_dev = torch.from_numpy(order).cuda()
    ops.check_index_errors("cuda")
    for c in (0, B, n - B):
        dev = _at(dt, order_dev, c, B, H, T)
        _check(dev, tables.assemble_host(t, order[c:c + B], H, T), ft)
        # the old entry on the same impressions: the same bits
        old = tables.assemble_batch(dt, order_dev[c:c + B].clone(), H, T)
        assert all(torch.equal(_bits(old[k]), _bits(dev[k])) for k in tables.BATCH_KEYS)
    ops.check_index_errors("cuda")                                     # nothing in range raises the flag
    for c in (n - B + 2, -1):
        dev = _at(dt, order_dev, c, B, H, T)
        with pytest.raises(IndexError):
            ops.check_index_errors("cuda")
        ops.check_index_errors("cuda")                                 # raised once, clear afterwards
        pos = c + np.arange(B)
        inside = np.nonzero((pos >= 0) & (pos < n))[0]
        assert 0 < inside.shape[0] < B
        host = tables.assemble_host(t, order[np.clip(pos, 0, n - 1)], H, T)
        _check(dev, host, ft, rows=torch.from_numpy(inside))           # the rows whose position is in range
        _check(dev, host, ft)                                          # ... and the others are the rows of the clamped position


def test_cursor_far_outside_is_clamped_not_followed(lib):
    """a cursor beyond either end by more than a batch (and by more than int64 addition could take): every row is the clamped end's"""
    from news_recommendation_model_amd import ops
    t = seeded_tables(dtype=np.float32)
    dt = t.to("cuda")
    order = _order(t.n_impressions)
    n = order.shape[0]
    order_dev = torch.from_numpy(order).cuda()
    ops.check_index_errors("cuda")
    for c, end in ((n, n - 1), (n + 1000, n - 1), (2 ** 63 - 1, n - 1), (-B, 0), (-2 ** 63, 0)):
        dev = _at(dt, order_dev, c, B, H, T)
        with pytest.raises(IndexError):
            ops.check_index_errors("cuda")
        _check(dev, tables.assemble_host(t, np.full(B, order[end]), H, T), torch.float32)
    ops.check_index_errors("cuda")


@pytest.mark.parametrize("shape", [(17, 1), (17, 2), (1, 5)], ids=["T1", "T2", "H1"])
def test_cursor_assembly_single_wave_shapes(lib, shape):
    """T in {1, 2} under both slot rules and H = 1: one wave per impression and row kind, a candidate wave with a single slot"""
    H_, T_ = shape
    t, _cases = slot_tables(max(T_, 2), dtype=np.float32)
    dt = t.to("cuda")
    order = _order(t.n_impressions, seed=2)
    n = order.shape[0]
    order_dev = torch.from_numpy(order).cuda()
    for keep in (True, False):
        for c in (0, n - B):
            _check(_at(dt, order_dev, c, B, H_, T_, keep), tables.assemble_host(t, order[c:c + B], H_, T_, keep), torch.float32)


# ---------------------------------------------------------------------------------------------------- the tally
LOG_CAP = 2
GUARD = 0x5A5A5A5A5A5A5A5A


def _tally_inputs(B_, seed):
    rng = np.random.default_rng(seed)
    calls = []
    for i in range(3):
        auc = rng.random(B_).astype(np.float32)
        one_class = rng.random(B_) < 0.15 if B_ > 1 else np.array([i == 1])
        auc[one_class] = -1.0
        calls.append((np.float32(0.3 + rng.random()), auc, rng.integers(0, 2, B_).astype(np.int32)))
    return calls


def _run_tally(calls):
    from news_recommendation_model_amd import ops
    state = torch.zeros(6 + LOG_CAP + 1, dtype=torch.int64, device="cuda")
    state[-1] = GUARD                                                  # one guard row behind the log
    cursor, sums, counts = state[0:1], state[1:4].view(torch.float64), state[4:6]
    log = state[6:6 + LOG_CAP].view(torch.float32).view(LOG_CAP, 2)
    for loss, auc, top1 in calls:
        ops.epoch_tally(torch.tensor(loss, device="cuda"), torch.from_numpy(auc).cuda(), torch.from_numpy(top1).cuda(), cursor, sums, counts, log)
    return state.cpu()


@pytest.mark.parametrize("B_", [1, 63, 64, 65, 255, 257, 1027])
def test_tally_is_the_hosts_float64_record(lib, B_):
    calls = _tally_inputs(B_, seed=B_)
    state = _run_tally(calls)
    sums, log = state[1:4].view(torch.float64).numpy(), state[6:6 + LOG_CAP].view(torch.float32).view(LOG_CAP, 2).numpy()
    s0, s1, hits, bad = np.float64(0.0), np.float64(0.0), 0, 0
    means = []
    for loss, auc, top1 in calls:
        s0 = s0 + np.float64(loss) * np.float64(B_)                    # train.py:82, one rounded product and one rounded sum per step
        ok = auc >= 0
        part = np.sum(auc[ok].astype(np.float64))
        s1 = s1 + part
        means.append(part / ok.sum() if ok.any() else np.float64(0.0))
        hits += int(top1.sum())
        bad += int((~ok).sum())
    assert bad > 0 and (hits > 0 or B_ == 1)
    print(f"B={B_}: sums {sums.tolist()} host {[float(s0), float(s1), hits]}, auc sum off by {abs(sums[1] - s1) / s1:.3g} relative")
    assert sums[0] == s0                                               # EQUAL: the host can restate the loss sum exactly
    assert abs(sums[1] - s1) <= B_ * 2.0 ** -52 * s1                   # association only
    assert sums[2] == hits and int(state[4]) == bad and int(state[5]) == 3 and int(state[0]) == 3 * B_
    for k in range(LOG_CAP):
        assert log[k, 0].view(np.int32) == calls[k][0].view(np.int32)                    # the loss, bit for bit
        assert abs(np.float64(log[k, 1]) - means[k]) <= np.spacing(np.float32(means[k])), (k, log[k, 1], means[k])      # rounded once
    assert int(state[-1]) == GUARD                                     # the third step did not write behind the log
    assert torch.equal(_run_tally(calls), state)                       # the same bits from run to run


# ---------------------------------------------------------------------------------------------------- the captured epoch
EB, EH, ET, EN = 8, 17, 5, 5 * 8 + 3
STEPS = 6                                                              # per epoch: five full batches and a tail of 3
WARMUP = 2
FWD_TOL = 1e-3              # the record of train_epochs_tables against train_epochs in test_gpu_tables.py
STEP_TOL = 1e-4             # a replayed step's loss against the eager step's   } test_graphed_train_step_replays_like_eager:
PARAM_ATOL = 5e-4           # parameters                                         } the same noise source, float-atomic order
LR1 = 3e-4
# Where the parameters are compared.  Adam divides a gradient by its own running size, so the float-atomic noise of a gradient that nearly
# cancels (one user's ``delta`` entry) comes out at the scale of the rate: the eager loop against ITSELF was, in separate runs, 3e-6 and
# 7e-5 apart after three steps from fresh weights and 7e-5 .. 1.5e-4 after an epoch at 1e-3 -- not ten times below PARAM_ATOL.  The runs are
# shortened, not the tolerance widened; every comparison starts from ONE common state taken from the first eager run:
#   - the FIRST REPLAY of epoch 0, one step from the state after the WARMUP eager steps (eager against eager: 4e-9 after one step);
#   - the first PARAM_STEPS steps of epoch 1 -- replays of a graph captured again at LR1 -- from the state after epoch 0 (eager against
#     eager at that rate: 7e-9 after three steps, 6e-6 .. 2e-5 after the six of the epoch).
# test_eager_spread_is_far_below_the_tolerances holds the second eager run, started from the same states, to a tenth of the tolerance.
PARAM_STEPS = 3
# (auc_avg is discrete: one flipped pair moves it by 0.25 / 43, more than FWD_TOL allows.  Should a near-tie flip a pair between two runs,
# the eager spread printed by test_eager_spread_is_far_below_the_tolerances shows it, and the remedy is another RECORD_SEED, not a tolerance.)
RECORD_SEED = 21
SEEDS = (3, 4)                                                         # the TableLoader seed of epoch 0 and of epoch 1


@pytest.fixture(scope="module")
def data():
    from news_recommendation_model_amd import synth
    dims = Dims()
    recs = synth.make_records(dims, 40, 12, EN, seed=RECORD_SEED, max_history=25, max_list=9)
    t = tables.ImpressionTables.from_records(*recs, dims, history_max=30)
    assert t.n_impressions == EN == 43
    user_num = t.max_user_id + 1
    return dims, t, t.to("cuda"), synth.make_state_dict(dims, seed=1, user_num=user_num), user_num


def _fresh(data):
    from news_recommendation_model_amd import trainer
    dims, _t, _dt, sd, user_num = data
    model = trainer.build_model(dims, user_num, sd, device="cuda")
    return model, trainer.FlatAdam(model)


def _save_state(model, opt):
    return {"opt": [getattr(opt, k).detach().clone() for k in ("flat_param", "exp_avg", "exp_avg_sq", "state")],
            "buffers": [b.detach().clone() for b in model.buffers()]}


def _load_state(model, opt, state):
    """weights, both Adam moments, the step counter and BatchNorm's running statistics, in place (a captured graph keeps its addresses)"""
    from news_recommendation_model_amd import ops
    with torch.no_grad():
        for k, src in zip(("flat_param", "exp_avg", "exp_avg_sq", "state"), state["opt"]):
            getattr(opt, k).copy_(src)
        for b, src in zip(model.buffers(), state["buffers"]):
            b.copy_(src)
    ops.repack_persistent(opt.params)                                  # (the cached weight images follow the weights, as after a step)


def _eager_two_epochs(data, first=None):
    """epoch 0 at the default rate, epoch 1 at LR1: records, per-step losses, the state after the WARMUP steps of epoch 0 and after epoch 0,
    the parameters one step after the former and PARAM_STEPS steps after the latter.  ``first``: an earlier run whose two states this one
    takes over where that run saved them"""
    from news_recommendation_model_amd import trainer
    model, opt = _fresh(data)
    out = {"rec": [], "steps": [], "params": []}
    for e, seed in enumerate(SEEDS):
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
        out["rec"] += trainer.train_epochs_tables(model, opt, data[2], 1, EB, EH, ET, seed=seed, on_batch=on_batch)
        out["steps"].append([float(x) for x in losses])
        if e == 0:
            out["state0"] = _save_state(model, opt)
    assert opt.steps == 2 * STEPS and len(out["params"]) == 2
    return out


@pytest.fixture(scope="module")
def eager(data):
    first = _eager_two_epochs(data)
    return first, _eager_two_epochs(data, first)


@pytest.fixture(scope="module")
def graphed(data, eager):
    """a GraphedTableEpoch driven by hand over the same two epochs, looked at after every step; it takes over the first eager run's states
    after the warm-up steps and after epoch 0, as the second eager run does"""
    from news_recommendation_model_amd import trainer
    _dims, t, dt, _sd, _ = data
    model, opt = _fresh(data)
    runner = trainer.GraphedTableEpoch(model, opt, dt, EB, EH, ET, warmup=WARMUP)
    out = {"rec": [], "params": [], "ids": [], "orders": [], "replayed": None, "counters": []}
    for e, seed in enumerate(SEEDS):
        if e == 1:
            opt.param_groups[0]["lr"] = LR1
            _load_state(model, opt, eager[0]["state0"])
        order = np.random.default_rng(seed).permutation(EN)
        runner.begin_epoch(order)
        ids = []
        for k in range(STEPS):
            runner.step()
            ids.append(runner.batch["impression_id"].cpu().numpy().copy())
            if (e, k) == (0, WARMUP - 1):
                _load_state(model, opt, eager[0]["state_w"])
            if (e, k) in ((0, WARMUP), (1, PARAM_STEPS - 1)):
                out["params"].append(opt.flat_param.detach().clone())
            if (e, k) == (1, 3):                                       # a replay of epoch 2: after the in-place refill of ``order``
                out["replayed"] = {key: v.clone() for key, v in runner.batch.items()}
        out["rec"].append(runner.end_epoch())
        out["ids"].append(ids)
        out["orders"].append(order)
        out["counters"].append((runner.eager_steps, runner.replays, runner.captures))
    out["steps"] = opt.steps
    return out


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_eager_spread_is_far_below_the_tolerances(lib, eager):
    """the eager loop against ITSELF: what the comparisons below may rely on is at least ten times above this"""
    a, b = eager
    rec = max(_rel(x[k], y[k]) for x, y in zip(a["rec"], b["rec"]) for k in ("loss_avg", "auc_avg"))
    step = max(_rel(x, y) for xs, ys in zip(a["steps"], b["steps"]) for x, y in zip(xs, ys))
    par = [float((x - y).abs().max()) for x, y in zip(a["params"], b["params"])]
    print(f"eager against eager from common states: record {rec:.3g} relative, step loss {step:.3g} relative, parameters {par[0]:.3g} absolute one "
          f"step after the warm-up, {par[1]:.3g} after {PARAM_STEPS} steps of epoch 1")
    assert 10 * rec <= FWD_TOL and 10 * step <= STEP_TOL and 10 * max(par) <= PARAM_ATOL


def test_every_impression_once_and_the_cursor_moves_inside_the_graph(lib, data, graphed):
    _dims, t, _dt, _sd, _ = data
    for e in range(2):
        order = graphed["orders"][e]
        for k in range(STEPS):
            assert np.array_equal(graphed["ids"][e][k], t.imp_id[order[k * EB:(k + 1) * EB]]), (e, k)
        assert sorted(np.concatenate(graphed["ids"][e]).tolist()) == sorted(t.imp_id.tolist())
        rec = graphed["rec"][e]
        assert rec["impressions"] == EN and rec["steps"] == STEPS and rec["one_class_rows"] == 0       # (impressions IS the cursor)
        assert len(rec["step_loss"]) == len(rec["step_auc"]) == STEPS
    assert graphed["steps"] == 2 * STEPS                               # (the common state of epoch 1 carries the count of six steps)
    # the first epoch: WARMUP eager steps, one capture, replays, the eager tail; the second: the rate changed, so one more capture, and
    # every full batch is a replay
    assert graphed["counters"] == [(WARMUP + 1, 5 - WARMUP, 1), (WARMUP + 2, 2 * 5 - WARMUP, 2)]
    _check(graphed["replayed"], tables.assemble_host(t, graphed["orders"][1][3 * EB:4 * EB], EH, ET), torch.float32)


def test_hand_driven_epochs_land_where_the_eager_loop_lands(lib, eager, graphed):
    ref = eager[0]
    for e in range(2):
        got = graphed["rec"][e]
        loss_avg, auc_avg = got["loss_sum"] / EN, got["auc_sum"] / EN
        print(f"epoch {e}: captured loss_avg {loss_avg:.9g} auc_avg {auc_avg:.9g}, eager {ref['rec'][e]['loss_avg']:.9g} {ref['rec'][e]['auc_avg']:.9g}; "
              f"parameters ({'after the first replay' if e == 0 else 'after %d replays at LR1' % PARAM_STEPS}) differ by "
              f"{float((graphed['params'][e] - ref['params'][e]).abs().max()):.3g}")
        assert _rel(loss_avg, ref["rec"][e]["loss_avg"]) <= FWD_TOL and _rel(auc_avg, ref["rec"][e]["auc_avg"]) <= FWD_TOL
        # epoch 1 ran at LR1 in both: a graph that kept the rate of its first capture lands elsewhere (an Adam step scales with the rate)
        assert torch.allclose(graphed["params"][e], ref["params"][e], rtol=0, atol=PARAM_ATOL), e
    for k in range(WARMUP, 5):                                         # the replays of epoch 0 against the eager steps
        assert _rel(graphed["rec"][0]["step_loss"][k], ref["steps"][0][k]) <= STEP_TOL, k
    # both checks can fail.  The replay moved some weight by more than the tolerance (a replay that did nothing is caught); and the steps of
    # epoch 1 moved some weight by ``moved`` at LR1, so at the first capture's rate they would have moved it by moved * 1e-3 / LR1
    assert float((ref["params"][0] - ref["state_w"]["opt"][0]).abs().max()) > 1.5 * PARAM_ATOL
    moved = float((ref["params"][1] - ref["state0"]["opt"][0]).abs().max())
    assert moved * (1e-3 / LR1 - 1) > 2 * PARAM_ATOL, moved


def test_train_epochs_tables_graph_record(lib, data, eager):
    from news_recommendation_model_amd import trainer
    dt = data[2]
    model, opt = _fresh(data)
    got = trainer.train_epochs_tables(model, opt, dt, 2, EB, EH, ET, seed=SEEDS[0], graph=True, graph_warmup=WARMUP)
    model_e, opt_e = _fresh(data)
    want = trainer.train_epochs_tables(model_e, opt_e, dt, 2, EB, EH, ET, seed=SEEDS[0])
    print("captured:", [{k: v for k, v in r.items() if not k.startswith("step_")} for r in got], "\neager:", want)
    assert opt.steps == opt_e.steps == 2 * STEPS and len(got) == 2
    sizes = [EB] * 5 + [EN - 5 * EB]
    for g, w in zip(got, want):
        assert set(g) == {"epoch", "lr", "impressions", "loss_avg", "auc_avg", "top1_avg", "step_loss", "step_auc"}
        assert g["epoch"] == w["epoch"] and g["lr"] == w["lr"] == 1e-3 and g["impressions"] == w["impressions"] == EN
        assert len(g["step_loss"]) == len(g["step_auc"]) == STEPS and 0.0 <= g["top1_avg"] <= 1.0
        s = np.float64(0.0)
        for loss, n in zip(g["step_loss"], sizes):
            s = s + np.float64(np.float32(loss)) * np.float64(n)
        assert g["loss_avg"] == float(s) / EN                          # the device's sum restated on the host from the returned log
        for k in ("loss_avg", "auc_avg"):
            assert _rel(g[k], w[k]) <= FWD_TOL, (k, g[k], w[k])
    # epoch 0 drew the permutation the fixture's eager run drew (one seed, one generator)
    assert _rel(got[0]["loss_avg"], eager[0]["rec"][0]["loss_avg"]) <= FWD_TOL
    opt.param_groups[0]["lr"] = LR1
    more = trainer.train_epochs_tables(model, opt, dt, 1, EB, EH, ET, seed=SEEDS[1], graph=True, graph_warmup=WARMUP)
    assert more[0]["lr"] == LR1 and more[0]["impressions"] == EN and opt.steps == 3 * STEPS


def test_one_class_rows_raise_at_the_epochs_end(lib):
    """an impression whose target is not in its list has one class in its row: the eager loop's ValueError, at the epoch's end"""
    from news_recommendation_model_amd import synth, trainer
    dims = Dims()
    recs = synth.make_records(dims, 40, 12, 2 * EB, seed=5, max_history=25, max_list=9, absent_target_frac=0.5)
    t = tables.ImpressionTables.from_records(*recs, dims, history_max=30)
    assert (tables.assemble_host(t, np.arange(t.n_impressions), EH, ET)["label"].sum(axis=1) == 0).any()
    user_num = t.max_user_id + 1
    model = trainer.build_model(dims, user_num, synth.make_state_dict(dims, seed=1, user_num=user_num), device="cuda")
    with pytest.raises(ValueError, match="Only one class present"):
        trainer.train_epochs_tables(model, trainer.FlatAdam(model), t, 1, EB, EH, ET, graph=True, graph_warmup=1)


def test_a_step_past_the_epochs_end_is_refused_on_the_host(lib, data):
    from news_recommendation_model_amd import trainer
    model, opt = _fresh(data)
    runner = trainer.GraphedTableEpoch(model, opt, data[2], EB, EH, ET, warmup=1)
    runner.begin_epoch(np.arange(EN))
    with pytest.raises(RuntimeError, match="left in the epoch"):
        runner.step(EB + 1)
    with pytest.raises(ValueError, match="order"):
        runner.begin_epoch(np.arange(EN - 1))
