"""GPU: batches assembled on the device from resident tables.  Every assembly case asserts EXACT equality with
tables.assemble_host (floats compared as bits; for float32 tables with the float64 host rows cast to float32): both forms of the kernel, both
table types, every history length and slot-rule case, the fixture's bucket borders, clamping of a bad selection; then the assembled batch
through the downstream ops and a seeded model against the uploaded host batch, and train_epochs_tables against train_epochs."""
import numpy as np
import pytest
import torch

from golden_util import rel_err
from tables_util import border_tables, history_tables, seeded_tables, slot_tables
from news_recommendation_model_amd import tables
from news_recommendation_model_amd.config import Dims

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-3              # dense against compact in test_gpu_history_train.py / test_gpu_candidate_train.py
# eval forward, assembled float32 batch against the uploaded float64 host batch: the kernels convert a float64 input to fp32 as they read it
# and the table values ARE fp32 numbers, so both runs see the same fp32 inputs; 128 ulp of the largest logit allows for nothing but that
EVAL_TOL = 128 * 2.0 ** -24
FLOATS = ("x_history", "x_target", "x_global")
DIMS = {"default": Dims(), "P6": Dims(pca_vector=6), "emb400": Dims.for_emb(400)}


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _check(dev, host, ft):
    assert set(dev) == set(tables.BATCH_KEYS)
    for k in tables.BATCH_KEYS:
        want = torch.from_numpy(np.ascontiguousarray(host[k]))
        if k in FLOATS:
            want = want.to(ft)
        got = dev[k].cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, want.dtype, got.shape, want.shape)
        assert torch.equal(_bits(got) if got.is_floating_point() else got, _bits(want) if want.is_floating_point() else want), k


def _assemble(t, sel, H, T, keep=True, dt=None):
    dt = t.to("cuda") if dt is None else dt
    return tables.assemble_batch(dt, torch.as_tensor(np.asarray(sel, dtype=np.int64)).cuda(), H, T, keep)


@pytest.mark.parametrize("name", list(DIMS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_assembly_is_bitwise_the_host_rows(lib, name, dtype):
    """both forms (80 / 78 and 416 / 414 columns in 16-byte units, 22 / 20 element by element), both table types; a selection with
    repeats, in reverse; more than one wave of history rows and a last wave that is not full"""
    dims = DIMS[name]
    t = seeded_tables(dims, dtype)
    assert lib.nrm_assemble_form(t.static_cols, t.art_static.shape[1]) == (1 if name == "P6" else 4)
    dt, ft = t.to("cuda"), torch.float32 if dtype == np.float32 else torch.float64
    n = t.n_impressions
    sel = np.concatenate([np.arange(n)[::-1], [3, 3, 0, n - 1]])
    for H, T, keep in ((17, 5, True), (17, 5, False), (30, 15, True), (3, 33, False)):
        dev = _assemble(t, sel, H, T, keep, dt)
        assert dev["x_history"].shape == (sel.shape[0], H, dims.history_cols) and dev["x_target"].shape == (sel.shape[0], T, dims.target_cols)
        _check(dev, tables.assemble_host(t, sel, H, T, keep), ft)
    again = _assemble(t, sel, 17, 5, True, dt)
    first = _assemble(t, sel, 17, 5, True, dt)
    assert all(torch.equal(again[k], first[k]) for k in tables.BATCH_KEYS)


@pytest.mark.parametrize("B", [0, 1, 5])
def test_batch_sizes(lib, B):
    t = seeded_tables(dtype=np.float32)
    sel = np.arange(B) * 7 % max(t.n_impressions, 1)
    dev = _assemble(t, sel, 17, 5)
    assert dev["x_history"].shape == (B, 17, 80) and dev["history_len"].shape == (B,)
    _check(dev, tables.assemble_host(t, sel, 17, 5), torch.float32)


@pytest.mark.parametrize("H", [1, 3, 17, 200])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_history_lengths(lib, H, dtype):
    """users with 0, 1, H-1, H and H+5 events"""
    t = history_tables(H, dtype=dtype)
    sel = np.arange(t.n_impressions)
    host = tables.assemble_host(t, sel, H, 3)
    assert sorted(set(host["history_len"].tolist())) == sorted({0, min(1, H), H - 1, H})
    _check(_assemble(t, sel, H, 3), host, torch.float32 if dtype == np.float32 else torch.float64)


@pytest.mark.parametrize("T", [1, 2, 15])
def test_slot_rule_cases(lib, T):
    """target among the first T-1, at T-1, later, absent, duplicated, none; lists of 0, 1, T-1, T, T+1, 3T entries; both slot rules"""
    for labelled in (True, False):
        t, cases = slot_tables(T, dtype=np.float32, labelled=labelled)
        dt, sel = t.to("cuda"), np.arange(t.n_impressions)
        for keep in (True, False):
            _check(_assemble(t, sel, 4, T, keep, dt), tables.assemble_host(t, sel, 4, T, keep), torch.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bucket_borders(lib, dtype):
    """the fixture's border times, the inputs on which integer arithmetic on the microseconds gives other buckets first"""
    t, delta = border_tables(dtype=dtype)
    sel = np.arange(t.n_impressions)
    dev = _assemble(t, sel, 1, 1)
    _check(dev, tables.assemble_host(t, sel, 1, 1), torch.float32 if dtype == np.float32 else torch.float64)
    want = torch.from_numpy(tables.time_buckets(delta)).to(dev["x_history"].dtype)
    assert torch.equal(dev["x_history"][:, 0, :4].cpu(), want) and torch.equal(dev["x_target"][:, 0, :4].cpu(), want)


def test_downstream_ops_read_the_padding(lib):
    """ops.history_len of the assembled rows is the emitted history_len; candidate_gather_groups accepts the padded candidates"""
    from news_recommendation_model_amd import compact, ops
    for dtype in (np.float32, np.float64):
        t = seeded_tables(dtype=dtype, list_lens=np.tile([1, 2, 3, 9], 12))
        sel = np.arange(t.n_impressions)
        dev = _assemble(t, sel, 17, 5)
        assert torch.equal(ops.history_len(dev["x_history"]), dev["history_len"])
        assert (dev["history_len"] == 0).any() and (dev["history_len"] == 17).any() and (dev["empty_num"] > 0).any()
        cand = compact.plan_candidate_groups(dev["empty_num"].cpu().numpy(), 5, max_groups=4)
        assert not cand.dense
        plan = compact.full_height_history_plan(cand, 17)
        tabs, ctabs = plan.upload("cuda"), cand.upload("cuda")
        ops.check_pad_errors("cuda")
        xt_a, xg_a, lab_a, roww = ops.candidate_gather_groups(dev["x_target"], dev["x_global"], dev["label"], tabs["perm"], tabs["bounds"],
                                                              ctabs["row_off"], ctabs["T_g"], cand.N)
        ops.check_pad_errors("cuda")                                   # every dropped cell equals its impression's padded candidate, bit for bit
        assert xt_a.shape[0] == cand.N < sel.shape[0] * 5 and float(roww.sum()) == sel.shape[0] * 5


def test_a_selection_outside_the_table_is_clamped_and_flagged(lib):
    from news_recommendation_model_amd import ops
    t = seeded_tables(dtype=np.float32)
    n = t.n_impressions
    ops.check_index_errors("cuda")
    dev = _assemble(t, [2, n + 3, -1, n - 1], 17, 5)
    with pytest.raises(IndexError):
        ops.check_index_errors("cuda")
    _check(dev, tables.assemble_host(t, [2, n - 1, 0, n - 1], 17, 5), torch.float32)
    ops.check_index_errors("cuda")                                     # cleared; a good selection leaves it alone
    _assemble(t, [0, 1], 17, 5)
    ops.check_index_errors("cuda")


# ---------------------------------------------------------------------------------------------------- end to end, B = 8, H = 17, T = 5
B, H, T = 8, 17, 5


@pytest.fixture(scope="module")
def e2e():
    from news_recommendation_model_amd import synth
    dims = Dims()
    recs = synth.make_records(dims, 40, 12, 16, seed=21, max_history=25, list_lens=np.tile([1, 2, 1, 9, 1, 3, 2, 6], 2), max_list=9)
    t = tables.ImpressionTables.from_records(*recs, dims, history_max=30)
    assert t.n_impressions == 16
    user_num = t.max_user_id + 1
    return dims, t, t.to("cuda"), synth.make_state_dict(dims, seed=1, user_num=user_num), user_num


def _host_batch(t, sel):
    from news_recommendation_model_amd import trainer
    host = tables.assemble_host(t, sel, H, T)
    return host, trainer.batch_to_device(host, "cuda")


def test_eval_forward_on_the_assembled_batch(lib, e2e):
    from news_recommendation_model_amd import trainer
    dims, t, dt, sd, user_num = e2e
    sel = np.arange(B)
    model = trainer.build_model(dims, user_num, sd, device="cuda").eval()
    dev = _assemble(t, sel, H, T, True, dt)
    _host, up = _host_batch(t, sel)
    assert dev["x_history"].dtype == torch.float32 and up["x_history"].dtype == torch.float64
    with torch.no_grad():
        a = model(dev["x_history"], dev["x_target"], dev["x_global"]).float().cpu().numpy()
        b = model(up["x_history"], up["x_target"], up["x_global"]).float().cpu().numpy()
    print(f"eval forward, assembled float32 against uploaded float64: rel err {rel_err(a, b):.3g}, bit-equal {np.array_equal(a, b)}")
    assert np.isfinite(b).all() and np.abs(b).max() > 0 and rel_err(a, b) <= EVAL_TOL


@pytest.mark.parametrize("flags", [{}, dict(compact_history=True, compact_candidates=True, max_groups=4), dict(compact_candidates=True, max_groups=4)],
                         ids=["dense", "both flags", "candidates"])
def test_train_step_on_the_assembled_batch(lib, e2e, flags):
    """one step on the loader's batch (with the producer's lengths attached) against the dense step on the uploaded host batch.  At H = 17
    the history planner (quantum 16) has nothing to drop, so with both flags the step plans from the known lengths and runs dense; with
    compact_candidates alone the candidate arenas are really trimmed (asserted on the plan)."""
    from news_recommendation_model_amd import compact, trainer
    dims, t, dt, sd, user_num = e2e
    sel = np.arange(B, 2 * B)
    dev = trainer.attach_known_lengths(_assemble(t, sel, H, T, True, dt), t.history_len(sel, H), t.empty_num_all(T)[sel])
    host, up = _host_batch(t, sel)
    assert np.array_equal(host["empty_num"], t.empty_num_all(T)[sel]) and (host["history_len"] < H).any()
    assert not compact.plan_candidate_groups(host["empty_num"], T, max_groups=4).dense
    runs = []
    for batch, kw in ((up, {}), (dev, flags)):
        model = trainer.build_model(dims, user_num, sd, device="cuda").train()
        loss, out = trainer.train_step(model, trainer.FlatAdam(model), batch, **kw)
        runs.append((float(loss), out.float().cpu().numpy()))
    (l0, o0), (l1, o1) = runs
    print(f"train_step {flags or 'dense'}: loss {l0:.9g} / {l1:.9g}, out rel err {rel_err(o1, o0):.3g}")
    assert o1.shape == (B, T) and abs(l1 - l0) <= FWD_TOL * abs(l0) and rel_err(o1, o0) < FWD_TOL
    torch.cuda.synchronize()


def test_loader_yields_the_keys_the_drivers_read(lib, e2e):
    dims, t, dt, _sd, _ = e2e
    loader = tables.TableLoader(dt, B, H, T, shuffle=True, seed=5)
    order = np.random.default_rng(5).permutation(t.n_impressions)
    assert len(loader) == 2 and np.array_equal(loader.order(), order)
    for i, batch in enumerate(loader):
        sel = order[i * B:(i + 1) * B]
        _check({k: batch[k] for k in tables.BATCH_KEYS}, tables.assemble_host(t, sel, H, T), torch.float32)
        host, _done, addr, ver = batch["history_len_host"]
        assert host.tolist() == t.history_len(sel, H).tolist() and (addr, ver) == (batch["x_history"].data_ptr(), batch["x_history"]._version)
        assert np.array_equal(batch["empty_num_host"][0], batch["empty_num"].cpu().numpy())


def test_train_epochs_tables_is_train_epochs_over_the_same_batches(lib, e2e):
    from news_recommendation_model_amd import trainer
    dims, t, dt, sd, user_num = e2e
    rng = np.random.default_rng(3)
    orders = [rng.permutation(t.n_impressions) for _ in range(2)]
    epoch = iter(orders)

    def make_loader():
        order = next(epoch)
        return [tables.assemble_host(t, order[i:i + B], H, T) for i in range(0, t.n_impressions, B)]
    model = trainer.build_model(dims, user_num, sd, device="cuda")
    want = trainer.train_epochs(model, trainer.FlatAdam(model), make_loader, 2)
    model = trainer.build_model(dims, user_num, sd, device="cuda")
    got = trainer.train_epochs_tables(model, trainer.FlatAdam(model), dt, 2, B, H, T, shuffle=True, seed=3)
    print("train_epochs:", want, "\ntrain_epochs_tables:", got)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g["epoch"] == w["epoch"] and g["lr"] == w["lr"] and g["impressions"] == w["impressions"] == 16
        for k in ("loss_avg", "auc_avg"):
            assert abs(g[k] - w[k]) <= FWD_TOL * abs(w[k]), (k, g[k], w[k])
