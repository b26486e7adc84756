"""CPU: the captured epoch on compacted batches as far as it goes without a device -- the epoch planner
(``compact.plan_epoch_groups``: one static group plan that every full batch of an epoch fits), the additive C entry's host validation, the
op's fake function, and the errors of ``train_epochs_tables(graph="grouped")`` / ``GroupedTableEpoch``."""
import ctypes

import numpy as np
import pytest
import torch

from tables_util import seeded_tables
from news_recommendation_model_amd import compact, tables
from news_recommendation_model_amd.config import Dims


def _lengths(rng, n, H, T):
    """history lengths (a fifth at H or beyond, some empty) and empty_num of n impressions"""
    L = np.clip(rng.gamma(1.3, 0.35 * H, n).astype(np.int64), 0, H + 5)
    L[rng.random(n) < 0.05] = 0
    return L, rng.integers(0, T + 1, n)


def _batches(L, n, order, B):
    nb = order.shape[0] // B
    full = order[:nb * B].reshape(nb, B)
    return L[full], n[full]


CASES = [(8, 40, 6, 76, 4, True, False), (8, 40, 6, 76, 4, True, True), (8, 40, 6, 76, 3, False, True), (16, 200, 15, 16 * 12 + 5, 2, True, True),
         (5, 17, 5, 43, 64, True, True), (1, 1, 1, 3, 4, True, True), (64, 200, 15, 640, 4, True, False)]


@pytest.mark.parametrize("B,H,T,N,max_groups,ch,cc", CASES)
def test_every_full_batch_fits_and_no_height_can_be_lowered(B, H, T, N, max_groups, ch, cc):
    rng = np.random.default_rng(B * 1000 + N + max_groups)
    L, empty = _lengths(rng, N, H, T)
    order = rng.permutation(N)
    plan = compact.plan_epoch_groups(L, empty, order, B, H, T, ch, cc, max_groups=max_groups, min_saving=0.0)
    Lc, n = np.clip(L, 0, H), T - np.clip(empty, 0, T)
    # the order: batch membership unchanged, every full batch ascending in its key (stable), the tail untouched
    nb = N // B
    assert plan.n_batches == nb and plan.order.shape == (N,) and np.array_equal(plan.order[nb * B:], order[nb * B:])
    key = Lc if ch else n
    for i in range(nb):
        mine, theirs = plan.order[i * B:(i + 1) * B], order[i * B:(i + 1) * B]
        assert sorted(mine.tolist()) == sorted(theirs.tolist())
        assert np.array_equal(mine, theirs[np.argsort(key[theirs], kind="stable")])
    assert 1 <= plan.G <= max_groups and plan.bounds[0] == 0 and plan.bounds[-1] == B and (np.diff(plan.bounds) > 0).all()
    Lb, nb_ = _batches(Lc, n, plan.order, B)
    size = np.diff(plan.bounds)
    h_pos, t_pos = np.repeat(plan.H_g, size), np.repeat(plan.T_g, size)
    assert (((Lb < h_pos) | (h_pos == H)) & ((nb_ < t_pos) | (t_pos == T))).all()                    # every full batch fits ...
    assert plan.fits(L, empty, order) and plan.fits(L, empty, plan.order)
    for g in range(plan.G):                                                                          # ... and nothing can be lowered
        lo, hi = plan.bounds[g], plan.bounds[g + 1]
        if ch:
            q = plan.quantum
            assert plan.H_g[g] % q == 0 or plan.H_g[g] == H
            lower = plan.H_g[g] - q if plan.H_g[g] % q == 0 else (plan.H_g[g] // q) * q              # the next height down
            assert lower < 1 or (Lb[:, lo:hi] >= lower).any(), (g, plan.H_g[g])
        else:
            assert plan.H_g[g] == H
        if cc:
            assert plan.T_g[g] == min(T, 1 + nb_[:, lo:hi].max())
        else:
            assert plan.T_g[g] == T
    assert (plan.cand is not None) == bool(cc and (plan.T_g < T).any()) and plan.hist.cand is plan.cand


@pytest.mark.parametrize("B,H,T,N,max_groups,ch,cc", CASES[:5])
def test_plan_has_the_shape_of_the_per_batch_plans(B, H, T, N, max_groups, ch, cc):
    """perm is the identity, and row_off, R, N and expand are what plan_history_groups / plan_candidate_groups give a batch that attains the
    envelope (each position as long as its longest occupant over the epoch) -- cut along the same groups"""
    rng = np.random.default_rng(7 * B + N)
    L, empty = _lengths(rng, N, H, T)
    order = rng.permutation(N)
    plan = compact.plan_epoch_groups(L, empty, order, B, H, T, ch, cc, max_groups=max_groups)
    ident = np.arange(B)
    assert np.array_equal(plan.hist.perm, ident) and np.array_equal(plan.hist.inverse, ident)
    Lb, nb_ = _batches(np.clip(L, 0, H), T - np.clip(empty, 0, T), plan.order, B)
    env_L, env_n = Lb.max(axis=0), nb_.max(axis=0)
    assert np.array_equal(plan.hist.hist_len, env_L if ch else np.full(B, H))
    if ch:
        ref = compact.plan_history_groups(env_L, H, max_groups=max_groups, quantum=plan.quantum)
        assert np.array_equal(ref.perm, ident)                                                    # (the envelope is sorted already)
        for k in ("bounds", "H_g", "w_g", "row_off"):
            assert np.array_equal(getattr(plan.hist, k), getattr(ref, k)), k
        assert plan.R == plan.hist.R == ref.R and abs(plan.hist.saving - ref.saving) < 1e-12
        cref = compact.plan_candidate_groups(T - env_n, T, history_plan=ref) if cc else None
    else:
        cref = compact.plan_candidate_groups(T - env_n, T, max_groups=max_groups)
        assert np.array_equal(cref.perm, ident)
        full = compact.full_height_history_plan(cref, H)
        for k in ("bounds", "H_g", "w_g", "row_off"):
            assert np.array_equal(getattr(plan.hist, k), getattr(full, k)), k
        assert plan.R == B * H
    if plan.cand is not None:
        assert np.array_equal(plan.cand.perm, ident) and np.array_equal(plan.cand.inverse, ident)
        for k in ("bounds", "T_g", "w_g", "row_off", "expand", "count"):
            assert np.array_equal(getattr(plan.cand, k), getattr(cref, k)), k
        assert plan.N == plan.cand.N == cref.N and abs(plan.saving - cref.saving) < 1e-12
        assert np.array_equal(plan.expand, cref.expand) and np.array_equal(plan.cand_row_off, cref.row_off)
    else:
        assert plan.N == B * T and np.array_equal(plan.expand, np.arange(B * T)) and np.array_equal(plan.cand_row_off, plan.bounds * T)
    assert plan.hist_row_off[-1] == plan.R and plan.cand_row_off[-1] == plan.N
    assert plan.hist_row_off.dtype == plan.T_g.dtype == plan.expand.dtype == np.int32


def test_fits_is_false_once_a_length_passes_its_group():
    B, H, T, N = 8, 40, 6, 76
    rng = np.random.default_rng(3)
    L = np.tile(np.array([3, 9, 10, 17, 30, 40, 44, 60]), 10)[:N]
    empty = np.where(np.arange(N) % 8 < 3, 3 + np.arange(N) % 3, rng.integers(0, T + 1, N))      # the short histories: at most 3 candidates
    order = np.arange(N)
    plan = compact.plan_epoch_groups(L, empty, order, B, H, T, True, True, max_groups=4)
    assert plan.T_g.tolist() == [4, 6, 6]
    assert plan.H_g.tolist() == [16, 32, 40] and plan.bounds.tolist() == [0, 3, 5, 8] and plan.R == 232 and not plan.dense
    assert plan.fits(L, empty, order)
    worse = L.copy()
    worse[0] = 16                                                      # 16 events need 17 rows: a fourth impression of batch 0 beyond 16
    assert not plan.fits(worse, empty, order)
    worse = L.copy()
    worse[75] = 16                                                     # ... in the partial batch, which runs dense: it still fits
    assert plan.fits(worse, empty, order)
    g = int(np.argmin(plan.T_g))
    assert plan.T_g[g] < T                                             # (these counts leave a group trimmed in the candidate axis)
    fewer = empty.copy()
    fewer[plan.order[plan.bounds[g]]] = T - plan.T_g[g]                # a member of that group gets T_g live candidates
    assert not plan.fits(L, fewer, order)
    # another epoch over the same classes (3 + 2 + 3 to a batch, in another order) fits; one that mixes the classes does not
    again = np.concatenate([rng.permutation(8) + 8 * i for i in rng.permutation(9)] + [np.arange(72, 76)])
    assert plan.fits(L, empty, again)
    mixed = np.concatenate([np.arange(0, 72).reshape(9, 8).T.reshape(-1), np.arange(72, 76)])      # batches of one class each
    assert not plan.fits(L, empty, mixed)


def test_dense_rule_and_degenerate_epochs():
    B, H, T = 8, 40, 6
    full = np.full(24, H)
    none = np.zeros(24, dtype=np.int64)
    plan = compact.plan_epoch_groups(full, none, np.arange(24), B, H, T, True, True)
    assert plan.dense and plan.G == 1 and plan.saving == 0.0 and plan.cand is None and plan.R == B * H and plan.N == B * T
    short = np.full(24, 3)
    plan = compact.plan_epoch_groups(short, none, np.arange(24), B, H, T, True, False)
    assert not plan.dense and plan.H_g.tolist() == [16] and abs(plan.saving - 0.6) < 1e-12
    assert compact.plan_epoch_groups(short, none, np.arange(24), B, H, T, True, False, min_saving=0.7).dense
    assert not compact.plan_epoch_groups(np.full(24, 25), none, np.arange(24), B, H, T, True, False, min_saving=0.1).dense      # 0.2
    assert compact.plan_epoch_groups(np.full(24, 25), none, np.arange(24), B, H, T, True, False).dense                          # < MIN_SAVING
    few = compact.plan_epoch_groups(short[:5], none[:5], np.arange(5), B, H, T, True, True)                # no full batch at all
    assert few.dense and few.n_batches == 0 and np.array_equal(few.order, np.arange(5)) and few.fits(short[:5], none[:5], np.arange(5))
    with pytest.raises(ValueError, match="neither"):
        compact.plan_epoch_groups(short, none, np.arange(24), B, H, T, False, False)
    with pytest.raises(ValueError, match="max_groups"):
        compact.plan_epoch_groups(short, none, np.arange(24), B, H, T, True, False, max_groups=65)
    with pytest.raises(IndexError):
        compact.plan_epoch_groups(short, none, np.arange(25), B, H, T, True, False)


@pytest.mark.parametrize("B,max_groups", [(256, 4), (1024, 4), (256, 2), (1024, 2)])
def test_epoch_plan_keeps_most_of_the_per_batch_saving(B, max_groups):
    """24 576 lengths of mean about 92 at H = 200, quantum 16: the epoch-wide plan saves within 0.07 of the mean per-batch plan"""
    N, H, T = 24576, 200, 15
    rng = np.random.default_rng(0)
    L = np.clip(rng.gamma(1.2, 92 / 1.2, N).astype(np.int64), 0, H)
    assert 80 < L.mean() < 100
    order = rng.permutation(N)
    plan = compact.plan_epoch_groups(L, np.zeros(N, dtype=np.int64), order, B, H, T, True, False, max_groups=max_groups)
    per_batch = np.mean([compact.plan_history_groups(L[order[i * B:(i + 1) * B]], H, max_groups=max_groups).saving for i in range(N // B)])
    print(f"B={B} max_groups={max_groups}: epoch plan saves {plan.saving:.3f}, per-batch plans {per_batch:.3f}")
    assert not plan.dense and per_batch - 0.07 <= plan.saving <= per_batch + 1e-12


def test_grouped_graph_errors_and_the_pinned_refusals():
    from news_recommendation_model_amd import trainer
    run = lambda **kw: trainer.train_epochs_tables(None, None, None, 1, 8, 17, 5, **kw)       # noqa: E731
    with pytest.raises(ValueError, match="compact_history=True and / or compact_candidates=True"):
        run(graph="grouped")
    with pytest.raises(RuntimeError, match="captured step"):                                  # graph=True refuses as before
        run(graph=True, compact_history=True)
    with pytest.raises(RuntimeError, match="captured step"):
        run(graph=True, compact_candidates=True, max_groups=4)
    with pytest.raises(RuntimeError, match="step_loss and step_auc"):
        run(graph="grouped", compact_history=True, on_batch=lambda *a: None)
    G = trainer.GroupedTableEpoch
    with pytest.raises(ValueError, match="neither"):
        G(None, None, None, 8, 17, 5, compact_history=False)
    class Hooked:
        def compact_history_applies(self):
            return False
    with pytest.raises(RuntimeError, match="forward_grouped"):                                # a model that does not take the grouped forward
        G(Hooked(), None, None, 8, 17, 5)

    class NoRowWeight:
        def compact_history_applies(self):
            return True

        def compact_candidates_applies(self):
            return False
    with pytest.raises(RuntimeError, match="row-weight form"):
        G(NoRowWeight(), None, None, 8, 17, 5, compact_candidates=True)
    with pytest.raises(TypeError, match="GroupedTableEpoch needs trainer.FlatAdam"):          # the sibling's constructor checks
        G(NoRowWeight(), object(), None, 8, 17, 5)
    opt = trainer.FlatAdam.__new__(trainer.FlatAdam)
    with pytest.raises(ValueError, match="at least one eager step"):
        G(NoRowWeight(), opt, None, 8, 17, 5, warmup=0)
    with pytest.raises(TypeError, match="GraphedTableEpoch needs trainer.FlatAdam"):
        trainer.GraphedTableEpoch(None, object(), None, 8, 17, 5)


def test_groups_entry_validates_on_the_host(lib):
    from news_recommendation_model_amd import native
    assert lib.nrm_abi_version() == 7 and native.ABI_VERSION == 7                            # additive: the version stays
    at = lib.nrm_assemble_groups_at
    d, g = native.AssembleTables(), native.AssembleGroups()
    p, q = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), ctypes.cast(ctypes.pointer(g), ctypes.c_void_p)
    assert at(p, None, None, 5, None, 1, 2, 2, 1, None) != 0 and b"null group struct" in lib.nrm_last_error()
    assert at(None, q, None, 5, None, 1, 2, 2, 1, None) != 0 and b"nrm_assemble_groups_at: null table struct" in lib.nrm_last_error()
    assert at(p, q, None, 0, None, 0, 2, 2, 1, None) == 0                                    # B = 0: nothing to launch
    assert at(p, q, None, 5, None, 1, 2, 2, 1, None) != 0 and b"null pointer (cursor)" in lib.nrm_last_error()
    word = ctypes.c_long(0)
    cur = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    buf = (ctypes.c_double * 8)()
    a = ctypes.cast(buf, ctypes.c_void_p).value                                              # (a host address: never read, nothing is launched)
    d.A = d.U = d.N = 1
    d.static_cols, d.S = 74, 76
    for name, _ in native.AssembleTables._fields_:
        if name not in ("A", "U", "E", "N", "L", "S", "static_cols", "is_f64"):
            setattr(d, name, a)
    for G, R, N in ((0, 1, 1), (65, 1, 1), (1, 0, 1), (1, 1, 0), (1, 5, 1), (1, 1, 3)):      # B * H = 4, B * T = 2
        g.G, g.R, g.N = G, R, N
        assert at(p, q, a, 5, cur, 1, 4, 2, 1, None) != 0 and b"G=%d R=%d N=%d" % (G, R, N) in lib.nrm_last_error()
    g.G, g.R, g.N = 1, 4, 2
    assert at(p, q, a, 5, cur, 1, 4, 2, 1, None) != 0 and b"null pointer (group tables)" in lib.nrm_last_error()


def test_groups_op_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from news_recommendation_model_amd import ops
    assert "assemble_groups_at" in ops.OPS and ops.assemble_groups_at is torch.ops.nrm.assemble_groups_at
    t = seeded_tables(Dims(pca_vector=6), dtype=np.float32)
    cpu = [torch.from_numpy(getattr(t, n)) for n in tables.TABLE_FIELDS]
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nrm.assemble_groups_at(cpu, torch.zeros(9, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 2, 3, 2, True, t.static_cols,
                                         i32(0, 2), i32(3), i32(0, 6), i32(2), i32(0, 4), 6, 4)
    with FakeTensorMode():
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")            # noqa: E731
        order, cursor = new((48,), torch.int64), new((1,), torch.int64)
        tabs = [new((4,), torch.int32), new((3,), torch.int32), new((4,), torch.int32), new((3,), torch.int32), new((4,), torch.int32)]
        for ft in (torch.float32, torch.float64):
            fake = [new(c.shape, ft if c.is_floating_point() else c.dtype) for c in cpu]
            out = torch.ops.nrm.assemble_groups_at(fake, order, cursor, 5, 40, 6, True, t.static_cols, *tabs, 152, 23)
            assert [(tuple(o.shape), o.dtype) for o in out] == [
                ((152, 22), ft), ((23, 20), ft), ((23, 3), ft), ((23,), torch.float64), ((23,), torch.float32), ((5, 6), torch.float64),
                ((5, 6), torch.int64), ((5,), torch.int64), ((5,), torch.int64), ((5,), torch.int64), ((5,), torch.int32)]
        with pytest.raises(RuntimeError, match="assemble_groups_at"):                       # more rows than the dense batch has
            torch.ops.nrm.assemble_groups_at(fake, order, cursor, 5, 40, 6, True, t.static_cols, *tabs, 201, 23)
        with pytest.raises(RuntimeError, match="assemble_groups_at"):                       # bounds is [G + 1]
            torch.ops.nrm.assemble_groups_at(fake, order, cursor, 5, 40, 6, True, t.static_cols, tabs[1], *tabs[1:], 152, 23)
        with pytest.raises(RuntimeError, match="cursor"):
            torch.ops.nrm.assemble_groups_at(fake, order, new((1,), torch.int32), 5, 40, 6, True, t.static_cols, *tabs, 152, 23)
    with pytest.raises(RuntimeError, match="host arrays"):
        tables.assemble_groups_at(t, torch.zeros(9, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 2, 3, 2, None)
