"""GPU: the record of an evaluation pass (epoch.hip: eval_tally_kernel through the C ABI nrm_eval_tally, alone) against
table_scoring_util.tally_reference: the float64 sums to association, everything else exactly -- counts, cursor, every record row with its
zero-filled columns, the rows a wrapped ring overwrites and the ones it leaves, the rows past the end of the pass that are neither
written nor counted, the guard rows behind every buffer -- in the labelled, the label-free and the record-free form, and bit for bit
again on a second run."""
import numpy as np
import pytest
import torch

from table_scoring_util import GUARD, tally_reference

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257]                                           # below, at and above one wave; more than one row per thread
WIDTHS = [(1, 1), (5, 3), (64, 64), (65, 64)]                          # (T, Tp)
G32 = GUARD & 0x7FFFFFFF


def _steps(B, Tp, seed, labels=True):
    rng = np.random.default_rng(seed)
    steps = []
    for i in range(3):
        auc = rng.random(B).astype(np.float32)
        auc[rng.random(B) < 0.15 if B > 1 else np.array([i == 1])] = -1.0
        metrics = (0.05 + 0.95 * rng.random((B, 3))).astype(np.float32)
        metrics[rng.random(B) < 0.15 if B > 1 else np.array([i == 2])] = -1.0
        step = dict(rank=rng.integers(0, Tp + 1, (B, Tp)).astype(np.int32), live=rng.integers(0, Tp + 1, B).astype(np.int32),
                    impression_id=rng.integers(1, 2 ** 62, B).astype(np.int64), auc=None, top1=None, metrics=None)
        if labels:
            step.update(auc=auc, top1=rng.integers(0, 2, B).astype(np.int32), metrics=metrics)
        steps.append(step)
    return steps


def _run(steps, T, n_order, cap):
    """the three steps through the C ABI -> host copies of (state [cursor | sums | counts | guard], rec_rank, rec_live, rec_id), each record
    buffer one guard row longer than ``cap``"""
    from news_recommendation_model_amd import native
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()      # noqa: E731
    p = lambda t: None if t is None else native.ptr(t)      # noqa: E731
    state = torch.zeros(11, dtype=torch.int64, device="cuda")
    state[10] = GUARD
    rec_rank = torch.full((cap + 1, T), G32, dtype=torch.int32, device="cuda")
    rec_live = torch.full((cap + 1,), G32, dtype=torch.int32, device="cuda")
    rec_id = torch.full((cap + 1,), GUARD, dtype=torch.int64, device="cuda")
    cursor, sums, counts = state[0:1], state[1:6], state[6:10]
    for s in steps:
        t = {k: dev(v) for k, v in s.items()}
        B, Tp = s["rank"].shape
        native.call("nrm_eval_tally", p(t["auc"]), p(t["top1"]), p(t["metrics"]), p(t["rank"]), p(t["live"]), p(t["impression_id"]), B, T, Tp,
                    p(cursor), n_order, p(sums), p(counts), p(rec_rank) if cap else None, p(rec_live) if cap else None,
                    p(rec_id) if cap else None, cap, native.stream_ptr())
    torch.cuda.synchronize()
    return state.cpu(), rec_rank.cpu().numpy(), rec_live.cpu().numpy(), rec_id.cpu().numpy()


def _compare(got, want, B, cap, T):
    state, rec_rank, rec_live, rec_id = got
    sums = state[1:6].view(torch.float64).numpy()
    print(f"sums {sums.tolist()} reference {want['sums'].tolist()} counts {state[6:10].tolist()} cursor {int(state[0])}")
    for k in (0, 2, 3, 4):                                             # association only: B * 2^-52 relative
        assert abs(sums[k] - want["sums"][k]) <= B * 2.0 ** -52 * abs(want["sums"][k]), (k, sums[k], want["sums"][k])
    assert sums[1] == want["sums"][1]
    assert state[6:10].tolist() == want["counts"].tolist() and int(state[0]) == want["cursor"]
    assert int(state[10]) == GUARD                                     # nothing behind the state
    assert np.array_equal(rec_rank[:cap], want["rec_rank"]) and np.array_equal(rec_live[:cap], want["rec_live"])
    assert np.array_equal(rec_id[:cap], want["rec_id"])
    assert (rec_rank[cap] == G32).all() and rec_live[cap] == G32 and rec_id[cap] == GUARD       # nothing behind the ring


@pytest.mark.parametrize("width", WIDTHS, ids=[f"T{t}_Tp{tp}" for t, tp in WIDTHS])
@pytest.mark.parametrize("B", SIZES)
def test_tally_record_and_sums(lib, B, width):
    """a ring of 2 B rows under three steps of B: the third wraps onto the first's rows, and its last rows overhang the pass"""
    T, Tp = width
    over = max(1, B // 4)
    n_order, cap = 3 * B - over, 2 * B
    steps = _steps(B, Tp, seed=1000 * B + T)
    want = tally_reference(steps, T, n_order, cap)
    assert want["counts"][3] == n_order and want["cursor"] == 3 * B    # the overhanging rows are not counted, the cursor still moves by B
    if B > 1:
        assert want["counts"][0] > 0 and want["counts"][1] > 0
        # the ring after the wrap: rows of the third step, then what the first step left where the third did not reach, then the second
        assert np.array_equal(want["rec_id"][:B - over], steps[2]["impression_id"][:B - over])
        assert np.array_equal(want["rec_id"][B - over:B], steps[0]["impression_id"][B - over:])
        assert np.array_equal(want["rec_id"][B:], steps[1]["impression_id"])
    else:
        assert want["rec_id"].tolist() == [steps[0]["impression_id"][0], steps[1]["impression_id"][0]]    # the third step lies outside
    if Tp < T:
        assert (want["rec_rank"][:, Tp:] == 0).all()
    got = _run(steps, T, n_order, cap)
    _compare(got, want, B, cap, T)
    again = _run(steps, T, n_order, cap)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, again))        # the same bits on a second run


@pytest.mark.parametrize("B", [1, 65, 257])
def test_tally_without_labels_and_without_a_record(lib, B):
    T, Tp = 5, 3
    steps = _steps(B, Tp, seed=B, labels=False)
    want = tally_reference(steps, T, 3 * B, 3 * B)
    assert not want["sums"].any() and want["counts"].tolist() == [0, 0, 3, 3 * B]
    _compare(_run(steps, T, 3 * B, 3 * B), want, B, 3 * B, T)
    # metrics only: no record buffers at all (cap = 0); the third step lies wholly behind a pass of 2 B impressions
    steps = _steps(B, Tp, seed=B + 1)
    want = tally_reference(steps, T, 2 * B, 0)
    _compare(_run(steps, T, 2 * B, 0), want, B, 0, T)
    assert want["counts"][3] == 2 * B


def test_host_side_refusals(lib):
    """refused by value before any launch, with the library's message; the cursor has not moved"""
    from news_recommendation_model_amd import native
    B, T, Tp, cap = 4, 5, 3, 8
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")      # noqa: E731
    auc, top1, met, rank, live, ids = z(B, torch.float32), z(B, torch.int32), z(3 * B, torch.float32), z(B * Tp, torch.int32), z(B, torch.int32), z(B, torch.int64)
    state, rr, rl, ri = z(10, torch.int64), z(cap * T, torch.int32), z(cap, torch.int32), z(cap, torch.int64)
    p = native.ptr
    good = [p(auc), p(top1), p(met), p(rank), p(live), p(ids), B, T, Tp, p(state[0:1]), 100, p(state[1:6]), p(state[6:10]), p(rr), p(rl), p(ri), cap,
            native.stream_ptr()]

    def refused(match, **change):
        names = ("auc", "top1", "metrics", "rank", "live", "impression_id", "B", "T", "Tp", "cursor", "n_order", "sums", "counts", "rec_rank",
                 "rec_live", "rec_id", "cap", "stream")
        args = [change.get(n, v) for n, v in zip(names, good)]
        with pytest.raises(RuntimeError, match=match):
            native.call("nrm_eval_tally", *args)
    refused("NULL together", top1=None)
    refused("NULL together", auc=None)
    refused("NULL together with cap = 0", rec_live=None)
    refused("NULL together with cap = 0", cap=0)
    refused("NULL together with cap = 0", rec_rank=None, rec_live=None, rec_id=None)
    refused("exceeds T", Tp=T + 1)
    refused("no multiple of B", cap=6)
    refused("needs rank, live and impression_id", rank=None)
    refused("null cursor", cursor=None)
    native.call("nrm_eval_tally", *good)                               # the unchanged arguments pass
    native.call("nrm_eval_tally", *[0 if i == 6 else v for i, v in enumerate(good)])      # B = 0 launches nothing
    torch.cuda.synchronize()
    assert int(state[0]) == B and state[6:10].tolist() == [0, 0, 1, B]
