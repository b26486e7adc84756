"""GPU: the fused scoring tail (nrm_ensemble_rank / torch.ops.nrm.ensemble_rank), predict_ranked / validate_ranked and the
test-set driver score_dataset (reference test.py:31-132).

Reference for the scores: the documented formula evaluated in FLOAT64 PyTorch here, from the same fp32 logits -- never the
kernel.  Gate: rtol = 1e-5, atol = 1e-7 elementwise on live columns, the project's gate for two evaluations of the same scores
(test_predict_follows_test_py_semantics); the fp32 ATen formulation sits at 0.017 of it against float64 on these inputs.
Ranks are exact.  Metrics: 1e-6 absolute (values in [0, 1]; the gate row_auc is held to)."""
import os
import zipfile

import numpy as np
import pytest
import torch

from golden_util import load_case

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-7
T_GRID = (1, 2, 5, 30, 100, 257, 1024)


def _inputs(T, M, B=11, seed=0):
    """fp32 logits clamp(4 randn, -10, 10) of M models and random trailing padding, rows with n = T included."""
    g = torch.Generator().manual_seed(1000 * T + 10 * M + seed)
    logits = [torch.clamp(4 * torch.randn(B, T, generator=g), -10, 10) for _ in range(M)]
    empty = torch.randint(0, T, (B,), generator=g, dtype=torch.int32)          # n = T - empty in [1, T]
    empty[::3] = 0                                                               # rows without padding: no second softmax
    return logits, empty


def _ref_scores(logits, empty):
    """float64: softmax per model over all T columns, mean in model order, second softmax over the de-padded slice."""
    B, T = logits[0].shape
    out = None
    for x in logits:
        p = torch.softmax(x.double(), dim=1)
        out = p if out is None else out + p
    out = out / len(logits)
    score = torch.zeros(B, T, dtype=torch.float64)
    for b in range(B):
        n = T - (int(empty[b]) if empty is not None else 0)
        score[b, :n] = torch.softmax(out[b, :n], dim=0) if n < T else out[b]
    return score


def _run(logits, empty, label=None):
    out = torch.ops.nrm.ensemble_rank([x.cuda() if not x.is_cuda else x for x in logits],
                                      empty.cuda() if empty is not None else None, label.cuda() if label is not None else None)
    torch.cuda.synchronize()
    return out


def _check_scores(score, live, logits, empty, what):
    B, T = logits[0].shape
    ref = _ref_scores([x.cpu() for x in logits], empty)
    n = T - (empty.long() if empty is not None else torch.zeros(B, dtype=torch.long))
    assert live.dtype == torch.int32 and torch.equal(live.cpu().long(), n), what
    got = score.cpu().double()
    mask = torch.arange(T)[None, :] < n[:, None]
    err = (got - ref).abs()
    worst = float((err[mask] / (ATOL + RTOL * ref[mask].abs())).max())
    print(f"{what}: worst |err| / (atol + rtol |ref|) = {worst:.4f}")
    assert worst <= 1.0, (what, worst)
    assert bool((got[~mask] == 0).all()), what                                   # padding columns are exactly 0


def _check_ranks(score, rank, live, what):
    from news_recommendation_model_amd import evaluation
    s, r, nn = score.cpu(), rank.cpu(), live.cpu()
    assert r.dtype == torch.int32
    for b in range(s.shape[0]):
        n = int(nn[b])
        assert r[b, :n].tolist() == evaluation.rank_row(s[b, :n].tolist()), (what, b)
        assert bool((r[b, n:] == 0).all()), (what, b)


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("T", T_GRID)
def test_scores_and_ranks_on_the_grid(lib, T, M):
    logits, empty = _inputs(T, M)
    score, rank, live, metrics = _run(logits, empty)
    assert tuple(metrics.shape) == (0, 3)
    _check_scores(score, live, logits, empty, f"T={T} M={M}")
    _check_ranks(score, rank, live, f"T={T} M={M}")


@pytest.mark.parametrize("T", [5, 30, 100])
def test_scores_without_empty_and_from_a_column_slice(lib, T):
    logits, empty = _inputs(T, 2, seed=1)
    score, rank, live, _ = _run(logits, None)                                    # empty = None: n = T everywhere
    _check_scores(score, live, logits, None, f"T={T} empty=None")
    _check_ranks(score, rank, live, f"T={T} empty=None")
    # a column slice of a wider tensor, as predict's trim produces: row stride T + 3, no copy is needed
    wide = [torch.cat([x, torch.full((x.shape[0], 3), 50.0)], dim=1).cuda() for x in logits]
    views = [w[:, :T] for w in wide]
    assert not views[0].is_contiguous() or T == 1
    score_v, rank_v, live_v, _ = _run(views, empty)
    _check_scores(score_v, live_v, logits, empty, f"T={T} column slice")
    dense = _run(logits, empty)
    assert torch.equal(score_v, dense[0]) and torch.equal(rank_v, dense[1])
    # the layout the models' own logits have: column 0 of a padded [B*T, 4] matrix (strides (4T, 4))
    B = logits[0].shape[0]
    padded = [torch.full((B * T, 4), -77.0).cuda() for _ in logits]
    for p, x in zip(padded, logits):
        p[:, 0] = x.reshape(-1).cuda()
    strided = [p[:, :1].reshape(B, T) for p in padded]
    assert strided[0].stride() == (4 * T, 4) or T == 1
    score_s, rank_s, _, _ = _run(strided, empty)
    assert torch.equal(score_s, dense[0]) and torch.equal(rank_s, dense[1])


def test_a_row_without_live_candidates_is_all_zeros(lib):
    logits, _ = _inputs(6, 2)
    empty = torch.tensor([0, 6, 9, 1] + [0] * 7, dtype=torch.int32)              # rows 1 and 2: nothing live (9 > T is clamped)
    label = torch.zeros(11, 6)
    label[:, 0] = 1
    score, rank, live, metrics = _run(logits, empty, label)
    assert live.tolist()[:4] == [6, 0, 0, 5]
    assert bool((score[1:3] == 0).all()) and bool((rank[1:3] == 0).all()) and bool((metrics[1:3] == -1).all())


@pytest.mark.parametrize("T", [30, 100])
def test_ties_break_by_index(lib, T):
    logits, empty = _inputs(T, 3, seed=2)
    empty[:] = 0
    empty[1] = 4
    for x in logits:
        x[:, 7] = x[:, 2]                                                        # two identical columns in every model
        x[4] = 1.5                                                               # one all-equal row
    score, rank, live, _ = _run(logits, empty)
    s, r = score.cpu(), rank.cpu()
    assert torch.equal(s[:, 2].view(torch.int32), s[:, 7].view(torch.int32))     # bitwise equal scores ...
    rest = [b for b in range(r.shape[0]) if b != 4]
    assert bool((r[rest, 7] == r[rest, 2] + 1).all())                            # ... the lower index gets the better rank
    assert r[4].tolist() == list(range(1, T + 1))
    _check_ranks(score, rank, live, f"T={T} ties")


def _ref_metrics(rank, label, live):
    """float64 NumPy: (rr, ndcg5, ndcg10) per row from the ranks and labels; -1 without a live positive."""
    out = np.full((rank.shape[0], 3), -1.0)
    for b in range(rank.shape[0]):
        n = int(live[b])
        r = rank[b, :n].astype(np.float64)
        y = (label[b, :n] > 0.5).astype(np.float64)
        n_pos = int(y.sum())
        if n_pos == 0:
            continue
        out[b, 0] = (y / r).sum() / n_pos
        for c, k in ((1, 5), (2, 10)):
            dcg = (y / np.log2(1.0 + r))[r <= k].sum()
            ideal = sum(1.0 / np.log2(1.0 + i) for i in range(1, min(k, n_pos) + 1))
            out[b, c] = dcg / ideal
    return out


@pytest.mark.parametrize("T", [12, 30, 100, 257])
def test_metrics_match_float64(lib, T):
    B = 24
    logits, empty = _inputs(T, 2, B=B, seed=3)
    g = torch.Generator().manual_seed(T)
    label = torch.zeros(B, T)
    n = T - empty.long()
    for b in range(B):
        if b % 3 == 0:                                                           # one positive among the live candidates
            label[b, int(torch.randint(0, int(n[b]), (1,), generator=g))] = 1
        elif b % 3 == 1:                                                         # several positives
            k = max(1, int(n[b]) // 2)
            label[b, torch.randperm(int(n[b]), generator=g)[:k]] = 1
    empty[5], empty[8] = 3, 2                                                    # positives only in the padding -> -1
    label[5], label[8] = 0, 0
    label[5, T - 2], label[8, T - 1] = 1, 1
    score, rank, live, metrics = _run(logits, empty, label)
    assert tuple(metrics.shape) == (B, 3) and metrics.dtype == torch.float32
    want = _ref_metrics(rank.cpu().numpy(), label.numpy(), live.cpu().numpy())
    got = metrics.cpu().numpy().astype(np.float64)
    print(f"T={T}: worst metric error {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() < 1e-6
    assert (want[[5, 8]] == -1).all() and (want[2] == -1).all() and (got[[5, 8]] == -1).all()
    live_rows = want[:, 0] >= 0
    assert live_rows.sum() >= B // 2 and (got[live_rows] >= 0).all() and (got[live_rows] <= 1 + 1e-6).all()
    _check_ranks(score, rank, live, f"T={T} metrics")


def test_metrics_hand_checked(lib):
    """A single positive at rank 3: rr = 1/3, ndcg5 = ndcg10 = 1/log2(4) = 0.5.  At rank 7: ndcg5 = 0, ndcg10 = 1/log2(8) = 1/3."""
    T = 12
    x = torch.arange(T, 0, -1, dtype=torch.float32)[None, :].repeat(2, 1)        # descending: column j has rank j + 1
    label = torch.zeros(2, T)
    label[0, 2], label[1, 6] = 1, 1
    _score, rank, _live, metrics = _run([x], None, label)
    assert rank[0].tolist() == list(range(1, T + 1))
    m = metrics.cpu().numpy().astype(np.float64)
    assert np.abs(m[0] - [1 / 3, 0.5, 0.5]).max() < 1e-6
    assert np.abs(m[1] - [1 / 7, 0.0, 1 / 3]).max() < 1e-6


def _tiny_pad_models():
    """The fixture as test_predict_follows_test_py_semantics prepares it: two models, empty_num = [2, 3, 2, 3], the click on
    candidate 0 of every row."""
    from news_recommendation_model_amd import synth, trainer
    case, dims, batch, sd, fx = load_case("tiny_pad")
    sd2 = synth.make_state_dict(dims, seed=5, user_num=int(batch["user_num"]))
    batch["empty_num"][:] = [2, 3, 2, 3]
    batch["label"][:] = 0
    batch["label"][:, 0] = 1
    for b, z in enumerate(batch["empty_num"]):
        batch["x_target"][b, case["T"] - z:] = 0
        batch["x_global"][b, case["T"] - z:] = 0
    models = [trainer.build_model(dims, int(batch["user_num"]), s, device="cuda") for s in (sd, sd2)]
    return case, dims, batch, models


def test_predict_ranked_against_predict_on_tiny_pad(lib):
    from news_recommendation_model_amd import evaluation, trainer
    case, dims, batch, models = _tiny_pad_models()
    tb = trainer.batch_to_device(batch, "cuda")
    scores, live = evaluation.predict(models, tb)
    s_r, rank, live_r, metrics = evaluation.predict_ranked(models, tb, with_metrics=True)
    assert s_r.shape == scores.shape == (4, case["T"] - 2)
    assert live_r.dtype == torch.int32 and torch.equal(live_r.long(), live.long())
    assert torch.allclose(s_r, scores, rtol=RTOL, atol=ATOL), float((s_r - scores).abs().max())
    _check_ranks(s_r, rank, live_r, "tiny_pad")
    three = evaluation.predict_ranked(models, tb)
    assert len(three) == 3 and torch.equal(three[0], s_r) and torch.equal(three[1], rank)
    # a host empty_num (what a DataLoader hands over) takes the copy-free path to the same result
    host = dict(tb, empty_num=torch.from_numpy(batch["empty_num"]))
    s_h, rank_h, live_h = evaluation.predict_ranked(models, host)
    assert torch.equal(s_h, s_r) and torch.equal(rank_h, rank) and torch.equal(live_h, live_r)
    auc_v, top1_v = evaluation.validate(models, [tb])
    got = evaluation.validate_ranked(models, [tb])
    assert sorted(got) == ["auc", "mrr", "ndcg10", "ndcg5", "top1"]
    assert abs(got["auc"] - auc_v) < 1e-6 and abs(got["top1"] - top1_v) < 1e-6
    want = _ref_metrics(rank.cpu().numpy(), tb["label"][:, :s_r.shape[1]].cpu().numpy(), live_r.cpu().numpy()).mean(0)
    assert abs(got["mrr"] - want[0]) < 1e-6 and abs(got["ndcg5"] - want[1]) < 1e-6 and abs(got["ndcg10"] - want[2]) < 1e-6
    assert np.abs(metrics.cpu().numpy().mean(0) - want).max() < 1e-6
    # a single-class row raises what validate raises
    one_class = dict(tb, label=torch.zeros_like(tb["label"]))
    with pytest.raises(ValueError, match="Only one class present"):
        evaluation.validate_ranked(models, [one_class])


def test_predict_ranked_captured_in_a_graph(lib):
    """Captured after a side-stream warm-up (as GraphedPredict warms up), replayed twice with new inputs copied into the static
    buffers: bitwise the eager call's outputs."""
    from news_recommendation_model_amd import evaluation
    case, dims, batch, models = _tiny_pad_models()
    names = ("x_history", "x_target", "x_global", "empty_num")
    host = {k: torch.from_numpy(np.ascontiguousarray(batch[k])) for k in names}
    trim = int(host["empty_num"].min())
    static = {k: host[k].cuda() for k in names}
    feed = dict(static, empty_num=evaluation._HostMin(static["empty_num"], torch.full_like(host["empty_num"], trim)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            evaluation.predict_ranked(models, feed)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_scores, g_rank, g_live = evaluation.predict_ranked(models, feed)
    flipped = {k: host[k].flip(0).contiguous() for k in names}                   # the same rows in another order: same trim
    rolled = {k: host[k].roll(1, 0).contiguous() for k in names}
    for new in (flipped, rolled):
        for k in names:
            static[k].copy_(new[k])
        graph.replay()
        torch.cuda.synchronize()
        got = (g_scores.clone(), g_rank.clone(), g_live.clone())
        eager = evaluation.predict_ranked(models, {k: (new[k].cuda() if k != "empty_num" else new[k]) for k in names})
        for a, b in zip(got, eager):
            assert torch.equal(a, b)
    assert not torch.equal(got[0], evaluation.predict_ranked(models, {k: (flipped[k].cuda() if k != "empty_num" else flipped[k]) for k in names})[0])


@pytest.mark.parametrize("T", [30, 100])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_a_non_finite_logit_stays_in_its_row(lib, T, poison):
    B = 9
    logits, empty = _inputs(T, 2, B=B, seed=4)
    label = torch.zeros(B, T)
    label[:, 0] = 1
    clean = [t.clone() for t in _run(logits, empty, label)]
    bad = [x.clone() for x in logits]
    bad[1][3, 5] = poison
    dirty = _run(bad, empty, label)                                              # (returns: _run synchronises)
    others = [b for b in range(B) if b != 3]
    for name, a, c in zip(("score", "rank", "live", "metrics"), dirty, clean):
        assert torch.equal(a[others].view(torch.int32), c[others].view(torch.int32)), name


def test_score_dataset_end_to_end(lib, tmp_path):
    """Order, ids, batching and file format of the driver.  Ranks are compared with rank_row on predict_ranked's OWN scores, not
    with ranks of predict()'s scores: after the second softmax a padded row is nearly flat, and two correct fp32 evaluations
    may order candidates that differ by 1e-6 relative differently."""
    from news_recommendation_model_amd import data_io, evaluation, synth, trainer
    case, dims, _batch, models = _tiny_pad_models()
    B, T = 13, 6
    b = synth.make_batch(dims, B, 5, T, seed=11, user_num=50)
    b["empty_num"] = np.array([1, 3, 2, 1, 4, 0, 2, 1, 3, 0, 2, 2, 5], dtype=np.int64)
    for i, z in enumerate(b["empty_num"]):
        if z:
            b["x_target"][i, T - z:] = 0
            b["x_global"][i, T - z:] = 0
    b["impression_id"] = np.array([900 + 7 * i for i in range(B)])
    records = data_io.records_from_batch(b)
    head = data_io.write_processed_dataset(records, str(tmp_path / "test_set"), subvolume_item_num=6)
    assert sorted(os.listdir(tmp_path)) == ["test_set", "test_set.subvolume0", "test_set.subvolume1", "test_set.subvolume2"]
    out_dir = str(tmp_path / "out")
    zpath = evaluation.score_dataset(models, head, out_dir, batch_size=5)
    lines = open(os.path.join(out_dir, "predictions.txt"), encoding="utf-8").read().splitlines(keepends=True)
    assert len(lines) == B
    loaded, _ = data_io.load_processed_dataset(head)
    want_lines = []
    for lo in range(0, B, 5):                                                    # batches of 5, 5, 3: the second straddles subvolumes
        cb = data_io.collate(loaded[lo:lo + 5])
        tb = {k: torch.from_numpy(cb[k]).cuda() for k in ("x_history", "x_target", "x_global")}
        tb["empty_num"] = torch.from_numpy(cb["empty_num"])
        s_r, rank, live = evaluation.predict_ranked(models, tb)
        s_p, live_p = evaluation.predict(models, tb)
        assert torch.equal(live.long(), live_p.long())
        for i in range(s_r.shape[0]):
            n = int(live[i])
            assert n == T - int(cb["empty_num"][i])
            assert torch.allclose(s_r[i, :n], s_p[i, :n], rtol=RTOL, atol=ATOL)
            ranks = evaluation.rank_row(s_r[i, :n].tolist())
            assert rank[i, :n].tolist() == ranks
            want_lines.append("{} [{}]\n".format(int(cb["impression_id"][i]), ",".join(str(r) for r in ranks)))
    assert lines == want_lines
    for i, line in enumerate(lines):                                             # line i = record i: its id, live[i] ranks
        head_id, body = line.split(" ")
        assert int(head_id) == 900 + 7 * i
        assert len(body.strip()[1:-1].split(",")) == T - int(b["empty_num"][i])
    assert os.path.basename(zpath) == "predictions.zip"
    with zipfile.ZipFile(zpath) as z:
        assert z.namelist() == ["predictions.txt"]
        assert z.read("predictions.txt").decode("utf-8") == "".join(lines)


def test_opcheck_ensemble_rank(lib):
    from news_recommendation_model_amd import ops   # noqa: F401  (registers the ops)
    logits, empty = _inputs(30, 2)
    xs = [x.cuda() for x in logits]
    label = torch.zeros(11, 30, device="cuda")
    label[:, 1] = 1
    torch.library.opcheck(torch.ops.nrm.ensemble_rank.default, (xs, empty.cuda(), None))
    torch.library.opcheck(torch.ops.nrm.ensemble_rank.default, (xs, empty.cuda(), label))
    torch.library.opcheck(torch.ops.nrm.ensemble_rank.default, (xs[:1], None, label))
