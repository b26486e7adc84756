"""GPU: the folded head tail (ops.head_tail: mlp.fc2 folded into out_mlp.fc1, csrc/head.hip head_fold_kernel /
head_fold_bwd_kernel) against a float64 evaluation of the UNFOLDED chain out_mlp(mlp(x)) on the CPU.

Yardstick: the error of the unfolded HIP path (NRM_HEAD_FOLD=0: two mlp_gelu nodes, the arithmetic before the fold) against the same
float64 values.  Over width -> hidden in {24 -> 6, 72 -> 18, 136 -> 34, 1608 -> 402} and 1, 63, 70 and 130 rows the folded path's
error (max |got - ref| / max |ref| per tensor) was measured against the unfolded one's for a2, the logits, da1, d(input) and the eight
parameter gradients (NRM_HEAD_FOLD_RECORD=<path> makes every case of the first test write its figures there, before it asserts).
profiles/head_fold.json is one MI355X run of that: worst ratio 3.87 (db1 at 24 -> 6, 130 rows), so the tests assert RATIO_BOUND = 32
= that ratio times 8, rounded up to a power of two -- the margin DESIGN section 3b took for run-to-run float atomics.  That run covers
eleven of the twelve quantities: the build it measured formed dW_o1 without its db' (x) b_m2 term (error 0.1-0.3 of the tensor's scale,
which this test caught), so for dwo the bound is PROVISIONAL until the file is recorded again; the file says the same.  An unfolded error
below half an ulp of the tensor's scale (2^-24) counts as 2^-24: no fp32 result is expected closer than that.

da1 is never materialised by either path (GELU'(z1) rides in the epilogue of the GEMM that forms it): it is read out of the real
backward kernels by running them once more with GELU' == 1 (z1 = 30: Phi = 1 and phi = 0 exactly in the kernel's evaluation) and an
identity first layer, so that d(input)[:, :hidden] IS da1, product by product.
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(24, 6), (72, 18), (136, 34), (1608, 402)]
ROWS = [1, 63, 70, 130]
PARAMS = ("w1", "b1", "wm", "bm", "wo", "bo", "w3", "b3")
FOLDED = ("wm", "bm", "wo", "bo")
QUANTITIES = ("a2", "logits", "da1", "dx") + tuple("d" + k for k in PARAMS)
RATIO_MEASURED = 3.87         # profiles/head_fold.json: error_ratios.worst_ratio (dwo not in that run: see the module docstring)
RATIO_BOUND = 32.0            # 8 x RATIO_MEASURED rounded up to a power of two
HALF_ULP = 2.0 ** -24
# two HIP evaluations of the same arithmetic that differ only in the order of a slab reduction's float atomics, or not at all
# (the fp32 bound tests/test_gpu_dense.py holds the dense kernels to against float64)
SAME_ARITHMETIC = 1e-5
# the folded against the unfolded evaluation of one model: two fp32 evaluations, each within SAME_ARITHMETIC of float64, times the 8 of
# the atomics margin; a stale image is off by percent
FOLD_VS_UNFOLD = 8.0 * SAME_ARITHMETIC


@functools.lru_cache(maxsize=None)
def _case(width, hid, M):
    g = torch.Generator(device="cpu").manual_seed(1000 * width + M)
    r = lambda *s: torch.randn(*s, generator=g)                        # noqa: E731
    p = {"w1": r(hid, width) / np.sqrt(width), "b1": 0.1 * r(hid), "wm": r(width, hid) / np.sqrt(hid), "bm": 0.1 * r(width),
         "wo": r(hid, width) / np.sqrt(width), "bo": 0.1 * r(hid), "w3": r(1, hid) / np.sqrt(hid), "b3": 0.1 * r(1)}
    return {"p": p, "x": r(M, width), "gy": r(M, 1), "width": width, "hid": hid, "M": M}


@functools.lru_cache(maxsize=None)
def _reference(width, hid, M):
    """float64, CPU, the unfolded chain; computed once per case and shared (read only)."""
    c = _case(width, hid, M)
    F = torch.nn.functional
    p = {k: v.double().requires_grad_(True) for k, v in c["p"].items()}
    x = c["x"].double().requires_grad_(True)
    a1 = F.gelu(F.linear(x, p["w1"], p["b1"]))
    a1.retain_grad()
    a2 = F.gelu(F.linear(F.linear(a1, p["wm"], p["bm"]), p["wo"], p["bo"]))
    y = F.linear(a2, p["w3"], p["b3"])
    y.backward(c["gy"].double())
    out = {"a2": a2.detach().numpy(), "logits": y.detach().numpy(), "da1": a1.grad.numpy(), "dx": x.grad.numpy()}
    out.update({"d" + k: p[k].grad.numpy() for k in PARAMS})
    return out


def _forward(fold, x, p):
    """-> (logits, h or None, a1, z1, a2, z2) through the ops themselves (their hidden outputs are what the checks need)."""
    if fold:
        y, a1, z1, a2, z2 = torch.ops.nrm.head_tail_fwd(x, p["w1"], p["b1"], p["wm"], p["bm"], p["wo"], p["bo"], p["w3"], p["b3"])
        return y, None, a1, z1, a2, z2
    h, a1, z1, _ = torch.ops.nrm.mlp_gelu_fwd(x, p["w1"], p["b1"], p["wm"], p["bm"], None)
    y, a2, z2, _ = torch.ops.nrm.mlp_gelu_fwd(h, p["wo"], p["bo"], p["w3"], p["b3"], None)
    return y, h, a1, z1, a2, z2


def _da1(fold, c, x, p, h, a1, z1, a2, z2, gy):
    hid, width = c["hid"], c["width"]
    eye = torch.zeros(hid, width, device="cuda")
    eye[:, :hid] = torch.eye(hid, device="cuda")
    one = torch.full((z1.shape[0], (hid + 3) // 4 * 4), 30.0, device="cuda")[:, :hid]      # GELU'(30) == 1 exactly; padded rows as the kernels want
    e = torch.empty(0, device="cuda")
    d = lambda t: t.detach()                                            # noqa: E731
    if fold:
        dx = torch.ops.nrm.head_tail_bwd(gy, d(x), eye, d(p["wm"]), d(p["bm"]), d(p["wo"]), d(p["bo"]), d(p["w3"]), d(a1), one, d(a2), d(z2),
                                         True, True, True, False, False, False, False)[0]
    else:
        dh = torch.ops.nrm.mlp_gelu_bwd(gy, d(h), d(p["wo"]), d(p["w3"]), d(a2), d(z2), e, None, True, True, True)[0]
        dx = torch.ops.nrm.mlp_gelu_bwd(dh, d(x), eye, d(p["wm"]), d(a1), one, e, None, True, True, True)[0]
    return dx[:, :hid]


def _run(c, fold, deferred=False, pre=None, frozen=(), want_da1=True, x_override=None):
    """One forward + backward of the tail on the GPU -> {quantity: numpy} (a frozen tensor's gradient: None)."""
    from news_recommendation_model_amd import ops
    p = {k: v.cuda().requires_grad_(k not in frozen) for k, v in c["p"].items()}
    x = (c["x"] if x_override is None else x_override).cuda().requires_grad_(True)
    gy = c["gy"].cuda()
    if pre is not None:
        for k in PARAMS:
            p[k].grad = pre[k].clone()
    y, h, a1, z1, a2, z2 = _forward(fold, x, p)
    if deferred:
        with ops.deferred_slab_reductions():
            y.backward(gy)
        ops.verify_deferred_targets(list(p.values()))
        ops.flush_slab_reductions()
    else:
        y.backward(gy)
    assert not ops._deferred["pending"]
    out = {"a2": a2, "logits": y, "dx": x.grad}
    if want_da1:
        out["da1"] = _da1(fold, c, x, p, h, a1, z1, a2, z2, gy)
    out.update({"d" + k: p[k].grad for k in PARAMS})
    torch.cuda.synchronize()
    return {k: (v.detach().cpu().numpy() if v is not None else None) for k, v in out.items()}


def error_ratios(width, hid, M):
    """{quantity: (folded error, unfolded error, ratio)} against float64 (what NRM_HEAD_FOLD_RECORD records)."""
    c, ref = _case(width, hid, M), _reference(width, hid, M)
    got_f, got_u = _run(c, True), _run(c, False)
    res = {}
    for q in QUANTITIES:
        ef, eu = rel_err(got_f[q], ref[q]), rel_err(got_u[q], ref[q])
        res[q] = (ef, eu, ef / max(eu, HALF_ULP))
    return res


def _record(width, hid, M, res):
    """NRM_HEAD_FOLD_RECORD=<path>: every case adds its figures (before it asserts) to that JSON file -- how the "error_ratios" part
    of profiles/head_fold.json is recorded on an MI355X."""
    import json
    import os
    path = os.environ.get("NRM_HEAD_FOLD_RECORD")
    if not path:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {"cases": {}}
    doc["cases"][f"{width}->{hid} rows {M}"] = {q: {"folded": ef, "unfolded": eu, "ratio": r} for q, (ef, eu, r) in res.items()}
    worst = max(((v["ratio"], f"{k} {q}") for k, c in doc["cases"].items() for q, v in c.items()))
    doc["worst_ratio"], doc["worst_at"] = worst
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("width,hid", SHAPES)
def test_folded_tail_holds_the_unfolded_paths_error_against_float64(lib, monkeypatch, width, hid, M):
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    res = error_ratios(width, hid, M)
    for q, (ef, eu, ratio) in res.items():
        print(f"head_fold {width}->{hid} M={M} {q}: folded {ef:.3e} unfolded {eu:.3e} ratio {ratio:.3f}")
    _record(width, hid, M, res)
    for q, (ef, eu, ratio) in res.items():
        assert ef <= RATIO_BOUND * max(eu, HALF_ULP), (q, ef, eu, ratio)


@pytest.mark.parametrize("width,hid,M", [(24, 6, 63), (136, 34, 130), (1608, 402, 70)])
def test_deferred_and_immediate_reductions_existing_grad_and_frozen_tensors(lib, monkeypatch, width, hid, M):
    """The split of dW' runs behind the flush inside ops.deferred_slab_reductions() and at once outside it: same gradients.  A
    gradient that exists already is accumulated into (immediate mode: train_step does not defer then).  Each of the four folded
    tensors frozen in turn gets no gradient and leaves the others what they were -- in both modes."""
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    c = _case(width, hid, M)
    base = _run(c, True, want_da1=False)
    close = lambda a, b: rel_err(a, b) <= SAME_ARITHMETIC                # noqa: E731
    deferred = _run(c, True, deferred=True, want_da1=False)
    for q in base:
        assert close(deferred[q], base[q]), q
    g = torch.Generator(device="cpu").manual_seed(5)
    pre = {k: torch.randn(c["p"][k].shape, generator=g).cuda() for k in PARAMS}
    acc = _run(c, True, pre=pre, want_da1=False)
    for k in PARAMS:
        assert close(acc["d" + k], base["d" + k] + pre[k].cpu().numpy()), k
    for frozen in FOLDED:
        for mode in (False, True):
            got = _run(c, True, deferred=mode, frozen=(frozen,), want_da1=False)
            assert got["d" + frozen] is None
            for q in base:
                if q != "d" + frozen:
                    assert close(got[q], base[q]), (frozen, mode, q)


@pytest.mark.parametrize("which", FOLDED)
def test_deferred_split_refuses_a_gradient_that_existed_before(lib, monkeypatch, which):
    """Inside ops.deferred_slab_reductions() the split writes into the buffers autograd adopted; a folded tensor that had a gradient
    already gets its new one accumulated elsewhere, which verify_deferred_targets must see for each of the four split targets."""
    from news_recommendation_model_amd import ops
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    c = _case(24, 6, 63)
    p = {k: v.cuda().requires_grad_(True) for k, v in c["p"].items()}
    p[which].grad = torch.ones_like(p[which])
    y = _forward(True, c["x"].cuda(), p)[0]
    with ops.deferred_slab_reductions():
        y.backward(c["gy"].cuda())
    with pytest.raises(RuntimeError, match="deferred slab reductions"):
        ops.verify_deferred_targets(list(p.values()))
    assert not ops._deferred["pending"]
    torch.cuda.synchronize()


def test_a_nan_row_stays_in_its_row(lib, monkeypatch):
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    c = _case(72, 18, 130)
    clean = _run(c, True)
    x = c["x"].clone()
    bad = 67                                                            # second 64-row block
    x[bad, 5] = float("nan")
    got = _run(c, True, x_override=x)
    keep = np.arange(c["M"]) != bad
    for q in ("logits", "da1", "dx", "a2"):
        assert np.isnan(got[q][bad]).any(), q
        assert np.array_equal(got[q][keep], clean[q][keep]), q


def _tiny(seed=2, emb=16, B=3, H=4, T=5, train=False):
    from news_recommendation_model_amd import config, synth, trainer
    dims = config.Dims.for_emb(emb, 40)
    sd = synth.make_state_dict(dims, seed=seed, user_num=7)
    batch = synth.make_batch(dims, B, H, T, seed=3, user_num=7)
    model = trainer.build_model(dims, 7, sd, device="cuda")
    model.train(train)
    return dims, model, trainer.batch_to_device(batch, "cuda")


def _logits(model, tb, monkeypatch, fold):
    if fold:
        monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    else:
        monkeypatch.setenv("NRM_HEAD_FOLD", "0")
    with torch.no_grad():
        out = model(tb["x_history"], tb["x_target"], tb["x_global"]).clone()
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    return out


def _folds_during(fn):
    from news_recommendation_model_amd import native
    native.kernel_events = []
    try:
        res = fn()
        n = sum(1 for tag, _, _ in native.kernel_events if tag == "nrm_head_fold")
    finally:
        native.kernel_events = None
    return res, n


def _assert_image_is_fresh(model, tb, monkeypatch):
    """The folded forward reads the image, the unfolded one the weights (through packed images the suite already trusts): a stale
    image shows as a difference far above fp32 rounding."""
    model_was_training = model.training
    model.eval()
    a, b = _logits(model, tb, monkeypatch, True), _logits(model, tb, monkeypatch, False)
    model.train(model_was_training)
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= FOLD_VS_UNFOLD


def test_image_follows_in_place_updates_load_state_dict_and_is_reused_in_eval(lib, monkeypatch):
    from news_recommendation_model_amd import evaluation, ops, synth
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    ops.invalidate_packed_weights()
    dims, model, tb = _tiny()
    assert model.head_fold_applies(dims.head_dim)
    _assert_image_is_fresh(model, tb, monkeypatch)
    before = _logits(model, tb, monkeypatch, True)
    with torch.no_grad():
        model.mlp.fc2.weight.mul_(1.5)
        model.out_mlp.fc1.bias.add_(0.3)
    _assert_image_is_fresh(model, tb, monkeypatch)
    assert rel_err(_logits(model, tb, monkeypatch, True).cpu().numpy(), before.cpu().numpy()) > 1e-3          # the update matters
    sd = synth.make_state_dict(dims, seed=9, user_num=7)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    _assert_image_is_fresh(model, tb, monkeypatch)
    # eval: the image is reused untouched between two predict calls
    feed = dict(tb, empty_num=torch.zeros(tb["x_target"].shape[0], dtype=torch.int64))
    evaluation.predict([model], feed)
    ent = next(iter(ops._folds.values()))
    ptrs = (ent.img_f.data_ptr(), ent.img_b.data_ptr(), ent.bias.data_ptr())
    (s1, _), n1 = _folds_during(lambda: evaluation.predict([model], feed))
    (s2, _), n2 = _folds_during(lambda: evaluation.predict([model], feed))
    assert n1 == 0 and n2 == 0 and torch.equal(s1, s2)
    assert next(iter(ops._folds.values())) is ent and ptrs == (ent.img_f.data_ptr(), ent.img_b.data_ptr(), ent.bias.data_ptr())
    model.out_mlp.fc1.weight.data.mul_(0.5)                             # invisible to the version counter ...
    ops.invalidate_packed_weights()                                     # ... so the caller says so: the image is dropped
    assert not ops._folds
    _, n3 = _folds_during(lambda: evaluation.predict([model], feed))
    assert n3 == 1
    _assert_image_is_fresh(model, tb, monkeypatch)


def test_flat_adam_step_refreshes_the_image_with_the_other_packed_weights(lib, monkeypatch):
    from news_recommendation_model_amd import ops, trainer
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    ops.invalidate_packed_weights()
    dims, model, tb = _tiny(train=True)
    opt = trainer.FlatAdam(model, lr=1e-2)
    trainer.train_step(model, opt, tb)                                   # creates the image (forward) and refreshes it (step)
    _, n = _folds_during(lambda: trainer.train_step(model, opt, tb))
    assert n == 1                                                        # behind FlatAdam.step(), none lazily in the forward
    assert not ops._deferred["pending"]
    _, n = _folds_during(lambda: _logits(model, tb, monkeypatch, True))
    assert n == 0
    _assert_image_is_fresh(model, tb, monkeypatch)
    # the folded and the unfolded step compute the same gradients: one step of each from the same state
    g = {}
    for fold in (True, False):
        monkeypatch.setenv("NRM_HEAD_FOLD", "1" if fold else "0")
        out = model(tb["x_history"], tb["x_target"], tb["x_global"])
        loss = model.loss(tb["user_id"], out, tb["label"])
        with ops.deferred_slab_reductions():
            loss.backward(ops.unit_grad(loss))
        opt.collect_grads()
        g[fold] = opt.flat_grad.clone()
        opt.zero_grad()
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    assert rel_err(g[True].cpu().numpy(), g[False].cpu().numpy()) <= FOLD_VS_UNFOLD


def test_captured_step_refolds_on_every_replay(lib, monkeypatch):
    """Two replays of a captured step land where two eager steps land (the existing captured-step test's bound), and after them
    the image inside the graph's memory is that of the updated weights."""
    from news_recommendation_model_amd import ops, trainer
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    ops.invalidate_packed_weights()
    _, eager, tb = _tiny(train=True)
    _, graphed, _ = _tiny(train=True)
    eopt, gopt = trainer.FlatAdam(eager), trainer.FlatAdam(graphed)
    for _ in range(3 + 2):
        le, _ = trainer.train_step(eager, eopt, tb)
    step = trainer.GraphedTrainStep(graphed, gopt, tb, warmup=3)
    for _ in range(2):
        lg, _ = step.replay()
    torch.cuda.synchronize()
    assert gopt.steps == eopt.steps == 5
    assert abs(float(lg) - float(le)) < 1e-4 * abs(float(le))
    for (k, a), (_, b) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.allclose(a, b, rtol=0, atol=5e-4), k
    _, n = _folds_during(lambda: _logits(graphed, tb, monkeypatch, True))
    assert n == 0                                                        # the replay left a current image: nothing to fold lazily
    _assert_image_is_fresh(graphed, tb, monkeypatch)


@pytest.mark.parametrize("how", ["hook", "relu"])
def test_a_hooked_or_non_gelu_tail_takes_the_two_call_path(lib, monkeypatch, how):
    from news_recommendation_model_amd import ops
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    ops.invalidate_packed_weights()
    dims, model, tb = _tiny()
    if how == "hook":
        seen = []
        model.out_mlp.register_forward_hook(lambda mod, args, out: seen.append(tuple(args[0].shape)))
    else:
        model.mlp.activation = torch.nn.ReLU()
    assert not model.head_fold_applies(dims.head_dim)
    a, n = _folds_during(lambda: _logits(model, tb, monkeypatch, True))
    b = _logits(model, tb, monkeypatch, False)
    assert n == 0 and not ops._folds and torch.equal(a, b)              # the same launches as with the switch off
    if how == "hook":
        assert seen and seen[0][1] == dims.head_dim                     # the hook saw mlp's full-width output


def test_opcheck_head_tail(lib):
    from news_recommendation_model_amd import ops   # noqa: F401
    c = _case(24, 6, 63)
    p = {k: v.cuda().requires_grad_(True) for k, v in c["p"].items()}
    x = c["x"].cuda().requires_grad_(True)
    torch.library.opcheck(torch.ops.nrm.head_tail_fwd.default, (x, p["w1"], p["b1"], p["wm"], p["bm"], p["wo"], p["bo"], p["w3"], p["b3"]))
