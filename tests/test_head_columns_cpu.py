"""CPU: the float64 statements of head_columns_util against float64 nn.BatchNorm1d (forward, the three gradients, both running
statistics) and torch.cat; the float32 emulation of every column kernel in the kernel's own order inside every bound on every case
the GPU test runs; and every mutant rejected at >= 4 x the bound by every entry it touches on every case it applies to -- by the
same ``check_case`` the GPU test applies to the C entries."""
import numpy as np
import pytest
import torch

import head_columns_util as hu


def _module(c, training, dtype=torch.float64):
    bn = torch.nn.BatchNorm1d(c["N"], eps=hu.EPS, momentum=0.1).to(dtype)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c["gamma"])); bn.bias.copy_(torch.from_numpy(c["beta"]))
        bn.running_mean.copy_(torch.from_numpy(c["run_mean"])); bn.running_var.copy_(torch.from_numpy(c["run_var"]))
    return bn.train(training)


def _torch_truth(c, training):
    bn = _module(c, training)
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    y = bn(x)
    y.backward(torch.from_numpy(c["dy"]).double())
    return dict(y=y.detach().numpy(), dx=x.grad.numpy(), dgamma=bn.weight.grad.numpy(), dbeta=bn.bias.grad.numpy(),
                running_mean=bn.running_mean.numpy(), running_var=bn.running_var.numpy())


def _close(a, b, tol=1e-12, scale=None):
    if scale is None:
        scale = np.abs(b).max(0) if np.ndim(b) == 2 else np.abs(b)
    return np.all(np.abs(a - b) <= tol * (scale + 1e-30) + 1e-300)


@pytest.mark.parametrize("R,N,family", [(7, 4, "a"), (257, 132, "b"), (513, 8, "b"), (2, 8, "a")])
def test_statements_match_float64_batch_norm(R, N, family):
    """The statements chained in float64 (every `given` value the float64 one) are nn.BatchNorm1d, per column to 1e-12."""
    c = hu.make_case(R, N, N, family)
    x, dy = hu.f64(c["x"]), hu.f64(c["dy"])
    m, e = float(np.float32(0.1)), float(np.float32(hu.EPS))
    # the module with the float32 momentum and eps the C entry receives
    bn = torch.nn.BatchNorm1d(N, eps=e, momentum=m).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c["gamma"])); bn.bias.copy_(torch.from_numpy(c["beta"]))
        bn.running_mean.copy_(torch.from_numpy(c["run_mean"])); bn.running_var.copy_(torch.from_numpy(c["run_var"]))
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = bn(xt)
    yt.backward(torch.from_numpy(dy))
    s0 = hu.ref_colreduce(0, x, None, None, None, R)[0][0]
    mean, _, run_mean, _ = hu.ref_finalize(0, s0, hu.f64(c["run_mean"]), R, 0.1, hu.EPS)
    s1 = hu.ref_colreduce(1, x, None, mean, None, R)[0][0]
    rstd, _, run_var, _ = hu.ref_finalize(1, s1, hu.f64(c["run_var"]), R, 0.1, hu.EPS)
    y = hu.ref_apply(x, mean, rstd, c["gamma"], c["beta"])[0]
    (db, _), (dg, _) = hu.ref_colreduce(2, x, dy, mean, rstd, R)
    dx = hu.ref_backward(x, dy, mean, rstd, c["gamma"], db, dg, None, R, 1)[0]
    # dx cancels (at R = 2 to nothing): judged on the scale of its terms, gamma rstd dy
    assert _close(y, yt.detach().numpy()) and _close(dx, xt.grad.numpy(), scale=np.abs(hu.f64(c["gamma"]) * rstd * dy).max(0))
    assert _close(dg, bn.weight.grad.numpy()) and _close(db, bn.bias.grad.numpy())
    assert _close(run_mean, bn.running_mean.numpy()) and _close(run_var, bn.running_var.numpy())
    # eval: the running statistics normalise; dx = gamma rstd dy, with `add` on top
    bn.eval()
    bn.zero_grad()
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = bn(xt)
    yt.backward(torch.from_numpy(dy))
    rm, rs = bn.running_mean.numpy(), 1.0 / np.sqrt(bn.running_var.numpy() + e)
    assert _close(hu.ref_apply(x, rm, rs, c["gamma"], c["beta"])[0], yt.detach().numpy())
    dx = hu.ref_backward(x, dy, rm, rs, c["gamma"], db, dg, c["add"], R, 0)[0]
    assert _close(dx, xt.grad.numpy() + hu.f64(c["add"]))
    (db, _), (dg, _) = hu.ref_colreduce(2, x, dy, rm, rs, R)
    assert _close(dg, bn.weight.grad.numpy()) and _close(db, bn.bias.grad.numpy())


def test_mul_and_concat_statements_match_torch():
    c = hu.make_case(9, 8, 8, "a")
    rg, re = hu.ref_mul_bwd(c["dy"], c["g"], c["e"])
    g, e = torch.from_numpy(c["g"]).double().requires_grad_(True), torch.from_numpy(c["e"]).double().requires_grad_(True)
    (g * e).backward(torch.from_numpy(c["dy"]).double())
    assert np.array_equal(rg, g.grad.float().numpy()) and np.array_equal(re, e.grad.float().numpy())
    for name, spec in hu.CONCAT_SPECS.items():                           # the emulation is the statement: against torch.cat
        for R in hu.CONCAT_ROWS:
            for extra in (0, 4):
                assert hu.check_concat(_TorchCat(), spec, R, extra)["concat"] == 0.0, (name, R, extra)


class _TorchCat:
    def concat(self, parts, out, ldo, R):
        out = out.copy()
        views = [torch.from_numpy(p["buf"][p["off"]:p["off"] + R * p["ld"]]).reshape(R, p["ld"])[:, :p["width"]] for p in parts]
        cat = torch.cat(views, dim=1).numpy()
        out[:R, :cat.shape[1]] = cat
        return out


@pytest.mark.parametrize("family", hu.FAMILIES)
@pytest.mark.parametrize("N", hu.COLS)
def test_emulation_stays_inside_every_bound(N, family):
    worst = {}
    for R in hu.ROWS:
        for extra in hu.LD_EXTRA:
            c = hu.make_case(R, N, N + extra, family)
            for order in ((1, -1) if R > hu.RPB else (1,)):
                res = hu.check_case(hu.Emulated(order=order), c)
                assert set(res) == set(hu.SUMS + hu.SUMS_PRIOR + hu.ELEMENTWISE + ("finalize0.mean", "finalize0.running", "finalize1.rstd", "finalize1.running"))
                for k, v in res.items():
                    assert v <= 1.0, (R, N, extra, family, order, k, v)
                    worst[k] = max(worst.get(k, 0.0), v)
    print({k: round(v, 3) for k, v in worst.items()})


def test_emulation_of_the_second_trip_case():
    R, N = hu.SECOND_TRIP
    assert R * (N // 4) > hu.EW_MAX_THREADS
    c = hu.make_case(R, N, N + 4, "b")
    res = hu.check_case(hu.Emulated(), c, elementwise_only=True)
    assert set(res) == set(hu.ELEMENTWISE) and all(v <= 1.0 for v in res.values()), res
    bad = hu.check_case(hu.Emulated("no_second_trip"), c, elementwise_only=True)
    assert all(bad[k] >= 4.0 for k in hu.ELEMENTWISE), bad


def test_emulation_of_finalize_and_concat():
    for R, N, running, m in hu.finalize_cases():
        res = hu.check_finalize(hu.Emulated(), R, N, running, m)
        assert len(res) == (4 if running else 2) and all(v <= 1.0 for v in res.values()), (R, N, running, m, res)
        if running and R > 1:
            assert hu.check_finalize(hu.Emulated("biased_running_var"), R, N, running, m)["finalize1.running"] >= 4.0, (R, N, m)
    for name, spec in hu.CONCAT_SPECS.items():
        for R in hu.CONCAT_ROWS:
            for extra in (0, 4):
                assert hu.check_concat(hu.Emulated(), spec, R, extra)["concat"] == 0.0, (name, R, extra)
                assert hu.check_concat(hu.Emulated("column_border"), spec, R, extra)["concat"] == hu.INF, (name, R, extra)
                if R > 1 and any(ld > w for w, ld, _ in spec):
                    assert hu.check_concat(hu.Emulated("ld_taken_as_N"), spec, R, extra)["concat"] == hu.INF, (name, R, extra)


@pytest.mark.parametrize("mutant", [m for m in hu.MUTANTS if m != "no_second_trip"])
def test_every_mutant_is_rejected_on_every_case_it_applies_to(mutant):
    """>= 4 x the bound in some element of EVERY entry the mutant touches, on every case it applies to"""
    seen = 0
    for R, N, ld, family in hu.column_cases():
        if not hu.applies(mutant, R, N, ld):
            continue
        res = hu.check_case(hu.Emulated(mutant), hu.make_case(R, N, ld, family))
        for entry in hu.MUTANTS[mutant]:
            assert res[entry] >= 4.0, (mutant, R, N, ld, family, entry, res[entry])
        seen += 1
    assert seen >= 30, seen


@pytest.mark.parametrize("training", [True, False])
def test_chained_bounds_hold_for_the_emulation_and_are_small(training):
    """chain_bounds against float64 nn.BatchNorm1d at the shape the GPU test gives ops.batch_norm: the emulated chain is inside it per
    column, and it stays a bound worth having (<= 2e-5 of the column's scale for y and dx; <= 1e-4 of sum|term| for the two sums)."""
    R, N = 257, 132
    c = hu.make_case(R, N, N + 8, "b")
    truth = _torch_truth(c, training)
    cb = hu.chain_bounds(c["x"], c["dy"], None, c["gamma"], c["beta"], c["run_mean"], c["run_var"], 0.1, hu.EPS, training)
    for name, (ref, _b) in cb.items():
        assert _close(ref, truth[name], 1e-10), name
    be = hu.Emulated()
    ld = N + 8
    x, dy = hu.matrix(c["x"], ld), hu.matrix(c["dy"], ld)
    gamma, beta = hu.vector(c["gamma"]), hu.vector(c["beta"])
    got = {}
    if training:
        s0, _ = be.colreduce(0, x, None, None, None, hu.out_vector(N, 0.0), None, R, N, ld)
        mean, got["running_mean"] = be.finalize(0, s0, hu.out_vector(N), hu.out_vector(N, c["run_mean"]), R, N, 0.1, hu.EPS)
        s1, _ = be.colreduce(1, x, None, mean, None, hu.out_vector(N, 0.0), None, R, N, ld)
        rstd, got["running_var"] = be.finalize(1, s1, hu.out_vector(N), hu.out_vector(N, c["run_var"]), R, N, 0.1, hu.EPS)
    else:
        mean = hu.vector(c["run_mean"])
        rstd = hu.vector(hu.f32(np.float32(1) / np.sqrt(c["run_var"] + np.float32(hu.EPS))))
    got["y"] = be.apply(x, mean, rstd, gamma, beta, hu.out_matrix(R, ld), R, N, ld)[:R]
    got["dbeta"], got["dgamma"] = be.colreduce(2, x, dy, mean, rstd, hu.out_vector(N, 0.0), hu.out_vector(N, 0.0), R, N, ld)
    got["dx"] = be.backward(x, dy, mean, rstd, gamma, got["dbeta"], got["dgamma"], None, hu.out_matrix(R, ld), R, N, ld, int(training))[:R]
    for name, (ref, b) in cb.items():
        g = got[name][..., :N]
        r = hu.ratio(g, ref, b)
        print(name, "emulation error / chained bound", round(r, 3))
        assert r <= 1.0, (name, r)
        if name in ("y", "dx"):
            assert np.all(b <= 2e-5 * np.abs(ref).max(0)), name
    for name, term in (("dbeta", hu.f64(c["dy"])), ("dgamma", hu.f64(c["dy"]) * (truth["y"] - hu.f64(c["beta"])) / hu.f64(c["gamma"]))):
        assert np.all(cb[name][1] <= 1e-4 * np.abs(term).sum(0)), name
