"""CPU: the float64 Adam step of adam_util against torch.optim.Adam in float64 and against the oracle's adam_update, the mutant they
must tell apart, sanity of the bounds, and the argument checks of nrm_adam_step / nrm_adam_step_dev (no device needed: they
return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import adam_util as au
from oracle import user_model_oracle as orc

N = 64


def _trajectory(wd, steps=5, mutant=None):
    """``steps`` reference steps fed with their own float64 results -> [(p, m, v)], and the gradients used"""
    h = au.hyper(wd)
    p, m, v = (a[:N].astype(np.float64) for a in au.make_state(N, 1))
    out, grads = [], []
    for step in range(1, steps + 1):
        g = au.make_grad(N, 10 + step, wide=step == 3)[:N].astype(np.float64)
        r = au.reference_step(p, g, m, v, step, h, mutant=mutant)
        p, m, v = r["p"], r["m"], r["v"]
        out.append((p, m, v))
        grads.append(g)
    return out, grads


def _torch_trajectory(wd, grads):
    h = au.hyper(wd)
    p = torch.from_numpy(au.make_state(N, 1)[0][:N].astype(np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    out = []
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_reference_matches_torch_adam_for_five_steps(wd):
    ours, grads = _trajectory(wd)
    for step, (a, b) in enumerate(zip(ours, _torch_trajectory(wd, grads)), 1):
        assert np.max(np.abs(a[0] - b[0])) <= 1e-13, step            # parameters of size 1; a step moves them by 1e-3
        assert _rel(a[1], b[1]) <= 1e-12 and _rel(a[2], b[2]) <= 1e-12, step


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_reference_matches_the_oracle_update(wd):
    h = au.hyper(wd)
    p0, m0, v0 = (a[:N].astype(np.float64) for a in au.make_state(N, 2, first=False))
    g = au.make_grad(N, 3)[:N].astype(np.float64)
    r = au.reference_step(p0, g, m0, v0, 4, h)
    p, m, v = (torch.from_numpy(a.copy()) for a in (p0, m0, v0))
    orc.adam_update(p, torch.from_numpy(g), m, v, 4, lr=h["lr"], b1=h["b1"], b2=h["b2"], eps=h["eps"], weight_decay=h["wd"])
    assert np.max(np.abs(r["p"] - p.numpy())) <= 1e-15
    assert _rel(r["m"], m.numpy()) <= 1e-14 and _rel(r["v"], v.numpy()) <= 1e-14


@pytest.mark.parametrize("mutant", au.MUTANTS)
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_torch_adam_tells_the_mutant_apart(wd, mutant):
    good, grads = _trajectory(wd)
    bad, _ = _trajectory(wd, mutant=mutant)
    want = _torch_trajectory(wd, grads)
    assert np.max(np.abs(bad[0][0] - want[0][0])) > 1e-4            # step 1: sqrt(bc2) = 0.03 against bc2 = 0.001
    assert np.max(np.abs(good[0][0] - want[0][0])) <= 1e-13


def test_bounds_are_small_and_positive():
    """What the GPU test allows: a few U relative for the moments where nothing cancels, and for the update a few U of the move plus
    U of the parameter -- far below the move itself."""
    for step, wd in ((1, 0.0), (2, 1e-5), (5, 0.1), (1000, 1e-5), (100000, 0.0)):
        h = au.hyper(wd)
        p, m, v = au.make_state(1024, step, first=step == 1)
        g = au.make_grad(1024, step + 1)
        r = au.reference_step(p, g, m, v, step, h)
        bm, bv, bdp = au.bounds(r, p, step, h)
        assert np.all(bm >= 0) and np.all(bv > 0) and np.all(bdp >= 0)
        assert np.all(bv <= 5 * au.U * r["v"] + 2.0 ** -148)
        calm = (1 - h["b1"]) * np.abs(r["gg"]) <= np.abs(r["m"])
        assert calm.mean() > 0.5 and np.all(bm[calm] <= 4 * au.U * np.abs(r["m"][calm]))
        moving = np.abs(r["dp"]) > 1e-5
        assert moving.mean() > 0.5
        # the bias corrections dominate early (b2^s / (1 - b2^s) = 999 at step 1): 2 ulp of powf there are 1.2e-4 of the move
        assert np.all(bdp[moving] <= 2.5e-4 * np.abs(r["dp"][moving]) + 2 * au.U * np.abs(p[moving]))
    b1, e1, b2s, e2 = au.state_bounds(1, au.hyper(0.0))
    assert abs(b1 - 0.1) < 1e-7 and abs(b2s - np.sqrt(0.001)) < 1e-6 and e1 < 40 * au.U and e2 < 2001 * au.U


def test_adam_entries_validate_on_the_host(lib):
    f = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x1004)                                   # 4-byte aligned only
    cf = ctypes.c_float
    hy = [cf(1e-3), cf(0.9), cf(0.999), cf(1e-8), cf(1e-5)]

    def host(p=f, g=f, m=f, v=f, n=8, step=1):
        return lib.nrm_adam_step(p, g, m, v, n, *hy, step, 1, None)

    def dev(p=f, g=f, m=f, v=f, n=8, state=f):
        return lib.nrm_adam_step_dev(p, g, m, v, n, *hy, state, 1, None)
    text = b"(n % 4 == 0, step >= 1, 16-byte aligned buffers)"
    for what, kw in {"n % 4": dict(n=6), "negative n": dict(n=-4), "step 0": dict(step=0), "negative step": dict(step=-1), "p unaligned": dict(p=odd),
                     "g unaligned": dict(g=odd), "m unaligned": dict(m=odd), "v unaligned": dict(v=odd)}.items():
        assert host(**kw) == -1, what                                # NRM_EINVAL
        assert lib.nrm_last_error().startswith(b"nrm_adam_step: n=") and lib.nrm_last_error().endswith(text), (what, lib.nrm_last_error())
    assert host(n=6) == -1 and lib.nrm_last_error() == b"nrm_adam_step: n=6 step=1 " + text
    assert host(step=0) == -1 and lib.nrm_last_error() == b"nrm_adam_step: n=8 step=0 " + text
    for what, kw in {"null p": dict(p=None), "null g": dict(g=None), "null m": dict(m=None), "null v": dict(v=None)}.items():
        assert host(**kw) == -1 and lib.nrm_last_error() == b"nrm_adam_step: null pointer", what
    assert host(n=0) == 0                                            # nothing to do: no launch
    text = b"(n % 4 == 0, 16-byte aligned buffers)"
    for what, kw in {"n % 4": dict(n=6), "negative n": dict(n=-4), "p unaligned": dict(p=odd), "g unaligned": dict(g=odd), "m unaligned": dict(m=odd),
                     "v unaligned": dict(v=odd)}.items():
        assert dev(**kw) == -1, what
        assert lib.nrm_last_error().startswith(b"nrm_adam_step_dev: n=") and lib.nrm_last_error().endswith(text), (what, lib.nrm_last_error())
    assert dev(n=6) == -1 and lib.nrm_last_error() == b"nrm_adam_step_dev: n=6 " + text
    for what, kw in {"null p": dict(p=None), "null state": dict(state=None)}.items():
        assert dev(**kw) == -1 and lib.nrm_last_error() == b"nrm_adam_step_dev: null pointer", what
    assert dev(n=0) == 0                                             # returns before the kernel that advances the state
