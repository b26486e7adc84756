"""GPU: the Adam kernels (pool_loss.hip: adam_kernel through nrm_adam_step, adam_prep_kernel + adam_dev_kernel through nrm_adam_step_dev)
against one float64 step of adam_util.reference_step, per step and element by element.  After every step the reference is reloaded
with the kernel's float32 p, m, v, so the errors of the steps do not compound and Adam's own amplification of a difference stays
out of the comparison.  The bounds on m, v and the update p' - p are derived in adam_util's docstring from the kernel's expression:
U |m64| + 2 U (1 - b1) |gg64| for m, U v64 + 4 U (1 - b2) gg64^2 + 2^-148 for v, and for the update six roundings, the two bias
corrections formed as 1 - powf(b, s) in fp32, the bounds on m and v carried through, and U |p| for the final subtraction.

Every buffer is four floats longer than the n the call is given; the tail must come back bit for bit.

Not here: replays of a captured nrm_adam_step_dev against eager calls.  With that test in this file (it passed) the suite's process
died in a later, older test's capture of a step with a side-stream branch; the cause was not found, so no test of this file creates
a stream or captures a graph.

Measured on MI355X (15 tests, 1.2 s): worst error / bound 0.99 (m), 0.99 (v), 0.98 (update) -- where one term dominates, the bound is a
single rounding of it, which some element of a thousand nearly reaches.  Before adam_kernel formed its bias corrections on the device,
the host-step entry's 1 - b1^3 differed from the device-side state in the last bit and the two entries' parameters with it.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adam_util as au  # noqa: E402
from news_recommendation_model_amd import native  # noqa: E402

WORST = {}
cf = ctypes.c_float


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _hy(h):
    return [cf(h[k]) for k in ("lr", "b1", "b2", "eps", "wd")]


def _host_step(lib, bufs, n, h, step, zero_grad):
    rc = lib.nrm_adam_step(*[native.ptr(b) for b in bufs], n, *_hy(h), step, zero_grad, native.stream_ptr())
    assert rc == 0, lib.nrm_last_error()


def _dev_step(lib, bufs, n, h, state, zero_grad):
    rc = lib.nrm_adam_step_dev(*[native.ptr(b) for b in bufs], n, *_hy(h), native.ptr(state), zero_grad, native.stream_ptr())
    assert rc == 0, lib.nrm_last_error()


def _check_step(tag, before, after, n, step, h, zero_grad):
    """before / after: numpy (p, g, m, v) of n + TAIL floats around one call."""
    p0, g0, m0, v0 = before
    p1, g1, m1, v1 = after
    for a, b, name in zip(before, after, "pgmv"):
        assert np.array_equal(_bits(a[n:]), _bits(b[n:])), (tag, name, "the floats behind n changed")
    if zero_grad:
        assert not _bits(g1[:n]).any(), (tag, "zero_grad = 1 leaves +0.0")
    else:
        assert np.array_equal(_bits(g1[:n]), _bits(g0[:n])), (tag, "zero_grad = 0 leaves g as it was")
    ref = au.reference_step(p0[:n], g0[:n], m0[:n], v0[:n], step, h)
    bm, bv, bdp = au.bounds(ref, p0[:n], step, h)
    assert np.isfinite(p1[:n]).all() and np.isfinite(m1[:n]).all() and np.isfinite(v1[:n]).all(), tag
    dp = p1[:n].astype(np.float64) - p0[:n].astype(np.float64)
    for name, err, b in (("m", np.abs(m1[:n] - ref["m"]), bm), ("v", np.abs(v1[:n] - ref["v"]), bv), ("update", np.abs(dp - ref["dp"]), bdp)):
        ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
        WORST[name] = max(WORST.get(name, 0.0), ratio)
        print(f"{tag} {name}: worst error / bound = {ratio:.3f}")
        assert np.all(err <= b), (tag, name, ratio)
    still = (g0[:n] == 0) & (m0[:n] == 0) & (v0[:n] == 0)
    assert still.any() or step > 1, tag
    if h["wd"] == 0:                                   # nothing moves such an element: 0 / (0 + eps)
        assert not _bits(m1[:n][still]).any() and not _bits(v1[:n][still]).any() and np.array_equal(_bits(p1[:n][still]), _bits(p0[:n][still])), tag
    else:                                              # only the decay term does: gg = wd p
        gg = h["wd"] * p0[:n][still].astype(np.float64)
        assert np.all(np.abs(m1[:n][still] - (1 - h["b1"]) * gg) <= 3 * au.U * np.abs((1 - h["b1"]) * gg)), tag


def _run_steps(lib, n, wd, entry, wide, steps=5, seed=0):
    h = au.hyper(wd)
    p, m, v = au.make_state(n, 100 + seed)
    bufs = _dev(p, au.make_grad(n, 0), m, v)
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    for step in range(1, steps + 1):
        g = au.make_grad(n, 200 + 10 * seed + step, wide=wide)
        bufs[1].copy_(torch.from_numpy(g))
        before = [b.cpu().numpy() for b in bufs]
        zero_grad = (step + seed) % 2
        if entry == "host":
            _host_step(lib, bufs, n, h, step, zero_grad)
        else:
            _dev_step(lib, bufs, n, h, state, zero_grad)
        torch.cuda.synchronize()
        _check_step((entry, n, wd, wide, step), before, [b.cpu().numpy() for b in bufs], n, step, h, zero_grad)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("wd", au.WEIGHT_DECAYS)
def test_five_steps_per_step_and_element(lib, entry, wd):
    """n = 4 .. 1028 (one float4, one block less one float4, a block, a block and one float4), gradients of size 1 and |g| across
    1e-20 .. 1e15 in one buffer, zero_grad alternating."""
    for i, n in enumerate(au.SIZES):
        _run_steps(lib, n, wd, entry, wide=False, seed=i)
        _run_steps(lib, n, wd, entry, wide=True, seed=i + 1)


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_second_trip_of_the_grid_stride_loop(lib, entry):
    """2048 blocks x 256 threads x 4 floats = 2 097 152: the float4 behind them is the first a thread takes on its second trip"""
    _run_steps(lib, au.SIZE_SECOND_TRIP, 1e-5, entry, wide=False, steps=2, seed=3)


@pytest.mark.parametrize("step", [1000, 100000])
def test_late_steps_of_the_host_entry(lib, step):
    for wd in au.WEIGHT_DECAYS:
        for wide in (False, True):
            n, h = 1028, au.hyper(wd)
            p, m, v = au.make_state(n, step + wide, wide=wide, first=False)
            bufs = _dev(p, au.make_grad(n, step + 7, wide=wide), m, v)
            before = [b.cpu().numpy() for b in bufs]
            _host_step(lib, bufs, n, h, step, 0)
            torch.cuda.synchronize()
            _check_step(("late", wd, wide, step), before, [b.cpu().numpy() for b in bufs], n, step, h, 0)


def _start(n, seed):
    p, m, v = au.make_state(n, seed, first=False)
    return [p, au.make_grad(n, seed + 1), m, v]


def test_device_step_state(lib):
    """state = {step, 1 - b1^step, sqrt(1 - b2^step)} after k = 1 .. 5 calls; a call with n = 0 returns before the kernel that
    advances it and leaves it as it is (asserted, so that a change of that is deliberate)."""
    h = au.hyper(1e-5)
    bufs = _dev(*_start(8, 1))
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    for k in range(1, 6):
        _dev_step(lib, bufs, 8, h, state, 0)
        torch.cuda.synchronize()
        s = state.cpu().numpy().astype(np.float64)
        bc1, e1, bc2s, e2 = au.state_bounds(k, h)
        print(f"step {k}: state {s[:3]}, float64 {bc1} {bc2s}, error / bound {abs(s[1] - bc1) / (e1 * bc1):.3f} {abs(s[2] - bc2s) / (e2 * bc2s):.3f}")
        assert s[0] == k and s[3] == 0
        assert abs(s[1] - bc1) <= e1 * bc1 and abs(s[2] - bc2s) <= e2 * bc2s, k
    before = [b.clone() for b in bufs] + [state.clone()]
    _dev_step(lib, bufs, 0, h, state, 1)
    torch.cuda.synchronize()
    for a, b in zip(before, bufs + [state]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("wd", au.WEIGHT_DECAYS)
def test_host_and_device_step_entries_agree_bitwise(lib, wd):
    """The two kernels are one expression; at equal step they must give the same bits."""
    h = au.hyper(wd)
    for n in (8, 1028):
        a, b = _dev(*_start(n, n)), _dev(*_start(n, n))
        state = torch.zeros(4, dtype=torch.float32, device="cuda")
        for step in range(1, 6):
            _host_step(lib, a, n, h, step, 0)
            _dev_step(lib, b, n, h, state, 0)
            torch.cuda.synchronize()
            s = state.cpu().numpy()
            host_bc1 = np.float32(1) - np.float32(h["b1"]) ** np.float32(step)
            host_bc2s = np.sqrt(np.float32(1) - np.float32(h["b2"]) ** np.float32(step))
            print(f"n {n} step {step}: device state {s[1]!r} {s[2]!r}, fp32 on the host {host_bc1!r} {host_bc2s!r}")
            for x, y, name in zip(a, b, "pgmv"):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (n, wd, step, name)


def test_zz_worst_ratios():
    print("worst error / bound:", {k: round(v, 3) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
