"""Shared by the tests of the Adam kernels (pool_loss.hip: adam_kernel behind nrm_adam_step, adam_prep_kernel + adam_dev_kernel behind
nrm_adam_step_dev): one step of float64 Adam written as oracle.user_model_oracle.adam_update writes it, the bounds one step of the
fp32 kernel is held to, the inputs, and the mutant the CPU test must tell from torch.optim.Adam.

The reference reads what the kernel reads: p, g, m, v are float32 values promoted to float64, and lr, beta1, beta2, eps and the
weight decay are the float32 values the C entry receives (``hyper``), promoted.  b^step is formed in float64.

The kernel (U = 2^-24; every fp32 operation is correctly rounded, a fused multiply-add rounds once):
    gg = fma(wd, p, g)                                   1 rounding
    m' = fma(b1, m, (1 - b1) * gg)                       1 - b1 is exact (Sterbenz); the product and the fma round
    v' = fma(b2, v, (1 - b2) * gg * gg)                  two products and the fma round
    denom = sqrt(v') / bc2s + eps                        3 roundings
    p' = p - (lr / bc1) * (m' / denom)                   3 roundings and the final subtraction

m':  |m' - m64| <= U |m64| + 2 U (1 - b1) |gg64|.  The two terms of m' may cancel, so the error is relative to the terms, not to their
     sum; where they do not cancel ((1 - b1) |gg64| <= |m64|) this is within the 4 U |m64| a purely relative statement would give.
v':  |v' - v64| <= U v64 + 4 U t64 + 2^-148 with t64 = (1 - b2) gg64^2: gg enters twice (2 U), two products (2 U), and the fma's own
     rounding; no cancellation, so this is at most 5 U v64 -- one U more than four roundings, because gg's rounding counts twice.
     2^-148: the second product and the fma may each round in the denormal range, half a denormal step (2^-150) each, doubled.
dp = p' - p:  |dp - dp64| <= (1 + 2^-10) [ |dp64| (6 U + E1 + E2 + Ev) + (lr / bc1) / denom64 * Bm ] + U max(|p|, |p64'|)
     6 U: the six roundings of denom and of the update before the subtraction; Bm: the bound on m' above, through dp = -(lr / bc1) m' / denom;
     Ev = dd / (denom64 - dd) with dd = [sqrt(v64 + Bv) - sqrt(max(v64 - Bv, 0))] / sqrt(bc2): the bound on v' through the square root;
     E1 = U (1 + 4 b1^s / (1 - b1^s)): bc1 = 1 - powf(b1, s) in fp32, powf within 2 ulp = 4 U b1^s, and the subtraction's rounding;
     E2 = E1(b2) / 2 + U: the same for 1 - powf(b2, s), halved by the square root, and the square root's rounding;
     U max(|p|, |p64'|): the final subtraction; 1 + 2^-10 covers the products of these first-order terms.
"""
import math

import numpy as np

U = 2.0 ** -24
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
WEIGHT_DECAYS = (0.0, 1e-5, 0.1)
SIZES = (4, 8, 1020, 1024, 1028)
SIZE_SECOND_TRIP = 2 * 1024 * 1024 + 4          # 2048 blocks x 256 threads x 4 floats, and one float4 more
TAIL = 4                                        # floats behind the n the call is given; they must not change
MUTANTS = ("bc2_no_sqrt",)                      # sqrt(v) / bc2 instead of sqrt(v) / sqrt(bc2)


def hyper(wd, **kw):
    """lr, b1, b2, eps, wd as the float32 values the C entry receives, as Python floats"""
    h = dict(HYPER, wd=wd, **kw)
    return {k: float(np.float32(v)) for k, v in h.items()}


def reference_step(p, g, m, v, step, h, mutant=None):
    """One step of oracle.user_model_oracle.adam_update in float64 -> dict of new m, v, p and what the bounds need."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = h["b1"], h["b2"]
    gg = g + h["wd"] * p
    m2 = b1 * m + (1 - b1) * gg
    t = (1 - b2) * gg * gg
    v2 = b2 * v + t
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = np.sqrt(v2) / (bc2 if mutant == "bc2_no_sqrt" else math.sqrt(bc2)) + h["eps"]
    dp = -(h["lr"] / bc1) * m2 / denom
    return dict(gg=gg, m=m2, v=v2, t=t, dp=dp, p=p + dp, denom=denom, bc1=bc1, bc2s=math.sqrt(bc2))


def bias_error(b, step):
    """relative error of 1 - powf(b, step) formed in fp32"""
    bs = b ** step
    return U * (1 + 4 * bs / (1 - bs))


def state_bounds(step, h):
    """(bc1, its relative bound, sqrt(bc2), its relative bound) of the device-side step state"""
    return 1 - h["b1"] ** step, bias_error(h["b1"], step), math.sqrt(1 - h["b2"] ** step), 0.5 * bias_error(h["b2"], step) + U


def bounds(ref, p_old, step, h):
    """-> (Bm, Bv, Bdp) of the module docstring, element-wise"""
    p_old = np.asarray(p_old, dtype=np.float64)
    bm = U * np.abs(ref["m"]) + 2 * U * (1 - h["b1"]) * np.abs(ref["gg"])
    bv = U * ref["v"] + 4 * U * ref["t"] + 2.0 ** -148
    _, e1, bc2s, e2 = state_bounds(step, h)
    dd = (np.sqrt(ref["v"] + bv) - np.sqrt(np.maximum(ref["v"] - bv, 0.0))) / bc2s
    ev = dd / (ref["denom"] - dd)
    assert np.all(ref["denom"] - dd > 0)
    bdp = ((1 + 2.0 ** -10) * (np.abs(ref["dp"]) * (6 * U + e1 + e2 + ev) + (h["lr"] / ref["bc1"]) / ref["denom"] * bm)
           + U * np.maximum(np.abs(p_old), np.abs(ref["p"])))
    return bm, bv, bdp


def make_state(n, seed, wide=False, first=True):
    """float32 p, m, v of n + TAIL floats; ``first``: the moments of a fresh optimizer (zeros)"""
    rng = np.random.default_rng(seed)
    N = n + TAIL
    p = rng.standard_normal(N).astype(np.float32)
    if first:
        return p, np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
    scale = 10.0 ** rng.uniform(-6, 2, N) if wide else 1.0
    m = (rng.standard_normal(N) * 0.1 * scale).astype(np.float32)
    v = ((rng.standard_normal(N) * scale) ** 2 * 0.01).astype(np.float32)
    return p, m, v


def make_grad(n, seed, wide=False):
    """float32 gradient of n + TAIL floats.  ``wide``: |g| log-uniform over 1e-20 .. 1e15 in one buffer.  Every seventh element is 0
    (with zero moments and no decay such an element must not move)."""
    rng = np.random.default_rng(seed)
    N = n + TAIL
    g = rng.standard_normal(N)
    if wide:
        g = np.sign(g) * 10.0 ** rng.uniform(-20, 15, N)
    g = g.astype(np.float32)
    g[::7] = 0.0
    return g
