"""Shared by the tests of the head's column kernels (head.hip behind nrm_colreduce, nrm_bn_finalize, nrm_bn_apply, nrm_bn_backward,
nrm_mul_bwd and nrm_concat_cols): numpy float64 statements of every entry written from the header comments of head.hip and
nrm_hotpath.h, the bound each element of each entry is held to, the cases, a float32 emulation of every kernel in the kernel's own
order, and the mutants the CPU test must see rejected.  ``check_case`` / ``check_finalize`` / ``check_concat`` run one case through a
backend -- the emulation here (CPU test) or the C entries (GPU test) -- and return the worst |got - ref| / bound per entry, so the CPU
test shows that the very check the GPU test applies rejects the mutants.

A reference reads what the kernel reads: the fp32 inputs promoted to float64 and the fp32 mean / rstd / s0 / s1 the kernel is GIVEN
(in a chain: the ones the previous entry returned), never recomputed ones.  momentum and eps are the float32 values the C entry
receives, promoted.

Bounds (U = 2^-24; the build uses no fast-math: every fp32 add, multiply, divide and square root is correctly rounded, a fused
multiply-add rounds once, so fusing only removes roundings from the counts; first order in U, the counts leave the second order room
except where noted).  k = 32 + 8 + ceil(R / 256): a term of a column sum passes through at most 32 additions in its thread (rows
ty, ty + 8, .. of a 256-row block; the first adds to 0 and is exact), 7 of the 8-way sum over ty in LDS and ceil(R / 256) float atomics
in any order (the first lands on 0 and is exact when nothing was there) -- k - 2 roundings at most, charged as k.

  nrm_colreduce mode 0, s0 of mode 2     k U sum_r |term|                              term = x or dy
  nrm_colreduce mode 1, s1 of mode 2     (k + 3) U sum_r |term|                        term = (x - mean)^2: x - mean rounds and enters
                                                                                       twice, the product rounds; term = dy (x - mean) rstd:
                                                                                       the difference and two products round
     onto prior content                  + ceil(R / 256) U |prior|                     the prior content enters the reference.  It is part
                                                                                       of the running sum of EVERY atomic of its column, so it
                                                                                       is charged one U per atomic: one U (the figure the issue
                                                                                       names) up to R = 256, two or three in the cases above it
  nrm_bn_finalize stage 0   mean         U |ref|                                       one division by float(R) (exact for R < 2^24)
                            running      4 U (|(1 - m) run| + |m v|)                   1 - m rounds, its product, v's division, m v, the sum
  nrm_bn_finalize stage 1   rstd         4 U |ref|                                     v's division and v + eps (halved by the square root),
                                                                                       the square root, the division: 3 U
                            running      6 U (|(1 - m) run| + |m v R / max(R - 1, 1)|)  v, m v, float(R) / float(R - 1), the product, the sum
  nrm_bn_apply                           4 U (|(x - mean) rstd gamma| + |beta|)        difference, two products, the sum
  nrm_bn_backward train                  8 U |gamma rstd| (|dy| + |s0 / R| + |xhat s1 / R|)    the xhat term: x - mean, xhat, xhat s1, 1 / R,
                                                                                       the product with it, its subtraction, gamma rstd and
                                                                                       the outer product: 8; the other two terms see fewer
     with add                            + U (|add| + |ref|)                           the final addition (ref includes add)
  nrm_bn_backward eval                   2 U |ref|  (+ the same add term)              two products; s0, s1, x, mean are not read
  nrm_mul_bwd                            bitwise float32(dy e), float32(dy g)          a product of two fp32 values is exact in float64
  nrm_concat_cols                        bitwise copy
Where a bound is 0 the result must be equal.  Every output buffer is prefilled with SENTINEL and has a row past R, columns [N, ld) and
four floats past a column vector's N: they must keep their bits.  Input padding holds NaN.

A constant column (family c) at 5.25: every partial sum 5.25 n, n <= 513, is exact, so s0 = 5.25 R, mean = 5.25, every x - mean = 0,
the column's sum of squares has bound 0 (must be equal to 0), and y = 0 rstd gamma + beta = beta bitwise.

Chained bounds (``chain_bounds``) for ops.batch_norm / ops.gate_block against float64 nn.BatchNorm1d: the table above carried through
mean -> variance -> rstd -> y, d gamma, d beta, dx and the running statistics per column, each step's bound on its input multiplied by
the derivative of the float64 expression (derivation at the function).

Mutants (each a one-line change of a kernel or launcher), the entries that must reject it at >= 4 x the bound, and where it applies:
  drop_last_row        r_hi = min(R, r_lo + rpb) - 1                      the column sums; R > 1
  drop_tail_block      the grid's y extent one block short                the column sums; R > 256
  column_border        col < N - 4: the last float4 is never written      every entry
  biased_running_var   no R / (R - 1)                                     running variance; R > 1, running present
  no_xhat_term         the xhat s1 / R term dropped                       backward train; R > 1 (at R = 1 every xhat is 0: no change)
  eval_uses_batch_terms  the train expression in eval mode                backward eval
  add_dropped          `add` not added                                    backward with add
  overwrite_instead_of_accumulate   a store in place of the atomic        the column sums onto prior content
  ld_taken_as_N        row r read / written at r N                        every matrix entry; ld > N and R > 1
  no_second_trip       the grid-stride loop's second trip not taken       apply, backward, mul_bwd at SECOND_TRIP
"""
import math

import numpy as np

U = 2.0 ** -24
EPS = 1e-5
RPB, TY, SLAB = 256, 8, 128                     # colred_launch: rows per block, blockDim.y, columns per block
EW_MAX_THREADS = 4096 * 256                     # ew_blocks caps the elementwise grids at 4096 blocks of 256 threads (one float4 each)
ROWS = (1, 7, 8, 9, 255, 256, 257, 513)
COLS = (4, 124, 128, 132, 264)
LD_EXTRA = (0, 4)
FAMILIES = ("a", "b", "c")
SECOND_TRIP = (4100, 1028)                      # R N / 4 = 1 053 700 > 4096 x 256
FIN_ROWS = (1, 2, 513, 30720)
FIN_COLS = (1, 255, 256, 257)
MOMENTA = (0.1, 1.0)
SENTINEL = np.float32(-12345.678)
TAIL = 4
INF = float("inf")

SUMS = ("colreduce0", "colreduce1", "colreduce2.s0", "colreduce2.s1")
SUMS_PRIOR = tuple(s + "+prior" for s in SUMS)
BWD = ("backward.train", "backward.train+add", "backward.eval", "backward.eval+add")
ELEMENTWISE = ("apply",) + BWD + ("mul_bwd.dg", "mul_bwd.de")
MUTANTS = {
    "drop_last_row": SUMS + SUMS_PRIOR,
    "drop_tail_block": SUMS + SUMS_PRIOR,
    "column_border": SUMS + SUMS_PRIOR + ("finalize0.mean", "finalize0.running", "finalize1.rstd", "finalize1.running") + ELEMENTWISE,
    "biased_running_var": ("finalize1.running",),
    "no_xhat_term": ("backward.train", "backward.train+add"),
    "eval_uses_batch_terms": ("backward.eval", "backward.eval+add"),
    "add_dropped": ("backward.train+add", "backward.eval+add"),
    "overwrite_instead_of_accumulate": SUMS_PRIOR,
    "ld_taken_as_N": SUMS + SUMS_PRIOR + ELEMENTWISE,
    "no_second_trip": ELEMENTWISE,
}


def applies(mutant, R, N, ld, second_trip=False):
    if mutant == "no_second_trip":
        return second_trip
    if second_trip and MUTANTS[mutant][0] in SUMS + SUMS_PRIOR + ("finalize1.running",):
        return False                                        # the second-trip case runs the elementwise kernels only
    return {"drop_last_row": R > 1, "drop_tail_block": R > RPB, "biased_running_var": R > 1, "no_xhat_term": R > 1,
            "ld_taken_as_N": ld > N and R > 1}.get(mutant, True)


def k_sum(R):
    return 32 + 8 + (R + RPB - 1) // RPB


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; where the bound is 0 the result must be equal; a non-finite result, or a violated
    equality -> inf"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    with np.errstate(all="ignore"):
        if got.size == 0:
            return 0.0
        if not (np.isfinite(got).all() and np.isfinite(ref).all() and np.isfinite(bound).all()):
            return INF
        err = np.abs(got - ref)
        zero = bound == 0
        if np.any(err[zero] != 0):
            return INF
        return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def same_bits(got, want):
    return 0.0 if np.array_equal(bits(got), bits(want)) else INF


# ------------------------------------------------------------------------------------------------ buffers
def matrix(values, ld, pad=np.nan):
    """[R + 1, ld] float32: the values in [:R, :N], ``pad`` in the columns [N, ld) and in the row past R"""
    R, N = values.shape
    m = np.full((R + 1, ld), pad, dtype=np.float32)
    m[:R, :N] = values
    return m


def out_matrix(R, ld):
    return np.full((R + 1, ld), SENTINEL, dtype=np.float32)


def vector(values, pad=np.nan):
    v = np.full(len(values) + TAIL, pad, dtype=np.float32)
    v[:len(values)] = values
    return v


def out_vector(N, fill=None):
    v = np.full(N + TAIL, SENTINEL, dtype=np.float32)
    if fill is not None:
        v[:N] = fill
    return v


def untouched(m, R, N):
    """the row past R and the columns [N, ld) of an output still hold the sentinel, bit for bit"""
    s = bits(SENTINEL)
    m = bits(m)
    return 0.0 if (m[R:] == s).all() and (m[:R, N:] == s).all() else INF


def untouched_tail(v, N):
    return 0.0 if (bits(v[N:]) == bits(SENTINEL)).all() else INF


# ------------------------------------------------------------------------------------------------ cases
def const_col(N):
    return N // 2


def make_case(R, N, ld, family, seed=0):
    """float32 inputs of one case: x = 3 N(0, 1) + 5 (a); column n scaled by 2^((n mod 7) - 3) (b: dy and add with it); one column
    constant at 5.25 (c)"""
    rng = np.random.default_rng([R, N, ld, "abc".index(family), seed])
    x = 3.0 * rng.standard_normal((R, N)) + 5.0
    dy, add = rng.standard_normal((R, N)), rng.standard_normal((R, N))
    if family == "b":
        sc = 2.0 ** ((np.arange(N) % 7) - 3.0)
        x, dy, add = x * sc, dy * sc, add * sc
    if family == "c":
        x[:, const_col(N)] = 5.25
    c = dict(R=R, N=N, ld=ld, family=family, x=f32(x), dy=f32(dy), add=f32(add),
             gamma=f32(1.0 + 0.25 * rng.standard_normal(N)), beta=f32(rng.standard_normal(N)),
             run_mean=f32(5.0 + rng.standard_normal(N)), run_var=f32(9.0 + rng.standard_normal(N)),
             g=f32(rng.standard_normal((R, N))), e=f32(rng.standard_normal((R, N))),
             prior=[f32(math.sqrt(R) * rng.standard_normal(N)) for _ in range(4)])
    return c


def column_cases():
    return [(R, N, N + extra, fam) for R in ROWS for N in COLS for extra in LD_EXTRA for fam in FAMILIES]


# ------------------------------------------------------------------------------------------------ float64 statements
def ref_colreduce(mode, x, dy, mean, rstd, R):
    """-> [(ref, bound)] of s0 (and s1 for mode 2) before any prior content; x, dy [R, N]; mean, rstd [N] as given"""
    x, k = f64(x), k_sum(R)
    if mode == 0:
        return [(x.sum(0), k * U * np.abs(x).sum(0))]
    d = x - f64(mean)
    if mode == 1:
        return [((d * d).sum(0), (k + 3) * U * (d * d).sum(0))]
    t = f64(dy) * d * f64(rstd)
    return [(f64(dy).sum(0), k * U * np.abs(f64(dy)).sum(0)), (t.sum(0), (k + 3) * U * np.abs(t).sum(0))]


def prior_bound(prior, R):
    return ((R + RPB - 1) // RPB) * U * np.abs(f64(prior))


def ref_finalize(stage, s, running, R, momentum, eps):
    """-> (out, bound, running', bound) (the last two None without running); momentum, eps: the float32 values, promoted"""
    m, e = float(np.float32(momentum)), float(np.float32(eps))
    v = f64(s) / R
    if stage == 0:
        out, b_out, new, n_round = v, U * np.abs(v), v, 4
    else:
        out = 1.0 / np.sqrt(v + e)
        b_out, new, n_round = 4 * U * np.abs(out), v * (R / max(R - 1, 1)), 6
    if running is None:
        return out, b_out, None, None
    a, b = (1.0 - m) * f64(running), m * new
    return out, b_out, a + b, n_round * U * (np.abs(a) + np.abs(b))


def ref_apply(x, mean, rstd, gamma, beta):
    t = (f64(x) - f64(mean)) * f64(rstd) * f64(gamma)
    return t + f64(beta), 4 * U * (np.abs(t) + np.abs(f64(beta)))


def ref_backward(x, dy, mean, rstd, gamma, s0, s1, add, R, training):
    kk = f64(gamma) * f64(rstd)
    if training:
        xh = (f64(x) - f64(mean)) * f64(rstd)
        t0, t1 = f64(s0) / R, xh * f64(s1) / R
        ref = kk * (f64(dy) - t0 - t1)
        bound = 8 * U * np.abs(kk) * (np.abs(f64(dy)) + np.abs(t0) + np.abs(t1))
    else:
        ref = kk * f64(dy)
        bound = 2 * U * np.abs(ref)
    if add is not None:
        ref = ref + f64(add)
        bound = bound + U * (np.abs(f64(add)) + np.abs(ref))
    return ref, bound


def ref_mul_bwd(dy, g, e):
    return f32(f64(dy) * f64(e)), f32(f64(dy) * f64(g))           # exact products, rounded once


def chain_bounds(x, dy, add, gamma, beta, run_mean, run_var, momentum, eps, training):
    """Float64 BatchNorm1d of the fp32 inputs and the bound on each fp32 result of the kernel chain, per element / column.

    train:  Bmean = k U sum|x| / R + U |mean|.   The kernel's sum of squares is around ITS mean m': sum (x - m')^2 = R var + R (m' - mean)^2, so
            Bs1 = (k + 3) U (R var + R Bmean^2) + R Bmean^2 and Bvar = Bs1 / R + U var.   rstd = (var + eps)^-1/2 has derivative
            -rstd^3 / 2, largest at the smallest variance in reach, r_up = (max(var - Bvar, 0) + eps)^-1/2:  Brstd = r_up^3 (Bvar + |eps32 - eps|) / 2
            + 4 U r_up (the module's eps is the double, the kernel's the float).   Bxhat = r_up Bmean + |x - mean| Brstd.
            By = 4 U (|xhat gamma| + |beta|) + |gamma| Bxhat.   Bdbeta = k U sum|dy|.   Bdgamma = (k + 3) U sum|dy| (|xhat| + Bxhat) + sum|dy| Bxhat.
            inner = dy - dbeta / R - xhat dgamma / R:  Binner = Bdbeta / R + (|xhat| + Bxhat) Bdgamma / R + Bxhat |dgamma| / R.
            Bdx = 8 U |gamma| r_up (|dy| + |dbeta / R| + |xhat dgamma / R| + Binner) + |gamma| Brstd |inner| + |gamma| r_up Binner + U (|add| + |ref|).
            running: the finalize bound + m (Bmean or Bvar R / (R - 1)) + |m32 - m| (|run| + |new|)  (the module's momentum is the double).
    eval:   mean = running_mean is read as it is; rstd = torch.rsqrt(running_var + eps) in fp32 (ATen, not a kernel of this project): 1 ulp = 2 U
            for rsqrt, U for the sum, U to spare: Brstd = 4 U rstd + rstd^3 |eps32 - eps| / 2, and the lines above with Bmean = 0 and eval's dx.
    Everything times 1 + 2^-10 for the products of these first-order terms."""
    x, dy, gamma, beta = f64(x), f64(dy), f64(gamma), f64(beta)
    R = x.shape[0]
    k, m32, e32 = k_sum(R), float(np.float32(momentum)), float(np.float32(eps))
    out = {}
    if training:
        mean = x.sum(0) / R
        var = ((x - mean) ** 2).sum(0) / R
        b_mean = k * U * np.abs(x).sum(0) / R + U * np.abs(mean)
        b_s1 = (k + 3) * U * (R * var + R * b_mean ** 2) + R * b_mean ** 2
        b_var = b_s1 / R + U * var
        r_up = 1.0 / np.sqrt(np.maximum(var - b_var, 0.0) + eps)
        rstd = 1.0 / np.sqrt(var + eps)
        b_rstd = 0.5 * r_up ** 3 * (b_var + abs(e32 - eps)) + 4 * U * r_up
        unb = R / max(R - 1, 1)
        for name, run, new, nr, b_new in (("running_mean", f64(run_mean), mean, 4, b_mean), ("running_var", f64(run_var), var * unb, 6, b_var * unb)):
            a, b = (1 - momentum) * run, momentum * new
            out[name] = (a + b, nr * U * (np.abs(a) + np.abs(b)) + momentum * b_new + abs(m32 - momentum) * (np.abs(run) + np.abs(new)))
    else:
        mean, var = f64(run_mean), f64(run_var)
        rstd = r_up = 1.0 / np.sqrt(var + eps)
        b_mean = np.zeros_like(mean)
        b_rstd = 4 * U * rstd + 0.5 * rstd ** 3 * abs(e32 - eps)
    d = x - mean
    xh = d * rstd
    b_xh = r_up * b_mean + np.abs(d) * b_rstd
    out["y"] = (xh * gamma + beta, 4 * U * (np.abs(xh * gamma) + np.abs(beta)) + np.abs(gamma) * b_xh)
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    b_db = k * U * np.abs(dy).sum(0)
    b_dg = (k + 3) * U * (np.abs(dy) * (np.abs(xh) + b_xh)).sum(0) + (np.abs(dy) * b_xh).sum(0)
    out["dbeta"], out["dgamma"] = (dbeta, b_db), (dgamma, b_dg)
    if training:
        inner = dy - dbeta / R - xh * dgamma / R
        b_inner = b_db / R + (np.abs(xh) + b_xh) * b_dg / R + b_xh * np.abs(dgamma) / R
        ref = gamma * rstd * inner
        b_dx = (8 * U * np.abs(gamma) * r_up * (np.abs(dy) + np.abs(dbeta / R) + np.abs(xh * dgamma / R) + b_inner)
                + np.abs(gamma) * b_rstd * np.abs(inner) + np.abs(gamma) * r_up * b_inner)
    else:
        ref = gamma * rstd * dy
        b_dx = 2 * U * np.abs(ref) + np.abs(gamma * dy) * b_rstd
    if add is not None:
        ref = ref + f64(add)
        b_dx = b_dx + U * (np.abs(f64(add)) + np.abs(ref))
    out["dx"] = (ref, b_dx)
    return {name: (r, (1 + 2.0 ** -10) * b) for name, (r, b) in out.items()}


# ------------------------------------------------------------------------------------------------ the float32 emulation
class Emulated:
    """Every kernel in float32 in its own order (products and sums rounded one by one: fusing would only remove roundings).
    ``order`` = -1: the blocks' atomics arrive in reverse.  ``mutant``: one of MUTANTS."""

    def __init__(self, mutant=None, order=1):
        self.mutant, self.order = mutant, order

    def _rows(self, m, R, N, ld):
        """the [R, N] block a kernel reads from / writes to a [R + 1, ld] buffer"""
        if self.mutant == "ld_taken_as_N":
            return m.reshape(-1)[:R * N].reshape(R, N)
        return m[:R, :N]

    def _cols(self, N):
        return N - 4 if self.mutant == "column_border" else N

    def _trips(self, R, N):
        """mask [R, N] of the elements the grid-stride loop reaches"""
        keep = np.ones((R, N), dtype=bool)
        if self.mutant == "no_second_trip":
            keep.reshape(-1, 4)[EW_MAX_THREADS:] = False
        keep[:, self._cols(N):] = False
        return keep

    def colreduce(self, mode, x, dy, mean, rstd, s0, s1, R, N, ld):
        s0, s1 = s0.copy(), None if s1 is None else s1.copy()
        X = self._rows(x, R, N, ld)
        with np.errstate(all="ignore"):
            if mode == 0:
                terms = [X]
            elif mode == 1:
                d = X - mean[:N]
                terms = [d * d]
            else:
                G = self._rows(dy, R, N, ld)
                terms = [G, (G * (X - mean[:N])) * rstd[:N]]
            r_end = R - 1 if self.mutant == "drop_last_row" else R
            nb = (R + RPB - 1) // RPB - (1 if self.mutant == "drop_tail_block" else 0)
            nc = self._cols(N)
            if self.mutant == "overwrite_instead_of_accumulate":
                s0[:nc] = 0
                if s1 is not None:
                    s1[:nc] = 0
            for b in list(range(nb))[::self.order]:
                lo, hi = b * RPB, min(r_end, (b + 1) * RPB)
                for t, s in zip(terms, (s0, s1)):
                    acc = np.zeros((TY, N), dtype=np.float32)
                    for r0 in range(lo, hi, TY):                       # thread ty adds row r0 + ty
                        n = min(TY, hi - r0)
                        acc[:n] += t[r0:r0 + n]
                    tot = acc[0].copy()
                    for y in range(1, TY):
                        tot += acc[y]
                    s[:nc] += tot[:nc]
        return s0, s1

    def finalize(self, stage, s, out, running, R, N, momentum, eps):
        out, running = out.copy(), None if running is None else running.copy()
        m, e, one = np.float32(momentum), np.float32(eps), np.float32(1)
        n = self._cols(N)
        with np.errstate(all="ignore"):
            v = s[:n] / np.float32(R)
            if stage == 0:
                out[:n], new = v, m * v
            else:
                out[:n] = one / np.sqrt(v + e)
                new = m * v if self.mutant == "biased_running_var" else (m * v) * (np.float32(R) / np.float32(max(R - 1, 1)))
            if running is not None:
                running[:n] = (one - m) * running[:n] + new
        return out, running

    def apply(self, x, mean, rstd, gamma, beta, y, R, N, ld):
        y = y.copy()
        with np.errstate(all="ignore"):
            v = (((self._rows(x, R, N, ld) - mean[:N]) * rstd[:N]) * gamma[:N]) + beta[:N]
        keep = self._trips(R, N)
        self._rows(y, R, N, ld)[keep] = v[keep]
        return y

    def backward(self, x, dy, mean, rstd, gamma, s0, s1, add, dx, R, N, ld, training):
        dx = dx.copy()
        G = self._rows(dy, R, N, ld)
        with np.errstate(all="ignore"):
            kk = gamma[:N] * rstd[:N]
            if training or self.mutant == "eval_uses_batch_terms":
                inv = np.float32(1) / np.float32(R)
                xh = (self._rows(x, R, N, ld) - mean[:N]) * rstd[:N]
                inner = G - s0[:N] * inv
                if self.mutant != "no_xhat_term":
                    inner = inner - (xh * s1[:N]) * inv
                v = kk * inner
            else:
                v = kk * G
            if add is not None and self.mutant != "add_dropped":
                v = v + self._rows(add, R, N, ld)
        keep = self._trips(R, N)
        self._rows(dx, R, N, ld)[keep] = v[keep]
        return dx

    def mul_bwd(self, dy, lddy, g, ldg, e, lde, dg, de, ldo, R, N):
        dg, de = dg.copy(), de.copy()
        keep = self._trips(R, N)
        with np.errstate(all="ignore"):
            d = self._rows(dy, R, N, lddy)
            self._rows(dg, R, N, ldo)[keep] = (d * self._rows(e, R, N, lde))[keep]
            self._rows(de, R, N, ldo)[keep] = (d * self._rows(g, R, N, ldg))[keep]
        return dg, de

    def concat(self, parts, out, ldo, R):
        out = out.copy()
        total = sum(p["width"] for p in parts)
        vec = ldo % 4 == 0 and total % 4 == 0 and all(p["width"] % 4 == 0 and p["ld"] % 4 == 0 and p["off"] % 4 == 0 for p in parts)
        stop = total - (4 if vec else 1) if self.mutant == "column_border" else total
        c = 0
        for p in parts:
            ld = p["width"] if self.mutant == "ld_taken_as_N" else p["ld"]
            src = p["buf"][p["off"]:]
            for r in range(R):
                w = max(0, min(p["width"], stop - c))
                out[r, c:c + w] = src[r * ld:r * ld + w]
            c += p["width"]
        return out


# ------------------------------------------------------------------------------------------------ one case through a backend
def _worst(res, name, *values):
    res[name] = max([res.get(name, 0.0)] + list(values))


def check_case(be, c, elementwise_only=False):
    """Run every entry on one case through backend ``be``, each entry judged against the float64 statement of what it was given.
    -> {entry: worst |got - ref| / bound}; inf: a non-finite result, a broken equality, or a changed sentinel."""
    R, N, ld, res = c["R"], c["N"], c["ld"], {}
    x, dy, add = matrix(c["x"], ld), matrix(c["dy"], ld), matrix(c["add"], ld)
    gamma, beta = vector(c["gamma"]), vector(c["beta"])
    momentum, eps = 0.1, EPS
    with np.errstate(all="ignore"):
        if elementwise_only:                                   # given statistics: float64 ones, rounded
            mean64 = f64(c["x"]).mean(0)
            mean = vector(f32(mean64))
            rstd = vector(f32(1.0 / np.sqrt(((f64(c["x"]) - mean64) ** 2).mean(0) + EPS)))
            xh = (f64(c["x"]) - mean64) * f64(rstd[:N])
            g0, g1 = vector(f32(f64(c["dy"]).sum(0))), vector(f32((f64(c["dy"]) * xh).sum(0)))
        else:
            def sums(mode, names, mean=None, rstd=None):
                """zero-filled accumulators, then accumulators with content -> the zero-filled run's results"""
                refs = ref_colreduce(mode, c["x"], c["dy"], None if mean is None else mean[:N], None if rstd is None else rstd[:N], R)
                first = None
                for prior in (False, True):
                    bufs = [out_vector(N, c["prior"][i] if prior else 0.0) for i in range(len(refs))]
                    got = be.colreduce(mode, x, dy if mode == 2 else None, mean, rstd, bufs[0], bufs[1] if mode == 2 else None, R, N, ld)
                    for i, (name, (ref, bound)) in enumerate(zip(names, refs)):
                        if prior:
                            ref, bound = ref + f64(c["prior"][i]), bound + prior_bound(c["prior"][i], R)
                        _worst(res, name + ("+prior" if prior else ""), ratio(got[i][:N], ref, bound), untouched_tail(got[i], N))
                    first = first or got
                return first
            s0 = sums(0, ["colreduce0"])[0]
            mean, run = be.finalize(0, s0, out_vector(N), out_vector(N, c["run_mean"]), R, N, momentum, eps)
            ref, b, rref, rb = ref_finalize(0, s0[:N], c["run_mean"], R, momentum, eps)
            _worst(res, "finalize0.mean", ratio(mean[:N], ref, b), untouched_tail(mean, N))
            _worst(res, "finalize0.running", ratio(run[:N], rref, rb), untouched_tail(run, N))
            s1 = sums(1, ["colreduce1"], mean=mean)[0]
            rstd, run = be.finalize(1, s1, out_vector(N), out_vector(N, c["run_var"]), R, N, momentum, eps)
            ref, b, rref, rb = ref_finalize(1, s1[:N], c["run_var"], R, momentum, eps)
            _worst(res, "finalize1.rstd", ratio(rstd[:N], ref, b), untouched_tail(rstd, N))
            _worst(res, "finalize1.running", ratio(run[:N], rref, rb), untouched_tail(run, N))
            if c["family"] == "c":                                 # exact sums: mean 5.25, a sum of squares equal to 0, rstd = eps^-1/2
                j = const_col(N)
                _worst(res, "colreduce0", same_bits(s0[j], np.float32(5.25 * R)))
                _worst(res, "finalize0.mean", same_bits(mean[j], np.float32(5.25)))
                _worst(res, "colreduce1", same_bits(s1[j], np.float32(0.0)))
            g0, g1 = sums(2, ["colreduce2.s0", "colreduce2.s1"], mean=mean, rstd=rstd)
        y = be.apply(x, mean, rstd, gamma, beta, out_matrix(R, ld), R, N, ld)
        ref, b = ref_apply(c["x"], mean[:N], rstd[:N], c["gamma"], c["beta"])
        _worst(res, "apply", ratio(y[:R, :N], ref, b), untouched(y, R, N))
        if c["family"] == "c" and not elementwise_only:
            j = const_col(N)
            _worst(res, "apply", same_bits(y[:R, j], np.full(R, c["beta"][j])))
        for training in (1, 0):
            for a in (None, add):
                dx = be.backward(x, dy, mean, rstd, gamma, g0, g1, a, out_matrix(R, ld), R, N, ld, training)
                ref, b = ref_backward(c["x"], c["dy"], mean[:N], rstd[:N], c["gamma"], g0[:N], g1[:N], None if a is None else c["add"], R, training)
                _worst(res, "backward." + ("train" if training else "eval") + ("" if a is None else "+add"), ratio(dx[:R, :N], ref, b), untouched(dx, R, N))
        # the gate product's backward with four different leading dimensions
        ldg, lde, ldo = N + 8, N + 12, (N + 4 if ld == N else N)
        dg, de = be.mul_bwd(dy, ld, matrix(c["g"], ldg), ldg, matrix(c["e"], lde), lde, out_matrix(R, ldo), out_matrix(R, ldo), ldo, R, N)
        rg, re = ref_mul_bwd(c["dy"], c["g"], c["e"])
        _worst(res, "mul_bwd.dg", same_bits(dg[:R, :N], rg), untouched(dg, R, N))
        _worst(res, "mul_bwd.de", same_bits(de[:R, :N], re), untouched(de, R, N))
    return res


def finalize_cases():
    return [(R, N, running, m) for R in FIN_ROWS for N in FIN_COLS for running in (True, False) for m in MOMENTA]


def check_finalize(be, R, N, running, momentum):
    """both stages on sums of the size a batch of R rows gives; for N > 1 one entry of the sum of squares is 0 (a constant column)"""
    rng = np.random.default_rng([R, N, int(running), int(momentum * 10)])
    res = {}
    for stage in (0, 1):
        s = R * (5.0 + rng.standard_normal(N)) if stage == 0 else R * rng.uniform(0.0, 18.0, N)
        if stage == 1 and N > 1:
            s[N // 2] = 0.0
        s = vector(f32(s))
        run0 = f32(5.0 + rng.standard_normal(N))
        out, run = be.finalize(stage, s, out_vector(N), out_vector(N, run0) if running else None, R, N, momentum, EPS)
        ref, b, rref, rb = ref_finalize(stage, s[:N], run0 if running else None, R, momentum, EPS)
        name = "finalize%d." % stage
        _worst(res, name + ("mean" if stage == 0 else "rstd"), ratio(out[:N], ref, b), untouched_tail(out, N))
        if running:
            _worst(res, name + "running", ratio(run[:N], rref, rb), untouched_tail(run, N))
        else:
            assert run is None
    return res


# nrm_concat_cols: (width, leading dimension, offset of the source in floats from a 16-byte aligned base) per part
CONCAT_SPECS = {
    "one part, vector": [(8, 8, 0)],
    "three parts, vector, one ld above its width": [(4, 4, 0), (12, 20, 0), (8, 8, 0)],
    "eight parts, vector": [(4, 4, 0), (8, 12, 0), (4, 4, 0), (12, 12, 0), (4, 8, 0), (4, 4, 0), (8, 8, 0), (4, 4, 0)],
    "a width of 3, scalar": [(4, 4, 0), (3, 3, 0), (8, 8, 0)],
    "one part of width 3, scalar": [(3, 5, 0)],
    "a source 4 bytes off, scalar": [(4, 4, 0), (8, 12, 1), (4, 4, 0)],
    "eight parts, scalar, ld above the width": [(1, 2, 0), (2, 2, 0), (3, 7, 0), (4, 4, 0), (5, 6, 0), (6, 6, 0), (7, 9, 0), (8, 8, 0)],
}
CONCAT_ROWS = (1, 7, 257)


def check_concat(be, spec, R, ldo_extra):
    rng = np.random.default_rng([len(spec), R, ldo_extra])
    parts, want = [], []
    for width, ld, off in spec:
        buf = np.full(off + R * ld + TAIL, np.nan, dtype=np.float32)
        vals = f32(rng.standard_normal((R, width)))
        for r in range(R):
            buf[off + r * ld:off + r * ld + width] = vals[r]
        parts.append(dict(buf=buf, off=off, ld=ld, width=width))
        want.append(vals)
    total = sum(p["width"] for p in parts)
    ldo = (total + 3) // 4 * 4 + ldo_extra
    out = be.concat(parts, out_matrix(R, ldo), ldo, R)
    return {"concat": max(same_bits(out[:R, :total], np.concatenate(want, axis=1)), untouched(out, R, total))}
