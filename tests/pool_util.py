"""Shared by the tests of the dense pool pair (pool_loss.hip: bmm_rows_kernel behind nrm_pool_bmm, rowdot_kernel behind nrm_pool_rowdot):
numpy float64 statements written from the header comments of pool_loss.hip and nrm_hotpath.h, the bound each element is held to, the
cases, a float32 emulation of both kernels in their own order, and the mutants the CPU test must see rejected.  ``check_bmm`` and
``check_rowdot`` run one case through a backend -- the emulation here (CPU test) or the C entries (GPU test) -- and return the worst
|got - ref| / bound, so the CPU test shows that the very check the GPU test applies rejects the mutants.

nrm_pool_bmm     out[b,i,:] (+)= sum_j W[b,i,j] X[b,j,:]       W element (b,i,j) at W[b wsb + i wsi + j wsj]; X rows ldx apart
nrm_pool_rowdot  ds[b,t,h]   = sum_d g[b,t,d] h[b,h,d]         g rows ldg apart; the first zero_n floats of zero_out become +0.0

Bounds (U = 2^-24, first order in U).  The fp32 MFMA is a k-ordered chain of fused multiply-adds, one rounding each, from the accumulator
it is given:
  pool_bmm      J U sum_j |W X|         one wave per task: a J-long chain from 0, a term sees at most J roundings.  JSPLIT: the four
                                        waves' chains (whole rounds of 4 rows: ceil(J / 16) * 4 rows each, the later ones shorter or empty)
                                        and three additions; adding an empty wave's 0 is exact and a wave with rows has at least one, so
                                        a term of wave 0 sees its chain and at most one rounding per other wave with rows: J again
     accumulate + U (|prior| + |ref|)   one addition onto what is there (ref includes the prior content)
  pool_rowdot   D U sum_d |g h|         a D-long chain: chunks of 16 columns in order, within a chunk the columns 4 q + e for e = 0 .. 3,
                                        q = 0 .. 3 (MFMA e contracts the columns {16 c + 4 q + e}); columns past D are products of zeros
One-hot W (a single 1.0 per row, at a random j): every other product is an exact zero in either form, so without `accumulate`
out[b,i,:] = X[b,j,:] BITWISE -- a wrong j, tile or lane shows.  One-hot g rows give ds[b,t,h] = h[b,h,d] bitwise.
Where a bound is 0 the result must be equal.  Four SENTINEL floats behind every output must keep their bits; X and g padding holds NaN.

Mutants (each a one-line change of a kernel) and where they apply:
  drop_last_j               j < j_hi - 1: the last row of a wave's range is not read                pool_bmm
  jsplit_quarter_lost       the partial tile of the last of waves 1 .. 3 that has rows is not added   pool_bmm, JSPLIT form, J >= 5 (the kernel
                            cuts in whole rounds of 4 rows: up to J = 4 wave 0 holds the whole range and there is no partial to lose)
  rows_swapped_within_tile  output rows i and i ^ 1 of a tile change places                         pool_bmm, I >= 2
  accumulate_overwrites     the store without the read                                              pool_bmm with accumulate
  last_chunk_dropped        nchunk = D / 16                                                         pool_rowdot, D % 16 != 0
  ldx_taken_as_D            rows taken as D apart                                                   pool_bmm: ldx > D, J > 1; pool_rowdot: ldg > D, T > 1
The three mutants that lose terms apply to the dense families: a one-hot operand has one term per row, lost only where the 1.0 happens to
sit in the part that is dropped.  rows_swapped_within_tile does not apply to one-hot W at J = 1, where every row of W is the same row.
"""
import numpy as np

U = 2.0 ** -24
SENTINEL = np.float32(-12345.678)
TAIL = 4
INF = float("inf")

BMM_I = (1, 15, 16, 17, 63, 64, 65)
BMM_J = (1, 3, 4, 5, 31, 32, 33, 130)
BMM_D = (4, 60, 64, 68, 132)
FORMS = (None, "0", "1")                                # NRM_POOL_JSPLIT: as dispatched, one wave per task, one workgroup per task
LAYOUTS = ("s", "sT")                                   # W = s [B, I, J] (wsi = J, wsj = 1);  W = s^T of a [B, J, I] array (wsi = 1, wsj = I)
BMM_FAMILIES = ("normal", "scaled", "onehot")
ROWDOT_T = (1, 15, 16, 17, 33)
ROWDOT_H = (1, 16, 63, 64, 65, 130)
ROWDOT_D = (4, 12, 16, 20, 36, 1024)
ROWDOT_B = (1, 3)
ROWDOT_FAMILIES = ("normal", "onehot")
ZERO_N = (0, 3, 300)
ZERO_LEN = 304
BMM_MUTANTS = ("drop_last_j", "jsplit_quarter_lost", "rows_swapped_within_tile", "accumulate_overwrites", "ldx_taken_as_D")
ROWDOT_MUTANTS = ("last_chunk_dropped", "ldx_taken_as_D")


def bmm_shapes():
    """(B, I, J, D): I x J around the 16-row tile, the 64-row group and the rounds of 4 rows, D around the 64-column slab, one impression"""
    return ([(3, i, j, 68) for i in BMM_I for j in BMM_J] + [(3, 17, 33, d) for d in BMM_D if d != 68]
            + [(1, 17, 33, 68), (1, 65, 130, 68)])


def rowdot_shapes():
    return [(b, t, h, d) for b in ROWDOT_B for t in ROWDOT_T for h in ROWDOT_H for d in ROWDOT_D]


def jsplit_taken(form, B, I, J, D):
    """bmm_rows_plan: which form a launch takes"""
    if form is not None:
        return form == "1"
    return B * ((D + 63) // 64) * ((I + 63) // 64) <= 1024 and J >= 32


def bmm_applies(mutant, family, jsplit, I, J, D, ldx, accumulate):
    dense = family != "onehot"
    return {"drop_last_j": dense, "jsplit_quarter_lost": dense and jsplit and J >= 5, "rows_swapped_within_tile": I >= 2 and (dense or J > 1),
            "accumulate_overwrites": bool(accumulate), "ldx_taken_as_D": ldx > D and J > 1}[mutant]


def rowdot_applies(mutant, family, T, D, ldg):
    return {"last_chunk_dropped": family != "onehot" and D % 16 != 0, "ldx_taken_as_D": ldg > D and T > 1}[mutant]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the result must be equal; a non-finite result or a violated equality -> inf"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    with np.errstate(all="ignore"):
        if not np.isfinite(got).all():
            return INF
        err = np.abs(got - ref)
        zero = bound == 0
        if np.any(err[zero] != 0):
            return INF
        return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def same_bits(got, want):
    return 0.0 if np.array_equal(bits(got), bits(want)) else INF


def tail_kept(buf, n):
    return 0.0 if (bits(buf[n:]) == bits(SENTINEL)).all() else INF


def _rows_buffer(vals, ld):
    """[B, n, D] values -> flat float32 of B n ld + TAIL floats, NaN in the columns [D, ld) and behind the last row"""
    B, n, D = vals.shape
    m = np.full((B, n, ld), np.nan, dtype=np.float32)
    m[:, :, :D] = vals
    return np.concatenate([m.reshape(-1), np.full(TAIL, np.nan, dtype=np.float32)])


# ------------------------------------------------------------------------------------------------ nrm_pool_bmm
def make_bmm(B, I, J, D, layout, ldx, family, seed=0):
    rng = np.random.default_rng([B, I, J, D, LAYOUTS.index(layout), ldx, BMM_FAMILIES.index(family), seed])
    X = rng.standard_normal((B, J, D))
    hot = None
    if family == "onehot":
        hot = rng.integers(0, J, (B, I))
        W = np.zeros((B, I, J))
        np.put_along_axis(W, hot[:, :, None], 1.0, axis=2)
    else:
        W = rng.standard_normal((B, I, J))
        if family == "scaled":                          # row i of W and column d of X by small powers of two
            W = W * 2.0 ** ((np.arange(I) % 5) - 2.0)[None, :, None]
            X = X * 2.0 ** ((np.arange(D) % 7) - 3.0)[None, None, :]
    W, X = f32(W), f32(X)
    if layout == "s":
        wmem, strides = W.reshape(-1).copy(), (I * J, J, 1)
    else:
        wmem, strides = np.ascontiguousarray(W.transpose(0, 2, 1)).reshape(-1), (I * J, 1, I)
    wmem = np.concatenate([wmem, np.full(TAIL, np.nan, dtype=np.float32)])
    prior = f32(rng.standard_normal((B, I, D)) * np.sqrt(J))
    ref = np.matmul(f64(W), f64(X))
    mag = np.matmul(np.abs(f64(W)), np.abs(f64(X)))
    return dict(B=B, I=I, J=J, D=D, ldx=ldx, family=family, W=W, X=X, wmem=wmem, strides=strides, xmem=_rows_buffer(X, ldx), prior=prior,
                ref=ref, mag=mag, hot=hot)


def bmm_bound(c, accumulate):
    ref, bound = c["ref"], c["J"] * U * c["mag"]
    if accumulate:
        ref = ref + f64(c["prior"])
        bound = bound + U * (np.abs(f64(c["prior"])) + np.abs(ref))
    return ref, bound


def check_bmm(be, c, accumulate, form):
    B, I, J, D = c["B"], c["I"], c["J"], c["D"]
    n = B * I * D
    out = np.full(n + TAIL, SENTINEL, dtype=np.float32)
    if accumulate:
        out[:n] = c["prior"].reshape(-1)
    got = be.bmm(c["wmem"], *c["strides"], c["xmem"], c["ldx"], out, B, I, J, D, accumulate, form)
    ref, bound = bmm_bound(c, accumulate)
    res = {"pool_bmm": max(ratio(got[:n].reshape(B, I, D), ref, bound), tail_kept(got, n))}
    if c["family"] == "onehot" and not accumulate:
        want = np.take_along_axis(c["X"], c["hot"][:, :, None], axis=1)
        res["pool_bmm.onehot"] = same_bits(got[:n].reshape(B, I, D), want)
    return res


# ------------------------------------------------------------------------------------------------ nrm_pool_rowdot
def make_rowdot(B, T, H, D, ldg, family, seed=0):
    rng = np.random.default_rng([B, T, H, D, ldg, ROWDOT_FAMILIES.index(family), seed])
    h = f32(rng.standard_normal((B, H, D)))
    hot = None
    if family == "onehot":
        hot = rng.integers(0, D, (B, T))
        g = np.zeros((B, T, D))
        np.put_along_axis(g, hot[:, :, None], 1.0, axis=2)
    else:
        g = rng.standard_normal((B, T, D))
    g = f32(g)
    ref = np.matmul(f64(g), f64(h).transpose(0, 2, 1))
    mag = np.matmul(np.abs(f64(g)), np.abs(f64(h)).transpose(0, 2, 1))
    hmem = np.concatenate([h.reshape(-1), np.full(TAIL, np.nan, dtype=np.float32)])
    return dict(B=B, T=T, H=H, D=D, ldg=ldg, family=family, g=g, h=h, gmem=_rows_buffer(g, ldg), hmem=hmem, ref=ref, mag=mag, hot=hot)


def check_rowdot(be, c, zero_n):
    B, T, H, D = c["B"], c["T"], c["H"], c["D"]
    n = B * T * H
    ds = np.full(n + TAIL, SENTINEL, dtype=np.float32)
    zero = np.full(ZERO_LEN, np.nan, dtype=np.float32)
    got, zgot = be.rowdot(c["gmem"], c["ldg"], c["hmem"], ds, B, T, H, D, zero, zero_n)
    res = {"pool_rowdot": max(ratio(got[:n].reshape(B, T, H), c["ref"], D * U * c["mag"]), tail_kept(got, n))}
    zb = bits(zgot)
    res["pool_rowdot.zero"] = 0.0 if not zb[:zero_n].any() and np.array_equal(zb[zero_n:], bits(zero)[zero_n:]) else INF
    if c["family"] == "onehot":
        want = np.take_along_axis(c["h"].transpose(0, 2, 1), c["hot"][:, :, None], axis=1)          # [B, T, H]: h[b, :, d_t]
        res["pool_rowdot.onehot"] = same_bits(got[:n].reshape(B, T, H), want)
    return res


# ------------------------------------------------------------------------------------------------ the float32 emulation
def _fma(a, b, acc):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64; the sum rounds to 53 bits and then to 24 (a double
    rounding differs from the single one only on a tie of the second, a case in 2^29)"""
    return (f64(a) * f64(b) + f64(acc)).astype(np.float32)


def _strided_rows(mem, base, n, ld, D):
    """[n, D]: the floats base + r ld .. + D of a flat buffer, r < n"""
    return mem[base + np.arange(n)[:, None] * ld + np.arange(D)[None, :]]


class Emulated:
    """Both kernels in float32 in their own order.  ``form`` of bmm: as the launcher's plan takes it."""

    def __init__(self, mutant=None):
        self.mutant = mutant

    def bmm(self, wmem, wsb, wsi, wsj, xmem, ldx, out, B, I, J, D, accumulate, form):
        out = out.copy()
        b_, i_, j_ = np.arange(B)[:, None, None], np.arange(I)[None, :, None], np.arange(J)[None, None, :]
        W = wmem[b_ * wsb + i_ * wsi + j_ * wsj]                                      # [B, I, J]
        ld = D if self.mutant == "ldx_taken_as_D" else ldx
        X = np.stack([_strided_rows(xmem, b * J * ldx, J, ld, D) for b in range(B)])          # [B, J, D] as the kernel strides it
        jsplit = jsplit_taken(form, B, I, J, D)
        jq = (J + 15) // 16 * 4 if jsplit else J
        parts = []
        with np.errstate(all="ignore"):
            for w in range(4 if jsplit else 1):
                lo, hi = w * jq, min(J, (w + 1) * jq)
                if self.mutant == "drop_last_j":
                    hi -= 1
                acc = np.zeros((B, I, D), dtype=np.float32)
                for j in range(lo, hi):
                    acc = _fma(W[:, :, j, None], X[:, j, None, :], acc)
                parts.append((acc, lo < min(J, (w + 1) * jq)))
            acc = parts[0][0]
            lost = max([w for w in range(1, len(parts)) if parts[w][1]], default=None) if self.mutant == "jsplit_quarter_lost" else None
            for w in range(1, len(parts)):
                if w != lost:
                    acc = acc + parts[w][0]
            if self.mutant == "rows_swapped_within_tile":
                idx = np.arange(I) ^ 1
                idx[idx >= I] = I - 1
                acc = acc[:, idx]
            n = B * I * D
            if accumulate and self.mutant != "accumulate_overwrites":
                acc = acc + out[:n].reshape(B, I, D)
        out[:n] = acc.reshape(-1)
        return out

    def rowdot(self, gmem, ldg, hmem, ds, B, T, H, D, zero_out, zero_n):
        ds, zero_out = ds.copy(), zero_out.copy()
        zero_out[:zero_n] = 0.0
        ld = D if self.mutant == "ldx_taken_as_D" else ldg
        g = np.stack([_strided_rows(gmem, b * T * ldg, T, ld, D) for b in range(B)])
        h = hmem[:B * H * D].reshape(B, H, D)
        nchunk = D // 16 if self.mutant == "last_chunk_dropped" else (D + 15) // 16
        acc = np.zeros((B, T, H), dtype=np.float32)
        with np.errstate(all="ignore"):
            for c in range(nchunk):
                for e in range(4):
                    for q in range(4):
                        d = 16 * c + 4 * q + e
                        if d < D:
                            acc = _fma(g[:, :, None, d], h[:, None, :, d], acc)
        ds[:B * T * H] = acc.reshape(-1)
        return ds, zero_out
