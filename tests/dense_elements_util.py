"""Shared by the per-element tests of the fp32 dense kernels (csrc/gemm.hip: gemm_nt_kernel behind nrm_gemm_nt, gemm_tn_kernel behind
nrm_gemm_tn, slab_reduce_kernel / slab_reduce_multi_kernel behind nrm_slab_reduce / nrm_slab_reduce_multi): numpy float64 statements
written from the header comments of nrm_hotpath.h and gemm.hip, the bound each element is held to, the cases, a float32 emulation of the
kernels in their own order, and the mutants the CPU test must see rejected.  ``check_nt``, ``check_tn`` and ``check_slab`` run one case
through a backend -- the emulation here (tests/test_dense_elements_cpu.py) or the C entries (tests/test_gpu_dense_elements.py) -- and
return {key: worst |got - ref| / bound}; where a bound is 0 the result must be equal, and a broken bitwise / sentinel rule is inf.

nrm_gemm_nt      y[m,n] = epi(sum_k x[m,k] W[n,k])             x rows ldx apart, W packed by nrm_gemm_pack (or src + sign2 src2 by _pack_multi)
nrm_gemm_tn      ws[s][j][i] = sum_{r in split s} A[r,i] B[r,j]   colsum[s][i] = sum_{r in split s} A[r,i]; split s = rows [s rps, min(R, (s+1) rps))
                                                                (nrm_gemm_tn_plan); the first zero_n floats of zero_out become +0.0
nrm_slab_reduce  out[i os_i + j os_j] += sum_s ws[s][j][i]       out2 += sign2 * the same;  vec_out[i] = sum_s vec[s][i] (stored)

Bounds (U = 2^-24, first order in U).  The fp32 MFMA is a k-ordered chain of fused multiply-adds from the accumulator it is given.
  gemm_nt acc      K U sum_k |x w|       a chain of 16 ceil(K / 16) steps from 0; the steps past K multiply packed zeros by x values the
                                         kernel has set to 0 (`e < kl`): exact.  A weight packed as src + sign2 src2 is one fmaf, one more
                                         rounding on every term: (K + 1) U sum_k |x| |src + sign2 src2|.  One-hot W: every product is exact and
                                         all but one are 0, so the chain bound is 0.
  + bias           U |ref|               v = fl(acc + b), ref = acc64 + b (bias NULL, or NRM_EPI_DGELU: no addition, no term)
  NRM_EPI_MUL      z as above; y = fl(z m) against float64 z_dev m within U |ref| (z_dev: the z the device stored)
  NRM_EPI_GELU     z as above; y against the float64 exact-erf gelu of z_dev within G |z_dev|
  NRM_EPI_DGELU    ref = acc64 gelu'64(z), bound |gelu'64(z)| K U sum |x w| + |acc64| G' + U |ref|     (z is an input here, unchanged after)
G and G' from common.hpp.  gelu2: he = (p t) e with t = rcp(fl(c ax + 1)), e = exp2(fl(fl(x x) c')), p = four fmas; y = fma(ax, fl(0.5 - he),
0.5 x) -- 0.5 x is exact.  A&S 7.1.26 is within 1.5e-7 of erfc, so A = 0.75e-7 of Phi.  Roundings, as absolute errors of he (e <= 1,
h(t) = p t <= 0.5, D1 = max |t h'(t)| on (0, 1], held <= 1.75 by the CPU test):
   t: fma, the folded constant, rcp at 1 ulp = 2 U: 4 U relative -> 4 D1 U = 7 U       Horner: U times the four intermediates (<= .73, .72, .57, .5) = 2.5 U
   the five coefficients rounded to fp32: U sum |a_k| / 2 = 2.24 U                     p t and (p t) e: 0.5 U each
   e: three roundings in its argument x^2 / 2 ln 2 move e by 3 U (x^2 / 2) relative; (x^2 / 2) he <= 0.184 -> 0.55 U; exp2 at 1 ulp: 2 U he <= U
   sum 14.3 U;  y adds fl(0.5 - he) (0.5 U) and the fma (U |y| <= U |x|):   G = A + 16 U = 1.03e-6, times |z|
gelu_grad4_times: cdf = fl(0.5 + copysign(fl(0.5 - he), x)) adds 0.5 U + U to he's A + 14.3 U; x phi(x) = fma(fl(x c''), e, cdf): two roundings on x c''
and e's (2 + 1.5 x^2) U relative on |x| phi <= 0.242 (|x|^3 phi <= 0.463): 1.66 U; the fma U |d| <= 1.13 U:   G' = A + 19 U = 1.21e-6, absolute on
gelu'; the product with acc is the U |ref| above.  The CPU test holds the fp32 transcription with exact reciprocal and exp2 to HALF of both.
  gemm_tn slab s   nrows_s U sum_{r in s} |a b|;  colsum (ceil(nrows_s / 4) + 2) U sum |a|: lane group q sums rows q, q + 4, ...; two sum_rows4 additions
  slab_reduce      a block sums its spc slabs in order from 0 (spc - 1 roundings), then one float atomic per split chunk lands on out in any order.
                   CORRECTED against the issue's U (|prior| + |ref|): each of the nchunk atomics rounds a partial sum that contains the prior, so
                   bound = (spc - 1 + nchunk) U sum_s |ws| + nchunk U |prior|   (spc, nchunk: slab_plan, mirrored here).  out2: the same (sign2 = -1
                   is exact).  vec_out: nsplit U sum_s |vec|.

Padding and sentinels.  The x padding [K, ldx) and the A / B padding hold NaN; so do the floats behind every input.  y and z are SENTINEL
everywhere before the call, two rows >= M and four floats behind them included: rows >= M and columns >= min(ld, 16 ceil(N / 16)) keep their
bits, columns [N, that) are zero afterwards: +0.0 in z and in y of NRM_EPI_BIAS / _GELU; in y of NRM_EPI_MUL / _DGELU the kernel stores
fl(0 m) / fl(gelu'(z) 0) of the (finite, non-zero) m / z padding, a zero with the sign of that factor (a FINDING of these tests: the header said
`zeros` and now says which).  The m padding is +-1.5, the saved-z padding +0.5 / -2.0 (gelu' = 0.87 / -0.085): the sign is checked bitwise.

Families.  normal: N(0, 1), W / sqrt(K).  scaled: row m of x by 2^e(m), row n of W by 2^f(n), e, f in -20 .. 20 (gemm_tn: the columns of A and
B; slabs: slab s and column i).  onehot: W has a single 1.0 per row n at k(n): NRM_EPI_BIAS gives fl(x[m,k(n)] + b[n]) BITWISE; gemm_tn:
column i of A has a single 1.0 per split at r_s(i), ws[s][j][i] = B[r_s(i), j] BITWISE.  tails (GELU, DGELU): z reaches +-12.

Mutants (each a one-line change of a kernel, applied in the emulation) and where they can show:
  gemm_nt  last_kchunk_dropped      kchunks = K / 16                        K % 16 != 0 (dense families)
           ragged_mask_off_by_one   e <= kl: x[m, K] enters                 K % 16 != 0 and ldx > K (the NaN of the padding; at ldx = K it is the next
           ragged_mask_absent       no select at all                        row's head times a packed zero, exact)
           last_col_tile_skipped    it < ntv - 1                            the last N-chunk has fewer valid tiles than NT
           ldx_taken_as_K           rows K apart                            ldx > K, M > 1
           rows_swapped             rows r, r ^ 1 of a tile                 M > 1 (dense)
           bias_one_tile_late       b[n + 16]                               bias given, not NRM_EPI_DGELU
           z_stored_after_gelu      the hazard of store_b128_guarded        NRM_EPI_GELU
           m_from_row_0             m of the block's first row              NRM_EPI_MUL, M > 1
           tanh_gelu                tanh form for erf                       NRM_EPI_GELU (dense: |z| ~ 1)
           dgelu_without_xphi       gelu' = Phi                             NRM_EPI_DGELU
           y_padding_not_zeroed     columns >= N of y not stored            N % 16 != 0 (a column of [N, ldy) inside the last tile)
  gemm_tn  last_partial_step_dropped  nsteps = nrows >> 2                   a split with nrows % 4 != 0 (dense)
           splits_overlap           r_hi one row further                    nsplit > 1 (dense)
           kt8_halves_exchanged     tn_col<8>: t < 4 and t >= 4 swapped     KT = 8 or DT = 8
           colsum_by_tj1            tj == 1 writes colsum                   colsum given and one j tile (with more, tile 1 holds the same sums)
           zero_tail_dropped        the scalar loop of zero_out             zero_n % 4 != 0
  slab     last_slab_dropped        s < s_hi - 1                            always
           store_not_add            out = v                                 non-zero prior, or nchunk > 1
           sign2_ignored            out2 += v                               out2 given
           vec_stops_at_256         the vector leg's first block only       vec given, ni > 256
           out2_with_out_strides    out2 + i os_i + j os_j                  out2 given (its strides differ from out's in every case here)
"""
import functools
import math
import os

import numpy as np

U = 2.0 ** -24
SENTINEL = np.float32(-12345.678)
TAIL = 4
INF = float("inf")
A_S = 0.75e-7                                           # A&S 7.1.26 on Phi
G_GELU = A_S + 16 * U
G_GRAD = A_S + 19 * U
D1_MAX = 1.75

EPI = {"bias": 0, "gelu": 1, "dgelu": 2, "mul": 3}
EPILOGUES = ("bias", "gelu", "dgelu", "mul")
NT_FAMILIES = {"bias": ("normal", "scaled", "onehot"), "gelu": ("normal", "scaled", "onehot", "tails"),
               "dgelu": ("normal", "scaled", "onehot", "tails"), "mul": ("normal", "scaled", "onehot")}
NT_WIDTHS = {4: (3, 1, 64), 5: (66, 80), 8: (128,), 9: (258,), 13: (402, 400, 1608)}      # the first of each carries the full M and K lists
NT_M = (1, 15, 16, 17, 63, 64, 65, 130)
NT_K = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 42, 130)
NT_PLANNED = {4: (4, 2), 5: (4, 2), 8: (3, 2), 9: (2, 3), 13: (1, 4)}                     # NT -> (MT, WPE) of the planned form
MT_WIDTHS = {4: (3, 64), 5: (66,), 8: (128,), 9: (258,)}                                  # the worker's widths (NRM_NT_SMALLM=0)
MT_K = 42
NT_MUTANTS = ("last_kchunk_dropped", "ragged_mask_off_by_one", "ragged_mask_absent", "last_col_tile_skipped", "ldx_taken_as_K", "rows_swapped",
              "bias_one_tile_late", "z_stored_after_gelu", "m_from_row_0", "tanh_gelu", "dgelu_without_xphi", "y_padding_not_zeroed")

TN_PAIRS = ((30, 125), (125, 30), (78, 30), (30, 78), (400, 400), (64, 64))               # test_gemm_tn_wave_tile_shapes: 2x8 8x2 5x2 2x5 5x5 4x4
TN_EXTRA = ((1, 2), (2, 17), (17, 1), (6, 30))
TN_R = (1, 3, 4, 5, 127, 128, 129, 515, 1001)
TN_WAVES = (None, "1")                                  # NRM_TN_WAVES: as planned (one round of wave slots), four splits at most
TN_FAMILIES = ("normal", "scaled", "onehot")
TN_MUTANTS = ("last_partial_step_dropped", "splits_overlap", "kt8_halves_exchanged", "colsum_by_tj1", "zero_tail_dropped")
ZERO_N = (0, 3, 300)
ZERO_LEN = 304

SLAB_SETS = ((5, 64, 64), (37, 130, 33), (1, 7, 5), (2, 127, 31), (4, 128, 32), (5, 129, 33), (37, 255, 31), (4, 257, 32), (2, 256, 1), (160, 64, 64), (20, 402, 70))
SLAB_MAX = 24
SLAB_MUTANTS = ("last_slab_dropped", "store_not_add", "sign2_ignored", "vec_stops_at_256", "out2_with_out_strides")


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pad4(n):
    return (n + 3) // 4 * 4


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


def _nan_tail(a):
    return np.concatenate([f32(a).reshape(-1), np.full(TAIL, np.nan, dtype=np.float32)])


def _rows_buffer(vals, ld, fill=np.nan):
    """[n, D] values -> flat float32 of n ld + TAIL floats, `fill` in the columns [D, ld), NaN behind the last row"""
    n, D = vals.shape
    m = np.full((n, ld), fill, dtype=np.float32)
    m[:, :D] = vals
    return _nan_tail(m)


# ------------------------------------------------------------------------------------------------ the float64 GELU and its fp32 transcription
_erfc = np.frompyfunc(math.erfc, 1, 1)


def phi_cdf64(z):
    return 0.5 * _erfc(-f64(z) / math.sqrt(2.0)).astype(np.float64)


def gelu64(z):
    return f64(z) * phi_cdf64(z)


def gelu_grad64(z):
    z = f64(z)
    return phi_cdf64(z) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in float64"""
    with np.errstate(all="ignore"):
        return f32(f64(a) * f64(b) + f64(c))


_C1 = np.float32(0.3275911) * np.float32(0.70710678118654752440)
_CE = np.float32(-0.5) * np.float32(1.44269504088896340736)
_C3 = np.float32(0.39894228040143267794)
_A = [np.float32(0.5) * np.float32(a) for a in (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)]
_HALF = np.float32(0.5)


def _he32(x):
    """gelu_half_erfc2 of common.hpp with an exact reciprocal and exp2: (0.5 erfc(|x| / sqrt 2), exp(-x^2 / 2))"""
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        t = f32(1.0 / f64(_fma(_C1, ax, np.float32(1.0))))
        e = f32(np.exp2(f64(f32(f32(x * x) * _CE))))
        p = _fma(_A[0], t, _A[1])
        for a in _A[2:]:
            p = _fma(p, t, a)
        return f32(f32(p * t) * e), e


def gelu32(x):
    x = f32(x)
    he, _ = _he32(x)
    return _fma(np.abs(x), f32(_HALF - he), f32(x * _HALF))


def gelu_grad32_times(x, g, without_xphi=False):
    x, g = f32(x), f32(g)
    he, e = _he32(x)
    with np.errstate(all="ignore"):
        cdf = f32(_HALF + np.copysign(f32(_HALF - he), x))
        d = cdf if without_xphi else _fma(f32(x * _C3), e, cdf)
        return f32(d * g)


def gelu_tanh32(x):
    x = f64(x)
    with np.errstate(all="ignore"):
        return f32(0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))))


def gelu_grid():
    """2^16 + 1 points of [-14, 14], +-0 and |z| < 2^-20"""
    tiny = [0.0, 2.0 ** -21, 2.0 ** -30, 2.0 ** -60, 1e-30, 2.0 ** -126]
    return f32(np.concatenate([np.linspace(-14.0, 14.0, 2 ** 16 + 1), tiny, [-t for t in tiny]]))


def gelu_grid_ratios():
    """(worst |gelu32 - gelu64| / (G |z|), worst |gelu'32 - gelu'64| / G') of the transcription with exact reciprocal and exp2"""
    z = gelu_grid()
    ones = np.ones_like(z)
    return (ratio(gelu32(z), gelu64(z), G_GELU * np.abs(f64(z))), ratio(gelu_grad32_times(z, ones), gelu_grad64(z), G_GRAD * f64(ones)))


def horner_d1():
    """max |t h'(t)| on (0, 1], h(t) = p(t) t the A&S polynomial with the halved coefficients"""
    t = np.linspace(0.0, 1.0, 100001)
    a = [float(c) for c in _A[::-1]]                        # a1 .. a5 (halved)
    return float(np.abs(sum((k + 1) * a[k] * t ** (k + 1) for k in range(5))).max())


# ------------------------------------------------------------------------------------------------ nrm_gemm_nt
def nt_plan(N, narrow=True):
    """gemm_nt_plan of gemm.hip: (NT, planned MT, nchunks)"""
    n16 = (N + 15) // 16
    if n16 <= 4:
        NT = 4
    else:
        p13, p8 = (n16 + 12) // 13 * 13, (n16 + 7) // 8 * 8
        NT, best = (13, p13) if p13 <= p8 else (8, p8)
        p9, p5 = (n16 + 8) // 9 * 9, (n16 + 4) // 5 * 5
        if narrow and p9 * 10 <= best * 9:
            NT, best = 9, p9
        if narrow and p5 * 10 <= best * 9:
            NT, best = 5, p5
    return NT, NT_PLANNED[NT][0], (n16 + NT - 1) // NT


def nt_form(M, N, small_m=True):
    """gemm_nt_select of gemm.hip (default NRM_NT_NARROW): (NT, MT, WPE, KC)"""
    NT, MT, nchunks = nt_plan(N)
    if small_m and MT > 1 and (M + 64 * MT - 1) // (64 * MT) * nchunks < 512:
        return (NT, 1, 4, 1)
    return (NT,) + NT_PLANNED[NT] + (1,)


def lib_nt_form(lib, M, N, K):
    v = lib.nrm_gemm_nt_form(M, N, K, 0)
    assert v > 0, (M, N, K, v)
    return (v & 255, (v >> 8) & 255, (v >> 16) & 255, (v >> 24) & 255)


def nt_shapes(NT):
    """(M, K, N) of the in-process cases of one NT: the first width with every M at K = 42 and every K at M = 65, the others M = 65, K in (17, 42)"""
    full = NT_WIDTHS[NT][0]
    out = [(M, 42, full) for M in NT_M] + [(65, K, full) for K in NT_K if K != 42]
    for N in NT_WIDTHS[NT][1:]:
        out += [(65, 17, N), (65, 42, N)]
    return out


def mt_shapes(NT):
    """the worker's cases: M around one and two workgroups of 64 MT rows"""
    MT = NT_PLANNED[NT][0]
    return [(M, MT_K, N) for N in MT_WIDTHS[NT] for M in (1, 64 * MT - 1, 64 * MT, 64 * MT + 1, 2 * 64 * MT + 17)]


VARIANTS = ((0, 0, True, False), (4, 4, False, False), (0, 4, False, True), (4, 0, True, False))      # (ldx - pad4 K, ldy - pad4 N, bias, src2 pack)


def nt_launches(shapes, families=None):
    """(M, K, N, epilogue, family, variant) of every launch over `shapes`: the variants go round, so every shape meets each of them"""
    out, n = [], 0
    for M, K, N in shapes:
        for epi in EPILOGUES:
            for family in NT_FAMILIES[epi]:
                if families is not None and family not in families:
                    continue
                out.append((M, K, N, epi, family, VARIANTS[n % 4]))
                n += 1
    return out


def make_nt(M, K, N, family, seed=0):
    """the operands of one (shape, family), shared by its epilogues and variants and never changed"""
    rng = np.random.default_rng([M, K, N, ("normal", "scaled", "onehot", "tails").index(family), seed])
    x = rng.standard_normal((M, K))
    hot = None
    if family == "onehot":
        hot = rng.integers(0, K, N)
        hot[::3] = K - 1                                 # every third output column selects the last column of x
        W = np.zeros((N, K))
        W[np.arange(N), hot] = 1.0
    else:
        W = rng.standard_normal((N, K)) / math.sqrt(K)
    if family == "scaled":
        x = x * 2.0 ** rng.integers(-20, 21, M)[:, None]
        W = W * 2.0 ** rng.integers(-20, 21, N)[:, None]
    if family == "tails":
        x = x * 4.0
    W2 = f32(rng.standard_normal((N, K)) / math.sqrt(K)) if family != "onehot" else np.zeros((N, K), dtype=np.float32)
    if family == "scaled":
        W2 = f32(f64(W2) * 2.0 ** rng.integers(-20, 21, N)[:, None])
    x, W = f32(x), f32(W)
    b = f32(rng.standard_normal(N) * (0.1 if family != "scaled" else 1.0))
    m = f32(rng.standard_normal((M, N)))
    zs = f32(rng.uniform(-12.0, 12.0, (M, N)) if family == "tails" else rng.standard_normal((M, N)))
    c = dict(M=M, K=K, N=N, family=family, x=x, W=W, W2=W2, b=b, m=m, zs=zs, hot=hot)
    for name, w in (("", f64(W)), ("2", f64(W) - f64(W2))):                 # the plain pack; src + sign2 src2 with sign2 = -1
        c["acc" + name] = f64(x) @ w.T
        c["mag" + name] = np.abs(f64(x)) @ np.abs(w).T
    return c


@functools.lru_cache(maxsize=None)
def nt_case(M, K, N, family):
    """made once, shared by the epilogues and variants (the backends copy what they write)"""
    return make_nt(M, K, N, family)


def _pad_vals(rows, n, a, b):
    """finite non-zero padding: a / b alternating by column and row"""
    p = np.where((np.arange(rows)[:, None] + np.arange(n)[None, :]) % 2 == 0, a, b)
    return f32(p)


def check_nt(be, c, epilogue, variant=VARIANTS[0], form=None):
    """one launch of nrm_gemm_nt; form: the (NT, MT, WPE, KC) the launch takes (default: as dispatched in a fresh process)"""
    M, K, N, family = c["M"], c["K"], c["N"], c["family"]
    dx, dy, with_bias, src2 = variant
    form = form or nt_form(M, N)
    ldx, ldy, ldz, ldm = pad4(K) + dx, pad4(N) + dy, pad4(N) + 4 - dy, pad4(N) + dx
    xmem = _rows_buffer(c["x"], ldx)
    ny = (M + 2) * ldy
    ymem = np.full(ny + TAIL, SENTINEL, dtype=np.float32)
    bias = _nan_tail(c["b"]) if with_bias and epilogue != "dgelu" else None
    zmem = mmem = None
    if epilogue != "bias":
        zmem = np.full((M + 2) * ldz + TAIL, SENTINEL, dtype=np.float32)
    if epilogue == "dgelu":
        zin = np.concatenate([c["zs"], _pad_vals(M, ldz - N, 0.5, -2.0)], axis=1)
        zmem[:M * ldz] = zin.reshape(-1)
    if epilogue == "mul":
        mmem = _nan_tail(np.concatenate([c["m"], _pad_vals(M, ldm - N, 1.5, -1.5)], axis=1))
    w2 = c["W2"] if src2 else None
    z_before = None if zmem is None else zmem.copy()
    ygot, zgot = be.gemm_nt(xmem, ldx, M, c["W"], w2, -1.0, N, K, bias, ymem, ldy, zmem, ldz, mmem, ldm, EPI[epilogue], form)

    onehot = family == "onehot" and not src2
    acc, mag = (c["acc2"], c["mag2"]) if src2 else (c["acc"], c["mag"])
    chain = np.zeros_like(mag) if onehot else (K + (1 if src2 else 0)) * U * mag
    zref, zbound = acc, chain
    if bias is not None:
        zref = acc + f64(c["b"])[None, :]
        zbound = chain + U * np.abs(zref)
    Y = ygot[:ny].reshape(M + 2, ldy)
    res, key = {}, "nt.%dx%d.%s" % (form[0], form[1], epilogue)
    pad16 = (N + 15) // 16 * 16

    def frame(buf, ld, pad_want):
        """rows >= M, the floats behind, the columns the kernel does not own keep their bits; the columns [N, min(ld, pad16)) are `pad_want`"""
        B = buf[:(M + 2) * ld].reshape(M + 2, ld)
        hi = min(ld, pad16)
        ok = (bits(B[M:]) == bits(SENTINEL)).all() and (bits(buf[(M + 2) * ld:]) == bits(SENTINEL)).all() and (bits(B[:M, hi:]) == bits(SENTINEL)).all()
        return 0.0 if ok and np.array_equal(bits(B[:M, N:hi]), bits(pad_want[:, :hi - N])) else INF

    zero_pad = np.zeros((M, 16), dtype=np.float32)
    if epilogue == "bias":
        worst = max(ratio(Y[:M, :N], zref, zbound), frame(ygot, ldy, zero_pad))
        if onehot:
            x_sel = c["x"][:, c["hot"]]
            res["nt.onehot"] = same_bits(Y[:M, :N], x_sel + c["b"][None, :] if bias is not None else x_sel)
    elif epilogue == "dgelu":
        zs = f64(c["zs"])
        gp = gelu_grad64(zs)
        ref = acc * gp
        bound = np.abs(gp) * chain + np.abs(acc) * G_GRAD + U * np.abs(ref)
        pad_want = np.copysign(np.float32(0.0), _pad_vals(M, max(ldz - N, 16), 1.0, -1.0))[:, :16]         # the sign of gelu'(+0.5), gelu'(-2)
        pad_want = np.where(np.arange(16)[None, :] < ldz - N, pad_want, np.float32(0.0))                    # (columns past ldz read as z = 0: gelu' = +0.5)
        worst = max(ratio(Y[:M, :N], ref, bound), frame(ygot, ldy, f32(pad_want)), same_bits(zgot, z_before))
        if onehot:                                       # acc is x[m, k(n)] exactly: what is left is gelu' alone
            res["gelu_grad"] = ratio(Y[:M, :N], ref, np.abs(acc) * G_GRAD + U * np.abs(ref))
    else:
        Z = zgot[:(M + 2) * ldz].reshape(M + 2, ldz)
        zdev = f64(Z[:M, :N])
        worst = max(ratio(Z[:M, :N], zref, zbound), frame(zgot, ldz, zero_pad))
        if not np.isfinite(zdev).all():
            worst = INF
        elif epilogue == "gelu":
            g = ratio(Y[:M, :N], gelu64(zdev), G_GELU * np.abs(zdev))
            res["gelu"] = g
            worst = max(worst, g, frame(ygot, ldy, zero_pad))
        else:
            ref = zdev * f64(c["m"])
            pad_want = np.copysign(np.float32(0.0), _pad_vals(M, max(ldm - N, 16), 1.0, -1.0))[:, :16]
            pad_want = np.where(np.arange(16)[None, :] < ldm - N, pad_want, np.float32(0.0))                # (columns past ldm read as m = +0)
            worst = max(worst, ratio(Y[:M, :N], ref, U * np.abs(ref)), frame(ygot, ldy, f32(pad_want)))
    res[key] = worst
    return res


def nt_applies(mutant, c, epilogue, variant, form):
    M, K, N, family = c["M"], c["K"], c["N"], c["family"]
    dx, dy, with_bias, src2 = variant
    dense = family != "onehot"
    NT = form[0]
    last = N - (N - 1) // (16 * NT) * 16 * NT             # columns of the last N-chunk
    return {"last_kchunk_dropped": dense and K % 16 != 0,
            "ragged_mask_off_by_one": K % 16 != 0 and pad4(K) + dx > K,
            "ragged_mask_absent": K % 16 != 0 and pad4(K) + dx > K,
            "last_col_tile_skipped": dense and (last + 15) // 16 < NT,
            "ldx_taken_as_K": dense and pad4(K) + dx > K and M > 1,
            "rows_swapped": dense and M > 1,
            "bias_one_tile_late": with_bias and epilogue != "dgelu" and family != "scaled",
            "z_stored_after_gelu": epilogue == "gelu" and family in ("normal", "tails"),
            "m_from_row_0": epilogue == "mul" and M > 1,
            "tanh_gelu": epilogue == "gelu" and family in ("normal", "tails"),
            "dgelu_without_xphi": epilogue == "dgelu" and family in ("normal", "tails", "onehot"),
            "y_padding_not_zeroed": min(pad4(N) + dy, (N + 15) // 16 * 16) > N}[mutant]


# ------------------------------------------------------------------------------------------------ nrm_gemm_tn
TN_SHAPES = ((4, 4), (5, 5), (2, 8), (8, 2), (5, 2), (2, 5))


def tn_plan(ni, nj, R, waves=None):
    """gemm_tn_plan of gemm.hip for fp32 (default NRM_TN_SHAPES): (nsplit, KT, DT, rows per split); waves: NRM_TN_WAVES"""
    ni16, nj16 = (ni + 15) // 16, (nj + 15) // 16
    best = None
    for kt, dt in TN_SHAPES:
        w = (ni16 + kt - 1) // kt * kt * ((nj16 + dt - 1) // dt * dt)
        if best is None or w < best:
            best, KT, DT = w, kt, dt
    tiles = (ni16 + KT - 1) // KT * ((nj16 + DT - 1) // DT)
    target = int(waves) if waves else 0
    if target <= 0:
        target = 1024 * (4 if KT * DT <= 16 else 3)
    ns = max(target // tiles // 4 * 4, 4)
    max_ns = (R + 127) // 128
    if ns > max_ns:
        ns = max(max_ns, 1)
    rps = max(((R + ns - 1) // ns + 3) // 4 * 4, 4)
    return max((R + rps - 1) // rps, 1), KT, DT, rps


def lib_tn_plan(lib, ni, nj, R):
    import ctypes
    kt, dt, rps = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    ns = lib.nrm_gemm_tn_plan(ni, nj, R, 0, ctypes.byref(kt), ctypes.byref(dt), ctypes.byref(rps))
    return ns, kt.value, dt.value, rps.value


def tn_shapes():
    """(ni, nj, R): every R on the two-by-eight, four-by-four and the narrow pairs, three R on the others (400 x 400: two short ones)"""
    out = []
    for ni, nj in TN_PAIRS + TN_EXTRA:
        full = (ni, nj) in ((30, 125), (64, 64), (6, 30), (2, 17))
        rs = TN_R if full else ((5, 129) if ni == 400 else (5, 129, 515))
        out += [(ni, nj, R) for R in rs]
    return out


def tn_launches():
    """(ni, nj, R, waves, family, lda - ni, colsum, zero_n) of every launch: the paddings, colsum and zero_out go round"""
    out, n = [], 0
    for ni, nj, R in tn_shapes():
        for waves in TN_WAVES:
            if waves is not None and tn_plan(ni, nj, R, waves) == tn_plan(ni, nj, R):
                continue
            for family in TN_FAMILIES:
                out.append((ni, nj, R, waves, family, (0, 3)[n % 2], n % 4 < 2, ((None,) + ZERO_N)[(n // 3) % 4]))
                n += 1
    return out


def make_tn(ni, nj, R, waves, family, dpad, seed=0):
    plan = tn_plan(ni, nj, R, waves)
    nsplit, KT, DT, rps = plan
    rng = np.random.default_rng([ni, nj, R, int(waves or 0), TN_FAMILIES.index(family), dpad, seed])
    B = rng.standard_normal((R, nj))
    hot = None
    if family == "onehot":
        A = np.zeros((R, ni))
        hot = np.zeros((nsplit, ni), dtype=np.int64)
        for s in range(nsplit):
            lo, hi = s * rps, min(R, (s + 1) * rps)
            hot[s] = rng.integers(lo, hi, ni)
            hot[s, ::3] = hi - 1                           # every third column selects the split's last row
            A[hot[s], np.arange(ni)] = 1.0
    else:
        A = rng.standard_normal((R, ni))
    if family == "scaled":
        A = A * 2.0 ** rng.integers(-20, 21, ni)[None, :]
        B = B * 2.0 ** rng.integers(-20, 21, nj)[None, :]
    A, B = f32(A), f32(B)
    lda, ldb = ni + dpad, nj + dpad
    return dict(ni=ni, nj=nj, R=R, waves=waves, family=family, plan=plan, A=A, B=B, lda=lda, ldb=ldb, amem=_rows_buffer(A, lda), bmem=_rows_buffer(B, ldb),
                hot=hot)


@functools.lru_cache(maxsize=None)
def tn_case(ni, nj, R, waves, family, dpad):
    return make_tn(ni, nj, R, waves, family, dpad)


def check_tn(be, c, colsum, zero_n, dws=0):
    """one launch of nrm_gemm_tn under NRM_TN_WAVES = c['waves']; zero_n None: no zero_out"""
    ni, nj, R = c["ni"], c["nj"], c["R"]
    nsplit, KT, DT, rps = c["plan"]
    assert be.tn_plan(ni, nj, R, c["waves"]) == c["plan"], "the plan of the launch is not the plan of the case"
    ldws = pad4(ni) + dws
    nws = nsplit * nj * ldws
    ws = np.full(nws + TAIL, SENTINEL, dtype=np.float32)
    cs = np.full(nsplit * ldws + TAIL, SENTINEL, dtype=np.float32) if colsum else None
    zo = np.full(ZERO_LEN, np.nan, dtype=np.float32) if zero_n is not None else None
    wgot, cgot, zgot = be.gemm_tn(c["amem"], c["lda"], ni, c["bmem"], c["ldb"], nj, R, ws, ldws, cs, zo, zero_n or 0, c["waves"], c["plan"])
    Wg = wgot[:nws].reshape(nsplit, nj, ldws)
    worst = 0.0 if (bits(wgot[nws:]) == bits(SENTINEL)).all() else INF
    cworst = 0.0
    A, B = f64(c["A"]), f64(c["B"])
    for s in range(nsplit):
        lo, hi = s * rps, min(R, (s + 1) * rps)
        ref = A[lo:hi].T @ B[lo:hi]
        mag = np.abs(A[lo:hi]).T @ np.abs(B[lo:hi])
        bound = np.zeros_like(mag) if c["family"] == "onehot" else (hi - lo) * U * mag
        got = Wg[s, :, :ni].T
        worst = max(worst, ratio(got, ref, bound))
        if c["family"] == "onehot":
            worst = max(worst, same_bits(got, c["B"][c["hot"][s]]))
        if colsum:
            cref, cmag = A[lo:hi].sum(0), np.abs(A[lo:hi]).sum(0)
            cworst = max(cworst, ratio(cgot[s * ldws:s * ldws + ni], cref, ((hi - lo + 3) // 4 + 2) * U * cmag))
    if zo is not None:
        zb = bits(zgot)
        if zb[:zero_n].any() or not np.array_equal(zb[zero_n:], bits(zo)[zero_n:]):
            worst = INF
    res = {"tn.%dx%d" % (KT, DT): worst}
    if colsum:
        res["tn.colsum"] = max(cworst, 0.0 if (bits(cgot[nsplit * ldws:]) == bits(SENTINEL)).all() else INF)
    return res


def tn_applies(mutant, c, colsum, zero_n):
    nsplit, KT, DT, rps = c["plan"]
    dense = c["family"] != "onehot"
    rows = [min(c["R"], (s + 1) * rps) - s * rps for s in range(nsplit)]
    return {"last_partial_step_dropped": dense and any(r % 4 for r in rows), "splits_overlap": dense and nsplit > 1,
            "kt8_halves_exchanged": 8 in (KT, DT) and dense, "colsum_by_tj1": bool(colsum) and (c["nj"] + 15) // 16 <= DT,
            "zero_tail_dropped": zero_n is not None and zero_n % 4 != 0}[mutant]


# ------------------------------------------------------------------------------------------------ nrm_slab_reduce / _multi
def slab_plan(nsplit, ni, nj, vec):
    """slab_plan of gemm.hip: (gx, nchunk, spc)"""
    tiles = (ni + 127) // 128 * ((nj + 31) // 32)
    gx = max(tiles, (ni + 255) // 256) if vec else tiles
    nchunk = max(min(512 // tiles, 128, (nsplit + 3) // 4), 1)
    spc = (nsplit + nchunk - 1) // nchunk
    return gx, (nsplit + spc - 1) // spc, spc


def make_slab(nsplit, ni, nj, n, seed=0):
    """set n of a case: out is the column block [off, off + nj) of a [ni, wide] matrix (SENTINEL outside the block, prior inside: zero for
    even n), out2 (every other set) a transposed [nj, ni + 3] matrix of its own, vec for n % 4 < 2 (and for even n where ni > 256: the vector leg's second block), ldws = pad4(ni) (+ 4 for odd n): NaN in [ni, ldws)"""
    rng = np.random.default_rng([nsplit, ni, nj, n, seed])
    ldws = pad4(ni) + 4 * (n % 2)
    scaled = n % 3 == 1
    w = rng.standard_normal((nsplit, nj, ni))
    v = rng.standard_normal((nsplit, ni))
    if scaled:
        w = w * 2.0 ** rng.integers(-20, 21, nsplit)[:, None, None] * 2.0 ** rng.integers(-20, 21, ni)[None, None, :]
        v = v * 2.0 ** rng.integers(-20, 21, nsplit)[:, None]
    w, v = f32(w), f32(v)
    ws = np.full((nsplit, nj, ldws), np.nan, dtype=np.float32)
    ws[:, :, :ni] = w
    vec = None
    if n % 4 < 2 or (ni > 256 and n % 2 == 0):
        vec = np.full((nsplit, ldws), np.nan, dtype=np.float32)
        vec[:, :ni] = v
    off, wide = 4, nj + 9
    prior = f32(rng.standard_normal((ni, nj)) * (np.abs(f64(w)).sum(0).T if scaled else math.sqrt(nsplit))) if n % 2 else np.zeros((ni, nj), dtype=np.float32)
    out = np.full((ni, wide), SENTINEL, dtype=np.float32)
    out[:, off:off + nj] = prior
    second = n % 2 == (n // 2) % 2
    out2 = prior2 = None
    if second:
        prior2 = f32(rng.standard_normal((nj, ni)))
        out2 = np.full((nj, ni + 3), SENTINEL, dtype=np.float32)
        out2[:, :ni] = prior2
    return dict(nsplit=nsplit, ni=ni, nj=nj, ldws=ldws, w=w, v=v, wsmem=_nan_tail(ws), vecmem=None if vec is None else _nan_tail(vec),
                outmem=np.concatenate([out.reshape(-1), np.full(TAIL, SENTINEL, dtype=np.float32)]), off=off, wide=wide, prior=prior,
                out2mem=None if out2 is None else np.concatenate([out2.reshape(-1), np.full(TAIL, SENTINEL, dtype=np.float32)]), prior2=prior2,
                plan=slab_plan(nsplit, ni, nj, vec is not None))


def slab_cases():
    """The small sets of test_slab_reduce_multi_matches_single_launches_and_numpy, its many-split and its wide set at a tenth of their
    size (160 x 64 x 64, 20 x 402 x 70), nsplit in (1, 2, 4, 5, 37) at ni around 128 and 256, nj around 32.
    single launches: every set twice (n and n + 1: prior zero / non-zero, out2 and vec go round); multi: all of them, twice over, in one call"""
    sets = [make_slab(ns, ni, nj, n) for n, (ns, ni, nj) in enumerate(SLAB_SETS + SLAB_SETS[::-1])]
    extra = [make_slab(ns, ni, nj, n + 2) for n, (ns, ni, nj) in enumerate(SLAB_SETS)]
    cases = [dict(sets=[s], multi=False) for s in sets] + [dict(sets=[s], multi=True) for s in extra[:3]]
    cases.append(dict(sets=sets + extra, multi=True))
    assert len(cases[-1]["sets"]) > SLAB_MAX
    return cases


def check_slab(be, case):
    got = be.slab_reduce([dict(s) for s in case["sets"]], case["multi"])
    worst = vworst = 0.0
    for s, (ogot, o2got, vgot) in zip(case["sets"], got):
        nsplit, ni, nj, off, wide = s["nsplit"], s["ni"], s["nj"], s["off"], s["wide"]
        gx, nchunk, spc = s["plan"]
        tot, mag = f64(s["w"]).sum(0).T, np.abs(f64(s["w"])).sum(0).T                    # [ni, nj]
        O, O0 = ogot[:ni * wide].reshape(ni, wide), s["outmem"][:ni * wide].reshape(ni, wide)
        keep = np.ones((ni, wide), dtype=bool)
        keep[:, off:off + nj] = False
        ok = np.array_equal(bits(O[keep]), bits(O0[keep])) and (bits(ogot[ni * wide:]) == bits(SENTINEL)).all()
        pr = f64(s["prior"])
        worst = max(worst, 0.0 if ok else INF, ratio(O[:, off:off + nj], pr + tot, (spc - 1 + nchunk) * U * mag + nchunk * U * np.abs(pr)))
        if s["out2mem"] is not None:
            P, P0 = o2got[:nj * (ni + 3)].reshape(nj, ni + 3), s["out2mem"][:nj * (ni + 3)].reshape(nj, ni + 3)
            ok = np.array_equal(bits(P[:, ni:]), bits(P0[:, ni:])) and (bits(o2got[nj * (ni + 3):]) == bits(SENTINEL)).all()
            p2 = f64(s["prior2"])
            worst = max(worst, 0.0 if ok else INF, ratio(P[:, :ni], p2 - tot.T, (spc - 1 + nchunk) * U * mag.T + nchunk * U * np.abs(p2)))
        if s["vecmem"] is not None:
            vworst = max(vworst, ratio(vgot[:ni], f64(s["v"]).sum(0), nsplit * U * np.abs(f64(s["v"])).sum(0)),
                         0.0 if (bits(vgot[ni:]) == bits(SENTINEL)).all() else INF)
    res = {"slab": worst}
    if any(s["vecmem"] is not None for s in case["sets"]):
        res["slab.vec"] = vworst
    return res


def slab_applies(mutant, case):
    ss = case["sets"]
    return {"last_slab_dropped": True, "store_not_add": any(s["prior"].any() or s["plan"][1] > 1 for s in ss),
            "sign2_ignored": any(s["out2mem"] is not None for s in ss), "out2_with_out_strides": any(s["out2mem"] is not None for s in ss),
            "vec_stops_at_256": any(s["vecmem"] is not None and s["ni"] > 256 for s in ss)}[mutant]


# ------------------------------------------------------------------------------------------------ the float32 emulation
def _gather(mem, idx, limit):
    """mem[idx] where idx < limit (a buffer descriptor's extent), else 0"""
    ok = idx < limit
    return np.where(ok, mem[np.where(ok, idx, 0)], np.float32(0.0))


class Emulated:
    """The kernels in float32, in their own order, from the memory they are given; ``mutant``: one of NT_ / TN_ / SLAB_MUTANTS"""

    def __init__(self, mutant=None):
        self.mutant = mutant

    def tn_plan(self, ni, nj, R, waves):
        assert os.environ.get("NRM_TN_WAVES") == waves
        return tn_plan(ni, nj, R, waves)

    def gemm_nt(self, xmem, ldx, M, w, w2, sign2, N, K, bias, ymem, ldy, zmem, ldz, mmem, ldm, epi, form):
        mu = self.mutant
        NT, MT = form[0], form[1]
        BM = 64 * MT
        W = f32(w) if w2 is None else _fma(np.float32(sign2), w2, w)
        kch = K // 16 if mu == "last_kchunk_dropped" else (K + 15) // 16
        Kp, Np = 16 * kch, (N + 15) // 16 * 16
        ld = K if mu == "ldx_taken_as_K" else ldx
        rl = np.arange(M) % BM
        rows_here = np.minimum(BM, M - (np.arange(M) - rl))
        k = np.arange(Kp)
        local = rl[:, None] * ld + k[None, :]
        X = _gather(xmem, (np.arange(M) - rl)[:, None] * ld + local, np.int64(len(xmem)))
        X = np.where(local < (rows_here * ld)[:, None], X, np.float32(0.0))
        if K % 16:
            cut = K + 1 if mu == "ragged_mask_off_by_one" else (Kp if mu == "ragged_mask_absent" else K)
            X = np.where((k >= cut)[None, :] & (k >= Kp - 16)[None, :], np.float32(0.0), X)
        Wp = np.zeros((Np, max(Kp, 1)), dtype=np.float32)
        Wp[:N, :min(K, Kp)] = W[:, :min(K, Kp)]
        acc = np.zeros((M, Np), dtype=np.float32)
        with np.errstate(all="ignore"):
            for c in range(kch):
                for j in range(4):
                    for q in range(4):
                        kk = 16 * c + 4 * q + j
                        if kk >= K and np.isfinite(X[:, kk]).all():
                            continue
                        acc = _fma(X[:, kk:kk + 1], Wp[None, :, kk], acc)
        if mu == "last_col_tile_skipped":
            for n0 in range(0, Np, 16 * NT):
                ntv = min(NT, (N - n0 + 15) >> 4)
                if ntv < NT:
                    acc[:, n0 + 16 * (ntv - 1):n0 + 16 * ntv] = 0.0
        if mu == "rows_swapped":
            sw = np.arange(M) ^ 1
            acc = np.where((sw < M)[:, None], acc[np.minimum(sw, M - 1)], np.float32(0.0))
        bb = np.zeros(Np, dtype=np.float32)
        if bias is not None and epi != 2:
            n = np.arange(N) + (16 if mu == "bias_one_tile_late" else 0)
            bb[:N] = _gather(bias, n, pad4(N))
        with np.errstate(all="ignore"):
            v = f32(acc + bb[None, :])

        def side(mem, ldv, rows):
            """[M, Np] of a side input: columns >= ldv read as 0"""
            cols = np.arange(Np)
            return np.where((cols < ldv)[None, :], mem[np.minimum(rows[:, None] * ldv + cols[None, :], len(mem) - 1)], np.float32(0.0))

        def store(mem, ldv, vals, first_pad=Np):
            out = mem.copy()
            hi = min(ldv, Np, first_pad)
            out[:M * ldv].reshape(M, ldv)[:, :hi] = vals[:, :hi]
            return out

        zout = zmem
        if epi == 0:
            y = v
        elif epi == 1:
            y = gelu_tanh32(v) if mu == "tanh_gelu" else gelu32(v)
            zout = store(zmem, ldz, y if mu == "z_stored_after_gelu" else v)
        elif epi == 3:
            rows = np.arange(M) - rl if mu == "m_from_row_0" else np.arange(M)
            with np.errstate(all="ignore"):
                y = f32(v * side(mmem, ldm, rows))
            zout = store(zmem, ldz, v)
        else:
            y = gelu_grad32_times(side(zmem, ldz, np.arange(M)), acc, without_xphi=mu == "dgelu_without_xphi")
        return store(ymem, ldy, y, N if mu == "y_padding_not_zeroed" else Np), zout

    def gemm_tn(self, amem, lda, ni, bmem, ldb, nj, R, ws, ldws, colsum, zero_out, zero_n, waves, plan):
        mu = self.mutant
        nsplit, KT, DT, rps = plan
        ws = ws.copy()
        colsum = None if colsum is None else colsum.copy()

        def operand(mem, ldv, ncol, W):
            cols = np.arange(ncol)
            if mu == "kt8_halves_exchanged" and W == 8:
                cols = cols // 128 * 128 + (cols % 128 ^ 64)
            return _gather(mem, np.arange(R)[:, None] * ldv + cols[None, :], np.int64(len(mem)))
        A, B = operand(amem, lda, ni, KT), operand(bmem, ldb, nj, DT)
        for s in range(nsplit):
            lo = s * rps
            hi = min(R, lo + rps + (1 if mu == "splits_overlap" else 0))
            n = hi - lo
            if mu == "last_partial_step_dropped":
                n = n >> 2 << 2
            C = np.zeros((ni, nj), dtype=np.float32)
            part = np.zeros((4, ni), dtype=np.float32)
            with np.errstate(all="ignore"):
                for r in range(lo, lo + n):
                    C = _fma(A[r][:, None], B[r][None, :], C)
                    part[(r - lo) % 4] = f32(part[(r - lo) % 4] + A[r])
                ws[s * nj * ldws:(s + 1) * nj * ldws].reshape(nj, ldws)[:, :ni] = C.T
                if colsum is not None and not (mu == "colsum_by_tj1" and (nj + 15) // 16 <= DT):
                    colsum[s * ldws:s * ldws + ni] = f32(f32(part[0] + part[1]) + f32(part[2] + part[3]))
        if zero_out is not None:
            zero_out = zero_out.copy()
            zero_out[:(zero_n >> 2 << 2) if mu == "zero_tail_dropped" else zero_n] = 0.0
        return ws, colsum, zero_out

    def slab_reduce(self, sets, multi):
        mu, res = self.mutant, []
        for s in sets:
            nsplit, ni, nj, ldws, off, wide = s["nsplit"], s["ni"], s["nj"], s["ldws"], s["off"], s["wide"]
            gx, nchunk, spc = s["plan"]
            ws = s["wsmem"][:nsplit * nj * ldws].reshape(nsplit, nj, ldws)
            out = s["outmem"].copy()
            out2 = None if s["out2mem"] is None else s["out2mem"].copy()
            ii, jj = np.arange(ni)[:, None], np.arange(nj)[None, :]
            o_idx = off + ii * wide + jj
            o2_idx = (ii * wide + jj) if mu == "out2_with_out_strides" else (ii + jj * (ni + 3))
            with np.errstate(all="ignore"):
                for ch in range(nchunk):
                    hi = min(nsplit, (ch + 1) * spc) - (1 if mu == "last_slab_dropped" else 0)
                    a = np.zeros((ni, nj), dtype=np.float32)
                    for k in range(ch * spc, hi):
                        a = f32(a + ws[k, :, :ni].T)
                    out[o_idx] = a if mu == "store_not_add" else f32(out[o_idx] + a)
                    if out2 is not None:
                        ok = o2_idx < len(out2)                   # (what a mutant would write past the buffer is dropped)
                        out2[o2_idx[ok]] = f32(out2[o2_idx[ok]] + (a if mu == "sign2_ignored" else -a)[ok])
                vout = None
                if s["vecmem"] is not None:
                    vec = s["vecmem"][:nsplit * ldws].reshape(nsplit, ldws)
                    vout = np.full(ni + TAIL, SENTINEL, dtype=np.float32)
                    n = min(ni, 256) if mu == "vec_stops_at_256" else ni
                    a = np.zeros(n, dtype=np.float32)
                    for k in range(nsplit):
                        a = f32(a + vec[k, :n])
                    vout[:n] = a
            res.append((out, out2, vout))
        return res
