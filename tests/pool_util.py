"""Shared by the tests of the pool kernels (pool_loss.hip: bmm_rows_kernel behind nrm_pool_bmm, rowdot_kernel behind nrm_pool_rowdot; their
ragged and weighted instantiations behind nrm_pool_bmm_ragged / _hragged / _wlast and nrm_pool_rowdot_wlast in the second half below):
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

The ragged and the weighted forms (the other instantiations of bmm_rows_kernel and rowdot_kernel), same machinery
---------------------------------------------------------------------------------------------------------------
nrm_pool_bmm_ragged    out[c,:] = sum_j s[c,j] h[b(c),j,:]                     s [N, H], h [B, H, D], out [N, D]; list b = rows c0_b .. c1_b - 1,
                                                                               c0_b = clamp(cand_off[b], 0, N), c1_b = clamp(cand_off[b+1], c0_b, N)
nrm_pool_bmm_hragged   out[c,:] = sum_{j<K_b} w_j s[c,j] h[r0_b + j,:]         r0_b = clamp(hist_off[b], 0, R), K_b = clamp(hist_off[b+1], r0_b, R) - r0_b;
                       w_j = 1 except w_{K_b-1} = hist_mult[b] where > 0       the scores of candidate i of list b: s[16 (t0_b + i nt_b) + j], nt_b =
                                                                               ceil(K_b / 16), t0_b = clamp(tile_pre[b], 0, Mt); only the first
                                                                               floor((Mt - t0_b) / nt_b) rows of a list are written, none where K_b = 0
nrm_pool_bmm_wlast     wlast_row = 0: nrm_pool_bmm with W[b,i,J-1] taken as wlast W[b,i,J-1]
                       wlast_row = 1: out[b,I-1,:] = wlast sum_j W[b,I-1,j] X[b,j,:] (+ what `accumulate` finds, unweighted); other rows as nrm_pool_bmm
nrm_pool_rowdot_wlast  nrm_pool_rowdot with ds[b,t,H-1] = wlast g[b,t,:] . h[b,H-1,:]
Rows of `out` that no list owns, or that a list is cut short of, keep what they held: the SENTINEL here.

Bounds.  The weight costs ONE more rounding on the terms it touches and nothing else changes in the chain:
  column weight (hragged, wlast_row = 0): the kernel forms a' = fl(w W[.,J-1]) where it reads W and feeds a' to the same chain, so the last
      term sees one rounding more than the J of the chain: (J + 1) U sum_j w_j |W X| holds for every term (J = K_b for hragged, H for the
      unweighted ragged entry, where it is the dense J U sum |W X|).  A weight that is a power of two -- 1 where hist_mult is 0 -- multiplies
      exactly and the factor stays J.
  row weight (wlast_row = 1): fl(w acc) on the finished product of row I - 1, one rounding on all of its terms:
      (J + 1) U w sum_j |W X| on that row, J U sum_j |W X| on the others; `accumulate` adds U (|prior| + |ref|) as in the dense entry,
      the prior unweighted (were the weight to scale the prior, the error would be (w - 1) |prior|: far outside).
  rowdot_wlast: fl(w acc) at the store of column H - 1: (D + 1) U w sum_d |g h| there, D U sum_d |g h| elsewhere.
One-hot rows: a row that selects the weighted row (or the weighted output row / column) has the single product w x, formed either as
fma(fl(w 1), x, 0) or as fl(w fl(1 x)): one rounding of the exact w x, so the result is fl(w x) BITWISE for every w, not only 1, 2 and 4.
Every third one-hot row selects the last (kept) row.  wlast = 1 must give the bits of the dense entry on the same memory.
Unread score columns (K_b .. 16 nt_b of every tile), unowned score rows and the ldx / ldg padding hold NaN.

Cases.  ragged: the counts (0, 1, 15, 16, 17, 64, 65, 130, 0) in two orders (two empty lists cannot stand first, in the middle AND last:
order 0 has them first and in the middle, order 1 in the middle and last; the cases alternate), N three rows longer than the lists;
H in (1, 4, 5, 33, 130) at D = 68 and D in (4, 132) at H = 33.  hragged: K_b = (1, 4, 5, 15, 16, 17, 33, 64, 65) under the counts
(17, 0, 1, 65, 16, 3, 130, 2, 64), hist_mult from (0, 2, 3, 37), the same D.  Clamped tables: see ragged_clamped / hragged_clamped.
wlast_row = 0: I in (1, 17, 65) x J in (1, 4, 5, 16, 17, 33, 37, 130), W = s.  wlast_row = 1: I in (1, 16, 17, 64, 65, 130) x J in (1, 5, 33),
both W layouts, accumulate 0 and 1, ldx alternating between D and D + 4.  rowdot_wlast: H x T x D x ldg as listed.  Weights (1, 2, 3, 37).

Mutants of the new forms (one-line changes of the kernels) and where they can show:
  count_not_taken            `I = ... - c0` dropped: every list has max_count rows            ragged: where such rows reach a row no list owns
  cand_off_w_base_dropped    `W += c0 wsi` dropped                                            ragged: a non-empty list with c0 > 0 (not one-hot s at H = 1)
  cand_off_out_base_dropped  `out += c0 ldo` dropped                                          ragged, hragged: a written list with c0 > 0
  hist_off_base_dropped      `X += r0 ldx` dropped                                            hragged: a written list with r0 > 0
  score_stride_from_k_max    wsi = 16 ceil(k_max / 16)                                        hragged: a list of >= 2 written rows, nt_b != ceil(k_max / 16)
  tile_pre_ignored           t0 = 0                                                           hragged: a written list with t0 > 0
  tile_clamp_dropped         I not cut to (Mt - t0) / nt                                      hragged: a list that is cut short (clamped tables only)
  hist_mult_ignored          wlast stays 1                                                    hragged: a written list with hist_mult > 1
  hist_mult_at_k_max         the weight at j == k_max - 1                                     hragged: a written list with hist_mult > 1 and K_b != k_max
  mult_in_every_wave         j == j_hi - 1 for J - 1: each wave weights its own last row       hragged, wlast_row = 0: JSPLIT, J >= 5, weight != 1, dense families
  wlast_ignored              the weight is never applied                                      wlast, rowdot_wlast: w != 1
  wlast_row_ignored          wlast_row = 1 taken as 0                                         wlast_row = 1: w != 1, I >= 2
  wlast_scales_prior         the weight after the accumulate                                  wlast_row = 1: w != 1, accumulate
  wlast_row_last_of_group    i == i0 + 63 for I - 1                                           wlast_row = 1: w != 1, I != 64
  rowdot_wlast_last_of_trip  hc == h0 + 63 for H - 1                                          rowdot_wlast: w != 1, H != 64
Ignoring `i0 >= I` (a task past its list does not leave) is no mutant of these kernels: nit <= 0 and the `i < I` of the store keep such a task
from computing or writing anything, so the early return saves time only and no check of results can see it.
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

WEIGHTS = (1, 2, 3, 37)
RAGGED_COUNTS = ((0, 17, 130, 1, 0, 65, 16, 64, 15), (15, 64, 0, 65, 1, 130, 17, 16, 0))       # empty lists first + middle, middle + last
RAGGED_H = (1, 4, 5, 33, 130)
RAGGED_D = (4, 68, 132)
HRAGGED_K = (1, 4, 5, 15, 16, 17, 33, 64, 65)
HRAGGED_COUNTS = (17, 0, 1, 65, 16, 3, 130, 2, 64)
HRAGGED_MULT = (2, 37, 0, 3, 0, 2, 37, 0, 3)
WLAST_R0_I, WLAST_R0_J = (1, 17, 65), (1, 4, 5, 16, 17, 33, 37, 130)
WLAST_R1_I, WLAST_R1_J = (1, 16, 17, 64, 65, 130), (1, 5, 33)
WLAST_B, WLAST_D = 2, 68
ROWDOT_WLAST_H, ROWDOT_WLAST_T, ROWDOT_WLAST_D, ROWDOT_WLAST_B = (1, 16, 63, 64, 65, 130), (1, 17), (4, 20, 36), 2
RAGGED_MUTANTS = ("count_not_taken", "cand_off_w_base_dropped", "cand_off_out_base_dropped")
HRAGGED_MUTANTS = ("cand_off_out_base_dropped", "hist_off_base_dropped", "score_stride_from_k_max", "tile_pre_ignored", "tile_clamp_dropped",
                   "hist_mult_ignored", "hist_mult_at_k_max", "mult_in_every_wave")
WLAST_MUTANTS = ("wlast_ignored", "mult_in_every_wave", "wlast_row_ignored", "wlast_scales_prior", "wlast_row_last_of_group")
ROWDOT_WLAST_MUTANTS = ("wlast_ignored", "rowdot_wlast_last_of_trip")


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


# ------------------------------------------------------------------------------------------------ nrm_pool_bmm_ragged / _hragged
def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def _exact_weight(w):
    """a power of two multiplies without a rounding"""
    w = int(w)
    return w & (w - 1) == 0


def ragged_lists(cand_off, N):
    """the header's clamping rule -> [(c0, rows)] per list"""
    out = []
    for b in range(len(cand_off) - 1):
        c0 = _clamp(cand_off[b], 0, N)
        out.append((c0, _clamp(cand_off[b + 1], c0, N) - c0))
    return out


def hragged_lists(cand_off, hist_off, hist_mult, tile_pre, N, R, Mt):
    """the header's clamping rules -> per list dict(c0, rows, r0, K, t0, nt, written, w): `written` of its `rows` have scores, none where K = 0"""
    out = []
    for b, (c0, rows) in enumerate(ragged_lists(cand_off, N)):
        r0 = _clamp(hist_off[b], 0, R)
        K = _clamp(hist_off[b + 1], r0, R) - r0
        nt, t0 = (K + 15) // 16, _clamp(tile_pre[b], 0, Mt)
        written = min(rows, (Mt - t0) // nt) if nt else 0
        out.append(dict(c0=c0, rows=rows, r0=r0, K=K, t0=t0, nt=nt, written=written, w=int(hist_mult[b]) if hist_mult[b] > 0 else 1))
    return out


def _no_row_twice(lists, N):
    seen = np.zeros(N, dtype=np.int64)
    for c0, rows in lists:
        seen[c0:c0 + rows] += 1
    assert seen.max(initial=0) <= 1, "two lists own the same row: the launch would race"
    return seen.astype(bool)


def _family_operands(rng, family, n, J, D, last_every_third=True):
    """W [n, J], X-scaling for D columns, hot [n] or None"""
    hot = None
    if family == "onehot":
        hot = rng.integers(0, J, n)
        if last_every_third:
            hot[::3] = J - 1
        W = np.zeros((n, J))
        W[np.arange(n), hot] = 1.0
    else:
        W = rng.standard_normal((n, J))
        if family == "scaled":
            W = W * 2.0 ** ((np.arange(n) % 5) - 2.0)[:, None]
    xs = 2.0 ** ((np.arange(D) % 7) - 3.0) if family == "scaled" else np.ones(D)
    return W, xs, hot


def make_ragged(cand_off, N, H, D, family, seed=0):
    """cand_off as given to the entry (clamped by the header's rule here); max_count = the longest clamped list"""
    cand_off = np.asarray(cand_off, dtype=np.int32)
    B = len(cand_off) - 1
    lists = ragged_lists(cand_off, N)
    owned = _no_row_twice(lists, N)
    rng = np.random.default_rng([B, N, H, D, BMM_FAMILIES.index(family), seed, 11])
    W, xs, hot = _family_operands(rng, family, N, H, D)
    W, X = f32(W), f32(rng.standard_normal((B, H, D)) * xs)
    ref, mag = np.zeros((N, D)), np.zeros((N, D))
    for b, (c0, rows) in enumerate(lists):
        ref[c0:c0 + rows] = f64(W[c0:c0 + rows]) @ f64(X[b])
        mag[c0:c0 + rows] = np.abs(f64(W[c0:c0 + rows])) @ np.abs(f64(X[b]))
    smem = W.copy()
    smem[~owned] = np.nan                                   # score rows of no list are not read
    want = None
    if hot is not None:
        want = np.zeros((N, D), dtype=np.float32)
        for b, (c0, rows) in enumerate(lists):
            want[c0:c0 + rows] = X[b][hot[c0:c0 + rows]]
    return dict(B=B, N=N, H=H, D=D, family=family, cand_off=cand_off, max_count=max([r for _, r in lists], default=0), lists=lists,
                owned=owned, smem=np.concatenate([smem.reshape(-1), np.full(TAIL, np.nan, dtype=np.float32)]),
                hmem=np.concatenate([X.reshape(-1), np.full(TAIL, np.nan, dtype=np.float32)]), ref=ref, bound=H * U * mag, want=want)


def ragged_case(order, H, D, family):
    counts = RAGGED_COUNTS[order]
    cand_off = np.concatenate([[0], np.cumsum(counts)])
    return make_ragged(cand_off, int(cand_off[-1]) + 3, H, D, family, seed=order)


def ragged_shapes():
    """(order of the counts, H, D)"""
    shapes = [(H, 68) for H in RAGGED_H] + [(33, D) for D in RAGGED_D if D != 68]
    return [(n % 2, H, D) for n, (H, D) in enumerate(shapes)]


def ragged_clamped(family, which):
    """N = 40 rows, H = 33, D = 68.  Table 0: a negative cand_off[0] (list 0 = rows 0 .. 2), cand_off[3] = 45 > N (list 2 = rows 20 .. 39) and
    cand_off[4] = 38 < cand_off[3] (list 3 starts at the clamped 40 and is empty).  Such entries leave no row unowned without making two
    lists overlap, so table 1 has the gaps: cand_off[1] < cand_off[0] (list 0 empty at 6, list 1 = rows 2 .. 8: rows 0, 1 unowned) and
    cand_off[6] < cand_off[5] (rows 36 .. 39 unowned)."""
    tab = ([-5, 3, 20, 45, 38], [6, 2, 9, 30, 30, 36, 33])[which]
    return make_ragged(tab, 40, 33, 68, family, seed=100 + which)


def make_hragged(cand_off, hist_off, hist_mult, tile_pre, N, R, Mt, D, family, seed=0):
    """tables as given to the entry; max_count / k_max = the longest clamped list / kept history"""
    tabs = [np.asarray(t, dtype=np.int32) for t in (cand_off, hist_off, hist_mult, tile_pre)]
    B = len(tabs[0]) - 1
    lists = hragged_lists(*tabs, N, R, Mt)
    _no_row_twice([(g["c0"], g["rows"]) for g in lists], N)
    rng = np.random.default_rng([B, N, R, Mt, D, BMM_FAMILIES.index(family), seed, 13])
    xs = 2.0 ** ((np.arange(D) % 7) - 3.0) if family == "scaled" else np.ones(D)
    X = f32(rng.standard_normal((R, D)) * xs)
    smem = np.full(16 * Mt + TAIL, np.nan, dtype=np.float32)
    ref, bound, owned = np.zeros((N, D)), np.zeros((N, D)), np.zeros(N, dtype=bool)
    want = np.zeros((N, D), dtype=np.float32) if family == "onehot" else None
    for g in lists:
        n, K, c0 = g["written"], g["K"], g["c0"]
        if n == 0:
            continue
        W, _, hot = _family_operands(rng, family, n, K, D)
        W = f32(W)
        idx = 16 * (g["t0"] + np.arange(n)[:, None] * g["nt"]) + np.arange(K)[None, :]
        assert idx.max() < 16 * Mt
        smem[idx] = W                                       # the columns K .. 16 nt of a candidate's tiles stay NaN
        wj = np.ones(K)
        wj[K - 1] = g["w"]
        Xb = X[g["r0"]:g["r0"] + K]
        ref[c0:c0 + n] = (f64(W) * wj) @ f64(Xb)
        bound[c0:c0 + n] = (K + (0 if _exact_weight(g["w"]) else 1)) * U * ((np.abs(f64(W)) * wj) @ np.abs(f64(Xb)))
        owned[c0:c0 + n] = True
        if hot is not None:
            want[c0:c0 + n] = (f64(Xb[hot]) * wj[hot][:, None]).astype(np.float32)      # fl(w x): w x is exact in float64
    return dict(B=B, N=N, R=R, Mt=Mt, D=D, family=family, cand_off=tabs[0], hist_off=tabs[1], hist_mult=tabs[2], tile_pre=tabs[3],
                max_count=max([g["rows"] for g in lists], default=0), k_max=max([g["K"] for g in lists], default=0), lists=lists, owned=owned,
                smem=smem, hmem=np.concatenate([X.reshape(-1), np.full(TAIL, np.nan, dtype=np.float32)]), ref=ref, bound=bound, want=want)


def hragged_case(D, family):
    K, counts = np.array(HRAGGED_K), np.array(HRAGGED_COUNTS)
    cand_off, hist_off = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(K)])
    tile_pre = np.concatenate([[0], np.cumsum(counts * ((K + 15) // 16))])
    return make_hragged(cand_off, hist_off, HRAGGED_MULT, tile_pre, int(cand_off[-1]) + 3, int(hist_off[-1]), int(tile_pre[-1]), D, family)


def hragged_clamped(family):
    """N = 40, R = 30, Mt = 27, D = 68, five lists:
      0  cand_off -5 -> rows 0 .. 2;  K = 5;  tile_pre -2 -> tile 0;  hist_mult 3
      1  rows 3 .. 19;  hist_off[2] = hist_off[1]: K = 0, nothing is written: the 17 rows keep what they held
      2  rows 20 .. 27;  K = 17, two tiles per candidate from tile 3;  hist_mult 0
      3  cand_off[4] = 45 -> rows 28 .. 39;  hist_off[4] = 35 > R -> K = 30 - 22 = 8;  from tile 19 only (27 - 19) / 1 = 8 of the 12 rows
         have scores: rows 28 .. 35 are written, 36 .. 39 left;  hist_mult 37
      4  cand_off[5] = 38 < 45: empty at row 40;  hist_off[5] = 33 < 35: K = 0;  tile_pre 40 > Mt"""
    return make_hragged([-5, 3, 20, 28, 45, 38], [0, 5, 5, 22, 35, 33], [3, 2, 0, 37, 5], [-2, 3, 3, 19, 40, 40], 40, 30, 27, 68, family, seed=7)


def _check_rows(key, got, c):
    N, D = c["N"], c["D"]
    out = got[:N * D].reshape(N, D)
    own = c["owned"]
    left = 0.0 if (bits(out[~own]) == bits(SENTINEL)).all() else INF
    res = {key: max(ratio(out[own], c["ref"][own], c["bound"][own]), left, tail_kept(got, N * D))}
    if c["want"] is not None:
        res[key + ".onehot"] = same_bits(out[own], c["want"][own])
    return res


def check_ragged(be, c, form):
    out = np.full(c["N"] * c["D"] + TAIL, SENTINEL, dtype=np.float32)
    got = be.bmm_ragged(c["smem"], c["hmem"], out, c["cand_off"], c["B"], c["N"], c["max_count"], c["H"], c["D"], form)
    return _check_rows("pool_bmm_ragged", got, c)


def check_hragged(be, c, form):
    out = np.full(c["N"] * c["D"] + TAIL, SENTINEL, dtype=np.float32)
    got = be.bmm_hragged(c["smem"], c["hmem"], out, c["cand_off"], c["hist_off"], c["hist_mult"], c["tile_pre"], c["B"], c["N"], c["max_count"],
                         c["R"], c["Mt"], c["k_max"], c["D"], form)
    return _check_rows("pool_bmm_hragged", got, c)


def ragged_applies(mutant, c):
    lists = c["lists"]
    if mutant == "count_not_taken":
        reach = np.zeros(c["N"], dtype=bool)
        for c0, _ in lists:
            reach[c0:c0 + c["max_count"]] = True
        return bool((reach & ~c["owned"]).any())
    if mutant == "cand_off_w_base_dropped" and c["family"] == "onehot" and c["H"] == 1:
        return False                                                # every row of a one-hot s is the same row at H = 1
    return any(rows > 0 and c0 > 0 for c0, rows in lists)           # the two dropped bases


def hragged_applies(mutant, c, jsplit):
    live = [g for g in c["lists"] if g["written"] > 0]
    kt = (c["k_max"] + 15) // 16
    dense = c["family"] != "onehot"
    return {"cand_off_out_base_dropped": any(g["c0"] > 0 for g in live), "hist_off_base_dropped": any(g["r0"] > 0 for g in live),
            "score_stride_from_k_max": any(g["written"] >= 2 and g["nt"] != kt for g in live), "tile_pre_ignored": any(g["t0"] > 0 for g in live),
            "tile_clamp_dropped": any(g["K"] > 0 and g["written"] < g["rows"] for g in c["lists"]),
            "hist_mult_ignored": any(g["w"] > 1 for g in live), "hist_mult_at_k_max": any(g["w"] > 1 and g["K"] != c["k_max"] for g in live),
            "mult_in_every_wave": dense and jsplit and any(g["w"] > 1 and g["K"] >= 5 for g in live)}[mutant]


# ------------------------------------------------------------------------------------------------ nrm_pool_bmm_wlast / nrm_pool_rowdot_wlast
def wlast_shapes(row):
    """(I, J, ldx): wlast_row = 0 at both ldx, wlast_row = 1 with ldx alternating"""
    if row == 0:
        return [(i, j, ldx) for i in WLAST_R0_I for j in WLAST_R0_J for ldx in (WLAST_D, WLAST_D + 4)]
    return [(i, j, WLAST_D + 4 * (n % 2)) for n, (i, j) in enumerate((i, j) for i in WLAST_R1_I for j in WLAST_R1_J)]


def make_wlast(I, J, ldx, layout, family):
    """a dense case whose every third one-hot row selects row J - 1"""
    c = make_bmm(WLAST_B, I, J, WLAST_D, layout, ldx, family, seed=1)
    if family != "onehot":
        return c
    hot = c["hot"].copy()
    hot[:, ::3] = J - 1
    W = np.zeros((WLAST_B, I, J), dtype=np.float32)
    np.put_along_axis(W, hot[:, :, None], 1.0, axis=2)
    wmem = (W if layout == "s" else np.ascontiguousarray(W.transpose(0, 2, 1))).reshape(-1)
    c.update(W=W, hot=hot, wmem=np.concatenate([wmem, np.full(TAIL, np.nan, dtype=np.float32)]))
    return c


def wlast_bound(c, w, row, accumulate):
    """-> ref, bound, the weights as an array that multiplies W"""
    I, J = c["I"], c["J"]
    wt = np.ones((I, J))
    if row:
        wt[I - 1, :] = w
    else:
        wt[:, J - 1] = w
    W, X = f64(c["W"]) * wt, f64(c["X"])
    ref, mag = np.matmul(W, X), np.matmul(np.abs(W), np.abs(X))
    fac = np.full((I, 1), float(J))
    if not _exact_weight(w):
        fac[I - 1 if row else slice(None)] += 1
    bound = fac * U * mag
    if accumulate:
        ref = ref + f64(c["prior"])
        bound = bound + U * (np.abs(f64(c["prior"])) + np.abs(ref))
    return ref, bound, wt


def check_wlast(be, c, w, row, accumulate, form):
    B, I, J, D = c["B"], c["I"], c["J"], c["D"]
    n = B * I * D
    out = np.full(n + TAIL, SENTINEL, dtype=np.float32)
    if accumulate:
        out[:n] = c["prior"].reshape(-1)
    got = be.bmm_wlast(c["wmem"], *c["strides"], c["xmem"], c["ldx"], out, B, I, J, D, accumulate, w, row, form)
    ref, bound, wt = wlast_bound(c, w, row, accumulate)
    key = f"pool_bmm_wlast.r{row}"
    res = {key: max(ratio(got[:n].reshape(B, I, D), ref, bound), tail_kept(got, n))}
    if c["family"] == "onehot" and not accumulate:
        x = np.take_along_axis(c["X"], c["hot"][:, :, None], axis=1)
        wsel = np.take_along_axis(np.broadcast_to(wt, (B, I, J)), c["hot"][:, :, None], axis=2)
        res[key + ".onehot"] = same_bits(got[:n].reshape(B, I, D), (f64(x) * wsel).astype(np.float32))
    if w == 1:
        res[key + ".dense_bits"] = same_bits(got, be.bmm(c["wmem"], *c["strides"], c["xmem"], c["ldx"], out, B, I, J, D, accumulate, form))
    return res


def wlast_applies(mutant, family, jsplit, row, I, J, w, accumulate):
    if w == 1:
        return False
    return {"wlast_ignored": True, "mult_in_every_wave": row == 0 and jsplit and J >= 5 and family != "onehot", "wlast_row_ignored": row == 1 and I >= 2,
            "wlast_scales_prior": row == 1 and bool(accumulate), "wlast_row_last_of_group": row == 1 and I != 64}[mutant]


def rowdot_wlast_shapes():
    return [(ROWDOT_WLAST_B, t, h, d, ldg) for h in ROWDOT_WLAST_H for t in ROWDOT_WLAST_T for d in ROWDOT_WLAST_D for ldg in (d, d + 4)]


def check_rowdot_wlast(be, c, w, zero_n):
    B, T, H, D = c["B"], c["T"], c["H"], c["D"]
    n = B * T * H
    ds = np.full(n + TAIL, SENTINEL, dtype=np.float32)
    zero = np.full(ZERO_LEN, np.nan, dtype=np.float32)
    got, zgot = be.rowdot_wlast(c["gmem"], c["ldg"], c["hmem"], ds, B, T, H, D, zero, zero_n, w)
    wt = np.ones(H)
    wt[H - 1] = w
    fac = np.full(H, float(D))
    if not _exact_weight(w):
        fac[H - 1] += 1
    res = {"pool_rowdot_wlast": max(ratio(got[:n].reshape(B, T, H), c["ref"] * wt, fac * wt * U * c["mag"]), tail_kept(got, n))}
    zb = bits(zgot)
    res["pool_rowdot_wlast.zero"] = 0.0 if not zb[:zero_n].any() and np.array_equal(zb[zero_n:], bits(zero)[zero_n:]) else INF
    if c["family"] == "onehot":
        want = np.take_along_axis(c["h"].transpose(0, 2, 1), c["hot"][:, :, None], axis=1)          # [B, T, H]
        res["pool_rowdot_wlast.onehot"] = same_bits(got[:n].reshape(B, T, H), (f64(want) * wt).astype(np.float32))
    if w == 1:
        dgot, dz = be.rowdot(c["gmem"], c["ldg"], c["hmem"], ds, B, T, H, D, zero, zero_n)
        res["pool_rowdot_wlast.dense_bits"] = max(same_bits(got, dgot), same_bits(zgot[zero_n:], dz[zero_n:]), same_bits(zgot[:zero_n], dz[:zero_n]))
    return res


def rowdot_wlast_applies(mutant, H, w):
    return w != 1 and (mutant == "wlast_ignored" or H != 64)


# ------------------------------------------------------------------------------------------------ the float32 emulation
def _fma(a, b, acc):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64; the sum rounds to 53 bits and then to 24 (a double
    rounding differs from the single one only on a tie of the second, a case in 2^29)"""
    return (f64(a) * f64(b) + f64(acc)).astype(np.float32)


def _strided_rows(mem, base, n, ld, D):
    """[n, D]: the floats base + r ld .. + D of a flat buffer, r < n"""
    return mem[base + np.arange(n)[:, None] * ld + np.arange(D)[None, :]]


def _chain(W, X, jsplit, wcol=None, every_wave=False):
    """bmm_rows_kernel's arithmetic for W [.., I, J], X [.., J, D]: per wave a j-ordered fused chain from 0 over its rows (the whole range, or
    whole rounds of 4 rows: ceil(J / 16) * 4 each), the waves' tiles added onto wave 0's in wave order.  wcol = (j, w): the kernel's
    `a *= wlast` where column j of W is read -- one fp32 product, then the chain.  every_wave: the mutant that tests j == j_hi - 1."""
    J = W.shape[-1]
    jq = (J + 15) // 16 * 4 if jsplit else J
    total = None
    for wave in range(4 if jsplit else 1):
        lo, hi = wave * jq, min(J, (wave + 1) * jq)
        acc = np.zeros(W.shape[:-1] + X.shape[-1:], dtype=np.float32)
        for j in range(lo, hi):
            a = W[..., j]
            if wcol is not None and (j == wcol[0] or (every_wave and j == hi - 1)):
                a = a * np.float32(wcol[1])
            acc = _fma(a[..., None], X[..., j, :][..., None, :], acc)
        total = acc if total is None else total + acc
    return total


def _take(mem, idx):
    """the emulation of a MUTANT may index past its buffer: it reads the last float (a NaN) there, where the kernel would read anything"""
    return mem[np.minimum(idx, len(mem) - 1)]


def _put_rows(out, row0, vals):
    """rows row0 .. of a flat [.., D] buffer; what a mutant would write past the buffer is dropped"""
    n, D = vals.shape
    n = max(0, min(n, (len(out) - row0 * D) // D))
    out[row0 * D:(row0 + n) * D] = vals[:n].reshape(-1)


class Emulated:
    """The kernels in float32 in their own order.  ``form`` of the bmm entries: as the launcher's plan takes it."""

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

    def bmm_ragged(self, smem, hmem, out, cand_off, B, N, max_count, H, D, form):
        out, m = out.copy(), self.mutant
        jsplit = jsplit_taken(form, B, max_count, H, D)
        with np.errstate(all="ignore"):
            for b in range(B):                              # (a mutant that writes a row twice: the later list wins here)
                c0 = _clamp(cand_off[b], 0, N)
                rows = max_count if m == "count_not_taken" else _clamp(cand_off[b + 1], c0, N) - c0
                rows = min(rows, (max_count + 63) // 64 * 64)                       # the row groups of the grid
                if rows <= 0:
                    continue
                w0 = 0 if m == "cand_off_w_base_dropped" else c0
                W = _take(smem, (w0 + np.arange(rows)[:, None]) * H + np.arange(H)[None, :])
                X = hmem[b * H * D:(b + 1) * H * D].reshape(H, D)
                _put_rows(out, 0 if m == "cand_off_out_base_dropped" else c0, _chain(W, X, jsplit))
        return out

    def bmm_hragged(self, smem, hmem, out, cand_off, hist_off, hist_mult, tile_pre, B, N, max_count, R, Mt, k_max, D, form):
        out, m = out.copy(), self.mutant
        jsplit = jsplit_taken(form, B, max_count, k_max, D)
        with np.errstate(all="ignore"):
            for b in range(B):
                c0 = _clamp(cand_off[b], 0, N)
                rows = _clamp(cand_off[b + 1], c0, N) - c0
                r0 = _clamp(hist_off[b], 0, R)
                K = _clamp(hist_off[b + 1], r0, R) - r0
                nt = (K + 15) // 16
                t0 = 0 if m == "tile_pre_ignored" else _clamp(tile_pre[b], 0, Mt)
                if m != "tile_clamp_dropped":
                    rows = min(rows, (Mt - t0) // nt if nt else 0)
                rows = min(rows, (max_count + 63) // 64 * 64)
                if rows <= 0 or K <= 0:
                    continue
                wsi = 16 * ((k_max + 15) // 16) if m == "score_stride_from_k_max" else 16 * nt
                W = _take(smem, 16 * t0 + np.arange(rows)[:, None] * wsi + np.arange(K)[None, :])
                x0 = 0 if m == "hist_off_base_dropped" else r0
                X = hmem[x0 * D:(x0 + K) * D].reshape(K, D)
                w = 1 if m == "hist_mult_ignored" or hist_mult[b] <= 0 else int(hist_mult[b])
                jw = k_max - 1 if m == "hist_mult_at_k_max" else K - 1
                acc = _chain(W, X, jsplit, wcol=(jw, w) if jw < K else None, every_wave=m == "mult_in_every_wave")
                _put_rows(out, 0 if m == "cand_off_out_base_dropped" else c0, acc)
        return out

    def _dense_operands(self, wmem, wsb, wsi, wsj, xmem, ldx, B, I, J, D):
        b_, i_, j_ = np.arange(B)[:, None, None], np.arange(I)[None, :, None], np.arange(J)[None, None, :]
        return wmem[b_ * wsb + i_ * wsi + j_ * wsj], np.stack([_strided_rows(xmem, b * J * ldx, J, ldx, D) for b in range(B)])

    def bmm_wlast(self, wmem, wsb, wsi, wsj, xmem, ldx, out, B, I, J, D, accumulate, wlast, wlast_row, form):
        out, m = out.copy(), self.mutant
        W, X = self._dense_operands(wmem, wsb, wsi, wsj, xmem, ldx, B, I, J, D)
        w = np.float32(1 if m == "wlast_ignored" else wlast)
        row = 0 if m == "wlast_row_ignored" else wlast_row
        rows = [i for i in range(I) if i % 64 == 63] if m == "wlast_row_last_of_group" else [I - 1]
        n = B * I * D
        with np.errstate(all="ignore"):
            acc = _chain(W, X, jsplit_taken(form, B, I, J, D), wcol=None if row else (J - 1, w), every_wave=m == "mult_in_every_wave")
            if row and m != "wlast_scales_prior":
                acc[:, rows] = acc[:, rows] * w
            if accumulate:
                acc = acc + out[:n].reshape(B, I, D)
            if row and m == "wlast_scales_prior":
                acc[:, rows] = acc[:, rows] * w
        out[:n] = acc.reshape(-1)
        return out

    def rowdot_wlast(self, gmem, ldg, hmem, ds, B, T, H, D, zero_out, zero_n, wlast):
        ds, zero_out = self.rowdot(gmem, ldg, hmem, ds, B, T, H, D, zero_out, zero_n)
        cols = [h for h in range(H) if h % 64 == 63] if self.mutant == "rowdot_wlast_last_of_trip" else [H - 1]
        if self.mutant != "wlast_ignored":
            acc = ds[:B * T * H].reshape(B, T, H)           # a view: the product at the store
            with np.errstate(all="ignore"):
                acc[:, :, cols] = np.float32(wlast) * acc[:, :, cols]
        return ds, zero_out
