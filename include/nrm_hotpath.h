/* nrm_hotpath.h -- C ABI of the MI355X (gfx950) hot path of News_Recommendation_Model.
 *
 * The reference has no FFI: its boundary is Python nn.Module.  This library is
 * what the Modules in news_recommendation_model_amd/modules.py bind through ctypes; every entry point
 * names the reference code it replaces.  Conventions:
 *   - all pointers are DEVICE pointers to fp32 (or as stated), row-major, caller-owned ("borrowed");
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it and never
 *     synchronises or allocates;
 *   - return value 0 = ok, otherwise a negative NRM_E* code; nrm_last_error() gives the text
 *     (thread-local).  Shapes are validated on the host before any launch;
 *   - D (feature width of one attention) must be a multiple of 4; B*T*H < 2^31.
 */
#ifndef NRM_HOTPATH_H
#define NRM_HOTPATH_H

#ifdef __cplusplus
extern "C" {
#endif

#define NRM_ABI_VERSION 7
#define NRM_OK 0
#define NRM_EINVAL (-1)   /* bad shape / alignment / null pointer */
#define NRM_ELAUNCH (-2)  /* HIP launch error */

typedef void* nrm_stream_t;

int nrm_abi_version(void);
const char* nrm_last_error(void);
/* 0 for a product build.  Non-zero: the library was compiled with one of the timing-diagnostic overrides of scripts/_diag
 * (kernels with parts of their work removed: results are WRONG by construction); the Python binding refuses to load such a
 * library unless NRM_ALLOW_DIAG_LIB=1. */
int nrm_build_flags(void);
/* Provenance (round 5): the sha256 over the kernel sources (csrc/ and this header, news_recommendation_model_amd/build.py
 * sources_digest()) this library was compiled from, and a one-line build record (compiler, flags, UTC time).  The Python
 * binding refuses a library whose digest differs from the sources lying next to it (NRM_ALLOW_STALE_LIB=1 overrides), bench.py
 * prints both, so a measured binary is tied to the sources it is shown with. */
const char* nrm_source_digest(void);
const char* nrm_build_info(void);

/* ---- pointwise history attention: reference models/attention_model.py:52-97
 *      (PointwiseAttentionExpanded.forward), score[b,t,h] = fc2(GELU(fc1(cat[h,t,t-h,t*h]))).
 * The caller supplies the two side projections of the split fc1 = [W_h | W_t | W_d | W_p]:
 *      u[b,h,:] = h[b,h,:] (W_h - W_d)^T + fc1.bias        v[b,t,:] = t[b,t,:] (W_t + W_d)^T          */

/* Arithmetic of the bilinear contraction, chosen per call (BASELINE config 2 names bf16, config 3 fp32):
 *   NRM_MMA_F32   v_mfma_f32_16x16x4_f32: exact fp32 products and sums
 *   NRM_MMA_BF16  v_mfma_f32_16x16x32_bf16: operands rounded to bf16 (the t*h product is formed in fp32 and rounded
 *                 once, W_p / dz / h / t are rounded as they are read), fp32 accumulation starting from the fp32 u + v;
 *                 GELU, the fc2 dot, scores, pool and every reduction stay fp32
 *   NRM_MMA_BF16X3  the same instruction with both operands split into hi + lo bf16 parts (lo = rounding remainder) and
 *                 three MFMAs per product (lo*hi + hi*lo + hi*hi): fp32-class accuracy (~2^-16 per product) at 3/16 of the
 *                 fp32 MFMA time -- the arithmetic that keeps the <= 1e-3 parity gate of BASELINE with bf16 matrix cores */
#define NRM_MMA_F32 0
#define NRM_MMA_BF16 1
#define NRM_MMA_BF16X3 2
/* floats to allocate for the packed copy of W_p used by nrm_pwattn_fwd (either arithmetic) */
long nrm_pwattn_packed_floats(int D);
/* fc1_weight: [D, 4D] with row stride ld; packs W_p = fc1_weight[:, 3D:4D] for the given arithmetic */
int nrm_pwattn_pack_wp(const float* fc1_weight, int ld, int D, int mma, float* packed, nrm_stream_t stream);
/* t [B,T,D], h [B,H,D], u [B,H,D], v [B,T,D] contiguous; w2 = fc2.weight [D]; b2 = fc2.bias [1];
 * z [B,T,H,D] pre-activation saved for backward (NULL in inference); s [B,T,H] scores */
int nrm_pwattn_fwd(const float* t, const float* h, const float* u, const float* v, const float* packed_wp,
                   const float* w2, const float* b2, float* z, float* s,
                   int B, int T, int H, int D, int mma, nrm_stream_t stream);

/* backward, step 1 (autograd of attention_model.py:29-32 through GELU and fc2), one pass over z:
 *   z <- dz = ds * w2 * gelu'(z) in place;  dw2[k] += sum ds*gelu(z)   (dw2 must be initialised)
 *   du[b,h,:] = sum_t dz[b,t,h,:]  (gradient of u)      dv[b,t,:] = sum_h dz[b,t,h,:]  (gradient of v)
 * ds [B,T,H]; du [B,H,D] and dv [B,T,D] are overwritten (histories longer than 256 rows are processed in chunks).
 *   db2 (optional, may be NULL): *db2 += sum ds, the fc2 bias gradient (must be initialised like dw2) */
/* dz_format: how dz is left in z_inout.  NRM_DZ_F32: fp32.  NRM_DZ_HL4 (for the bf16 arithmetics): every aligned group of 4
 * values as 4 bf16 hi + 4 bf16 lo (lo = bf16 of the rounding remainder) in the same 16 bytes -- the MFMA-ready operand that
 * nrm_pwattn_bwd_rw_dtdh and the dW_p-only pass of nrm_pwattn_bwd_contract read without conversion (du, dv, dw2 are computed
 * from the fp32 values either way). */
#define NRM_DZ_F32 0
#define NRM_DZ_HL4 1
int nrm_pwattn_bwd_dz(float* z_inout, const float* ds, const float* w2, float* dw2, float* db2, float* du, float* dv,
                      int B, int T, int H, int D, int dz_format, nrm_stream_t stream);
/* number of [D,D] partial slabs nrm_pwattn_bwd_contract writes into `ws` (depends on the arithmetic: tile shapes differ) */
int nrm_pwattn_bwd_nsplit(int B, int T, int H, int D, int mma);
/* backward, step 2 (the bilinear term): given dz [B,T,H,D], t, h and W_p (row stride ldwp)
 *   dt[b,t,d] += sum_{h,k} dz W_p[k,d] h[b,h,d]      dh[b,h,d] += sum_{t,k} dz W_p[k,d] t[b,t,d]
 *   ws[i][d][k] (i < nsplit) = partial of dW_p[k,d] = sum_{b,t,h} dz[b,t,h,k] t[b,t,d] h[b,h,d]
 *                              (TRANSPOSED slabs: sum them over i, then transpose)
 * dt/dh are accumulated into (float atomics), ws is overwritten.
 * passes: bit 0 = the (b,t)-grouped launch (dt, ws), bit 1 = the (b,h)-grouped launch (dh); 3 = both.
 * passes = 4: the (b,t)-grouped launch WITHOUT its dt epilogue -- only ws (dt, dh may be NULL).  For a caller that wants no
 * row gradients at all (the model's text+image attention reads raw input columns: neither t nor h has a gradient), or -- bf16
 * arithmetics with dz in NRM_DZ_HL4 -- beside nrm_pwattn_bwd_rw_dtdh, which then delivers dt and dh.
 * dz_format names the layout of dz (NRM_DZ_HL4 only with passes = 4 and a bf16 arithmetic). */
int nrm_pwattn_bwd_contract(const float* dz, const float* t, const float* h, const float* wp, int ldwp,
                            float* dt, float* dh, float* ws,
                            int B, int T, int H, int D, int passes, int mma, int dz_format, nrm_stream_t stream);
/* Which kernel one launch of nrm_pwattn_bwd_contract takes (additive entry point, the ABI version is unchanged): the plan and
 * the selection of the launch itself, the environment knobs included, without any device call.  pass: 1, 2 or 4 (passes = 3
 * is launch 1, then launch 2).  Returns -1 for a combination nrm_pwattn_bwd_contract refuses, otherwise
 *   bits 0-1  kernel family: 0 serial E-form, 1 pipelined E-form ((b,h) groups), 2 one-accumulator dW_p, 3 32-row dW_p
 *   bit 2     EXACT (D fills whole wave tiles: no column guards)       bit 3  wave tile 5x5 (clear: 4x4)
 *   bit 4     the pass writes dW_p slabs     bit 5  it forms a row gradient (dt or dh)     bit 6  it reads NRM_DZ_HL4 */
int nrm_pwattn_bwd_form(int T, int H, int D, int pass, int mma, int dz_format);
/* How many consecutive (b,t) groups the fp32 dW_p-only launch (passes = 4, NRM_DZ_F32) of nrm_pwattn_bwd_contract reduces together
 * in whole 4-row steps (additive entry point, the ABI version is unchanged; no device call, the environment knobs applied -- NRM_DW_PACK=0
 * keeps every group on its own).  1: per group, its last step padded -- H % 4 == 0, splits shorter than a super-group, every launch that
 * is not the one-accumulator kernel; 2 for H = 2 mod 4, 4 for odd H.  Depends on B through the groups per split.  -1: bad arguments. */
int nrm_pwattn_bwd_dw_pack(int B, int T, int H, int D, int mma);
/* What one launch of the attention backward runs (additive entry point, the ABI version is unchanged): the answer of the host function
 * the launch itself switches on (bwd_dz_select, bwd_e_plan + bwd_e_select, pwattn_bwd_dp_select, pwattn_bwd_rw_select), without a device
 * call, a launch or an allocation, with the environment knobs applied as the launches apply them -- NRM_DZ_ROWS, NRM_BH_PIPE,
 * NRM_DW_DIRECT, NRM_DW_R32, NRM_DW_PACK, NRM_BT_WAVES, NRM_BH_WAVES, NRM_BT_INTERLEAVE, NRM_BT_ORDER, NRM_DP_GRID, NRM_BRW_WAVES and
 * NRM_BRW_TSPLIT at every call; NRM_BWD_RW and NRM_DZ_NARROW as latched at their first use in the process.
 *   launch: NRM_BWD_LAUNCH_DZ (nrm_pwattn_bwd_dz; pass and mma are not read), NRM_BWD_LAUNCH_CONTRACT (one launch of
 *           nrm_pwattn_bwd_contract: pass 1, 2 or 4), NRM_BWD_LAUNCH_DP (nrm_pwattn_bwd_dp_dtdh; pass, mma, dz_format not read),
 *           NRM_BWD_LAUNCH_RW (nrm_pwattn_bwd_rw_dtdh; pass and dz_format not read).
 *   cus: compute units of the device the launch would go to; 0: those of the current device, or 256 where there is none.
 * out[NRM_PWATTN_BWD_PLAN_LEN]; out[0] = valid (0: the launch entry answers with an error for this selection -- the dz slab needs more
 * than 160 KB of LDS, the dP walk or the resident-W backward does not take the shape) and the fields behind the last one named are 0:
 *   NRM_BWD_LAUNCH_DZ        [1] family 0 slab (bwd_dz_kernel), 1 full-row (bwd_dz_rows_kernel)   [2] threads per workgroup
 *                            [3] rows-per-thread class of the full-row form: 1 (up to 3 rows), 2 (4 to 6); 0 slab
 *                            [4] slab_cols  [5] slabs  [6] hchunk  [7] nhc (history chunks)   (slab form; 0 otherwise)
 *                            [8] dynamic LDS above 64 KB   [9] the narrowing loop ran   [10] dz_format as asked
 *   NRM_BWD_LAUNCH_CONTRACT  [1] kernel family as bits 0-1 of nrm_pwattn_bwd_form   [2] wave tile 4 | 5   [3] EXACT   [4] mma
 *                            [5] dW_p slabs written   [6] a row gradient formed   [7] NRM_DZ_HL4 read   [8] pack (nrm_pwattn_bwd_dw_pack)
 *                            [9] interleaved walk, [10] block order, as the kernel honours them (the pipelined, the packed and the 32-row
 *                            kernel walk blocked, the pipelined and the 32-row kernel take order 0)
 *                            [11] nkw  [12] ndcol  [13] nsplit  [14] gps (groups per split)  [15] groups of the last split
 *                            [16] live splits (waves) of the last workgroup  [17] G (groups)
 *   NRM_BWD_LAUNCH_DP        [1] NT  [2] nchunks  [3] kchunks  [4] steps  [5] workgroups  [6] most steps one workgroup walks
 *                            [7] most (row block, N-chunk) items one workgroup walks
 *   NRM_BWD_LAUNCH_RW        [1] NG  [2] mma  [3] EXACT  [4] nks (reduction slices)  [5] workgroups  [6] waves per workgroup  [7] tsplit
 *                            [8] tasks (of one slice)  [9] rounds: trips of the busiest wave's task loop  [10] plain_dh (no dh atomics)
 * Returns 0, or -1 with nrm_last_error() set ("nrm_pwattn_bwd_plan: ...") for arguments the launch entries refuse by value. */
#define NRM_PWATTN_BWD_PLAN_LEN 18
#define NRM_BWD_LAUNCH_DZ 0
#define NRM_BWD_LAUNCH_CONTRACT 1
#define NRM_BWD_LAUNCH_DP 2
#define NRM_BWD_LAUNCH_RW 3
int nrm_pwattn_bwd_plan(int launch, int B, int T, int H, int D, int pass, int mma, int dz_format, int cus, int* out);
/* backward, step 2 in the "resident W_p" form (bf16 arithmetics, D <= 256): the same dt / dh as above from ONE contraction
 * dP = dz W_p whose W_p image stays in LDS and whose dz operand (NRM_DZ_HL4) is read exactly once; autograd of
 * models/attention_model.py:81-92 w.r.t. target and history.  nrm_pwattn_bwd_rw_supported: 1 if (D, mma) has this form;
 * packed: nrm_pwattn_bwd_rw_packed_floats floats filled by nrm_pwattn_bwd_rw_pack from fc1_weight [D, 4D] (row stride ld). */
int nrm_pwattn_bwd_rw_supported(int D, int mma);
long nrm_pwattn_bwd_rw_packed_floats(int D, int mma);
int nrm_pwattn_bwd_rw_pack(const float* fc1_weight, int ld, int D, int mma, float* packed, nrm_stream_t stream);
int nrm_pwattn_bwd_rw_dtdh(const float* dz_hl4, const float* t, const float* h, const float* packed, float* dt, float* dh,
                           int B, int T, int H, int D, int mma, nrm_stream_t stream);

/* backward, step 2 in the "dP walk" form (fp32, D % 4 == 0, H >= 16): the same dt / dh as nrm_pwattn_bwd_contract passes 1 + 2
 * from ONE contraction dP = dz W_p with the forward's streaming skeleton (dz fp32, read once per 208-column chunk of d); the
 * caller then takes dW_p from nrm_pwattn_bwd_contract with passes = 4.  Autograd of models/attention_model.py:81-92 w.r.t.
 * target and history.  nrm_pwattn_bwd_dp_supported: 1 if (D, H) has this form;
 * packed: nrm_pwattn_bwd_dp_packed_floats floats filled by nrm_pwattn_bwd_dp_pack from fc1_weight [D, 4D] (row stride ld).
 * dt / dh are accumulated into (float atomics). */
int nrm_pwattn_bwd_dp_supported(int D, int H);
long nrm_pwattn_bwd_dp_packed_floats(int D, int H);
int nrm_pwattn_bwd_dp_pack(const float* fc1_weight, int ld, int D, int H, float* packed, nrm_stream_t stream);
int nrm_pwattn_bwd_dp_dtdh(const float* dz, const float* t, const float* h, const float* packed, float* dt, float* dh,
                           int B, int T, int H, int D, nrm_stream_t stream);

/* ---- dense layers: reference MLP.forward (models/attention_model.py:29-32: fc1 -> GELU -> fc2), the history
 *      projection w1 (models/user_invariant_interest_model.py:78) and the attention's side projections.
 * Weights are re-packed per call into the kernel's streaming layout (they change every optimizer step).
 * All activation matrices are row-major with a leading dimension that is a multiple of 4 floats and 16-byte
 * aligned rows.  Padding columns [ncols, ld): those of x (nrm_gemm_nt) and of A / B (nrm_gemm_tn) are never used and may hold
 * anything, NaN included; those of m (NRM_EPI_MUL) and of the saved z (NRM_EPI_DGELU) are multiplied by an exact zero and must hold
 * finite values.  The library writes zeros to the columns [N, pad) of y and of the z it stores, pad = min(ld, N rounded up to 16):
 * +0.0, except that y takes the sign of the factor there (0 * m, 0 * gelu'(z)) under NRM_EPI_MUL and NRM_EPI_DGELU; columns
 * from pad on are not touched.  Rows >= M are not touched.                                                    */
#define NRM_EPI_BIAS 0   /* y = x W^T + bias                                                              */
#define NRM_EPI_GELU 1   /* z = x W^T + bias (saved for backward), y = gelu(z)                            */
#define NRM_EPI_DGELU 2  /* y = (x W^T) * gelu'(z)      (z = pre-activation saved by NRM_EPI_GELU)        */
#define NRM_EPI_MUL 3    /* z = x W^T + bias (kept for backward), y = z * m: the gate of user_model.py:33 */
/* mma: the arithmetic the packed image is for (NRM_MMA_F32: the fp32 streaming layout of gemm_nt; NRM_MMA_BF16 / _BF16X3: bf16
 * hi [+ lo] MFMA fragments).  Dense layers on the bf16 matrix cores (BASELINE config 2) keep fp32 accumulation, bias, GELU and
 * column sums; nrm_gemm_nt_bf16_supported says whether a reduction width K fits the resident-row form (else use NRM_MMA_F32). */
long nrm_gemm_packed_floats(int nrows, int ncols, int mma);
int nrm_gemm_nt_bf16_supported(int M, int K, int mma);
/* Which kernel a launch of nrm_gemm_nt(M, N, K, mma) takes (additive entry point, the ABI version is unchanged): the selection of
 * the launch itself, without any device call, with the environment knobs applied as the launch applies them (NRM_RX_BM at every
 * call; NRM_NT_SMALLM, NRM_NT_NARROW and NRM_RX_MIN_WGS as latched at their first use in the process).
 *   NRM_MMA_F32:            NT | MT << 8 | WPE << 16 | KC << 24   of gemm_nt_kernel<NT, MT, EPI, WPE>: NT 16-column tiles per
 *                           N-chunk, MT 16-row tiles per wave (a workgroup holds 64 * MT rows), WPE waves per SIMD the kernel is built
 *                           for, KC 16-wide K-chunks per LDS stage (always 1: the deeper stages are gone, the byte keeps its place)
 *   NRM_MMA_BF16 / _BF16X3: RT | G << 8   of gemm_nt_rx_kernel<RT, MMA, EPI, G>: 16 * RT resident rows per workgroup, weight
 *                           fragments in groups of G reduction chunks; 0 where nrm_gemm_nt_bf16_supported is 0
 * -1: bad arguments (M, N or K <= 0, unknown mma). */
int nrm_gemm_nt_form(int M, int N, int K, int mma);
/* packs the logical [nrows x ncols] matrix src[r*row_stride + c*col_stride]; rows become output columns of
 * nrm_gemm_nt, columns its reduction index.  Linear.forward: (W[N,K], K, 1, N, K); dX = dY W: (W, 1, K, K, N) */
int nrm_gemm_pack(const float* src, long row_stride, long col_stride, int nrows, int ncols, float* packed,
                  nrm_stream_t stream);
/* the same for n matrices in ONE launch (descs is a HOST array, copied into the kernel arguments): what a training loop
 * calls once per optimizer step for every Linear in both GEMM orientations instead of once per GEMM.  With src2 != NULL the
 * packed matrix is src + sign2 * src2 (same strides): the attention's side projections W_h - W_d and W_t + W_d
 * (reference models/attention_model.py:81-86, re-associated) are formed here. */
typedef struct {
    const float* src; const float* src2; float sign2;
    long row_stride, col_stride; int nrows, ncols;
    float* packed;           /* nrm_gemm_packed_floats(nrows, ncols, mma) floats */
    int mma;                 /* NRM_MMA_*: layout of the packed image */
} nrm_pack_desc;
int nrm_gemm_pack_multi(const nrm_pack_desc* descs, int n, nrm_stream_t stream);
/* y[M, N] (ld ldy) = epilogue( x[M, K] (ld ldx) * packed^T ), bias [N] or NULL; m [M, N] (ld ldm) for NRM_EPI_MUL */
int nrm_gemm_nt(const float* x, int ldx, int M, const float* packed, int N, int K, const float* bias,
                float* y, int ldy, float* z, int ldz, const float* m, int ldm, int epilogue, int mma, nrm_stream_t stream);
/* C[i,j] = sum_r A[r,i] B[r,j]  (dW = dY^T X): writes nsplit TRANSPOSED partial slabs ws[s][j][ldws] and, if
 * colsum != NULL, colsum[s][i] = sum_r A[r,i] (the bias gradient); sum over s.  ldws % 4 == 0, ldws >= ncols_i */
int nrm_gemm_tn_nsplit(int ncols_i, int ncols_j, int R, int mma);
/* The whole plan of that launch (additive entry point, the ABI version is unchanged), without any device call and with NRM_TN_WAVES
 * (read at every call) and NRM_TN_SHAPES (latched) applied as the launch applies them: returns nsplit, and through the non-NULL
 * pointers the wave tile (*kt x *dt MFMA tiles of 16 columns of i / of j) and the rows of a split -- split s sums the rows
 * [s * rows_per_split, min(R, (s + 1) * rows_per_split)) into slab s.  -1: bad arguments (a width or R <= 0, unknown mma). */
int nrm_gemm_tn_plan(int ncols_i, int ncols_j, int R, int mma, int* kt, int* dt, int* rows_per_split);
/* zero_out (optional, 16-byte aligned): zero_n floats there are set to 0 by the same launch -- the gradient buffer that
 * nrm_slab_reduce will then add the slabs to */
int nrm_gemm_tn(const float* A, int lda, int ncols_i, const float* B, int ldb, int ncols_j, int R,
                float* ws, int ldws, float* colsum, float* zero_out, long zero_n, int mma, nrm_stream_t stream);

/* the split slabs ws[s][j][ldws] of nrm_gemm_tn / nrm_pwattn_bwd_contract summed over s and ADDED (float atomics; the
 * caller zero-initialises, or accumulates on purpose) where the gradient lives:
 *     out[i*out_istride + j*out_jstride] += sum_s ws[s][j][i]      (i < ni, j < nj)
 * (nj, 1) strides give C[i,j] row-major, i.e. the transpose of a slab; (ld, 1) with an offset pointer a column block of a
 * wider matrix.  out2 (optional) += sign2 * the same value -- the (t - h) block of fc1's gradient
 * (attention_model.py:81-86) is da_t - da_h.  vec [nsplit][ldws] (optional, the colsum slabs of nrm_gemm_tn):
 * vec_out[i] = sum_s vec[s][i]  (the bias gradient; stored, not added). */
int nrm_slab_reduce(const float* ws, int nsplit, int nj, int ldws, int ni, float* out, long out_istride, long out_jstride,
                    float* out2, long out2_istride, long out2_jstride, float sign2,
                    const float* vec, float* vec_out, nrm_stream_t stream);
/* n slab sets in ONE launch (entries as the arguments of nrm_slab_reduce): the 14 reductions of a training step are small,
 * latency-bound launches that depend on nothing but their own slabs, so a caller may defer them and flush them together
 * before the optimizer reads the gradients (reference: autograd's per-parameter accumulation behind train.py:73). */
typedef struct nrm_slab_desc {
    const float* ws; int nsplit, nj, ldws, ni;
    float* out; long out_istride, out_jstride;
    float* out2; long out2_istride, out2_jstride; float sign2;
    const float* vec; float* vec_out;
} nrm_slab_desc;
int nrm_slab_reduce_multi(const nrm_slab_desc* descs, int n, nrm_stream_t stream);

/* ---- head fold (additive entry points, the ABI version is unchanged; reference models/user_model.py:34, out_mlp(mlp(gated))): mlp.fc2 (w_m2 [Q, R], b_m2 [Q]) feeds out_mlp.fc1
 * (w_o1 [P, Q], b_o1 [P]) with no nonlinearity in between, so  z2 = a1 W'^T + b',  W' = w_o1 w_m2 [P, R],  b' = w_o1 b_m2 + b_o1.
 * nrm_head_fold forms W' on the fp32 MFMA pipe and writes it straight into nrm_gemm_nt's packed layout in both orientations:
 * packed_fwd = the image of W' (nrm_gemm_packed_floats(P, R, NRM_MMA_F32) floats: z2 = nrm_gemm_nt(a1, packed_fwd, N = P, K = R)),
 * packed_bwd = the image of W'^T (nrm_gemm_packed_floats(R, P, ...): da1 = nrm_gemm_nt(dz2, packed_bwd, N = R, K = P)), and
 * bias = b' [P].  The weights are contiguous, Q % 4 == 0, w_o1 16-byte aligned; b_o1 / b_m2 may be NULL. */
int nrm_head_fold(const float* w_o1, const float* b_o1, const float* w_m2, const float* b_m2, int P, int Q, int R,
                  float* packed_fwd, float* packed_bwd, float* bias, nrm_stream_t stream);
/* the gradients of the four folded tensors from the (reduced) dwp = dz2^T a1 [P, ldp] and dbp = colsum(dz2) [P]:
 * dw_o1 = dwp w_m2^T + dbp (x) b_m2 [P, Q] (out_mlp.fc1 saw mlp.fc2's output including its bias; b_m2 may be NULL),
 * dw_m2 = w_o1^T dwp [Q, R], db_o1 = dbp, db_m2 = w_o1^T dbp [Q]; contiguous outputs, overwritten; a NULL output is not computed.
 * ldp % 4 == 0, 16-byte aligned rows. */
int nrm_head_fold_bwd(const float* dwp, int ldp, const float* dbp, const float* w_o1, const float* w_m2, const float* b_m2,
                      int P, int Q, int R, float* dw_o1, float* dw_m2, float* db_o1, float* db_m2, nrm_stream_t stream);

/* ---- BatchNorm1d over rows (reference models/user_model.py:18,32), N % 4 == 0, ld % 4 == 0.
 * nrm_colreduce mode 0: s0 += sum_r x;  1: s0 += sum_r (x-mean)^2;  2: s0 += sum_r dy, s1 += sum_r dy*(x-mean)*rstd */
int nrm_colreduce(int mode, const float* x, const float* dy, const float* mean, const float* rstd,
                  float* s0, float* s1, int R, int N, int ld, nrm_stream_t stream);
/* between the reductions (train mode): stage 0: out = mean = s/R, running = (1-momentum) running + momentum mean;
 * stage 1: var = s/R, out = rstd = 1/sqrt(var + eps), running = (1-momentum) running + momentum var R/(R-1).
 * running may be NULL. */
int nrm_bn_finalize(int stage, const float* s, float* out, float* running, int R, int N, float momentum, float eps,
                    nrm_stream_t stream);
/* backward of the gate product y = g * e (models/user_model.py:33): dg = dy * e, de = dy * g; [R, N], N % 4 == 0 */
int nrm_mul_bwd(const float* dy, int lddy, const float* g, int ldg, const float* e, int lde, float* dg, float* de, int ldo,
                int R, int N, nrm_stream_t stream);
int nrm_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                 float* y, int R, int N, int ld, nrm_stream_t stream);
/* training != 0: dx = gamma*rstd*(dy - s0/R - xhat*s1/R) with s0,s1 from nrm_colreduce mode 2; else gamma*rstd*dy.
 * add (optional, same [R, ld] layout) is added to dx: the gradient the rows receive from their second consumer, the gate
 * product of user_model.py:33, joins here instead of in a separate elementwise pass. */
int nrm_bn_backward(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                    const float* s0, const float* s1, const float* add, float* dx, int R, int N, int ld, int training,
                    nrm_stream_t stream);
/* out[R, ldo] = cat(parts, dim=1) in one launch (reference models/user_model.py:31 cat[eu_H, eu_L, ec],
 * user_invariant_interest_model.py:81,88): n <= 8 row-major sources srcs[i] [R, widths[i]] with leading dimension lds[i]
 * (HOST arrays, copied into the kernel arguments) */
int nrm_concat_cols(const float* const* srcs, const long* lds, const int* widths, int n, float* out, int ldo, long R,
                    nrm_stream_t stream);

/* ---- weighted pool (reference models/user_invariant_interest_model.py:86-87, no softmax, no mask)
 * out[b,i,:] (+)= sum_j W[b,i,j] * X[b,j,:]   W element (b,i,j) at W[b*wsb + i*wsi + j*wsj]; X [B,J,D] with row stride ldx
 * (>= D: a column block of a wider matrix, e.g. the head gradient's pooled slice); out [B,I,D] contiguous.
 * forward: W = scores [B,T,H], X = history;  d history: W = scores^T (wsi=1, wsj=H), X = d pooled, accumulate = 1 adds onto
 * the history gradient the attention backward has already written */
int nrm_pool_bmm(const float* W, long wsb, long wsi, long wsj, const float* X, int ldx, float* out,
                 int B, int I, int J, int D, int accumulate, nrm_stream_t stream);
/* ds[b,t,h] = sum_d g[b,t,d] * h[b,h,d]   (gradient of the pool w.r.t. the scores); g [B,T,D] with row stride ldg.
 * zero_out / zero_n (optional): zero_n floats at zero_out are cleared by this launch -- the dw2 | db2 accumulators of the
 * nrm_pwattn_bwd_dz call that follows on the same stream (one launch less per attention) */
int nrm_pool_rowdot(const float* g, int ldg, const float* h, float* ds, int B, int T, int H, int D, float* zero_out, int zero_n,
                    nrm_stream_t stream);

/* ---- instant-interest layer (reference models/user_instant_interest_model.py: ReLU(Linear(3 -> 8)) on the popularity scalars
 * of a candidate).  x [R, K] dense, fp32 or fp64; weight [N, K]; K <= 4, N <= 8.
 * forward: y [R, ldy] = ReLU(x W^T + b), columns N..ldy-1 written as 0.
 * backward: dwb[n*K + k] += sum_r g[r,n] x[r,k] and dwb[N*K + n] += sum_r g[r,n] with g = dy (row stride lddy) where the
 * pre-activation is positive (recomputed from x); dwb (N*K + N floats) must be initialised; x has no gradient. */
int nrm_small_linear_relu_fwd(const void* x, int x_is_f64, const float* weight, const float* bias, float* y, long R, int K, int N, int ldy,
                              nrm_stream_t stream);
int nrm_small_linear_relu_bwd(const void* x, int x_is_f64, const float* weight, const float* bias, const float* dy, int lddy, long R,
                              int K, int N, float* dwb, nrm_stream_t stream);

/* ---- loss (reference models/user_model.py:37-43): (1-alpha)*BCE(softmax_T(out), y) + alpha*BCE(softmax_T(out +
 * delta[id]), y), mean over B*T, log clamped at -100.  Writes loss_sum[0] += loss, dout [B,T] = dL/dout and
 * ddelta[id[b]] += dL/ddelta (loss_sum and ddelta must be zero-initialised).  Any T >= 1 (a lane
 * keeps its candidates in registers up to T = 256 and re-reads the row beyond).  delta has n_delta entries;
 * a negative id counts from the end as in torch indexing, an id still outside [0, n_delta) is clamped and sets
 * err[0] = 1 (the reference raises IndexError at user_model.py:40; never an out-of-bounds access here).
 * out_stride / dout_stride: floats between consecutive (b, t) entries -- 1 for dense [B,T]; 4 for the single column of a
 * zero-padded [B*T, 4] matrix (the layout the logit GEMM writes and the GEMM consuming dout reads; dout then gets (g,0,0,0)).
 * label: [B,T] dense, fp32 or (label_is_f64) fp64 as the reference's DataLoader yields it. */
int nrm_loss_fwd_bwd(const float* out, int out_stride, const void* label, int label_is_f64, const long* user_id, const float* delta,
                     long n_delta, float alpha, int B, int T, float* loss_sum, float* dout, int dout_stride, float* ddelta, int* err,
                     nrm_stream_t stream);

/* ---- Adam over one flat fp32 buffer (reference train.py:48,73-75): g += wd*p; m,v update; bias correction for
 * `step` (1-based); p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps); optionally zeroes g (optimizer.zero_grad()).
 * n % 4 == 0, 16-byte aligned buffers. */
int nrm_adam_step(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, int zero_grad, nrm_stream_t stream);
/* n gradient tensors -> their slots of the flat gradient buffer in ONE launch (reference train.py:73-74: what sits between
 * loss.backward() and optimizer.step(); with data parallelism, what the single all-reduce then runs on).  srcs / offsets /
 * counts are HOST arrays (copied into the kernel arguments at call time): flat[offsets[i] .. +counts[i]) = srcs[i][0 ..
 * counts[i]); a NULL source zero-fills its slot.  Contiguous fp32 sources. */
int nrm_gather_flat(const float* const* srcs, const long* offsets, const long* counts, int n, float* flat, long flat_n,
                    nrm_stream_t stream);
/* the same with the step counter on the device (state = float[4]: {step, 1-beta1^step, sqrt(1-beta2^step), -},
 * zero-initialised by the caller, advanced by the call): safe to capture in a hipGraph and replay */
int nrm_adam_step_dev(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float* state, int zero_grad, nrm_stream_t stream);

/* ---- embedding front end: reference models/user_invariant_interest_model.py:50-71,74-79 (slice_x,
 * feature_embedding, time_embedding).  x: [nrows, xcols] packed rows (tool/process_data.py:198-240), fp64
 * (x_is_f64 != 0) or fp32: [year,month,day,hour | text_img P | category | sub-category x n_sub | sentiment x3 |
 * type | (behaviour != 0: read_time, scroll)].  Writes the label rows lab[nrows, ldlab] = [Emb_cat(cat)+mean
 * Emb_cat(sub) e0 | ReLU(W_s s + b_s) e1 | Emb_type e2 | sum of 4 time embeddings e3 | (read_time, scroll)] zero
 * padded to ldlab, and the text/image block ti[nrows, ldti] as fp32.  err[0] is set to 1 on an out-of-range index
 * (the index is clamped; the reference raises IndexError). */
int nrm_frontend_fwd(const void* x, int x_is_f64, int nrows, int xcols, int P, int n_sub, int behaviour,
                     const float* cat_tab, int n_cat, int e0, const float* sen_w, const float* sen_b, int e1,
                     const float* type_tab, int n_type, int e2,
                     const float* year_tab, const float* month_tab, const float* day_tab, const float* hour_tab,
                     int n_year, int n_month, int n_day, int n_hour, int e3,
                     float* lab, int ldlab, float* ti, int ldti, int* err, nrm_stream_t stream);
/* backward of the label rows: accumulates (+=, float atomics) the table / sentiment-layer gradients.  d_cat_tab may be NULL:
 * the category-table gradient is then left to nrm_frontend_cat_grad.  The seven other gradient pointers may be NULL together
 * (d_cat_tab is then required): the small tables are left to nrm_frontend_bwd_tables */
int nrm_frontend_bwd(const void* x, int x_is_f64, int nrows, int xcols, int P, int n_sub, int behaviour,
                     const float* dlab, int lddl, const float* sen_w, const float* sen_b,
                     int n_cat, int e0, int e1, int n_type, int e2, int n_year, int n_month, int n_day, int n_hour, int e3,
                     float* d_cat_tab, float* d_sen_w, float* d_sen_b, float* d_type_tab,
                     float* d_year_tab, float* d_month_tab, float* d_day_tab, float* d_hour_tab, nrm_stream_t stream);

/* gradients of the small tables (type, year, month, day, hour) and of the sentiment layer for up to two row sets (nrows = 0 skips
 * one; both have the element type x_is_f64) as a one-hot contraction on v_mfma_f32_16x16x4_f32: a persistent launch whose
 * workgroups store partial tables to ws, and a second kernel that adds them to the gradients (+=) in a fixed order, so the result
 * is bitwise the same from run to run.  Non-finite gradient elements and rows with a non-finite sentiment scalar reach exactly the
 * cells they reach in nrm_frontend_bwd (by float atomics).  ws: nrm_frontend_tables_ws_floats(nrows0 + nrows1, ...) floats; that
 * function returns 0 for a shape these kernels do not take (more than 128 accumulator tiles of 16 x 16, or a staged block beyond
 * 64 KB of LDS): such a shape goes to nrm_frontend_bwd. */
long nrm_frontend_tables_ws_floats(long nrows_total, int n_sub, int e1, int n_type, int e2, int n_year, int n_month, int n_day, int n_hour, int e3);
int nrm_frontend_bwd_tables(const void* x0, int nrows0, int xcols0, int behaviour0, const float* dlab0, int lddl0,
                            const void* x1, int nrows1, int xcols1, int behaviour1, const float* dlab1, int lddl1, int x_is_f64,
                            int P, int n_sub, const float* sen_w, const float* sen_b,
                            int e0, int e1, int n_type, int e2, int n_year, int n_month, int n_day, int n_hour, int e3,
                            float* d_sen_w, float* d_sen_b, float* d_type_tab,
                            float* d_year_tab, float* d_month_tab, float* d_day_tab, float* d_hour_tab, float* ws, nrm_stream_t stream);

/* category-table gradient of up to two row sets (history rows, candidate rows; nrows = 0 skips one) by a counting sort of the
 * (row, slot) references by category id and a gather-sum over runs of equal ids -- instead of (1 + n_sub) * e0 float atomics per
 * row.  d_cat_tab [n_cat, e0] is accumulated into (+=).  ws: nrm_frontend_cat_ws_ints(n_cat, nrows0 + nrows1, n_sub) int32 of
 * scratch.  Both row sets have the same element type (x_is_f64).  Summation order inside an id varies from run to run.  Up to
 * 16384 ids the sort histograms and places the references in LDS, slice by slice, with no global atomic per reference.
 * ws holds, with nref = (nrows0 + nrows1) * (n_sub + 1): [3 n_cat + 4 counters | nref category ids in reference order | refs:
 * the nref references (row * (n_sub + 1) + slot, set 1 after set 0) sorted by id | refcat: their ids | per-slice histograms]. */
long nrm_frontend_cat_ws_ints(int n_cat, long nrows_total, int n_sub);
int nrm_frontend_cat_grad(const void* x0, int nrows0, int xcols0, const float* dlab0, int lddl0,
                          const void* x1, int nrows1, int xcols1, const float* dlab1, int lddl1, int x_is_f64,
                          int P, int n_sub, int n_cat, int e0, float* d_cat_tab, int* ws, nrm_stream_t stream);

/* ---- per-impression ROC-AUC and top-1 hit (reference train.py:77-80, verify.py:25-36, tool/evaluation.py:3-5;
 * sklearn roc_auc_score for binary labels = Mann-Whitney U with ties counted 1/2).  score, label [B,T]; len [B]
 * (int32, candidates that count per row, NULL = T).  auc[b] = -1 where a row holds a single class. */
int nrm_row_auc(const float* score, const float* label, const int* len, int B, int T, float* auc, int* top1,
                nrm_stream_t stream);

/* ---- scoring tail of a test set (reference test.py:58-70 model_test, :118-126 get_string_of_prediction), one launch:
 *   p_m = softmax over ALL T columns of model m's logits (padding columns included, as in the reference), out = mean over the
 *   M models (summed in model order), score = softmax(out[0:n]) on rows with n < T and out otherwise, where
 *   n = clamp(T - empty[b], 0, T); rank[j] = 1 + #{i < n: score[i] > score[j]} + #{i < j: score[i] == score[j]} -- the 1-based
 *   position a stable descending sort gives.  Columns j >= n get score 0 and rank 0 (a row with n = 0 is all zeros; ATen's
 *   softmax of an all-masked row gives NaN there).  live[b] = n.
 * logits / row_stride / col_stride: HOST arrays of M (1 .. 8) entries: device pointer of each model's [B, T] fp32 logits, its row
 *   stride and its column stride in floats (col_stride NULL = 1 everywhere; the models' own logits are column 0 of a padded
 *   [B*T, 4] GEMM output, column stride 4).  The pointers travel to the kernel by value: nothing is stacked or copied.
 * empty [B] int32 (trailing padding candidates per row after the caller's common trim; NULL = 0 everywhere).
 * label [B, T] fp32 and metrics [B, 3] fp32 are NULL together.  With y = label > 0.5 over the live columns, metrics[b] =
 *   (rr, ndcg5, ndcg10): rr = (sum y / rank) / sum y, ndcg_k = (sum over rank <= k of y / log2(1 + rank)) / (sum over
 *   r = 1 .. min(k, n_pos) of 1 / log2(1 + r)); all three are -1 where the row has no live positive.  (Sums in fp64, stored as fp32.)
 * score [B, T] fp32, rank [B, T] int32, live [B] int32, all dense.  1 <= T <= nrm_ensemble_rank_max_candidates() (>= 1024); B = 0 is a
 * no-op.  Rows are independent: a NaN / Inf in one row's logits stays in that row's outputs. */
int nrm_ensemble_rank_max_candidates(void);
int nrm_ensemble_rank(const float* const* logits, const long* row_stride, const long* col_stride, int M, const int* empty,
                      const float* label, int B, int T, float* score, int* rank, int* live, float* metrics, nrm_stream_t stream);

/* ---- compact scoring path (inference only; additive entry points, the ABI version is unchanged).
 * A processed test set pads every candidate list with all-zero rows to the longest list of the data set.  All padded candidates of
 * one impression have the same inputs, hence the same logit, so an impression with n live candidates that keeps e' padded columns
 * after the batch's common trim needs n + [e' > 0] forward rows instead of T' = n + e': the live ones and ONE representative padded
 * candidate whose exp enters the first softmax e' times.  Tables (int32, device): cand_off [B + 1] prefix sums of the rows per
 * impression, cand_imp [N] impression of each compact row, pad_mult [B] = e'.  The kernels clamp table entries to the arrays.
 *
 * nrm_compact_gather: copies the N rows (b, t), t < n_b + [e'_b > 0], of x_target [B, T, target_cols] and x_global
 *   [B, T, global_cols] (each float64 or float32, as its *_is_f64 says) into xt_compact [N, target_cols] and xg_compact [N, global_cols], and
 *   compares every other kept padded column t in (n_b, T - trim) bitwise with the representative column n_b; a difference, or tables
 *   with n_b + e'_b != T - trim, sets *flag = 1 (flag: host-visible int32, written in the error case only).  The trimmed columns
 *   are not read.
 * nrm_pwattn_fwd_ragged: nrm_pwattn_fwd without a z store for candidate rows t, v [N, D] (row c belongs to impression cand_imp[c]),
 *   history rows h, u [B, H, D], scores s [N, H].  fp32 arithmetic only: mma other than NRM_MMA_F32 is refused.  max_count = the
 *   longest list (max over b of cand_off[b + 1] - cand_off[b]).
 * nrm_pool_bmm_ragged: out[c, :] = sum_j s[c, j] h[cand_imp[c], j, :] for s [N, H], h [B, H, D], out [N, D].  List b is the rows
 *   c0_b .. c1_b - 1 with c0_b = clamp(cand_off[b], 0, N) and c1_b = clamp(cand_off[b + 1], c0_b, N); max_count is the longest list.
 *   The entry WRITES exactly the rows of the lists (two lists must not own the same row) and LEAVES every other row of out as it
 *   was: the rows before the first list and behind the last one.  (Should max_count be smaller than a list, that list's rows from
 *   max_count on are either written or left.)  The planners of compact.py give every row to a list: no row of `pooled` is left.
 * nrm_ensemble_rank_ragged: nrm_ensemble_rank for compact logits: model m's entry c lies at logits[m][c * col_stride[m]]
 *   (col_stride NULL = 1); impression b owns the entries cand_off[b] .. cand_off[b + 1] - 1, the last of which stands for pad_mult[b]
 *   padded columns where pad_mult[b] > 0:
 *     p_j = exp(l_j - mx) / (sum over live i of exp(l_i - mx) + e' exp(l_pad - mx)),  mx = max over the live and the pad logit,
 *   then the mean over the models, the second softmax over the live values where e' > 0, rank and metrics exactly as
 *   nrm_ensemble_rank, written to the SAME dense outputs score / rank [B, T] (0 on padding columns), live [B], metrics [B, 3]. */
int nrm_compact_gather(const void* x_target, int target_cols, int target_is_f64, const void* x_global, int global_cols, int global_is_f64,
                       const int* cand_off, const int* pad_mult, int B, int T, int trim, int N,
                       void* xt_compact, void* xg_compact, int* flag, nrm_stream_t stream);
int nrm_pwattn_fwd_ragged(const float* t, const float* h, const float* u, const float* v, const float* packed_wp,
                          const float* w2, const float* b2, float* s, const int* cand_imp, const int* cand_off,
                          int B, int N, int max_count, int H, int D, int mma, nrm_stream_t stream);
int nrm_pool_bmm_ragged(const float* s, const float* h, float* out, const int* cand_off, int B, int N, int max_count, int H, int D,
                        nrm_stream_t stream);
int nrm_ensemble_rank_ragged(const float* const* logits, const long* col_stride, int M, const int* cand_off, const int* pad_mult, int N,
                             const float* label, int B, int T, float* score, int* rank, int* live, float* metrics, nrm_stream_t stream);

/* ---- history compaction (inference): the compact scoring path, ragged in the history too
 * The reference's ETL writes every history as history_max_num rows and leaves the rows past the user's own all-zero; the model does
 * not mask them (user_invariant_interest_model.py:77-78, 83-87: they are scored and pooled like any other row).  With
 * L_b = 1 + the last history row of impression b that holds any non-zero bit, the rows j >= L_b have the same front-end row, the same
 * u row and, for any candidate c, the same score, so K_b = L_b + [L_b < H] rows are kept -- the live ones and ONE representative
 * padded row -- and pooled[c, :] = sum_{j < L_b} s[c, j] h[b, j, :] + (H - L_b) s[c, L_b] h[b, L_b, :].  Tables (int32, device):
 * hist_off [B + 1] prefix sums of K_b, hist_mult [B] = H - L_b, tile_pre [B + 1] prefix sums of count_b ceil(K_b / 16) (count_b =
 * cand_off[b + 1] - cand_off[b]); the scores of a compact candidate are ceil(K_b / 16) whole 16-row tiles of s [16 Mt], Mt = tile_pre[B].
 * Every entry replaces work of user_invariant_interest_model.py:77-78, 83-87 on the padded rows.  Table entries are clamped to the arrays.
 *
 * nrm_history_len: hist_len[b] = L_b of x_history [B, H, cols] (float64 or float32, read as the front end reads them).  The test is
 *   bitwise: a row holding -0.0 or a NaN is live, and an all-zero row below a live one is kept.  One pass; clears hist_len first.
 * nrm_history_gather: xh_compact[hist_off[b] + j, :] = x_history[b, j, :] for j < K_b (bitwise); R = hist_off[B], k_max = max K_b.
 * nrm_history_tiles: tile_tab [Mt] x 4 int32 (16-byte aligned) = per score tile {compact candidate, first row of the tile in h / u,
 *   valid rows of the tile, impression}; built on the device from the [B + 1] tables, one thread per candidate.
 * nrm_pwattn_fwd_hragged: nrm_pwattn_fwd_ragged for history rows h, u [R, D] and scores s [16 Mt]; rows of a tile past its valid ones
 *   are written as 0.  fp32 arithmetic only: mma other than NRM_MMA_F32 is refused.
 * nrm_pool_bmm_hragged: out[c, :] = sum_{j < K_b} w_j s[c, j] h[hist_off[b] + j, :], w_j = 1 except w_{K_b - 1} = hist_mult[b] where
 *   hist_mult[b] > 0; s is read, never changed.  With the lists of nrm_pool_bmm_ragged, r0_b = clamp(hist_off[b], 0, R), K_b =
 *   clamp(hist_off[b + 1], r0_b, R) - r0_b, nt_b = ceil(K_b / 16) and t0_b = clamp(tile_pre[b], 0, Mt), the scores of candidate i of list b
 *   are s[16 (t0_b + i nt_b) + j], j < K_b (the columns K_b .. 16 nt_b of its tiles are not read), and the entry WRITES the first
 *   min(c1_b - c0_b, floor((Mt - t0_b) / nt_b)) rows of every list with K_b >= 1: never past the scores there are.  It LEAVES as they
 *   were the rows of a list with K_b = 0, the rows a list is cut short of, and the rows no list owns.  build_plan keeps K_b >= 1
 *   wherever H >= 1 and its tile_pre holds every candidate's tiles, so ops.attend_pool_hragged_fwd returns no unwritten row.
 *   B is not limited to 65535 as in the dense pool entries: the launch is a one-dimensional grid of (impression, slab, row group)
 *   tasks and refuses only a task count past 2^31 workgroups. */
int nrm_history_len(const void* x_history, int cols, int is_f64, int B, int H, int* hist_len, nrm_stream_t stream);
int nrm_history_gather(const void* x_history, int cols, int is_f64, const int* hist_off, int B, int H, int R, int k_max, void* xh_compact,
                       nrm_stream_t stream);
int nrm_history_tiles(const int* cand_imp, const int* cand_off, const int* hist_off, const int* tile_pre, int B, int N, int R, int Mt,
                      void* tile_tab, nrm_stream_t stream);
int nrm_pwattn_fwd_hragged(const float* t, const float* h, const float* u, const float* v, const float* packed_wp,
                           const float* w2, const float* b2, float* s, const int* cand_imp, const int* cand_off, const int* hist_off,
                           const int* tile_pre, const void* tile_tab, int B, int N, int max_count, int R, int Mt, int k_max, int D, int mma,
                           nrm_stream_t stream);
int nrm_pool_bmm_hragged(const float* s, const float* h, float* out, const int* cand_off, const int* hist_off, const int* hist_mult,
                         const int* tile_pre, int B, int N, int max_count, int R, int Mt, int k_max, int D, nrm_stream_t stream);

/* Which kernel a launch of nrm_pwattn_fwd / _fwd_ragged / _fwd_hragged takes (additive entry point, the ABI version is unchanged): the
 * answer of the selector the launches themselves switch on, without a kernel launch or an allocation, with the environment knobs applied
 * as the launches apply them (NRM_FWD_CT, NRM_FWD_WALK_F32 and NRM_FWD_TSPLIT at every call; NRM_FWD_WALK as latched at its first use
 * in the process).
 *   ragged = 0: nrm_pwattn_fwd(B, T, H, D, mma) with (save_z = 1) or without a z buffer; N, max_count and k_max are not read.
 *   ragged = 1: nrm_pwattn_fwd_ragged(B, N, max_count, H, D, mma); T is not read.
 *   ragged = 2: nrm_pwattn_fwd_hragged(B, N, max_count, Mt = T, k_max, D, mma): T carries Mt, the number of 16-row score tiles; H is
 *               not read.
 *   cus: compute units of the device the launch would go to; 0: those of the current device, or 256 where there is none.
 * out[NRM_PWATTN_FWD_FORM_LEN]:
 *   [0] valid     0: the selection has no kernel and the launch is refused (a ragged form asked for with bf16 arithmetic or a z store,
 *                 a width the bf16 forward cannot hold)
 *   [1] family    NRM_FWD_STREAM (pwattn_fwd_kernel), NRM_FWD_RW_TILE (pwattn_fwd_rw_kernel), NRM_FWD_WALK_BF16 (pwattn_fwd_walk_kernel),
 *                 NRM_FWD_WALK_F32 (pwattn_fwd_walk_f32_kernel)
 *   [2..6]        NT, MT, WPE, CT, NW of pwattn_fwd_kernel<NT, MT, SAVE_Z, WPE, CT, NW, ..> (NRM_FWD_STREAM; 0 otherwise)
 *   [7], [8]      NTS of the resident forms, KCH of the walks (fp32 walk: KCH = NTS) (0 for NRM_FWD_STREAM)
 *   [9..11]       mma, save_z, ragged as asked
 *   [12] nsplit   column slices of the resident forms whose partial scores are added (1: one slice, no atomics)
 *   [13] tsplit   parts the candidate walk of a task is cut into (walks; 1 otherwise)
 *   [14]          workgroups of the launch
 *   [15] tasks    16-row tiles (NRM_FWD_RW_TILE), walk tasks (impression x 16 history rows x part), workgroups (NRM_FWD_STREAM);
 *                 0: the entry returns without a launch
 *   [16] rounds   ceil(tasks / (workgroups per slice x waves per workgroup)), 16 waves in NRM_FWD_RW_TILE and 8 in the walks: how often
 *                 the busiest wave goes round its persistent loop; 1 for NRM_FWD_STREAM
 *   [17] nchunks  N-chunks the width is streamed in (NRM_FWD_STREAM; 0 otherwise)
 * Returns 0, or -1 with nrm_last_error() set ("nrm_pwattn_fwd_form: ...") for arguments the launch entries refuse by value. */
#define NRM_PWATTN_FWD_FORM_LEN 18
#define NRM_FWD_STREAM 0
#define NRM_FWD_RW_TILE 1
#define NRM_FWD_WALK_BF16 2
#define NRM_FWD_WALK_F32 3
int nrm_pwattn_fwd_form(int B, int T, int H, int D, int mma, int save_z, int ragged, int N, int max_count, int k_max, int cus, int* out);

/* ---- training on compacted histories: length groups through the dense kernels
 * The padded history rows are scored and pooled unmasked in training too (reference models/user_invariant_interest_model.py:77-78,
 * 83-87).  The batch is sorted by history length and cut into G contiguous groups; group g (impressions b0_g .. b0_{g+1} - 1 of the
 * sorted order) is trimmed to H_g <= H rows and runs through the DENSE attention entries above with H = H_g.  Where H_g < H, row
 * H_g - 1 of every impression of the group is a padded row that stands for w_g = H - H_g + 1 equal rows, and only the pool sees it:
 *   pooled[b,t,:] = sum_{j < H_g - 1} s[b,t,j] h[b,j,:] + w_g s[b,t,H_g - 1] h[b,H_g - 1,:]
 *
 * nrm_history_gather_groups: the grouped history arena, xh_arena[row_off[g] + (b - b0_g) H_g + j, :] = x_history[src_imp[b], j, :] for
 *   j < H_g (bitwise, float64 or float32; the sorted x_history is never formed).  Tables (int32, device): src_imp [B] (the sort
 *   permutation), group_b0 [G + 1], group_row_off [G + 1], group_h [G]; R = group_row_off[G]; G <= 64.  One wave per kept row, one launch
 *   for all groups; table entries are clamped to the arrays.  Replaces the padded rows' share of user_invariant_interest_model.py:75-78.
 * nrm_pool_bmm_wlast: nrm_pool_bmm with a weighted last row, wlast >= 1.  wlast_row = 0: the weight is on the reduction index J - 1,
 *   applied where W is read (forward pool, user_invariant_interest_model.py:86-87; W = s stays unweighted in memory).  wlast_row = 1: the
 *   weight is on output row I - 1 and scales only the product formed by this launch, not what `accumulate` finds there (the pool's
 *   history gradient, autograd's backward of :86-87).  wlast = 1 is bitwise nrm_pool_bmm.
 * nrm_pool_rowdot_wlast: nrm_pool_rowdot with ds[b,t,H - 1] = wlast * g[b,t,:] . h[b,H - 1,:] (autograd's backward of :86-87 with respect
 *   to the scores); wlast = 1 is bitwise nrm_pool_rowdot. */
int nrm_history_gather_groups(const void* x_history, int cols, int is_f64, const int* src_imp, const int* group_b0, const int* group_row_off,
                              const int* group_h, int G, int B, int H, int R, void* xh_arena, nrm_stream_t stream);
int nrm_pool_bmm_wlast(const float* W, long wsb, long wsi, long wsj, const float* X, int ldx, float* out,
                       int B, int I, int J, int D, int accumulate, float wlast, int wlast_row, nrm_stream_t stream);
int nrm_pool_rowdot_wlast(const float* g, int ldg, const float* h, float* ds, int B, int T, int H, int D, float* zero_out, int zero_n,
                          float wlast, nrm_stream_t stream);

/* ---- training on compacted candidate lists: row weights for BatchNorm and the loss
 * The training ETL pads every candidate list with all-zero rows (reference tool/process_data.py:214-217, 249-252).  The batch is sorted by
 * n_b = T - empty_b and cut into G contiguous groups; group g keeps T_g = min(T, max n_b + 1) columns.  Where T_g < T, column T_g - 1 of
 * every impression of the group is a padded candidate that stands for w_g = T - T_g + 1 equal ones.  Everything but BatchNorm's batch
 * statistics (models/user_model.py:18,32) and the loss (:37-43) is row-wise in the candidate; those two take the weight.
 *
 * nrm_candidate_gather_groups: the grouped candidate arenas, arena[row_off[g] + (b - b0_g) T_g + t, :] = x[src_imp[b], t, :] for t < T_g, of
 *   x_target [B, T, target_cols], x_global [B, T, global_cols] and label [B, T] (bitwise, float64 or float32 each), and row_weight [N]
 *   (w_g on a group's last column, 1 elsewhere).  Every dropped cell (t >= T_g) is compared bitwise with column T_g - 1 of its impression in
 *   all three tensors; a difference (or tables that place a row outside the arena) sets flag[0] = 1 (the pad-error flag of
 *   nrm_compact_gather).  Tables (int32, device): src_imp [B], group_b0 [G + 1], group_row_off [G + 1], group_t [G]; N = group_row_off[G];
 *   G <= 64.  One wave per cell, one launch for all groups; table entries are clamped to the arrays.
 * nrm_colreduce_roww: nrm_colreduce modes 0 and 1 with a row weight: s0 += sum_r w_r x;  s0 += sum_r w_r (x - mean)^2.  nrm_bn_finalize
 *   then takes R = the rows of the batch (sum_r w_r).  All weights 1 is bitwise nrm_colreduce.
 * nrm_bn_backward_roww: the train-mode nrm_bn_backward with dx_r = gamma rstd (dy_r - w_r s0/n - w_r xhat_r s1/n) + add_r, n = n_rows, the
 *   rows of the batch; s0, s1 are nrm_colreduce mode 2's plain sums over the R rows of the launch (dy carries the weight already).  All
 *   weights 1 with n_rows = R is bitwise nrm_bn_backward.
 * nrm_loss_fwd_bwd_wlast: nrm_loss_fwd_bwd for one group: column T - 1 of every impression counts wlast >= 1 times in both softmax
 *   denominators and both BCE sums, dout[b, T - 1] is the sum over the copies, and the mean is inv_n = 1 / (rows of the batch) -- loss_sum and
 *   ddelta accumulate over one call per group.  wlast = 1 with inv_n = 1 / (B T) is bitwise nrm_loss_fwd_bwd. */
int nrm_candidate_gather_groups(const void* x_target, int target_cols, int target_is_f64, const void* x_global, int global_cols, int global_is_f64,
                                const void* label, int label_is_f64, const int* src_imp, const int* group_b0, const int* group_row_off,
                                const int* group_t, int G, int B, int T, int N, void* xt_arena, void* xg_arena, void* label_arena, float* row_weight,
                                int* flag, nrm_stream_t stream);
int nrm_colreduce_roww(int mode, const float* x, const float* mean, const float* row_weight, float* s0, int R, int N, int ld, nrm_stream_t stream);
int nrm_bn_backward_roww(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma, const float* s0,
                         const float* s1, const float* add, const float* row_weight, float* dx, int R, int n_rows, int N, int ld,
                         nrm_stream_t stream);
int nrm_loss_fwd_bwd_wlast(const float* out, int out_stride, const void* label, int label_is_f64, const long* user_id, const float* delta,
                           long n_delta, float alpha, int B, int T, float wlast, float inv_n, float* loss_sum, float* dout, int dout_stride,
                           float* ddelta, int* err, nrm_stream_t stream);

/* ---- batch assembly from device-resident tables (additive entry point, the ABI version is unchanged)
 * Writes the processed record of reference tool/process_data.py:190-252 (process_dataset's loop body, batch_type 0 and 2) for the B
 * impressions sel[0 .. B) straight from index-based tables, instead of reading it from the host:
 *   x_history [B, H, hc]  row j < min(events of the user, H): [year, month, day, hour of (impression time - event time) | the article's
 *                         static row | read time, scroll]; the rows behind are +0.0          hc = 4 + static_cols + 2
 *   x_target  [B, T, tc]  slot s: [buckets of (impression time - publish time) | static row]   tc = 4 + static_cols
 *   x_global  [B, T, 3]   the article's three normalised counters
 *   label [B, T] float64 (1 where the slot holds the target), label_id [B, T] int64 (the article's id, -1 on an empty slot),
 *   empty_num [B] = empty slots, user_id [B], impression_id [B], history_len [B] int32 = min(events of the user, H)
 * Slots: 0 .. T-2 are the first T-1 in-view entries.  With NRM_ASSEMBLE_KEEP_TARGET_SLOT (batch_type 0) slot T-1 is in-view entry T-1 if
 * one of the first T-1 is the target, else the first entry at position >= T-1 that is the target, else empty; without the flag
 * (batch_type 2) it is entry T-1.  Empty slots are +0.0 rows with label 0.
 * Time buckets (tool/normalization.py sec_norm): sec = max(0, delta_us / 1e6) in float64, then for (365 d, 3000), (30 d, 12), (1 d, 30),
 * (1 h, 23): k = min(int(sec / standard), cap), sec -= standard * k -- float64 arithmetic, once per row.
 * Tables (device): art_static [A, S] rows of S = static_cols rounded up to a multiple of 4 elements, tail zero, 16-byte aligned and below
 * 2^32 bytes; art_global [A, 3]; the floating tables (art_static, art_global, ev_read, ev_scroll) are all float64 (is_f64 != 0) or all
 * float32 and the three x outputs have their type.  user_off [U + 1], imp_off [N + 1] are prefix sums; events of a user lie most recent
 * first.  ev_art, imp_inview, imp_target (-1 = none) index art_*; imp_user indexes user_*.
 * Every table entry is clamped to its array; an entry of sel outside [0, N) is clamped and sets err[0] = 1 (the index flag of
 * nrm_frontend_fwd).  One wave writes 16 rows of one impression in 16-byte units where hc % 4 == 0 (candidate rows, which start 8 bytes
 * off in float32, in 8-byte units) and element by element otherwise; no atomics, the output is the same bit for bit from run to run.
 * B = 0 launches nothing.  H * hc and T * tc elements of one impression stay below 2^31 bytes. */
typedef struct nrm_assemble_tables {
    const void* art_static; const void* art_global; const long* art_pub_us; const long* art_id;
    const long* user_off; const int* ev_art; const long* ev_time_us; const void* ev_read; const void* ev_scroll; const long* user_id;
    const int* imp_user; const long* imp_time_us; const long* imp_off; const int* imp_inview; const int* imp_target; const long* imp_id;
    long A, U, E, N, L;              /* articles, users, events, impressions, in-view entries */
    int S, static_cols, is_f64;
    /* outputs */
    void* x_history; void* x_target; void* x_global; double* label; long* label_id; long* empty_num; long* user_id_out;
    long* impression_id; int* history_len;
    int* err;
} nrm_assemble_tables;
#define NRM_ASSEMBLE_KEEP_TARGET_SLOT 1
int nrm_assemble_batch(const nrm_assemble_tables* tables, const long* sel, int B, int H, int T, int flags, nrm_stream_t stream);
/* the form nrm_assemble_batch writes rows in (the answer of the host function the launch switches on, no device call):
 * 4 = 16-byte units (8-byte units for float32 candidate rows), 1 = element by element; -1: bad arguments */
int nrm_assemble_form(int static_cols, int S);
/* The same kernel reading its impressions at a DEVICE-side cursor (additive; nrm_assemble_tables keeps its layout): impression b of the
 * batch is order[*cursor + b], order [n_order] and cursor [1] on the device.  Nothing of the launch depends on host data but the
 * pointers, so a captured launch assembles another batch at every replay once something on the stream moves the cursor
 * (nrm_epoch_tally).  A position *cursor + b outside [0, n_order) is clamped into the range and sets err[0] = 1 like an entry outside
 * the table: a replay past the end of an epoch writes clamped rows, is reported, and reads nothing outside order.  The cursor is read
 * once per wave (a uniform load), no atomics.  nrm_assemble_batch(sel, B) is the case "no cursor, n_order = B".  n_order >= 1 where
 * B > 0 (and below 2^62). */
int nrm_assemble_batch_at(const nrm_assemble_tables* tables, const long* order, long n_order, const long* cursor, int B, int H, int T,
                          int flags, nrm_stream_t stream);

/* The cursor form writing STRAIGHT INTO THE GROUPED ARENAS of a static group plan (additive, the ABI version is unchanged; DESIGN.md
 * section 5i).  The batch arrives sorted by length (the host sorts every batch's slice of order): place b of the batch belongs to group g
 * with bounds[g] <= b < bounds[g + 1], which keeps h_g[g] <= H history rows and t_g[g] <= T candidate slots per impression.
 *   history row j < h_g[g] of place b  -> row hist_row_off[g] + (b - bounds[g]) * h_g[g] + j of tables->x_history, here [R, hc]
 *   candidate slot s < t_g[g]          -> row cand_row_off[g] + (b - bounds[g]) * t_g[g] + s of tables->x_target [N, tc], tables->x_global
 *                                         [N, 3], label_arena [N] float64 and row_weight [N] fp32 = T - t_g[g] + 1 on slot t_g[g] - 1, else 1
 * -- bit for bit the rows nrm_history_gather_groups / nrm_candidate_gather_groups copy out of nrm_assemble_batch_at's dense tensors with the
 * identity permutation; the dense x tensors are never written.  label [B, T], label_id, empty_num, user_id_out, impression_id and
 * history_len are written as nrm_assemble_batch_at writes them.  A block of 16 history rows at or beyond h_g[g] exits at once.
 * An impression with h_g[g] or more events where h_g[g] < H, or t_g[g] or more live candidates where t_g[g] < T, does not fit its group and
 * sets misfit[0] = 1; its kept rows are written all the same.  The tables (int32, device) are clamped entry by entry, and an impression
 * whose rows would not lie inside [0, R) / [0, N) writes none of them and sets the flag: nothing is written outside the arenas whatever the
 * tables hold.  1 <= G <= 64, R, N >= 1.  Plain vector stores, no atomics. */
typedef struct nrm_assemble_groups {
    const int* bounds; const int* h_g; const int* hist_row_off; const int* t_g; const int* cand_row_off;
    int G, R, N;
    double* label_arena; float* row_weight; int* misfit;
} nrm_assemble_groups;
int nrm_assemble_groups_at(const nrm_assemble_tables* tables, const nrm_assemble_groups* groups, const long* order, long n_order,
                           const long* cursor, int B, int H, int T, int flags, nrm_stream_t stream);

/* ---- the record of a table-fed epoch kept on the device (additive)
 * One launch of ONE workgroup at the end of a step, in place of the epoch loop's per-step accumulations (reference train.py:77-94):
 *   sums[0] += (double)*loss * B           train.py:82 total_loss += loss.item() * B  (one rounded product, one rounded sum: no fma)
 *   sums[1] += sum of auc[b] >= 0,  counts[0] += rows with auc[b] < 0 (one class in the row),  sums[2] += sum of top1[b]
 *   step_log[k] = {*loss, mean of the auc[b] >= 0 (0 without one)} with k = counts[1], unless k >= log_cap      train.py:83,93-94
 *   counts[1] += 1,  *cursor += B
 * auc / top1 [B] are the outputs of nrm_row_auc.  float64 accumulation in a fixed order (per-thread strided sums, a fixed shuffle
 * tree, the wave partials in wave order), no atomics: the same bits from run to run.  All stores are plain stores of one lane.
 * B = 0 launches nothing.  step_log may be null where log_cap = 0. */
int nrm_epoch_tally(const float* loss, const float* auc, const int* top1, int B, long* cursor, double* sums, long* counts,
                    float* step_log, long log_cap, nrm_stream_t stream);

/* ---- the record of a table-fed evaluation pass kept on the device (additive, the ABI version is unchanged)
 * One launch of ONE workgroup at the end of an evaluation step of B impressions whose scoring tail ran at width Tp (1 <= Tp <= T), in
 * place of the per-batch sums of reference verify.py:25-43 and the per-batch device-to-host copy of test.py:118-130:
 *   row b of the step is position p = *cursor + b of the pass; rows with p outside [0, n_order) are neither summed nor written
 *   sums[0] += sum of auc[b] >= 0,        counts[0] += rows with auc[b] < 0 (one class in the row),  sums[1] += sum of top1[b]
 *   sums[2..4] += sums of metrics[b][0..2] over the rows with metrics[b][0] >= 0,  counts[1] += rows with metrics[b][0] < 0
 *   counts[2] += 1 (steps),  counts[3] += rows with p inside the pass (the rows written, where there is a record)
 *   rec_rank[p % cap][0..T) = rank[b][0..Tp) then 0,  rec_live[p % cap] = live[b],  rec_id[p % cap] = impression_id[b]
 *   *cursor += B (a plain store of one lane, after every row has read the cursor)
 * auc [B] fp32 / top1 [B] int32 are the outputs of nrm_row_auc, NULL together; metrics [B,3] fp32, rank [B,Tp] int32 and live [B] int32
 * those of nrm_ensemble_rank (metrics NULL: a data set without labels); impression_id [B] int64; sums [5] float64, counts [4] int64.
 * rec_rank [cap,T] int32, rec_live [cap] int32, rec_id [cap] int64 are NULL together with cap = 0 (a pass that keeps the sums only);
 * cap > 0 is a multiple of B.  float64 accumulation in the fixed order of nrm_epoch_tally, no atomics: the same bits from run to run.
 * All stores are plain stores.  B = 0 launches nothing. */
int nrm_eval_tally(const float* auc, const int* top1, const float* metrics, const int* rank, const int* live, const long* impression_id,
                   int B, int T, int Tp, long* cursor, long n_order, double* sums, long* counts, int* rec_rank, int* rec_live, long* rec_id,
                   long cap, nrm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NRM_HOTPATH_H */
