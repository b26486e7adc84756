// extern "C" entry points declared in include/nrm_hotpath.h: host-side validation + launches only.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../include/nrm_hotpath.h"
#include "common.hpp"
#include "pwattn.hpp"
#include "gemm.hpp"
#include "head.hpp"
#include "pool_loss.hpp"
#include "frontend.hpp"
#include "scoring.hpp"
#include "compact.hpp"
#include "assemble.hpp"
#include "epoch.hpp"

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return NRM_OK;
    return fail(NRM_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// wave slots of the chip at 2 waves/SIMD: 256 CUs x 4 SIMDs x 2
static const int kTargetWaves = 2048;
// Wave tasks of the two backward contraction launches.  Measured on MI355X at C3 (scripts/sweep_waves.sh): several
// rounds of smaller tasks balance better than exactly one round (dh pass 4.81 -> 4.58 ms at 4 rounds of 3 waves/SIMD,
// dt/dW pass 5.81 -> 5.56 ms at 3 rounds; every split of the dW pass costs one [D,D] partial slab).
// NRM_BT_WAVES / NRM_BH_WAVES override them for tuning.
static const int kBtWaves = 6144;
static const int kBtMinGroups = 96;     // groups per split of the dt/dW pass (each split = one [D, D] slab of dW_p)
static const int kBhWaves = 12288;
static const int kTnWaves = 0;         // gemm_tn (dW = dY^T X): 0 = one round of wave tasks at the chosen kernel's occupancy (gemm_tn_plan); NRM_TN_WAVES overrides

static int check_dims(const char* fn, int B, int T, int H, int D) {
    if (B < 0 || T <= 0 || H <= 0 || D <= 0) return fail(NRM_EINVAL, "%s: B=%d T=%d H=%d D=%d must be positive", fn, B, T, H, D);
    if (D % 4) return fail(NRM_EINVAL, "%s: D=%d must be a multiple of 4", fn, D);
    if (D > 1024) return fail(NRM_EINVAL, "%s: D=%d > 1024 not supported", fn, D);
    const long M = (long)B * T * H;
    // buffer descriptors address with 32-bit byte offsets; 2^31 is reserved as the "masked row" marker
    if (M >= (1L << 31) || (long)B * T * D >= (1L << 29) || (long)B * H * D >= (1L << 29))
        return fail(NRM_EINVAL, "%s: B*T*H=%ld exceeds 2^31 rows or a [B,T,D]/[B,H,D] operand exceeds 2^31 bytes", fn, M);
    return NRM_OK;
}

// plan of the (b,t)-grouped pass: nrm_pwattn_bwd_nsplit sizes the slab buffer that nrm_pwattn_bwd_contract then fills
static nrm::BwdEPlan bwd_bt_plan(int B, int T, int D, int mma) {
    const char* e = getenv("NRM_BT_WAVES");
    return nrm::bwd_e_plan(D, B * T, e ? atoi(e) : kBtWaves, kBtMinGroups, mma);
}

// One launch of nrm_pwattn_bwd_contract: its parameter block and plan.  G = B G2 groups of R rows; X_g = the dz rows of group g, Y_g =
// the R rows y[b]; out[g] += the row gradient.  pass 1: groups (b,t), rows r = h: X_g = dz[b,t,:,:], Y_g = h[b]; out = dt, scale rows = t,
// dW_p slabs in ws; pass 4: the same without its dt epilogue; pass 2: groups (b,h), rows r = t: X_g = dz[b,:,h,:], Y_g = t[b]; out = dh
struct BwdPass { nrm::BwdEParams p; nrm::BwdEPlan pl; bool with_dw; };
static BwdPass bwd_pass(int pass, const float* dz, const float* t, const float* h, const float* wp, int ldwp, float* dt, float* dh,
                        float* ws, int B, int T, int H, int D, int mma, int dz_format) {
    const bool bh = pass == 2;
    const int G2 = bh ? H : T, R = bh ? T : H; const long HD = (long)H * D;
    nrm::BwdEParams p = {};
    p.X = dz; p.xs1 = (long)T * HD; p.xs2 = bh ? D : HD; p.xrs = bh ? HD : D;
    p.Y = bh ? t : h; p.ys1 = (long)R * D; p.yrs = D;
    p.wp = wp; p.ldwp = ldwp; p.out = bh ? dh : dt; p.ldo = D;
    p.G = B * G2; p.G2 = G2; p.R = R; p.D = D;
    p.with_dt = pass != 4; p.x_hl4 = dz_format == NRM_DZ_HL4;
    // big groups (C5: 128 rows x 768 columns = 393 KB of dz each): the waves of a workgroup walk neighbouring groups, which
    // cuts what an XCD's L2 must hold -- FETCH_SIZE of the (b,t) pass at C5 26.3 -> 8.0 GB, same duration (the MALL had been
    // absorbing the re-reads); small groups keep the blocked walk.  NRM_BT_INTERLEAVE=0|1 forces either (tests).
    p.interleave = (long)R * D * (long)sizeof(float) > (256L << 10);       // ((b,h) pass: read by the serial kernel only -- bf16 forms, short T)
    if (const char* e = getenv("NRM_BT_INTERLEAVE")) p.interleave = atoi(e);
    if (bh) {                                           // no dW_p accumulators (<= 168 VGPRs): three waves per SIMD
        const char* e = getenv("NRM_BH_WAVES");
        return {p, nrm::bwd_e_plan(D, p.G, e ? atoi(e) : kBhWaves, 1, mma), false};
    }
    p.srow = t; p.lds_ = D; p.ws = ws;
    if (const char* e = getenv("NRM_BT_ORDER")) p.order = atoi(e);
    return {p, bwd_bt_plan(B, T, D, mma), true};
}

static bool bwd_dz_format_ok(int passes, int mma, int dz_format) {     // NRM_DZ_HL4: the dW_p-only pass (4) of the bf16 arithmetics alone
    return dz_format == NRM_DZ_F32 || (dz_format == NRM_DZ_HL4 && passes == 4 && mma != NRM_MMA_F32);
}

extern "C" {

int nrm_abi_version(void) { return NRM_ABI_VERSION; }
int nrm_build_flags(void) { return nrm::pwattn_fwd_diag_flags() | nrm::pwattn_fwd_rw_diag_flags() | nrm::pwattn_bwd_diag_flags() |
                                    nrm::pwattn_bwd_rw_diag_flags() | nrm::pwattn_bwd_dp_diag_flags() | nrm::gemm_bf16_diag_flags() | nrm::gemm_diag_flags()
#if defined(NRM_STORE_GUARD) && NRM_STORE_GUARD != 2
                                    | 0x200                            // 16-byte stores without (or with a weaker) hazard guard: common.hpp
#endif
                                    ; }
const char* nrm_last_error(void) { return g_err; }

long nrm_pwattn_packed_floats(int D) {
    if (D <= 0) return 0;
    const nrm::FwdPlan pl = nrm::pwattn_fwd_plan(D);
    // fp32: kchunks 16-column chunks of rows x 64 B, the rows of the form the width takes (pack_wp_launch).  bf16 / bf16x3
    // (pwattn_fwd_rw.hip): k32 chunks x (1 | 2) images x plan rows x 64 B, where the resident-W plan may pad the rows up to one more
    // slice -- size for the largest of the three
    const int rows0 = nrm::pwattn_fwd_uses_rw(D, NRM_MMA_F32) ? nrm::pwattn_rw_plan(D, NRM_MMA_F32).rows : pl.rows;
    const long f32 = (long)pl.kchunks * rows0 * 16;
    const nrm::RwPlan r3 = nrm::pwattn_rw_plan(D, NRM_MMA_BF16X3), r1 = nrm::pwattn_rw_plan(D, NRM_MMA_BF16);
    const long b3 = (long)r3.k32 * 2 * r3.rows * 16, b1 = (long)r1.k32 * r1.rows * 16;
    const long need = f32 > b3 ? (f32 > b1 ? f32 : b1) : (b3 > b1 ? b3 : b1);
    return need + 256 * 4 * 2;   // + over-read pad of the staging loop
}

static int check_mma(const char* fn, int mma) {
    if (mma != NRM_MMA_F32 && mma != NRM_MMA_BF16 && mma != NRM_MMA_BF16X3)
        return fail(NRM_EINVAL, "%s: mma=%d (NRM_MMA_F32, NRM_MMA_BF16 or NRM_MMA_BF16X3)", fn, mma);
    return NRM_OK;
}

int nrm_pwattn_pack_wp(const float* fc1_weight, int ld, int D, int mma, float* packed, nrm_stream_t stream) {
    if (!fc1_weight || !packed) return fail(NRM_EINVAL, "nrm_pwattn_pack_wp: null pointer");
    if (D <= 0 || D % 4 || ld < 4 * D) return fail(NRM_EINVAL, "nrm_pwattn_pack_wp: D=%d ld=%d (need D%%4==0, ld>=4D)", D, ld);
    if (int rc = check_mma("nrm_pwattn_pack_wp", mma)) return rc;
    const nrm::FwdPlan pl = nrm::pwattn_fwd_plan(D);
    return check_hip(nrm::pack_wp_launch(fc1_weight + 3 * (long)D, ld, D, pl, mma, packed, (hipStream_t)stream), "pack_wp");
}

// parameter block of the dense and the ragged forward: `cand` candidate rows in t / v (B T dense; N ragged, with T = 1), B H rows in h / u
static nrm::FwdParams fwd_params(const float* t, const float* h, const float* u, const float* v, const float* packed_wp, const float* w2,
                                 const float* b2, float* z, float* s, long cand, int T, int B, int H, int D, const nrm::FwdPlan& pl) {
    nrm::FwdParams p;
    p.t = t; p.h = h; p.u = u; p.v = v; p.wp = packed_wp; p.w2 = w2; p.b2 = b2; p.z = z; p.s = s;
    p.M = cand * H; p.T = T; p.H = H; p.D = D;
    p.ldt = D; p.ldh = D; p.ldu = D; p.ldv = D;
    p.wp_bytes = (unsigned)(nrm_pwattn_packed_floats(D) * 4);
    p.t_bytes = (unsigned)(cand * D * 4);
    p.h_bytes = (unsigned)((long)B * H * D * 4);
    p.rows = pl.rows; p.kchunks = pl.kchunks; p.nchunks = pl.nchunks;
    return p;
}

int nrm_pwattn_fwd(const float* t, const float* h, const float* u, const float* v, const float* packed_wp,
                   const float* w2, const float* b2, float* z, float* s,
                   int B, int T, int H, int D, int mma, nrm_stream_t stream) {
    if (int rc = check_dims("nrm_pwattn_fwd", B, T, H, D)) return rc;
    if (int rc = check_mma("nrm_pwattn_fwd", mma)) return rc;
    if (!t || !h || !u || !v || !packed_wp || !w2 || !b2 || !s) return fail(NRM_EINVAL, "nrm_pwattn_fwd: null pointer");
    if (B == 0) return NRM_OK;
    const nrm::FwdPlan pl = nrm::pwattn_fwd_plan(D);
    if (mma != NRM_MMA_F32 && !nrm::pwattn_fwd_uses_rw(D, mma))
        return fail(NRM_EINVAL, "nrm_pwattn_fwd: D=%d is too wide for the bf16 forward (one 16-column slice of W_p must fit the LDS)", D);
    const nrm::FwdParams p = fwd_params(t, h, u, v, packed_wp, w2, b2, z, s, (long)B * T, T, B, H, D, pl);
    return check_hip(nrm::pwattn_fwd_launch(p, mma, (hipStream_t)stream), "pwattn_fwd");
}

int nrm_pwattn_fwd_ragged(const float* t, const float* h, const float* u, const float* v, const float* packed_wp,
                          const float* w2, const float* b2, float* s, const int* cand_imp, const int* cand_off,
                          int B, int N, int max_count, int H, int D, int mma, nrm_stream_t stream) {
    if (int rc = check_mma("nrm_pwattn_fwd_ragged", mma)) return rc;
    if (mma != NRM_MMA_F32)
        return fail(NRM_EINVAL, "nrm_pwattn_fwd_ragged: mma=%d: the ragged forward has fp32 arithmetic only (NRM_MMA_F32); the bf16 / bf16x3 "
                                "forms exist for dense candidate lists (nrm_pwattn_fwd)", mma);
    if (B < 0 || N < 0 || max_count < 0 || max_count > N || H <= 0 || D <= 0)
        return fail(NRM_EINVAL, "nrm_pwattn_fwd_ragged: B=%d N=%d max_count=%d H=%d D=%d (B, N >= 0, 0 <= max_count <= N, H, D > 0)", B, N, max_count, H, D);
    if (D % 4) return fail(NRM_EINVAL, "nrm_pwattn_fwd_ragged: D=%d must be a multiple of 4", D);
    if (D > 1024) return fail(NRM_EINVAL, "nrm_pwattn_fwd_ragged: D=%d > 1024 not supported", D);
    if ((long)N * H >= (1L << 31) || (long)N * D >= (1L << 29) || (long)B * H * D >= (1L << 29))
        return fail(NRM_EINVAL, "nrm_pwattn_fwd_ragged: N*H=%ld exceeds 2^31 rows or a [N,D]/[B,H,D] operand exceeds 2^31 bytes", (long)N * H);
    if (!t || !h || !u || !v || !packed_wp || !w2 || !b2 || !s || !cand_imp || !cand_off) return fail(NRM_EINVAL, "nrm_pwattn_fwd_ragged: null pointer");
    if (N == 0 || B == 0) return NRM_OK;
    const nrm::FwdPlan pl = nrm::pwattn_fwd_plan(D);
    const nrm::FwdParams p = fwd_params(t, h, u, v, packed_wp, w2, b2, nullptr, s, N, 1, B, H, D, pl);
    nrm::RaggedTabs rg;
    rg.cand_imp = cand_imp; rg.cand_off = cand_off; rg.B = B; rg.N = N; rg.max_count = max_count;
    return check_hip(nrm::pwattn_fwd_ragged_launch(p, rg, (hipStream_t)stream), "pwattn_fwd_ragged");
}

int nrm_pwattn_fwd_hragged(const float* t, const float* h, const float* u, const float* v, const float* packed_wp,
                           const float* w2, const float* b2, float* s, const int* cand_imp, const int* cand_off, const int* hist_off,
                           const int* tile_pre, const void* tile_tab, int B, int N, int max_count, int R, int Mt, int k_max, int D, int mma,
                           nrm_stream_t stream) {
    if (int rc = check_mma("nrm_pwattn_fwd_hragged", mma)) return rc;
    if (mma != NRM_MMA_F32)
        return fail(NRM_EINVAL, "nrm_pwattn_fwd_hragged: mma=%d: the ragged forward has fp32 arithmetic only (NRM_MMA_F32); the bf16 / bf16x3 "
                                "forms exist for dense candidate lists (nrm_pwattn_fwd)", mma);
    if (B < 0 || N < 0 || max_count < 0 || max_count > N || R < 0 || Mt < 0 || k_max < 0 || k_max > R || D <= 0)
        return fail(NRM_EINVAL, "nrm_pwattn_fwd_hragged: B=%d N=%d max_count=%d R=%d Mt=%d k_max=%d D=%d (B, N, R, Mt >= 0, 0 <= max_count <= N, "
                                "0 <= k_max <= R, D > 0)", B, N, max_count, R, Mt, k_max, D);
    if (D % 4) return fail(NRM_EINVAL, "nrm_pwattn_fwd_hragged: D=%d must be a multiple of 4", D);
    if (D > 1024) return fail(NRM_EINVAL, "nrm_pwattn_fwd_hragged: D=%d > 1024 not supported", D);
    if (16L * Mt >= (1L << 31) || (long)N * D >= (1L << 29) || (long)R * D >= (1L << 29))
        return fail(NRM_EINVAL, "nrm_pwattn_fwd_hragged: 16*Mt=%ld exceeds 2^31 rows or a [N,D]/[R,D] operand exceeds 2^31 bytes", 16L * Mt);
    if (!t || !h || !u || !v || !packed_wp || !w2 || !b2 || !s || !cand_imp || !cand_off || !hist_off || !tile_pre || !tile_tab)
        return fail(NRM_EINVAL, "nrm_pwattn_fwd_hragged: null pointer");
    if ((uintptr_t)tile_tab & 15) return fail(NRM_EINVAL, "nrm_pwattn_fwd_hragged: tile_tab must be 16-byte aligned");
    if (N == 0 || B == 0 || Mt == 0 || R == 0) return NRM_OK;
    const nrm::FwdPlan pl = nrm::pwattn_fwd_plan(D);
    nrm::FwdParams p = fwd_params(t, h, u, v, packed_wp, w2, b2, nullptr, s, N, 1, B, 1, D, pl);
    p.M = 16L * Mt;
    p.h_bytes = (unsigned)((long)R * D * 4);
    nrm::RaggedTabs rg;
    rg.cand_imp = cand_imp; rg.cand_off = cand_off; rg.B = B; rg.N = N; rg.max_count = max_count;
    rg.hist_off = hist_off; rg.tile_pre = tile_pre; rg.tile_tab = (const int4*)tile_tab; rg.R = R; rg.Mt = Mt; rg.k_max = k_max;
    return check_hip(nrm::pwattn_fwd_hragged_launch(p, rg, (hipStream_t)stream), "pwattn_fwd_hragged");
}

int nrm_pwattn_fwd_form(int B, int T, int H, int D, int mma, int save_z, int ragged, int N, int max_count, int k_max, int cus, int* out) {
    const char* fn = "nrm_pwattn_fwd_form";
    if (!out) { fail(NRM_EINVAL, "%s: null pointer", fn); return -1; }
    if (check_mma(fn, mma)) return -1;
    if (ragged < 0 || ragged > 2 || (save_z != 0 && save_z != 1) || cus < 0) {
        fail(NRM_EINVAL, "%s: save_z=%d ragged=%d cus=%d (save_z 0 or 1, ragged 0, 1 or 2, cus >= 0)", fn, save_z, ragged, cus);
        return -1;
    }
    long M;
    if (ragged == 0) {
        if (check_dims(fn, B, T, H, D)) return -1;
        M = (long)B * T * H;
    } else {
        // the checks of nrm_pwattn_fwd_ragged / _hragged that need no pointer; ragged == 2: T is Mt, the number of 16-row score tiles
        const int Mt = ragged == 2 ? T : 0;
        if (ragged == 2) H = 1;
        if (B < 0 || N < 0 || max_count < 0 || max_count > N || H <= 0 || D <= 0 || D % 4 || D > 1024 || Mt < 0 || k_max < 0 ||
            (ragged == 1 ? (long)N * H : 16L * Mt) >= (1L << 31) || (long)N * D >= (1L << 29)) {
            fail(NRM_EINVAL, "%s: B=%d N=%d max_count=%d H=%d D=%d Mt=%d k_max=%d (B, N, Mt, k_max >= 0, 0 <= max_count <= N, H > 0, D a positive "
                             "multiple of 4 up to 1024, fewer than 2^31 rows)", fn, B, N, max_count, H, D, Mt, k_max);
            return -1;
        }
        M = ragged == 1 ? (long)N * H : 16L * Mt;
        if (N == 0 || B == 0) M = 0;                                     // the entries return before any launch
        T = 1;
    }
    const nrm::FwdForm f = nrm::pwattn_fwd_select(M, B, T, H, D, mma, save_z != 0, ragged, N, max_count, k_max, cus ? cus : nrm::device_cus());
    const int v[NRM_PWATTN_FWD_FORM_LEN] = {f.valid, f.family, f.NT, f.MT, f.WPE, f.CT, f.NW, f.NTS, f.KCH, f.mma, f.save_z, f.ragged,
                                            f.nsplit, f.tsplit, f.wgs * (f.nsplit > 0 ? f.nsplit : 1), (int)f.tasks, f.rounds, f.nchunks};
    for (int i = 0; i < NRM_PWATTN_FWD_FORM_LEN; ++i) out[i] = v[i];
    return 0;
}

int nrm_pwattn_bwd_dz(float* z_inout, const float* ds, const float* w2, float* dw2, float* db2, float* du, float* dv,
                      int B, int T, int H, int D, int dz_format, nrm_stream_t stream) {
    if (int rc = check_dims("nrm_pwattn_bwd_dz", B, T, H, D)) return rc;
    if (!z_inout || !ds || !w2 || !dw2 || !du || !dv) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dz: null pointer");
    if (B > 65535) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dz: B=%d > 65535 (one grid row per impression)", B);
    if (dz_format != NRM_DZ_F32 && dz_format != NRM_DZ_HL4) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dz: dz_format=%d (NRM_DZ_F32 or NRM_DZ_HL4)", dz_format);
    return check_hip(nrm::bwd_dz_launch(z_inout, ds, w2, dw2, db2, du, dv, B, T, H, D, dz_format, (hipStream_t)stream), "bwd_dz");
}

int nrm_pwattn_bwd_rw_supported(int D, int mma) { return nrm::pwattn_bwd_rw_plan(D, mma).ng ? 1 : 0; }
long nrm_pwattn_bwd_rw_packed_floats(int D, int mma) { return nrm::pwattn_bwd_rw_packed_floats(D, mma); }

int nrm_pwattn_bwd_rw_pack(const float* fc1_weight, int ld, int D, int mma, float* packed, nrm_stream_t stream) {
    if (!fc1_weight || !packed) return fail(NRM_EINVAL, "nrm_pwattn_bwd_rw_pack: null pointer");
    if (D <= 0 || D % 4 || ld < 4 * D) return fail(NRM_EINVAL, "nrm_pwattn_bwd_rw_pack: D=%d ld=%d (need D%%4==0, ld>=4D)", D, ld);
    if (!nrm_pwattn_bwd_rw_supported(D, mma)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_rw_pack: D=%d mma=%d has no resident-W backward", D, mma);
    return check_hip(nrm::pwattn_bwd_rw_pack_launch(fc1_weight + 3 * (long)D, ld, D, mma, packed, (hipStream_t)stream), "bwd_rw_pack");
}

int nrm_pwattn_bwd_rw_dtdh(const float* dz_hl4, const float* t, const float* h, const float* packed, float* dt, float* dh,
                           int B, int T, int H, int D, int mma, nrm_stream_t stream) {
    if (int rc = check_dims("nrm_pwattn_bwd_rw_dtdh", B, T, H, D)) return rc;
    if (!dz_hl4 || !t || !h || !packed || !dt || !dh) return fail(NRM_EINVAL, "nrm_pwattn_bwd_rw_dtdh: null pointer");
    if (!nrm_pwattn_bwd_rw_supported(D, mma)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_rw_dtdh: D=%d mma=%d has no resident-W backward", D, mma);
    if ((long)T * H * D * 4 >= (1L << 31)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_rw_dtdh: one impression's dz block exceeds 2^31 bytes");
    if (B == 0) return NRM_OK;
    nrm::BwdRwParams p = {};
    p.dz = dz_hl4; p.t = t; p.h = h; p.wimg = packed; p.dt = dt; p.dh = dh; p.B = B; p.T = T; p.H = H; p.D = D;
    p.w_bytes = (unsigned)(nrm_pwattn_bwd_rw_packed_floats(D, mma) * 4);
    return check_hip(nrm::pwattn_bwd_rw_launch(p, mma, (hipStream_t)stream), "bwd_rw_dtdh");
}

int nrm_pwattn_bwd_dp_supported(int D, int H) { return nrm::pwattn_bwd_dp_plan(D, H).NT ? 1 : 0; }
long nrm_pwattn_bwd_dp_packed_floats(int D, int H) { return nrm::pwattn_bwd_dp_packed_floats(D, H); }

int nrm_pwattn_bwd_dp_pack(const float* fc1_weight, int ld, int D, int H, float* packed, nrm_stream_t stream) {
    if (!fc1_weight || !packed) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dp_pack: null pointer");
    if (D <= 0 || D % 4 || ld < 4 * D) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dp_pack: D=%d ld=%d (need D%%4==0, ld>=4D)", D, ld);
    if (!nrm_pwattn_bwd_dp_supported(D, H)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dp_pack: D=%d H=%d has no dP-walk backward", D, H);
    return check_hip(nrm::pwattn_bwd_dp_pack_launch(fc1_weight + 3 * (long)D, ld, D, H, packed, (hipStream_t)stream), "bwd_dp_pack");
}

int nrm_pwattn_bwd_dp_dtdh(const float* dz, const float* t, const float* h, const float* packed, float* dt, float* dh,
                           int B, int T, int H, int D, nrm_stream_t stream) {
    if (int rc = check_dims("nrm_pwattn_bwd_dp_dtdh", B, T, H, D)) return rc;
    if (!dz || !t || !h || !packed || !dt || !dh) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dp_dtdh: null pointer");
    if (!nrm_pwattn_bwd_dp_supported(D, H)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dp_dtdh: D=%d H=%d has no dP-walk backward (D %% 4 == 0, H >= 16)", D, H);
    // a row block of 64 history rows spans at most 63 / H + 2 impressions, whose dz blocks one buffer descriptor must cover
    if ((long)(63 / H + 2) * T * H * D * 4 >= (1L << 31)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dp_dtdh: the dz blocks of one row block exceed 2^31 bytes");
    if ((long)B * H * D * 4 >= (1L << 31) || (long)B * T * D * 4 >= (1L << 31)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_dp_dtdh: t or h exceeds 2^31 bytes");
    if (B == 0) return NRM_OK;
    nrm::BwdDpParams p = {};
    p.dz = dz; p.t = t; p.h = h; p.wimg = packed; p.dt = dt; p.dh = dh; p.B = B; p.T = T; p.H = H; p.D = D;
    p.w_bytes = (unsigned)(nrm_pwattn_bwd_dp_packed_floats(D, H) * 4);
    p.t_bytes = (unsigned)((long)B * T * D * 4); p.h_bytes = (unsigned)((long)B * H * D * 4);
    return check_hip(nrm::pwattn_bwd_dp_launch(p, (hipStream_t)stream), "bwd_dp_dtdh");
}

int nrm_pwattn_bwd_nsplit(int B, int T, int H, int D, int mma) {
    if (B <= 0 || T <= 0 || H <= 0 || D <= 0) return 0;
    return bwd_bt_plan(B, T, D, mma).nsplit;
}

int nrm_pwattn_bwd_contract(const float* dz, const float* t, const float* h, const float* wp, int ldwp,
                            float* dt, float* dh, float* ws, int B, int T, int H, int D, int passes, int mma,
                            int dz_format, nrm_stream_t stream) {
    if (int rc = check_dims("nrm_pwattn_bwd_contract", B, T, H, D)) return rc;
    if (int rc = check_mma("nrm_pwattn_bwd_contract", mma)) return rc;
    if (passes != 1 && passes != 2 && passes != 3 && passes != 4) return fail(NRM_EINVAL, "nrm_pwattn_bwd_contract: passes=%d", passes);
    if (!bwd_dz_format_ok(passes, mma, dz_format))
        return fail(NRM_EINVAL, "nrm_pwattn_bwd_contract: passes=%d mma=%d with dz_format=%d (only the dW_p-only pass, 4, of the bf16 arithmetics reads NRM_DZ_HL4)", passes, mma, dz_format);
    if (!dz || !t || !h || !wp) return fail(NRM_EINVAL, "nrm_pwattn_bwd_contract: null pointer");
    if (((passes & 1) && (!dt || !ws)) || ((passes & 2) && !dh) || (passes == 4 && !ws)) return fail(NRM_EINVAL, "nrm_pwattn_bwd_contract: null output");
    if (ldwp < D || ldwp % 4) return fail(NRM_EINVAL, "nrm_pwattn_bwd_contract: ldwp=%d", ldwp);
    if (B == 0) return NRM_OK;
    for (int pass : {passes == 4 ? 4 : passes & 1, passes & 2}) {
        if (!pass) continue;
        const BwdPass a = bwd_pass(pass, dz, t, h, wp, ldwp, dt, dh, ws, B, T, H, D, mma, dz_format);
        if (int rc = check_hip(nrm::bwd_e_launch(a.p, a.pl, a.with_dw, mma, (hipStream_t)stream), pass == 2 ? "bwd_e pass 2" : "bwd_e pass 1")) return rc;
    }
    return NRM_OK;
}

int nrm_pwattn_bwd_form(int T, int H, int D, int pass, int mma, int dz_format) {
    if (check_dims("nrm_pwattn_bwd_form", 1, T, H, D) || check_mma("nrm_pwattn_bwd_form", mma)) return -1;
    if ((pass != 1 && pass != 2 && pass != 4) || !bwd_dz_format_ok(pass, mma, dz_format)) return -1;
    const BwdPass a = bwd_pass(pass, nullptr, nullptr, nullptr, nullptr, D, nullptr, nullptr, nullptr, 1, T, H, D, mma, dz_format);
    const nrm::BwdEForm f = nrm::bwd_e_select(a.p, a.pl, a.with_dw, mma, nrm::bwd_e_knobs());
    if (f.family == nrm::BWD_E_REFUSED) return -1;
    return f.family | (f.exact ? 4 : 0) | (a.pl.DT == 5 ? 8 : 0) | (f.with_dw ? 16 : 0) | (f.with_dt ? 32 : 0) | (f.xhl4 ? 64 : 0);
}

int nrm_pwattn_bwd_dw_pack(int B, int T, int H, int D, int mma) {
    if (B <= 0 || check_dims("nrm_pwattn_bwd_dw_pack", B, T, H, D) || check_mma("nrm_pwattn_bwd_dw_pack", mma)) return -1;
    const BwdPass a = bwd_pass(4, nullptr, nullptr, nullptr, nullptr, D, nullptr, nullptr, nullptr, B, T, H, D, mma, NRM_DZ_F32);
    const nrm::BwdEForm f = nrm::bwd_e_select(a.p, a.pl, a.with_dw, mma, nrm::bwd_e_knobs());
    return f.family == nrm::BWD_DW_DIRECT ? f.pack : 1;
}

int nrm_pwattn_bwd_plan(int launch, int B, int T, int H, int D, int pass, int mma, int dz_format, int cus, int* out) {
    const char* fn = "nrm_pwattn_bwd_plan";
    if (!out) { fail(NRM_EINVAL, "%s: null pointer", fn); return -1; }
    if (launch < NRM_BWD_LAUNCH_DZ || launch > NRM_BWD_LAUNCH_RW || cus < 0) { fail(NRM_EINVAL, "%s: launch=%d cus=%d", fn, launch, cus); return -1; }
    if (check_dims(fn, B, T, H, D)) return -1;
    if (!cus && (launch == NRM_BWD_LAUNCH_DP || launch == NRM_BWD_LAUNCH_RW)) cus = nrm::device_cus();
    int v[NRM_PWATTN_BWD_PLAN_LEN] = {};
    if (launch == NRM_BWD_LAUNCH_DZ) {                                   // the value checks of nrm_pwattn_bwd_dz
        if (B > 65535 || (dz_format != NRM_DZ_F32 && dz_format != NRM_DZ_HL4)) { fail(NRM_EINVAL, "%s: B=%d dz_format=%d (B <= 65535, NRM_DZ_F32 or NRM_DZ_HL4)", fn, B, dz_format); return -1; }
        const nrm::BwdDzForm f = nrm::bwd_dz_select(B, T, H, D);
        const int w[] = {f.valid, f.family, f.threads, f.rows_class, f.slab_cols, f.nslab, f.hchunk, f.nhc, f.big_lds, f.narrowed, dz_format};
        if (f.valid) for (size_t i = 0; i < sizeof(w) / sizeof(w[0]); ++i) v[i] = w[i];
    } else if (launch == NRM_BWD_LAUNCH_CONTRACT) {                      // ... of nrm_pwattn_bwd_contract, for one of its launches
        if (check_mma(fn, mma)) return -1;
        if ((pass != 1 && pass != 2 && pass != 4) || !bwd_dz_format_ok(pass, mma, dz_format)) { fail(NRM_EINVAL, "%s: pass=%d mma=%d dz_format=%d", fn, pass, mma, dz_format); return -1; }
        const BwdPass a = bwd_pass(pass, nullptr, nullptr, nullptr, nullptr, D, nullptr, nullptr, nullptr, B, T, H, D, mma, dz_format);
        const nrm::BwdEForm f = nrm::bwd_e_select(a.p, a.pl, a.with_dw, mma, nrm::bwd_e_knobs());
        if (f.family != nrm::BWD_E_REFUSED && a.p.G > 0) {
            const nrm::BwdEWalk wk = nrm::bwd_e_walk(a.p, a.pl, f);
            const int w[] = {1, f.family, a.pl.DT, f.exact, f.mma, f.with_dw, f.with_dt, f.xhl4, f.family == nrm::BWD_DW_DIRECT ? f.pack : 1,
                             wk.interleave, wk.order, a.pl.nkw, a.pl.ndcol, a.pl.nsplit, a.pl.gps, wk.last_groups, wk.last_live, a.p.G};
            for (size_t i = 0; i < sizeof(w) / sizeof(w[0]); ++i) v[i] = w[i];
        }
    } else if (launch == NRM_BWD_LAUNCH_DP) {                            // ... of nrm_pwattn_bwd_dp_dtdh
        if ((long)(63 / H + 2) * T * H * D * 4 >= (1L << 31)) { fail(NRM_EINVAL, "%s: the dz blocks of one row block exceed 2^31 bytes", fn); return -1; }
        const nrm::BwdDpForm f = nrm::pwattn_bwd_dp_select(B, T, H, D, cus);
        if (f.valid) {
            int max_steps, max_items;
            nrm::pwattn_bwd_dp_extent(f, T, max_steps, max_items);
            const int w[] = {1, f.pl.NT, f.pl.nchunks, f.pl.kchunks, (int)f.steps, (int)f.grid, max_steps, max_items};
            for (size_t i = 0; i < sizeof(w) / sizeof(w[0]); ++i) v[i] = w[i];
        }
    } else {                                                             // ... of nrm_pwattn_bwd_rw_dtdh
        if (check_mma(fn, mma)) return -1;
        if ((long)T * H * D * 4 >= (1L << 31)) { fail(NRM_EINVAL, "%s: one impression's dz block exceeds 2^31 bytes", fn); return -1; }
        const nrm::BwdRwForm f = nrm::pwattn_bwd_rw_select(B, T, H, D, mma, cus);
        if (f.valid) {
            const int w[] = {1, f.NG, f.mma, f.exact, f.nks, f.wgs * f.nks, f.nw, f.tsplit, (int)f.tasks, f.rounds, f.plain_dh};
            for (size_t i = 0; i < sizeof(w) / sizeof(w[0]); ++i) v[i] = w[i];
        }
    }
    for (int i = 0; i < NRM_PWATTN_BWD_PLAN_LEN; ++i) out[i] = v[i];
    return 0;
}

// ------------------------------------------------------------------------------------------- dense layers
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

long nrm_gemm_packed_floats(int nrows, int ncols, int mma) {
    if (nrows <= 0 || ncols <= 0) return 0;
    if (mma == NRM_MMA_BF16 || mma == NRM_MMA_BF16X3)                    // weight fragments of gemm_nt_rx: 1 KiB per (tile, chunk, image)
        return (long)((nrows + 15) / 16) * ((ncols + 31) / 32) * (mma == NRM_MMA_BF16X3 ? 2 : 1) * 256 + 1024;
    const nrm::GemmNtPlan pl = nrm::gemm_nt_plan(nrows);
    return (long)((ncols + 15) / 16) * pl.rows * 16 + 1024;
}

int nrm_gemm_nt_bf16_supported(int M, int K, int mma) { return nrm::gemm_nt_rx_bm(M, K, mma) ? 1 : 0; }

int nrm_gemm_nt_form(int M, int N, int K, int mma) {
    if (M <= 0 || N <= 0 || K <= 0 || check_mma("nrm_gemm_nt_form", mma)) return -1;
    if (mma != NRM_MMA_F32) {
        const nrm::GemmRxForm f = nrm::gemm_nt_rx_select(M, K, mma);
        return f.RT ? (f.RT | f.G << 8) : 0;
    }
    const nrm::GemmNtForm f = nrm::gemm_nt_select(M, nrm::gemm_nt_plan(N));
    return f.NT | f.MT << 8 | f.WPE << 16 | f.KC << 24;
}

int nrm_gemm_pack(const float* src, long row_stride, long col_stride, int nrows, int ncols, float* packed,
                  nrm_stream_t stream) {
    if (!src || !packed || nrows <= 0 || ncols <= 0) return fail(NRM_EINVAL, "nrm_gemm_pack: bad argument");
    const nrm::GemmNtPlan pl = nrm::gemm_nt_plan(nrows);
    return check_hip(nrm::pack_rows_launch(src, row_stride, col_stride, nrows, ncols, pl.rows, (ncols + 15) / 16, packed,
                                           (hipStream_t)stream), "pack_rows");
}

int nrm_gemm_pack_multi(const nrm_pack_desc* descs, int n, nrm_stream_t stream) {
    if (n < 0 || (n > 0 && !descs)) return fail(NRM_EINVAL, "nrm_gemm_pack_multi: bad argument");
    for (int lo = 0; lo < n; lo += nrm::PACK_MAX) {
        const int m = n - lo < nrm::PACK_MAX ? n - lo : nrm::PACK_MAX;
        nrm::PackTable tab = {};
        long mx = 0;
        for (int i = 0; i < m; ++i) {
            const nrm_pack_desc& d = descs[lo + i];
            if (!d.src || !d.packed || d.nrows <= 0 || d.ncols <= 0) return fail(NRM_EINVAL, "nrm_gemm_pack_multi: entry %d is malformed", lo + i);
            const nrm::GemmNtPlan pl = nrm::gemm_nt_plan(d.nrows);
            nrm::PackEntry& e = tab.e[i];
            e.src = d.src; e.src2 = d.src2; e.dst = d.packed; e.rs = d.row_stride; e.cs = d.col_stride;
            e.nrows = d.nrows; e.ncols = d.ncols; e.rows = pl.rows; e.kchunks = (d.ncols + 15) / 16; e.sign2 = d.sign2; e.fmt = 0;
            if (d.mma == NRM_MMA_BF16 || d.mma == NRM_MMA_BF16X3) {
                e.fmt = d.mma == NRM_MMA_BF16X3 ? 2 : 1; e.rows = (d.nrows + 15) / 16 * 16; e.kchunks = (d.ncols + 31) / 32;
            } else if (d.mma != NRM_MMA_F32) return fail(NRM_EINVAL, "nrm_gemm_pack_multi: entry %d: mma=%d", lo + i, d.mma);
            const long total = e.fmt ? (long)(e.rows / 16) * e.kchunks * 512 : (long)e.kchunks * e.rows * 16;
            if (total > mx) mx = total;
        }
        if (int rc = check_hip(nrm::pack_rows_multi_launch(tab, m, mx, (hipStream_t)stream), "pack_rows_multi")) return rc;
    }
    return NRM_OK;
}

int nrm_gemm_nt(const float* x, int ldx, int M, const float* packed, int N, int K, const float* bias,
                float* y, int ldy, float* z, int ldz, const float* m, int ldm, int epilogue, int mma, nrm_stream_t stream) {
    if (!x || !packed || !y) return fail(NRM_EINVAL, "nrm_gemm_nt: null pointer");
    if (M < 0 || N <= 0 || K <= 0) return fail(NRM_EINVAL, "nrm_gemm_nt: M=%d N=%d K=%d", M, N, K);
    if (ldx % 4 || ldy % 4 || ldx < K || ldy < N || !al16(x) || !al16(y))
        return fail(NRM_EINVAL, "nrm_gemm_nt: ldx=%d ldy=%d must be multiples of 4 covering K=%d / N=%d, rows 16-B aligned", ldx, ldy, K, N);
    if (epilogue != NRM_EPI_BIAS && (!z || ldz % 4 || ldz < N || !al16(z)))
        return fail(NRM_EINVAL, "nrm_gemm_nt: epilogue %d needs z with ldz %% 4 == 0, ldz >= N", epilogue);
    if (epilogue < 0 || epilogue > 3) return fail(NRM_EINVAL, "nrm_gemm_nt: epilogue=%d", epilogue);
    if (epilogue == NRM_EPI_MUL && (!m || ldm % 4 || ldm < N || !al16(m)))
        return fail(NRM_EINVAL, "nrm_gemm_nt: NRM_EPI_MUL needs m with ldm %% 4 == 0, ldm >= N");
    if ((long)256 * (ldx > ldy ? ldx : ldy) * 4 >= (1L << 31)) return fail(NRM_EINVAL, "nrm_gemm_nt: leading dimension too large");
    if (int rc = check_mma("nrm_gemm_nt", mma)) return rc;
    if (mma != NRM_MMA_F32) {                                          // bf16 matrix cores: resident-X form (gemm_bf16.hip)
        if (!nrm::gemm_nt_rx_bm(M > 0 ? M : 1, K, mma)) return fail(NRM_EINVAL, "nrm_gemm_nt: K=%d is too wide for the bf16 form (nrm_gemm_nt_bf16_supported)", K);
        nrm::GemmRxParams r = {};
        r.x = x; r.ldx = ldx; r.xcols = ldx; r.wq = packed; r.wq_bytes = (unsigned)(nrm_gemm_packed_floats(N, K, mma) * 4);
        r.bias = bias; r.N = N; r.y = y; r.ldy = ldy;
        r.z = epilogue == NRM_EPI_BIAS ? nullptr : z; r.ldz = epilogue == NRM_EPI_BIAS ? 4 : ldz;
        r.m = epilogue == NRM_EPI_MUL ? m : nullptr; r.ldm = epilogue == NRM_EPI_MUL ? ldm : 4;
        r.M = M; r.K = K; r.k32 = (K + 31) / 32; r.nt16 = (N + 15) / 16;
        return check_hip(nrm::gemm_nt_rx_launch(r, epilogue, mma, (hipStream_t)stream), "gemm_nt_rx");
    }
    const nrm::GemmNtPlan pl = nrm::gemm_nt_plan(N);
    nrm::GemmNtParams p;
    p.x = x; p.ldx = ldx; p.xcols = ldx; p.wp = packed; p.wp_bytes = (unsigned)(nrm_gemm_packed_floats(N, K, NRM_MMA_F32) * 4);
    p.rows = pl.rows; p.bias = bias; p.N = N; p.y = y; p.ldy = ldy;
    p.z = epilogue == NRM_EPI_BIAS ? nullptr : z; p.ldz = epilogue == NRM_EPI_BIAS ? 4 : ldz;
    p.m = epilogue == NRM_EPI_MUL ? m : nullptr; p.ldm = epilogue == NRM_EPI_MUL ? ldm : 4;
    p.M = M; p.K = K; p.kchunks = (K + 15) / 16;
    return check_hip(nrm::gemm_nt_launch(p, pl, epilogue, (hipStream_t)stream), "gemm_nt");
}

// bf16 forms: a wave's row range is consumed 16/3x faster, so fewer, longer ranges (and fewer slabs for the reduction that
// follows): C2 gemm_tn 0.045 -> 0.036 ms per launch, slab reduction 0.20 -> 0.08 ms per step
static const int kTnWavesBf16 = 1024;
static int tn_waves(int mma = 0) {
    if (const char* e = getenv("NRM_TN_WAVES")) return atoi(e);
    return mma ? kTnWavesBf16 : kTnWaves;
}

int nrm_gemm_tn_nsplit(int ncols_i, int ncols_j, int R, int mma) {
    if (ncols_i <= 0 || ncols_j <= 0 || R <= 0) return 0;
    return nrm::gemm_tn_plan(ncols_i, ncols_j, R, tn_waves(mma), mma).nsplit;
}

int nrm_gemm_tn_plan(int ncols_i, int ncols_j, int R, int mma, int* kt, int* dt, int* rows_per_split) {
    if (ncols_i <= 0 || ncols_j <= 0 || R <= 0 || (mma != NRM_MMA_F32 && mma != NRM_MMA_BF16 && mma != NRM_MMA_BF16X3)) return -1;
    const nrm::GemmTnPlan pl = nrm::gemm_tn_plan(ncols_i, ncols_j, R, tn_waves(mma), mma);
    if (kt) *kt = pl.KT;
    if (dt) *dt = pl.DT;
    if (rows_per_split) *rows_per_split = pl.rps;
    return pl.nsplit;
}

int nrm_gemm_tn(const float* A, int lda, int ncols_i, const float* B, int ldb, int ncols_j, int R,
                float* ws, int ldws, float* colsum, float* zero_out, long zero_n, int mma, nrm_stream_t stream) {
    if (!A || !B || !ws) return fail(NRM_EINVAL, "nrm_gemm_tn: null pointer");
    if (ncols_i <= 0 || ncols_j <= 0 || R <= 0 || lda < ncols_i || ldb < ncols_j)
        return fail(NRM_EINVAL, "nrm_gemm_tn: ncols_i=%d ncols_j=%d R=%d lda=%d ldb=%d", ncols_i, ncols_j, R, lda, ldb);
    if (ldws % 4 || ldws < ncols_i || !al16(ws)) return fail(NRM_EINVAL, "nrm_gemm_tn: ldws=%d", ldws);
    if (int rc = check_mma("nrm_gemm_tn", mma)) return rc;
    const nrm::GemmTnPlan pl = nrm::gemm_tn_plan(ncols_i, ncols_j, R, tn_waves(mma), mma);
    if ((long)pl.rps * (lda > ldb ? lda : ldb) * 4 >= (1L << 31)) return fail(NRM_EINVAL, "nrm_gemm_tn: split too large");
    if (mma != NRM_MMA_F32 && (lda % 4 || ldb % 4 || ((uintptr_t)A & 15) || ((uintptr_t)B & 15)))
        return fail(NRM_EINVAL, "nrm_gemm_tn: the bf16 forms read 16-byte row segments (lda, ldb multiples of 4, 16-byte aligned rows)");
    nrm::GemmTnParams p = {};
    p.A = A; p.lda = lda; p.acols = lda; p.B = B; p.ldb = ldb; p.bcols = ldb;
    if (zero_out && (zero_n < 0 || !al16(zero_out))) return fail(NRM_EINVAL, "nrm_gemm_tn: zero_out must be 16-byte aligned, zero_n >= 0");
    p.ws = ws; p.ldws = ldws; p.colsum = colsum; p.R = R; p.ncols_j = ncols_j;
    p.zero_out = zero_out; p.zero_n = zero_out ? zero_n : 0;
    if (mma != NRM_MMA_F32) return check_hip(nrm::gemm_tn_bf16_launch(p, pl, mma, (hipStream_t)stream), "gemm_tn_bf16");
    return check_hip(nrm::gemm_tn_launch(p, pl, (hipStream_t)stream), "gemm_tn");
}

int nrm_slab_reduce(const float* ws, int nsplit, int nj, int ldws, int ni, float* out, long out_istride, long out_jstride,
                    float* out2, long out2_istride, long out2_jstride, float sign2,
                    const float* vec, float* vec_out, nrm_stream_t stream) {
    if (!ws || !out) return fail(NRM_EINVAL, "nrm_slab_reduce: null pointer");
    if (nsplit <= 0 || nj <= 0 || ni <= 0 || ldws < ni) return fail(NRM_EINVAL, "nrm_slab_reduce: nsplit=%d nj=%d ni=%d ldws=%d", nsplit, nj, ni, ldws);
    if ((vec == nullptr) != (vec_out == nullptr)) return fail(NRM_EINVAL, "nrm_slab_reduce: vec and vec_out go together");
    nrm::SlabReduceParams p;
    p.ws = ws; p.nsplit = nsplit; p.nj = nj; p.ldws = ldws; p.ni = ni; p.out = out; p.ors = out_istride; p.ocs = out_jstride;
    p.out2 = out2; p.ors2 = out2_istride; p.ocs2 = out2_jstride; p.sign2 = sign2; p.vec = vec; p.vec_out = vec_out;
    return check_hip(nrm::slab_reduce_launch(p, (hipStream_t)stream), "slab_reduce");
}

int nrm_slab_reduce_multi(const nrm_slab_desc* descs, int n, nrm_stream_t stream) {
    if (n < 0 || (n > 0 && !descs)) return fail(NRM_EINVAL, "nrm_slab_reduce_multi: bad argument");
    if (n == 0) return NRM_OK;
    std::vector<nrm::SlabReduceParams> ps((size_t)n);
    for (int i = 0; i < n; ++i) {
        const nrm_slab_desc& d = descs[i];
        if (!d.ws || !d.out) return fail(NRM_EINVAL, "nrm_slab_reduce_multi: entry %d: null pointer", i);
        if (d.nsplit <= 0 || d.nj <= 0 || d.ni <= 0 || d.ldws < d.ni)
            return fail(NRM_EINVAL, "nrm_slab_reduce_multi: entry %d: nsplit=%d nj=%d ni=%d ldws=%d", i, d.nsplit, d.nj, d.ni, d.ldws);
        if ((d.vec == nullptr) != (d.vec_out == nullptr)) return fail(NRM_EINVAL, "nrm_slab_reduce_multi: entry %d: vec and vec_out go together", i);
        nrm::SlabReduceParams& p = ps[(size_t)i];
        p.ws = d.ws; p.nsplit = d.nsplit; p.nj = d.nj; p.ldws = d.ldws; p.ni = d.ni; p.out = d.out; p.ors = d.out_istride; p.ocs = d.out_jstride;
        p.out2 = d.out2; p.ors2 = d.out2_istride; p.ocs2 = d.out2_jstride; p.sign2 = d.sign2; p.vec = d.vec; p.vec_out = d.vec_out;
    }
    return check_hip(nrm::slab_reduce_multi_launch(ps.data(), n, (hipStream_t)stream), "slab_reduce_multi");
}

// head fold: W' = W_o1 W_m2, b' = W_o1 b_m2 + b_o1 (head.hip)
int nrm_head_fold(const float* w_o1, const float* b_o1, const float* w_m2, const float* b_m2, int P, int Q, int R,
                  float* packed_fwd, float* packed_bwd, float* bias, nrm_stream_t stream) {
    if (!w_o1 || !w_m2 || !packed_fwd || !packed_bwd || !bias) return fail(NRM_EINVAL, "nrm_head_fold: null pointer");
    if (P <= 0 || Q <= 0 || R <= 0 || Q % 4 || !al16(w_o1))
        return fail(NRM_EINVAL, "nrm_head_fold: P=%d Q=%d R=%d (Q a multiple of 4, w_o1 16-byte aligned)", P, Q, R);
    const nrm::GemmNtPlan pf = nrm::gemm_nt_plan(P), pb = nrm::gemm_nt_plan(R);
    nrm::HeadFoldParams p = {};
    p.wo = w_o1; p.wm = w_m2; p.bo = b_o1; p.bm = b_m2; p.img_f = packed_fwd; p.img_b = packed_bwd; p.bias = bias;
    p.P = P; p.Q = Q; p.R = R; p.rows_f = pf.rows; p.kch_f = (R + 15) / 16; p.rows_b = pb.rows; p.kch_b = (P + 15) / 16;
    return check_hip(nrm::head_fold_launch(p, (hipStream_t)stream), "head_fold");
}

int nrm_head_fold_bwd(const float* dwp, int ldp, const float* dbp, const float* w_o1, const float* w_m2, const float* b_m2,
                      int P, int Q, int R, float* dw_o1, float* dw_m2, float* db_o1, float* db_m2, nrm_stream_t stream) {
    if (!dwp || !dbp || !w_o1 || !w_m2) return fail(NRM_EINVAL, "nrm_head_fold_bwd: null pointer");
    if (P <= 0 || Q <= 0 || R <= 0 || ldp % 4 || ldp < R || !al16(dwp))
        return fail(NRM_EINVAL, "nrm_head_fold_bwd: P=%d Q=%d R=%d ldp=%d (ldp a multiple of 4 covering R, 16-byte aligned rows)", P, Q, R, ldp);
    nrm::HeadSplitParams p = {};
    p.dwp = dwp; p.ldp = ldp; p.dbp = dbp; p.wo = w_o1; p.wm = w_m2; p.bm = b_m2; p.dwo = dw_o1; p.dwm = dw_m2; p.dbo = db_o1; p.dbm = db_m2;
    p.P = P; p.Q = Q; p.R = R;
    return check_hip(nrm::head_fold_bwd_launch(p, (hipStream_t)stream), "head_fold_bwd");
}

// ------------------------------------------------------------------------------------------- BatchNorm
static int check_bn(const char* fn, int R, int N, int ld) {
    if (R < 0 || N <= 0 || N % 4 || ld % 4 || ld < N) return fail(NRM_EINVAL, "%s: R=%d N=%d ld=%d (N, ld multiples of 4)", fn, R, N, ld);
    return NRM_OK;
}

int nrm_colreduce(int mode, const float* x, const float* dy, const float* mean, const float* rstd,
                  float* s0, float* s1, int R, int N, int ld, nrm_stream_t stream) {
    if (int rc = check_bn("nrm_colreduce", R, N, ld)) return rc;
    if (!x || !s0 || (mode >= 1 && !mean) || (mode == 2 && (!dy || !rstd || !s1)) || mode < 0 || mode > 2)
        return fail(NRM_EINVAL, "nrm_colreduce: bad argument for mode %d", mode);
    return check_hip(nrm::colred_launch(mode, x, dy, mean, rstd, s0, s1, R, N, ld, (hipStream_t)stream), "colreduce");
}

int nrm_bn_finalize(int stage, const float* s, float* out, float* running, int R, int N, float momentum, float eps,
                    nrm_stream_t stream) {
    if (!s || !out) return fail(NRM_EINVAL, "nrm_bn_finalize: null pointer");
    if ((stage != 0 && stage != 1) || R <= 0 || N <= 0) return fail(NRM_EINVAL, "nrm_bn_finalize: stage=%d R=%d N=%d", stage, R, N);
    return check_hip(nrm::bn_finalize_launch(stage, s, out, running, R, N, momentum, eps, (hipStream_t)stream), "bn_finalize");
}

int nrm_mul_bwd(const float* dy, int lddy, const float* g, int ldg, const float* e, int lde, float* dg, float* de, int ldo,
                int R, int N, nrm_stream_t stream) {
    if (!dy || !g || !e || !dg || !de) return fail(NRM_EINVAL, "nrm_mul_bwd: null pointer");
    if (R < 0 || N <= 0 || N % 4 || lddy % 4 || ldg % 4 || lde % 4 || ldo % 4 || lddy < N || ldg < N || lde < N || ldo < N ||
        !al16(dy) || !al16(g) || !al16(e) || !al16(dg) || !al16(de))
        return fail(NRM_EINVAL, "nrm_mul_bwd: R=%d N=%d (N and leading dimensions multiples of 4, 16-byte aligned rows)", R, N);
    return check_hip(nrm::mul_bwd_launch(dy, g, e, dg, de, R, N, lddy, ldg, lde, ldo, (hipStream_t)stream), "mul_bwd");
}

int nrm_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                 float* y, int R, int N, int ld, nrm_stream_t stream) {
    if (int rc = check_bn("nrm_bn_apply", R, N, ld)) return rc;
    if (!x || !mean || !rstd || !gamma || !beta || !y) return fail(NRM_EINVAL, "nrm_bn_apply: null pointer");
    return check_hip(nrm::bn_apply_launch(x, mean, rstd, gamma, beta, y, R, N, ld, (hipStream_t)stream), "bn_apply");
}

int nrm_bn_backward(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                    const float* s0, const float* s1, const float* add, float* dx, int R, int N, int ld, int training,
                    nrm_stream_t stream) {
    if (int rc = check_bn("nrm_bn_backward", R, N, ld)) return rc;
    if (!dy || !rstd || !gamma || !dx || (training && (!x || !mean || !s0 || !s1)))
        return fail(NRM_EINVAL, "nrm_bn_backward: null pointer");
    return check_hip(nrm::bn_bwd_launch(x, dy, mean, rstd, gamma, s0, s1, add, dx, R, N, ld, training, (hipStream_t)stream), "bn_backward");
}


int nrm_concat_cols(const float* const* srcs, const long* lds, const int* widths, int n, float* out, int ldo, long R,
                    nrm_stream_t stream) {
    if (!srcs || !lds || !widths || !out) return fail(NRM_EINVAL, "nrm_concat_cols: null pointer");
    if (n < 1 || n > nrm::CONCAT_MAX || R < 0) return fail(NRM_EINVAL, "nrm_concat_cols: n=%d (1..%d) R=%ld", n, nrm::CONCAT_MAX, R);
    nrm::ConcatTable tab = {};
    int total = 0;
    for (int i = 0; i < n; ++i) {
        if (!srcs[i] || widths[i] <= 0 || lds[i] < widths[i]) return fail(NRM_EINVAL, "nrm_concat_cols: part %d (width %d, ld %ld)", i, widths[i], lds[i]);
        tab.src[i] = srcs[i]; tab.ld[i] = lds[i]; tab.start[i] = total;
        total += widths[i];
    }
    tab.n = n;
    if (ldo < total) return fail(NRM_EINVAL, "nrm_concat_cols: ldo=%d < %d columns", ldo, total);
    return check_hip(nrm::concat_cols_launch(tab, out, R, ldo, total, (hipStream_t)stream), "concat_cols");
}

// ------------------------------------------------------------------------------------------- pool / loss / Adam
int nrm_pool_bmm(const float* W, long wsb, long wsi, long wsj, const float* X, int ldx, float* out,
                 int B, int I, int J, int D, int accumulate, nrm_stream_t stream) {
    if (!W || !X || !out) return fail(NRM_EINVAL, "nrm_pool_bmm: null pointer");
    if (B < 0 || I <= 0 || J <= 0 || D <= 0 || D % 4 || B > 65535) return fail(NRM_EINVAL, "nrm_pool_bmm: B=%d I=%d J=%d D=%d", B, I, J, D);
    if (ldx < D || ldx % 4 || !al16(X) || (long)J * ldx * 4 >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_pool_bmm: ldx=%d (>= D, a multiple of 4, X 16-byte aligned, J*ldx*4 < 2^31)", ldx);
    return check_hip(nrm::bmm_rows_launch(W, wsb, wsi, wsj, X, (long)J * ldx, ldx, out, (long)I * D, D, B, I, J, D, accumulate,
                                          (hipStream_t)stream), "pool_bmm");
}

int nrm_pool_bmm_ragged(const float* s, const float* h, float* out, const int* cand_off, int B, int N, int max_count, int H, int D,
                        nrm_stream_t stream) {
    if (!s || !h || !out || !cand_off) return fail(NRM_EINVAL, "nrm_pool_bmm_ragged: null pointer");
    if (B < 0 || N < 0 || max_count < 0 || max_count > N || H <= 0 || D <= 0 || D % 4 || B > 65535)
        return fail(NRM_EINVAL, "nrm_pool_bmm_ragged: B=%d N=%d max_count=%d H=%d D=%d", B, N, max_count, H, D);
    if (!al16(h) || !al16(out) || (long)H * D * 4 >= (1L << 31) || (long)N * H >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_pool_bmm_ragged: h and out must be 16-byte aligned, H*D*4 and N*H below 2^31");
    return check_hip(nrm::bmm_rows_ragged_launch(s, H, h, (long)H * D, D, out, D, cand_off, B, N, max_count, H, D, (hipStream_t)stream), "pool_bmm_ragged");
}

int nrm_pool_rowdot(const float* g, int ldg, const float* h, float* ds, int B, int T, int H, int D, float* zero_out, int zero_n,
                    nrm_stream_t stream) {
    if (!g || !h || !ds) return fail(NRM_EINVAL, "nrm_pool_rowdot: null pointer");
    if (B < 0 || T <= 0 || H <= 0 || D <= 0 || D % 4 || D > 1024 || B > 65535) return fail(NRM_EINVAL, "nrm_pool_rowdot: B=%d T=%d H=%d D=%d", B, T, H, D);
    if (ldg < D || ldg % 4 || !al16(g) || (long)T * ldg * 4 >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_pool_rowdot: ldg=%d (>= D, a multiple of 4, g 16-byte aligned, T*ldg*4 < 2^31)", ldg);
    if (zero_n < 0 || (zero_n > 0 && !zero_out)) return fail(NRM_EINVAL, "nrm_pool_rowdot: zero_n=%d without zero_out", zero_n);
    return check_hip(nrm::rowdot_launch(g, (long)T * ldg, ldg, h, (long)H * D, D, ds, B, T, H, D, zero_out, zero_n, (hipStream_t)stream), "pool_rowdot");
}

int nrm_small_linear_relu_fwd(const void* x, int x_is_f64, const float* weight, const float* bias, float* y, long R, int K, int N, int ldy,
                              nrm_stream_t stream) {
    if (!x || !weight || !y) return fail(NRM_EINVAL, "nrm_small_linear_relu_fwd: null pointer");
    if (R < 0 || K < 1 || K > 4 || N < 1 || N > 8 || ldy < N) return fail(NRM_EINVAL, "nrm_small_linear_relu_fwd: R=%ld K=%d N=%d ldy=%d (K <= 4, N <= 8)", R, K, N, ldy);
    return check_hip(nrm::small_linear_relu_fwd_launch(x, x_is_f64, weight, bias, y, R, K, N, ldy, (hipStream_t)stream), "small_linear_relu_fwd");
}

int nrm_small_linear_relu_bwd(const void* x, int x_is_f64, const float* weight, const float* bias, const float* dy, int lddy, long R,
                              int K, int N, float* dwb, nrm_stream_t stream) {
    if (!x || !weight || !dy || !dwb) return fail(NRM_EINVAL, "nrm_small_linear_relu_bwd: null pointer");
    if (R < 0 || K < 1 || K > 4 || N < 1 || N > 8 || lddy < N) return fail(NRM_EINVAL, "nrm_small_linear_relu_bwd: R=%ld K=%d N=%d lddy=%d (K <= 4, N <= 8)", R, K, N, lddy);
    return check_hip(nrm::small_linear_relu_bwd_launch(x, x_is_f64, weight, bias, dy, lddy, R, K, N, dwb, (hipStream_t)stream), "small_linear_relu_bwd");
}

int nrm_loss_fwd_bwd(const float* out, int out_stride, const void* label, int label_is_f64, const long* user_id, const float* delta,
                     long n_delta, float alpha, int B, int T, float* loss_sum, float* dout, int dout_stride, float* ddelta, int* err,
                     nrm_stream_t stream) {
    if (!out || !label || !user_id || !delta || !loss_sum || !dout || !ddelta || !err) return fail(NRM_EINVAL, "nrm_loss_fwd_bwd: null pointer");
    if (B < 0 || T <= 0 || n_delta < 1 || (long)B * T >= (1L << 29))
        return fail(NRM_EINVAL, "nrm_loss_fwd_bwd: B=%d T=%d n_delta=%ld (T >= 1, n_delta >= 1, B*T < 2^29)", B, T, n_delta);
    if (out_stride < 1 || dout_stride < 1 || (dout_stride == 4 && !al16(dout)))
        return fail(NRM_EINVAL, "nrm_loss_fwd_bwd: out_stride=%d dout_stride=%d (>= 1; dout 16-byte aligned for stride 4)", out_stride, dout_stride);
    return check_hip(nrm::loss_launch(out, out_stride, label, label_is_f64, user_id, delta, n_delta, alpha, B, T, loss_sum, dout, dout_stride,
                                      ddelta, err, (hipStream_t)stream), "loss");
}

int nrm_adam_step(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, int zero_grad, nrm_stream_t stream) {
    if (!p || !g || !m || !v) return fail(NRM_EINVAL, "nrm_adam_step: null pointer");
    if (n < 0 || n % 4 || step < 1 || !al16(p) || !al16(g) || !al16(m) || !al16(v))
        return fail(NRM_EINVAL, "nrm_adam_step: n=%ld step=%d (n %% 4 == 0, step >= 1, 16-byte aligned buffers)", n, step);
    return check_hip(nrm::adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, zero_grad, (hipStream_t)stream), "adam");
}


int nrm_gather_flat(const float* const* srcs, const long* offsets, const long* counts, int n, float* flat, long flat_n,
                    nrm_stream_t stream) {
    if ((n > 0 && (!srcs || !offsets || !counts)) || !flat) return fail(NRM_EINVAL, "nrm_gather_flat: null pointer");
    if (n < 0) return fail(NRM_EINVAL, "nrm_gather_flat: n=%d", n);
    for (int lo = 0; lo < n; lo += nrm::GATHER_MAX) {
        const int m = n - lo < nrm::GATHER_MAX ? n - lo : nrm::GATHER_MAX;
        nrm::GatherTable tab;
        long mx = 0;
        for (int i = 0; i < m; ++i) {
            if (offsets[lo + i] < 0 || counts[lo + i] < 0 || offsets[lo + i] + counts[lo + i] > flat_n)
                return fail(NRM_EINVAL, "nrm_gather_flat: entry %d (offset %ld, count %ld) leaves the flat buffer of %ld floats",
                            lo + i, offsets[lo + i], counts[lo + i], flat_n);
            tab.src[i] = srcs[lo + i]; tab.off[i] = offsets[lo + i]; tab.cnt[i] = counts[lo + i];
            if (counts[lo + i] > mx) mx = counts[lo + i];
        }
        if (int rc = check_hip(nrm::gather_flat_launch(tab, m, mx, flat, (hipStream_t)stream), "gather_flat")) return rc;
    }
    return NRM_OK;
}

int nrm_adam_step_dev(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float* state, int zero_grad, nrm_stream_t stream) {
    if (!p || !g || !m || !v || !state) return fail(NRM_EINVAL, "nrm_adam_step_dev: null pointer");
    if (n < 0 || n % 4 || !al16(p) || !al16(g) || !al16(m) || !al16(v))
        return fail(NRM_EINVAL, "nrm_adam_step_dev: n=%ld (n %% 4 == 0, 16-byte aligned buffers)", n);
    return check_hip(nrm::adam_dev_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, state, zero_grad, (hipStream_t)stream), "adam_dev");
}

int nrm_row_auc(const float* score, const float* label, const int* len, int B, int T, float* auc, int* top1,
                nrm_stream_t stream) {
    if (!score || !label || !auc || !top1) return fail(NRM_EINVAL, "nrm_row_auc: null pointer");
    if (B < 0 || T <= 0) return fail(NRM_EINVAL, "nrm_row_auc: B=%d T=%d", B, T);
    return check_hip(nrm::row_auc_launch(score, label, len, B, T, auc, top1, (hipStream_t)stream), "row_auc");
}

int nrm_ensemble_rank_max_candidates(void) { return nrm::ENSEMBLE_MAX_CANDIDATES; }

int nrm_ensemble_rank(const float* const* logits, const long* row_stride, const long* col_stride, int M, const int* empty,
                      const float* label, int B, int T, float* score, int* rank, int* live, float* metrics, nrm_stream_t stream) {
    if (!logits || !row_stride || !score || !rank || !live) return fail(NRM_EINVAL, "nrm_ensemble_rank: null pointer");
    if (M < 1 || M > nrm::ENSEMBLE_MAX_MODELS) return fail(NRM_EINVAL, "nrm_ensemble_rank: M=%d models (1 .. %d)", M, nrm::ENSEMBLE_MAX_MODELS);
    if (B < 0 || T <= 0) return fail(NRM_EINVAL, "nrm_ensemble_rank: B=%d T=%d", B, T);
    if (T > nrm::ENSEMBLE_MAX_CANDIDATES)
        return fail(NRM_EINVAL, "nrm_ensemble_rank: T=%d candidates exceed the cap of %d (nrm_ensemble_rank_max_candidates)", T, nrm::ENSEMBLE_MAX_CANDIDATES);
    if ((label == nullptr) != (metrics == nullptr)) return fail(NRM_EINVAL, "nrm_ensemble_rank: label and metrics must be given together or both be NULL");
    nrm::EnsembleLogits lg = {};
    for (int m = 0; m < M; ++m) {
        if (!logits[m]) return fail(NRM_EINVAL, "nrm_ensemble_rank: logits[%d] is a null pointer", m);
        const long cs = col_stride ? col_stride[m] : 1;
        if (row_stride[m] < 0 || cs < 1) return fail(NRM_EINVAL, "nrm_ensemble_rank: model %d has row stride %ld, column stride %ld (need >= 0, >= 1)", m, row_stride[m], cs);
        lg.ptr[m] = logits[m]; lg.row_stride[m] = row_stride[m]; lg.col_stride[m] = cs;
    }
    return check_hip(nrm::ensemble_rank_launch(lg, M, empty, label, B, T, score, rank, live, metrics, (hipStream_t)stream), "ensemble_rank");
}

int nrm_pool_bmm_hragged(const float* s, const float* h, float* out, const int* cand_off, const int* hist_off, const int* hist_mult,
                         const int* tile_pre, int B, int N, int max_count, int R, int Mt, int k_max, int D, nrm_stream_t stream) {
    if (!s || !h || !out || !cand_off || !hist_off || !hist_mult || !tile_pre) return fail(NRM_EINVAL, "nrm_pool_bmm_hragged: null pointer");
    if (B < 0 || N < 0 || max_count < 0 || max_count > N || R < 0 || Mt < 0 || k_max < 0 || k_max > R || D <= 0 || D % 4)
        return fail(NRM_EINVAL, "nrm_pool_bmm_hragged: B=%d N=%d max_count=%d R=%d Mt=%d k_max=%d D=%d", B, N, max_count, R, Mt, k_max, D);
    if (((uintptr_t)h | (uintptr_t)out) & 15 || (long)R * D * 4 >= (1L << 31) || 16L * Mt >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_pool_bmm_hragged: h and out must be 16-byte aligned, R*D*4 and 16*Mt below 2^31");
    if (R == 0 || Mt == 0) return NRM_OK;
    return check_hip(nrm::bmm_rows_hragged_launch(s, h, D, out, D, cand_off, hist_off, hist_mult, tile_pre, B, N, max_count, R, Mt, k_max, D,
                                                  (hipStream_t)stream), "pool_bmm_hragged");
}

int nrm_history_len(const void* x_history, int cols, int is_f64, int B, int H, int* hist_len, nrm_stream_t stream) {
    if (B < 0 || H < 0 || cols <= 0) return fail(NRM_EINVAL, "nrm_history_len: B=%d H=%d cols=%d", B, H, cols);
    const long words = (long)cols * (is_f64 ? 2 : 1);
    if ((long)H * words >= (1L << 31)) return fail(NRM_EINVAL, "nrm_history_len: H*cols=%ld words of one impression exceed 2^31", (long)H * words);
    if ((B > 0 && !hist_len) || (B > 0 && H > 0 && !x_history)) return fail(NRM_EINVAL, "nrm_history_len: null pointer");
    if ((uintptr_t)x_history & 3) return fail(NRM_EINVAL, "nrm_history_len: x_history must be 4-byte aligned");
    return check_hip(nrm::history_len_launch((const unsigned*)x_history, B, H, (int)words, hist_len, (hipStream_t)stream), "history_len");
}

int nrm_history_gather(const void* x_history, int cols, int is_f64, const int* hist_off, int B, int H, int R, int k_max, void* xh_compact,
                       nrm_stream_t stream) {
    if (B < 0 || H < 0 || cols <= 0 || R < 0 || k_max < 0 || k_max > H || (long)R > (long)B * H)
        return fail(NRM_EINVAL, "nrm_history_gather: B=%d H=%d cols=%d R=%d k_max=%d (0 <= k_max <= H, R <= B*H)", B, H, cols, R, k_max);
    if ((long)cols * 2 >= (1L << 31)) return fail(NRM_EINVAL, "nrm_history_gather: cols=%d", cols);
    if (!hist_off || (R > 0 && (!x_history || !xh_compact))) return fail(NRM_EINVAL, "nrm_history_gather: null pointer");
    return check_hip(nrm::history_gather_launch((const unsigned*)x_history, (unsigned*)xh_compact, cols * (is_f64 ? 2 : 1), hist_off, B, H, R, k_max,
                                                (hipStream_t)stream), "history_gather");
}

int nrm_history_tiles(const int* cand_imp, const int* cand_off, const int* hist_off, const int* tile_pre, int B, int N, int R, int Mt,
                      void* tile_tab, nrm_stream_t stream) {
    if (B < 0 || N < 0 || R < 0 || Mt < 0) return fail(NRM_EINVAL, "nrm_history_tiles: B=%d N=%d R=%d Mt=%d", B, N, R, Mt);
    if (16L * Mt >= (1L << 31)) return fail(NRM_EINVAL, "nrm_history_tiles: 16*Mt=%ld exceeds 2^31 rows", 16L * Mt);
    if (!cand_imp || !cand_off || !hist_off || !tile_pre || (Mt > 0 && !tile_tab)) return fail(NRM_EINVAL, "nrm_history_tiles: null pointer");
    if ((uintptr_t)tile_tab & 15) return fail(NRM_EINVAL, "nrm_history_tiles: tile_tab must be 16-byte aligned");
    return check_hip(nrm::history_tiles_launch(cand_imp, cand_off, hist_off, tile_pre, B, N, R, Mt, (int4*)tile_tab, (hipStream_t)stream), "history_tiles");
}

// ---- training on compacted histories
int nrm_history_gather_groups(const void* x_history, int cols, int is_f64, const int* src_imp, const int* group_b0, const int* group_row_off,
                              const int* group_h, int G, int B, int H, int R, void* xh_arena, nrm_stream_t stream) {
    if (B < 0 || H < 0 || cols <= 0 || R < 0 || G < 0 || G > nrm::HISTORY_GROUPS_MAX || (long)R > (long)B * H)
        return fail(NRM_EINVAL, "nrm_history_gather_groups: B=%d H=%d cols=%d R=%d G=%d (0 <= G <= %d, R <= B*H)", B, H, cols, R, G, nrm::HISTORY_GROUPS_MAX);
    if ((long)cols * 2 >= (1L << 31)) return fail(NRM_EINVAL, "nrm_history_gather_groups: cols=%d", cols);
    if (R > 0 && (!x_history || !xh_arena || !src_imp || !group_b0 || !group_row_off || !group_h || G == 0))
        return fail(NRM_EINVAL, "nrm_history_gather_groups: null pointer (or R=%d rows in G=0 groups)", R);
    return check_hip(nrm::history_gather_groups_launch((const unsigned*)x_history, (unsigned*)xh_arena, cols * (is_f64 ? 2 : 1), src_imp, group_b0,
                                                       group_row_off, group_h, G, B, H, R, (hipStream_t)stream), "history_gather_groups");
}

int nrm_pool_bmm_wlast(const float* W, long wsb, long wsi, long wsj, const float* X, int ldx, float* out,
                       int B, int I, int J, int D, int accumulate, float wlast, int wlast_row, nrm_stream_t stream) {
    if (!W || !X || !out) return fail(NRM_EINVAL, "nrm_pool_bmm_wlast: null pointer");
    if (B < 0 || I <= 0 || J <= 0 || D <= 0 || D % 4 || B > 65535) return fail(NRM_EINVAL, "nrm_pool_bmm_wlast: B=%d I=%d J=%d D=%d", B, I, J, D);
    if (ldx < D || ldx % 4 || !al16(X) || (long)J * ldx * 4 >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_pool_bmm_wlast: ldx=%d (>= D, a multiple of 4, X 16-byte aligned, J*ldx*4 < 2^31)", ldx);
    if (!(wlast >= 1.f) || (wlast_row != 0 && wlast_row != 1))
        return fail(NRM_EINVAL, "nrm_pool_bmm_wlast: wlast=%g wlast_row=%d (wlast >= 1: the rows the last one stands for; wlast_row 0 or 1)", (double)wlast, wlast_row);
    return check_hip(nrm::bmm_rows_wlast_launch(W, wsb, wsi, wsj, X, (long)J * ldx, ldx, out, (long)I * D, D, B, I, J, D, accumulate, wlast, wlast_row,
                                                (hipStream_t)stream), "pool_bmm_wlast");
}

int nrm_pool_rowdot_wlast(const float* g, int ldg, const float* h, float* ds, int B, int T, int H, int D, float* zero_out, int zero_n,
                          float wlast, nrm_stream_t stream) {
    if (!g || !h || !ds) return fail(NRM_EINVAL, "nrm_pool_rowdot_wlast: null pointer");
    if (B < 0 || T <= 0 || H <= 0 || D <= 0 || D % 4 || D > 1024 || B > 65535) return fail(NRM_EINVAL, "nrm_pool_rowdot_wlast: B=%d T=%d H=%d D=%d", B, T, H, D);
    if (ldg < D || ldg % 4 || !al16(g) || (long)T * ldg * 4 >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_pool_rowdot_wlast: ldg=%d (>= D, a multiple of 4, g 16-byte aligned, T*ldg*4 < 2^31)", ldg);
    if (zero_n < 0 || (zero_n > 0 && !zero_out)) return fail(NRM_EINVAL, "nrm_pool_rowdot_wlast: zero_n=%d without zero_out", zero_n);
    if (!(wlast >= 1.f)) return fail(NRM_EINVAL, "nrm_pool_rowdot_wlast: wlast=%g (>= 1: the rows the last one stands for)", (double)wlast);
    return check_hip(nrm::rowdot_wlast_launch(g, (long)T * ldg, ldg, h, (long)H * D, D, ds, B, T, H, D, zero_out, zero_n, wlast, (hipStream_t)stream),
                     "pool_rowdot_wlast");
}

// ---- training on compacted candidate lists
int nrm_candidate_gather_groups(const void* x_target, int target_cols, int target_is_f64, const void* x_global, int global_cols, int global_is_f64,
                                const void* label, int label_is_f64, const int* src_imp, const int* group_b0, const int* group_row_off,
                                const int* group_t, int G, int B, int T, int N, void* xt_arena, void* xg_arena, void* label_arena, float* row_weight,
                                int* flag, nrm_stream_t stream) {
    if (B < 0 || T <= 0 || N < 0 || G < 0 || G > nrm::HISTORY_GROUPS_MAX || target_cols <= 0 || global_cols <= 0 || (long)N > (long)B * T ||
        (long)B * T >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_candidate_gather_groups: B=%d T=%d N=%d G=%d target_cols=%d global_cols=%d (0 <= G <= %d, N <= B*T < 2^31)", B, T, N, G,
                    target_cols, global_cols, nrm::HISTORY_GROUPS_MAX);
    if ((long)target_cols * 2 >= (1L << 31) || (long)global_cols * 2 >= (1L << 31))
        return fail(NRM_EINVAL, "nrm_candidate_gather_groups: target_cols=%d global_cols=%d", target_cols, global_cols);
    if (!flag || (B > 0 && (!x_target || !x_global || !label || !src_imp || !group_b0 || !group_row_off || !group_t || G == 0)) ||
        (N > 0 && (!xt_arena || !xg_arena || !label_arena || !row_weight)))
        return fail(NRM_EINVAL, "nrm_candidate_gather_groups: null pointer (or B=%d impressions in G=0 groups)", B);
    nrm::CandidateGatherParams p;
    p.xt = (const unsigned*)x_target; p.xg = (const unsigned*)x_global; p.lab = (const unsigned*)label;
    p.xt_a = (unsigned*)xt_arena; p.xg_a = (unsigned*)xg_arena; p.lab_a = (unsigned*)label_arena; p.roww = row_weight;
    p.wt = target_cols * (target_is_f64 ? 2 : 1); p.wg = global_cols * (global_is_f64 ? 2 : 1); p.wl = label_is_f64 ? 2 : 1;
    p.src_imp = src_imp; p.b0 = group_b0; p.row_off = group_row_off; p.tg = group_t; p.G = G; p.B = B; p.T = T; p.N = N; p.flag = flag;
    return check_hip(nrm::candidate_gather_groups_launch(p, (hipStream_t)stream), "candidate_gather_groups");
}

int nrm_colreduce_roww(int mode, const float* x, const float* mean, const float* row_weight, float* s0, int R, int N, int ld, nrm_stream_t stream) {
    if (int rc = check_bn("nrm_colreduce_roww", R, N, ld)) return rc;
    if (!x || !s0 || !row_weight || (mode == 1 && !mean) || mode < 0 || mode > 1)
        return fail(NRM_EINVAL, "nrm_colreduce_roww: bad argument for mode %d (modes 0 and 1 have a row-weight form)", mode);
    return check_hip(nrm::colred_roww_launch(mode, x, mean, row_weight, s0, R, N, ld, (hipStream_t)stream), "colreduce_roww");
}

int nrm_bn_backward_roww(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma, const float* s0,
                         const float* s1, const float* add, const float* row_weight, float* dx, int R, int n_rows, int N, int ld,
                         nrm_stream_t stream) {
    if (int rc = check_bn("nrm_bn_backward_roww", R, N, ld)) return rc;
    if (!dy || !rstd || !gamma || !dx || !x || !mean || !s0 || !s1 || !row_weight) return fail(NRM_EINVAL, "nrm_bn_backward_roww: null pointer");
    if (n_rows < R) return fail(NRM_EINVAL, "nrm_bn_backward_roww: n_rows=%d < R=%d (the batch has at least the rows of the launch)", n_rows, R);
    return check_hip(nrm::bn_bwd_roww_launch(x, dy, mean, rstd, gamma, s0, s1, add, row_weight, dx, R, n_rows, N, ld, (hipStream_t)stream),
                     "bn_backward_roww");
}

int nrm_loss_fwd_bwd_wlast(const float* out, int out_stride, const void* label, int label_is_f64, const long* user_id, const float* delta,
                           long n_delta, float alpha, int B, int T, float wlast, float inv_n, float* loss_sum, float* dout, int dout_stride,
                           float* ddelta, int* err, nrm_stream_t stream) {
    if (!out || !label || !user_id || !delta || !loss_sum || !dout || !ddelta || !err) return fail(NRM_EINVAL, "nrm_loss_fwd_bwd_wlast: null pointer");
    if (B < 0 || T <= 0 || n_delta < 1 || (long)B * T >= (1L << 29))
        return fail(NRM_EINVAL, "nrm_loss_fwd_bwd_wlast: B=%d T=%d n_delta=%ld (T >= 1, n_delta >= 1, B*T < 2^29)", B, T, n_delta);
    if (out_stride < 1 || dout_stride < 1 || (dout_stride == 4 && !al16(dout)))
        return fail(NRM_EINVAL, "nrm_loss_fwd_bwd_wlast: out_stride=%d dout_stride=%d (>= 1; dout 16-byte aligned for stride 4)", out_stride, dout_stride);
    if (!(wlast >= 1.f) || !(inv_n > 0.f))
        return fail(NRM_EINVAL, "nrm_loss_fwd_bwd_wlast: wlast=%g inv_n=%g (wlast >= 1: the candidates the last column stands for; inv_n > 0)", (double)wlast,
                    (double)inv_n);
    return check_hip(nrm::loss_wlast_launch(out, out_stride, label, label_is_f64, user_id, delta, n_delta, alpha, B, T, wlast, inv_n, loss_sum, dout,
                                            dout_stride, ddelta, err, (hipStream_t)stream), "loss_wlast");
}

int nrm_ensemble_rank_ragged(const float* const* logits, const long* col_stride, int M, const int* cand_off, const int* pad_mult, int N,
                             const float* label, int B, int T, float* score, int* rank, int* live, float* metrics, nrm_stream_t stream) {
    if (!logits || !cand_off || !pad_mult || !score || !rank || !live) return fail(NRM_EINVAL, "nrm_ensemble_rank_ragged: null pointer");
    if (M < 1 || M > nrm::ENSEMBLE_MAX_MODELS) return fail(NRM_EINVAL, "nrm_ensemble_rank_ragged: M=%d models (1 .. %d)", M, nrm::ENSEMBLE_MAX_MODELS);
    if (B < 0 || T <= 0 || N < 0) return fail(NRM_EINVAL, "nrm_ensemble_rank_ragged: B=%d T=%d N=%d", B, T, N);
    if (T > nrm::ENSEMBLE_MAX_CANDIDATES)
        return fail(NRM_EINVAL, "nrm_ensemble_rank_ragged: T=%d candidates exceed the cap of %d (nrm_ensemble_rank_max_candidates)", T, nrm::ENSEMBLE_MAX_CANDIDATES);
    if ((label == nullptr) != (metrics == nullptr)) return fail(NRM_EINVAL, "nrm_ensemble_rank_ragged: label and metrics must be given together or both be NULL");
    nrm::EnsembleLogits lg = {};
    for (int m = 0; m < M; ++m) {
        if (!logits[m] && N > 0) return fail(NRM_EINVAL, "nrm_ensemble_rank_ragged: logits[%d] is a null pointer", m);
        const long cs = col_stride ? col_stride[m] : 1;
        if (cs < 1) return fail(NRM_EINVAL, "nrm_ensemble_rank_ragged: model %d has entry stride %ld (need >= 1)", m, cs);
        lg.ptr[m] = logits[m]; lg.row_stride[m] = 0; lg.col_stride[m] = cs;
    }
    return check_hip(nrm::ensemble_rank_ragged_launch(lg, M, cand_off, pad_mult, N, label, B, T, score, rank, live, metrics, (hipStream_t)stream),
                     "ensemble_rank_ragged");
}

int nrm_compact_gather(const void* x_target, int target_cols, int target_is_f64, const void* x_global, int global_cols, int global_is_f64,
                       const int* cand_off, const int* pad_mult, int B, int T, int trim, int N,
                       void* xt_compact, void* xg_compact, int* flag, nrm_stream_t stream) {
    if (B < 0 || T <= 0 || trim < 0 || trim > T || N < 0 || target_cols <= 0 || global_cols <= 0)
        return fail(NRM_EINVAL, "nrm_compact_gather: B=%d T=%d trim=%d N=%d target_cols=%d global_cols=%d", B, T, trim, N, target_cols, global_cols);
    if ((long)N > (long)B * (T - trim)) return fail(NRM_EINVAL, "nrm_compact_gather: N=%d compact rows exceed the B*(T - trim)=%ld kept cells", N, (long)B * (T - trim));
    if (!cand_off || !pad_mult || !flag || !x_target || !x_global || (N > 0 && (!xt_compact || !xg_compact))) return fail(NRM_EINVAL, "nrm_compact_gather: null pointer");
    nrm::CompactGatherParams p;
    p.xt = (const unsigned*)x_target; p.xg = (const unsigned*)x_global; p.xt_c = (unsigned*)xt_compact; p.xg_c = (unsigned*)xg_compact;
    p.wt = target_cols * (target_is_f64 ? 2 : 1); p.wg = global_cols * (global_is_f64 ? 2 : 1);
    p.cand_off = cand_off; p.pad_mult = pad_mult; p.B = B; p.T = T; p.Tp = T - trim; p.N = N; p.flag = flag;
    return check_hip(nrm::compact_gather_launch(p, (hipStream_t)stream), "compact_gather");
}

// ------------------------------------------------------------------------------------------- embedding front end
static int check_fe(const char* fn, int nrows, int xcols, int P, int n_sub, int behaviour, int e0, int e1, int e2, int e3) {
    if (nrows < 0 || P <= 0 || n_sub < 0 || e0 <= 0 || e1 <= 0 || e2 <= 0 || e3 <= 0)
        return fail(NRM_EINVAL, "%s: bad dimension", fn);
    if (n_sub > 16) return fail(NRM_EINVAL, "%s: n_sub=%d (<= 16 sub-category slots)", fn, n_sub);
    const int need = 4 + P + 1 + n_sub + 3 + 1 + (behaviour ? 2 : 0);
    if (xcols < need) return fail(NRM_EINVAL, "%s: packed rows have %d columns, layout needs %d", fn, xcols, need);
    return NRM_OK;
}

int nrm_frontend_fwd(const void* x, int x_is_f64, int nrows, int xcols, int P, int n_sub, int behaviour,
                     const float* cat_tab, int n_cat, int e0, const float* sen_w, const float* sen_b, int e1,
                     const float* type_tab, int n_type, int e2,
                     const float* year_tab, const float* month_tab, const float* day_tab, const float* hour_tab,
                     int n_year, int n_month, int n_day, int n_hour, int e3,
                     float* lab, int ldlab, float* ti, int ldti, int* err, nrm_stream_t stream) {
    if (int rc = check_fe("nrm_frontend_fwd", nrows, xcols, P, n_sub, behaviour, e0, e1, e2, e3)) return rc;
    if (!x || !cat_tab || !sen_w || !sen_b || !type_tab || !year_tab || !month_tab || !day_tab || !hour_tab || !lab || !ti || !err)
        return fail(NRM_EINVAL, "nrm_frontend_fwd: null pointer");
    if (ldlab < e0 + e1 + e2 + e3 + (behaviour ? 2 : 0) || ldti < P) return fail(NRM_EINVAL, "nrm_frontend_fwd: ldlab=%d ldti=%d too small", ldlab, ldti);
    nrm::FrontendParams p = {};
    p.cat_tab = cat_tab; p.sen_w = sen_w; p.sen_b = sen_b; p.type_tab = type_tab;
    p.year_tab = year_tab; p.month_tab = month_tab; p.day_tab = day_tab; p.hour_tab = hour_tab;
    p.n_cat = n_cat; p.n_type = n_type; p.n_year = n_year; p.n_month = n_month; p.n_day = n_day; p.n_hour = n_hour;
    p.e0 = e0; p.e1 = e1; p.e2 = e2; p.e3 = e3; p.P = P; p.n_sub = n_sub; p.xcols = xcols; p.behaviour = behaviour;
    p.lab = lab; p.ldlab = ldlab; p.ti = ti; p.ldti = ldti; p.err = err;
    return check_hip(nrm::frontend_fwd_launch(p, x, x_is_f64, nrows, (hipStream_t)stream), "frontend_fwd");
}

int nrm_frontend_bwd(const void* x, int x_is_f64, int nrows, int xcols, int P, int n_sub, int behaviour,
                     const float* dlab, int lddl, const float* sen_w, const float* sen_b,
                     int n_cat, int e0, int e1, int n_type, int e2, int n_year, int n_month, int n_day, int n_hour, int e3,
                     float* d_cat_tab, float* d_sen_w, float* d_sen_b, float* d_type_tab,
                     float* d_year_tab, float* d_month_tab, float* d_day_tab, float* d_hour_tab, nrm_stream_t stream) {
    if (int rc = check_fe("nrm_frontend_bwd", nrows, xcols, P, n_sub, behaviour, e0, e1, e2, e3)) return rc;
    const int n_small = !!d_sen_w + !!d_sen_b + !!d_type_tab + !!d_year_tab + !!d_month_tab + !!d_day_tab + !!d_hour_tab;
    if (!x || !dlab || !sen_w || !sen_b || (n_small != 7 && (n_small != 0 || !d_cat_tab)))
        return fail(NRM_EINVAL, "nrm_frontend_bwd: null pointer");
    if (lddl < e0 + e1 + e2 + e3) return fail(NRM_EINVAL, "nrm_frontend_bwd: lddl=%d too small", lddl);
    nrm::FrontendParams p = {};
    p.sen_w = sen_w; p.sen_b = sen_b;
    p.d_cat_tab = d_cat_tab; p.d_sen_w = d_sen_w; p.d_sen_b = d_sen_b; p.d_type_tab = d_type_tab;
    p.d_year_tab = d_year_tab; p.d_month_tab = d_month_tab; p.d_day_tab = d_day_tab; p.d_hour_tab = d_hour_tab;
    p.n_cat = n_cat; p.n_type = n_type; p.n_year = n_year; p.n_month = n_month; p.n_day = n_day; p.n_hour = n_hour;
    p.e0 = e0; p.e1 = e1; p.e2 = e2; p.e3 = e3; p.P = P; p.n_sub = n_sub; p.xcols = xcols; p.behaviour = behaviour;
    return check_hip(nrm::frontend_bwd_launch(p, x, x_is_f64, dlab, lddl, nrows, (hipStream_t)stream), "frontend_bwd");
}

static nrm::FrontendParams tab_dims(int n_sub, int e1, int n_type, int e2, int n_year, int n_month, int n_day, int n_hour, int e3) {
    nrm::FrontendParams p = {};
    p.n_type = n_type; p.n_year = n_year; p.n_month = n_month; p.n_day = n_day; p.n_hour = n_hour;
    p.e1 = e1; p.e2 = e2; p.e3 = e3; p.n_sub = n_sub;
    return p;
}

long nrm_frontend_tables_ws_floats(long nrows_total, int n_sub, int e1, int n_type, int e2, int n_year, int n_month, int n_day, int n_hour, int e3) {
    if (nrows_total <= 0 || n_sub < 0) return 0;
    return nrm::tab_grad_ws_floats(tab_dims(n_sub, e1, n_type, e2, n_year, n_month, n_day, n_hour, e3), nrows_total);
}

int nrm_frontend_bwd_tables(const void* x0, int nrows0, int xcols0, int behaviour0, const float* dlab0, int lddl0,
                            const void* x1, int nrows1, int xcols1, int behaviour1, const float* dlab1, int lddl1, int x_is_f64,
                            int P, int n_sub, const float* sen_w, const float* sen_b,
                            int e0, int e1, int n_type, int e2, int n_year, int n_month, int n_day, int n_hour, int e3,
                            float* d_sen_w, float* d_sen_b, float* d_type_tab,
                            float* d_year_tab, float* d_month_tab, float* d_day_tab, float* d_hour_tab, float* ws, nrm_stream_t stream) {
    if (nrows0 > 0) if (int rc = check_fe("nrm_frontend_bwd_tables", nrows0, xcols0, P, n_sub, behaviour0, e0, e1, e2, e3)) return rc;
    if (nrows1 > 0) if (int rc = check_fe("nrm_frontend_bwd_tables", nrows1, xcols1, P, n_sub, behaviour1, e0, e1, e2, e3)) return rc;
    if (nrows0 < 0 || nrows1 < 0 || (long)nrows0 + nrows1 >= (1L << 31) - 64) return fail(NRM_EINVAL, "nrm_frontend_bwd_tables: nrows=%d,%d", nrows0, nrows1);
    if ((nrows0 > 0 && (!x0 || !dlab0 || lddl0 < e0 + e1 + e2 + e3)) || (nrows1 > 0 && (!x1 || !dlab1 || lddl1 < e0 + e1 + e2 + e3)))
        return fail(NRM_EINVAL, "nrm_frontend_bwd_tables: null pointer or lddl too small");
    if (!sen_w || !sen_b || !d_sen_w || !d_sen_b || !d_type_tab || !d_year_tab || !d_month_tab || !d_day_tab || !d_hour_tab || !ws)
        return fail(NRM_EINVAL, "nrm_frontend_bwd_tables: null pointer");
    nrm::FrontendParams p = tab_dims(n_sub, e1, n_type, e2, n_year, n_month, n_day, n_hour, e3);
    p.e0 = e0; p.P = P; p.n_cat = 1;               // (the category columns are not read here)
    p.sen_w = sen_w; p.sen_b = sen_b;
    p.d_sen_w = d_sen_w; p.d_sen_b = d_sen_b; p.d_type_tab = d_type_tab;
    p.d_year_tab = d_year_tab; p.d_month_tab = d_month_tab; p.d_day_tab = d_day_tab; p.d_hour_tab = d_hour_tab;
    if (nrm::tab_grad_ws_floats(p, (long)nrows0 + nrows1) <= 0 && nrows0 + nrows1 > 0)
        return fail(NRM_EINVAL, "nrm_frontend_bwd_tables: shape not taken (nrm_frontend_tables_ws_floats is 0): use nrm_frontend_bwd");
    return check_hip(nrm::tab_grad_launch(p, x0, nrows0, xcols0, dlab0, lddl0, x1, nrows1, xcols1, dlab1, lddl1, x_is_f64, ws,
                                          (hipStream_t)stream), "frontend_bwd_tables");
}

long nrm_frontend_cat_ws_ints(int n_cat, long nrows_total, int n_sub) {
    if (n_cat <= 0 || nrows_total < 0 || n_sub < 0) return 0;
    return nrm::cat_grad_ws_ints(n_cat, nrows_total, n_sub);
}

int nrm_frontend_cat_grad(const void* x0, int nrows0, int xcols0, const float* dlab0, int lddl0,
                          const void* x1, int nrows1, int xcols1, const float* dlab1, int lddl1, int x_is_f64,
                          int P, int n_sub, int n_cat, int e0, float* d_cat_tab, int* ws, nrm_stream_t stream) {
    if (nrows0 < 0 || nrows1 < 0 || P <= 0 || n_sub < 1 || n_sub > 16 || n_cat <= 0 || e0 <= 0 || e0 > 512)
        return fail(NRM_EINVAL, "nrm_frontend_cat_grad: nrows=%d,%d P=%d n_sub=%d n_cat=%d e0=%d (1 <= n_sub <= 16, e0 <= 512)", nrows0, nrows1, P, n_sub, n_cat, e0);
    if ((nrows0 > 0 && (!x0 || !dlab0 || lddl0 < e0 || xcols0 < 4 + P + 1 + n_sub)) || (nrows1 > 0 && (!x1 || !dlab1 || lddl1 < e0 || xcols1 < 4 + P + 1 + n_sub)) || !d_cat_tab || !ws)
        return fail(NRM_EINVAL, "nrm_frontend_cat_grad: null pointer, lddl < e0 or packed rows too short");
    if (((long)nrows0 + nrows1) * (n_sub + 1) >= (1L << 31)) return fail(NRM_EINVAL, "nrm_frontend_cat_grad: more than 2^31 table references");
    return check_hip(nrm::cat_grad_launch(x0, nrows0, xcols0, dlab0, lddl0, x1, nrows1, xcols1, dlab1, lddl1, x_is_f64, P, n_sub, n_cat, e0,
                                          d_cat_tab, ws, (hipStream_t)stream), "frontend_cat_grad");
}

int nrm_assemble_form(int static_cols, int S) { return nrm::assemble_form(static_cols, S); }

// nrm_assemble_batch (no cursor, n_order = B), nrm_assemble_batch_at and nrm_assemble_groups_at (groups: the plan whose arenas the x
// pointers of the table struct are): one validation, one launch
static int assemble_entry(const char* who, const nrm_assemble_tables* tables, const long* sel, long n_order, const long* cursor, bool at, int B,
                          int H, int T, int flags, nrm_stream_t stream, const nrm_assemble_groups* groups = nullptr) {
    if (!tables) return fail(NRM_EINVAL, "%s: null table struct", who);
    const nrm_assemble_tables& t = *tables;
    if (B < 0 || H <= 0 || T <= 0 || (flags & ~NRM_ASSEMBLE_KEEP_TARGET_SLOT))
        return fail(NRM_EINVAL, "%s: B=%d H=%d T=%d flags=%d (B >= 0, H, T > 0, flags 0 or NRM_ASSEMBLE_KEEP_TARGET_SLOT)", who, B, H, T, flags);
    if (B == 0) return NRM_OK;
    if (at && (n_order < 1 || n_order >= (1L << 62))) return fail(NRM_EINVAL, "%s: n_order=%ld (1 <= n_order < 2^62 where B > 0)", who, n_order);
    if (at && !cursor) return fail(NRM_EINVAL, "%s: null pointer (cursor)", who);
    const long sz = t.is_f64 ? 8 : 4;
    if (t.A < 1 || t.A >= (1L << 31) || t.U < 1 || t.U >= (1L << 31) || t.N < 1 || t.E < 0 || t.L < 0)
        return fail(NRM_EINVAL, "%s: A=%ld U=%ld E=%ld N=%ld L=%ld (1 <= A, U < 2^31, N >= 1, E, L >= 0)", who, t.A, t.U, t.E, t.N, t.L);
    if (t.static_cols < 1 || t.S != (t.static_cols + 3) / 4 * 4 || t.A * t.S * sz >= (1L << 32))
        return fail(NRM_EINVAL, "%s: static_cols=%d S=%d A=%ld (S = static_cols rounded up to a multiple of 4; art_static below 2^32 bytes)",
                    who, t.static_cols, t.S, t.A);
    const long hc = 4 + t.static_cols + 2, tc = 4 + t.static_cols;
    if ((long)H * hc * sz >= (1L << 31) || (long)T * tc * sz >= (1L << 31) || (long)B * T >= (1L << 31))
        return fail(NRM_EINVAL, "%s: H=%d T=%d B=%d: the rows of one impression exceed 2^31 bytes (or B*T >= 2^31)", who, H, T, B);
    if (!sel || !t.art_static || !t.art_global || !t.art_pub_us || !t.art_id || !t.user_off || !t.user_id || !t.imp_user || !t.imp_time_us ||
        !t.imp_off || !t.imp_target || !t.imp_id || (t.E > 0 && (!t.ev_art || !t.ev_time_us || !t.ev_read || !t.ev_scroll)) || (t.L > 0 && !t.imp_inview) ||
        !t.x_history || !t.x_target || !t.x_global || !t.label || !t.label_id || !t.empty_num || !t.user_id_out || !t.impression_id ||
        !t.history_len || !t.err)
        return fail(NRM_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)t.art_static | (uintptr_t)t.x_history | (uintptr_t)t.x_target) & 15)
        return fail(NRM_EINVAL, "%s: art_static, x_history and x_target must be 16-byte aligned", who);
    nrm::AssembleParams p;
    p.t = t; p.sel = sel; p.cursor = cursor; p.n_order = n_order; p.B = B; p.H = H; p.T = T; p.keep_target_slot = (flags & NRM_ASSEMBLE_KEEP_TARGET_SLOT) ? 1 : 0;
    if (!groups) return check_hip(nrm::assemble_launch(p, (hipStream_t)stream), "assemble_batch");
    const nrm_assemble_groups& g = *groups;
    if (g.G < 1 || g.G > nrm::HISTORY_GROUPS_MAX || g.R < 1 || g.N < 1 || (long)g.R > (long)B * H || (long)g.N > (long)B * T)
        return fail(NRM_EINVAL, "%s: G=%d R=%d N=%d (1 <= G <= %d, 1 <= R <= B*H, 1 <= N <= B*T)", who, g.G, g.R, g.N, nrm::HISTORY_GROUPS_MAX);
    if (!g.bounds || !g.h_g || !g.hist_row_off || !g.t_g || !g.cand_row_off || !g.label_arena || !g.row_weight || !g.misfit)
        return fail(NRM_EINVAL, "%s: null pointer (group tables)", who);
    nrm::AssembleGroupsParams q;
    q.a = p; q.bounds = g.bounds; q.h_g = g.h_g; q.hist_row_off = g.hist_row_off; q.t_g = g.t_g; q.cand_row_off = g.cand_row_off;
    q.label_arena = g.label_arena; q.row_weight = g.row_weight; q.misfit = g.misfit; q.G = g.G; q.R = g.R; q.N = g.N;
    return check_hip(nrm::assemble_groups_launch(q, (hipStream_t)stream), "assemble_groups");
}

int nrm_assemble_batch(const nrm_assemble_tables* tables, const long* sel, int B, int H, int T, int flags, nrm_stream_t stream) {
    return assemble_entry("nrm_assemble_batch", tables, sel, B, nullptr, false, B, H, T, flags, stream);
}

int nrm_assemble_batch_at(const nrm_assemble_tables* tables, const long* order, long n_order, const long* cursor, int B, int H, int T,
                          int flags, nrm_stream_t stream) {
    return assemble_entry("nrm_assemble_batch_at", tables, order, n_order, cursor, true, B, H, T, flags, stream);
}

int nrm_assemble_groups_at(const nrm_assemble_tables* tables, const nrm_assemble_groups* groups, const long* order, long n_order,
                           const long* cursor, int B, int H, int T, int flags, nrm_stream_t stream) {
    if (!groups) return fail(NRM_EINVAL, "nrm_assemble_groups_at: null group struct");
    return assemble_entry("nrm_assemble_groups_at", tables, order, n_order, cursor, true, B, H, T, flags, stream, groups);
}

int nrm_epoch_tally(const float* loss, const float* auc, const int* top1, int B, long* cursor, double* sums, long* counts,
                    float* step_log, long log_cap, nrm_stream_t stream) {
    if (B < 0 || log_cap < 0) return fail(NRM_EINVAL, "nrm_epoch_tally: B=%d log_cap=%ld (both >= 0)", B, log_cap);
    if (!loss || !auc || !top1 || !cursor || !sums || !counts || (log_cap > 0 && !step_log)) return fail(NRM_EINVAL, "nrm_epoch_tally: null pointer");
    return check_hip(nrm::epoch_tally_launch(loss, auc, top1, B, cursor, sums, counts, step_log, log_cap, (hipStream_t)stream), "epoch_tally");
}

int nrm_eval_tally(const float* auc, const int* top1, const float* metrics, const int* rank, const int* live, const long* impression_id,
                   int B, int T, int Tp, long* cursor, long n_order, double* sums, long* counts, int* rec_rank, int* rec_live, long* rec_id,
                   long cap, nrm_stream_t stream) {
    if (B < 0 || T < 1 || Tp < 1 || n_order < 0 || cap < 0)
        return fail(NRM_EINVAL, "nrm_eval_tally: B=%d T=%d Tp=%d n_order=%ld cap=%ld (B, n_order, cap >= 0; T, Tp >= 1)", B, T, Tp, n_order, cap);
    if (Tp > T) return fail(NRM_EINVAL, "nrm_eval_tally: Tp=%d exceeds T=%d (the record row holds T columns)", Tp, T);
    if (!cursor || !sums || !counts) return fail(NRM_EINVAL, "nrm_eval_tally: null cursor, sums or counts");
    if (!auc != !top1) return fail(NRM_EINVAL, "nrm_eval_tally: auc and top1 are NULL together (the outputs of nrm_row_auc) or both given");
    const int n_rec = (rec_rank != nullptr) + (rec_live != nullptr) + (rec_id != nullptr);
    if ((cap == 0 && n_rec != 0) || (cap > 0 && n_rec != 3))
        return fail(NRM_EINVAL, "nrm_eval_tally: rec_rank, rec_live and rec_id are NULL together with cap = 0, or all given with cap > 0 (cap=%ld)", cap);
    if (cap > 0 && (!rank || !live || !impression_id)) return fail(NRM_EINVAL, "nrm_eval_tally: a record (cap=%ld) needs rank, live and impression_id", cap);
    if (cap > 0 && B > 0 && cap % B) return fail(NRM_EINVAL, "nrm_eval_tally: cap=%ld is no multiple of B=%d (a step's rows stay together in the ring)", cap, B);
    return check_hip(nrm::eval_tally_launch(auc, top1, metrics, rank, live, impression_id, B, T, Tp, cursor, n_order, sums, counts, rec_rank, rec_live,
                                            rec_id, cap, (hipStream_t)stream), "eval_tally");
}

}  // extern "C"
