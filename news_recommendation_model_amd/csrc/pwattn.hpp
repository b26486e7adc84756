// Parameter blocks and host-side launchers shared by the pointwise-attention kernels and capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace nrm {

// ---- forward (pwattn_fwd.hip)
struct FwdParams {
    const float* t;      // [B*T, ldt]
    const float* h;      // [B*H, ldh]
    const float* u;      // [B*H, ldu]   (includes fc1 bias)
    const float* v;      // [B*T, ldv]
    const float* wp;     // packed, see pack_wp_kernel
    const float* w2;     // [D]
    const float* b2;     // [1]
    float* z;            // [M, D] or nullptr
    float* s;            // [M]
    long M;              // B*T*H
    int T, H, D;
    int ldt, ldh, ldu, ldv;
    unsigned wp_bytes, t_bytes, h_bytes;   // buffer-descriptor extents (t/v share t_bytes, h/u share h_bytes)
    int rows;            // padded row count of packed W_p  (= nchunks * NT * 16)
    int kchunks;         // K-chunks of the packed W_p: ceil(D/16) (fp32 operands) or ceil(D/32) (bf16 operands)
    int nchunks;         // number of N-chunks (each NT*16 output columns)
};
// Ragged candidate lists (inference, compact scoring): candidate rows t / v are [N, D] and belong to impression cand_imp[c]; the
// candidates of impression b are the rows cand_off[b] .. cand_off[b + 1] - 1.  Passed as a kernel argument of its own behind the
// dense parameter block; the dense instantiations never read it.
struct RaggedTabs {
    const int* cand_imp;   // [N]
    const int* cand_off;   // [B + 1]
    int B, N;
    int max_count;         // longest candidate list (host side: task grids)
    // History-ragged form (compact scoring with history compaction): h / u are the R kept history rows, impression b
    // owns the rows hist_off[b] .. hist_off[b + 1] - 1 (K_b of them), and a candidate's scores are nt_b = ceil(K_b / 16) whole 16-row tiles
    // of s [16 Mt].  Read by the HRAG instantiations only.
    const int* hist_off;   // [B + 1]
    const int* tile_pre;   // [B + 1] prefix sums of count_b nt_b: first tile of impression b's first candidate
    const int4* tile_tab;  // [Mt] per tile {candidate, first row in h / u, valid rows, impression} (history_tiles_launch)
    int R, Mt, k_max;      // k_max: longest kept history (host side: task grids, image choice)
};
struct FwdPlan { int NT, MT, nchunks, rows, kchunks; };
FwdPlan pwattn_fwd_plan(int D);
// Every environment knob of the forward, read in ONE place (fwd_knobs, pwattn_fwd.hip).  walk (NRM_FWD_WALK) is latched at the first
// call in the process; ct (NRM_FWD_CT), walk_f32 (NRM_FWD_WALK_F32) and tsplit (NRM_FWD_TSPLIT) are read at every call.  ct / walk_f32:
// -1 unset, 0, 1.  None of them changes the packed W_p image, which depends on D and the arithmetic alone.
struct FwdKnobs { int walk, ct, walk_f32, tsplit; bool tsplit_set; };      // tsplit counts only where tsplit_set
FwdKnobs fwd_knobs();
// What one forward launch runs: chosen by pwattn_fwd_select (host arithmetic only, no HIP call); the launches switch on it and on nothing else.
enum FwdFamily { FWD_STREAM = 0, FWD_RW_TILE = 1, FWD_WALK_BF16 = 2, FWD_WALK_F32 = 3 };
struct FwdForm {
    int valid;                    // 0: the selection has no instantiation (the launch returns hipErrorInvalidValue)
    int family;                   // FwdFamily
    int NT, MT, WPE, CT, NW;      // FWD_STREAM: pwattn_fwd_kernel<NT, MT, SAVE_Z, WPE, CT, NW, RAGGED, HRAG>
    int NTS, KCH;                 // FWD_RW_TILE: pwattn_fwd_rw_kernel<NTS, ..>; the walks: <NTS, .., KCH> (fp32 walk: KCH = NTS)
    int mma, save_z, ragged;      // arithmetic; z stored; 0 dense, 1 candidates, 2 candidates and history
    int nsplit, tsplit;           // column slices of the resident forms (1 otherwise); parts of the candidate walk (1 otherwise)
    int wgs;                      // workgroups per slice (the grid is wgs * nsplit)
    long tasks;                   // row tiles (FWD_RW_TILE), walk tasks, or workgroups (FWD_STREAM); 0: nothing is launched
    int rounds;                   // ceil(tasks / (wgs * waves per workgroup)): trips of the busiest wave's persistent loop; FWD_STREAM: 1
    int nchunks;                  // FWD_STREAM: N-chunks the width is streamed in
};
// M: flattened rows (B T H dense, N H ragged, 16 Mt history-ragged); B: impressions; T, H as in FwdParams (ragged: T = 1; history-ragged:
// H = 1); N, max_count, k_max as in RaggedTabs (ragged forms only); cus: compute units of the device the launch goes to
FwdForm pwattn_fwd_select(long M, int B, int T, int H, int D, int mma, bool save_z, int ragged, int N, int max_count, int k_max, int cus);
FwdForm pwattn_fwd_rw_select(long M, int B, int T, int H, int D, int mma, bool save_z, int ragged, int N, int max_count, int k_max, int cus,
                             const FwdKnobs& kn);
hipError_t pwattn_fwd_launch(const FwdParams& p, int mma, hipStream_t st);
// fp32 arithmetic, no z store; p.M = N * H, p.T is not read
hipError_t pwattn_fwd_ragged_launch(const FwdParams& p, const RaggedTabs& rg, hipStream_t st);
// ragged in the history too: p.M = 16 * rg.Mt, p.h_bytes covers the R kept rows, p.T and p.H are not read
hipError_t pwattn_fwd_hragged_launch(const FwdParams& p, const RaggedTabs& rg, hipStream_t st);
hipError_t pack_wp_launch(const float* w, int ldw, int D, const FwdPlan& pl, int mma, float* packed, hipStream_t st);
// resident-W forward (pwattn_fwd_rw.hip): mma = 0 (fp32 MFMA), 1 (bf16 operands) or 2 (bf16x3: hi + lo split).  The output
// columns are cut into nsplit slices of nts 16-column tiles whose whole image stays resident in LDS (persistent workgroups).
struct RwPlan { int nts, nsplit, rows, k32, wimg; };      // rows = padded rows of the packed image = nsplit * nts * 16; k32 = chunks
RwPlan pwattn_rw_plan(int D, int mma);
bool pwattn_fwd_uses_rw(int D, int mma);                  // which forward (and which packed layout) a call takes
// launches a FWD_RW_TILE / FWD_WALK_* form (ragged: fp32, D <= 128 -- one resident slice); called by the launches of pwattn_fwd.hip
hipError_t pwattn_fwd_rw_launch_form(const FwdParams& p, const RaggedTabs& rg, const struct FwdForm& f, hipStream_t st);
hipError_t pack_wp_bf16_launch(const float* w, int ldw, int D, int mma, float* packed, hipStream_t st);

// ---- backward (pwattn_bwd.hip)
struct BwdEParams {
    const float* X; long xs1, xs2, xrs;   // X_g[r,k] at X[g1*xs1 + g2*xs2 + r*xrs + k],  g = g1*G2 + g2
    const float* Y; long ys1, yrs;        // Y_g[r,d] at Y[g1*ys1 + r*yrs + d]
    const float* wp; int ldwp;            // W_p[k,d] at wp[k*ldwp + d]
    const float* srow; int lds_;          // scale row of group g at srow[g*lds_ + d]     (WITH_DW)
    float* out; int ldo;                  // out[g*ldo + d] += sum_k W_p[k,d] E_g[k,d]
    float* ws;                            // [nsplit][D][D] partial dW_p^T  (ws[s][d][k])      (WITH_DW)
    int G, G2, R, D;
    int gps;                              // groups per split
    int nkw, ndcol;                       // k-ranges and d-columns of the wave-tile grid
    int nsplit;
    int interleave;                       // the 4 waves of a workgroup walk one group range round-robin (serial and one-accumulator kernels; the pipelined and 32-row kernels always walk blocked)
    int x_hl4;                            // X is in the NRM_DZ_HL4 format (bf16 forms only): no conversion of the dz operand
    int with_dt;                          // 0: the (b,t)-grouped pass only accumulates dW_p (dt comes from pwattn_bwd_rw.hip)
    int order;                            // block order inside an XCD: 0 = (split group, k-range, d-column), 1 = (k-range, split group, d-column) (serial and one-accumulator kernels; the pipelined and 32-row kernels always take 0 -- e_tile / e_groups in pwattn_bwd.hip)
};
struct BwdEPlan { int DT, KT, ndcol, nkw, nsplit, gps; };
BwdEPlan bwd_e_plan(int D, int G, int target_waves, int min_gps = 1, int mma = 0);
// Which contraction kernel a launch takes: chosen by bwd_e_select (host arithmetic only, no HIP call), launched by bwd_e_launch
enum BwdEFamily { BWD_E_REFUSED = -1, BWD_E_SERIAL = 0, BWD_E_PIPE = 1, BWD_DW_DIRECT = 2, BWD_DW_R32 = 3 };
struct BwdEKnobs { bool pipe, dw_direct, dw_r32, dw_pack; };   // NRM_BH_PIPE, NRM_DW_DIRECT, NRM_DW_R32, NRM_DW_PACK: each on unless set to 0
BwdEKnobs bwd_e_knobs();                                  // the environment as it is NOW (every launch asks again)
struct BwdEForm {
    int family;                                           // BwdEFamily; BWD_E_REFUSED: a combination the kernels cannot express
    bool with_dw, with_dt, xhl4; int ks;                  // what the pass forms and reads (bwd_e_kernel's WITH_DW, WITH_DT, XHL4, KS)
    bool exact; int mma;                                  // EXACT: D fills whole wave tiles; MMA: 0 fp32, 1 bf16, 2 bf16x3
    int pack = 1;                                         // BWD_DW_DIRECT: groups reduced together in whole steps (bwd_dw_pack_kernel); 1: per group
};
BwdEForm bwd_e_select(const BwdEParams& p, const BwdEPlan& pl, bool with_dw, int mma, const BwdEKnobs& knobs);
hipError_t bwd_e_launch(const BwdEParams& p, const BwdEPlan& pl, bool with_dw, int mma, hipStream_t st);
// The walk of a selected launch as its kernel honours it: p.interleave and p.order count in the serial and the one-accumulator kernel only
// (the packed one walks blocked, the pipelined and the 32-row kernel walk blocked in order 0: e_tile / e_groups in pwattn_bwd.hip)
struct BwdEWalk { int interleave, order, last_groups, last_live; };   // groups of the last split; live splits (waves) of the last workgroup
BwdEWalk bwd_e_walk(const BwdEParams& p, const BwdEPlan& pl, const BwdEForm& f);
// What one dz-pass launch runs: chosen by bwd_dz_select (host arithmetic only, no HIP call; NRM_DZ_ROWS read at every call, NRM_DZ_NARROW
// latched at the first); bwd_dz_launch switches on it and on nothing else
enum BwdDzFamily { BWD_DZ_SLAB = 0, BWD_DZ_ROWS = 1 };
struct BwdDzForm {
    int valid;                                            // 0: the slab needs more LDS than a workgroup has (the launch returns hipErrorInvalidValue)
    int family, threads, rows_class;                      // BWD_DZ_ROWS: bwd_dz_rows_kernel<threads, rows_class, 3> (rows_class 1: up to 3 rows per thread, 2: 4..6)
    int slab_cols, nslab, hchunk, nhc;                    // BWD_DZ_SLAB: bwd_dz_kernel's column slabs and history chunks
    size_t shm; bool big_lds, narrowed;                   // its dynamic LDS; above 64 KB; the narrowing loop ran
};
BwdDzForm bwd_dz_select(int B, int T, int H, int D);
// dz_format: 0 = fp32 dz in place, 1 = NRM_DZ_HL4 (every aligned group of 4 values as 4 bf16 hi + 4 bf16 lo, in place)
hipError_t bwd_dz_launch(float* z, const float* ds, const float* w2, float* dw2, float* db2, float* du, float* dv,
                         int B, int T, int H, int D, int dz_format, hipStream_t st);

// ---- backward of the bilinear term, resident-W form for the bf16 arithmetics (pwattn_bwd_rw.hip): dt and dh from ONE read of dz
struct BwdRwParams {
    const float* dz;     // [B*T*H, D] in the NRM_DZ_HL4 format
    const float* t;      // [B*T, D]
    const float* h;      // [B*H, D]
    const float* wimg;   // packed by pwattn_bwd_rw_pack_launch
    float* dt;           // [B*T, D]  +=
    float* dh;           // [B*H, D]  +=
    int B, T, H, D;
    unsigned w_bytes;
    int tsplit;          // parts of the candidate walk (set by the launcher)
};
struct BwdRwPlan { int ng, kc, nks, wimg, k32, rows; };   // ng == 0: this (D, mma) keeps the E-form
BwdRwPlan pwattn_bwd_rw_plan(int D, int mma);
long pwattn_bwd_rw_packed_floats(int D, int mma);
hipError_t pwattn_bwd_rw_pack_launch(const float* wp, int ldw, int D, int mma, float* packed, hipStream_t st);
hipError_t pwattn_bwd_rw_launch(const BwdRwParams& p, int mma, hipStream_t st);
// What one resident-W backward launch runs: chosen by pwattn_bwd_rw_select (host arithmetic only, no HIP call; NRM_BRW_WAVES and
// NRM_BRW_TSPLIT read at every call); the launch switches on it and on nothing else.  cus: compute units of the device
struct BwdRwForm {
    int valid;                                            // 0: this (D, mma) keeps the E-form
    int NG, mma; bool exact;                              // bwd_dp_rw_kernel<NG, MMA, EXACT>
    int nks, wgs, nw, tsplit;                             // reduction slices; workgroups per slice (the grid is wgs * nks); waves per workgroup; parts of the candidate walk
    long tasks; int rounds; bool plain_dh;                // tasks of one slice; trips of the busiest wave's task loop; one task owns its dh rows (no atomics)
};
BwdRwForm pwattn_bwd_rw_select(int B, int T, int H, int D, int mma, int cus);

// ---- backward of the bilinear term in fp32, dP walk form (pwattn_bwd_dp.hip): dt and dh from ONE contraction dP = dz W_p with the
// forward's K-chunk-streaming skeleton; dW_p then comes from the (b,t) pass without its dt epilogue
struct BwdDpParams {
    const float* dz;     // [B*T*H, D] fp32
    const float* t;      // [B*T, D]
    const float* h;      // [B*H, D]
    const float* wimg;   // packed by pwattn_bwd_dp_pack_launch
    float* dt;           // [B*T, D]  +=
    float* dh;           // [B*H, D]  +=
    int B, T, H, D;
    unsigned w_bytes, t_bytes, h_bytes;
    int rows, kchunks, nchunks;   // of the plan (set by the launcher)
    long steps;                   // (row blocks of 64) x N-chunks x T (set by the launcher)
};
struct BwdDpPlan { int NT, nchunks, rows, kchunks; };     // NT == 0: this (D, H) keeps the E-form
BwdDpPlan pwattn_bwd_dp_plan(int D, int H);
long pwattn_bwd_dp_packed_floats(int D, int H);
hipError_t pwattn_bwd_dp_pack_launch(const float* wp, int ldw, int D, int H, float* packed, hipStream_t st);
hipError_t pwattn_bwd_dp_launch(BwdDpParams p, hipStream_t st);
// What one dP-walk launch runs: chosen by pwattn_bwd_dp_select (host arithmetic only, no HIP call; NRM_DP_GRID read at every call); the
// launch switches on it and on nothing else.  cus: compute units of the device
struct BwdDpForm {
    int valid;                                            // 0: this (D, H) keeps the E-form, or more than 2^31 - 1 steps
    BwdDpPlan pl; long steps; long grid;                  // bwd_dp_walk_kernel<pl.NT>; (row blocks of 64) x N-chunks x T; workgroups (0: nothing to launch)
};
BwdDpForm pwattn_bwd_dp_select(int B, int T, int H, int D, int cus);
// most steps / most (row block, N-chunk) items one workgroup of the launch walks (the plan query asks; the launch does not)
void pwattn_bwd_dp_extent(const BwdDpForm& f, int T, int& max_steps, int& max_items);

// Non-zero when the translation unit was compiled with a timing-diagnostic override (scripts/_diag): such a library computes
// WRONG results by construction; capi.hip ORs these into nrm_build_flags() and native.load refuses a non-zero value.
int pwattn_fwd_diag_flags();        // pwattn_fwd.hip:     bit 0 NRM_DIAG_FWD, bit 1 XCD_REMAP off
int pwattn_fwd_rw_diag_flags();     // pwattn_fwd_rw.hip:  bit 2 NRM_DIAG_RW
int pwattn_bwd_rw_diag_flags();     // pwattn_bwd_rw.hip:  bit 9 NRM_DIAG_BRW
int pwattn_bwd_dp_diag_flags();     // pwattn_bwd_dp.hip:  bit 10 NRM_DIAG_DP
int pwattn_bwd_diag_flags();        // pwattn_bwd.hip:     bits 3.. NRM_EPI_AHEAD off, GELU_AT_LOAD, NOEPI, NOATOM, NOLOAD, NRM_PIPE_SGB off

}  // namespace nrm
