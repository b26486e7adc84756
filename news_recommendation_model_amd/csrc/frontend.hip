// Front end of UserInvariantInterestModel: packed feature rows -> embedded label rows + fp32 text/image rows.
// Reference: models/user_invariant_interest_model.py:50-71,74-79 (slice_x, feature_embedding, time_embedding).
//
// Packed row (tool/process_data.py:198-240):  [year, month, day, hour | text_img P | category | sub-category x NS |
//   sentiment x 3 | type | (history only: read_time, scroll)], fp64 out of the reference DataLoader or fp32.
// Label row written here:  [ Emb_cat(category) + mean_NS Emb_cat(sub) : e0 | ReLU(W_s sentiment + b_s) : e1 |
//   Emb_type(type) : e2 | Emb_year + Emb_month + Emb_day + Emb_hour : e3 | (history: read_time, scroll) ], zero padded
//   to a leading dimension that is a multiple of 4; the text/image block is copied to a dense fp32 [rows, P] matrix.
// The category table serves category AND sub-categories; the mean includes padding id 0 (as the reference does).
//
// Backward scatters d(label row) into the tables.  The category table (3000 rows) takes global float atomics (one
// contiguous run of e0 columns per row id); the tiny hot tables (type 16 rows, year/month/day/hour, sentiment W/b)
// would serialise on a handful of addresses, so each workgroup first sums its rows in LDS and flushes once.
#include <algorithm>
#include "common.hpp"
#include "frontend.hpp"

namespace nrm {

template <typename XT>
__device__ __forceinline__ int row_index(const XT* xr, int col, int limit, int* err) {
    const int i = (int)xr[col];
    if (i < 0 || i >= limit) { *err = 1; return i < 0 ? 0 : limit - 1; }   // reference: IndexError; here: flag + clamp
    return i;
}

// Row headers of a block of consecutive rows, decoded once into LDS: the table indices and the sentiment scalars.  Every
// later loop is then a flat walk over (row, column) pairs with no dependent global load in front of its table access -- the
// first version decoded a row's header with every thread and walked rows one after the other (one workgroup per row in the
// forward, 32 serial rows in the backward): latency-bound, 62 + 190 us at the reference's default sizes for 43 MB.
constexpr int FE_MAXSUB = 16;                      // sub-category slots per row (reference: 5)
constexpr int FE_HDR = 6 + FE_MAXSUB;              // year, month, day, hour, category, type, sub-categories
struct RowHeaders {
    int* idx;                                      // [rows][FE_HDR]
    float* sen;                                    // [rows][4]
};

template <typename XT>
__device__ __forceinline__ void stage_headers(const FrontendParams& p, int xcols, int* err, const XT* __restrict__ x, int r_lo, int nr,
                                              const RowHeaders& hd, int nthreads) {
    const int P = p.P, NS = p.n_sub;
    const int c_cat = 4 + P, c_sub = c_cat + 1, c_sen = c_sub + NS, c_typ = c_sen + 3;
    const int items = 9 + NS;                      // 6 + NS indices, 3 scalars
    for (int i = threadIdx.x; i < nr * items; i += nthreads) {
        const int r = i / items, k = i - r * items;
        const XT* xr = x + (size_t)(r_lo + r) * xcols;
        if (k < 4) {
            const int lim = k == 0 ? p.n_year : k == 1 ? p.n_month : k == 2 ? p.n_day : p.n_hour;
            hd.idx[r * FE_HDR + k] = row_index(xr, k, lim, err);
        } else if (k == 4) {
            hd.idx[r * FE_HDR + 4] = row_index(xr, c_cat, p.n_cat, err);
        } else if (k == 5) {
            hd.idx[r * FE_HDR + 5] = row_index(xr, c_typ, p.n_type, err);
        } else if (k < 6 + NS) {
            hd.idx[r * FE_HDR + k] = row_index(xr, c_sub + (k - 6), p.n_cat, err);
        } else {
            hd.sen[r * 4 + (k - 6 - NS)] = (float)xr[c_sen + (k - 6 - NS)];
        }
    }
}

// FWD_ROWS consecutive rows per workgroup of 256 threads; the outputs of consecutive rows are contiguous, so the flat
// (row, column) walk stores whole cache lines
constexpr int FWD_ROWS = 8;
constexpr int FE_THREADS = 256;

template <typename XT>
__global__ __launch_bounds__(FE_THREADS) void frontend_fwd_kernel(const FrontendParams p, const XT* __restrict__ x, int nrows) {
    __shared__ int h_idx[FWD_ROWS * FE_HDR];
    __shared__ float h_sen[FWD_ROWS * 4];
    const int r_lo = blockIdx.x * FWD_ROWS, nr = min(FWD_ROWS, nrows - r_lo);
    const RowHeaders hd = {h_idx, h_sen};
    stage_headers(p, p.xcols, p.err, x, r_lo, nr, hd, FE_THREADS);
    __syncthreads();
    const int P = p.P, NS = p.n_sub;
    const int c_beh = 4 + P + 1 + NS + 3 + 1;
    const int e0 = p.e0, e1 = p.e1, e2 = p.e2, e3 = p.e3;
    const int width = e0 + e1 + e2 + e3 + (p.behaviour ? 2 : 0);
    const float inv_ns = 1.0f / (float)NS;
    float* lab = p.lab + (size_t)r_lo * p.ldlab;
    for (int i = threadIdx.x; i < nr * p.ldlab; i += FE_THREADS) {
        const int r = i / p.ldlab, c = i - r * p.ldlab;
        const int* hi = h_idx + r * FE_HDR;
        float v = 0.f;
        if (c < e0) {
            float sub = 0.f;
            for (int k = 0; k < NS; ++k) sub += p.cat_tab[(size_t)hi[6 + k] * e0 + c];
            v = p.cat_tab[(size_t)hi[4] * e0 + c] + sub * inv_ns;
        } else if (c < e0 + e1) {
            const int j = c - e0;
            const float pre = p.sen_b[j] + p.sen_w[j * 3] * h_sen[r * 4] + p.sen_w[j * 3 + 1] * h_sen[r * 4 + 1] + p.sen_w[j * 3 + 2] * h_sen[r * 4 + 2];
            v = fmaxf(pre, 0.f);
        } else if (c < e0 + e1 + e2) {
            v = p.type_tab[(size_t)hi[5] * e2 + (c - e0 - e1)];
        } else if (c < e0 + e1 + e2 + e3) {
            const int k = c - e0 - e1 - e2;
            v = p.year_tab[(size_t)hi[0] * e3 + k] + p.month_tab[(size_t)hi[1] * e3 + k] + p.day_tab[(size_t)hi[2] * e3 + k] + p.hour_tab[(size_t)hi[3] * e3 + k];
        } else if (c < width) {
            v = (float)x[(size_t)(r_lo + r) * p.xcols + c_beh + (c - (e0 + e1 + e2 + e3))];
        }
        lab[i] = v;
    }
    float* ti = p.ti + (size_t)r_lo * p.ldti;
    for (int i = threadIdx.x; i < nr * p.ldti; i += FE_THREADS) {
        const int r = i / p.ldti, c = i - r * p.ldti;
        ti[i] = c < P ? (float)x[(size_t)(r_lo + r) * p.xcols + 4 + c] : 0.f;
    }
}

// A workgroup (256 threads) walks groups of FE_ROWS consecutive rows (grid-stride) and keeps ONE set of LDS accumulators for
// the small tables over all of them: the flush at the end is one float atomic per touched cell and WORKGROUP, all workgroups
// hitting the same few thousand addresses.  At most FE_MAX_BLOCKS workgroups.
constexpr int FE_ROWS = 32;
constexpr int FE_MAX_BLOCKS = 512;

template <typename XT>
__global__ __launch_bounds__(FE_THREADS) void frontend_bwd_kernel(const FrontendParams p, const XT* __restrict__ x,
                                                                 const float* __restrict__ dlab, int lddl, int nrows) {
    extern __shared__ float sm[];
    const int e0 = p.e0, e1 = p.e1, e2 = p.e2, e3 = p.e3;
    float* a_type = sm;                                  // [n_type][e2]
    float* a_year = a_type + p.n_type * e2;              // [n_year][e3]
    float* a_month = a_year + p.n_year * e3;
    float* a_day = a_month + p.n_month * e3;
    float* a_hour = a_day + p.n_day * e3;
    float* a_sen = a_hour + p.n_hour * e3;               // [e1][4] = dW (3) | db
    const int total = (int)(a_sen + e1 * 4 - sm);
    const RowHeaders hd = {reinterpret_cast<int*>(sm + total), sm + total + FE_ROWS * FE_HDR};
    for (int i = threadIdx.x; i < total; i += FE_THREADS) sm[i] = 0.f;
    int dummy = 0;                                       // (the forward has already flagged out-of-range ids of these rows)
    const int NS = p.n_sub;
    const float inv_ns = 1.0f / (float)NS;
    const int small = e1 + e2 + e3;
    const int ngroups = (nrows + FE_ROWS - 1) / FE_ROWS;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int r_lo = grp * FE_ROWS, nr = min(FE_ROWS, nrows - r_lo);
        __syncthreads();                                 // the previous group's readers of the headers are done (and the zeroing)
        stage_headers(p, p.xcols, &dummy, x, r_lo, nr, hd, FE_THREADS);
        __syncthreads();
        const float* g0 = dlab + (size_t)r_lo * lddl;
        // (1) category table: a flat walk over (row, column < e0): 1 + NS float atomics each, nothing serial between rows
        //     (d_cat_tab == nullptr: the caller forms that gradient with cat_grad_launch below instead)
        for (int i = threadIdx.x; i < (p.d_cat_tab ? nr * e0 : 0); i += FE_THREADS) {
            const int r = i / e0, c = i - r * e0;
            const int* hi = hd.idx + r * FE_HDR;
            const float gv = g0[(size_t)r * lddl + c];
            atomicAdd(p.d_cat_tab + (size_t)hi[4] * e0 + c, gv);
            const float gs = gv * inv_ns;
            for (int k = 0; k < NS; ++k) atomicAdd(p.d_cat_tab + (size_t)hi[6 + k] * e0 + c, gs);
        }
        // (2) the small hot tables: a flat walk over (row, small column) with LDS float atomics (a few dozen per row)
        //     (d_type_tab == nullptr: the caller forms these gradients with tab_grad_launch below instead)
        for (int i = threadIdx.x; i < (p.d_type_tab ? nr * small : 0); i += FE_THREADS) {
            const int r = i / small, cs = i - r * small;
            const float gv = g0[(size_t)r * lddl + e0 + cs];
            const int* hi = hd.idx + r * FE_HDR;
            if (cs < e1) {
                const float s0 = hd.sen[r * 4], s1 = hd.sen[r * 4 + 1], s2 = hd.sen[r * 4 + 2];
                const float pre = p.sen_b[cs] + p.sen_w[cs * 3] * s0 + p.sen_w[cs * 3 + 1] * s1 + p.sen_w[cs * 3 + 2] * s2;
                if (pre > 0.f && gv != 0.f) {            // ReLU'
                    atomicAdd(a_sen + cs * 4 + 0, gv * s0);
                    atomicAdd(a_sen + cs * 4 + 1, gv * s1);
                    atomicAdd(a_sen + cs * 4 + 2, gv * s2);
                    atomicAdd(a_sen + cs * 4 + 3, gv);
                }
            } else if (cs < e1 + e2) {
                atomicAdd(a_type + hi[5] * e2 + (cs - e1), gv);
            } else {
                const int k = cs - e1 - e2;
                atomicAdd(a_year + hi[0] * e3 + k, gv);
                atomicAdd(a_month + hi[1] * e3 + k, gv);
                atomicAdd(a_day + hi[2] * e3 + k, gv);
                atomicAdd(a_hour + hi[3] * e3 + k, gv);
            }
        }
    }
    __syncthreads();
    if (!p.d_type_tab) return;
    // flush: one float atomic per touched LDS cell (zeros are skipped)
    for (int i = threadIdx.x; i < p.n_type * e2; i += FE_THREADS) if (a_type[i] != 0.f) atomicAdd(p.d_type_tab + i, a_type[i]);
    for (int i = threadIdx.x; i < p.n_year * e3; i += FE_THREADS) if (a_year[i] != 0.f) atomicAdd(p.d_year_tab + i, a_year[i]);
    for (int i = threadIdx.x; i < p.n_month * e3; i += FE_THREADS) if (a_month[i] != 0.f) atomicAdd(p.d_month_tab + i, a_month[i]);
    for (int i = threadIdx.x; i < p.n_day * e3; i += FE_THREADS) if (a_day[i] != 0.f) atomicAdd(p.d_day_tab + i, a_day[i]);
    for (int i = threadIdx.x; i < p.n_hour * e3; i += FE_THREADS) if (a_hour[i] != 0.f) atomicAdd(p.d_hour_tab + i, a_hour[i]);
    for (int i = threadIdx.x; i < e1 * 4; i += FE_THREADS) {
        const float v = a_sen[i];
        if (v != 0.f) {
            const int j = i >> 2, w = i & 3;
            if (w < 3) atomicAdd(p.d_sen_w + j * 3 + w, v); else atomicAdd(p.d_sen_b + j, v);
        }
    }
}

static size_t bwd_lds_bytes(const FrontendParams& p) {
    return sizeof(float) * ((size_t)p.n_type * p.e2 + (size_t)(p.n_year + p.n_month + p.n_day + p.n_hour) * p.e3 + (size_t)p.e1 * 4 +
                            (size_t)FE_ROWS * (FE_HDR + 4));
}

hipError_t frontend_fwd_launch(const FrontendParams& p, const void* x, int x_is_f64, int nrows, hipStream_t st) {
    if (nrows <= 0) return hipSuccess;
    if (p.n_sub > FE_MAXSUB) return hipErrorInvalidValue;
    const dim3 grid((nrows + FWD_ROWS - 1) / FWD_ROWS);
    if (x_is_f64) hipLaunchKernelGGL(frontend_fwd_kernel<double>, grid, dim3(FE_THREADS), 0, st, p, (const double*)x, nrows);
    else          hipLaunchKernelGGL(frontend_fwd_kernel<float>, grid, dim3(FE_THREADS), 0, st, p, (const float*)x, nrows);
    return hipGetLastError();
}

hipError_t frontend_bwd_launch(const FrontendParams& p, const void* x, int x_is_f64, const float* dlab, int lddl,
                               int nrows, hipStream_t st) {
    if (nrows <= 0) return hipSuccess;
    const size_t shm = bwd_lds_bytes(p);
    if (shm > 160 * 1024 || p.n_sub > FE_MAXSUB) return hipErrorInvalidValue;
    const dim3 grid(std::min((nrows + FE_ROWS - 1) / FE_ROWS, FE_MAX_BLOCKS));
    if (x_is_f64) {
        if (shm > 64 * 1024) { hipError_t e = hipFuncSetAttribute((const void*)frontend_bwd_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(frontend_bwd_kernel<double>, grid, dim3(FE_THREADS), shm, st, p, (const double*)x, dlab, lddl, nrows);
    } else {
        if (shm > 64 * 1024) { hipError_t e = hipFuncSetAttribute((const void*)frontend_bwd_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(frontend_bwd_kernel<float>, grid, dim3(FE_THREADS), shm, st, p, (const float*)x, dlab, lddl, nrows);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Small-table gradients as a one-hot contraction on the matrix cores.  d_tab[i, c] = sum_r [idx_r == i] dlab[r, c] is A * B with
// A[i][r] a 0/1 compare of the row's header index against the tile's 16 index rows and B[r][c] the gradient rows; the sentiment
// layer's dW | db is the same with A[0..3][r] = (s_r0, s_r1, s_r2, 1) and B[r][j] = relu'_rj dlab[r, j].  v_mfma_f32_16x16x4_f32
// takes 4 rows per step.  The accumulator tiles (type 1 x ceil(e2/16), the four time tables ceil(n/16) x ceil(e3/16), sentiment
// 1 x ceil(e1/16); 59 at e = (200, 100, 50, 50)) are dealt to the 8 waves of a workgroup, at most TB_MAXT = 16 each (64 registers).
//
// The launch is persistent: at most TB_WG_PER_CU workgroups per CU, each walking a contiguous range of TB_ROWS-row chunks of the
// (up to two) row sets.  Per chunk the workgroup stages the row headers and the small columns of dlab in LDS (the ReLU gate is
// applied there), then every wave runs its tiles over the chunk's 4-row steps, A built in registers, B read from LDS.  No LDS
// accumulators and no float atomics: a workgroup stores its partial tables to the workspace with plain stores, and tab_reduce_kernel
// sums the partials in a fixed order into the arena -- the small-table gradients are bitwise reproducible from run to run.
//
// Containment: 0 * NaN is NaN, so a non-finite B element would reach all 16 index rows of its tiles where the scatter reaches one
// cell.  A non-finite gradient element, and the sentiment-column elements of a row with a non-finite sentiment scalar (whose A
// entries are zeroed as well), are staged as 0 and added to their own cells with the scatter's arithmetic and global float atomics
// (rare; behind a ballot).  Columns of a ragged tile beyond the table's width read LDS that nobody wrote: column c of B reaches
// column c of D only, and those columns are not stored.
constexpr int TB_THREADS = 512;
constexpr int TB_WAVES = TB_THREADS / 64;
constexpr int TB_ROWS = 32;                        // rows per chunk (8 steps)
constexpr int TB_MAXT = 16;                        // accumulator tiles per wave
constexpr int TB_MAXTILES = TB_WAVES * TB_MAXT;
constexpr int TB_WG_PER_CU = 2;
constexpr int TB_CB = 4;                          // blocks of 64 columns staged per round
constexpr int TB_RED_CELLS = 64, TB_RED_SLICES = 16;   // tab_reduce_kernel: cells per workgroup, slices of the partials per cell

struct TabTile {                                   // one 16 x 16 accumulator tile
    short hdr, ibase;                              // header slot of the index (0..3 time, 5 type; -1: sentiment), first index row
    short coff, ncol;                              // first column in the staged small block, valid columns
    int dst;                                       // cell of D[0][0] in a partial
    short ldr, ldc;                                // cell strides of D's rows and columns
};
struct TabSet { const void* x; const float* dlab; int nrows, xcols, lddl, nchunks; };
struct TabParams {
    FrontendParams p;                              // dimensions, sen_w / sen_b, d_* (xcols: per set)
    TabSet set[2];
    int ntiles, tiles_per_wave, cells, ldb, chunks_per_wg;
    float* ws;                                     // [gridDim.x][cells] partials
    TabTile tile[TB_MAXTILES];
};

__device__ __forceinline__ bool fe_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

template <typename XT, int NT>                     // NT: accumulator tiles per wave (slots beyond the wave's tiles run a tile that matches no index)
__global__ __launch_bounds__(TB_THREADS, TB_WG_PER_CU * TB_WAVES / 4) void tab_grad_kernel(const TabParams q) {
    extern __shared__ float sm[];
    const FrontendParams& p = q.p;
    const int e0 = p.e0, e1 = p.e1, e2 = p.e2, e3 = p.e3;
    const int small = e1 + e2 + e3, ldb = q.ldb;
    float* s_b = sm;                                                   // [TB_ROWS][ldb] staged gradient block
    float* s_wb = s_b + TB_ROWS * ldb;                                 // [e1][4] = W_s (3) | b_s
    float* s_sen = s_wb + 4 * e1;                                      // [TB_ROWS][4] sentiment scalars as read
    float* s_sa = s_sen + TB_ROWS * 4;                                 // [TB_ROWS][4] A operand: (s0, s1, s2, 1), 0 for a non-finite row
    int* s_idx = reinterpret_cast<int*>(s_sa + TB_ROWS * 4);           // [TB_ROWS][FE_HDR], -1 in the rows that pad the last step
    const RowHeaders hd = {s_idx, s_sen};
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, lk = lane >> 4;

    for (int i = threadIdx.x; i < e1 * 4; i += TB_THREADS) s_wb[i] = (i & 3) < 3 ? p.sen_w[(i >> 2) * 3 + (i & 3)] : p.sen_b[i >> 2];

    const int t_lo = wave * q.tiles_per_wave;
    const int my_nt = max(0, min(q.tiles_per_wave, q.ntiles - t_lo));
    int t_desc[NT];                                                    // hdr + 1 (3 bits) | ibase (15 bits) | coff: one SGPR per tile
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const TabTile& d = q.tile[min(t_lo + t, TB_MAXTILES - 1)];
        const int v = t < my_nt ? (d.hdr + 1) | (d.ibase << 3) | (d.coff << 18) : 1 | (0x7fff << 3);
        t_desc[t] = __builtin_amdgcn_readfirstlane(v);
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    int dummy = 0;                                       // (the forward has already flagged out-of-range ids of these rows)
    const int nchunks = q.set[0].nchunks + q.set[1].nchunks;
    const int ch_lo = blockIdx.x * q.chunks_per_wg, ch_hi = min(nchunks, ch_lo + q.chunks_per_wg);
    for (int ch = ch_lo; ch < ch_hi; ++ch) {
        const int si = ch >= q.set[0].nchunks;
        const TabSet& set = q.set[si];
        const int r_lo = (ch - (si ? q.set[0].nchunks : 0)) * TB_ROWS, nr = min(TB_ROWS, set.nrows - r_lo);
        const int nr4 = (nr + 3) & ~3;
        const float* g0 = set.dlab + (size_t)r_lo * set.lddl + e0;
        __syncthreads();                                 // the previous chunk's readers are done (and s_wb is written)
        // a wave stages rows wave, wave + 8, ...: the loads of a round (4 rows x TB_CB blocks of 64 columns) are issued together,
        // and those of the first round before the headers are staged, so that the two latencies overlap
        for (int cb = 0; cb < small; cb += 64 * TB_CB) {
            float gvs[TB_ROWS / TB_WAVES][TB_CB];
#pragma unroll
            for (int k = 0; k < TB_ROWS / TB_WAVES; ++k)
#pragma unroll
                for (int u = 0; u < TB_CB; ++u) {
                    const int r = wave + k * TB_WAVES, c = cb + 64 * u + lane;
                    gvs[k][u] = (r < nr && c < small) ? g0[(size_t)r * set.lddl + c] : 0.f;
                }
            if (cb == 0) {
                stage_headers(p, set.xcols, &dummy, reinterpret_cast<const XT*>(set.x), r_lo, nr, hd, TB_THREADS);
                __syncthreads();
                for (int i = threadIdx.x; i < nr4 * 4; i += TB_THREADS) {
                    const int r = i >> 2, k = i & 3;
                    const bool ok = r < nr && fe_finite(s_sen[r * 4]) && fe_finite(s_sen[r * 4 + 1]) && fe_finite(s_sen[r * 4 + 2]);
                    s_sa[i] = ok ? (k < 3 ? s_sen[i] : 1.f) : 0.f;
                }
                for (int i = nr * FE_HDR + threadIdx.x; i < nr4 * FE_HDR; i += TB_THREADS) s_idx[i] = -1;
            }
#pragma unroll
            for (int k = 0; k < TB_ROWS / TB_WAVES; ++k) {
                const int r = wave + k * TB_WAVES;
                if (r >= nr4) break;
                const int* hi = s_idx + r * FE_HDR;
#pragma unroll
                for (int u = 0; u < TB_CB; ++u) {
                    const int c = cb + 64 * u + lane;
                    if (c >= small) break;
                    const float gv = gvs[k][u];
                    float v = 0.f;
                    if (r < nr) {
                        const bool fin = fe_finite(gv);
                        if (c < e1) {
                            const float s0 = s_sen[r * 4], s1 = s_sen[r * 4 + 1], s2 = s_sen[r * 4 + 2];
                            const f32x4 wb = *reinterpret_cast<const f32x4*>(s_wb + 4 * c);
                            const float pre = wb[3] + wb[0] * s0 + wb[1] * s1 + wb[2] * s2;
                            const bool on = pre > 0.f && gv != 0.f;                      // ReLU'
                            const bool slow = !fin || !(fe_finite(s0) && fe_finite(s1) && fe_finite(s2));
                            if (__ballot(slow)) {
                                if (slow && on) {
                                    atomicAdd(p.d_sen_w + c * 3 + 0, gv * s0);
                                    atomicAdd(p.d_sen_w + c * 3 + 1, gv * s1);
                                    atomicAdd(p.d_sen_w + c * 3 + 2, gv * s2);
                                    atomicAdd(p.d_sen_b + c, gv);
                                }
                            }
                            v = (on && !slow) ? gv : 0.f;
                        } else {
                            if (__ballot(!fin)) {
                                if (!fin) {
                                    if (c < e1 + e2) {
                                        atomicAdd(p.d_type_tab + hi[5] * e2 + (c - e1), gv);
                                    } else {
                                        const int kk = c - e1 - e2;
                                        atomicAdd(p.d_year_tab + hi[0] * e3 + kk, gv);
                                        atomicAdd(p.d_month_tab + hi[1] * e3 + kk, gv);
                                        atomicAdd(p.d_day_tab + hi[2] * e3 + kk, gv);
                                        atomicAdd(p.d_hour_tab + hi[3] * e3 + kk, gv);
                                    }
                                }
                            }
                            v = fin ? gv : 0.f;
                        }
                    }
                    s_b[r * ldb + c] = v;
                }
            }
        }
        __syncthreads();
        // A comes from one LDS word per lane and tile: the row's index in slot hdr, or the row's A entry of the sentiment layer
        const int* s_a = reinterpret_cast<const int*>(s_sa);
        const int a_sen = lk * 4 + (li & 3), a_idx = TB_ROWS * 4 + lk * FE_HDR;
        for (int r0 = 0; r0 < nr4; r0 += 4) {
            // (the tile is decoded here, on the scalar unit: hoisted out of the loops the decoded fields cost 4 registers a tile;
            //  all LDS reads of a step are issued before its first MFMA, and the choice between the two kinds of A is bitwise)
            float b[NT];
            int raw[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                int d = t_desc[t];
                asm volatile("" : "+s"(d));
                const int hdr = (d & 7) - 1, coff = d >> 18;
                b[t] = s_b[(r0 + lk) * ldb + coff + li];
                raw[t] = s_a[hdr >= 0 ? r0 * FE_HDR + a_idx + hdr : r0 * 4 + a_sen];
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                int d = t_desc[t];
                asm volatile("" : "+s"(d));
                const int m = (d & 7) ? -1 : 0, ibase = (d >> 3) & 0x7fff;
                const int one_hot = raw[t] == ibase + li ? __float_as_int(1.f) : 0, sen = li < 4 ? raw[t] : 0;
                acc[t] = mfma16(__int_as_float((one_hot & m) | (sen & ~m)), b[t], acc[t]);
            }
        }
    }
    // the partial tables of this workgroup: every cell is written by exactly one tile
    float* part = q.ws + (size_t)blockIdx.x * q.cells;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < my_nt) {
            const TabTile& d = q.tile[t_lo + t];
            const int nrow = d.hdr >= 0 ? min(16, (d.hdr == 5 ? p.n_type : d.hdr == 0 ? p.n_year : d.hdr == 1 ? p.n_month : d.hdr == 2 ? p.n_day : p.n_hour) - d.ibase) : 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 4 * lk + k;
                if (row < nrow && li < d.ncol) part[d.dst + row * d.ldr + li * d.ldc] = acc[t][k];
            }
        }
    }
}

// arena += the partials, summed in a fixed order: a cell's TB_RED_SLICES slices of the partials one after the other, then slice 0 + 1 + ...
__global__ __launch_bounds__(TB_RED_CELLS * TB_RED_SLICES) void tab_reduce_kernel(const FrontendParams p, const float* __restrict__ ws, int nparts, int cells) {
    __shared__ float s[TB_RED_SLICES][TB_RED_CELLS];
    const int cl = threadIdx.x & (TB_RED_CELLS - 1), slice = threadIdx.x / TB_RED_CELLS;
    const int cell = blockIdx.x * TB_RED_CELLS + cl;
    const int per = (nparts + TB_RED_SLICES - 1) / TB_RED_SLICES;
    float v = 0.f;
    if (cell < cells) {
        const int g_hi = min(nparts, (slice + 1) * per);
        int g = slice * per;
        for (; g + 8 <= g_hi; g += 8) {
            float t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = ws[(size_t)(g + k) * cells + cell];
#pragma unroll
            for (int k = 0; k < 8; ++k) v += t[k];
        }
        for (; g < g_hi; ++g) v += ws[(size_t)g * cells + cell];
    }
    s[slice][cl] = v;
    __syncthreads();
    if (slice || cell >= cells) return;
    v = s[0][cl];
#pragma unroll
    for (int k = 1; k < TB_RED_SLICES; ++k) v += s[k][cl];
    int i = cell;
    float* dst;
    if (i < p.n_type * p.e2) dst = p.d_type_tab + i;
    else if ((i -= p.n_type * p.e2) < p.n_year * p.e3) dst = p.d_year_tab + i;
    else if ((i -= p.n_year * p.e3) < p.n_month * p.e3) dst = p.d_month_tab + i;
    else if ((i -= p.n_month * p.e3) < p.n_day * p.e3) dst = p.d_day_tab + i;
    else if ((i -= p.n_day * p.e3) < p.n_hour * p.e3) dst = p.d_hour_tab + i;
    else { i -= p.n_hour * p.e3; dst = (i & 3) < 3 ? p.d_sen_w + (i >> 2) * 3 + (i & 3) : p.d_sen_b + (i >> 2); }
    *dst += v;
}

// tiles, cells and LDS of a shape; false: the shape is left to frontend_bwd_kernel
struct TabPlan { int ntiles, cells, ldb; size_t shm; };
static bool tab_plan(const FrontendParams& p, TabPlan* pl) {
    if (p.e1 <= 0 || p.e2 <= 0 || p.e3 <= 0 || p.n_type <= 0 || p.n_year <= 0 || p.n_month <= 0 || p.n_day <= 0 || p.n_hour <= 0) return false;
    const long n_time = (long)p.n_year + p.n_month + p.n_day + p.n_hour;
    if (n_time > 30000 || p.n_type > 30000 || (long)p.e1 + p.e2 + p.e3 > 4096) return false;       // (TabTile holds shorts)
    auto up = [](int n) { return (n + 15) / 16; };
    const long tiles = (long)up(p.e1) + (long)up(p.n_type) * up(p.e2) +
                       (long)(up(p.n_year) + up(p.n_month) + up(p.n_day) + up(p.n_hour)) * up(p.e3);
    if (tiles > TB_MAXTILES) return false;
    const int small = p.e1 + p.e2 + p.e3;
    pl->ntiles = (int)tiles;
    pl->cells = p.n_type * p.e2 + (int)n_time * p.e3 + 4 * p.e1;
    pl->ldb = (small + 63) / 64 * 64 + 16;             // >= small + 16 (ragged tiles read past the width), rows 16 banks apart
    pl->shm = sizeof(float) * ((size_t)TB_ROWS * pl->ldb + 4 * (size_t)p.e1 + (size_t)TB_ROWS * (8 + FE_HDR));
    return pl->shm <= 64 * 1024;
}

static void tab_grid(long nrows0, long nrows1, int* grid, int* chunks_per_wg) {
    const long nchunks = (nrows0 + TB_ROWS - 1) / TB_ROWS + (nrows1 + TB_ROWS - 1) / TB_ROWS;
    const long cap = (long)TB_WG_PER_CU * device_cus();
    const long per = std::max<long>(1, (nchunks + cap - 1) / cap);
    *chunks_per_wg = (int)per;
    *grid = (int)((nchunks + per - 1) / per);            // every workgroup has at least one chunk
}

long tab_grad_ws_floats(const FrontendParams& p, long nrows_total) {
    TabPlan pl;
    if (nrows_total <= 0 || nrows_total >= (1L << 31) - 2 * TB_ROWS || p.n_sub > FE_MAXSUB || !tab_plan(p, &pl)) return 0;
    // (two row sets have at most one chunk more than one set of as many rows)
    const long nchunks = (nrows_total + TB_ROWS - 1) / TB_ROWS + 1;
    return std::min<long>(nchunks, (long)TB_WG_PER_CU * device_cus()) * pl.cells;
}

hipError_t tab_grad_launch(const FrontendParams& p, const void* x0, int nrows0, int xcols0, const float* dlab0, int lddl0,
                           const void* x1, int nrows1, int xcols1, const float* dlab1, int lddl1, int x_is_f64, float* ws, hipStream_t st) {
    if ((long)nrows0 + nrows1 <= 0) return hipSuccess;
    TabParams q = {};
    TabPlan pl;
    if (p.n_sub > FE_MAXSUB || !tab_plan(p, &pl)) return hipErrorInvalidValue;
    q.p = p;
    q.set[0] = {x0, dlab0, nrows0, xcols0, lddl0, (nrows0 + TB_ROWS - 1) / TB_ROWS};
    q.set[1] = {x1, dlab1, nrows1, xcols1, lddl1, (nrows1 + TB_ROWS - 1) / TB_ROWS};
    q.ntiles = pl.ntiles; q.cells = pl.cells; q.ldb = pl.ldb; q.ws = ws;
    q.tiles_per_wave = (pl.ntiles + TB_WAVES - 1) / TB_WAVES;
    int grid = 0;
    tab_grid(nrows0, nrows1, &grid, &q.chunks_per_wg);
    // the tiles, in the order of the cells of a partial: type, year, month, day, hour, sentiment
    int nt = 0, cell = 0;
    auto table = [&](int hdr, int n, int e, int coff) {
        for (int ib = 0; ib < n; ib += 16)
            for (int c = 0; c < e; c += 16)
                q.tile[nt++] = {(short)hdr, (short)ib, (short)(coff + c), (short)std::min(16, e - c), cell + ib * e + c, (short)e, 1};
        cell += n * e;
    };
    table(5, p.n_type, p.e2, p.e1);
    table(0, p.n_year, p.e3, p.e1 + p.e2);
    table(1, p.n_month, p.e3, p.e1 + p.e2);
    table(2, p.n_day, p.e3, p.e1 + p.e2);
    table(3, p.n_hour, p.e3, p.e1 + p.e2);
    for (int c = 0; c < p.e1; c += 16) q.tile[nt++] = {-1, 0, (short)c, (short)std::min(16, p.e1 - c), cell + 4 * c, 1, 4};
    if (nt != pl.ntiles || cell + 4 * p.e1 != pl.cells) return hipErrorInvalidValue;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(TB_THREADS), pl.shm, st, q); };
    if (q.tiles_per_wave <= 4)      x_is_f64 ? launch(tab_grad_kernel<double, 4>) : launch(tab_grad_kernel<float, 4>);
    else if (q.tiles_per_wave <= 8) x_is_f64 ? launch(tab_grad_kernel<double, 8>) : launch(tab_grad_kernel<float, 8>);
    else                            x_is_f64 ? launch(tab_grad_kernel<double, TB_MAXT>) : launch(tab_grad_kernel<float, TB_MAXT>);
    hipLaunchKernelGGL(tab_reduce_kernel, dim3((pl.cells + TB_RED_CELLS - 1) / TB_RED_CELLS), dim3(TB_RED_CELLS * TB_RED_SLICES), 0, st, p, ws, grid, pl.cells);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Category-table gradient without one float atomic per reference.  A row refers to the table 1 + NS times (its category, weight
// 1, and its NS sub-category slots, weight 1/NS each); the scatter above costs (1 + NS) * e0 float atomics per row, and float
// atomics run at 65-165 G/s chip-wide (L2 atomic units; one private copy of the table per XCD changed nothing), which made this
// the slowest small kernel of a step (0.59 ms at C3, 0.21 of a 1.5 ms step at the reference's default sizes).  Instead:
//   count   histogram of the references' category ids
//   scan    exclusive prefix -> first slot of every id
//   fill    counting sort: reference i goes to slot start[id] + cursor[id]++
//   gather  one wave per chunk of 64 SORTED references: it walks them in order, sums weight * dlab[row, :e0] in registers
//           while the id stays the same and adds a finished run to its table row (float atomics: one run per id and chunk,
//           ~N/64 + n_cat runs instead of N references)
// Count and fill take no global atomic per reference where the histogram fits the LDS (n_cat <= CAT_LDS_MAX): a workgroup
// histograms a contiguous slice of the references in LDS and writes its row of counts; cat_colscan_kernel turns every id's column
// of counts into the slice's offset inside the id's run (and the id's total); the fill re-reads the slice and places its
// references with LDS atomics from start[id] + offset.  A larger n_cat keeps the global counters and cursors.
// Both row sets of a step (history and candidate rows) go through one sort.  Order inside a run depends on the fill's atomics,
// so sums differ in the last bits from run to run -- as the atomic scatter's did.
struct CatRefs {
    const void* x[2]; const float* dlab[2];
    int nrows[2], xcols[2], lddl[2];
    int c_cat, NS, n_cat, e0;
    long nref;                                     // (nrows[0] + nrows[1]) * (NS + 1)
};

template <typename XT>
__global__ __launch_bounds__(256) void cat_count_kernel(const CatRefs p, int* __restrict__ count, int* __restrict__ cat_of) {
    const int S = p.NS + 1;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.nref; i += (long)gridDim.x * 256) {
        long r = i / S;
        const int j = (int)(i - r * S);
        const int set = r >= p.nrows[0];
        if (set) r -= p.nrows[0];
        const XT* xr = reinterpret_cast<const XT*>(p.x[set]) + (size_t)r * p.xcols[set];
        int c = (int)xr[p.c_cat + j];
        c = c < 0 ? 0 : (c >= p.n_cat ? p.n_cat - 1 : c);                 // (out-of-range ids were flagged by the forward)
        cat_of[i] = c;
        atomicAdd(count + c, 1);
    }
}

__global__ __launch_bounds__(1024) void cat_scan_kernel(const int* __restrict__ count, int* __restrict__ start, int n) {
    __shared__ int part[1024];
    const int per = (n + 1023) / 1024;
    const int lo = threadIdx.x * per, hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                           // inclusive scan of the 1024 partial sums
        const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (int i = lo; i < hi; ++i) { start[i] = run; run += count[i]; }
    if (threadIdx.x == 1023) start[n] = part[1023];
}

__global__ __launch_bounds__(256) void cat_fill_kernel(long nref, const int* __restrict__ cat_of, const int* __restrict__ start,
                                                       int* __restrict__ cursor, int* __restrict__ refs, int* __restrict__ refcat) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nref; i += (long)gridDim.x * 256) {
        const int c = cat_of[i];
        const int pos = start[c] + atomicAdd(cursor + c, 1);
        refs[pos] = (int)i;
        refcat[pos] = c;
    }
}

constexpr int CAT_COLS = 8;                        // column chunks of 64 per lane: e0 <= 512
__global__ __launch_bounds__(256) void cat_gather_kernel(const CatRefs p, const int* __restrict__ refs, const int* __restrict__ refcat,
                                                         float* __restrict__ d_cat) {
    const int lane = threadIdx.x & 63;
    const long chunk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long base = chunk * 64;
    if (base >= p.nref) return;
    const int S = p.NS + 1;
    const float inv_ns = 1.0f / (float)p.NS;
    const int my_ref = base + lane < p.nref ? refs[base + lane] : -1;
    const int my_cat = base + lane < p.nref ? refcat[base + lane] : -1;
    const int n_here = (int)min((long)64, p.nref - base);
    float acc[CAT_COLS];
#pragma unroll
    for (int k = 0; k < CAT_COLS; ++k) acc[k] = 0.f;
    int cur = __builtin_amdgcn_readfirstlane(my_cat);
    auto flush = [&](int c) {
        float* row = d_cat + (size_t)c * p.e0;
#pragma unroll
        for (int k = 0; k < CAT_COLS; ++k) {
            if (64 * k + lane < p.e0) atomicAdd(row + 64 * k + lane, acc[k]);
            acc[k] = 0.f;
        }
    };
    for (int t0 = 0; t0 < n_here; t0 += 4) {
        // the rows of four references are requested together (nothing between them depends on the run bookkeeping)
        float v[4][CAT_COLS];
        int cs[4];
        float ws[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u;
            const int i = __builtin_amdgcn_readlane(my_ref, t & 63);
            cs[u] = t < n_here ? __builtin_amdgcn_readlane(my_cat, t & 63) : -1;
            long r = i / S;
            const int j = i - (int)r * S;
            ws[u] = j ? inv_ns : 1.0f;
            const int set = r >= p.nrows[0];
            if (set) r -= p.nrows[0];
            const float* g = p.dlab[set] + (size_t)r * p.lddl[set];
#pragma unroll
            for (int k = 0; k < CAT_COLS; ++k) v[u][k] = (t < n_here && 64 * k + lane < p.e0) ? g[64 * k + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (cs[u] < 0) break;
            if (cs[u] != cur) { flush(cur); cur = cs[u]; }
#pragma unroll
            for (int k = 0; k < CAT_COLS; ++k) acc[k] = fmaf(ws[u], v[u][k], acc[k]);
        }
    }
    flush(cur);
}

constexpr int CAT_LDS_MAX = 16384;                // ids whose histogram fits 64 KB of LDS
constexpr int CAT_SLICE = 4096;                    // references per workgroup (more where that gives over CAT_MAX_GROUPS workgroups)
constexpr int CAT_MAX_GROUPS = 256;
static int cat_groups(long nref) { return (int)std::max<long>(1, std::min<long>(CAT_MAX_GROUPS, (nref + CAT_SLICE - 1) / CAT_SLICE)); }

template <typename XT>
__global__ __launch_bounds__(1024) void cat_hist_kernel(const CatRefs p, int slice, int* __restrict__ hist, int* __restrict__ cat_of) {
    extern __shared__ int h[];                                             // [n_cat]
    for (int i = threadIdx.x; i < p.n_cat; i += 1024) h[i] = 0;
    __syncthreads();
    const int S = p.NS + 1;
    const long lo_l = (long)blockIdx.x * slice, hi_l = lo_l + slice;
    const int lo = (int)(lo_l < p.nref ? lo_l : p.nref), hi = (int)(hi_l < p.nref ? hi_l : p.nref);
    for (int i = lo + threadIdx.x; i < hi; i += 1024) {
        int r = i / S;
        const int j = i - r * S;
        const int set = r >= p.nrows[0];
        if (set) r -= p.nrows[0];
        const XT* xr = reinterpret_cast<const XT*>(p.x[set]) + (size_t)r * p.xcols[set];
        int c = (int)xr[p.c_cat + j];
        c = c < 0 ? 0 : (c >= p.n_cat ? p.n_cat - 1 : c);                 // (out-of-range ids were flagged by the forward)
        cat_of[i] = c;
        atomicAdd(h + c, 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < p.n_cat; i += 1024) hist[(size_t)blockIdx.x * p.n_cat + i] = h[i];
}

// hist[g][c]: count of id c in slice g -> the slice's offset inside the id's run; count[c] = the id's total.  A workgroup takes
// 64 ids, four threads an id: each sums a quarter of the groups, the quarters are chained through LDS, and each writes its offsets
__global__ __launch_bounds__(256) void cat_colscan_kernel(int* __restrict__ hist, int* __restrict__ count, int groups, int n_cat) {
    __shared__ int part[4][64];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int per = (groups + 3) / 4, g_lo = min(groups, q * per), g_hi = min(groups, g_lo + per);
    int sum = 0;
    if (c < n_cat) {
        int g = g_lo;
        for (; g + 8 <= g_hi; g += 8) {
            int t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = hist[(size_t)(g + k) * n_cat + c];
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += t[k];
        }
        for (; g < g_hi; ++g) sum += hist[(size_t)g * n_cat + c];
    }
    part[q][cl] = sum;
    __syncthreads();
    if (c >= n_cat) return;
    int run = 0;
    for (int k = 0; k < q; ++k) run += part[k][cl];
    if (q == 3) count[c] = run + sum;
    int g = g_lo;
    for (; g + 8 <= g_hi; g += 8) {
        int t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = hist[(size_t)(g + k) * n_cat + c];
#pragma unroll
        for (int k = 0; k < 8; ++k) { hist[(size_t)(g + k) * n_cat + c] = run; run += t[k]; }
    }
    for (; g < g_hi; ++g) {
        const int v = hist[(size_t)g * n_cat + c];
        hist[(size_t)g * n_cat + c] = run;
        run += v;
    }
}

__global__ __launch_bounds__(1024) void cat_place_kernel(long nref, int slice, int n_cat, const int* __restrict__ cat_of,
                                                         const int* __restrict__ start, const int* __restrict__ hist,
                                                         int* __restrict__ refs, int* __restrict__ refcat) {
    extern __shared__ int h[];                                             // [n_cat] next slot of every id for this slice
    for (int i = threadIdx.x; i < n_cat; i += 1024) h[i] = start[i] + hist[(size_t)blockIdx.x * n_cat + i];
    __syncthreads();
    const long lo_l = (long)blockIdx.x * slice, hi_l = lo_l + slice;
    const int lo = (int)(lo_l < nref ? lo_l : nref), hi = (int)(hi_l < nref ? hi_l : nref);
    for (int i = lo + threadIdx.x; i < hi; i += 1024) {
        const int c = cat_of[i];
        const int pos = atomicAdd(h + c, 1);
        refs[pos] = i;
        refcat[pos] = c;
    }
}

long cat_grad_ws_ints(int n_cat, long nrows_total, int n_sub) {
    const long nref = nrows_total * (n_sub + 1);
    return 3L * n_cat + 4 + 3L * nref + (n_cat <= CAT_LDS_MAX ? (long)cat_groups(nref) * n_cat : 0);
}

hipError_t cat_grad_launch(const void* x0, int nrows0, int xcols0, const float* dlab0, int lddl0,
                           const void* x1, int nrows1, int xcols1, const float* dlab1, int lddl1, int x_is_f64,
                           int P, int n_sub, int n_cat, int e0, float* d_cat, int* ws, hipStream_t st) {
    CatRefs p = {};
    p.x[0] = x0; p.x[1] = x1; p.dlab[0] = dlab0; p.dlab[1] = dlab1;
    p.nrows[0] = nrows0; p.nrows[1] = nrows1; p.xcols[0] = xcols0; p.xcols[1] = xcols1; p.lddl[0] = lddl0; p.lddl[1] = lddl1;
    p.c_cat = 4 + P; p.NS = n_sub; p.n_cat = n_cat; p.e0 = e0;
    p.nref = ((long)nrows0 + nrows1) * (n_sub + 1);
    if (p.nref <= 0) return hipSuccess;
    if (e0 > 64 * CAT_COLS || n_sub < 1 || p.nref >= (1L << 31)) return hipErrorInvalidValue;
    int* count = ws;
    int* cursor = ws + n_cat;
    int* start = ws + 2 * n_cat;                   // n_cat + 1 entries
    int* cat_of = ws + 3 * n_cat + 4;
    int* refs = cat_of + p.nref;
    int* refcat = refs + p.nref;
    if (n_cat <= CAT_LDS_MAX) {
        int* hist = refcat + p.nref;                 // [groups][n_cat]
        const int groups = cat_groups(p.nref);
        const int slice = (int)((p.nref + groups - 1) / groups);
        const size_t shm = sizeof(int) * (size_t)n_cat;
        if (x_is_f64) hipLaunchKernelGGL(cat_hist_kernel<double>, dim3(groups), dim3(1024), shm, st, p, slice, hist, cat_of);
        else          hipLaunchKernelGGL(cat_hist_kernel<float>, dim3(groups), dim3(1024), shm, st, p, slice, hist, cat_of);
        hipLaunchKernelGGL(cat_colscan_kernel, dim3((n_cat + 63) / 64), dim3(256), 0, st, hist, count, groups, n_cat);
        hipLaunchKernelGGL(cat_scan_kernel, dim3(1), dim3(1024), 0, st, count, start, n_cat);
        hipLaunchKernelGGL(cat_place_kernel, dim3(groups), dim3(1024), shm, st, p.nref, slice, n_cat, cat_of, start, hist, refs, refcat);
    } else {
        hipError_t e = hipMemsetAsync(count, 0, sizeof(int) * 2 * (size_t)n_cat, st);
        if (e != hipSuccess) return e;
        const unsigned blocks = (unsigned)std::min<long>((p.nref + 255) / 256, 2048);
        if (x_is_f64) hipLaunchKernelGGL(cat_count_kernel<double>, dim3(blocks), dim3(256), 0, st, p, count, cat_of);
        else          hipLaunchKernelGGL(cat_count_kernel<float>, dim3(blocks), dim3(256), 0, st, p, count, cat_of);
        hipLaunchKernelGGL(cat_scan_kernel, dim3(1), dim3(1024), 0, st, count, start, n_cat);
        hipLaunchKernelGGL(cat_fill_kernel, dim3(blocks), dim3(256), 0, st, p.nref, cat_of, start, cursor, refs, refcat);
    }
    const long chunks = (p.nref + 63) / 64;
    hipLaunchKernelGGL(cat_gather_kernel, dim3((unsigned)((chunks + 3) / 4)), dim3(256), 0, st, p, refs, refcat, d_cat);
    return hipGetLastError();
}

}  // namespace nrm
