// A step's batch written on the device from resident tables: the loop body of the reference's ETL
// (tool/process_data.py:190-252, batch_type 0 and 2) as ONE gather kernel.  The processed record copies an article's row into every
// impression that mentions it; here the article rows, the users' events and the impressions' lists stay in HBM as index-based tables and a
// step's x_history / x_target / x_global / label / label_id / empty_num are written from a list of impression indices.
//
// One wave per 16 rows of one impression (history rows, or candidate slots).  Its lanes 0..15 fetch the rows' metadata -- article, time,
// read time, scroll: one coalesced load per structure-of-arrays column -- and run the float64 bucket arithmetic once per row; the four
// buckets travel as one packed word.  Then all 64 lanes walk the 16 rows as ONE run of consecutive units (a unit = V elements: 16 bytes
// where V * sizeof = 16), taking the row's metadata from its lane by a shuffle: unit 0 of a row is the four buckets, the middle units are
// straight copies of the aligned art_static row, the last one splices read time and scroll behind the type.  A padded row is written in full
// as +0.0.  The candidate waves first find the source of slot T - 1 with one pass over the impression's list (ballots, no atomics).
// Reads of art_static and all row stores go through bounded buffer descriptors; every index is clamped to its array before a plain load.
// Which impression a wave works on is sel[b], or sel[*cursor + b] with a cursor that lives on the device (nrm_assemble_batch_at): that launch
// depends on no host data, so a captured step assembles another batch at every replay (csrc/epoch.hip moves the cursor).
#include <cstdint>
#include <climits>
#include "common.hpp"
#include "assemble.hpp"
#include "compact.hpp"

namespace nrm {

constexpr int ASM_ROWS = 16;          // rows of one wave
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

// tool/normalization.py sec_norm, in its own float64 arithmetic (NOT integer arithmetic on microseconds: the float subtraction leaves a
// residue at bucket borders that the next division sees): year | month << 12 | day << 16 | hour << 21.  std * k is exact in float64, so a
// contraction into an fma changes nothing.
__device__ __forceinline__ unsigned time_buckets(long dt_us) {
    double sec = fmax(0.0, (double)dt_us / 1e6);
    const double stds[4] = {31536000.0, 2592000.0, 86400.0, 3600.0};
    const double caps[4] = {3000.0, 12.0, 30.0, 23.0};
    const int shifts[4] = {0, 12, 16, 21};
    unsigned pack = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double k = fmin(floor(sec / stds[i]), caps[i]);
        sec -= stds[i] * k;
        pack |= (unsigned)(int)k << shifts[i];
    }
    return pack;
}
__device__ __forceinline__ int bucket_of(unsigned pack, int e) {
    return e == 0 ? (int)(pack & 0xfffu) : e == 1 ? (int)((pack >> 12) & 0xfu) : e == 2 ? (int)((pack >> 16) & 0x1fu) : (int)((pack >> 21) & 0x1fu);
}

// a wave-uniform address the compiler formed in vector registers (a 64-bit product of the wave's impression): as two scalars, so that the
// descriptor built on it is scalar and no buffer operation is wrapped in a loop over "distinct" descriptors
template <typename P> __device__ __forceinline__ P* uniform_ptr(P* p) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return reinterpret_cast<P*>(((uint64_t)hi << 32) | lo);
}

template <int NW> __device__ __forceinline__ void unit_load(unsigned (&w)[NW], const __amdgpu_buffer_rsrc_t rs, unsigned voff) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (NW == 1) {
        w[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0);
    } else if constexpr (NW == 2) {
        const auto x = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 0, 0);
        w[0] = x[0]; w[1] = x[1];
    } else {
#pragma unroll
        for (int i = 0; i < NW / 4; ++i) {
            const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + 16u * i, 0, 0);
            w[4 * i] = x[0]; w[4 * i + 1] = x[1]; w[4 * i + 2] = x[2]; w[4 * i + 3] = x[3];
        }
    }
#endif
}
template <int NW> __device__ __forceinline__ void unit_store(const unsigned (&w)[NW], const __amdgpu_buffer_rsrc_t rs, unsigned voff) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (NW == 1) {
        __builtin_amdgcn_raw_buffer_store_b32(w[0], rs, voff, 0, 0);
    } else if constexpr (NW == 2) {
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{w[0], w[1]}, rs, voff, 0, 0);
    } else {
#pragma unroll
        for (int i = 0; i < NW / 4; ++i) store_b128_guarded(u32x4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]}, rs, voff + 16u * i, 0);
    }
#endif
}

// The wave's nrows rows (lane r < nrows holds row r's article -- -1: a padded row --, packed buckets, read time and scroll), written to
// rows row0 .. row0 + nrows - 1 of the [*, cols] block behind rs_out as one run of units of V elements.  The shuffles run with the whole
// wave active (a bpermute reads 0 from a lane that is switched off).
template <typename T, int V>
__device__ __forceinline__ void write_rows(const __amdgpu_buffer_rsrc_t rs_out, const __amdgpu_buffer_rsrc_t rs_static, int row0, int nrows, int cols,
                                           int S, int Sw, bool behaviour, int my_art, unsigned my_pack, T my_read, T my_scroll) {
    constexpr int NW = V * (int)sizeof(T) / 4;
    const int lane = threadIdx.x & 63;
    const int upr = cols / V, total = nrows * upr;
    for (int g0 = 0; g0 < total; g0 += 64) {
        const int g = g0 + lane;
        const bool active = g < total;
        const int r = active ? g / upr : 0;
        const int art = __shfl(my_art, r);
        const unsigned pack = __shfl(my_pack, r);
        const T rd = __shfl(my_read, r), sc = __shfl(my_scroll, r);
        if (!active) continue;
        const int e0 = (g - r * upr) * V;
        T v[V];
        unsigned w[NW];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = T(0);
        if (art >= 0) {
            if (e0 < 4) {                                             // V divides 4: a unit holds buckets only
#pragma unroll
                for (int k = 0; k < V; ++k) v[k] = (T)bucket_of(pack, e0 + k);
            } else {
                if (e0 - 4 < Sw) {
                    unit_load<NW>(w, rs_static, ((unsigned)art * (unsigned)S + (unsigned)(e0 - 4)) * (unsigned)sizeof(T));
                    __builtin_memcpy(v, w, sizeof(v));
                }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int c = e0 - 4 + k;
                    if (c >= Sw) v[k] = !behaviour ? T(0) : c == Sw ? rd : c == Sw + 1 ? sc : T(0);
                }
            }
        }
        __builtin_memcpy(w, v, sizeof(v));
        unit_store<NW>(w, rs_out, (unsigned)((row0 + r) * cols + e0) * (unsigned)sizeof(T));
    }
}

// The impression of place b of the batch: sel[b], or with a device-side cursor sel[*cursor + b] (one uniform load per wave: the pointer is a
// kernel argument).  The cursor is first brought into [-B, n_order] -- beyond either end every place of the batch is outside anyway, and
// the sum below cannot overflow -- then the place is clamped into sel and reported like an entry outside the table.
__device__ __forceinline__ long wave_impression(const AssembleParams& p, int b, int lane) {
    long pos = b;
    if (p.cursor) pos += min(max(*p.cursor, -(long)p.B), p.n_order);
    const bool off_end = pos < 0 || pos >= p.n_order;
    long n = p.sel[min(max(pos, 0L), p.n_order - 1)];
    if (off_end || n < 0 || n >= p.t.N) {
        if (lane == 0) *p.t.err = 1;
        n = min(max(n, 0L), p.t.N - 1);
    }
    return n;
}

// The in-view position slot T - 1 takes (>= L: it stays empty): one pass of the wave over the impression's list (ballots, no atomics).
__device__ __forceinline__ int last_slot_pos(const int* list, int L, int target, int T1, bool keep_target_slot, int lane) {
    if (!keep_target_slot) return T1;
    bool early = false;
    int late = -1;
    if (target >= 0) {
        for (int i0 = 0; i0 < L && !early && late < 0; i0 += 64) {
            const int i = i0 + lane;
            const bool hit = i < L && list[i] == target;
            early = __any(hit && i < T1);
            const unsigned long long m = __ballot(hit && i >= T1);
            if (m) late = i0 + __ffsll((long long)m) - 1;
        }
    }
    return early ? T1 : late >= 0 ? late : L;
}

template <typename T, int VH, int VT>
__global__ __launch_bounds__(256) void assemble_kernel(const AssembleParams p) {
    const nrm_assemble_tables& t = p.t;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nh = (p.H + ASM_ROWS - 1) / ASM_ROWS, nt = (p.T + ASM_ROWS - 1) / ASM_ROWS, per = nh + nt;
    const long item = (long)blockIdx.x * 4 + wave;
    if (item >= (long)p.B * per) return;
    const int b = (int)(item / per), w = (int)(item - (long)b * per);
    const long n = wave_impression(p, b, lane);
    const int u = (int)min(max((long)t.imp_user[n], 0L), t.U - 1);
    const long t_imp = t.imp_time_us[n];
    const int Sw = t.static_cols, S = t.S, amax = (int)t.A - 1;
    const __amdgpu_buffer_rsrc_t rs_static = buffer_rsrc(t.art_static, (unsigned)(t.A * S * (long)sizeof(T)));
    if (w < nh) {                                                      // 16 history rows
        const int hc = 4 + Sw + 2;
        const long off = min(max(t.user_off[u], 0L), t.E);
        const int cnt = (int)min(min(max(t.user_off[u + 1], off), t.E) - off, (long)p.H);
        const int j0 = w * ASM_ROWS, nrows = min(ASM_ROWS, p.H - j0), j = j0 + lane;
        int art = -1;
        unsigned pack = 0;
        T rd = T(0), sc = T(0);
        if (lane < nrows && j < cnt) {
            art = min(max(t.ev_art[off + j], 0), amax);
            pack = time_buckets(t_imp - t.ev_time_us[off + j]);
            rd = static_cast<const T*>(t.ev_read)[off + j];
            sc = static_cast<const T*>(t.ev_scroll)[off + j];
        }
        const __amdgpu_buffer_rsrc_t rs_out = buffer_rsrc(uniform_ptr(static_cast<T*>(t.x_history) + (long)b * p.H * hc), (unsigned)((long)p.H * hc * (long)sizeof(T)));
        write_rows<T, VH>(rs_out, rs_static, j0, nrows, hc, S, Sw, true, art, pack, rd, sc);
        if (w == 0 && lane == 0) {
            t.history_len[b] = cnt;
            t.user_id_out[b] = t.user_id[u];
            t.impression_id[b] = t.imp_id[n];
        }
        return;
    }
    // 16 candidate slots
    const int tc = 4 + Sw, wc = w - nh, T1 = p.T - 1;
    const long loff = min(max(t.imp_off[n], 0L), t.L);
    const int L = (int)min(min(max(t.imp_off[n + 1], loff), t.L) - loff, (long)INT_MAX);
    const int* list = t.imp_inview + loff;
    const int target = t.imp_target[n];                                // -1: none
    const int last_pos = last_slot_pos(list, L, target, T1, p.keep_target_slot != 0, lane);
    const int s0 = wc * ASM_ROWS, nrows = min(ASM_ROWS, p.T - s0), s = s0 + lane;
    int art = -1;
    unsigned pack = 0;
    if (lane < nrows) {
        const int pos = s == T1 ? last_pos : s;
        const bool live = pos < L;
        double lab = 0.0;
        long id = -1;
        T gl[3] = {T(0), T(0), T(0)};
        if (live) {
            const int raw = list[pos];
            art = min(max(raw, 0), amax);
            pack = time_buckets(t_imp - t.art_pub_us[art]);
            lab = (target >= 0 && raw == target) ? 1.0 : 0.0;
            id = t.art_id[art];
#pragma unroll
            for (int k = 0; k < 3; ++k) gl[k] = static_cast<const T*>(t.art_global)[(long)art * 3 + k];
        }
        const long cell = (long)b * p.T + s;
        t.label[cell] = lab;
        t.label_id[cell] = id;
#pragma unroll
        for (int k = 0; k < 3; ++k) static_cast<T*>(t.x_global)[cell * 3 + k] = gl[k];
    }
    const __amdgpu_buffer_rsrc_t rs_out = buffer_rsrc(uniform_ptr(static_cast<T*>(t.x_target) + (long)b * p.T * tc), (unsigned)((long)p.T * tc * (long)sizeof(T)));
    write_rows<T, VT>(rs_out, rs_static, s0, nrows, tc, S, Sw, false, art, pack, T(0), T(0));
    if (wc == 0 && lane == 0) t.empty_num[b] = (long)(p.T - min(L, T1) - (last_pos < L ? 1 : 0));
}

// The same batch written STRAIGHT INTO THE GROUPED ARENAS of a static group plan: the batch arrives sorted, place b
// belongs to the group g with bounds[g] <= b < bounds[g + 1] (a wave-uniform walk over at most HISTORY_GROUPS_MAX entries), history row
// j < H_g of place b is arena row hist_row_off[g] + (b - bounds[g]) * H_g + j and candidate slot s < T_g is arena row cand_row_off[g] +
// (b - bounds[g]) * T_g + s of x_target, x_global, the label arena and the row weights -- bit for bit what history_gather_groups and
// candidate_gather_groups (csrc/compact.hip) copy out of the dense tensors with the identity permutation, which are never formed.  t.x_history
// / t.x_target / t.x_global point at the arenas [R, hc] / [N, tc] / [N, 3]; label [B, T], label_id, empty_num, history_len, user_id and
// impression_id are the dense kernel's.  A block of rows at or beyond H_g exits at once.  An impression that does not fit its group -- H_g or
// more events where H_g < H, T_g or more live candidates where T_g < T -- raises *misfit; every table entry is clamped and an impression whose
// rows would not lie inside an arena writes none of them (and raises the flag): whatever the tables hold, nothing is written outside.
template <typename T, int VH, int VT>
__global__ __launch_bounds__(256) void assemble_groups_kernel(const AssembleGroupsParams q) {
    const AssembleParams& p = q.a;
    const nrm_assemble_tables& t = p.t;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nh = (p.H + ASM_ROWS - 1) / ASM_ROWS, nt = (p.T + ASM_ROWS - 1) / ASM_ROWS, per = nh + nt;
    const long item = (long)blockIdx.x * 4 + wave;
    if (item >= (long)p.B * per) return;
    const int b = (int)(item / per), w = (int)(item - (long)b * per);
    int g = 0;
    for (int k = 1; k < q.G; ++k)
        if (min(max(q.bounds[k], 0), p.B) <= b) g = k;
    const int bg = min(max(q.bounds[g], 0), b);
    const int hg = min(max(q.h_g[g], 1), p.H), tg = min(max(q.t_g[g], 1), p.T);
    if (w < nh && w * ASM_ROWS >= hg) return;                          // rows the group does not keep
    const long n = wave_impression(p, b, lane);
    const int u = (int)min(max((long)t.imp_user[n], 0L), t.U - 1);
    const long t_imp = t.imp_time_us[n];
    const int Sw = t.static_cols, S = t.S, amax = (int)t.A - 1;
    const __amdgpu_buffer_rsrc_t rs_static = buffer_rsrc(t.art_static, (unsigned)(t.A * S * (long)sizeof(T)));
    if (w < nh) {                                                      // up to 16 of the H_g history rows
        const int hc = 4 + Sw + 2;
        const long off = min(max(t.user_off[u], 0L), t.E);
        const int cnt = (int)min(min(max(t.user_off[u + 1], off), t.E) - off, (long)p.H);
        const int j0 = w * ASM_ROWS, nrows = min(ASM_ROWS, hg - j0), j = j0 + lane;
        const long row0 = (long)min(max(q.hist_row_off[g], 0), q.R) + (long)(b - bg) * hg;
        const bool inside = row0 + hg <= (long)q.R;
        int art = -1;
        unsigned pack = 0;
        T rd = T(0), sc = T(0);
        if (lane < nrows && j < cnt) {
            art = min(max(t.ev_art[off + j], 0), amax);
            pack = time_buckets(t_imp - t.ev_time_us[off + j]);
            rd = static_cast<const T*>(t.ev_read)[off + j];
            sc = static_cast<const T*>(t.ev_scroll)[off + j];
        }
        if (inside) {
            const __amdgpu_buffer_rsrc_t rs_out = buffer_rsrc(uniform_ptr(static_cast<T*>(t.x_history) + row0 * hc), (unsigned)((long)hg * hc * (long)sizeof(T)));
            write_rows<T, VH>(rs_out, rs_static, j0, nrows, hc, S, Sw, true, art, pack, rd, sc);
        }
        if (w == 0 && lane == 0) {
            t.history_len[b] = cnt;
            t.user_id_out[b] = t.user_id[u];
            t.impression_id[b] = t.imp_id[n];
            if (!inside || (hg < p.H && cnt >= hg)) *q.misfit = 1;
        }
        return;
    }
    // 16 candidate slots: the dense label / label_id of all of them, the arena rows of those below T_g
    const int tc = 4 + Sw, wc = w - nh, T1 = p.T - 1;
    const long loff = min(max(t.imp_off[n], 0L), t.L);
    const int L = (int)min(min(max(t.imp_off[n + 1], loff), t.L) - loff, (long)INT_MAX);
    const int* list = t.imp_inview + loff;
    const int target = t.imp_target[n];                                // -1: none
    const int last_pos = last_slot_pos(list, L, target, T1, p.keep_target_slot != 0, lane);
    const int s0 = wc * ASM_ROWS, nrows = min(ASM_ROWS, p.T - s0), s = s0 + lane;
    const long cell0 = (long)min(max(q.cand_row_off[g], 0), q.N) + (long)(b - bg) * tg;
    const bool inside = cell0 + tg <= (long)q.N;
    int art = -1;
    unsigned pack = 0;
    if (lane < nrows) {
        const int pos = s == T1 ? last_pos : s;
        const bool live = pos < L;
        double lab = 0.0;
        long id = -1;
        T gl[3] = {T(0), T(0), T(0)};
        if (live) {
            const int raw = list[pos];
            art = min(max(raw, 0), amax);
            pack = time_buckets(t_imp - t.art_pub_us[art]);
            lab = (target >= 0 && raw == target) ? 1.0 : 0.0;
            id = t.art_id[art];
#pragma unroll
            for (int k = 0; k < 3; ++k) gl[k] = static_cast<const T*>(t.art_global)[(long)art * 3 + k];
        }
        const long cell = (long)b * p.T + s;
        t.label[cell] = lab;
        t.label_id[cell] = id;
        if (inside && s < tg) {
            const long row = cell0 + s;
            q.label_arena[row] = lab;
            q.row_weight[row] = s == tg - 1 ? (float)(p.T - tg + 1) : 1.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) static_cast<T*>(t.x_global)[row * 3 + k] = gl[k];
        }
    }
    if (inside && s0 < tg) {
        const __amdgpu_buffer_rsrc_t rs_out = buffer_rsrc(uniform_ptr(static_cast<T*>(t.x_target) + cell0 * tc), (unsigned)((long)tg * tc * (long)sizeof(T)));
        write_rows<T, VT>(rs_out, rs_static, s0, min(ASM_ROWS, tg - s0), tc, S, Sw, false, art, pack, T(0), T(0));
    }
    if (wc == 0 && lane == 0) {
        const int empty = p.T - min(L, T1) - (last_pos < L ? 1 : 0);
        t.empty_num[b] = (long)empty;
        if (!inside || (tg < p.T && p.T - empty >= tg)) *q.misfit = 1;
    }
}

int assemble_form(int static_cols, int S) {
    if (static_cols < 1 || S < static_cols) return -1;
    return ((4 + static_cols + 2) % 4 == 0 && S % 4 == 0 && S >= static_cols + 2) ? 4 : 1;
}

// the grid (one wave per 16 rows of one impression, four to a block) and the form of either kernel; < 0: arguments no launch takes
static long assemble_grid(const AssembleParams& p, int& form) {
    if (p.n_order < 1) return -1;
    const long per = (p.H + ASM_ROWS - 1) / ASM_ROWS + (p.T + ASM_ROWS - 1) / ASM_ROWS;
    const long nblk = ((long)p.B * per + 3) / 4;
    form = assemble_form(p.t.static_cols, p.t.S);
    return (nblk > 0x7fffffffL || form < 0) ? -1 : nblk;
}

hipError_t assemble_launch(const AssembleParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    int form;
    const long nblk = assemble_grid(p, form);
    if (nblk < 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk), block(256);
    if (p.t.is_f64) {
        if (form == 4) hipLaunchKernelGGL((assemble_kernel<double, 4, 2>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((assemble_kernel<double, 1, 1>), grid, block, 0, st, p);
    } else {
        if (form == 4) hipLaunchKernelGGL((assemble_kernel<float, 4, 2>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((assemble_kernel<float, 1, 1>), grid, block, 0, st, p);
    }
    return hipGetLastError();
}

hipError_t assemble_groups_launch(const AssembleGroupsParams& q, hipStream_t st) {
    const AssembleParams& p = q.a;
    if (p.B <= 0) return hipSuccess;
    int form;
    const long nblk = assemble_grid(p, form);
    if (nblk < 0 || q.G < 1 || q.G > HISTORY_GROUPS_MAX || q.R < 1 || q.N < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk), block(256);
    if (p.t.is_f64) {
        if (form == 4) hipLaunchKernelGGL((assemble_groups_kernel<double, 4, 2>), grid, block, 0, st, q);
        else hipLaunchKernelGGL((assemble_groups_kernel<double, 1, 1>), grid, block, 0, st, q);
    } else {
        if (form == 4) hipLaunchKernelGGL((assemble_groups_kernel<float, 4, 2>), grid, block, 0, st, q);
        else hipLaunchKernelGGL((assemble_groups_kernel<float, 1, 1>), grid, block, 0, st, q);
    }
    return hipGetLastError();
}

}  // namespace nrm
