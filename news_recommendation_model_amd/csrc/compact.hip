// Head of the compact scoring path (inference): candidate lists are padded with all-zero rows to the longest list of the data set,
// and every padded candidate of one impression has the same input rows, hence the same logit.  The compact path therefore scores
// each impression's n live candidates and ONE representative padded candidate (column n) and lets the scoring tail count it e' times.
// This kernel copies those rows of x_target and x_global into compact [N, cols] arrays (bitwise, float64 or float32 as they come)
// and CHECKS what the identity rests on: every other padded column a row keeps after the common trim must be bitwise equal to the
// representative.  A difference -- or tables that do not add up to Tp columns -- raises a flag in host-visible memory, like the
// front end's index flag: written only in the error case, read by the host whenever it likes, no synchronisation on the hot path.
// The trimmed columns are never read, as the reference never reads them.
// One wave per (impression, kept column); rows are independent: a wave reads its own cell and its row's representative only.
#include <cstdint>
#include "compact.hpp"

namespace nrm {

__global__ __launch_bounds__(256) void compact_gather_kernel(const CompactGatherParams p) {
    const int lane = threadIdx.x & 63;
    const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= (long)p.B * p.Tp) return;
    const int b = (int)(cell / p.Tp), t = (int)(cell - (long)b * p.Tp);
    const int c0 = min(max(p.cand_off[b], 0), p.N);
    const int cnt = min(min(max(p.cand_off[b + 1], c0), p.N) - c0, p.Tp);
    const int e = max(p.pad_mult[b], 0);
    const int n = e > 0 ? max(cnt - 1, 0) : cnt;                       // live candidates; column n is the representative where e > 0
    if (t == 0 && lane == 0 && (n + e != p.Tp || (e > 0 && cnt < 1))) *p.flag = 1;
    const long src = (long)b * p.T + t;
    if (t < cnt) {                                                     // a live candidate or the representative: copy
        const long dst = (long)c0 + t;
        for (int w = lane; w < p.wt; w += 64) p.xt_c[dst * p.wt + w] = p.xt[src * p.wt + w];
        for (int w = lane; w < p.wg; w += 64) p.xg_c[dst * p.wg + w] = p.xg[src * p.wg + w];
    } else if (e > 0 && cnt >= 1) {                                    // another padded column of this row: must equal the representative
        const long rep = (long)b * p.T + n;
        bool differs = false;
        for (int w = lane; w < p.wt; w += 64) differs |= p.xt[src * p.wt + w] != p.xt[rep * p.wt + w];
        for (int w = lane; w < p.wg; w += 64) differs |= p.xg[src * p.wg + w] != p.xg[rep * p.wg + w];
        if (differs) *p.flag = 1;
    }
}

hipError_t compact_gather_launch(const CompactGatherParams& p, hipStream_t st) {
    const long cells = (long)p.B * p.Tp;
    if (cells <= 0) return hipSuccess;
    if ((cells + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, st, p);
    return hipGetLastError();
}

// ---- history compaction (section 5d)
// History length: ONE pass over x_history as a flat array of 32-bit words.  A thread reads 16-byte vectors 256 apart (a wave reads 1 KiB of
// consecutive words: neighbouring rows of an impression side by side), keeps (impression, 1 + last live row) of what it saw and hands it
// over with a vector atomic max -- one per wave where the whole wave saw one impression, one per lane otherwise.  The test is on the BITS:
// -0.0 and NaN count as live.  hist_len is cleared by the launcher.
constexpr int HL_VECS = 8;                  // 16-byte vectors per thread
__global__ __launch_bounds__(256) void history_len_kernel(const unsigned* __restrict__ x, long nvec, long nwords, int H, int words, int B,
                                                          int* __restrict__ hist_len) {
    int cur_b = -1, cur_l = 0;
    auto flush = [&]() { if (cur_b >= 0 && cur_b < B && cur_l > 0) atomicMax(hist_len + cur_b, cur_l); };
    auto note = [&](int b, int j) {
        if (b != cur_b) { flush(); cur_b = b; cur_l = 0; }
        cur_l = max(cur_l, j + 1);
    };
    const long rowlen = (long)H * words;
    const long v0 = (long)blockIdx.x * (256 * HL_VECS) + threadIdx.x;
    for (int i = 0; i < HL_VECS; ++i) {
        const long v = v0 + (long)i * 256;
        if (v >= nvec) break;
        const uint4 w4 = reinterpret_cast<const uint4*>(x)[v];
        if ((w4.x | w4.y | w4.z | w4.w) == 0u) continue;
        const long g = v * 4;
        int b = (int)(g / rowlen);
        const int rem = (int)(g - (long)b * rowlen);      // H * words < 2^31 (checked by the entry point)
        int j = rem / words, c = rem - j * words;
        const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (w[k]) note(b, j);
            if (++c == words) { c = 0; if (++j == H) { j = 0; ++b; } }
        }
    }
    // the words past the last whole vector (fewer than four): thread 0 of block 0
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long g = nvec * 4; g < nwords; ++g)
            if (x[g]) { const int b = (int)(g / rowlen); note(b, (int)((g - (long)b * rowlen) / words)); }
    const int b0 = __shfl(cur_b, 0);
    if (__all(cur_b == b0 || cur_b < 0)) {                 // one impression in the whole wave: reduce, one atomic
        int l = cur_b < 0 ? 0 : cur_l;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) l = max(l, __shfl_xor(l, o));
        int bb = cur_b;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bb = max(bb, __shfl_xor(bb, o));
        if ((threadIdx.x & 63) == 0 && bb >= 0 && bb < B && l > 0) atomicMax(hist_len + bb, l);
    } else {
        flush();
    }
}

hipError_t history_len_launch(const unsigned* x, int B, int H, int words, int* hist_len, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(hist_len, 0, (size_t)B * sizeof(int), st)) return e;
    const long nwords = (long)B * H * words;
    if (nwords <= 0) return hipSuccess;
    const long nvec = ((uintptr_t)x & 15) ? 0 : nwords / 4;          // an unaligned view: word by word (never the DataLoader's tensors)
    if (nvec == 0) {
        hipLaunchKernelGGL(history_len_kernel, dim3(1), dim3(256), 0, st, x, 0L, nwords, H, words, B, hist_len);
        return hipGetLastError();
    }
    const long nblk = (nvec + 256 * HL_VECS - 1) / (256 * HL_VECS);
    if (nblk > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(history_len_kernel, dim3((unsigned)nblk), dim3(256), 0, st, x, nvec, nwords, H, words, B, hist_len);
    return hipGetLastError();
}

// One wave per (impression, kept row): row j < K_b of impression b goes to compact row hist_off[b] + j, as compact_gather_kernel places a
// candidate.  Table entries are clamped to the arrays.
__global__ __launch_bounds__(256) void history_gather_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ xh_c, int words,
                                                             const int* __restrict__ hist_off, int B, int H, int R, int k_max) {
    const int lane = threadIdx.x & 63;
    const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= (long)B * k_max) return;
    const int b = (int)(cell / k_max), j = (int)(cell - (long)b * k_max);
    const int r0 = min(max(hist_off[b], 0), R);
    const int K = min(min(max(hist_off[b + 1], r0), R) - r0, H);
    if (j >= K) return;
    const long src = ((long)b * H + j) * words, dst = ((long)r0 + j) * words;
    for (int w = lane; w < words; w += 64) xh_c[dst + w] = x[src + w];
}

hipError_t history_gather_launch(const unsigned* x, unsigned* xh_c, int words, const int* hist_off, int B, int H, int R, int k_max, hipStream_t st) {
    const long cells = (long)B * k_max;
    if (cells <= 0 || R <= 0) return hipSuccess;
    if ((cells + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(history_gather_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, st, x, xh_c, words, hist_off, B, H, R, k_max);
    return hipGetLastError();
}

// Grouped arena (section 5e).  One wave per kept row r < R: its group is the last g with row_off[g] <= r (G is a handful: a walk), then
// r - row_off[g] = (b - b0[g]) * hg[g] + j.  Every table entry is clamped: a table that does not add up copies a wrong row or none,
// never reads or writes outside x [B, H, words] and xh_g [R, words].
__global__ __launch_bounds__(256) void history_gather_groups_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ xh_g, int words,
                                                                    const int* __restrict__ src_imp, const int* __restrict__ b0,
                                                                    const int* __restrict__ row_off, const int* __restrict__ hg,
                                                                    int G, int B, int H, int R) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    int g = 0;
    for (int k = 1; k < G; ++k)
        if ((long)min(max(row_off[k], 0), R) <= row) g = k;
    const int r0 = min(max(row_off[g], 0), R);
    const int hgg = min(max(hg[g], 1), H);
    const int local = (int)(row - r0);
    const int bs = min(max(b0[g], 0), B - 1) + local / hgg, j = local - (local / hgg) * hgg;      // j < hgg <= H
    if (bs >= B) return;
    const int b = min(max(src_imp[bs], 0), B - 1);
    const long src = ((long)b * H + j) * words, dst = row * words;
    for (int w = lane; w < words; w += 64) xh_g[dst + w] = x[src + w];
}

hipError_t history_gather_groups_launch(const unsigned* x, unsigned* xh_g, int words, const int* src_imp, const int* b0, const int* row_off,
                                        const int* hg, int G, int B, int H, int R, hipStream_t st) {
    if (R <= 0 || B <= 0 || G <= 0 || H <= 0) return hipSuccess;
    hipLaunchKernelGGL(history_gather_groups_kernel, dim3((unsigned)(((long)R + 3) / 4)), dim3(256), 0, st, x, xh_g, words, src_imp, b0, row_off, hg,
                       G, B, H, R);
    return hipGetLastError();
}

// Candidate arena of the compacted training step (section 5f).  One wave per cell (sorted impression bs, column t) of the B * T cells: its
// group is the last g with b0[g] <= bs (a walk, as above), T_g = tg[g] the columns the group keeps.  A kept cell (t < T_g) is copied to arena
// row row_off[g] + (bs - b0[g]) * T_g + t of all three tensors and gets its row weight: T - T_g + 1 on the group's last column, 1 elsewhere.
// A dropped cell (t >= T_g) must be bitwise equal to column T_g - 1 of its impression in all three tensors: the host's empty_num is checked,
// not trusted.  Every table entry is clamped and a row outside the arena is not written (and raises the flag): tables that do not add up
// copy a wrong row or none, never read outside the [B, T] inputs or write outside the [N] arenas.
__global__ __launch_bounds__(256) void candidate_gather_groups_kernel(const CandidateGatherParams p) {
    const int lane = threadIdx.x & 63;
    const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= (long)p.B * p.T) return;
    const int bs = (int)(cell / p.T), t = (int)(cell - (long)bs * p.T);
    int g = 0;
    for (int k = 1; k < p.G; ++k)
        if (min(max(p.b0[k], 0), p.B) <= bs) g = k;
    const int bg = min(max(p.b0[g], 0), bs);
    const int tg = min(max(p.tg[g], 1), p.T);
    const int b = min(max(p.src_imp[bs], 0), p.B - 1);
    const long src = (long)b * p.T + t;
    if (t < tg) {
        const long dst = (long)min(max(p.row_off[g], 0), p.N) + (long)(bs - bg) * tg + t;
        if (dst >= p.N) { if (lane == 0) *p.flag = 1; return; }
        for (int w = lane; w < p.wt; w += 64) p.xt_a[dst * p.wt + w] = p.xt[src * p.wt + w];
        for (int w = lane; w < p.wg; w += 64) p.xg_a[dst * p.wg + w] = p.xg[src * p.wg + w];
        for (int w = lane; w < p.wl; w += 64) p.lab_a[dst * p.wl + w] = p.lab[src * p.wl + w];
        if (lane == 0) p.roww[dst] = t == tg - 1 ? (float)(p.T - tg + 1) : 1.f;
    } else {
        const long rep = (long)b * p.T + (tg - 1);
        bool differs = false;
        for (int w = lane; w < p.wt; w += 64) differs |= p.xt[src * p.wt + w] != p.xt[rep * p.wt + w];
        for (int w = lane; w < p.wg; w += 64) differs |= p.xg[src * p.wg + w] != p.xg[rep * p.wg + w];
        for (int w = lane; w < p.wl; w += 64) differs |= p.lab[src * p.wl + w] != p.lab[rep * p.wl + w];
        if (differs) *p.flag = 1;
    }
}

hipError_t candidate_gather_groups_launch(const CandidateGatherParams& p, hipStream_t st) {
    const long cells = (long)p.B * p.T;
    if (cells <= 0 || p.G <= 0) return hipSuccess;
    if ((cells + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(candidate_gather_groups_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, st, p);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void history_tiles_kernel(const int* __restrict__ cand_imp, const int* __restrict__ cand_off,
                                                            const int* __restrict__ hist_off, const int* __restrict__ tile_pre, int B, int N,
                                                            int R, int Mt, int4* __restrict__ tile_tab) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const int b = min(max(cand_imp[c], 0), B - 1);
    const int r0 = min(max(hist_off[b], 0), R);
    const int K = min(max(hist_off[b + 1], r0), R) - r0;
    const int nt = (K + 15) >> 4;
    const long first = (long)tile_pre[b] + (long)(c - cand_off[b]) * nt;
    for (int jt = 0; jt < nt; ++jt) {
        const long tile = first + jt;
        if (tile >= 0 && tile < Mt) tile_tab[tile] = make_int4(c, r0 + 16 * jt, min(16, K - 16 * jt), b);
    }
}

hipError_t history_tiles_launch(const int* cand_imp, const int* cand_off, const int* hist_off, const int* tile_pre, int B, int N, int R, int Mt,
                                int4* tile_tab, hipStream_t st) {
    if (N <= 0 || B <= 0 || Mt <= 0) return hipSuccess;
    // a table that does not add up leaves tiles unwritten: {0, 0, 0, 0} = no valid row
    if (hipError_t e = hipMemsetAsync(tile_tab, 0, (size_t)Mt * sizeof(int4), st)) return e;
    hipLaunchKernelGGL(history_tiles_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, cand_imp, cand_off, hist_off, tile_pre, B, N, R, Mt, tile_tab);
    return hipGetLastError();
}

}  // namespace nrm
