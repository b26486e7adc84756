// Head of the compact scoring path (inference): candidate lists are padded with all-zero rows to the longest list of the data set,
// and every padded candidate of one impression has the same input rows, hence the same logit.  The compact path therefore scores
// each impression's n live candidates and ONE representative padded candidate (column n) and lets the scoring tail count it e' times.
// This kernel copies those rows of x_target and x_global into compact [N, cols] arrays (bitwise, float64 or float32 as they come)
// and CHECKS what the identity rests on: every other padded column a row keeps after the common trim must be bitwise equal to the
// representative.  A difference -- or tables that do not add up to Tp columns -- raises a flag in host-visible memory, like the
// front end's index flag: written only in the error case, read by the host whenever it likes, no synchronisation on the hot path.
// The trimmed columns are never read, as the reference never reads them.
// One wave per (impression, kept column); rows are independent: a wave reads its own cell and its row's representative only.
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

}  // namespace nrm
