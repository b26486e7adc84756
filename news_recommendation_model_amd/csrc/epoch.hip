// The record of a table-fed epoch kept on the device: what the epoch loops of trainer.py do after every step with
// about eight small ATen launches -- reference train.py:77-94: total_loss += loss.item() * B, the running AUC, the per-step loss list -- as
// ONE launch of one workgroup that also moves the cursor the next step's assemble kernel reads.  Being on the stream and free of host
// data it is part of the captured step: a replayed graph knows which batch it is on because the step before it said so here.
//
// Sums are float64 in a fixed order -- a thread's rows b = tid, tid + 256, ... in that order, a fixed shuffle tree over the wave, the four
// wave partials in wave order -- and without atomics, so an epoch's record is the same bit for bit from run to run.  sums[0] takes ONE
// rounded product and ONE rounded sum per step (contraction is off in this file: an fma would round once and the host could not restate
// it).  Every store is a plain store of thread 0.
#include "epoch.hpp"

#pragma clang fp contract(off)

namespace nrm {

constexpr int TALLY_THREADS = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;                                                         // lane 0 holds the sum
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}

__global__ __launch_bounds__(TALLY_THREADS) void epoch_tally_kernel(const float* __restrict__ loss, const float* __restrict__ auc,
                                                                    const int* __restrict__ top1, int B, long* cursor, double* sums,
                                                                    long* counts, float* step_log, long log_cap) {
    __shared__ double s_auc[TALLY_THREADS / 64];
    __shared__ int s_bad[TALLY_THREADS / 64], s_hit[TALLY_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a = 0.0;
    int bad = 0, hit = 0;
    for (int b = tid; b < B; b += TALLY_THREADS) {
        const float v = auc[b];
        if (v >= 0.0f) a += (double)v;
        else ++bad;                                                   // one class in the row (a NaN would count here too)
        hit += top1[b];
    }
    a = wave_sum(a);
    bad = wave_sum(bad);
    hit = wave_sum(hit);
    if (lane == 0) { s_auc[wave] = a; s_bad[wave] = bad; s_hit[wave] = hit; }
    __syncthreads();
    if (tid != 0) return;
    double auc_sum = 0.0;
    long n_bad = 0, n_hit = 0;
    for (int w = 0; w < TALLY_THREADS / 64; ++w) { auc_sum += s_auc[w]; n_bad += s_bad[w]; n_hit += s_hit[w]; }
    const float l = *loss;
    const double prod = (double)l * (double)B;
    sums[0] = sums[0] + prod;
    sums[1] = sums[1] + auc_sum;
    sums[2] = sums[2] + (double)n_hit;
    counts[0] += n_bad;
    const long k = counts[1];
    if (k >= 0 && k < log_cap) {
        const long n_ok = (long)B - n_bad;
        step_log[2 * k] = l;
        step_log[2 * k + 1] = n_ok > 0 ? (float)(auc_sum / (double)n_ok) : 0.0f;
    }
    counts[1] = k + 1;
    *cursor += (long)B;
}

hipError_t epoch_tally_launch(const float* loss, const float* auc, const int* top1, int B, long* cursor, double* sums, long* counts,
                              float* step_log, long log_cap, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(epoch_tally_kernel, dim3(1), dim3(TALLY_THREADS), 0, st, loss, auc, top1, B, cursor, sums, counts, step_log, log_cap);
    return hipGetLastError();
}

}  // namespace nrm
