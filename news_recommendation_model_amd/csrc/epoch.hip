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

// The evaluation sibling: the record of a validation or scoring pass.  One launch of one workgroup at the end of an
// evaluation step -- reference verify.py:25-43 (the running AUC / top-1 sums of model_validation) and test.py:118-130 (the ranks a
// submission line is written from) -- that adds the step's row metrics to five float64 sums in the fixed order above, copies the step's
// ranks, live counts and impression ids into a ring of `cap` rows (row p % cap for position p = *cursor + b of the pass, columns Tp .. T - 1
// written as 0) and moves the cursor.  A row whose position lies outside [0, n_order) is neither written nor summed: a replay past the end
// of a pass changes nothing but the step count and the cursor.  Every thread reads the cursor before the barrier and thread 0 stores it
// after, so no row sees the moved value.
__global__ __launch_bounds__(TALLY_THREADS) void eval_tally_kernel(const float* __restrict__ auc, const int* __restrict__ top1,
                                                                   const float* __restrict__ metrics, const int* __restrict__ rank,
                                                                   const int* __restrict__ live, const long* __restrict__ impression_id, int B,
                                                                   int T, int Tp, long* cursor, long n_order, double* sums, long* counts,
                                                                   int* rec_rank, int* rec_live, long* rec_id, long cap) {
    constexpr int NW = TALLY_THREADS / 64;
    __shared__ double s_sum[4][NW];
    __shared__ int s_cnt[4][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long c = *cursor;
    double a = 0.0, rr = 0.0, n5 = 0.0, n10 = 0.0;
    int hit = 0, bad_auc = 0, bad_met = 0, rows = 0;
    for (int b = tid; b < B; b += TALLY_THREADS) {
        const long p = c + (long)b;
        if (p < 0 || p >= n_order) continue;
        ++rows;
        if (auc) {
            const float v = auc[b];
            if (v >= 0.0f) a += (double)v;
            else ++bad_auc;                                           // one class in the row (a NaN would count here too)
            hit += top1[b];
        }
        if (metrics) {
            const float m0 = metrics[3 * b];
            if (m0 >= 0.0f) { rr += (double)m0; n5 += (double)metrics[3 * b + 1]; n10 += (double)metrics[3 * b + 2]; }
            else ++bad_met;                                           // no live positive in the row
        }
        if (cap > 0) {
            const long r = p % cap;
            rec_live[r] = live[b];
            rec_id[r] = impression_id[b];
        }
    }
    if (cap > 0) {
        const long cells = (long)B * (long)T;
        for (long i = tid; i < cells; i += TALLY_THREADS) {
            const int b = (int)(i / T), j = (int)(i - (long)b * T);
            const long p = c + (long)b;
            if (p < 0 || p >= n_order) continue;
            rec_rank[(p % cap) * (long)T + j] = j < Tp ? rank[(long)b * Tp + j] : 0;
        }
    }
    a = wave_sum(a); rr = wave_sum(rr); n5 = wave_sum(n5); n10 = wave_sum(n10);
    hit = wave_sum(hit); bad_auc = wave_sum(bad_auc); bad_met = wave_sum(bad_met); rows = wave_sum(rows);
    if (lane == 0) {
        s_sum[0][wave] = a; s_sum[1][wave] = rr; s_sum[2][wave] = n5; s_sum[3][wave] = n10;
        s_cnt[0][wave] = hit; s_cnt[1][wave] = bad_auc; s_cnt[2][wave] = bad_met; s_cnt[3][wave] = rows;
    }
    __syncthreads();
    if (tid != 0) return;
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    long k[4] = {0, 0, 0, 0};
    for (int w = 0; w < NW; ++w)
        for (int i = 0; i < 4; ++i) { d[i] += s_sum[i][w]; k[i] += s_cnt[i][w]; }
    sums[0] = sums[0] + d[0];
    sums[1] = sums[1] + (double)k[0];
    sums[2] = sums[2] + d[1];
    sums[3] = sums[3] + d[2];
    sums[4] = sums[4] + d[3];
    counts[0] += k[1];
    counts[1] += k[2];
    counts[2] += 1;
    counts[3] += k[3];
    *cursor = c + (long)B;
}

hipError_t eval_tally_launch(const float* auc, const int* top1, const float* metrics, const int* rank, const int* live,
                             const long* impression_id, int B, int T, int Tp, long* cursor, long n_order, double* sums, long* counts,
                             int* rec_rank, int* rec_live, long* rec_id, long cap, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(eval_tally_kernel, dim3(1), dim3(TALLY_THREADS), 0, st, auc, top1, metrics, rank, live, impression_id, B, T, Tp, cursor,
                       n_order, sums, counts, rec_rank, rec_live, rec_id, cap);
    return hipGetLastError();
}

}  // namespace nrm
