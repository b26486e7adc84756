// Scoring tail of the reference's test.py as ONE kernel (test.py:58-70 model_test, :118-126 get_string_of_prediction):
//   p_m   = softmax over ALL T columns of model m's logits (the first softmax sees the padding columns, as in the reference)
//   out   = (p_0 + ... + p_{M-1}) / M                                  summed in model order
//   score = softmax(out[0:n]) where the row still carries padding (n < T), out otherwise          (test.py:68 / :70)
//   rank  = 1 + #{i < n: score[i] > score[j]} + #{i < j: score[i] == score[j]}                    (stable descending sort)
// and, with labels, the reciprocal rank and nDCG@5 / @10 of the row.  One wave per impression, four waves per workgroup,
// lane = candidate (strided for T > 64), like row_auc_kernel.  The row of out / score lives in a register per lane when
// T <= 64 and in the wave's slice of LDS above; every lane computes its own elements from the wave-wide max and sum, so two
// columns with identical logits in every model get bitwise identical scores (the tie-break is then by index).
// Rows are independent: a wave reads and writes its own row only, every loop is bounded by T.
#include "scoring.hpp"
#include "common.hpp"

namespace nrm {

__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ double wave_sum64d(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// REG: T <= 64, the lane's one element stays in a register and the rank loop reads the others with v_readlane.
// RAGGED (compact scoring path): model m's logits are ONE compact vector; impression b owns its entries cand_off[b] .. cand_off[b + 1] - 1:
// the n live candidates and, where pad_mult[b] = e' > 0 padded columns are kept, one representative padded candidate behind them.
// All e' padded columns of a row have the same logit (same all-zero input rows, same history), so
//   p_j = exp(l_j - mx) / (sum_{i < n} exp(l_i - mx) + e' exp(l_pad - mx)),   mx = max over the live and the pad logit
// is the first softmax over all T = n + e' columns; everything after it (mean, second softmax where e' > 0, rank, metrics) and the dense
// [B, T] outputs are those of the dense form.  Offsets and counts are clamped to the arrays.
template <bool REG, bool RAGGED = false>
__global__ __launch_bounds__(256) void ensemble_rank_kernel(const EnsembleLogits lg, int M, const int* __restrict__ empty,
                                                            const float* __restrict__ label, int B, int T,
                                                            float* __restrict__ score, int* __restrict__ rank,
                                                            int* __restrict__ live, float* __restrict__ metrics,
                                                            const int* __restrict__ cand_off, const int* __restrict__ pad_mult, int N) {
    extern __shared__ __attribute__((aligned(16))) float rows[];       // [4][T] when !REG
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;                                                // (no workgroup barrier below: waves are independent)
    int e = 0, c0 = 0, cnt = 0;                                        // RAGGED: padded columns kept, first compact entry, entries
    if (RAGGED) {
        c0 = min(max(cand_off[b], 0), N);
        cnt = min(min(max(cand_off[b + 1], c0), N) - c0, T);
        e = max(pad_mult[b], 0);
    } else {
        e = empty ? empty[b] : 0;
    }
    const bool has_pad = RAGGED ? e > 0 : false;
    const int n = RAGGED ? (has_pad ? max(cnt - 1, 0) : cnt)
                         : (e <= 0 ? T : (e >= T ? 0 : T - e));        // live candidates, always within [0, T]
#define NRM_AGAIN (RAGGED ? has_pad : n < T)                           /* the row keeps padding: second softmax over the live slice */
    float* row = rows + (REG ? 0 : wave * T);
    float* s_out = score + (long)b * T;
    int* r_out = rank + (long)b * T;
    const float NEG_INF = -__builtin_huge_valf();
    const float models = (float)M;

    // ---- mean over the models of softmax over all T columns
    float acc = 0.f;                                                   // REG: the lane's element of the sum
    for (int m = 0; m < M; ++m) {
        const long cs = lg.col_stride[m];
        const float* x = RAGGED ? lg.ptr[m] + (long)c0 * cs : lg.ptr[m] + (long)b * lg.row_stride[m];
        if (RAGGED) {
            const float mult = (float)e;                               // weight of the representative padded entry (index n)
            if (REG) {
                const float xj = lane < cnt ? x[lane * cs] : NEG_INF;
                const float mx = wave_max64(xj);
                const float ex = lane < cnt ? expf(xj - mx) : 0.f;
                const float sum = wave_sum64(lane == n ? ex * mult : ex);          // (lane == n < cnt only where has_pad)
                acc += lane < n ? ex / sum : 0.f;
            } else {
                float mx = NEG_INF;
                for (int j = lane; j < cnt; j += 64) mx = fmaxf(mx, x[j * cs]);
                mx = wave_max64(mx);
                float sum = 0.f;
                for (int j = lane; j < cnt; j += 64) {
                    const float ex = expf(x[j * cs] - mx);
                    sum += j == n ? ex * mult : ex;
                }
                sum = wave_sum64(sum);
                for (int j = lane; j < T; j += 64) {
                    const float pj = j < n ? expf(x[j * cs] - mx) / sum : 0.f;
                    row[j] = m ? row[j] + pj : pj;
                }
            }
        } else if (REG) {
            const float xj = lane < T ? x[lane * cs] : NEG_INF;
            const float mx = wave_max64(xj);
            const float ex = lane < T ? expf(xj - mx) : 0.f;
            const float sum = wave_sum64(ex);
            acc += ex / sum;
        } else {
            float mx = NEG_INF;
            for (int j = lane; j < T; j += 64) mx = fmaxf(mx, x[j * cs]);
            mx = wave_max64(mx);
            float sum = 0.f;
            for (int j = lane; j < T; j += 64) sum += expf(x[j * cs] - mx);
            sum = wave_sum64(sum);
            for (int j = lane; j < T; j += 64) {                       // (a lane touches its own columns of the LDS row only)
                const float p = expf(x[j * cs] - mx) / sum;
                row[j] = m ? row[j] + p : p;
            }
        }
    }

    // ---- second softmax over the de-padded slice, scores out (0 on padding columns)
    float sc = 0.f;                                                    // REG: the lane's score
    if (REG) {
        const float o = acc / models;
        if (NRM_AGAIN) {
            const float mx = wave_max64(lane < n ? o : NEG_INF);
            const float ex = lane < n ? expf(o - mx) : 0.f;
            const float sum = wave_sum64(ex);
            sc = lane < n ? ex / sum : 0.f;
        } else {
            sc = o;
        }
        if (lane < T) s_out[lane] = sc;
    } else {
        if (NRM_AGAIN) {
            float mx = NEG_INF;
            for (int j = lane; j < n; j += 64) {
                const float o = row[j] / models;
                row[j] = o;
                mx = fmaxf(mx, o);
            }
            mx = wave_max64(mx);
            float sum = 0.f;
            for (int j = lane; j < n; j += 64) sum += expf(row[j] - mx);
            sum = wave_sum64(sum);
            for (int j = lane; j < T; j += 64) {
                const float v = j < n ? expf(row[j] - mx) / sum : 0.f;
                row[j] = v;
                s_out[j] = v;
            }
        } else {
            for (int j = lane; j < T; j += 64) {
                const float v = row[j] / models;
                row[j] = v;
                s_out[j] = v;
            }
        }
        // the rank loop reads the other lanes' columns: the wave's LDS writes above must have landed (one wave, program order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    // ---- rank (O(n^2 / 64) compares per wave) and the metrics' sums
    const bool want = label != nullptr;
    const float* y = want ? label + (long)b * T : nullptr;
    double rr = 0.0, d5 = 0.0, d10 = 0.0, npos = 0.0;
    auto tally = [&](int j, int r) {
        if (want && y[j] > 0.5f) {
            npos += 1.0;
            rr += 1.0 / (double)r;
            if (r <= 10) {
                const double g = 1.0 / log2((double)(1 + r));
                d10 += g;
                if (r <= 5) d5 += g;
            }
        }
    };
    if (REG) {
        int r = 1;
        for (int i = 0; i < n; ++i) {
            const float si = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc), i));
            r += (si > sc || (si == sc && i < lane)) ? 1 : 0;
        }
        if (lane < T) r_out[lane] = lane < n ? r : 0;
        if (lane < n) tally(lane, r);
    } else {
        for (int j = lane; j < T; j += 64) {
            int r = 0;
            if (j < n) {
                const float sj = row[j];
                r = 1;
                for (int i = 0; i < n; ++i) {
                    const float si = row[i];                           // same address in every lane: an LDS broadcast
                    r += (si > sj || (si == sj && i < j)) ? 1 : 0;
                }
                tally(j, r);
            }
            r_out[j] = r;
        }
    }
    if (lane == 0) live[b] = n;
    if (want) {
        npos = wave_sum64d(npos); rr = wave_sum64d(rr); d5 = wave_sum64d(d5); d10 = wave_sum64d(d10);
        if (lane == 0) {
            float* mo = metrics + (long)b * 3;
            if (npos > 0.0) {
                double i5 = 0.0, i10 = 0.0;                            // ideal DCG: the positives on ranks 1 .. min(k, n_pos)
                for (int r = 1; r <= 10 && (double)r <= npos; ++r) {
                    const double g = 1.0 / log2((double)(1 + r));
                    i10 += g;
                    if (r <= 5) i5 += g;
                }
                mo[0] = (float)(rr / npos); mo[1] = (float)(d5 / i5); mo[2] = (float)(d10 / i10);
            } else {
                mo[0] = -1.f; mo[1] = -1.f; mo[2] = -1.f;
            }
        }
    }
}

#undef NRM_AGAIN

hipError_t ensemble_rank_launch(const EnsembleLogits& logits, int M, const int* empty, const float* label, int B, int T,
                                float* score, int* rank, int* live, float* metrics, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    const dim3 grid((B + 3) / 4), block(256);
    if (T <= 64)
        hipLaunchKernelGGL(ensemble_rank_kernel<true>, grid, block, 0, st, logits, M, empty, label, B, T, score, rank, live, metrics,
                           nullptr, nullptr, 0);
    else
        hipLaunchKernelGGL(ensemble_rank_kernel<false>, grid, block, 4 * (size_t)T * sizeof(float), st, logits, M, empty, label, B, T,
                           score, rank, live, metrics, nullptr, nullptr, 0);
    return hipGetLastError();
}

hipError_t ensemble_rank_ragged_launch(const EnsembleLogits& logits, int M, const int* cand_off, const int* pad_mult, int N,
                                       const float* label, int B, int T, float* score, int* rank, int* live, float* metrics, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    const dim3 grid((B + 3) / 4), block(256);
    if (T <= 64)
        hipLaunchKernelGGL((ensemble_rank_kernel<true, true>), grid, block, 0, st, logits, M, nullptr, label, B, T, score, rank, live, metrics,
                           cand_off, pad_mult, N);
    else
        hipLaunchKernelGGL((ensemble_rank_kernel<false, true>), grid, block, 4 * (size_t)T * sizeof(float), st, logits, M, nullptr, label, B, T,
                           score, rank, live, metrics, cand_off, pad_mult, N);
    return hipGetLastError();
}

}  // namespace nrm
