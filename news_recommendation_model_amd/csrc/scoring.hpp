// Launcher of csrc/scoring.hip: the tail of the reference's test.py (ensemble softmax mean, second softmax over the de-padded
// slice, 1-based rank, ranking metrics) as one kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace nrm {

constexpr int ENSEMBLE_MAX_MODELS = 8;
constexpr int ENSEMBLE_MAX_CANDIDATES = 2048;      // one fp32 row per wave in LDS: 4 waves x 2048 x 4 B = 32 KiB per workgroup

// the models' logit matrices, passed BY VALUE as a kernel argument: nothing is stacked or copied on the device first
struct EnsembleLogits {
    const float* ptr[ENSEMBLE_MAX_MODELS];
    long row_stride[ENSEMBLE_MAX_MODELS];          // in floats
    long col_stride[ENSEMBLE_MAX_MODELS];          // in floats (1 = dense rows; 4 = column 0 of a padded [B*T, 4] GEMM output)
};

hipError_t ensemble_rank_launch(const EnsembleLogits& logits, int M, const int* empty, const float* label, int B, int T,
                                float* score, int* rank, int* live, float* metrics, hipStream_t st);

// ragged form (compact scoring): model m's compact logits at logits.ptr[m] + c * col_stride[m] (row_stride is not read), impression b owns the
// entries cand_off[b] .. cand_off[b + 1] - 1, the last of them standing for pad_mult[b] padded columns where pad_mult[b] > 0
hipError_t ensemble_rank_ragged_launch(const EnsembleLogits& logits, int M, const int* cand_off, const int* pad_mult, int N,
                                       const float* label, int B, int T, float* score, int* rank, int* live, float* metrics, hipStream_t st);

}  // namespace nrm
