// Launcher of csrc/compact.hip: the gather + padding check at the head of the compact scoring path.
#pragma once
#include <hip/hip_runtime.h>

namespace nrm {

struct CompactGatherParams {
    const unsigned* xt; const unsigned* xg;     // [B*T, wt] / [B*T, wg] as 32-bit words (a float64 column is two words)
    unsigned* xt_c; unsigned* xg_c;             // [N, wt] / [N, wg]
    int wt, wg;
    const int* cand_off;                        // [B + 1]
    const int* pad_mult;                        // [B]
    int B, T, Tp, N;                            // Tp = T - common trim: the columns the reference keeps
    int* flag;                                  // set to 1 on a padded row that differs from its representative (or a plan that does not add up)
};
hipError_t compact_gather_launch(const CompactGatherParams& p, hipStream_t st);

}  // namespace nrm
