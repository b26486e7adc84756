// Launcher of csrc/epoch.hip: the record of a table-fed epoch kept on the device.
#pragma once
#include <hip/hip_runtime.h>

namespace nrm {

hipError_t epoch_tally_launch(const float* loss, const float* auc, const int* top1, int B, long* cursor, double* sums, long* counts,
                              float* step_log, long log_cap, hipStream_t st);

}  // namespace nrm
