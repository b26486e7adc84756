// Launcher of csrc/epoch.hip: the records of a table-fed epoch and of a table-fed evaluation pass (5h) kept on the device.
#pragma once
#include <hip/hip_runtime.h>

namespace nrm {

hipError_t epoch_tally_launch(const float* loss, const float* auc, const int* top1, int B, long* cursor, double* sums, long* counts,
                              float* step_log, long log_cap, hipStream_t st);
hipError_t eval_tally_launch(const float* auc, const int* top1, const float* metrics, const int* rank, const int* live,
                             const long* impression_id, int B, int T, int Tp, long* cursor, long n_order, double* sums, long* counts,
                             int* rec_rank, int* rec_live, long* rec_id, long cap, hipStream_t st);

}  // namespace nrm
