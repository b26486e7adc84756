// Launcher of csrc/assemble.hip: a step's batch written on the device from resident tables.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nrm_hotpath.h"

namespace nrm {

struct AssembleParams {
    nrm_assemble_tables t;
    const long* sel;                  // impression b is sel[cursor ? *cursor + b : b]; n_order entries
    const long* cursor;               // device, or null
    long n_order;
    int B, H, T, keep_target_slot;
};
// 4: rows in 16-byte units (hc % 4 == 0 and S a multiple of 4), 1: element by element.  The ONE place the form is chosen.
int assemble_form(int static_cols, int S);
hipError_t assemble_launch(const AssembleParams& p, hipStream_t st);

}  // namespace nrm
