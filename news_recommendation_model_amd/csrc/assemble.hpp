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

// The batch written straight into the grouped arenas of a static group plan.  ``a.t.x_history`` / ``x_target`` /
// ``x_global`` are the ARENAS [R, hc] / [N, tc] / [N, 3]; the five tables are int32 on the device.
struct AssembleGroupsParams {
    AssembleParams a;
    const int* bounds;                // [G + 1] group g = places bounds[g] .. bounds[g + 1] - 1 of the (sorted) batch
    const int* h_g;                   // [G] history rows kept per impression
    const int* hist_row_off;          // [G + 1] first history arena row of the group
    const int* t_g;                   // [G] candidate slots kept per impression
    const int* cand_row_off;          // [G + 1] first candidate arena row of the group
    double* label_arena;              // [N]
    float* row_weight;                // [N]
    int* misfit;                      // raised by an impression that does not fit its group
    int G, R, N;
};
hipError_t assemble_groups_launch(const AssembleGroupsParams& p, hipStream_t st);

}  // namespace nrm
