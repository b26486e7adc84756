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

// ---- history compaction: the trailing all-zero history rows of an impression are dropped like its padded candidates
// hist_len[b] = 1 + the last row of x_history [B, H, words] (32-bit words: a float64 column is two) that holds any non-zero BIT, 0 if none
hipError_t history_len_launch(const unsigned* x, int B, int H, int words, int* hist_len, hipStream_t st);
// xh_c[hist_off[b] + j, :] = x[b, j, :] for j < hist_off[b + 1] - hist_off[b] (bitwise); k_max = the longest kept history (it sizes the grid)
hipError_t history_gather_launch(const unsigned* x, unsigned* xh_c, int words, const int* hist_off, int B, int H, int R, int k_max, hipStream_t st);
// Grouped history arena of the compacted training step (section 5e): group g holds the impressions b0[g] .. b0[g + 1] - 1 of the sorted batch, each
// trimmed to hg[g] rows, from arena row row_off[g]; sorted impression b is impression src_imp[b] of x.  One launch for all G groups.
constexpr int HISTORY_GROUPS_MAX = 64;
hipError_t history_gather_groups_launch(const unsigned* x, unsigned* xh_g, int words, const int* src_imp, const int* b0, const int* row_off,
                                        const int* hg, int G, int B, int H, int R, hipStream_t st);
// Grouped candidate arena of the step that trains on compacted candidate lists (section 5f): group g holds the impressions b0[g] .. b0[g + 1] - 1
// of the sorted batch, each trimmed to tg[g] candidate columns, from arena row row_off[g]; where tg[g] < T the group's last column stands for
// T - tg[g] + 1 equal padded candidates (its row weight) and every dropped cell is compared with it.  One launch for all G groups.
struct CandidateGatherParams {
    const unsigned* xt; const unsigned* xg; const unsigned* lab;     // [B*T, wt] / [B*T, wg] / [B*T, wl] as 32-bit words
    unsigned* xt_a; unsigned* xg_a; unsigned* lab_a;                 // [N, wt] / [N, wg] / [N, wl]
    float* roww;                                                     // [N]
    int wt, wg, wl;
    const int* src_imp; const int* b0; const int* row_off; const int* tg;     // [B], [G + 1], [G + 1], [G]
    int G, B, T, N;
    int* flag;                                                       // the pad-error flag of CompactGatherParams
};
hipError_t candidate_gather_groups_launch(const CandidateGatherParams& p, hipStream_t st);
// Per-tile table of the history-ragged attention: the score rows of compact candidate c (impression b = cand_imp[c], K_b kept history rows)
// are nt_b = ceil(K_b / 16) whole 16-row tiles, tile_pre[b] + (c - cand_off[b]) nt_b + jt; entry = {c, first row of the tile in h_c / u,
// valid rows of the tile, b}.  One thread per candidate writes its nt_b entries.
hipError_t history_tiles_launch(const int* cand_imp, const int* cand_off, const int* hist_off, const int* tile_pre, int B, int N, int R, int Mt,
                                int4* tile_tab, hipStream_t st);

}  // namespace nrm
