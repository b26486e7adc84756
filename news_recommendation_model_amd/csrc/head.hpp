// Launchers of the BatchNorm column kernels (head.hip), shared with capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace nrm {
hipError_t colred_launch(int mode, const float* x, const float* dy, const float* mean, const float* rstd,
                         float* s0, float* s1, int R, int N, int ld, hipStream_t st);
hipError_t bn_apply_launch(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           float* y, long R, int N, int ld, hipStream_t st);
hipError_t bn_bwd_launch(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                         const float* s0, const float* s1, const float* add, float* dx, long R, int N, int ld, int training,
                         hipStream_t st);
// row-weight forms: row r stands for roww[r] equal rows of a batch of n_rows rows; modes 0 and 1 only, training only
hipError_t colred_roww_launch(int mode, const float* x, const float* mean, const float* roww, float* s0, int R, int N, int ld, hipStream_t st);
hipError_t bn_bwd_roww_launch(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                              const float* s0, const float* s1, const float* add, const float* roww, float* dx, long R, long n_rows, int N, int ld,
                              hipStream_t st);
constexpr int CONCAT_MAX = 8;
struct ConcatTable { const float* src[CONCAT_MAX]; long ld[CONCAT_MAX]; int start[CONCAT_MAX]; int n; };
hipError_t concat_cols_launch(const ConcatTable& tab, float* out, long R, int ldo, int total, hipStream_t st);
hipError_t bn_finalize_launch(int stage, const float* s, float* out, float* running, int R, int N, float momentum, float eps,
                              hipStream_t st);
hipError_t mul_bwd_launch(const float* dy, const float* g, const float* e, float* dg, float* de, long R, int N,
                          int lddy, int ldg, int lde, int ldo, hipStream_t st);
hipError_t small_linear_relu_fwd_launch(const void* x, int x_is_f64, const float* w, const float* b, float* y, long R, int K, int N,
                                        int ldy, hipStream_t st);
hipError_t small_linear_relu_bwd_launch(const void* x, int x_is_f64, const float* w, const float* b, const float* dy, int lddy,
                                        long R, int K, int N, float* dwb, hipStream_t st);
// head fold (head.hip): W' = W_o1 W_m2 into both packed gemm_nt images, and the split of its gradient
struct HeadFoldParams {
    const float* wo; const float* wm;     // W_o1 [P, Q], W_m2 [Q, R], contiguous; Q % 4 == 0, W_o1 16-byte aligned
    const float* bo; const float* bm;     // b_o1 [P], b_m2 [Q], or nullptr
    float* img_f; float* img_b;           // packed rows of W' ([P x R]) and of W'^T ([R x P])
    float* bias;                          // b' [P]
    int P, Q, R;
    int rows_f, kch_f, rows_b, kch_b;     // padded rows / 16-column chunks of the two images (gemm_nt_plan)
    int ti, tj;                           // filled by head_fold_launch
};
hipError_t head_fold_launch(HeadFoldParams p, hipStream_t st);
struct HeadSplitParams {
    const float* dwp; int ldp;            // dW' [P, ldp], ldp % 4 == 0, 16-byte aligned rows, columns [R, ldp) ignored
    const float* dbp;                     // db' [P]
    const float* wo; const float* wm;
    const float* bm;                      // b_m2 [Q] or nullptr
    float* dwo; float* dwm; float* dbo; float* dbm;      // outputs (contiguous, overwritten); nullptr: not wanted
    int P, Q, R;
    int na, nb, mm_blocks;                // filled by head_fold_bwd_launch
};
hipError_t head_fold_bwd_launch(HeadSplitParams p, hipStream_t st);
}  // namespace nrm
