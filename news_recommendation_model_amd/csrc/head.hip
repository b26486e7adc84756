// BatchNorm1d over the [B*T, N] head rows (reference models/user_model.py:18,32: nn.BatchNorm1d, eps 1e-5,
// biased variance for normalisation) as HBM-bound column kernels.  gfx950 only.
//   colred_kernel<0>   s0[n] += sum_r x                              (mean)
//   colred_kernel<1>   s0[n] += sum_r (x - mean)^2                   (two-pass variance: no cancellation)
//   colred_kernel<2>   s0[n] += sum_r dy ; s1[n] += sum_r dy * (x - mean) * rstd       (d beta, d gamma)
//   bn_apply_kernel    y = (x - mean) * rstd * gamma + beta
//   bn_bwd_kernel      dx = gamma * rstd * (dy - s0/R - xhat * s1/R)    (train)   |  gamma * rstd * dy  (eval)
// ROWW (training on compacted candidate lists): row r of the launch stands for roww[r] >= 1 equal rows of the
// batch.  Modes 0 and 1 then sum roww[r] * x and roww[r] * (x - mean)^2, and the two column terms of the backward are multiplied by
// roww[r]; mode 2 sums gradients that already carry the weight and has no such form.  R of the finalisation and of 1/R in the backward is
// the row count of the BATCH (n_rows), not of the launch.  ROWW = false compiles to the code the kernels had before the flag.
// Layout: thread = one float4 of columns; blockDim (32, 8); a workgroup sweeps `rpb` rows of a 128-column slab
// and adds its partial sums with float atomics (R/rpb adds per column).
#include "common.hpp"
#include "head.hpp"

namespace nrm {

template <int MODE, bool ROWW = false>
__global__ __launch_bounds__(256) void colred_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     float* __restrict__ s0, float* __restrict__ s1,
                                                     int R, int N, int ld, int rpb, const float* __restrict__ roww) {
    __shared__ f32x4 red[2][8][32];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int col = blockIdx.x * 128 + 4 * tx;
    const bool cok = col < N;                       // N % 4 == 0
    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0, mu = a0, rs = a0;
    if (cok && MODE >= 1) mu = *reinterpret_cast<const f32x4*>(mean + col);
    if (cok && MODE == 2) rs = *reinterpret_cast<const f32x4*>(rstd + col);
    const int r_lo = blockIdx.y * rpb, r_hi = min(R, r_lo + rpb);
    if (cok) {
        for (int r = r_lo + ty; r < r_hi; r += 8) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)r * ld + col);
            if (MODE == 0) { if (ROWW) a0 += xv * roww[r]; else a0 += xv; }
            else if (MODE == 1) { const f32x4 d = xv - mu; if (ROWW) a0 += d * (d * roww[r]); else a0 += d * d; }      // weight 1: the same fma
            else {
                const f32x4 g = *reinterpret_cast<const f32x4*>(dy + (size_t)r * ld + col);
                a0 += g;
                a1 += g * (xv - mu) * rs;
            }
        }
    }
    red[0][ty][tx] = a0;
    if (MODE == 2) red[1][ty][tx] = a1;
    __syncthreads();
    if (ty == 0 && cok) {
        f32x4 t0 = red[0][0][tx], t1 = red[1][0][tx];
#pragma unroll
        for (int y = 1; y < 8; ++y) { t0 += red[0][y][tx]; if (MODE == 2) t1 += red[1][y][tx]; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            atomicAdd(s0 + col + e, t0[e]);
            if (MODE == 2) atomicAdd(s1 + col + e, t1[e]);
        }
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ y,
                                                       long R, int N, int ld) {
    const int n4 = N >> 2;
    const long total = R * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / n4;
        const int col = (int)(i - r * n4) * 4;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * ld + col);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + col), rs = *reinterpret_cast<const f32x4*>(rstd + col);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + col), b = *reinterpret_cast<const f32x4*>(beta + col);
        *reinterpret_cast<f32x4*>(y + r * ld + col) = (xv - mu) * rs * g + b;
    }
}

template <bool ROWW = false>
__global__ __launch_bounds__(256) void bn_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ s0,
                                                     const float* __restrict__ s1, const float* __restrict__ add,
                                                     float* __restrict__ dx, long R, int N, int ld, int training,
                                                     const float* __restrict__ roww, long n_rows) {
    const int n4 = N >> 2;
    const long total = R * n4;
    const float invR = 1.0f / (float)(ROWW ? n_rows : R);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / n4;
        const int col = (int)(i - r * n4) * 4;
        const f32x4 g = *reinterpret_cast<const f32x4*>(dy + r * ld + col);
        const f32x4 rs = *reinterpret_cast<const f32x4*>(rstd + col), ga = *reinterpret_cast<const f32x4*>(gamma + col);
        f32x4 out;
        if (training) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * ld + col);
            const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + col);
            const f32x4 a = *reinterpret_cast<const f32x4*>(s0 + col), b = *reinterpret_cast<const f32x4*>(s1 + col);
            const f32x4 xh = (xv - mu) * rs;
            // the weight goes onto the column sums first: with weight 1 the expression below is the unweighted one, operation for operation
            if (ROWW) { const float w = roww[r]; const f32x4 aw = a * w, bw = b * w; out = ga * rs * (g - aw * invR - xh * bw * invR); }
            else out = ga * rs * (g - a * invR - xh * b * invR);
        } else {
            out = ga * rs * g;
        }
        // the rows feed a second consumer besides BatchNorm (the gate product, user_model.py:33): its gradient joins here
        if (add) out += *reinterpret_cast<const f32x4*>(add + r * ld + col);
        *reinterpret_cast<f32x4*>(dx + r * ld + col) = out;
    }
}

// train-mode statistics between the column reductions (was ~8 tiny ATen launches per BatchNorm call):
//   stage 0: mean = s0 / R;  running_mean = (1 - momentum) running_mean + momentum mean
//   stage 1: var = s1 / R (biased, normalises);  rstd = 1/sqrt(var + eps);
//            running_var = (1 - momentum) running_var + momentum var R/(R-1)      (unbiased, nn.BatchNorm1d)
__global__ __launch_bounds__(256) void bn_finalize_kernel(int stage, const float* __restrict__ s, float* __restrict__ out,
                                                          float* __restrict__ running, int R, int N, float momentum, float eps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float v = s[i] / (float)R;
    if (stage == 0) {
        out[i] = v;
        if (running) running[i] = (1.0f - momentum) * running[i] + momentum * v;
    } else {
        out[i] = 1.0f / sqrtf(v + eps);
        if (running) running[i] = (1.0f - momentum) * running[i] + momentum * v * ((float)R / (float)(R > 1 ? R - 1 : 1));
    }
}

hipError_t bn_finalize_launch(int stage, const float* s, float* out, float* running, int R, int N, float momentum, float eps,
                              hipStream_t st) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((N + 255) / 256), dim3(256), 0, st, stage, s, out, running, R, N, momentum, eps);
    return hipGetLastError();
}

// backward of the gate product y = g * e (reference models/user_model.py:33): dg = dy * e, de = dy * g in one pass
__global__ __launch_bounds__(256) void mul_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ g,
                                                      const float* __restrict__ e, float* __restrict__ dg,
                                                      float* __restrict__ de, long R, int N, int lddy, int ldg, int lde,
                                                      int ldo) {
    const int n4 = N >> 2;
    const long total = R * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / n4;
        const int col = (int)(i - r * n4) * 4;
        const f32x4 d = *reinterpret_cast<const f32x4*>(dy + r * lddy + col);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + r * ldg + col);
        const f32x4 ev = *reinterpret_cast<const f32x4*>(e + r * lde + col);
        *reinterpret_cast<f32x4*>(dg + r * ldo + col) = d * ev;
        *reinterpret_cast<f32x4*>(de + r * ldo + col) = d * gv;
    }
}

hipError_t colred_launch(int mode, const float* x, const float* dy, const float* mean, const float* rstd,
                         float* s0, float* s1, int R, int N, int ld, hipStream_t st) {
    if (R <= 0) return hipSuccess;
    const int rpb = 256;
    const dim3 grid((N + 127) / 128, (R + rpb - 1) / rpb), block(32, 8);
    const float* none = nullptr;
    if (mode == 0) hipLaunchKernelGGL(colred_kernel<0>, grid, block, 0, st, x, dy, mean, rstd, s0, s1, R, N, ld, rpb, none);
    else if (mode == 1) hipLaunchKernelGGL(colred_kernel<1>, grid, block, 0, st, x, dy, mean, rstd, s0, s1, R, N, ld, rpb, none);
    else if (mode == 2) hipLaunchKernelGGL(colred_kernel<2>, grid, block, 0, st, x, dy, mean, rstd, s0, s1, R, N, ld, rpb, none);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t colred_roww_launch(int mode, const float* x, const float* mean, const float* roww, float* s0, int R, int N, int ld, hipStream_t st) {
    if (R <= 0) return hipSuccess;
    const int rpb = 256;
    const float* none = nullptr;
    float* nos1 = nullptr;
    const dim3 grid((N + 127) / 128, (R + rpb - 1) / rpb), block(32, 8);
    if (mode == 0) hipLaunchKernelGGL((colred_kernel<0, true>), grid, block, 0, st, x, none, mean, none, s0, nos1, R, N, ld, rpb, roww);
    else if (mode == 1) hipLaunchKernelGGL((colred_kernel<1, true>), grid, block, 0, st, x, none, mean, none, s0, nos1, R, N, ld, rpb, roww);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

static int ew_blocks(long total) { long b = (total + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

hipError_t bn_apply_launch(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           float* y, long R, int N, int ld, hipStream_t st) {
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_blocks(R * (N >> 2))), dim3(256), 0, st, x, mean, rstd, gamma, beta, y, R, N, ld);
    return hipGetLastError();
}

hipError_t mul_bwd_launch(const float* dy, const float* g, const float* e, float* dg, float* de, long R, int N,
                          int lddy, int ldg, int lde, int ldo, hipStream_t st) {
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(mul_bwd_kernel, dim3(ew_blocks(R * (N >> 2))), dim3(256), 0, st, dy, g, e, dg, de, R, N, lddy, ldg, lde, ldo);
    return hipGetLastError();
}

hipError_t bn_bwd_launch(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                         const float* s0, const float* s1, const float* add, float* dx, long R, int N, int ld, int training,
                         hipStream_t st) {
    if (R <= 0) return hipSuccess;
    const float* none = nullptr;
    hipLaunchKernelGGL(bn_bwd_kernel<false>, dim3(ew_blocks(R * (N >> 2))), dim3(256), 0, st, x, dy, mean, rstd, gamma, s0, s1, add, dx, R, N, ld, training,
                       none, R);
    return hipGetLastError();
}

hipError_t bn_bwd_roww_launch(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                              const float* s0, const float* s1, const float* add, const float* roww, float* dx, long R, long n_rows, int N, int ld,
                              hipStream_t st) {
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(bn_bwd_kernel<true>, dim3(ew_blocks(R * (N >> 2))), dim3(256), 0, st, x, dy, mean, rstd, gamma, s0, s1, add, dx, R, N, ld, 1,
                       roww, n_rows);
    return hipGetLastError();
}

// e = cat[parts...] along the columns (reference models/user_model.py:31, user_invariant_interest_model.py:81,88) in one launch:
// up to 8 row-major [R, w_i] sources (any leading dimension) -> out[R, ldo]; columns are copied dword by dword (the part
// widths of the head -- D_l, P, 8 -- need not be multiples of 4 in general)
template <int VEC>      // VEC = 4: every width, leading dimension and base address is a multiple of 4 floats (16 bytes)
__global__ __launch_bounds__(256) void concat_cols_kernel(const ConcatTable tab, float* __restrict__ out, unsigned R, int ldo, int total) {
    const unsigned tv = (unsigned)(total / VEC);
    const unsigned n = R * tv;                                          // host guarantees R * total < 2^31
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned r = i / tv;
        const int c = (int)(i - r * tv) * VEC;
        int k = 0;
#pragma unroll
        for (int j = 1; j < CONCAT_MAX; ++j) k += (j < tab.n && c >= tab.start[j]) ? 1 : 0;
        const float* src = tab.src[k] + (size_t)r * tab.ld[k] + (c - tab.start[k]);
        float* dst = out + (size_t)r * ldo + c;
        if (VEC == 4) *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(src);
        else *dst = *src;
    }
}

hipError_t concat_cols_launch(const ConcatTable& tab, float* out, long R, int ldo, int total, hipStream_t st) {
    if (R <= 0 || total <= 0) return hipSuccess;
    if (R * total >= (1L << 31)) return hipErrorInvalidValue;
    bool vec = (ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int i = 0; i < tab.n; ++i)
        vec = vec && (tab.start[i] & 3) == 0 && (tab.ld[i] & 3) == 0 && (reinterpret_cast<uintptr_t>(tab.src[i]) & 15) == 0;
    vec = vec && (total & 3) == 0;
    if (vec) hipLaunchKernelGGL(concat_cols_kernel<4>, dim3(ew_blocks(R * (total / 4))), dim3(256), 0, st, tab, out, (unsigned)R, ldo, total);
    else     hipLaunchKernelGGL(concat_cols_kernel<1>, dim3(ew_blocks(R * total)), dim3(256), 0, st, tab, out, (unsigned)R, ldo, total);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// y = ReLU(x W^T + b) for a handful of input and output columns (reference models/user_instant_interest_model.py: the 3
// popularity scalars of a candidate -> 8 features).  As a GEMM this was a zero-padded copy of x, a K = 4 launch, a clamp --
// and the same again backwards; here: one thread per row forward, a register reduction over rows backward.
constexpr int SL_KMAX = 4, SL_NMAX = 8;

template <typename XT>
__global__ __launch_bounds__(256) void small_linear_relu_fwd_kernel(const XT* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ b, float* __restrict__ y,
                                                                    long R, int K, int N, int ldy) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float xk[SL_KMAX];
#pragma unroll
    for (int k = 0; k < SL_KMAX; ++k) xk[k] = k < K ? (float)x[r * K + k] : 0.f;
    float* yr = y + r * ldy;
    for (int n = 0; n < ldy; ++n) {
        float v = 0.f;
        if (n < N) {
            v = b ? b[n] : 0.f;
#pragma unroll
            for (int k = 0; k < SL_KMAX; ++k) if (k < K) v = fmaf(w[n * K + k], xk[k], v);
            v = v <= 0.f ? 0.f : v;                                      // NaN stays NaN, as in torch.relu (fmaxf would give 0)
        }
        yr[n] = v;                                                       // padding columns are written as 0
    }
}

// dwb[n*K + k] += sum_r g[r,n] x[r,k],  dwb[N*K + n] += sum_r g[r,n],  g = dy where the pre-activation is positive
template <typename XT>
__global__ __launch_bounds__(256) void small_linear_relu_bwd_kernel(const XT* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ b, const float* __restrict__ dy,
                                                                    int lddy, long R, int K, int N, float* __restrict__ dwb) {
    float acc[SL_NMAX][SL_KMAX + 1];
#pragma unroll
    for (int n = 0; n < SL_NMAX; ++n)
#pragma unroll
        for (int k = 0; k <= SL_KMAX; ++k) acc[n][k] = 0.f;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long)gridDim.x * 256) {
        float xk[SL_KMAX];
#pragma unroll
        for (int k = 0; k < SL_KMAX; ++k) xk[k] = k < K ? (float)x[r * K + k] : 0.f;
#pragma unroll
        for (int n = 0; n < SL_NMAX; ++n) {
            if (n < N) {
                float pre = b ? b[n] : 0.f;
#pragma unroll
                for (int k = 0; k < SL_KMAX; ++k) if (k < K) pre = fmaf(w[n * K + k], xk[k], pre);
                const float g = pre > 0.f ? dy[r * lddy + n] : 0.f;
#pragma unroll
                for (int k = 0; k < SL_KMAX; ++k) acc[n][k] = fmaf(g, xk[k], acc[n][k]);
                acc[n][SL_KMAX] += g;
            }
        }
    }
    // wave sums -> LDS -> one float atomic per output and WORKGROUP (all workgroups hit the same N * (K + 1) addresses: with one
    // atomic per wave this tail was most of the kernel)
    __shared__ float part[4][SL_NMAX * (SL_KMAX + 1)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < SL_NMAX; ++n)
#pragma unroll
        for (int k = 0; k <= SL_KMAX; ++k) {
            const float v = wave_sum64(acc[n][k]);
            if (lane == 0) part[wave][n * (SL_KMAX + 1) + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < SL_NMAX * (SL_KMAX + 1)) {
        const int n = threadIdx.x / (SL_KMAX + 1), k = threadIdx.x - n * (SL_KMAX + 1);
        const float v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (n < N && (k < K || k == SL_KMAX) && v != 0.f) atomicAdd(dwb + (k == SL_KMAX ? N * K + n : n * K + k), v);
    }
}

hipError_t small_linear_relu_fwd_launch(const void* x, int x_is_f64, const float* w, const float* b, float* y, long R, int K, int N,
                                        int ldy, hipStream_t st) {
    if (R <= 0) return hipSuccess;
    if (K < 1 || K > SL_KMAX || N < 1 || N > SL_NMAX || ldy < N) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((R + 255) / 256));
    if (x_is_f64) hipLaunchKernelGGL(small_linear_relu_fwd_kernel<double>, grid, dim3(256), 0, st, (const double*)x, w, b, y, R, K, N, ldy);
    else          hipLaunchKernelGGL(small_linear_relu_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)x, w, b, y, R, K, N, ldy);
    return hipGetLastError();
}

hipError_t small_linear_relu_bwd_launch(const void* x, int x_is_f64, const float* w, const float* b, const float* dy, int lddy,
                                        long R, int K, int N, float* dwb, hipStream_t st) {
    if (R <= 0) return hipSuccess;
    if (K < 1 || K > SL_KMAX || N < 1 || N > SL_NMAX || lddy < N) return hipErrorInvalidValue;
    long blocks = (R + 255) / 256;                                       // one row per thread up to 256 workgroups (one atomic per output each)
    if (blocks > 256) blocks = 256;
    if (x_is_f64) hipLaunchKernelGGL(small_linear_relu_bwd_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)x, w, b, dy, lddy, R, K, N, dwb);
    else          hipLaunchKernelGGL(small_linear_relu_bwd_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x, w, b, dy, lddy, R, K, N, dwb);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Head fold (reference models/user_model.py:34: out_mlp(mlp(gated))): no nonlinearity sits between mlp.fc2 [Q, R] and
// out_mlp.fc1 [P, Q], so the step evaluates  z2 = a1 W'^T + b'  with  W' = W_o1 W_m2 [P, R],  b' = W_o1 b_m2 + b_o1  and never
// forms the Q-wide intermediate.  Both kernels are weight-sized: fp32 MFMA 16 x 16 tiles, operands straight from global memory.
//
//   head_fold_kernel      one workgroup per 16 x 16 tile of W'; its four waves take every fourth 16-wide chunk of the reduction
//                         over Q (a chain of Q/64 chunk rounds per wave instead of Q/16), the partial tiles meet in LDS, and the
//                         tile goes straight into gemm_nt's packed operand layout (pack_rows_kernel) TWICE: as rows of W' (the
//                         forward) and as rows of W'^T (da1 = dz2 W').  Tiles of the images' zero padding are written too.
//   head_fold_bwd_kernel  dW_o1 = dW' W_m2^T + db' (x) b_m2 [P, Q],  dW_m2 = W_o1^T dW' [Q, R]: one wave per 16 x 16 output tile (reduction over
//                         R / P: 26 chunks at the flagship widths), plus db_o1 = db', db_m2 = W_o1^T db' on the last workgroups.
__global__ __launch_bounds__(256) void head_fold_kernel(const HeadFoldParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float part[4][16][17];
    __shared__ float bpart[4][16];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int ti = blockIdx.x % p.ti, tj = blockIdx.x / p.ti;
    const int i0 = ti * 16, j0 = tj * 16;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float bs = 0.f;
    if (i0 < p.P && j0 < p.R) {                                        // (workgroup-uniform) else: a tile of the padding
        const int nch = (p.Q + 15) >> 4;
        const int i = i0 + r16, j = j0 + r16;
        const bool iok = i < p.P, jok = j < p.R;
        const float* arow = p.wo + (size_t)(iok ? i : 0) * p.Q;
        const bool want_b = tj == 0 && p.bm != nullptr;
        // lane (r16, q) holds k = 16 c + 4 q + e in operand e: MFMA e of a chunk reduces over k = e, 4 + e, 8 + e, 12 + e
        // four chunks per round: their 4 + 16 loads are in flight together (chunks past the end load nothing: k >= Q)
        for (int c = wave; c < nch; c += 16) {
            f32x4 a[4];
            float b[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = 16 * (c + 4 * u) + 4 * q;
                a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (iok && k < p.Q) a[u] = *reinterpret_cast<const f32x4*>(arow + k);      // Q % 4 == 0: the float4 is inside the row or past it
#pragma unroll
                for (int e = 0; e < 4; ++e) b[u][e] = (jok && k + e < p.Q) ? p.wm[(size_t)(k + e) * p.R + j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = mfma16(a[u][e], b[u][e], acc);
                const int k = 16 * (c + 4 * u) + 4 * q;
                if (want_b && iok && k < p.Q) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) bs = fmaf(a[u][e], p.bm[k + e], bs);
                }
            }
        }
    }
    // lane holds W'[i0 + 4 q + e][j0 + r16] (this wave's share of the reduction)
#pragma unroll
    for (int e = 0; e < 4; ++e) part[wave][4 * q + e][r16] = acc[e];
    bs = sum_rows4(bs);
    if (q == 0) bpart[wave][r16] = bs;
    __syncthreads();
    const int a = tid >> 4, b = tid & 15;
    float v = (part[0][a][b] + part[1][a][b]) + (part[2][a][b] + part[3][a][b]);
    if (i0 + a >= p.P || j0 + b >= p.R) v = 0.f;                       // the images' padding is exactly zero
    part[0][a][b] = v;
    __syncthreads();
    {   // rows of W': packed[c = tj][row = i][16]
        const int row = i0 + a;
        if (row < p.rows_f && tj < p.kch_f)
            p.img_f[((size_t)tj * p.rows_f + row) * 16 + 4 * ((b >> 2) ^ swz4(row)) + (b & 3)] = v;
    }
    {   // rows of W'^T: packed[c = ti][row = j][16]
        const int row = j0 + a;
        if (row < p.rows_b && ti < p.kch_b)
            p.img_b[((size_t)ti * p.rows_b + row) * 16 + 4 * ((b >> 2) ^ swz4(row)) + (b & 3)] = part[0][b][a];
    }
    if (tj == 0 && tid < 16 && i0 + tid < p.P)
        p.bias[i0 + tid] = ((bpart[0][tid] + bpart[1][tid]) + (bpart[2][tid] + bpart[3][tid])) + (p.bo ? p.bo[i0 + tid] : 0.f);
#endif
}

hipError_t head_fold_launch(HeadFoldParams p, hipStream_t st) {
    p.ti = p.rows_f / 16;                                              // rows_f >= 16 kch_b, rows_b >= 16 kch_f: the grid covers both images
    p.tj = p.rows_b / 16;
    if (p.ti < p.kch_b || p.tj < p.kch_f) return hipErrorInvalidValue;
    hipLaunchKernelGGL(head_fold_kernel, dim3((unsigned)(p.ti * p.tj)), dim3(256), 0, st, p);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void head_fold_bwd_kernel(const HeadSplitParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    if ((int)blockIdx.x >= p.mm_blocks) {                               // vector leg
        const int c = ((int)blockIdx.x - p.mm_blocks) * 256 + tid;
        if (p.dbm && c < p.Q) {
            float s = 0.f;
#pragma unroll 4
            for (int i = 0; i < p.P; ++i) s = fmaf(p.wo[(size_t)i * p.Q + c], p.dbp[i], s);
            p.dbm[c] = s;
        }
        if (p.dbo && c < p.P) p.dbo[c] = p.dbp[c];
        return;
    }
    const int id = blockIdx.x * 4 + wave;
    if (id >= p.na + p.nb) return;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int tq = (p.Q + 15) >> 4, tr = (p.R + 15) >> 4;
    if (id < p.na) {
        // dW_o1[i, c] = sum_j dW'[i, j] W_m2[c, j]
        const int c0 = (id % tq) * 16, i0 = (id / tq) * 16;
        const int i = i0 + r16, c = c0 + r16;
        const bool iok = i < p.P, cok = c < p.Q;
        const float* arow = p.dwp + (size_t)(iok ? i : 0) * p.ldp;
        const float* brow = p.wm + (size_t)(cok ? c : 0) * p.R;
        for (int k0 = 0; k0 < p.R; k0 += 16) {
            const int k = k0 + 4 * q;
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
            float b[4];
            if (iok && k < p.R) a = *reinterpret_cast<const f32x4*>(arow + k);      // ldp = pad4(R): the float4 stays inside the row
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool kok = k + e < p.R;
                a[e] = kok ? a[e] : 0.f;
                b[e] = (cok && kok) ? brow[k + e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma16(a[e], b[e], acc);
        }
        // out_mlp.fc1 saw mlp.fc2's output INCLUDING its bias: dW_o1 = dz2^T (a1 W_m2^T + b_m2) = dW' W_m2^T + db' (x) b_m2
        const float bmc = (p.bm && cok) ? p.bm[c] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + 4 * q + e < p.P && cok) p.dwo[(size_t)(i0 + 4 * q + e) * p.Q + c] = fmaf(p.dbp[i0 + 4 * q + e], bmc, acc[e]);
    } else {
        // dW_m2[c, j] = sum_i W_o1[i, c] dW'[i, j]
        const int t = id - p.na;
        const int j0 = (t % tr) * 16, c0 = (t / tr) * 16;
        const int c = c0 + r16, j = j0 + r16;
        const bool cok = c < p.Q, jok = j < p.R;
        for (int k0 = 0; k0 < p.P; k0 += 16) {
            const int k = k0 + 4 * q;
            float a[4], b[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool kok = k + e < p.P;
                a[e] = (cok && kok) ? p.wo[(size_t)(k + e) * p.Q + c] : 0.f;
                b[e] = (jok && kok) ? p.dwp[(size_t)(k + e) * p.ldp + j] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma16(a[e], b[e], acc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + 4 * q + e < p.Q && jok) p.dwm[(size_t)(c0 + 4 * q + e) * p.R + j] = acc[e];
    }
#endif
}

hipError_t head_fold_bwd_launch(HeadSplitParams p, hipStream_t st) {
    const int tp = (p.P + 15) / 16, tq = (p.Q + 15) / 16, tr = (p.R + 15) / 16;
    p.na = p.dwo ? tp * tq : 0;
    p.nb = p.dwm ? tq * tr : 0;
    p.mm_blocks = (p.na + p.nb + 3) / 4;
    const int nv = (p.dbm || p.dbo) ? ((p.Q > p.P ? p.Q : p.P) + 255) / 256 : 0;
    if (p.mm_blocks + nv == 0) return hipSuccess;
    hipLaunchKernelGGL(head_fold_bwd_kernel, dim3((unsigned)(p.mm_blocks + nv)), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace nrm
