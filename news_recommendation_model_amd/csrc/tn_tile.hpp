// Column layout and operand loads of a wave's block of W MFMA tiles, shared by gemm_tn_kernel (gemm.hip) and the backward
// contractions of the pointwise attention (pwattn_bwd.hip).
#pragma once
#include "common.hpp"

namespace nrm {

// Column layout of an operand block of W MFMA tiles (W in {2, 4, 5, 8}): fragment index r (0..15) of tile t is block column
//     W = 2:  2 r + t            (one  8-byte load per lane and reduction step)
//     W = 4:  4 r + t            (one 16-byte load)
//     W = 5:  4 r + t | 64 + r   (16 + 4 bytes)
//     W = 8:  4 r + t | 64 + 4 r + (t - 4)      (two 16-byte loads)
// so a lane's loads feed W MFMA operands without any shuffle.  Round 4 added W = 2 and 8: the head's weight gradients are
// 26 x 101 tiles of 16 (402 x 1608), which 4 x 4 wave tiles cover with 10.4 % padding and 2 x 8 with 3 % (13 x 13 exactly
// in i); w1's 25 x 26 tiles are exact in 5 x 2.
template <int W> __device__ __forceinline__ int tn_col(int t, int r) {
    if (W == 2) return 2 * r + t;
    if (W == 5 && t == 4) return 64 + r;
    if (W == 8 && t >= 4) return 64 + 4 * r + (t - 4);
    return 4 * r + t;
}
#if defined(__HIP_DEVICE_COMPILE__)
// One reduction row of the block: the low load (tiles 0..3, or 0..1 at W = 2) and the high load (the tiles above, W = 5 and 8) of
// a lane.  Apart, so that a kernel with two operands can issue both wide loads before the narrow ones.
template <int W> __device__ __forceinline__ void tn_load_lo(float (&v)[W], const __amdgpu_buffer_rsrc_t rs, unsigned vlo, int soff) {
    if constexpr (W == 2) {
        const auto x = __builtin_amdgcn_raw_buffer_load_b64(rs, vlo, soff, 0);
        v[0] = __uint_as_float(x[0]); v[1] = __uint_as_float(x[1]);
    } else {
        const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, vlo, soff, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __uint_as_float(x[e]);
    }
}
template <int W> __device__ __forceinline__ void tn_load_hi(float (&v)[W], const __amdgpu_buffer_rsrc_t rs, unsigned vhi, int soff) {
    if constexpr (W == 5) v[4] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, vhi, soff, 0));
    if constexpr (W == 8) {
        const u32x4 y = __builtin_amdgcn_raw_buffer_load_b128(rs, vhi, soff, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 + e] = __uint_as_float(y[e]);
    }
}
template <int W> __device__ __forceinline__ void tn_load(float (&v)[W], const __amdgpu_buffer_rsrc_t rs, unsigned vlo, unsigned vhi, int soff) {
    tn_load_lo<W>(v, rs, vlo, soff);
    tn_load_hi<W>(v, rs, vhi, soff);
}
#endif

}  // namespace nrm
