// The row idiom of the LayerNorm family (norm.hip, embed_misc.hip, vit_imagenet.hip): one 64-lane wave per row, the row in
// registers as NC float4 chunks per lane (chunk c of a lane is float4 number lane + 64 c of the row; D <= NC * 256), fp32
// statistics from wave shuffles.  The family's rules stand here once: the chunk walk, the rounding order of the row mean and
// variance, the affine tail, the sums and the fixed last step of the LayerNorm backward, the stem's row, the NC ladder.
// Each kernel keeps its row-to-workgroup mapping, its loads and stores and its own sums; what stays written out in
// ln_bwd_kernel and in the two embed backward kernels, and why, is said there and in profiles/ln_row_ab.md.
#pragma once
#include <type_traits>
#include "aim_common.h"

// The chunk walk: the statement that follows runs for the lane's live chunks, c = 0 .. NC - 1 unrolled, ch = the row's
// float4 number (the expansion ends in an `if`: no `else` after the statement).  A macro, not a template taking the body
// as a lambda: the loop has to stand in the kernel itself.  Inside a helper it is unrolled before the helper is inlined,
// the kernel's row offsets are then computed again under every chunk's branch, no instantiation keeps its instruction
// stream and eight of them gain one to four VGPRs (profiles/ln_row_ab.md).
#define LN_ROW_CHUNKS(c, ch, NC, lane, nch) \
    _Pragma("unroll") for (int c = 0; c < (NC); ++c) \
        if (const int ch = (lane) + c * 64; ch < (nch))

namespace ln_row {

// ---- statistics: two passes over the row in registers ----
// the lane's share of a sum over the row, one chunk: (a+b)+(c+d); the chunks are added in order, then the wave (row_mean)
__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ float row_mean(float lane_sum, int D) { return wave_sum(lane_sum) / (float)D; }
// q + the chunk's squared deviations, one by one
__device__ __forceinline__ float add_sqdev4(float q, f32x4 v, float mu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = v[e] - mu;
        q += d * d;
    }
    return q;
}
__device__ __forceinline__ float row_rstd(float lane_sqdev, int D, float eps) { return rsqrtf(row_mean(lane_sqdev, D) + eps); }

__device__ __forceinline__ f32x4 ln_affine4(f32x4 v, float mu, float rs, f32x4 g, f32x4 b) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (v[e] - mu) * rs * g[e] + b[e];
    return y;
}

// ---- backward ----
// The first half, one live chunk: xh = (v - mu) rs and g = dy gamma stay in registers, s1 and s2 are the lane's running sums
// of g and of g xh (element by element; the product fused into the sum).  The row's m1 = row_mean(s1, D) and
// m2 = row_mean(s2, D) then feed the last step.  (ln_bwd_fsum_kernel; ln_bwd_kernel spells the same arithmetic out, for
// the registers of two of its instantiations.)
__device__ __forceinline__ void ln_bwd_chunk(f32x4 v, f32x4 dy, f32x4 gamma, float mu, float rs, f32x4& xh, f32x4& g, float& s1,
                                             float& s2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xh[e] = (v[e] - mu) * rs;
        g[e] = dy[e] * gamma[e];
        s1 += g[e];
        s2 = __builtin_fmaf(g[e], xh[e], s2);
    }
}

// The last steps of one element of the LayerNorm backward in ONE fixed operation order, whatever the compiler would fuse in
// the kernel around them: xhat * m2 folded into the subtraction (fma), the scale, then the residual as an addition of its own.
// ln_bwd_kernel and ln_bwd_fsum_kernel both go through these, which is what makes their dx the same bits (left to the
// compiler, one kernel fused rs * t + dres and all four xhat * m2, the other neither the first nor two of the four).
__device__ __forceinline__ float ln_bwd_elem(float g, float xh, float m1, float m2, float rs) {
#pragma clang fp contract(off)
    return rs * __builtin_fmaf(-xh, m2, g - m1);
}
__device__ __forceinline__ f32x4 ln_add_res(f32x4 o, f32x4 r) {
#pragma clang fp contract(off)
    return o + r;
}

// ---- the stem ----
// four columns c4 .. c4 + 3 of the stem's row (bt, n) before ln_pre: (cls | tok + pos) + temporal, as the forward builds it
template <typename TX>
__device__ __forceinline__ f32x4 embed_value(const TX* tok, const float* cls, const float* pos, const float* tmp, long long bt,
                                             int n, int t, int G2, int D, int c4) {
    f32x4 v = n == 0 ? *(const f32x4*)(cls + c4) : load4f(tok + (bt * G2 + (n - 1)) * D + c4);
    v += *(const f32x4*)(pos + (long long)n * D + c4);
    v += *(const f32x4*)(tmp + (long long)t * D + c4);
    return v;
}

// ---- host: the NC rule of every launch of the family ----
// chunks per lane as D needs them, 5 .. 8 in one instance; f(std::integral_constant<int, NC>)
template <typename F>
inline void nc_dispatch(int D, F f) {
    const int nc = (D + 255) / 256;
    if (nc <= 1) f(std::integral_constant<int, 1>{});
    else if (nc == 2) f(std::integral_constant<int, 2>{});
    else if (nc == 3) f(std::integral_constant<int, 3>{});
    else if (nc == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

}  // namespace ln_row
