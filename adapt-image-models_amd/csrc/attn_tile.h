// Tile steps shared by the attention kernels (attn_fwd.hip, attn_bwd.hip, win_attn.hip): head dim 64, one token per MFMA
// column / lane quartet, the other side's tokens streamed from swizzled LDS images.  The layout-level pieces (tr_frag,
// store_tiles16, stage_rows, load_frag) live beside the image in aim_common.h.
#pragma once
#include "aim_common.h"

namespace attn_tile {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float C2 = 0.125f * LOG2E;      // 1/sqrt(dh) * log2(e): the softmax, and its recomputation, run in base 2

// p = exp2(x) limited to [0, 1]: the limit is the clamp bit of the v_exp_f32 itself (no instruction of its own).  A true
// probability never exceeds 1, but a key past N has a zero-filled K row, so s = 0 and x = -lse log2(e): for a query whose
// log-sum-exp is below -88.7 (every logit strongly negative) exp2(x) is +inf, its dS is +-inf or NaN, and that times the zero
// K^T row put NaN into dQ.  With p <= 1 the dS of such a key is finite and its zero K^T row removes it, as designed.
__device__ __forceinline__ float prob_exp2(float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(x), 0.f, 1.f); }

// s[t][e] = sum_d img[t 16 + fq 4 + e][d] * x[lane & 15][d] for the 16 NT rows of an image
template <int NT>
__device__ __forceinline__ void tile_scores(f32x4 (&s)[NT], const AIM_LDS char* img, const bf16x8 (&xf)[2], int frow, int fq) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 af = lds_read8(img + swz_off(t * 16 + frow, ks * 4 + fq));
            s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[ks], s[t], 0, 0, 0);
        }
    }
}

// o[dt][e] += sum over the 32 rows of block kk of img[row][dt 16 + fq 4 + e] * wf[row], wf being two score tiles' bf16
// accumulators (tiles 2 kk and 2 kk + 1: the k order of tr_frag)
__device__ __forceinline__ void accum32(f32x4 (&o)[4], const AIM_LDS char* img, int kk, bf16x8 wf, int frow, int fq) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(img, kk, dt, frow, fq), wf, o[dt], 0, 0, 0);
}

// o[dt][e] += sum_rows img[row][dt 16 + fq 4 + e] * bf16(w[row]) over the 16 NT rows of an image (w in the tile_scores layout)
template <int NT>
__device__ __forceinline__ void tile_accum(f32x4 (&o)[4], const AIM_LDS char* img, const f32x4 (&w)[NT], int frow, int fq) {
#pragma unroll
    for (int kk = 0; kk < NT / 2; ++kk) {
        bf16x8 wf;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wf[e] = (bf16_t)w[2 * kk][e];
            wf[4 + e] = (bf16_t)w[2 * kk + 1][e];
        }
        accum32(o, img, kk, wf, frow, fq);
    }
}

// The dQ step of one query tile (query on the lane) over the 32 keys of block kk, keys on the MFMA row:  S^T = K Q^T and
// dP^T - delta = V dO^T with the accumulators started from -delta,  p = prob_exp2(s C2 - L2),  dS^T = bf16(p (dP^T - delta))
// used directly as the second operand of  dQ^T += K^T dS^T.  No key mask: rows of K and V past N are zero-filled in LDS, so
// such a key has a finite p (at most 1) and its dS meets a zero K^T row.  The 1/sqrt(dh) factor of dS is left to the caller's
// store.  per_key(key, bf16(p), bf16(dS)) sees every (key, query) of the lane.
template <typename F>
__device__ __forceinline__ void dq_key_pair(f32x4 (&dq)[4], const AIM_LDS char* sK, const AIM_LDS char* sV, int kk,
                                            const bf16x8 (&qf)[2], const bf16x8 (&dof)[2], float delta, float L2, int frow,
                                            int fq, F per_key) {
    bf16x8 dsf;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = 2 * kk + u;
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{-delta, -delta, -delta, -delta};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 kf = lds_read8(sK + swz_off(t * 16 + frow, ks * 4 + fq));
            const bf16x8 vf = lds_read8(sV + swz_off(t * 16 + frow, ks * 4 + fq));
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[ks], dp, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = prob_exp2(s[e] * C2 - L2);
            const bf16_t pb = (bf16_t)p, db = (bf16_t)(p * dp[e]);
            dsf[u * 4 + e] = db;
            per_key(t * 16 + fq * 4 + e, pb, db);
        }
    }
    accum32(dq, sK, kk, dsf, frow, fq);
}

// dO . O of a row whose 64 values lie in 8 lanes (8 each), on all eight: DPP quad_perm xor 1, xor 2, then row_half_mirror
// (the other quad of the eight); the ds_bpermute form of __shfl_xor made the pipelined kernel's delta wave its critical path
__device__ __forceinline__ float row_dot8(bf16x8 d8, bf16x8 o8) {
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) dl += (float)d8[e] * (float)o8[e];
    dl += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, dl), 0xB1, 0xF, 0xF, true));
    dl += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, dl), 0x4E, 0xF, 0xF, true));
    dl += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, dl), 0x141, 0xF, 0xF, true));
    return dl;
}

}  // namespace attn_tile
