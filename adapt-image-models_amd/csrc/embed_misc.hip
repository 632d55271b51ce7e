// Patch-embedding glue and the small reductions / casts around the AIM block.  gfx950 only.
//
// patchify / embed_ln / embed_bwd: reference vit_clip.py:434-447 -- rearrange 'b c t h w -> (b t) c h w',
//   conv1 (kernel = stride = patch, no bias; done as a GEMM over the patch matrix written here),
//   class_embedding concat (:439), + positional_embedding (:440), + temporal_embedding (:443-445),
//   ln_pre (:447).  Optional uint8 input fuses the GPUNormalize pre-hook
//   (mmaction/utils/module_hooks.py:73-85): x.float().sub_(mean).div_(std).
//   The patch gather is ONE kernel template, patchify_kernel<TIN, TOUT, BLEND>: bf16 or f32 output (the fp32 verification
//   mode's entry points sit in fp32.hip), with or without a mixup / cutmix of two clips.  Its four entry points
//   (aim_patchify, aim_patchify_blend, aim_patchify_f32, aim_patchify_blend_f32) keep their own checks and share
//   aim_patchify_launch.
// frame_sum / colsum / cast / scale_rows: bandwidth-bound helpers for the hand-written backward
//   (per-frame token sums for the broadcast S_Adapter term, bias gradients, bf16 weight staging).
#include "aim_common.h"
#include "aim_kernels_internal.h"
#include "ln_row.h"

namespace {
using namespace ln_row;

constexpr int MAXC = 8;

// ---- the patch gather, with mini-batch blending fused into it (AimBlend: aim_kernels_internal.h) --------------------------
// the reference's eager `lam * a + (1 - lam) * b` rounds each product and the sum: no contraction into an FMA here
__device__ __forceinline__ float blend_mix(float a, float b, float lam, float oml) {
    return __fadd_rn(__fmul_rn(lam, a), __fmul_rn(oml, b));
}
// the partner of clip b: the host builds a permutation, the clamp keeps a bad table from reading outside the batch
__device__ __forceinline__ long long blend_partner(const AimBlend& bl, long long b, int B) {
    return (long long)min(max(bl.partner[b], 0), B - 1);
}
__device__ __forceinline__ bool blend_in_box(const AimBlend& bl, int y, int x) {
    return y >= bl.y1 && y < bl.y2 && x >= bl.x1 && x < bl.x2;
}

// one pixel, normalised when the uint8 GPUNormalize is fused
template <typename TIN>
__device__ __forceinline__ float load_px(const TIN* src, const float* mean3, const float* std3, int c) {
    float v = (float)*src;
    if (mean3) v = (v - mean3[c]) / std3[c];
    return v;
}
// 8 consecutive pixels of one image row (16-byte aligned image, x a multiple of 8): one or two 16-byte loads instead of eight
// scalar ones with their index arithmetic
template <typename TIN>
__device__ __forceinline__ void load_px8(const TIN* src, const float* mean3, const float* std3, int c, float v[8]) {
    if constexpr (sizeof(TIN) == 4) {
        const f32x4 a0 = *(const f32x4*)src, a1 = *(const f32x4*)(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = a0[e];
            v[4 + e] = a1[e];
        }
    } else if constexpr (sizeof(TIN) == 2) {
        const bf16x8 a0 = *(const bf16x8*)src;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)a0[e];
    } else {
        const uint2 a0 = *(const uint2*)src;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = (float)((a0.x >> (8 * e)) & 0xffu);
            v[4 + e] = (float)((a0.y >> (8 * e)) & 0xffu);
        }
    }
    if (mean3) {
        const float m = mean3[c], sd = std3[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (v[e] - m) / sd;
    }
}

// A[(bt*G*G + gy*G + gx)][c*p*p + py*p + px] = img[b][c][t][gy*p+py][gx*p+px], bf16 or f32; one thread per 16 bytes of a row
// of A (pad columns k >= 3 p p: zero).  BLEND: a mixup / cutmix of clip b and clip partner[b] is applied while gathering, so
// the blended clip is never written; mixup blends the NORMALISED values (lam * norm(a) + oml * norm(b)).  `bl` is read by
// the BLEND instantiations only.
template <typename TIN, typename TOUT, bool BLEND>
__global__ __launch_bounds__(256) void patchify_kernel(const TIN* __restrict__ img, const float* __restrict__ mean3,
                                                       const float* __restrict__ std3, TOUT* __restrict__ A, int B, int T,
                                                       int H, int W, int p, int Kp, AimBlend bl) {
    constexpr int NC = 16 / sizeof(TOUT);
    const int G = W / p, Gy = H / p, K = 3 * p * p;
    const long long rows = (long long)B * T * Gy * G;
    const int cpr = Kp / NC;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * cpr) return;
    const long long row = idx / cpr;
    const int k0 = (int)(idx - row * cpr) * NC;
    const int gx = (int)(row % G), gy = (int)((row / G) % Gy);
    const long long bt = row / ((long long)G * Gy);
    const int t = (int)(bt % T);
    const long long b = bt / T, plane = (long long)T * H * W;
    long long pb = b;
    bool mixup = false;
    if constexpr (BLEND) {
        pb = blend_partner(bl, b, B);
        mixup = bl.mode == 1;
    }
    float v[8];      // the first NC are the thread's columns; f32 output (a verification mode) always gathers pixel by pixel
    if (NC == 8 && (p & 7) == 0 && (W & 7) == 0 && k0 + 8 <= K && ((unsigned long long)img & 15) == 0) {
        // patch width a multiple of 8 (ViT-B/16), bf16 output: the thread's 8 columns are 8 consecutive pixels of one image row
        const int c = k0 / (p * p), rem = k0 - c * p * p, py = rem / p, px = rem - py * p;
        const int y = gy * p + py, x0 = gx * p + px;
        const long long pix = ((long long)t * H + y) * W + x0;
        const TIN* sa = img + (b * 3 + c) * plane + pix;
        if constexpr (BLEND) {
            // cutmix loads the partner's run only where the box covers it: a run outside the box reads clip b, a run inside
            // it clip partner[b], a run across an edge both
            const TIN* sb = img + (pb * 3 + c) * plane + pix;
            const bool rowin = y >= bl.y1 && y < bl.y2;
            const bool none = !mixup && (!rowin || x0 + 8 <= bl.x1 || x0 >= bl.x2);
            const bool all = !mixup && rowin && x0 >= bl.x1 && x0 + 8 <= bl.x2;
            load_px8(all ? sb : sa, mean3, std3, c, v);
            if (!none && !all) {
                float q[8];
                load_px8(sb, mean3, std3, c, q);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (mixup)
                        v[e] = blend_mix(v[e], q[e], bl.lam, bl.oml);
                    else if (x0 + e >= bl.x1 && x0 + e < bl.x2)
                        v[e] = q[e];
                }
            }
        } else {
            load_px8(sa, mean3, std3, c, v);
        }
    } else {
#pragma unroll
        for (int e = 0; e < NC; ++e) {
            const int k = k0 + e;
            v[e] = 0.f;
            if (k < K) {
                const int c = k / (p * p), rem = k - c * p * p, py = rem / p, px = rem - py * p;
                const int y = gy * p + py, x = gx * p + px;
                const long long pix = ((long long)t * H + y) * W + x;
                const TIN* sa = img + (b * 3 + c) * plane + pix;
                if constexpr (BLEND) {
                    const TIN* sb = img + (pb * 3 + c) * plane + pix;
                    if (mixup)
                        v[e] = blend_mix(load_px(sa, mean3, std3, c), load_px(sb, mean3, std3, c), bl.lam, bl.oml);
                    else
                        v[e] = load_px(blend_in_box(bl, y, x) ? sb : sa, mean3, std3, c);
                } else {
                    v[e] = load_px(sa, mean3, std3, c);
                }
            }
        }
    }
    typedef __attribute__((ext_vector_type(NC))) TOUT out_t;
    out_t o;
#pragma unroll
    for (int e = 0; e < NC; ++e) o[e] = (TOUT)v[e];
    *(out_t*)(A + row * Kp + k0) = o;
}

template <int NC>
__global__ __launch_bounds__(256) void embed_ln_kernel(const bf16_t* __restrict__ tok, const float* __restrict__ cls,
                                                       const float* __restrict__ pos, const float* __restrict__ tmp,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ x, float* __restrict__ mean,
                                                       float* __restrict__ rstd, int B, int T, int N, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * T * N) return;
    const long long bt = row / N;
    const int n = (int)(row - bt * N), t = (int)(bt % T), nch = D >> 2;
    f32x4 v[NC];
    float s = 0.f, q = 0.f;
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
        v[c] = embed_value(tok, cls, pos, tmp, bt, n, t, N - 1, D, ch * 4);
        s += sum4(v[c]);
    }
    const float mu = row_mean(s, D);
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) q = add_sqdev4(q, v[c], mu);
    const float rs = row_rstd(q, D, eps);
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
    LN_ROW_CHUNKS(c, ch, NC, lane, nch)
        store4(x + row * D + ch * 4, ln_affine4(v[c], mu, rs, *(const f32x4*)(gamma + ch * 4), *(const f32x4*)(beta + ch * 4)));
}

// grid (T, chunks): every wave walks rows (b, n) of frame-time t, accumulates ln_pre's input gradient
// in registers and adds it into dtemporal[t] once at the end.
template <int NC, typename TDX>
__global__ __launch_bounds__(256) void embed_bwd_kernel(const TDX* __restrict__ dx, const bf16_t* __restrict__ tok,
                                                        const float* __restrict__ cls, const float* __restrict__ pos,
                                                        const float* __restrict__ tmp, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        float* __restrict__ dtemporal, float* __restrict__ partial, int B,
                                                        int T, int N, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x, nch = D >> 2;
    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int total = B * N;
    for (int r = blockIdx.y * 4 + wave; r < total; r += gridDim.y * 4) {
        const int b = r / N, n = r - b * N;
        const long long bt = (long long)b * T + t, row = bt * N + n;
        const float mu = mean[row], rs = rstd[row];
        f32x4 g[NC], xh[NC];
        float s1 = 0.f, s2 = 0.f;
        // Written out, not ln_bwd_chunk and ln_bwd_elem: here the compiler chooses what it contracts (it fuses part of the
        // g xh products into s2, and the scale into the accumulation), and dtemporal keeps the bits of that choice.
        LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
            const f32x4 v = embed_value(tok, cls, pos, tmp, bt, n, t, N - 1, D, ch * 4);
            const f32x4 d = load4f(dx + row * D + ch * 4);
            const f32x4 gm = *(const f32x4*)(gamma + ch * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xh[c][e] = (v[e] - mu) * rs;
                g[c][e] = d[e] * gm[e];
                s1 += g[c][e];
                s2 += g[c][e] * xh[c][e];
            }
        }
        const float m1 = row_mean(s1, D), m2 = row_mean(s2, D);
        LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c][e] += rs * (g[c][e] - m1 - xh[c][e] * m2);
        }
    }
    if (partial) {
        // deterministic form: the block's four waves are summed in a fixed order through LDS and the block's partial row goes
        // to partial[t][blockIdx.y][D]; embed_bwd_finish_kernel adds the rows up in order (no atomics anywhere)
        __shared__ float red[3][NC * 256];
        if (wave > 0) {
            LN_ROW_CHUNKS(c, ch, NC, lane, nch) *(f32x4*)(&red[wave - 1][ch * 4]) = acc[c];
        }
        __syncthreads();
        if (wave == 0) {
            LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
                f32x4 a = acc[c];
                for (int w = 0; w < 3; ++w) a += *(const f32x4*)(&red[w][ch * 4]);
                *(f32x4*)(partial + ((long long)t * gridDim.y + blockIdx.y) * D + ch * 4) = a;
            }
        }
        return;
    }
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(dtemporal + (long long)t * D + ch * 4 + e, acc[c][e]);
    }
}

// dtemporal[t][c] += sum over the blocks' partial rows, in a fixed order: 64 columns x 4 row groups per workgroup, eight loads in
// flight per thread (the first version walked the 256 partial rows one dependent load at a time: 114 us)
__global__ __launch_bounds__(256) void embed_bwd_finish_kernel(const float* __restrict__ partial, float* __restrict__ dtemporal,
                                                               int chunks, int D) {
    __shared__ float red[4][64];
    const int t = blockIdx.x, cl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const bool live = c < D;
    const float* p = partial + (long long)t * chunks * D + (live ? c : 0);
    float a = 0.f;
    int y = g;
    for (; y + 28 < chunks; y += 32) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(long long)(y + 4 * u) * D];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; y < chunks; y += 4) a += p[(long long)y * D];
    red[g][cl] = a;
    __syncthreads();
    if (g == 0 && live) dtemporal[(long long)t * D + c] += (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// out[frame][d] = sum_tok w[tok] x[frame][tok][d].  Block (frame, 64-column group): 4 token groups x 64 float4-columns; a
// thread walks tokens g, g+4, ... with eight loads in flight, the four partial sums meet in LDS in a fixed order.  (The first
// version walked all tokens of a column in one thread, four loads in flight: latency-bound at 0.6 TB/s, and it opens the
// backward's class-token chain.)
template <typename TX>
__global__ __launch_bounds__(256) void frame_sum_kernel(const TX* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ out, int ntok, int D) {
    __shared__ f32x4 part[4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int d4 = blockIdx.y * 64 + cl;                   // float4 column
    const bool live = d4 * 4 < D;
    const long long f = blockIdx.x;
    const TX* p = x + f * ntok * (long long)D + (live ? d4 * 4 : 0);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    int t = g;
    for (; t + 28 < ntok; t += 32) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = load4f(p + (long long)(t + 4 * u) * D);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (w ? w[t + 4 * u] : 1.0f) * v[u];
    }
    for (; t < ntok; t += 4) acc += (w ? w[t] : 1.0f) * load4f(p + (long long)t * D);
    part[g][cl] = acc;
    __syncthreads();
    if (g == 0 && live) *(f32x4*)(out + f * D + d4 * 4) = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
}

__global__ __launch_bounds__(256) void colsum_kernel(const bf16_t* __restrict__ X, int ldx, const float* __restrict__ af,
                                                     const float* __restrict__ at, int ntok, float* __restrict__ out,
                                                     int M, int C, int rows_per_block) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    float acc = 0.f;
    for (int r = r0; r < r1; ++r) {
        float rs = 1.f;
        if (af || at) {
            const int f = r / ntok, tk = r - f * ntok;
            if (af) rs *= af[f];
            if (at) rs *= at[tk];
        }
        acc += rs * (float)X[(long long)r * ldx + c];
    }
    atomicAdd(out + c, acc);
}

// 8 columns per thread (16-byte loads); threads = (C/8 column groups) x (row slots); rows strided by slots
__global__ __launch_bounds__(256) void colsum8_kernel(const bf16_t* __restrict__ X, int ldx, const float* __restrict__ af,
                                                      const float* __restrict__ at, int ntok, float* __restrict__ out,
                                                      float* __restrict__ partial, int M, int C, int rows_per_block) {
    const int cg = C >> 3;
    const int nrs = 256 / cg > 0 ? 256 / cg : 1;
    const int t = threadIdx.x;
    const int col = t % cg;   // column group
    const int rslot = t / cg;
    const bool live = rslot < nrs;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // 4 independent 16-byte loads in flight per thread
    int r = r0 + rslot;
    for (; live && r + 3 * nrs < r1; r += 4 * nrs) {
        bf16x8 v[4];
        float rs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rr = r + u * nrs;
            v[u] = *(const bf16x8*)(X + (long long)rr * ldx + col * 8);
            rs[u] = 1.f;
            if (af || at) {
                const int f = rr / ntok, tk = rr - f * ntok;
                if (af) rs[u] *= af[f];
                if (at) rs[u] *= at[tk];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += rs[u] * (float)v[u][e];
    }
    for (; live && r < r1; r += nrs) {
        float rs = 1.f;
        if (af || at) {
            const int f = r / ntok, tk = r - f * ntok;
            if (af) rs *= af[f];
            if (at) rs *= at[tk];
        }
        const bf16x8 v = *(const bf16x8*)(X + (long long)r * ldx + col * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += rs * (float)v[e];
    }
    // reduce the row slots of this block through LDS, then ONE atomic per column per block
    __shared__ float red[256 * 8];
    if (live) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(rslot * cg + col) * 8 + e] = acc[e];
    }
    __syncthreads();
    if (rslot == 0) {
        for (int s2 = 1; s2 < nrs; ++s2)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += red[(s2 * cg + col) * 8 + e];
        if (partial) {       // stage 1 of a two-stage reduction: no atomics, no contention
            f32x4* p = (f32x4*)(partial + (long long)blockIdx.y * C + col * 8);
            p[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
            p[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) atomicAdd(out + col * 8 + e, acc[e]);
        }
    }
}

// stage 2: out[c] += sum_p partial[p][c].  ONE block of 64 columns x 16 row-slots per column group: every sum has a fixed
// order (slot s adds partials s, s+16, ...; the slots are added 0..15) and the update is a plain read-modify-write --
// bitwise reproducible, no atomics; it runs off the critical path.
__global__ __launch_bounds__(1024) void colsum_finish_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                             int P, int C) {
    __shared__ float red[1024];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int slot = threadIdx.x >> 6;
    float acc = 0.f;
    if (c < C)
        for (int p = slot; p < P; p += 16) acc += partial[(long long)p * C + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (slot == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) t += red[threadIdx.x + 64 * s2];
        out[c] += t;
    }
}

__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long long n) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        const f32x4 v = *(const f32x4*)(src + i);
        *(bf16x4*)(dst + i) = pack4(v[0], v[1], v[2], v[3]);
    } else {
        for (long long j = i; j < n; ++j) dst[j] = (bf16_t)src[j];
    }
}

// row-strided destination: dst[r * ldd + c] = src[r * C + c]
__global__ __launch_bounds__(256) void cast_strided_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int R,
                                                           int C, int ldd) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)R * C) return;
    const int r = (int)(i / C), c = (int)(i - (long long)r * C);
    dst[(long long)r * ldd + c] = (bf16_t)src[i];
}

// dst[c][r] = src[r][c]
__global__ __launch_bounds__(256) void cast_transpose_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst,
                                                             int R, int C, int ldd) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + tx;
        tile[j][tx] = (r < R && c < C) ? src[(long long)r * C + c] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + tx;
        if (c < C && r < R) dst[(long long)c * ldd + r] = (bf16_t)tile[tx][j];
    }
}

__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                         bf16_t* __restrict__ y, float* __restrict__ yf, int R, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)R * C) return;
    const float v = x[i] * s[i / C];
    if (y) y[i] = (bf16_t)v;
    if (yf) yf[i] = v;
}

// One launch for a whole table of small casts (this step's adapter weights -> bf16 GEMM operands, both
// orientations).  grid (n descriptors, 16): block (d, y) strides over descriptor d's elements.
__global__ __launch_bounds__(256) void cast_multi_kernel(const aim_cast_desc* __restrict__ table) {
    const aim_cast_desc d = table[blockIdx.x];
    const float* src = (const float*)d.src;
    bf16_t* dst = (bf16_t*)d.dst;
    const int n = d.R * d.C;                        // (ops.CastTable checks R * C < 2^31)
    if (d.transpose == 0 && (d.C & 3) == 0 && (d.ldd & 3) == 0 && ((unsigned long long)src & 15) == 0 && ((unsigned long long)dst & 7) == 0) {
        // row-major cast, four elements per thread
        const int n4 = n >> 2, c4n = d.C >> 2;
        for (int i = (int)blockIdx.y * 256 + threadIdx.x; i < n4; i += (int)gridDim.y * 256) {
            const int r = i / c4n, c = (i - r * c4n) * 4;
            const f32x4 v = *(const f32x4*)(src + (long long)i * 4);
            *(bf16x4*)(dst + (long long)r * d.ldd + c) = pack4(v[0], v[1], v[2], v[3]);
        }
        return;
    }
    if (d.transpose == 1 && (d.R & 31) == 0 && (d.C & 31) == 0) {
        // transposed cast by 32 x 32 tiles through LDS: coalesced reads along C, coalesced writes along R
        __shared__ float tile[32][33];
        const int tc = d.C >> 5, ntile = (d.R >> 5) * tc;
        const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 8 rows of 32 per pass
        for (int tl = blockIdx.y; tl < ntile; tl += gridDim.y) {
            const int r0 = (tl / tc) * 32, c0 = (tl - (tl / tc) * tc) * 32;
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[ty + k * 8][tx] = src[(long long)(r0 + ty + k * 8) * d.C + c0 + tx];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[(long long)(c0 + ty + k * 8) * d.ldd + r0 + tx] = (bf16_t)tile[tx][ty + k * 8];
            __syncthreads();
        }
        return;
    }
    // (r, c) advance incrementally: no division per element
    const int step = (int)gridDim.y * 256, dr = step / d.C, dc = step - dr * d.C;
    int i = (int)blockIdx.y * 256 + threadIdx.x;
    int r = i / d.C, c = i - r * d.C;
    for (; i < n; i += step) {
        const float v = src[i];
        if (d.transpose == 2) ((float*)d.dst)[(long long)r * d.ldd + c] = v;       // fp32 copy (bias staging)
        else if (d.transpose) dst[(long long)c * d.ldd + r] = (bf16_t)v;
        else dst[(long long)r * d.ldd + c] = (bf16_t)v;
        r += dr;
        c += dc;
        if (c >= d.C) {
            c -= d.C;
            ++r;
        }
    }
}

// AdamW (decoupled weight decay) on flat fp32 buffers, torch.optim.AdamW semantics.
// One element's update.  The four-wide body and the n % 4 tail both run THIS function, with its three fused multiply-adds
// spelled out and no other contraction allowed: the compiler contracts the two loops differently when left to choose, and an
// element's result must not depend on where it sits in the flat buffer.  c = 1 - lr wd (one fma), a = lr / bc1.
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float c, float a, float b1, float omb1,
                                           float b2, float omb2, float bc2s, float eps) {
#pragma clang fp contract(off)
    m = __builtin_fmaf(omb1, g, b1 * m);
    v = __builtin_fmaf(b2, v, omb2 * g * g);
    p = __builtin_fmaf(c, p, -(a * m / (sqrtf(v) / bc2s + eps)));
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long long n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2s, float gs) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float c = __builtin_fmaf(-lr, wd, 1.0f), a = lr / bc1, omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    if (i + 3 < n) {
        f32x4 pp = *(f32x4*)(p + i), mm = *(f32x4*)(m + i), vv = *(f32x4*)(v + i);
        const f32x4 gg = *(const f32x4*)(g + i) * gs;       // gs = 1 / world: the SUM all-reduce becomes the mean here
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], me = mm[e], ve = vv[e];
            adamw_elem(pe, gg[e], me, ve, c, a, b1, omb1, b2, omb2, bc2s, eps);
            pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        *(f32x4*)(p + i) = pp;
        *(f32x4*)(m + i) = mm;
        *(f32x4*)(v + i) = vv;
    } else {
        for (long long j = i; j < n; ++j) {
            float pp = p[j], mm = m[j], vv = v[j];
            adamw_elem(pp, g[j] * gs, mm, vv, c, a, b1, omb1, b2, omb2, bc2s, eps);
            p[j] = pp; m[j] = mm; v[j] = vv;
        }
    }
}

}  // namespace

extern "C" int aim_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream) {
    AIM_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adamw: bad arguments");
    AIM_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0,
                  "adamw: p, g, m and v must be 16-byte aligned");
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2s = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       (long long)n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale);
    AIM_CHECK_LAUNCH("aim_adamw_flat");
    return 0;
}

// BLENDABLE = false: bf16 clips, which no blend entry point accepts (no BLEND instantiation for them)
template <typename TIN, typename TOUT, bool BLENDABLE = true>
static void patchify_launch(dim3 grid, hipStream_t st, const void* imgs, const float* mean3, const float* std3, void* A, int B,
                            int T, int H, int W, int p, int Kp, const AimBlend* blend) {
    if constexpr (BLENDABLE) {
        if (blend) {
            hipLaunchKernelGGL((patchify_kernel<TIN, TOUT, true>), grid, dim3(256), 0, st, (const TIN*)imgs, mean3, std3, (TOUT*)A,
                               B, T, H, W, p, Kp, *blend);
            return;
        }
    }
    hipLaunchKernelGGL((patchify_kernel<TIN, TOUT, false>), grid, dim3(256), 0, st, (const TIN*)imgs, mean3, std3, (TOUT*)A, B, T,
                       H, W, p, Kp, AimBlend{});
}

// The one launcher behind aim_patchify, aim_patchify_blend and (fp32.hip) aim_patchify_f32, aim_patchify_blend_f32, which have
// checked the shape and the pointers.  who: the prefix of the entry point's messages.  Returns -1, with no error set, when
// there is no gather for in_dtype with this output type and blend: the entry point words that refusal itself.
int aim_patchify_launch(const char* who, bool f32_out, const void* imgs, int in_dtype, const float* mean3, const float* std3,
                        void* A, int B, int T, int H, int W, int p, int Kp, const AimBlend* blend, hipStream_t st) {
    if (blend) {
        AIM_CHECK_ARG(blend->partner, "%s: partner is NULL", who);
        AIM_CHECK_ARG(blend->mode == 1 || blend->mode == 2, "%s: mode must be 1 (mixup) or 2 (cutmix), got %d", who, blend->mode);
        AIM_CHECK_ARG(blend->mode == 1 || (0 <= blend->x1 && blend->x1 <= blend->x2 && blend->x2 <= W && 0 <= blend->y1 &&
                                           blend->y1 <= blend->y2 && blend->y2 <= H),
                      "%s: box x [%d, %d) y [%d, %d) outside the %d x %d image", who, blend->x1, blend->x2, blend->y1, blend->y2, W, H);
    }
    decltype(&patchify_launch<float, float>) launch = nullptr;
    if (in_dtype == 0)
        launch = f32_out ? patchify_launch<float, float> : patchify_launch<float, bf16_t>;
    else if (in_dtype == 1)
        launch = f32_out ? patchify_launch<uint8_t, float> : patchify_launch<uint8_t, bf16_t>;
    else if (in_dtype == 2 && !f32_out && !blend)
        launch = patchify_launch<bf16_t, bf16_t, false>;
    if (!launch) return -1;
    const long long total = (long long)B * T * (H / p) * (W / p) * (Kp / (f32_out ? 4 : 8));      // a thread per 16 bytes of A
    launch(dim3((unsigned)((total + 255) / 256)), st, imgs, mean3, std3, A, B, T, H, W, p, Kp, blend);
    char name[40];
    snprintf(name, sizeof name, "aim_%s", who);
    AIM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int aim_patchify(const void* imgs, int in_dtype, const float* mean3, const float* std3, aim_bf16* A, int B,
                            int T, int H, int W, int p, int Kp, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && p > 0 && H % p == 0 && W % p == 0, "patchify: bad shape H=%d W=%d p=%d", H, W, p);
    AIM_CHECK_ARG(Kp >= 3 * p * p && (Kp % 8) == 0, "patchify: Kp=%d must be >= 3*p*p and a multiple of 8", Kp);
    AIM_CHECK_ARG(imgs && A && ((!mean3) == (!std3)), "patchify: null pointer");
    const int rc = aim_patchify_launch("patchify", false, imgs, in_dtype, mean3, std3, A, B, T, H, W, p, Kp, nullptr, (hipStream_t)stream);
    AIM_CHECK_ARG(rc >= 0, "patchify: in_dtype must be 0 (f32), 1 (uint8) or 2 (bf16), got %d", in_dtype);
    return rc;
}

extern "C" int aim_embed_ln(const aim_bf16* tok, const float* cls, const float* pos, const float* temporal,
                            const float* gamma, const float* beta, float* x, float* mean, float* rstd, int B, int T,
                            int N, int D, float eps, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && N > 1 && D > 0 && (D % 4) == 0 && D <= MAXC * 256, "embed_ln: bad shape N=%d D=%d", N, D);
    AIM_CHECK_ARG(tok && cls && pos && temporal && gamma && beta && x && mean && rstd, "embed_ln: null pointer");
    const long long rows = (long long)B * T * N;
    nc_dispatch(D, [&](auto nc) {
        hipLaunchKernelGGL(embed_ln_kernel<decltype(nc)::value>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)tok, cls, pos, temporal, gamma, beta, x, mean, rstd, B, T, N, D, eps);
    });
    AIM_CHECK_LAUNCH("aim_embed_ln");
    return 0;
}

extern "C" int aim_embed_bwd(const void* dx, int dx_is_bf16, const aim_bf16* tok, const float* cls, const float* pos,
                             const float* temporal, const float* gamma, const float* mean, const float* rstd,
                             float* dtemporal, int B, int T, int N, int D, float* workspace, int64_t workspace_bytes,
                             void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && N > 1 && D > 0 && (D % 4) == 0 && D <= MAXC * 256, "embed_bwd: bad shape N=%d D=%d", N, D);
    AIM_CHECK_ARG(dx && tok && cls && pos && temporal && gamma && mean && rstd && dtemporal, "embed_bwd: null pointer");
    int chunks = (B * N + 3) / 4;
    const int want = (2048 + T - 1) / T;
    if (chunks > want) chunks = want;
    // with scratch ([T][chunks][D] fp32, aim_embed_bwd_workspace_bytes) the reduction is two-stage and bitwise reproducible
    float* partial = (workspace && workspace_bytes >= (int64_t)T * chunks * D * 4) ? workspace : nullptr;
    nc_dispatch(D, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        if (dx_is_bf16)
            hipLaunchKernelGGL((embed_bwd_kernel<NC, bf16_t>), dim3(T, chunks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dx,
                               (const bf16_t*)tok, cls, pos, temporal, gamma, mean, rstd, dtemporal, partial, B, T, N, D);
        else
            hipLaunchKernelGGL((embed_bwd_kernel<NC, float>), dim3(T, chunks), dim3(256), 0, (hipStream_t)stream, (const float*)dx,
                               (const bf16_t*)tok, cls, pos, temporal, gamma, mean, rstd, dtemporal, partial, B, T, N, D);
    });
    AIM_CHECK_LAUNCH("aim_embed_bwd");
    if (partial) {
        hipLaunchKernelGGL(embed_bwd_finish_kernel, dim3(T, (D + 63) / 64), dim3(256), 0, (hipStream_t)stream, partial, dtemporal,
                           chunks, D);
        AIM_CHECK_LAUNCH("aim_embed_bwd(finish)");
    }
    return 0;
}

extern "C" int64_t aim_embed_bwd_workspace_bytes(int B, int T, int N, int D) {
    int chunks = (B * N + 3) / 4;
    const int want = (2048 + T - 1) / T;
    if (chunks > want) chunks = want;
    return (int64_t)T * chunks * D * 4;
}

extern "C" int aim_frame_sum(const void* x, int x_is_bf16, const float* w, float* out, int frames, int ntok, int D, void* stream) {
    AIM_CHECK_ARG(frames > 0 && ntok > 0 && D > 0 && (D % 4) == 0 && x && out, "frame_sum: bad arguments");
    if (x_is_bf16)
        hipLaunchKernelGGL(frame_sum_kernel<bf16_t>, dim3(frames, (D / 4 + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, w, out, ntok, D);
    else
        hipLaunchKernelGGL(frame_sum_kernel<float>, dim3(frames, (D / 4 + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                           (const float*)x, w, out, ntok, D);
    AIM_CHECK_LAUNCH("aim_frame_sum");
    return 0;
}

extern "C" int aim_colsum_bf16(const aim_bf16* X, int ldx, const float* af, const float* at, int ntok, float* out,
                               int M, int C, float* workspace, int64_t workspace_bytes, void* stream) {
    AIM_CHECK_ARG(M > 0 && C > 0 && X && out, "colsum: bad arguments");
    if (af || at) AIM_CHECK_ARG(ntok > 0, "colsum: ntok required with row factors");
    if ((C % 8) == 0 && C <= 2048 && (ldx % 8) == 0) {
        int rpb8 = (M + 1023) / 1024;        // <= 1024 row blocks
        if (rpb8 < 64) rpb8 = 64;
        int P = (M + rpb8 - 1) / rpb8;
        // two-stage (partials + finish, fixed summation order) when the caller provides scratch; without scratch a small
        // problem runs as ONE block (the only writer of each column) and a large one falls back to one atomic per
        // column per block
        float* partial = (workspace && workspace_bytes >= (int64_t)P * C * 4 && P > 1) ? workspace : nullptr;
        if (!partial && M <= 2048) {
            rpb8 = M;
            P = 1;
        }
        hipLaunchKernelGGL(colsum8_kernel, dim3(1, P), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, ldx, af, at,
                           ntok, out, partial, M, C, rpb8);
        AIM_CHECK_LAUNCH("aim_colsum_bf16");
        if (partial) {
            hipLaunchKernelGGL(colsum_finish_kernel, dim3((C + 63) / 64), dim3(1024), 0, (hipStream_t)stream, partial, out, P, C);
            AIM_CHECK_LAUNCH("aim_colsum_bf16(finish)");
        }
        return 0;
    }
    int rpb = (M + 511) / 512;
    if (rpb < 64) rpb = 64;
    hipLaunchKernelGGL(colsum_kernel, dim3((C + 255) / 256, (M + rpb - 1) / rpb), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)X, ldx, af, at, ntok, out, M, C, rpb);
    AIM_CHECK_LAUNCH("aim_colsum_bf16");
    return 0;
}

extern "C" int aim_cast_bf16(const float* src, aim_bf16* dst, int R, int C, int transpose, int ldd, void* stream) {
    AIM_CHECK_ARG(R > 0 && C > 0 && src && dst, "cast: bad arguments");
    AIM_CHECK_ARG(ldd == 0 || ldd >= (transpose ? R : C), "cast: ldd=%d smaller than the destination row", ldd);
    hipStream_t st = (hipStream_t)stream;
    if (transpose) {
        hipLaunchKernelGGL(cast_transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, st, src, (bf16_t*)dst, R, C,
                           ldd ? ldd : R);
    } else if (ldd && ldd != C) {
        const long long n = (long long)R * C;
        hipLaunchKernelGGL(cast_strided_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, (bf16_t*)dst, R, C, ldd);
    } else {
        const long long n = (long long)R * C;
        hipLaunchKernelGGL(cast_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, src, (bf16_t*)dst, n);
    }
    AIM_CHECK_LAUNCH("aim_cast_bf16");
    return 0;
}

extern "C" int aim_cast_multi(const aim_cast_desc* table_dev, int n, void* stream) {
    AIM_CHECK_ARG(table_dev && n > 0, "cast_multi: bad arguments");
    hipLaunchKernelGGL(cast_multi_kernel, dim3(n, 16), dim3(256), 0, (hipStream_t)stream, table_dev);
    AIM_CHECK_LAUNCH("aim_cast_multi");
    return 0;
}

// dst[r * dst_row_stride + c] += src[r * C + c]: the class rows' share of a gradient, produced on the side stream,
// folded into the token-major bf16 tensor on the main one
__global__ __launch_bounds__(256) void add_rows_kernel(bf16_t* __restrict__ dst, long long dst_row_stride,
                                                       const float* __restrict__ src, int R, int C) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (long long)R * C) return;
    const int r = (int)(i / C), c = (int)(i - (long long)r * C);
    bf16x4* d = (bf16x4*)(dst + r * dst_row_stride + c);
    const f32x4 a = *(const f32x4*)(src + i);
    const bf16x4 o = *d;
    *d = pack4((float)o[0] + a[0], (float)o[1] + a[1], (float)o[2] + a[2], (float)o[3] + a[3]);
}

extern "C" int aim_add_rows_bf16(aim_bf16* dst, int64_t dst_row_stride, const float* src, int R, int C, void* stream) {
    AIM_CHECK_ARG(R > 0 && C > 0 && (C % 4) == 0 && (dst_row_stride % 4) == 0 && dst && src, "add_rows: bad arguments");
    const long long n = (long long)R * C / 4;
    hipLaunchKernelGGL(add_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)dst,
                       (long long)dst_row_stride, src, R, C);
    AIM_CHECK_LAUNCH("aim_add_rows_bf16");
    return 0;
}

extern "C" int aim_scale_rows(const float* x, const float* s, aim_bf16* y, float* y_f32, int R, int C, void* stream) {
    AIM_CHECK_ARG(R > 0 && C > 0 && x && s && (y || y_f32), "scale_rows: bad arguments");
    const long long n = (long long)R * C;
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, s,
                       (bf16_t*)y, y_f32, R, C);
    AIM_CHECK_LAUNCH("aim_scale_rows");
    return 0;
}

extern "C" int aim_patchify_blend(const void* imgs, int in_dtype, const float* mean3, const float* std3, aim_bf16* A, int B,
                                  int T, int H, int W, int p, int Kp, const int* partner, int mode, float lam, float oml,
                                  int x1, int y1, int x2, int y2, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && p > 0 && H % p == 0 && W % p == 0, "patchify_blend: bad shape H=%d W=%d p=%d", H, W, p);
    AIM_CHECK_ARG(Kp >= 3 * p * p && (Kp % 8) == 0, "patchify_blend: Kp=%d must be >= 3*p*p and a multiple of 8", Kp);
    AIM_CHECK_ARG(imgs && A && ((!mean3) == (!std3)), "patchify_blend: null pointer");
    const AimBlend bl{partner, mode, lam, oml, x1, y1, x2, y2};
    const int rc = aim_patchify_launch("patchify_blend", false, imgs, in_dtype, mean3, std3, A, B, T, H, W, p, Kp, &bl, (hipStream_t)stream);
    AIM_CHECK_ARG(rc >= 0, "patchify_blend: in_dtype must be 0 (f32) or 1 (uint8), got %d", in_dtype);
    return rc;
}
