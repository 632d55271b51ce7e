// ViT_ImageNet embedding (no ln_pre) and the reproducible LayerNorm gamma / beta gradients of the full-parameter backward.
// gfx950 only.
//
// embed_nopre_fwd: reference vit_imagenet.py:241-251 -- patch tokens (conv + bias, computed by the caller's GEMM in fp32),
//   cls_token concat, + pos_embed, + temporal_embedding, in the reference's order of additions; no LayerNorm.
// embed_nopre_bwd: d cls_token, d pos_embed, d temporal_embedding, the conv bias gradient and the token rows of d(x) (the
//   conv weight gradient's operand).  Every sum runs in one fixed order (per-frame and per-token column sums first, then the
//   finish pass): no atomics, bitwise reproducible.
// layernorm_gb_bwd: dgamma += sum_m dy[m] * xhat[m], dbeta += sum_m dy[m] over any number of rows, two-stage (row-chunk
//   partial slabs, then an ordered sum over the slabs).
#include "aim_common.h"
#include "aim_kernels_internal.h"
#include "ln_row.h"

namespace {

// x[(bt*N + n)][d] = ((n == 0 ? cls[d] : tok[bt*(N-1) + n-1][d]) + pos[n][d]) + temporal[t][d]; one thread per 4 columns
__global__ __launch_bounds__(256) void embed_nopre_fwd_kernel(const float* __restrict__ tok, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, const float* __restrict__ temporal,
                                                              float* __restrict__ x, int BT, int T, int N, int D) {
    const int c4 = D / 4;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)BT * N * c4) return;
    const long long row = idx / c4;
    const int d = (int)(idx - row * c4) * 4;
    const int n = (int)(row % N);
    const long long bt = row / N;
    const int t = (int)(bt % T);
    const f32x4 a = n == 0 ? *(const f32x4*)(cls + d) : *(const f32x4*)(tok + (bt * (N - 1) + n - 1) * D + d);
    const f32x4 p = *(const f32x4*)(pos + (long long)n * D + d);
    const f32x4 e = *(const f32x4*)(temporal + (long long)t * D + d);
    *(f32x4*)(x + row * D + d) = (a + p) + e;
}

// per frame f: fsum[f][d] = sum_n dx[f*N + n][d] (n ascending); dtok[f*(N-1) + n-1] = dx[f*N + n] for n >= 1
template <typename T>
__global__ __launch_bounds__(256) void embed_nopre_frames_kernel(const T* __restrict__ dx, T* __restrict__ dtok,
                                                                 float* __restrict__ fsum, int N, int D) {
    const int f = blockIdx.x;
    const int d = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (d >= D) return;
    const T* src = dx + (long long)f * N * D + d;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; ++n) {
        acc += load4f(src + (long long)n * D);
        if (dtok && n > 0) {
            if constexpr (sizeof(T) == 4)
                *(f32x4*)(dtok + ((long long)f * (N - 1) + n - 1) * D + d) = *(const f32x4*)(src + (long long)n * D);
            else
                *(bf16x4*)(dtok + ((long long)f * (N - 1) + n - 1) * D + d) = *(const bf16x4*)(src + (long long)n * D);
        }
    }
    *(f32x4*)(fsum + (long long)f * D + d) = acc;
}

// per token n: psum[n][d] = sum_f dx[f*N + n][d] (f ascending); dpos[n][d] += psum[n][d]
template <typename T>
__global__ __launch_bounds__(256) void embed_nopre_tokens_kernel(const T* __restrict__ dx, float* __restrict__ psum,
                                                                 float* __restrict__ dpos, int BT, int N, int D) {
    const int n = blockIdx.x;
    const int d = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (d >= D) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < BT; ++f) acc += load4f(dx + ((long long)f * N + n) * D + d);
    *(f32x4*)(psum + (long long)n * D + d) = acc;
    if (dpos) *(f32x4*)(dpos + (long long)n * D + d) += acc;
}

// dcls[d] += psum[0][d]; dbias[d] += sum_{n >= 1} psum[n][d]; dtemporal[t][d] += sum_b fsum[b*T + t][d]
__global__ __launch_bounds__(256) void embed_nopre_finish_kernel(const float* __restrict__ fsum, const float* __restrict__ psum,
                                                                 float* __restrict__ dcls, float* __restrict__ dbias,
                                                                 float* __restrict__ dtemporal, int B, int T, int N, int D) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    if (dcls) dcls[d] += psum[d];
    if (dbias) {
        float s = 0.f;
        for (int n = 1; n < N; ++n) s += psum[(long long)n * D + d];
        dbias[d] += s;
    }
    if (dtemporal) {
        for (int t = 0; t < T; ++t) {
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += fsum[((long long)b * T + t) * D + d];
            dtemporal[(long long)t * D + d] += s;
        }
    }
}

// rows per partial slab of layernorm_gb_bwd: at least 16, and at most 1 024 slabs (ViT-B/16 at 8 clips: 788 slabs of 16 rows, enough
// workgroups to cover the chip; at 64 clips 1 019 slabs of 99 rows)
__host__ __device__ __forceinline__ int gb_rows_per_slab(int rows) {
    const int r = (rows + 1023) / 1024;
    return r < 16 ? 16 : r;
}

// slab p: part[p][d] = sum_m dy[m][d] * (x[m][d] - mean[m]) * rstd[m], part[P + p][d] = sum_m dy[m][d]  (m ascending)
template <typename T>
__global__ __launch_bounds__(256) void ln_gb_partial_kernel(const T* __restrict__ dy, long long lddy, const float* __restrict__ x,
                                                            long long ldx, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, float* __restrict__ part, int rows,
                                                            int rps, int D) {
    const int p = blockIdx.x, P = gridDim.x;
    const int d = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (d >= D) return;
    const int m0 = p * rps, m1 = min(rows, m0 + rps);
    f32x4 ag = {0.f, 0.f, 0.f, 0.f}, ab = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int m = m0; m < m1; ++m) {
        const f32x4 g = load4f(dy + (long long)m * lddy + d);
        const f32x4 xv = *(const f32x4*)(x + (long long)m * ldx + d);
        const float mu = mean[m], rs = rstd[m];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ag[e] = fmaf(g[e], (xv[e] - mu) * rs, ag[e]);
            ab[e] += g[e];
        }
    }
    *(f32x4*)(part + (long long)p * D + d) = ag;
    *(f32x4*)(part + ((long long)P + p) * D + d) = ab;
}

// 64 columns per workgroup, 16 slab slots of 64 lanes: slot s sums slabs s, s + 16, ... in order, then lane c adds the 16 slots
// in order (fixed summation order: bitwise reproducible)
__global__ __launch_bounds__(1024) void ln_gb_finish_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int P, int D) {
    __shared__ float red[2][1024];
    const int lane = threadIdx.x & 63, slot = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float sg = 0.f, sb = 0.f;
    if (c < D) {
        for (int p = slot; p < P; p += 16) {
            sg += part[(long long)p * D + c];
            sb += part[((long long)P + p) * D + c];
        }
    }
    red[0][threadIdx.x] = sg;
    red[1][threadIdx.x] = sb;
    __syncthreads();
    if (slot == 0 && c < D) {
        float tg = 0.f, tb = 0.f;
        for (int s2 = 0; s2 < 16; ++s2) {
            tg += red[0][lane + 64 * s2];
            tb += red[1][lane + 64 * s2];
        }
        if (dgamma) dgamma[c] += tg;
        if (dbeta) dbeta[c] += tb;
    }
}

}  // namespace

extern "C" int aim_embed_nopre_fwd(const float* tok, const float* cls, const float* pos, const float* temporal, float* x, int B,
                                   int T, int N, int D, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && N > 1 && D > 0 && (D % 4) == 0 && tok && cls && pos && temporal && x,
                  "embed_nopre_fwd: bad arguments B=%d T=%d N=%d D=%d", B, T, N, D);
    const long long work = (long long)B * T * N * (D / 4);
    hipLaunchKernelGGL(embed_nopre_fwd_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tok, cls,
                       pos, temporal, x, B * T, T, N, D);
    AIM_CHECK_LAUNCH("aim_embed_nopre_fwd");
    return 0;
}

extern "C" int64_t aim_embed_nopre_bwd_workspace_bytes(int B, int T, int N, int D) {
    return ((int64_t)B * T + N) * D * 4;
}

extern "C" int aim_embed_nopre_bwd(const void* dx, int dx_is_bf16, void* dtok, float* dcls, float* dpos, float* dtemporal,
                                   float* dbias, int B, int T, int N, int D, float* workspace, int64_t workspace_bytes,
                                   void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && N > 1 && D > 0 && (D % 4) == 0 && dx, "embed_nopre_bwd: bad arguments B=%d T=%d N=%d D=%d",
                  B, T, N, D);
    AIM_CHECK_ARG(workspace && workspace_bytes >= aim_embed_nopre_bwd_workspace_bytes(B, T, N, D),
                  "embed_nopre_bwd: workspace of %lld bytes needed", (long long)aim_embed_nopre_bwd_workspace_bytes(B, T, N, D));
    hipStream_t st = (hipStream_t)stream;
    const int BT = B * T;
    float* fsum = workspace;
    float* psum = workspace + (long long)BT * D;
    const dim3 cb((D / 4 + 255) / 256);
    if (dx_is_bf16) {
        hipLaunchKernelGGL(embed_nopre_frames_kernel<bf16_t>, dim3(BT, cb.x), dim3(256), 0, st, (const bf16_t*)dx, (bf16_t*)dtok,
                           fsum, N, D);
        AIM_CHECK_LAUNCH("aim_embed_nopre_bwd(frames)");
        hipLaunchKernelGGL(embed_nopre_tokens_kernel<bf16_t>, dim3(N, cb.x), dim3(256), 0, st, (const bf16_t*)dx, psum, dpos, BT,
                           N, D);
    } else {
        hipLaunchKernelGGL(embed_nopre_frames_kernel<float>, dim3(BT, cb.x), dim3(256), 0, st, (const float*)dx, (float*)dtok,
                           fsum, N, D);
        AIM_CHECK_LAUNCH("aim_embed_nopre_bwd(frames)");
        hipLaunchKernelGGL(embed_nopre_tokens_kernel<float>, dim3(N, cb.x), dim3(256), 0, st, (const float*)dx, psum, dpos, BT, N,
                           D);
    }
    AIM_CHECK_LAUNCH("aim_embed_nopre_bwd(tokens)");
    hipLaunchKernelGGL(embed_nopre_finish_kernel, dim3((D + 255) / 256), dim3(256), 0, st, fsum, psum, dcls, dbias, dtemporal, B,
                       T, N, D);
    AIM_CHECK_LAUNCH("aim_embed_nopre_bwd(finish)");
    return 0;
}

extern "C" int64_t aim_layernorm_gb_bwd_workspace_bytes(int rows, int D) {
    if (rows <= 0 || D <= 0) return 0;
    const int rps = gb_rows_per_slab(rows);
    return (int64_t)2 * ((rows + rps - 1) / rps) * D * 4;
}

extern "C" int aim_layernorm_gb_bwd(const void* dy, int dy_is_bf16, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                                    const float* rstd, float* dgamma, float* dbeta, int rows, int D, float* workspace,
                                    int64_t workspace_bytes, void* stream) {
    AIM_CHECK_ARG(rows > 0 && D > 0 && (D % 4) == 0 && dy && x && mean && rstd && (dgamma || dbeta),
                  "layernorm_gb_bwd: bad arguments rows=%d D=%d", rows, D);
    AIM_CHECK_ARG(lddy >= D && ldx >= D && (lddy % 4) == 0 && (ldx % 4) == 0, "layernorm_gb_bwd: row strides must be >= D and "
                  "multiples of 4 (lddy=%lld ldx=%lld)", (long long)lddy, (long long)ldx);
    AIM_CHECK_ARG(workspace && workspace_bytes >= aim_layernorm_gb_bwd_workspace_bytes(rows, D),
                  "layernorm_gb_bwd: workspace of %lld bytes needed", (long long)aim_layernorm_gb_bwd_workspace_bytes(rows, D));
    hipStream_t st = (hipStream_t)stream;
    const int rps = gb_rows_per_slab(rows);
    const int P = (rows + rps - 1) / rps;
    const dim3 grid(P, (D / 4 + 255) / 256);
    if (dy_is_bf16)
        hipLaunchKernelGGL(ln_gb_partial_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)dy, (long long)lddy, x,
                           (long long)ldx, mean, rstd, workspace, rows, rps, D);
    else
        hipLaunchKernelGGL(ln_gb_partial_kernel<float>, grid, dim3(256), 0, st, (const float*)dy, (long long)lddy, x,
                           (long long)ldx, mean, rstd, workspace, rows, rps, D);
    AIM_CHECK_LAUNCH("aim_layernorm_gb_bwd(partial)");
    hipLaunchKernelGGL(ln_gb_finish_kernel, dim3((D + 63) / 64), dim3(1024), 0, st, workspace, dgamma, dbeta, P, D);
    AIM_CHECK_LAUNCH("aim_layernorm_gb_bwd(finish)");
    return 0;
}

namespace {
using namespace ln_row;

// ---- TimeSformer (reference timesformer.py:196-208): the full backward of the fused stem x = ln_pre([cls ; tok] + pos + temporal)
// (aim_embed_ln / aim_embed_ln_f32), for a model whose stem trains ----
// Stage 1, grid (N, T), four waves: the block owns token n of frame-time t and its waves walk the clips b = wave, wave + 4, ...
// One wave per row: u is rebuilt as the forward builds it, xhat = (u - mean) rstd, the two row means come from wave shuffles,
// du = rstd (gamma dx - mean_d(gamma dx) - xhat mean_d(gamma dx xhat)).  du goes to dtok (rows n >= 1) and into three register
// sums: du, dx xhat, dx.  The block adds its four waves in wave order through LDS and writes one row of each to the workspace:
//   S[n][t][D] (du) | Gg[n*T + t][D] (dx xhat) | Gb[n*T + t][D] (dx)      -- 3 N T D floats.
// Stage 2 adds those rows in a fixed order (embed_ln_bwd_finish_kernel, ln_gb_finish_kernel).  No atomics anywhere.
constexpr int EMB_MAXC = 8;  // float4 chunks per lane: D <= 8*4*64 = 2048, what aim_embed_ln takes.  (NC <= 4, D <= 1024, is every model
                             // built here and fits the registers; the bf16 instance at NC = 8 spills 764 of them: correct, not fast)

template <int NC, typename TX>      // TX: the type of dx, tok and dtok (bf16_t | float)
__global__ __launch_bounds__(256) void embed_ln_bwd_rows_kernel(const TX* __restrict__ dx, const TX* __restrict__ tok,
                                                                const float* __restrict__ cls, const float* __restrict__ pos,
                                                                const float* __restrict__ tmp, const float* __restrict__ gamma,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                TX* __restrict__ dtok, float* __restrict__ part, int B, int T,
                                                                int N, int D) {
    __shared__ float red[3][NC * 256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x, t = blockIdx.y, nch = D >> 2;
    f32x4 adu[NC], adg[NC], adb[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) adu[c] = adg[c] = adb[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = wave; b < B; b += 4) {
        const long long bt = (long long)b * T + t, row = bt * N + n;
        const float mu = mean[row], rs = rstd[row];
        f32x4 g[NC], xh[NC];
        float s1 = 0.f, s2 = 0.f;
        // Written out, as in embed_bwd_kernel, not ln_bwd_chunk and ln_bwd_elem: what the compiler contracts here (part of the
        // g xh products into s2) is what the bits of dtok and of the three sums are.
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
                adg[c][e] = fmaf(d[e], xh[c][e], adg[c][e]);
                adb[c][e] += d[e];
            }
        }
        const float m1 = row_mean(s1, D), m2 = row_mean(s2, D);
        LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
            f32x4 du;
#pragma unroll
            for (int e = 0; e < 4; ++e) du[e] = rs * (g[c][e] - m1 - xh[c][e] * m2);
            adu[c] += du;
            if (dtok && n > 0) store4(dtok + (bt * (N - 1) + (n - 1)) * D + ch * 4, du);
        }
    }
    // the four waves' sums meet in LDS and are added in wave order; one quantity at a time (NC = 8: 24 KB of LDS)
    const long long NT = (long long)gridDim.x * gridDim.y, p = (long long)n * T + t;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        f32x4* acc = q == 0 ? adu : (q == 1 ? adg : adb);
        if (q > 0) __syncthreads();
        if (wave > 0) {
            LN_ROW_CHUNKS(c, ch, NC, lane, nch) *(f32x4*)(&red[wave - 1][ch * 4]) = acc[c];
        }
        __syncthreads();
        if (wave == 0) {
            LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
                f32x4 a = acc[c];
                for (int w = 0; w < 3; ++w) a += *(const f32x4*)(&red[w][ch * 4]);
                *(f32x4*)(part + (q * NT + p) * D + ch * 4) = a;
            }
        }
    }
}

// grid ((D + 63) / 64, N + T), 64 columns x 4 row groups.  blockIdx.y = n < N: dpos[n] += sum_t S[n][t] (and dcls += the same sum
// for n = 0: the same additions in the same order, so d(class_embedding)'s increment has the bits of d(positional_embedding)[0]'s);
// blockIdx.y = N + t: dtemporal[t] += sum_n S[n][t].  Group g adds rows g, g + 4, ... in order, then the four groups in order.
__global__ __launch_bounds__(256) void embed_ln_bwd_finish_kernel(const float* __restrict__ S, float* __restrict__ dcls,
                                                                  float* __restrict__ dpos, float* __restrict__ dtemporal, int T,
                                                                  int N, int D) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const bool live = c < D;
    const bool tokens = (int)blockIdx.y < N;                    // (uniform over the block)
    const int n = (int)blockIdx.y, t = (int)blockIdx.y - N;
    if (tokens ? (!dpos && !(dcls && n == 0)) : !dtemporal) return;
    float a = 0.f;
    if (live) {
        if (tokens)
            for (int k = g; k < T; k += 4) a += S[((long long)n * T + k) * D + c];
        else
            for (int k = g; k < N; k += 4) a += S[((long long)k * T + t) * D + c];
    }
    red[g][cl] = a;
    __syncthreads();
    if (g == 0 && live) {
        const float s = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
        if (tokens) {
            if (dpos) dpos[(long long)n * D + c] += s;
            if (dcls && n == 0) dcls[c] += s;
        } else {
            dtemporal[(long long)t * D + c] += s;
        }
    }
}

}  // namespace

extern "C" int64_t aim_embed_ln_bwd_workspace_bytes(int B, int T, int N, int D) {
    if (B <= 0 || T <= 0 || N <= 0 || D <= 0) return 0;
    return (int64_t)3 * N * T * D * 4;
}

extern "C" int aim_embed_ln_bwd(const void* dx, int is_bf16, const void* tok, const float* cls, const float* pos,
                                const float* temporal, const float* gamma, const float* mean, const float* rstd, void* dtok,
                                float* dcls, float* dpos, float* dtemporal, float* dgamma, float* dbeta, int B, int T, int N, int D,
                                float* workspace, int64_t workspace_bytes, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && N > 1 && D > 0 && (D % 4) == 0 && D <= EMB_MAXC * 256 && T <= 65535 &&
                      (long long)N + T <= 65535 && (long long)N * T <= (1 << 24),
                  "embed_ln_bwd: bad shape B=%d T=%d N=%d D=%d (D a multiple of 4, at most %d; N + T at most 65535)", B, T, N, D,
                  EMB_MAXC * 256);
    AIM_CHECK_ARG(dx && tok && cls && pos && temporal && gamma && mean && rstd, "embed_ln_bwd: null input pointer");
    AIM_CHECK_ARG(dtok || dcls || dpos || dtemporal || dgamma || dbeta, "embed_ln_bwd: no output requested");
    // rows are moved four elements at a time: 16 bytes of f32, 8 bytes of bf16
    const uintptr_t am = is_bf16 ? 7 : 15;
    AIM_CHECK_ARG((((uintptr_t)dx | (uintptr_t)tok | (uintptr_t)dtok) & am) == 0 &&
                      (((uintptr_t)cls | (uintptr_t)pos | (uintptr_t)temporal | (uintptr_t)gamma | (uintptr_t)workspace) & 15) == 0 &&
                      (((uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)dcls | (uintptr_t)dpos | (uintptr_t)dtemporal |
                        (uintptr_t)dgamma | (uintptr_t)dbeta) & 3) == 0,
                  "embed_ln_bwd: misaligned pointer (dx / tok / dtok: %d bytes; cls / pos / temporal / gamma / workspace: 16)",
                  (int)am + 1);
    AIM_CHECK_ARG(workspace && workspace_bytes >= aim_embed_ln_bwd_workspace_bytes(B, T, N, D),
                  "embed_ln_bwd: workspace of %lld bytes needed", (long long)aim_embed_ln_bwd_workspace_bytes(B, T, N, D));
    hipStream_t st = (hipStream_t)stream;
    const int P = N * T;
    ln_row::nc_dispatch(D, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        if (is_bf16)
            hipLaunchKernelGGL((embed_ln_bwd_rows_kernel<NC, bf16_t>), dim3(N, T), dim3(256), 0, st, (const bf16_t*)dx,
                               (const bf16_t*)tok, cls, pos, temporal, gamma, mean, rstd, (bf16_t*)dtok, workspace, B, T, N, D);
        else
            hipLaunchKernelGGL((embed_ln_bwd_rows_kernel<NC, float>), dim3(N, T), dim3(256), 0, st, (const float*)dx,
                               (const float*)tok, cls, pos, temporal, gamma, mean, rstd, (float*)dtok, workspace, B, T, N, D);
    });
    AIM_CHECK_LAUNCH("aim_embed_ln_bwd(rows)");
    if (dcls || dpos || dtemporal) {
        hipLaunchKernelGGL(embed_ln_bwd_finish_kernel, dim3((D + 63) / 64, N + T), dim3(256), 0, st, workspace, dcls, dpos,
                           dtemporal, T, N, D);
        AIM_CHECK_LAUNCH("aim_embed_ln_bwd(finish)");
    }
    if (dgamma || dbeta) {      // the slabs [P][D] (dx xhat) and [P][D] (dx) behind S, summed as aim_layernorm_gb_bwd sums its slabs
        hipLaunchKernelGGL(ln_gb_finish_kernel, dim3((D + 63) / 64), dim3(1024), 0, st, workspace + (long long)P * D, dgamma,
                           dbeta, P, D);
        AIM_CHECK_LAUNCH("aim_embed_ln_bwd(gamma, beta)");
    }
    return 0;
}
