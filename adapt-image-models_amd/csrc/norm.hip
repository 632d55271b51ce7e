// LayerNorm forward / backward (fp32 statistics) for the AIM block.  gfx950 only.
//
// Replaces reference vit_clip.py:71-77 (`LayerNorm.forward`: fp32 nn.LayerNorm, eps 1e-5) at its
// call sites ln_1 (:224,264,265), ln_2 (:285), ln_pre (:447), ln_post (:452).
// One 64-lane wave per row, 4 rows per 256-thread block; the row lives in registers (float4 chunks),
// two-pass mean / variance, wavefront shuffles for the reductions; HBM-bound by design:
// fwd moves 4 B (x) + 2 B (bf16 y) per element.
#include "aim_common.h"
#include "aim_kernels_internal.h"
#include "ln_row.h"

namespace {
using namespace ln_row;

constexpr int MAXC = 8;  // float4 chunks per lane: D <= 8*4*64 = 2048 (template NC = chunks actually used)

// (TX: an fp32 or a bf16 row, read through load4f: the fp8 inference path keeps its residual stream in bf16)
template <int NC, typename TX = float>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const TX* __restrict__ x, long long ldx,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     bf16_t* __restrict__ yb, float* __restrict__ yf, long long ldy,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     int rows, int D, float eps, unsigned char* __restrict__ y8 = nullptr) {
    const int lane = threadIdx.x & 63;
    const int row = (int)AIM_REV_BLOCK * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = D >> 2;
    const TX* xr = x + (long long)row * ldx;
    f32x4 v[NC];
    float s = 0.f, q = 0.f;
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
        v[c] = load4f(xr + ch * 4);
        s += sum4(v[c]);
    }
    const float mu = row_mean(s, D);
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) q = add_sqdev4(q, v[c], mu);
    const float rs = row_rstd(q, D, eps);
    if (lane == 0) {
        if (mean) mean[row] = mu;
        if (rstd) rstd[row] = rs;
    }
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
        const f32x4 y = ln_affine4(v[c], mu, rs, *(const f32x4*)(gamma + ch * 4), *(const f32x4*)(beta + ch * 4));
        if (yb) store4(yb + (long long)row * ldy + ch * 4, y);
        if (yf) store4(yf + (long long)row * ldy + ch * 4, y);
        if (y8) *(unsigned*)(y8 + (long long)row * ldy + ch * 4) = pack4_fp8(y[0], y[1], y[2], y[3]);
    }
}

// dx = dres + rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = dy * gamma
template <int NC, typename TDY, typename TDR>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const TDY* __restrict__ dy, long long lddy,
                                                     const float* __restrict__ x, long long ldx,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const TDR* __restrict__ dres,
                                                     long long lddres, float* __restrict__ dx, bf16_t* __restrict__ dxb,
                                                     long long lddx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                     int rows, int D) {
    const int lane = threadIdx.x & 63;
    const int row = (int)AIM_REV_BLOCK * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = D >> 2;
    const float mu = mean[row], rs = rstd[row];
    f32x4 g[NC], xh[NC];
    float s1 = 0.f, s2 = 0.f;
    // ln_bwd_chunk's arithmetic written out (ln_bwd_fsum_kernel calls it; dx_eq_layernorm_bwd holds the two to the same bits):
    // through the helper the operands of s1's add come out in the other order and <1, float, .> needs 26 / 28 VGPRs for 24 / 26
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
        const f32x4 d = load4f(dy + (long long)row * lddy + ch * 4);
        const f32x4 xv = *(const f32x4*)(x + (long long)row * ldx + ch * 4);
        const f32x4 gm = *(const f32x4*)(gamma + ch * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xh[c][e] = (xv[e] - mu) * rs;
            g[c][e] = d[e] * gm[e];
            s1 += g[c][e];
            s2 = __builtin_fmaf(g[c][e], xh[c][e], s2);
        }
        if (dgamma) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                atomicAdd(dgamma + ch * 4 + e, d[e] * xh[c][e]);
                atomicAdd(dbeta + ch * 4 + e, d[e]);
            }
        }
    }
    const float m1 = row_mean(s1, D), m2 = row_mean(s2, D);
    LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ln_bwd_elem(g[c][e], xh[c][e], m1, m2, rs);
        if (dres) o = ln_add_res(o, load4f(dres + (long long)row * lddres + ch * 4));
        if (dx) store4(dx + (long long)row * lddx + ch * 4, o);
        if (dxb) store4(dxb + (long long)row * lddx + ch * 4, o);
    }
}


// ln_bwd_kernel for bf16 dy / dres / dx that ALSO emits per-frame weighted column sums of the dx it stores:
//   partial[frame][g][c] = sum over the frame's token group g of w[n] * dx_bf16[frame*ntok + n][c].
// The block backward needs sum_n dms1[n] * d(x1)[frame, n, :] for the per-frame S_Adapter vector path; taken here, from the
// values in registers, it replaces a separate pass over the 155 MB tensor (aim_frame_sum) that opened the class-token chain
// on the side stream and ran starved of CUs beside a persistent GEMM.  One workgroup = one (frame, token group); a wave walks
// every fourth row of the group (the per-row arithmetic is ln_bwd_kernel's, bit for bit); the four waves' sums meet in LDS
// in a fixed order, the G groups are summed by aim_frame_sum over the [frames][G][D] partials (fixed order: reproducible).
// launch_bounds (256, 6) + a wave-uniform row index (scalar address arithmetic): left alone the compiler spends 98 VGPRs
// (4 waves per SIMD) and the kernel runs at 4.8 TB/s; now 70 VGPRs, 7 waves per SIMD.
template <int NC>
__global__ __launch_bounds__(256, (NC <= 4 ? 6 : 2)) void ln_bwd_fsum_kernel(const bf16_t* __restrict__ dy, long long lddy,
                                                          const float* __restrict__ x, long long ldx,
                                                          const float* __restrict__ gamma, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const bf16_t* __restrict__ dres,
                                                          bf16_t* __restrict__ dxb, long long lddx, const float* __restrict__ w,
                                                          float* __restrict__ partial, int ntok, int G, int D) {
    __shared__ f32x4 red[4][NC * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform rows: scalar address arithmetic
    const int bid = (int)AIM_REV_BLOCK;
    const int frame = bid / G, g = bid - frame * G;
    const int rg = (ntok + G - 1) / G;
    const int n_end = min(ntok, (g + 1) * rg);
    const int nch = D >> 2;
    f32x4 fs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) fs[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma nounroll
    for (int n = g * rg + wave; n < n_end; n += 4) {
        asm volatile("" ::: "memory");          // one row at a time: no loads of the next row hoisted into this one (registers)
        const long long row = (long long)frame * ntok + n;
        const float mu = mean[row], rs = rstd[row];
        const float wt = w ? w[n] : 1.0f;
        f32x4 gv[NC], xh[NC];
        float s1 = 0.f, s2 = 0.f;
        LN_ROW_CHUNKS(c, ch, NC, lane, nch) {      // (gamma: L1-resident; held across rows it costs 12 VGPRs)
            const f32x4 d = load4f(dy + row * lddy + ch * 4);
            ln_bwd_chunk(*(const f32x4*)(x + row * ldx + ch * 4), d, *(const f32x4*)(gamma + ch * 4), mu, rs, xh[c], gv[c], s1, s2);
        }
        const float m1 = row_mean(s1, D), m2 = row_mean(s2, D);
        LN_ROW_CHUNKS(c, ch, NC, lane, nch) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ln_bwd_elem(gv[c][e], xh[c][e], m1, m2, rs);
            o = ln_add_res(o, load4f(dres + row * lddx + ch * 4));
            const bf16x4 ob = pack4(o[0], o[1], o[2], o[3]);
            *(bf16x4*)(dxb + row * lddx + ch * 4) = ob;
#pragma unroll
            for (int e = 0; e < 4; ++e) fs[c][e] += wt * (float)ob[e];      // the STORED (bf16) value, like a pass over dx
        }
    }
    LN_ROW_CHUNKS(c, ch, NC, lane, NC * 64) red[wave][ch] = fs[c];      // (every chunk: a dead one holds zeros)
    __syncthreads();
    for (int ch = threadIdx.x; ch < nch; ch += 256)
        *(f32x4*)(partial + (long long)bid * D + ch * 4) = (red[0][ch] + red[1][ch]) + (red[2][ch] + red[3][ch]);
}

}  // namespace

// The one launch behind aim_layernorm_fwd, _fwd_fp8 and _fwd_x16, which have checked the shape and the pointers and differ in
// the row type and in which of the outputs they leave null.  name: the entry point, for the launch error's message.
template <typename TX>
static int ln_fwd_launch(const char* name, const TX* x, int64_t ldx, const float* gamma, const float* beta, bf16_t* y_bf16,
                         float* y_f32, uint8_t* y_fp8, int64_t ldy, float* mean, float* rstd, int rows, int D, float eps,
                         void* stream) {
    nc_dispatch(D, [&](auto nc) {
        hipLaunchKernelGGL((ln_fwd_kernel<decltype(nc)::value, TX>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x,
                           (long long)ldx, gamma, beta, y_bf16, y_f32, (long long)ldy, mean, rstd, rows, D, eps, y_fp8);
    });
    AIM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int aim_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta,
                                 aim_bf16* y_bf16, float* y_f32, int64_t ldy, float* mean, float* rstd,
                                 int rows, int D, float eps, void* stream) {
    AIM_CHECK_ARG(rows > 0 && D > 0 && (D % 4) == 0 && D <= MAXC * 256, "layernorm_fwd: bad shape rows=%d D=%d", rows, D);
    AIM_CHECK_ARG(x && gamma && beta && (y_bf16 || y_f32), "layernorm_fwd: null pointer");
    AIM_CHECK_ARG((ldx % 4) == 0 && (ldy % 4) == 0, "layernorm_fwd: strides must be multiples of 4");
    return ln_fwd_launch("aim_layernorm_fwd", x, ldx, gamma, beta, (bf16_t*)y_bf16, y_f32, nullptr, ldy, mean, rstd, rows, D, eps,
                         stream);
}

extern "C" int aim_layernorm_fwd_fp8(const float* x, int64_t ldx, const float* gamma, const float* beta, uint8_t* y_fp8,
                                     int64_t ldy, int rows, int D, float eps, void* stream) {
    AIM_CHECK_ARG(rows > 0 && D > 0 && (D % 4) == 0 && D <= MAXC * 256, "layernorm_fwd_fp8: bad shape rows=%d D=%d", rows, D);
    AIM_CHECK_ARG(x && gamma && beta && y_fp8, "layernorm_fwd_fp8: null pointer");
    AIM_CHECK_ARG((ldx % 4) == 0 && (ldy % 4) == 0, "layernorm_fwd_fp8: strides must be multiples of 4");
    return ln_fwd_launch("aim_layernorm_fwd_fp8", x, ldx, gamma, beta, nullptr, nullptr, y_fp8, ldy, nullptr, nullptr, rows, D,
                         eps, stream);
}

// bf16 rows in (the fp8 inference path's residual stream); y as bf16 and / or f32 and / or fp8
extern "C" int aim_layernorm_fwd_x16(const aim_bf16* x, int64_t ldx, const float* gamma, const float* beta, aim_bf16* y_bf16,
                                     float* y_f32, uint8_t* y_fp8, int64_t ldy, int rows, int D, float eps, void* stream) {
    AIM_CHECK_ARG(rows > 0 && D > 0 && (D % 4) == 0 && D <= MAXC * 256, "layernorm_fwd_x16: bad shape rows=%d D=%d", rows, D);
    AIM_CHECK_ARG(x && gamma && beta && (y_bf16 || y_f32 || y_fp8), "layernorm_fwd_x16: null pointer");
    AIM_CHECK_ARG((ldx % 4) == 0 && (ldy % 4) == 0, "layernorm_fwd_x16: strides must be multiples of 4");
    return ln_fwd_launch("aim_layernorm_fwd_x16", (const bf16_t*)x, ldx, gamma, beta, (bf16_t*)y_bf16, y_f32, y_fp8, ldy, nullptr,
                         nullptr, rows, D, eps, stream);
}

namespace {
// dgamma[c] += sum_r dy[r][c] * xhat[r][c], dbeta[c] += sum_r dy[r][c] in a fixed order (bitwise reproducible).  The path trains ln_post only (B*T rows), so the walk is short; beyond AIM_LN_DPARAM_ROWS rows the
// main kernel's per-element atomics are used instead.
// (256 threads = 64 columns x 4 row groups, a thread walks rows g, g+4, ... with the loads of four rows in flight, the groups
//  meet in LDS in a fixed order: the first version walked all rows in one thread, one dependent row at a time -- 146 us for
//  512 rows of ln_post.)
template <typename TDY>
__global__ __launch_bounds__(256) void ln_dparam_kernel(const TDY* __restrict__ dy, long long lddy, const float* __restrict__ x,
                                                       long long ldx, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta, int rows, int D) {
    __shared__ float red[2][4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const bool live = c < D;
    const int cc = live ? c : 0;
    float ag = 0.f, ab = 0.f;
    int r = g;
    for (; r + 12 < rows; r += 16) {
        float d[4], xv[4], mu[4], rs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rr = r + 4 * u;
            d[u] = (float)dy[(long long)rr * lddy + cc];
            xv[u] = x[(long long)rr * ldx + cc];
            mu[u] = mean[rr];
            rs[u] = rstd[rr];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ag += d[u] * ((xv[u] - mu[u]) * rs[u]);
            ab += d[u];
        }
    }
    for (; r < rows; r += 4) {
        const float d = (float)dy[(long long)r * lddy + cc];
        ag += d * ((x[(long long)r * ldx + cc] - mean[r]) * rstd[r]);
        ab += d;
    }
    red[0][g][cl] = ag;
    red[1][g][cl] = ab;
    __syncthreads();
    if (g == 0 && live) {
        dgamma[c] += (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
        dbeta[c] += (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
    }
}
constexpr int AIM_LN_DPARAM_ROWS = 8192;
}  // namespace

extern "C" int aim_layernorm_bwd(const void* dy, int dy_is_bf16, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                                 const float* mean, const float* rstd, const void* dres, int dres_is_bf16, int64_t lddres,
                                 float* dx, aim_bf16* dx_bf16, int64_t lddx, float* dgamma, float* dbeta, int rows, int D,
                                 void* stream) {
    AIM_CHECK_ARG(rows > 0 && D > 0 && (D % 4) == 0 && D <= MAXC * 256, "layernorm_bwd: bad shape rows=%d D=%d", rows, D);
    AIM_CHECK_ARG(dy && x && gamma && mean && rstd && (dx || dx_bf16), "layernorm_bwd: null pointer");
    AIM_CHECK_ARG((!dgamma) == (!dbeta), "layernorm_bwd: dgamma and dbeta go together");
    AIM_CHECK_ARG((ldx % 4) == 0 && (lddy % 4) == 0 && (lddx % 4) == 0 && (!dres || (lddres % 4) == 0),
                  "layernorm_bwd: strides must be multiples of 4");
    if (dgamma && rows <= AIM_LN_DPARAM_ROWS) {      // parameter gradients apart, in a fixed order
        if (dy_is_bf16)
            hipLaunchKernelGGL(ln_dparam_kernel<bf16_t>, dim3((D + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                               (long long)lddy, x, (long long)ldx, mean, rstd, dgamma, dbeta, rows, D);
        else
            hipLaunchKernelGGL(ln_dparam_kernel<float>, dim3((D + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const float*)dy,
                               (long long)lddy, x, (long long)ldx, mean, rstd, dgamma, dbeta, rows, D);
        AIM_CHECK_LAUNCH("aim_layernorm_bwd(dparam)");
        dgamma = nullptr;
        dbeta = nullptr;
    }
    nc_dispatch(D, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
#define AIM_LN_BWD_T(TDY, TDR)                                                                                      \
    hipLaunchKernelGGL((ln_bwd_kernel<NC, TDY, TDR>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream,        \
                       (const TDY*)dy, (long long)lddy, x, (long long)ldx, gamma, mean, rstd, (const TDR*)dres,       \
                       (long long)lddres, dx, (bf16_t*)dx_bf16, (long long)lddx, dgamma, dbeta, rows, D)
        if (dy_is_bf16 && dres_is_bf16) AIM_LN_BWD_T(bf16_t, bf16_t);
        else if (dy_is_bf16) AIM_LN_BWD_T(bf16_t, float);
        else if (dres_is_bf16) AIM_LN_BWD_T(float, bf16_t);
        else AIM_LN_BWD_T(float, float);
#undef AIM_LN_BWD_T
    });
    AIM_CHECK_LAUNCH("aim_layernorm_bwd");
    return 0;
}

extern "C" int aim_layernorm_bwd_fsum(const aim_bf16* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                                      const float* mean, const float* rstd, const aim_bf16* dres, aim_bf16* dx_bf16,
                                      int64_t lddx, const float* w, float* fsum_partial, int groups, int frames, int ntok,
                                      int D, void* stream) {
    AIM_CHECK_ARG(frames > 0 && ntok > 0 && groups > 0 && D > 0 && (D % 4) == 0 && D <= 8 * 256,
                  "layernorm_bwd_fsum: bad shape frames=%d ntok=%d groups=%d D=%d", frames, ntok, groups, D);
    AIM_CHECK_ARG(dy && x && gamma && mean && rstd && dres && dx_bf16 && fsum_partial, "layernorm_bwd_fsum: null pointer");
    AIM_CHECK_ARG((ldx % 4) == 0 && (lddy % 4) == 0 && (lddx % 4) == 0, "layernorm_bwd_fsum: strides must be multiples of 4");
    nc_dispatch(D, [&](auto nc) {
        hipLaunchKernelGGL(ln_bwd_fsum_kernel<decltype(nc)::value>, dim3(frames * groups), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)dy, (long long)lddy, x, (long long)ldx, gamma, mean, rstd, (const bf16_t*)dres,
                           (bf16_t*)dx_bf16, (long long)lddx, w, fsum_partial, ntok, groups, D);
    });
    AIM_CHECK_LAUNCH("aim_layernorm_bwd_fsum");
    return 0;
}
