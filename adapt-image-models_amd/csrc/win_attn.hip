// Self-attention inside 3-D windows of the patch grid (AIM_FLASH_WIN's temporal branch), forward and backward.  gfx950 only.
//
// Replaces reference vitclip_aim_flash_win.py:146-225 (window_partition -> attn -> window_reverse on the patch tokens).  A
// window of (wt, wh, ww) holds S = wt wh ww tokens (784 at 224/16 and (16,7,7)): too many to keep a whole score row resident
// as attn_fwd.hip does (N <= 288), so K and V stream through LDS in 64-key tiles under an online (max, sum) rescale.
//
// Addressing.  The partition and its inverse are addresses: token i = (dt wh + dh) ww + dw of window (b, it, ih, iw) is row
// (b T + it wt + dt) P + 1 + (ih wh + dh) G + iw ww + dw of the frame-major buffers (P >= N token rows per frame; rows N .. P - 1
// are spare).  The staging of a tile gathers its 64 rows (one buffer_load ... lds per 8 rows; a lane's voffset is its own row,
// so a gather costs what a dense tile costs), the own-side fragments and the stores use the same rule.  The class row and the
// spare rows of a frame are never addressed.
//
// One workgroup = one (window, head, chunk of NW x 16 "own" tokens); wave w owns 16 of them, one per MFMA column / lane
// quartet, exactly the fragment layout of attn_fwd.hip (S^T = K Q^T: streamed token on the MFMA row, own token on the lane;
// O^T = V^T P^T through ds_read_b64_tr_b16 of the row-major image).  Three kernels share that skeleton:
//   fwd : own = queries, streamed = (K, V).  Per tile: s = K q, m' = max(m, max s), alpha = 2^((m - m') c), l = l alpha + sum p,
//         O = O alpha + V^T bf16(p), p = 2^((s - m') c) <= 1.  End: out = bf16(O / l), lse = m / 8 + log l.
//   dq  : own = queries, streamed = (K, V).  delta = dO . out (fp32, also stored for the next kernel), p = 2^(s c - lse log2 e),
//         dS = p (V dO - delta) / 8, dQ^T += K^T bf16(dS).
//   dkv : own = keys, streamed = (Q, dO, lse, delta).  The same p and dS with the roles swapped (query on the MFMA row),
//         dV^T += dO^T bf16(p), dK^T += Q^T bf16(dS).
// A dK/dV pass plus a dQ pass rather than one pass: in one pass either dQ or (dK, dV) is a sum ACROSS workgroups (atomics or a
// [S/64, S, 64] fp32 partial buffer per item and a reduction); with two passes every result row has one writer and a fixed
// summation order (the tile order), each pass holds 32 / 64 accumulator VGPRs and 16 KiB of LDS, and the price is computing
// s and dP twice (5 MFMA products against 3.5 per pass pair: 7 against 5).  Every patch token lies in exactly one window.
//
// The kernels are templates on MODE: WIN_PLAIN is the window partition above, WIN_WRAP the box partition of shifted windows whose
// t windows wrap round the clip (AIM_FLASH's odd blocks; the rule stands above the *_shift entry points at the end of the file),
// WIN_CUT the one in which t is cut like h and w (AIM's odd blocks; above the *_cut entry points).  Only win_item, win_row and
// the early exit of a workgroup past a small box differ.
//
// Tails: streamed rows past S are zero-filled by the buffer bounds check (AIM_OOB) and their probabilities forced to 0; own
// tokens past S load the window's last token and are not stored.
#include <stdio.h>

#include "attn_tile.h"
#include "aim_kernels_internal.h"

namespace {

using namespace attn_tile;

constexpr int WIN_MAX_S = AIM_WIN_ATTN_MAX_S;
constexpr int WIN_PLAIN = 0, WIN_WRAP = 1, WIN_CUT = 2;

struct WinGeom {
    int T, P, G, H;       // P: tokens per frame of the buffers (row stride); the grid's tokens are 1 .. G G
    int wt, wh, ww;       // window extents (after clipping)
    int nh, nw, nW;       // boxes along h and w, boxes per clip (nW = boxes along t * nh * nw)
    int S;                // tokens of a whole window (the largest box)
    int st, sh, sw;       // shifts (the *_shift entries; 0 otherwise)
};

// One sequence: the box [t0, t0 + et) x [h0, h0 + eh) x [w0, w0 + ew) of the grid, S = et eh ew tokens in (dt, dh, dw) row-major
// order.  Unshifted: every box is a window (et = wt, eh = wh, ew = ww, S = g.S).  Shifted: the rule above the *_shift entry
// points (et = wt) or above the *_cut ones.
struct WinItem {
    int b, h, t0, h0, w0;
    int et, eh, ew, S;
};

// segment j of an axis of extent w cut at 0, s, s + w, s + 2 w, ...: its start and its length (s = 0: j w and w)
__device__ __forceinline__ void axis_segment(int j, int w, int s, int G, int* start, int* len) {
    const int a = j ? s + (j - 1) * w : 0;
    const int e = s + j * w < G ? s + j * w : G;
    *start = s ? a : j * w;
    *len = s ? e - a : w;
}

template <int MODE>
__device__ __forceinline__ WinItem win_item(const WinGeom& g, int item) {
    WinItem it;
    it.h = item % g.H;
    const int bw = item / g.H, win = bw % g.nW;
    it.b = bw / g.nW;
    const int iw = win % g.nw, r = win / g.nw, ih = r % g.nh, itt = r / g.nh;
    if (MODE == WIN_PLAIN) {
        it.t0 = itt * g.wt;
        it.h0 = ih * g.wh;
        it.w0 = iw * g.ww;
        it.et = g.wt, it.eh = g.wh, it.ew = g.ww, it.S = g.S;
    } else {
        if (MODE == WIN_WRAP) {
            it.t0 = itt * g.wt + g.st;      // rolled: frames t0 + dt taken modulo T in win_row
            it.et = g.wt;
        } else {
            axis_segment(itt, g.wt, g.st, g.T, &it.t0, &it.et);      // t0 + et <= T: no frame index is taken modulo T
        }
        axis_segment(ih, g.wh, g.sh, g.G, &it.h0, &it.eh);
        axis_segment(iw, g.ww, g.sw, g.G, &it.w0, &it.ew);
        it.S = it.et * it.eh * it.ew;
    }
    return it;
}

// row, within the clip, of token i of the box
template <int MODE>
__device__ __forceinline__ int win_row(const WinGeom& g, const WinItem& it, int i) {
    const int hw = it.eh * it.ew;
    const int dt = i / hw, r = i - dt * hw, dh = r / it.ew, dw = r - dh * it.ew;
    int f = it.t0 + dt;
    if (MODE == WIN_WRAP && f >= g.T) f -= g.T;      // f <= (T - wt + st) + wt - 1 < 2 T: one subtraction is the modulo
    return f * g.P + 1 + (it.h0 + dh) * g.G + it.w0 + dw;
}

// index into the [B T, H, P] statistics of clip row r
__device__ __forceinline__ long long stat_index(const WinGeom& g, const WinItem& it, int r) {
    const int f = r / g.P, n = r - f * g.P;
    return (((long long)it.b * g.T + f) * g.H + it.h) * g.P + n;
}

// gather the 64 streamed tokens i0 .. i0 + 63 of the window into two swizzled 8 KiB images (rows past S: zeros)
template <int MODE>
__device__ __forceinline__ void stage_pair(__amdgpu_buffer_rsrc_t ra, int lda2, AIM_LDS char* ia, __amdgpu_buffer_rsrc_t rb, int ldb2,
                                           AIM_LDS char* ib, const WinGeom& g, const WinItem& it, int i0, int wave, int nwaves,
                                           int lane) {
    const int srow = lane >> 3, schunk = (lane & 7) ^ srow;
    for (int p = wave; p < 8; p += nwaves) {
        const int i = i0 + p * 8 + srow;
        unsigned va = AIM_OOB, vb = AIM_OOB;
        if (i < it.S) {
            const int r = win_row<MODE>(g, it, i);
            va = (unsigned)(r * lda2 + schunk * 16);
            vb = (unsigned)(r * ldb2 + schunk * 16);
        }
        stage_piece(ra, ia + p * 1024, va);
        stage_piece(rb, ib + p * 1024, vb);
    }
}

// tile_accum (attn_tile.h) with the transposed reads WRITTEN OUT, for win_attn_dkv_kernel alone: through tr_frag that kernel
// takes 116 VGPRs where it took 112 (profiles/attn_tile_ab.md).  The rows, chunks and halves are those of aim_common.h tr_frag.
__device__ __forceinline__ void tile_accum_dkv(f32x4 (&o)[4], const AIM_LDS char* img, const f32x4 (&w)[4], int frow, int fq) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        bf16x8 pf;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            pf[e] = (bf16_t)w[2 * kk][e];
            pf[4 + e] = (bf16_t)w[2 * kk + 1][e];
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const int r0 = (2 * kk) * 16 + fq * 4 + (frow >> 2);
            const int ch = dt * 2 + ((frow & 3) >> 1), half = (frow & 1) * 8;
            const bf16x4 v0 = lds_read_tr4(img + swz_off(r0, ch) + half);
            const bf16x4 v1 = lds_read_tr4(img + swz_off(r0 + 16, ch) + half);
            bf16x8 vf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vf[e] = v0[e];
                vf[4 + e] = v1[e];
            }
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
        }
    }
}

#define WIN_PROLOGUE                                                                           \
    __shared__ __attribute__((aligned(16))) char smem_raw[2 * 8192];                           \
    AIM_LDS char* sA = (AIM_LDS char*)smem_raw;                                                \
    AIM_LDS char* sB = sA + 8192;                                                              \
    const WinItem it = win_item<MODE>(g, (int)blockIdx.x);                                    \
    const int tid = threadIdx.x, lane = tid & 63;                                              \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = (int)(blockDim.x >> 6); \
    if (MODE != WIN_PLAIN && (int)blockIdx.y * nwaves * 16 >= it.S) return; /* a small box: before any barrier */ \
    const int frow = lane & 15, fq = lane >> 4;                                                \
    const int D = g.H * 64, ld = 3 * D;                                                        \
    const long long clip_rows = (long long)g.T * g.P;                                          \
    const int own0 = ((int)blockIdx.y * nwaves + wave) * 16;                                   \
    const bool active = own0 < it.S;                                                           \
    const int oi = own0 + frow;                                                                \
    const bool own_ok = oi < it.S;                                                             \
    const int orow = win_row<MODE>(g, it, own_ok ? oi : it.S - 1);                            \
    const int ntiles = (it.S + 63) >> 6;

template <int MODE>
__global__ __launch_bounds__(512) void win_attn_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                           float* __restrict__ lse, const WinGeom g) {
    WIN_PROLOGUE
    const bf16_t* cq = qkv + (long long)it.b * clip_rows * ld + it.h * 64;
    const long long span = ((clip_rows - 1) * ld + 64) * 2;
    const __amdgpu_buffer_rsrc_t rK = make_rsrc(cq + D, span), rV = make_rsrc(cq + 2 * D, span);
    bf16x8 qf[2];
    load_frag(qf, cq + (long long)orow * ld, fq);
    float m = -INFINITY, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < ntiles; ++kt) {
        if (kt) __syncthreads();
        stage_pair<MODE>(rK, ld * 2, sA, rV, ld * 2, sB, g, it, kt * 64, wave, nwaves, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!active) continue;
        f32x4 s[4];
        tile_scores(s, sA, qf, frow, fq);
        if (kt == ntiles - 1 && (it.S & 63)) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kt * 64 + t * 16 + fq * 4 + e >= it.S) s[t][e] = -INFINITY;
        }
        float mx = m;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, s[t][e]);
        mx = quad_max(mx);
        const float alpha = __builtin_amdgcn_exp2f((m - mx) * C2);      // first tile: 2^-inf = 0
        const float mc = mx * C2;
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = __builtin_amdgcn_exp2f(s[t][e] * C2 - mc);
                s[t][e] = p;
                sum += p;
            }
        sum = quad_sum(sum);
        l = l * alpha + sum;
        m = mx;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
        tile_accum(o, sB, s, frow, fq);
    }
    if (!active) return;
    const float inv = 1.0f / l;
    if (fq == 0 && own_ok) lse[stat_index(g, it, orow)] = m * 0.125f + __logf(l);
    store_tiles16(out + ((long long)it.b * clip_rows + orow) * D + it.h * 64, o, inv, own_ok, fq);
}

// own = queries: delta and dQ
template <int MODE>
__global__ __launch_bounds__(512) void win_attn_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out,
                                                          const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                          float* __restrict__ delta, bf16_t* __restrict__ dqkv, const WinGeom g) {
    WIN_PROLOGUE
    const bf16_t* cq = qkv + (long long)it.b * clip_rows * ld + it.h * 64;
    const long long span = ((clip_rows - 1) * ld + 64) * 2;
    const __amdgpu_buffer_rsrc_t rK = make_rsrc(cq + D, span), rV = make_rsrc(cq + 2 * D, span);
    const long long grow = (long long)it.b * clip_rows + orow;
    bf16x8 qf[2], dof[2];
    load_frag(qf, cq + (long long)orow * ld, fq);
    load_frag(dof, dout + grow * D + it.h * 64, fq);
    float dl = 0.f;
    {
        bf16x8 of[2];
        load_frag(of, out + grow * D + it.h * 64, fq);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) dl = fmaf((float)dof[ks][e], (float)of[ks][e], dl);
        dl = quad_sum(dl);
    }
    const long long si = stat_index(g, it, orow);
    const float lse2 = lse[si] * LOG2E;
    if (active && fq == 0 && own_ok) delta[si] = dl;
    f32x4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < ntiles; ++kt) {
        if (kt) __syncthreads();
        stage_pair<MODE>(rK, ld * 2, sA, rV, ld * 2, sB, g, it, kt * 64, wave, nwaves, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!active) continue;
        f32x4 s[4], dp[4];
        tile_scores(s, sA, qf, frow, fq);
        tile_scores(dp, sB, dof, frow, fq);
        const bool tail = kt == ntiles - 1 && (it.S & 63);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float p = __builtin_amdgcn_exp2f(s[t][e] * C2 - lse2);
                if (tail && kt * 64 + t * 16 + fq * 4 + e >= it.S) p = 0.f;
                s[t][e] = p * (dp[t][e] - dl) * 0.125f;
            }
        tile_accum(acc, sA, s, frow, fq);
    }
    if (!active) return;
    store_tiles16(dqkv + grow * ld + it.h * 64, acc, 1.0f, own_ok, fq);
}

// own = keys: dK and dV
template <int MODE>
__global__ __launch_bounds__(512) void win_attn_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           bf16_t* __restrict__ dqkv, const WinGeom g) {
    WIN_PROLOGUE
    __shared__ __attribute__((aligned(16))) float s_lse[64], s_delta[64];
    const bf16_t* cq = qkv + (long long)it.b * clip_rows * ld + it.h * 64;
    const bf16_t* cdo = dout + (long long)it.b * clip_rows * D + it.h * 64;
    const __amdgpu_buffer_rsrc_t rQ = make_rsrc(cq, ((clip_rows - 1) * ld + 64) * 2);
    const __amdgpu_buffer_rsrc_t rO = make_rsrc(cdo, ((clip_rows - 1) * D + 64) * 2);
    const long long grow = (long long)it.b * clip_rows + orow;
    bf16x8 kf[2], vf[2];
    load_frag(kf, cq + (long long)orow * ld + D, fq);
    load_frag(vf, cq + (long long)orow * ld + 2 * D, fq);
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qt = 0; qt < ntiles; ++qt) {
        if (qt) __syncthreads();
        stage_pair<MODE>(rQ, ld * 2, sA, rO, D * 2, sB, g, it, qt * 64, wave, nwaves, lane);
        if (tid < 64) {      // a streamed query past S: lse = +inf makes its probability 2^-inf = 0
            const int i = qt * 64 + tid;
            float a = INFINITY, d = 0.f;
            if (i < it.S) {
                const long long si = stat_index(g, it, win_row<MODE>(g, it, i));
                a = lse[si] * LOG2E;
                d = delta[si];
            }
            s_lse[tid] = a;
            s_delta[tid] = d;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!active) continue;
        f32x4 s[4], dp[4];
        tile_scores(s, sA, kf, frow, fq);
        tile_scores(dp, sB, vf, frow, fq);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 a = *(const f32x4*)&s_lse[t * 16 + fq * 4];
            const f32x4 d = *(const f32x4*)&s_delta[t * 16 + fq * 4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = __builtin_amdgcn_exp2f(s[t][e] * C2 - a[e]);
                s[t][e] = p;
                dp[t][e] = p * (dp[t][e] - d[e]) * 0.125f;
            }
        }
        tile_accum_dkv(dv, sB, s, frow, fq);
        tile_accum_dkv(dk, sA, dp, frow, fq);
    }
    if (!active) return;
    store_tiles16(dqkv + grow * ld + D + it.h * 64, dk, 1.0f, own_ok, fq);
    store_tiles16(dqkv + grow * ld + 2 * D + it.h * 64, dv, 1.0f, own_ok, fq);
}

// argument checks shared by both entry points; fills the geometry, the grid and the block size
int win_geom(const char* who, WinGeom* g, dim3* grid, int* threads, int B, int T, int N, int P, int H, int wt, int wh, int ww,
             int st = 0, int sh = 0, int sw = 0, bool cut_t = false) {
    AIM_CHECK_ARG(B > 0 && T > 0 && N > 1 && P >= N && H > 0 && wt > 0 && wh > 0 && ww > 0,
                  "%s: unsupported shape B=%d T=%d N=%d P=%d H=%d window=(%d,%d,%d)", who, B, T, N, P, H, wt, wh, ww);
    int G = 1;
    while ((long long)(G + 1) * (G + 1) <= N - 1) ++G;
    AIM_CHECK_ARG(G * G == N - 1, "%s: N - 1 = %d patch tokens are not a square grid", who, N - 1);
    wt = wt < T ? wt : T;      // get_window_size: an extent that reaches the grid's is clipped to it
    wh = wh < G ? wh : G;
    ww = ww < G ? ww : G;
    AIM_CHECK_ARG(T % wt == 0 && G % wh == 0 && G % ww == 0, "%s: window (%d,%d,%d) does not divide the grid (%d,%d,%d)", who, wt,
                  wh, ww, T, G, G);
    const long long S = (long long)wt * wh * ww;
    AIM_CHECK_ARG(S <= WIN_MAX_S, "%s: %lld tokens per window, at most %d", who, S, WIN_MAX_S);
    AIM_CHECK_ARG((long long)T * P * 3 * 64 * H * 2 < 0x7fffffffLL, "%s: a clip's qkv rows span more than 2 GiB (T=%d P=%d H=%d)",
                  who, T, P, H);
    AIM_CHECK_ARG(st >= 0 && sh >= 0 && sw >= 0 && st < wt && sh < wh && sw < ww,
                  "%s: shift (%d,%d,%d) outside [0, window) of the clipped window (%d,%d,%d)", who, st, sh, sw, wt, wh, ww);
    AIM_CHECK_ARG(!(st && wt == T) && !(sh && wh == G) && !(sw && ww == G),
                  "%s: shift (%d,%d,%d) on an axis whose window (%d,%d,%d) spans the grid (%d,%d,%d)", who, st, sh, sw, wt, wh, ww,
                  T, G, G);
    // a shifted h / w axis is cut at 0, s, s + w, ...: one segment more than windows; so is t where it is cut and not rolled
    const int nh = G / wh + (sh ? 1 : 0), nw = G / ww + (sw ? 1 : 0), nt = T / wt + (cut_t && st ? 1 : 0);
    const long long items = (long long)B * nt * nh * nw * H;
    AIM_CHECK_ARG(items < 0x7fffffffLL, "%s: %lld (window, head) items", who, items);
    g->T = T, g->P = P, g->G = G, g->H = H;
    g->wt = wt, g->wh = wh, g->ww = ww;
    g->nh = nh, g->nw = nw, g->nW = nt * nh * nw;
    g->S = (int)S;
    g->st = st, g->sh = sh, g->sw = sw;
    const int nwaves = S <= 16 ? 1 : S <= 32 ? 2 : S <= 64 ? 4 : 8;
    *threads = nwaves * 64;
    *grid = dim3((unsigned)items, (unsigned)((S + nwaves * 16 - 1) / (nwaves * 16)));
    return 0;
}

// "aim_<who><part>", the name AIM_CHECK_LAUNCH gives a failed launch (the macro evaluates it only then)
const char* launch_name(char (&buf)[48], const char* who, const char* part) {
    snprintf(buf, sizeof buf, "aim_%s%s", who, part);
    return buf;
}

// the host side of the three forward entries: WIN_CUT is the mode whose t axis is cut, the other two leave it whole
template <int MODE>
int launch_fwd(const char* who, const aim_bf16* qkv, aim_bf16* out, float* lse, int B, int T, int N, int P, int H, int wt, int wh,
               int ww, int st, int sh, int sw, void* stream) {
    WinGeom g;
    dim3 grid;
    int threads;
    char name[48];
    if (int rc = win_geom(who, &g, &grid, &threads, B, T, N, P, H, wt, wh, ww, st, sh, sw, MODE == WIN_CUT)) return rc;
    AIM_CHECK_ARG(qkv && out && lse, "%s: null pointer", who);
    hipLaunchKernelGGL(win_attn_fwd_kernel<MODE>, grid, dim3(threads), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)out, lse,
                       g);
    AIM_CHECK_LAUNCH(launch_name(name, who, ""));
    return 0;
}

// ... and of the three backward entries
template <int MODE>
int launch_bwd(const char* who, const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse, float* delta,
               aim_bf16* dqkv, int B, int T, int N, int P, int H, int wt, int wh, int ww, int st, int sh, int sw, void* stream) {
    WinGeom g;
    dim3 grid;
    int threads;
    char name[48];
    if (int rc = win_geom(who, &g, &grid, &threads, B, T, N, P, H, wt, wh, ww, st, sh, sw, MODE == WIN_CUT)) return rc;
    AIM_CHECK_ARG(qkv && out && dout && lse && delta && dqkv, "%s: null pointer", who);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(win_attn_dq_kernel<MODE>, grid, dim3(threads), 0, s, (const bf16_t*)qkv, (const bf16_t*)out,
                       (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv, g);
    AIM_CHECK_LAUNCH(launch_name(name, who, "(dq)"));
    hipLaunchKernelGGL(win_attn_dkv_kernel<MODE>, grid, dim3(threads), 0, s, (const bf16_t*)qkv, (const bf16_t*)dout, lse, delta,
                       (bf16_t*)dqkv, g);
    AIM_CHECK_LAUNCH(launch_name(name, who, "(dkv)"));
    return 0;
}

}  // namespace

extern "C" int aim_win_attn_fwd(const aim_bf16* qkv, aim_bf16* out, float* lse, int B, int T, int N, int P, int H, int wt,
                                int wh, int ww, void* stream) {
    return launch_fwd<WIN_PLAIN>("win_attn_fwd", qkv, out, lse, B, T, N, P, H, wt, wh, ww, 0, 0, 0, stream);
}

extern "C" int aim_win_attn_bwd(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse, float* delta,
                                aim_bf16* dqkv, int B, int T, int N, int P, int H, int wt, int wh, int ww, void* stream) {
    return launch_bwd<WIN_PLAIN>("win_attn_bwd", qkv, out, dout, lse, delta, dqkv, B, T, N, P, H, wt, wh, ww, 0, 0, 0, stream);
}

// Shifted windows (AIM_FLASH's odd blocks, vitclip_aim_flash.py: roll by -shift, strips along the border, attention inside each
// strip, nine cats, roll back).  In ORIGINAL coordinates that is, each axis on its own:
//   h, w with shift s > 0: [0, G) cut at 0, s, s + w, s + 2 w, ..., G -- a first segment of s, whole windows, a last segment of
//     w - s.  Nothing wraps: the rolled strips [-w:-s] and [-s:] ARE the last and the first segment.
//   t: whole windows in rolled coordinates; window k holds the frames (k wt + st + dt) mod T.  The last one wraps.
// One sequence = one (t window, h segment, w segment) box, tokens in (dt, dh, dw) row-major order; the boxes partition the patch
// tokens and the t map is a bijection on the clip's frames, so every result row still has one writer.  The boxes differ in
// size: gridDim.y is sized by the largest (a whole window) and a workgroup past its own box's S leaves before its first
// barrier; the tile loop runs to the box's own S.  With st = sh = sw = 0 the items, the token order and the tile order are
// those of the unshifted kernels, hence their bits.
extern "C" int aim_win_attn_fwd_shift(const aim_bf16* qkv, aim_bf16* out, float* lse, int B, int T, int N, int P, int H, int wt,
                                      int wh, int ww, int st, int sh, int sw, void* stream) {
    return launch_fwd<WIN_WRAP>("win_attn_fwd_shift", qkv, out, lse, B, T, N, P, H, wt, wh, ww, st, sh, sw, stream);
}

extern "C" int aim_win_attn_bwd_shift(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse,
                                      float* delta, aim_bf16* dqkv, int B, int T, int N, int P, int H, int wt, int wh, int ww,
                                      int st, int sh, int sw, void* stream) {
    return launch_bwd<WIN_WRAP>("win_attn_bwd_shift", qkv, out, dout, lse, delta, dqkv, B, T, N, P, H, wt, wh, ww, st, sh, sw, stream);
}

// Cut windows (AIM's odd blocks, vitclip_aim.py: roll by -shift, attention inside whole windows of the rolled grid under an
// additive -100 mask between the regions compute_mask numbers, roll back).  The regions of an axis are [0, T - w), [T - w, T - s),
// [T - s, T) in rolled coordinates, so a rolled window that holds the wrap point falls into the pieces on either side of it.  In
// ORIGINAL coordinates EVERY axis, t included, is therefore cut at 0, s, s + w, s + 2 w, ..., extent: a first segment of s, whole
// windows, a last segment of w - s; an axis with s = 0 keeps plain windows.  One sequence = one (t segment, h segment, w segment)
// box, (T / wt + (st > 0)) nh nw of them per clip, with plain softmax attention inside (a weight of exactly 0 where the reference
// leaves at most (S - 1) e^(spread - 100)).  Everything else is the *_shift entries': arguments, buffers, refusals, one writer per row.
// With st = 0 the items, the token order and the tile order are those of *_shift at the same (sh, sw), hence their bits.
extern "C" int aim_win_attn_fwd_cut(const aim_bf16* qkv, aim_bf16* out, float* lse, int B, int T, int N, int P, int H, int wt,
                                    int wh, int ww, int st, int sh, int sw, void* stream) {
    return launch_fwd<WIN_CUT>("win_attn_fwd_cut", qkv, out, lse, B, T, N, P, H, wt, wh, ww, st, sh, sw, stream);
}

extern "C" int aim_win_attn_bwd_cut(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse, float* delta,
                                    aim_bf16* dqkv, int B, int T, int N, int P, int H, int wt, int wh, int ww, int st, int sh,
                                    int sw, void* stream) {
    return launch_bwd<WIN_CUT>("win_attn_bwd_cut", qkv, out, dout, lse, delta, dqkv, B, T, N, P, H, wt, wh, ww, st, sh, sw, stream);
}
