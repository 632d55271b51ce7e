// Attention of SwinTransformer2D_Adapter (reference swin2d_adapter.py:159-254 and :356-395), forward and backward: head width 32,
// sequences of at most 64 tokens under a learned additive bias.  gfx950 only.
//
// Two kinds of sequence over the same fused qkv [rows, 3 C] bf16 (C = 32 H, frame-major rows (frame, h, w)):
//   window  : the w x w tokens of one window of the grid ROLLED by -s (the reference's torch.roll / window_partition), S = w w.
//             Token i = (iy, ix) of window (wy, wx) of frame f has rolled coordinates (wy w + iy, wx w + ix) and lies at row
//             f L + ((wy w + iy + s) mod G) G + (wx w + ix + s) mod G: roll, partition, window_reverse and the roll back are
//             addresses, nothing is copied into window order.  With s > 0 each rolled axis has the reference's three regions
//             [0, G - w), [G - w, G - s), [G - s, G); a (query, key) pair of different regions -- the pairs that get -100 in
//             attn_mask -- is given the weight EXACTLY 0 (the reference leaves at most (S - 1) e^(spread - 100)): the softmax
//             runs over the keys of the query's own region.  In original coordinates those regions are the boxes that cut
//             each axis at 0, s, s + w, ...; the window-local token order makes the dense bias
//             [H, S, S] index directly as bias[h][i][j].
//   temporal: the T' <= 32 frame tokens of one (clip, position): token t of sequence (b, n) is row (b T' + t) L + n.
//
// One workgroup = one (sequence, head), CAP = 32 or 64 token slots (S <= CAP), CAP / 16 waves; wave v owns 16 tokens, one per
// MFMA column (lane & 15), the other side's tokens on the MFMA rows: the fragment layout of attn_tile.h with ONE K-step of
// v_mfma_f32_16x16x32_bf16 per score tile (head width 32).  A whole sequence is one key tile: no online rescale.
//   fwd: x = s (32^-1/2 log2 e) + bias log2 e on the fp32 score (q is never scaled), p = 2^(x - max) in fp32,
//        O^T = V^T bf16(p), out = bf16(O / sum p), lse2 = max + log2 sum p (base 2).
//   bwd: phase A (own = queries): p = 2^(x - lse2), dP = V dO, delta = sum_j p_j dP_j, dS = p (dP - delta), all fp32 (a one-key
//        sequence gets dS = 0 exactly); dS is added, unrounded, to the lane's bias-gradient registers; dQ^T = 32^-1/2 K^T bf16(dS);
//        bf16(p)^T and bf16(dS)^T go to LDS.
//        phase B (own = keys): dV^T = dO^T bf16(p), dK^T = 32^-1/2 Q^T bf16(dS).  Every row of dqkv has one writer.
// Rounding points: bf16 q, k, v, dO; bf16 p and dS as MFMA operands; everything else fp32.
//
// Bias gradient, sum over sequences of P o (dP - delta) (no scale factor): two stages, fixed order, no atomics.  The backward
// grid is (chunks, H); a workgroup walks the sequences of its chunk in ascending order and each lane keeps the 4 CAP / 16
// (query, key) sums it owns in registers, then writes them to partial[chunk][h][S][S]; a second kernel adds the chunks in
// ascending order.  aim_swin_bias_scatter folds the dense [H, S, S] gradient into the [table, H] parameter by walking the
// index buffer in ascending order, one thread per table entry.  Equal bits on every run.
//
// Slots past S hold zeros in LDS, have p = 0 and are never stored; every global access is of a token below S.
#include <stdio.h>

#include "attn_tile.h"
#include "aim_kernels_internal.h"

namespace {

using attn_tile::LOG2E;
using attn_tile::prob_exp2;

constexpr int HD = 32;                                     // head width
constexpr float QK_SCALE = 0.17677669529663687f;           // 32^-1/2
constexpr float QK_SCALE2 = QK_SCALE * LOG2E;

struct SeqGeom {
    int temporal;             // 0: windows, 1: temporal sequences
    int S, H, nseq;
    int L;                    // rows per frame
    int G, w, s, nwx, nW;     // windows: grid side, window side, shift, windows per row, windows per frame
    int T;                    // temporal: tokens per sequence (= S)
};

// row of token i of sequence seq, and its mask region (0 where nothing is masked)
__device__ __forceinline__ void seq_token(const SeqGeom& g, int seq, int i, int* row, int* reg) {
    if (g.temporal) {
        const int b = seq / g.L, n = seq - b * g.L;
        *row = (b * g.T + i) * g.L + n;
        *reg = 0;
        return;
    }
    const int f = seq / g.nW, win = seq - f * g.nW, wy = win / g.nwx, wx = win - wy * g.nwx;
    const int iy = i / g.w, ix = i - iy * g.w;
    const int y = wy * g.w + iy, x = wx * g.w + ix;
    int ry = 0, rx = 0;
    if (g.s) {
        ry = y < g.G - g.w ? 0 : (y < g.G - g.s ? 1 : 2);
        rx = x < g.G - g.w ? 0 : (x < g.G - g.s ? 1 : 2);
    }
    int oy = y + g.s, ox = x + g.s;
    if (oy >= g.G) oy -= g.G;
    if (ox >= g.G) ox -= g.G;
    *row = f * g.L + oy * g.G + ox;
    *reg = ry * 3 + rx;
}

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (bf16_t)0.f;
    return z;
}

// 8 values of a row into the row-major image [CAP][32] and, with `imgT`, the transposed image [32][CAP]
template <int CAP>
__device__ __forceinline__ void put8(bf16_t* img, bf16_t* imgT, int r, int c, bf16x8 v) {
    if (img) *(bf16x8*)&img[r * HD + c * 8] = v;
    if (imgT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) imgT[(c * 8 + e) * CAP + r] = v[e];
    }
}

// two score tiles' fp32 accumulators (tiles 2 kk, 2 kk + 1) as the second MFMA operand: k position 8 fq + 4 u + e is token
// 16 (2 kk + u) + 4 fq + e
__device__ __forceinline__ bf16x8 pack_pair(f32x4 a, f32x4 b) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = (bf16_t)a[e];
        r[4 + e] = (bf16_t)b[e];
    }
    return r;
}

// the first operand that goes with pack_pair: row d of a transposed image [32][CAP], tokens in the same k order
template <int CAP>
__device__ __forceinline__ bf16x8 tr_pair(const bf16_t* imgT, int d, int kk, int fq) {
    const bf16x4 v0 = *(const bf16x4*)&imgT[d * CAP + (2 * kk) * 16 + fq * 4];
    const bf16x4 v1 = *(const bf16x4*)&imgT[d * CAP + (2 * kk + 1) * 16 + fq * 4];
    return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int CAP>
__global__ __launch_bounds__(CAP * 4) void swin_attn_fwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                                bf16_t* __restrict__ out, float* __restrict__ lse, const SeqGeom g) {
    constexpr int NT = CAP / 16;
    __shared__ __attribute__((aligned(16))) bf16_t sQ[CAP * HD], sK[CAP * HD], sVt[HD * CAP];
    __shared__ int sRow[CAP], sReg[CAP];
    const int item = (int)blockIdx.x, seq = item / g.H, h = item - seq * g.H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frow = lane & 15, fq = lane >> 4;
    const int C = g.H * HD, ld = 3 * C, S = g.S;
    {
        const int r = tid >> 2, c = tid & 3;
        bf16x8 q = zero8(), k = zero8(), v = zero8();
        if (r < S) {
            int row, reg;
            seq_token(g, seq, r, &row, &reg);
            if (c == 0) sRow[r] = row, sReg[r] = reg;
            const bf16_t* p = qkv + (long long)row * ld + h * HD + c * 8;
            q = *(const bf16x8*)p;
            k = *(const bf16x8*)(p + C);
            v = *(const bf16x8*)(p + 2 * C);
        } else if (c == 0) {
            sRow[r] = 0, sReg[r] = -1;
        }
        put8<CAP>(sQ, nullptr, r, c, q);
        put8<CAP>(sK, nullptr, r, c, k);
        put8<CAP>(nullptr, sVt, r, c, v);
    }
    __syncthreads();
    const int qi = wave * 16 + frow;
    const bool qv = qi < S;
    const int qb = qv ? qi : S - 1;      // a slot past S computes the last token's row and stores nothing
    const int rq = sReg[qb];
    const bf16x8 qf = *(const bf16x8*)&sQ[qb * HD + fq * 8];
    const float* brow = bias + ((long long)h * S + qb) * S;
    f32x4 s[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const bf16x8 kf = *(const bf16x8*)&sK[(t * 16 + frow) * HD + fq * 8];
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = t * 16 + fq * 4 + e;
            float x = -INFINITY;
            if (key < S && sReg[key] == rq) x = fmaf(s[t][e], QK_SCALE2, brow[key] * LOG2E);
            s[t][e] = x;
            mx = fmaxf(mx, x);
        }
    }
    mx = quad_max(mx);      // finite: the query's own key is in its region
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = __builtin_amdgcn_exp2f(s[t][e] - mx);
            s[t][e] = p;
            sum += p;
        }
    sum = quad_sum(sum);
    f32x4 o[2];
    o[0] = o[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NT / 2; ++kk) {
        const bf16x8 pf = pack_pair(s[2 * kk], s[2 * kk + 1]);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_pair<CAP>(sVt, dt * 16 + frow, kk, fq), pf, o[dt], 0, 0, 0);
    }
    if (!qv) return;
    const float inv = 1.0f / sum;
    bf16_t* orow = out + (long long)sRow[qi] * C + h * HD;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) store4(orow + dt * 16 + fq * 4, o[dt] * inv);
    if (fq == 0) lse[(long long)item * CAP + qi] = mx + __log2f(sum);
}

template <int CAP>
__global__ __launch_bounds__(CAP * 4) void swin_attn_bwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                                const bf16_t* __restrict__ dout, const float* __restrict__ lse, bf16_t* __restrict__ dqkv,
                                                                float* __restrict__ partial, int per_chunk, const SeqGeom g) {
    constexpr int NT = CAP / 16;
    __shared__ __attribute__((aligned(16))) bf16_t sK[CAP * HD], sV[CAP * HD], sQ[CAP * HD], sdO[CAP * HD];
    __shared__ __attribute__((aligned(16))) bf16_t sKt[HD * CAP], sQt[HD * CAP], sdOt[HD * CAP];
    __shared__ __attribute__((aligned(16))) bf16_t sPt[CAP * CAP], sdSt[CAP * CAP];      // [key][query]
    __shared__ int sRow[CAP], sReg[CAP];
    const int chunk = (int)blockIdx.x, h = (int)blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frow = lane & 15, fq = lane >> 4;
    const int C = g.H * HD, ld = 3 * C, S = g.S;
    const int seq0 = chunk * per_chunk, seq1 = seq0 + per_chunk < g.nseq ? seq0 + per_chunk : g.nseq;
    const int qi = wave * 16 + frow;      // the lane's token: a query in phase A, a key in phase B
    const bool qv = qi < S;
    const int qb = qv ? qi : S - 1;
    const float* brow = bias + ((long long)h * S + qb) * S;
    f32x4 db[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) db[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int seq = seq0; seq < seq1; ++seq) {
        __syncthreads();      // the previous sequence's phase B has read the images
        {
            const int r = tid >> 2, c = tid & 3;
            bf16x8 q = zero8(), k = zero8(), v = zero8(), d = zero8();
            if (r < S) {
                int row, reg;
                seq_token(g, seq, r, &row, &reg);
                if (c == 0) sRow[r] = row, sReg[r] = reg;
                const bf16_t* p = qkv + (long long)row * ld + h * HD + c * 8;
                q = *(const bf16x8*)p;
                k = *(const bf16x8*)(p + C);
                v = *(const bf16x8*)(p + 2 * C);
                d = *(const bf16x8*)(dout + (long long)row * C + h * HD + c * 8);
            } else if (c == 0) {
                sRow[r] = 0, sReg[r] = -1;
            }
            put8<CAP>(sQ, sQt, r, c, q);
            put8<CAP>(sK, sKt, r, c, k);
            put8<CAP>(sV, nullptr, r, c, v);
            put8<CAP>(sdO, sdOt, r, c, d);
        }
        __syncthreads();
        // ---- phase A: own = queries
        const int item = seq * g.H + h;
        const int rq = sReg[qb];
        const bf16x8 qf = *(const bf16x8*)&sQ[qb * HD + fq * 8];
        const bf16x8 dof = *(const bf16x8*)&sdO[qb * HD + fq * 8];
        const float lse2 = lse[(long long)item * CAP + qb];
        f32x4 ds[NT], dp[NT];
        float dl = 0.f;      // delta = sum_j p_j dP_j (= dO . O): a one-key sequence gets dS = 0 exactly
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bf16x8 kf = *(const bf16x8*)&sK[(t * 16 + frow) * HD + fq * 8];
            const bf16x8 vf = *(const bf16x8*)&sV[(t * 16 + frow) * HD + fq * 8];
            const f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int key = t * 16 + fq * 4 + e;
                float p = 0.f;
                if (qv && key < S && sReg[key] == rq) p = prob_exp2(fmaf(sc[e], QK_SCALE2, brow[key] * LOG2E) - lse2);
                ds[t][e] = p;
                dl = fmaf(p, dp[t][e], dl);
            }
        }
        dl = quad_sum(dl);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int key = t * 16 + fq * 4 + e;
                const float p = ds[t][e], d = p * (dp[t][e] - dl);
                ds[t][e] = d;
                db[t][e] += d;
                sPt[key * CAP + qi] = (bf16_t)p;
                sdSt[key * CAP + qi] = (bf16_t)d;
            }
        {
            f32x4 dq[2];
            dq[0] = dq[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < NT / 2; ++kk) {
                const bf16x8 dsf = pack_pair(ds[2 * kk], ds[2 * kk + 1]);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_pair<CAP>(sKt, dt * 16 + frow, kk, fq), dsf, dq[dt], 0, 0, 0);
            }
            if (qv) {
                bf16_t* row = dqkv + (long long)sRow[qi] * ld + h * HD;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) store4(row + dt * 16 + fq * 4, dq[dt] * QK_SCALE);
            }
        }
        __syncthreads();
        // ---- phase B: own = keys; the reduction runs over the queries, 32 per K-step, contiguous in the [key][query] images
        f32x4 dk[2], dv[2];
        dk[0] = dk[1] = dv[0] = dv[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int qq = 0; qq < CAP / 32; ++qq) {
            const bf16x8 pf = *(const bf16x8*)&sPt[qi * CAP + qq * 32 + fq * 8];
            const bf16x8 dsf = *(const bf16x8*)&sdSt[qi * CAP + qq * 32 + fq * 8];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 dot = *(const bf16x8*)&sdOt[(dt * 16 + frow) * CAP + qq * 32 + fq * 8];
                const bf16x8 qt = *(const bf16x8*)&sQt[(dt * 16 + frow) * CAP + qq * 32 + fq * 8];
                dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dot, pf, dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, dsf, dk[dt], 0, 0, 0);
            }
        }
        if (qv) {
            bf16_t* row = dqkv + (long long)sRow[qi] * ld + h * HD;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                store4(row + C + dt * 16 + fq * 4, dk[dt] * QK_SCALE);
                store4(row + 2 * C + dt * 16 + fq * 4, dv[dt]);
            }
        }
    }
    if (partial && qv) {
        float* prow = partial + (((long long)chunk * g.H + h) * S + qi) * S;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int key = t * 16 + fq * 4 + e;
                if (key < S) prow[key] = db[t][e];
            }
    }
}

// dense[i] = sum over the chunks, in ascending order, of partial[c][i]
__global__ void swin_bias_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dense, int nchunks, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    for (int c = 0; c < nchunks; ++c) acc += partial[(long long)c * n + i];
    dense[i] = acc;
}

// dtable[t][h] += sum, over the index entries equal to t in ascending order, of dense[h][entry]
__global__ void swin_bias_scatter_kernel(const float* __restrict__ dense, const int* __restrict__ index, float* __restrict__ dtable,
                                         int H, int SS, int ntable) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntable * H) return;
    const int t = i / H, h = i - t * H;
    float acc = 0.f;
    for (int e = 0; e < SS; ++e)
        if (index[e] == t) acc += dense[(long long)h * SS + e];
    dtable[i] += acc;
}

int chunks_of(int nseq, int H, int* per_chunk) {
    int n = (1024 + H - 1) / H;
    if (n > nseq) n = nseq;
    const int per = (nseq + n - 1) / n;
    *per_chunk = per;
    return (nseq + per - 1) / per;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int window_geom(const char* who, SeqGeom* g, int frames, int res, int H, int w, int s) {
    AIM_CHECK_ARG(frames > 0 && res > 0 && H > 0 && w > 0, "%s: unsupported shape frames=%d res=%d H=%d window=%d", who, frames, res, H, w);
    AIM_CHECK_ARG(w * w <= 64, "%s: %d tokens per window, at most 64 (one key tile)", who, w * w);
    AIM_CHECK_ARG(w <= res && res % w == 0, "%s: window %d does not divide the resolution %d", who, w, res);
    AIM_CHECK_ARG(s >= 0 && s < w && !(s && w == res), "%s: shift %d outside [0, window %d), or on a window that spans the grid", who, s, w);
    const long long rows = (long long)frames * res * res, nseq = (long long)frames * (res / w) * (res / w);
    AIM_CHECK_ARG(rows * 3 * HD * H < 0x7fffffffLL && nseq * H < 0x7fffffffLL, "%s: %lld rows of %d heads are too many", who, rows, H);
    g->temporal = 0, g->S = w * w, g->H = H, g->nseq = (int)nseq, g->L = res * res;
    g->G = res, g->w = w, g->s = s, g->nwx = res / w, g->nW = (res / w) * (res / w), g->T = 0;
    return 0;
}

int temporal_geom(const char* who, SeqGeom* g, int B, int T, int L, int H) {
    AIM_CHECK_ARG(B > 0 && T > 0 && L > 0 && H > 0, "%s: unsupported shape B=%d T=%d L=%d H=%d", who, B, T, L, H);
    AIM_CHECK_ARG(T <= 32, "%s: %d frame tokens per sequence, at most 32", who, T);
    const long long rows = (long long)B * T * L, nseq = (long long)B * L;
    AIM_CHECK_ARG(rows * 3 * HD * H < 0x7fffffffLL && nseq * H < 0x7fffffffLL, "%s: %lld rows of %d heads are too many", who, rows, H);
    g->temporal = 1, g->S = T, g->H = H, g->nseq = (int)nseq, g->L = L;
    g->G = 0, g->w = 0, g->s = 0, g->nwx = 1, g->nW = 1, g->T = T;
    return 0;
}

int launch_fwd(const char* who, const SeqGeom& g, const aim_bf16* qkv, const float* bias, aim_bf16* out, float* lse, void* stream) {
    AIM_CHECK_ARG(qkv && bias && out && lse, "%s: null pointer", who);
    AIM_CHECK_ARG(aligned16(qkv) && aligned16(out), "%s: qkv and out must be 16-byte aligned", who);
    const dim3 grid((unsigned)(g.nseq * g.H));
    if (g.S <= 32)
        hipLaunchKernelGGL(swin_attn_fwd_kernel<32>, grid, dim3(128), 0, (hipStream_t)stream, (const bf16_t*)qkv, bias, (bf16_t*)out, lse, g);
    else
        hipLaunchKernelGGL(swin_attn_fwd_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, bias, (bf16_t*)out, lse, g);
    AIM_CHECK_LAUNCH(who);
    return 0;
}

int launch_bwd(const char* who, const SeqGeom& g, const aim_bf16* qkv, const float* bias, const aim_bf16* dout, const float* lse,
               aim_bf16* dqkv, float* dbias, float* workspace, int64_t workspace_bytes, void* stream) {
    AIM_CHECK_ARG(qkv && bias && dout && lse && dqkv, "%s: null pointer", who);
    AIM_CHECK_ARG(aligned16(qkv) && aligned16(dout) && aligned16(dqkv), "%s: the bf16 buffers must be 16-byte aligned", who);
    int per = 0;
    const int nchunks = chunks_of(g.nseq, g.H, &per);
    const long long n = (long long)g.H * g.S * g.S;
    if (dbias)
        AIM_CHECK_ARG(workspace && workspace_bytes >= (int64_t)nchunks * n * 4, "%s: the bias gradient needs a workspace of %lld bytes", who,
                      (long long)nchunks * n * 4);
    float* partial = dbias ? workspace : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nchunks, (unsigned)g.H);
    if (g.S <= 32)
        hipLaunchKernelGGL(swin_attn_bwd_kernel<32>, grid, dim3(128), 0, st, (const bf16_t*)qkv, bias, (const bf16_t*)dout, lse, (bf16_t*)dqkv, partial, per, g);
    else
        hipLaunchKernelGGL(swin_attn_bwd_kernel<64>, grid, dim3(256), 0, st, (const bf16_t*)qkv, bias, (const bf16_t*)dout, lse, (bf16_t*)dqkv, partial, per, g);
    AIM_CHECK_LAUNCH(who);
    if (dbias) {
        hipLaunchKernelGGL(swin_bias_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partial, dbias, nchunks, (int)n);
        AIM_CHECK_LAUNCH(who);
    }
    return 0;
}

}  // namespace

extern "C" int64_t aim_swin_attn_bwd_workspace_bytes(int nseq, int H, int S) {
    if (nseq <= 0 || H <= 0 || S <= 0) return 0;
    int per = 0;
    return (int64_t)chunks_of(nseq, H, &per) * H * S * S * 4;
}

extern "C" int aim_swin_win_attn_fwd(const aim_bf16* qkv, const float* bias, aim_bf16* out, float* lse, int frames, int res, int H,
                                     int window, int shift, void* stream) {
    SeqGeom g;
    if (int rc = window_geom("swin_win_attn_fwd", &g, frames, res, H, window, shift)) return rc;
    return launch_fwd("swin_win_attn_fwd", g, qkv, bias, out, lse, stream);
}

extern "C" int aim_swin_win_attn_bwd(const aim_bf16* qkv, const float* bias, const aim_bf16* dout, const float* lse,
                                     aim_bf16* dqkv, float* dbias, int frames, int res, int H, int window, int shift,
                                     float* workspace, int64_t workspace_bytes, void* stream) {
    SeqGeom g;
    if (int rc = window_geom("swin_win_attn_bwd", &g, frames, res, H, window, shift)) return rc;
    return launch_bwd("swin_win_attn_bwd", g, qkv, bias, dout, lse, dqkv, dbias, workspace, workspace_bytes, stream);
}

extern "C" int aim_swin_tattn_fwd(const aim_bf16* qkv, const float* bias, aim_bf16* out, float* lse, int B, int T, int L, int H,
                                  void* stream) {
    SeqGeom g;
    if (int rc = temporal_geom("swin_tattn_fwd", &g, B, T, L, H)) return rc;
    return launch_fwd("swin_tattn_fwd", g, qkv, bias, out, lse, stream);
}

extern "C" int aim_swin_tattn_bwd(const aim_bf16* qkv, const float* bias, const aim_bf16* dout, const float* lse,
                                  aim_bf16* dqkv, float* dbias, int B, int T, int L, int H, float* workspace, int64_t workspace_bytes,
                                  void* stream) {
    SeqGeom g;
    if (int rc = temporal_geom("swin_tattn_bwd", &g, B, T, L, H)) return rc;
    return launch_bwd("swin_tattn_bwd", g, qkv, bias, dout, lse, dqkv, dbias, workspace, workspace_bytes, stream);
}

extern "C" int aim_swin_bias_scatter(const float* dense, const int* index, float* dtable, int H, int SS, int ntable, void* stream) {
    AIM_CHECK_ARG(dense && index && dtable, "swin_bias_scatter: null pointer");
    AIM_CHECK_ARG(H > 0 && SS > 0 && SS <= 4096 && ntable > 0 && (long long)ntable * H < 0x7fffffffLL,
                  "swin_bias_scatter: unsupported shape H=%d entries=%d table=%d", H, SS, ntable);
    hipLaunchKernelGGL(swin_bias_scatter_kernel, dim3((unsigned)((ntable * H + 127) / 128)), dim3(128), 0, (hipStream_t)stream, dense,
                       index, dtable, H, SS, ntable);
    AIM_CHECK_LAUNCH("swin_bias_scatter");
    return 0;
}
