// Attention of SwinTransformer3D (reference swin_transformer.py, WindowAttention3D and SwinTransformerBlock3D.forward_part1),
// forward and backward: head width 32, 3-D windows of up to 1024 tokens streamed in 64-token tiles, under the learned 3-D
// relative-position bias read straight from its table.  gfx950 only.
//
// Sequences.  In original coordinates the reference's roll by -shift, window_partition, -100 mask, window_reverse and roll
// back are plain softmax attention inside BOXES: each axis of the (D, G, G) token grid is cut at 0, s, s + w, s + 2w, ... (at
// 0, w, 2w, ... where that axis's shift is 0), nothing wraps, and a pair the mask gives -100 has the weight EXACTLY 0 (DESIGN.md
// section 2k).  A sequence is one box; its tokens are numbered t-major over the box's own extent (lt, lh, lw), each extent being
// s, w or w - s, so a box holds between 1 and wt wh ww tokens.  Token (ct, ch, cw) of a box with origin (t0, h0, w0) of clip b
// is row ((b D + t0 + ct) G + h0 + ch) G + w0 + cw of the fused qkv [rows, 3 C] bf16 (C = 32 H): no copy into window order.
//
// Bias.  index(q, k) = f(q) - f(k) + const with f(t, h, w) = (t (2Wh - 1) + h)(2Ww - 1) + w on box-local coordinates and
// const = f(Wt - 1, Wh - 1, Ww - 1), (Wt, Wh, Ww) being the FULL window of the constructor (the table's strides) also where
// the effective t extent wt was clipped to the clip.  The head's column of the [table, H] fp32 parameter sits in LDS, already
// times log2 e; a per-tile LDS array of the streamed tokens' f makes the bias one subtraction and one LDS gather per score.
//
// Capacity: at most MAX_S = 1024 tokens per window and TAB_CAP = 5248 table entries (20.5 KiB): (16,7,7) has 784 and 5239.
//
// One workgroup = 256 threads = 4 waves; wave v owns 16 tokens of a 64-token tile, one per MFMA column (lane & 15), the
// streamed side's tokens on the MFMA rows: one K-step of v_mfma_f32_16x16x32_bf16 per 16 x 16 score tile, two O tiles.
//   fwd  (grid: (box, head) x query tile): K and V^T stream through LDS; x = s (32^-1/2 log2 e) + bias log2 e on the fp32
//        score (q is never scaled), online (max, sum) rescale per tile, p = 2^(x - max) in fp32, O^T += V^T bf16(p),
//        out = bf16(O / sum p), lse2 = max + log2 sum p (base 2) at [row][head].
//   bwd 1 (grid as fwd, own = queries): sweep 1 over the key tiles gives delta = sum_j p_j dP_j in fp32 (p = 2^(x - lse2),
//        dP = V dO; a one-key box gets dS = 0 exactly), stored at [row][head]; sweep 2 forms dS = p (dP - delta) and
//        dQ^T = 32^-1/2 K^T bf16(dS).
//   bwd 2 (grid: walk x head, own = keys): the workgroup walks a fixed list of boxes; per key tile it streams Q and dO,
//        recomputes p and dS from lse2 and delta, dV^T = dO^T bf16(p), dK^T = 32^-1/2 Q^T bf16(dS).
// A workgroup past a small box leaves before any barrier.  Every row of dqkv has one writer and a fixed summation order.
// Rounding points: bf16 q, k, v, dO; bf16 p and dS as MFMA operands; everything else fp32.
//
// Table gradient, dtable[r][h] += sum over boxes and pairs with index(q, k) = r of dS (no scale factor, no atomics): bwd 2 adds
// each unrounded fp32 dS into partial[walk][h][pos(q)][pos(k)], pos(ct, ch, cw) = (ct wh + ch) ww + cw on the window lattice
// (only differences of positions matter, so box-local coordinates do); the boxes of a walk are run one after another by one
// workgroup, so every element has one owner at a time.  A second kernel adds the walks in ascending order into a dense
// [H, S, S]; a third gives each thread one (r, h) and sums the pairs k = q - r in ascending q onto what the table gradient
// holds.  Equal bits on every run, and dqkv does not depend on whether the table gradient is asked for.
#include <stdio.h>

#include "attn_tile.h"
#include "aim_kernels_internal.h"

namespace {

using attn_tile::LOG2E;
using attn_tile::prob_exp2;

constexpr int HD = 32;                                     // head width
constexpr int TILE = 64;                                   // streamed tokens per tile, and own tokens per workgroup
constexpr int NT = TILE / 16;
constexpr int MAX_S = 1024;                                // tokens per window
constexpr int TAB_CAP = 5248;                              // table entries
constexpr float QK_SCALE = 0.17677669529663687f;           // 32^-1/2
constexpr float QK_SCALE2 = QK_SCALE * LOG2E;

struct Geom3 {
    int B, D, G, H;
    int wt, wh, ww;           // effective window
    int st, sh, sw;           // shift
    int nbt, nbh, nbw;        // boxes per axis
    int nbox, nboxes;         // boxes per clip, boxes in all
    int fh, fw;               // 2 Wh - 1, 2 Ww - 1: the strides of f
    int cst, ntab;            // f(Wt - 1, Wh - 1, Ww - 1), table entries
    int Sw;                   // wt wh ww
};

struct Box {
    int row0;                 // row of the box's origin
    int lt, lh, lw, S;
};

__device__ __forceinline__ void axis_cut(int i, int n, int w, int s, int* start, int* len) {
    if (s == 0) {
        *start = i * w, *len = w;
    } else if (i == 0) {
        *start = 0, *len = s;
    } else {
        const int a = s + (i - 1) * w;
        *start = a, *len = n - a < w ? n - a : w;
    }
}

__device__ __forceinline__ Box box_of(const Geom3& g, int box) {
    const int clip = box / g.nbox, r = box - clip * g.nbox;
    const int bt = r / (g.nbh * g.nbw), r2 = r - bt * g.nbh * g.nbw, bh = r2 / g.nbw, bw = r2 - bh * g.nbw;
    int t0, h0, w0;
    Box b;
    axis_cut(bt, g.D, g.wt, g.st, &t0, &b.lt);
    axis_cut(bh, g.G, g.wh, g.sh, &h0, &b.lh);
    axis_cut(bw, g.G, g.ww, g.sw, &w0, &b.lw);
    b.row0 = ((clip * g.D + t0) * g.G + h0) * g.G + w0;
    b.S = b.lt * b.lh * b.lw;
    return b;
}

// token i < b.S of a box: its row, f and lattice position
__device__ __forceinline__ void box_token(const Geom3& g, const Box& b, int i, int* row, int* f, int* pos) {
    const int ct = i / (b.lh * b.lw), r = i - ct * b.lh * b.lw, ch = r / b.lw, cw = r - ch * b.lw;
    *row = b.row0 + (ct * g.G + ch) * g.G + cw;
    *f = (ct * g.fh + ch) * g.fw + cw;
    *pos = (ct * g.wh + ch) * g.ww + cw;
}

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (bf16_t)0.f;
    return z;
}

// 8 values of a row into the row-major image [TILE][32] and, with `imgT`, the transposed image [32][TILE]
__device__ __forceinline__ void put8(bf16_t* img, bf16_t* imgT, int r, int c, bf16x8 v) {
    if (img) *(bf16x8*)&img[r * HD + c * 8] = v;
    if (imgT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) imgT[(c * 8 + e) * TILE + r] = v[e];
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

// the first operand that goes with pack_pair: row d of a transposed image [32][TILE], tokens in the same k order
__device__ __forceinline__ bf16x8 tr_pair(const bf16_t* imgT, int d, int kk, int fq) {
    const bf16x4 v0 = *(const bf16x4*)&imgT[d * TILE + (2 * kk) * 16 + fq * 4];
    const bf16x4 v1 = *(const bf16x4*)&imgT[d * TILE + (2 * kk + 1) * 16 + fq * 4];
    return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ void load_table(float* sTab, const float* __restrict__ table, const Geom3& g, int h, int tid) {
    for (int i = tid; i < g.ntab; i += 256) sTab[i] = table[(long long)i * g.H + h] * LOG2E;
}

__global__ __launch_bounds__(256) void swin3d_attn_fwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ table,
                                                              bf16_t* __restrict__ out, float* __restrict__ lse, const Geom3 g) {
    __shared__ float sTab[TAB_CAP];
    __shared__ __attribute__((aligned(16))) bf16_t sK[TILE * HD], sVt[HD * TILE];
    __shared__ int sF[TILE];
    const int item = (int)blockIdx.x, box = item / g.H, h = item - box * g.H;
    const Box b = box_of(g, box);
    const int S = b.S;
    if ((int)blockIdx.y * TILE >= S) return;      // before any barrier
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frow = lane & 15, fq = lane >> 4;
    const int C = g.H * HD, ld = 3 * C;
    load_table(sTab, table, g, h, tid);
    const int qi = (int)blockIdx.y * TILE + wave * 16 + frow;
    const bool qv = qi < S;
    int qrow, qf_, qpos;
    box_token(g, b, qv ? qi : S - 1, &qrow, &qf_, &qpos);      // a slot past S computes the last token's row and stores nothing
    const int fqc = qf_ + g.cst;
    const bf16x8 qf = *(const bf16x8*)(qkv + (long long)qrow * ld + h * HD + fq * 8);
    float mx = -INFINITY, sum = 0.f;      // sum: the lane's own keys; the quad is added at the end
    f32x4 o[2];
    o[0] = o[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < S; k0 += TILE) {
        __syncthreads();      // the previous tile has been read
        {
            const int r = tid >> 2, c = tid & 3;
            bf16x8 k = zero8(), v = zero8();
            int f = 0;
            if (k0 + r < S) {
                int row, pos;
                box_token(g, b, k0 + r, &row, &f, &pos);
                const bf16_t* p = qkv + (long long)row * ld + C + h * HD + c * 8;
                k = *(const bf16x8*)p;
                v = *(const bf16x8*)(p + C);
            }
            if (c == 0) sF[r] = f;
            put8(sK, nullptr, r, c, k);
            put8(nullptr, sVt, r, c, v);
        }
        __syncthreads();
        f32x4 s[NT];
        float tmx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bf16x8 kf = *(const bf16x8*)&sK[(t * 16 + frow) * HD + fq * 8];
            s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int key = t * 16 + fq * 4 + e;
                float x = -INFINITY;
                if (k0 + key < S) x = fmaf(s[t][e], QK_SCALE2, sTab[fqc - sF[key]]);
                s[t][e] = x;
                tmx = fmaxf(tmx, x);
            }
        }
        tmx = quad_max(tmx);      // finite: a tile has at least one key of the box
        const float mn = fmaxf(mx, tmx), alpha = __builtin_amdgcn_exp2f(mx - mn);
        mx = mn;
        sum *= alpha;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = __builtin_amdgcn_exp2f(s[t][e] - mn);
                s[t][e] = p;
                sum += p;
            }
        o[0] = o[0] * alpha;
        o[1] = o[1] * alpha;
#pragma unroll
        for (int kk = 0; kk < NT / 2; ++kk) {
            const bf16x8 pf = pack_pair(s[2 * kk], s[2 * kk + 1]);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_pair(sVt, dt * 16 + frow, kk, fq), pf, o[dt], 0, 0, 0);
        }
    }
    sum = quad_sum(sum);
    if (!qv) return;
    const float inv = 1.0f / sum;
    bf16_t* orow = out + (long long)qrow * C + h * HD;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) store4(orow + dt * 16 + fq * 4, o[dt] * inv);
    if (fq == 0) lse[(long long)qrow * g.H + h] = mx + __log2f(sum);
}

// bwd 1: own = queries.  Sweep 1: delta; sweep 2: dQ.
__global__ __launch_bounds__(256) void swin3d_attn_bwd_dq_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ table,
                                                                 const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                 float* __restrict__ delta, bf16_t* __restrict__ dqkv, const Geom3 g) {
    __shared__ float sTab[TAB_CAP];
    __shared__ __attribute__((aligned(16))) bf16_t sK[TILE * HD], sV[TILE * HD], sKt[HD * TILE];
    __shared__ int sF[TILE];
    const int item = (int)blockIdx.x, box = item / g.H, h = item - box * g.H;
    const Box b = box_of(g, box);
    const int S = b.S;
    if ((int)blockIdx.y * TILE >= S) return;      // before any barrier
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frow = lane & 15, fq = lane >> 4;
    const int C = g.H * HD, ld = 3 * C;
    load_table(sTab, table, g, h, tid);
    const int qi = (int)blockIdx.y * TILE + wave * 16 + frow;
    const bool qv = qi < S;
    int qrow, qf_, qpos;
    box_token(g, b, qv ? qi : S - 1, &qrow, &qf_, &qpos);
    const int fqc = qf_ + g.cst;
    const bf16x8 qf = *(const bf16x8*)(qkv + (long long)qrow * ld + h * HD + fq * 8);
    const bf16x8 dof = *(const bf16x8*)(dout + (long long)qrow * C + h * HD + fq * 8);
    const float lse2 = lse[(long long)qrow * g.H + h];
    float dl = 0.f;      // delta = sum_j p_j dP_j (= dO . O): a one-key box gets dS = 0 exactly
    f32x4 dq[2];
    dq[0] = dq[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int k0 = 0; k0 < S; k0 += TILE) {
            __syncthreads();      // the previous tile has been read
            {
                const int r = tid >> 2, c = tid & 3;
                bf16x8 k = zero8(), v = zero8();
                int f = 0;
                if (k0 + r < S) {
                    int row, pos;
                    box_token(g, b, k0 + r, &row, &f, &pos);
                    const bf16_t* p = qkv + (long long)row * ld + C + h * HD + c * 8;
                    k = *(const bf16x8*)p;
                    v = *(const bf16x8*)(p + C);
                }
                if (c == 0) sF[r] = f;
                put8(sK, sKt, r, c, k);
                put8(sV, nullptr, r, c, v);
            }
            __syncthreads();
            f32x4 ds[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16x8 kf = *(const bf16x8*)&sK[(t * 16 + frow) * HD + fq * 8];
                const bf16x8 vf = *(const bf16x8*)&sV[(t * 16 + frow) * HD + fq * 8];
                const f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int key = t * 16 + fq * 4 + e;
                    float p = 0.f;
                    if (k0 + key < S) p = prob_exp2(fmaf(sc[e], QK_SCALE2, sTab[fqc - sF[key]]) - lse2);
                    if (sweep == 0) {
                        dl = fmaf(p, dp[e], dl);
                        ds[t][e] = 0.f;
                    } else {
                        ds[t][e] = p * (dp[e] - dl);
                    }
                }
            }
            if (sweep == 1) {
#pragma unroll
                for (int kk = 0; kk < NT / 2; ++kk) {
                    const bf16x8 dsf = pack_pair(ds[2 * kk], ds[2 * kk + 1]);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_pair(sKt, dt * 16 + frow, kk, fq), dsf, dq[dt], 0, 0, 0);
                }
            }
        }
        if (sweep == 0) {
            dl = quad_sum(dl);
            if (qv && fq == 0) delta[(long long)qrow * g.H + h] = dl;
        }
    }
    if (!qv) return;
    bf16_t* row = dqkv + (long long)qrow * ld + h * HD;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) store4(row + dt * 16 + fq * 4, dq[dt] * QK_SCALE);
}

// bwd 2: own = keys; the workgroup walks boxes [walk per_walk, (walk + 1) per_walk) in ascending order
__global__ __launch_bounds__(256) void swin3d_attn_bwd_dkv_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ table,
                                                                  const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                  const float* __restrict__ delta, bf16_t* __restrict__ dqkv,
                                                                  float* partial, int per_walk, const Geom3 g) {
    __shared__ float sTab[TAB_CAP];
    __shared__ __attribute__((aligned(16))) bf16_t sQ[TILE * HD], sdO[TILE * HD], sQt[HD * TILE], sdOt[HD * TILE];
    __shared__ int sF[TILE], sPos[TILE];
    __shared__ float sL[TILE], sD[TILE];
    const int walk = (int)blockIdx.x, h = (int)blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frow = lane & 15, fq = lane >> 4;
    const int C = g.H * HD, ld = 3 * C;
    load_table(sTab, table, g, h, tid);
    const int box0 = walk * per_walk, box1 = box0 + per_walk < g.nboxes ? box0 + per_walk : g.nboxes;
    float* pbase = partial ? partial + ((long long)walk * g.H + h) * g.Sw * g.Sw : nullptr;
    for (int box = box0; box < box1; ++box) {
        const Box b = box_of(g, box);
        const int S = b.S;
        for (int k0 = 0; k0 < S; k0 += TILE) {
            const int ki = k0 + wave * 16 + frow;
            const bool kv = ki < S;
            int krow, kf_, kpos;
            box_token(g, b, kv ? ki : S - 1, &krow, &kf_, &kpos);
            const bf16x8 kf = *(const bf16x8*)(qkv + (long long)krow * ld + C + h * HD + fq * 8);
            const bf16x8 vf = *(const bf16x8*)(qkv + (long long)krow * ld + 2 * C + h * HD + fq * 8);
            f32x4 dk[2], dv[2];
            dk[0] = dk[1] = dv[0] = dv[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int q0 = 0; q0 < S; q0 += TILE) {
                __syncthreads();      // the previous tile has been read
                {
                    const int r = tid >> 2, c = tid & 3;
                    bf16x8 q = zero8(), d = zero8();
                    int f = 0, pos = 0;
                    float l2 = 0.f, de = 0.f;
                    if (q0 + r < S) {
                        int row;
                        box_token(g, b, q0 + r, &row, &f, &pos);
                        q = *(const bf16x8*)(qkv + (long long)row * ld + h * HD + c * 8);
                        d = *(const bf16x8*)(dout + (long long)row * C + h * HD + c * 8);
                        if (c == 0) l2 = lse[(long long)row * g.H + h], de = delta[(long long)row * g.H + h];
                    }
                    if (c == 0) sF[r] = f + g.cst, sPos[r] = pos, sL[r] = l2, sD[r] = de;
                    put8(sQ, sQt, r, c, q);
                    put8(sdO, sdOt, r, c, d);
                }
                __syncthreads();
                f32x4 pa[NT], ds[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const bf16x8 qa = *(const bf16x8*)&sQ[(t * 16 + frow) * HD + fq * 8];
                    const bf16x8 da = *(const bf16x8*)&sdO[(t * 16 + frow) * HD + fq * 8];
                    const f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, vf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int qq = t * 16 + fq * 4 + e;
                        const bool valid = kv && q0 + qq < S;
                        float p = 0.f;
                        if (valid) p = prob_exp2(fmaf(sc[e], QK_SCALE2, sTab[sF[qq] - kf_]) - sL[qq]);
                        const float d = p * (dp[e] - sD[qq]);
                        pa[t][e] = p;
                        ds[t][e] = d;
                        if (pbase && valid) pbase[(long long)sPos[qq] * g.Sw + kpos] += d;
                    }
                }
#pragma unroll
                for (int kk = 0; kk < NT / 2; ++kk) {
                    const bf16x8 pf = pack_pair(pa[2 * kk], pa[2 * kk + 1]);
                    const bf16x8 dsf = pack_pair(ds[2 * kk], ds[2 * kk + 1]);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_pair(sdOt, dt * 16 + frow, kk, fq), pf, dv[dt], 0, 0, 0);
                        dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_pair(sQt, dt * 16 + frow, kk, fq), dsf, dk[dt], 0, 0, 0);
                    }
                }
            }
            if (kv) {
                bf16_t* row = dqkv + (long long)krow * ld + h * HD;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    store4(row + C + dt * 16 + fq * 4, dk[dt] * QK_SCALE);
                    store4(row + 2 * C + dt * 16 + fq * 4, dv[dt]);
                }
            }
        }
    }
}

__global__ void swin3d_zero_kernel(float* __restrict__ p, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

// dense[i] = sum over the walks, in ascending order, of partial[walk][i]
__global__ void swin3d_walk_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dense, int nwalks, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    for (int c = 0; c < nwalks; ++c) acc += partial[(long long)c * n + i];
    dense[i] = acc;
}

// dtable[r][h] += sum, over the lattice pairs with q - k = the displacement of r in ascending q, of dense[h][q][k]
__global__ void swin3d_table_fold_kernel(const float* __restrict__ dense, float* __restrict__ dtable, int Wt, int Wh, int Ww,
                                         const Geom3 g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.ntab * g.H) return;
    const int r = i / g.H, h = i - r * g.H;
    const int dt = r / (g.fh * g.fw) - (Wt - 1), r2 = r % (g.fh * g.fw), dh = r2 / g.fw - (Wh - 1), dw = r2 % g.fw - (Ww - 1);
    float acc = 0.f;
    const float* d = dense + (long long)h * g.Sw * g.Sw;
    for (int qt = dt > 0 ? dt : 0; qt < g.wt && qt - dt < g.wt; ++qt)
        for (int qh = dh > 0 ? dh : 0; qh < g.wh && qh - dh < g.wh; ++qh)
            for (int qw = dw > 0 ? dw : 0; qw < g.ww && qw - dw < g.ww; ++qw) {
                const int qpos = (qt * g.wh + qh) * g.ww + qw, kpos = ((qt - dt) * g.wh + qh - dh) * g.ww + qw - dw;
                acc += d[(long long)qpos * g.Sw + kpos];
            }
    dtable[i] += acc;
}

// the boxes a workgroup of bwd 2 walks, and the number of walks
int walks_of(int nboxes, int H, int* per_walk) {
    int n = (1024 + H - 1) / H;
    if (n > nboxes) n = nboxes;
    const int per = (nboxes + n - 1) / n;
    *per_walk = per;
    return (nboxes + per - 1) / per;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

int axis_ok(const char* who, const char* axis, int n, int w, int s, int W) {
    AIM_CHECK_ARG(w > 0 && w <= n && n % w == 0, "%s: window %d does not divide the %s extent %d", who, w, axis, n);
    AIM_CHECK_ARG(s >= 0 && s < w && !(s && w == n), "%s: %s shift %d outside [0, window %d), or on a window that spans the axis", who,
                  axis, s, w);
    AIM_CHECK_ARG(W >= w, "%s: the full %s window %d is smaller than the effective window %d", who, axis, W, w);
    return 0;
}

int make_geom(const char* who, Geom3* g, int B, int D, int G, int H, int wt, int wh, int ww, int st, int sh, int sw, int Wt, int Wh,
              int Ww) {
    AIM_CHECK_ARG(B > 0 && D > 0 && G > 0 && H > 0, "%s: unsupported shape clips=%d D=%d G=%d H=%d", who, B, D, G, H);
    if (int rc = axis_ok(who, "t", D, wt, st, Wt)) return rc;
    if (int rc = axis_ok(who, "h", G, wh, sh, Wh)) return rc;
    if (int rc = axis_ok(who, "w", G, ww, sw, Ww)) return rc;
    const long long Sw = (long long)wt * wh * ww, ntab = (2LL * Wt - 1) * (2LL * Wh - 1) * (2LL * Ww - 1);
    AIM_CHECK_ARG(Sw <= MAX_S, "%s: %lld tokens per window, at most %d", who, Sw, MAX_S);
    AIM_CHECK_ARG(ntab <= TAB_CAP, "%s: %lld table entries, at most %d", who, ntab, TAB_CAP);
    g->B = B, g->D = D, g->G = G, g->H = H, g->wt = wt, g->wh = wh, g->ww = ww, g->st = st, g->sh = sh, g->sw = sw;
    g->nbt = D / wt + (st ? 1 : 0), g->nbh = G / wh + (sh ? 1 : 0), g->nbw = G / ww + (sw ? 1 : 0);
    const long long rows = (long long)B * D * G * G, nbox = (long long)g->nbt * g->nbh * g->nbw;
    AIM_CHECK_ARG(rows * 3 * HD * H < 0x7fffffffLL && nbox * B * H < 0x7fffffffLL, "%s: %lld rows of %d heads are too many", who, rows, H);
    g->nbox = (int)nbox, g->nboxes = (int)(nbox * B);
    g->fh = 2 * Wh - 1, g->fw = 2 * Ww - 1;
    g->cst = ((Wt - 1) * g->fh + Wh - 1) * g->fw + Ww - 1, g->ntab = (int)ntab, g->Sw = (int)Sw;
    return 0;
}

}  // namespace

extern "C" int64_t aim_swin3d_attn_bwd_workspace_bytes(int clips, int D, int G, int H, int wt, int wh, int ww, int st, int sh, int sw) {
    if (clips <= 0 || D <= 0 || G <= 0 || H <= 0 || wt <= 0 || wh <= 0 || ww <= 0 || D % wt || G % wh || G % ww) return 0;
    const long long nboxes = (long long)clips * (D / wt + (st ? 1 : 0)) * (G / wh + (sh ? 1 : 0)) * (G / ww + (sw ? 1 : 0));
    const long long Sw = (long long)wt * wh * ww;
    if (nboxes >= 0x7fffffffLL || Sw > MAX_S) return 0;
    int per = 0;
    return ((int64_t)walks_of((int)nboxes, H, &per) + 1) * H * Sw * Sw * 4;
}

extern "C" int aim_swin3d_attn_fwd(const aim_bf16* qkv, const float* table, aim_bf16* out, float* lse, int clips, int D, int G, int H,
                                   int wt, int wh, int ww, int st, int sh, int sw, int Wt, int Wh, int Ww, void* stream) {
    const char* who = "swin3d_attn_fwd";
    Geom3 g;
    if (int rc = make_geom(who, &g, clips, D, G, H, wt, wh, ww, st, sh, sw, Wt, Wh, Ww)) return rc;
    AIM_CHECK_ARG(qkv && table && out && lse, "%s: null pointer", who);
    AIM_CHECK_ARG(aligned16(qkv) && aligned16(out), "%s: qkv and out must be 16-byte aligned", who);
    AIM_CHECK_ARG(aligned4(table) && aligned4(lse), "%s: table and lse must be 4-byte aligned", who);
    const dim3 grid((unsigned)(g.nboxes * g.H), (unsigned)((g.Sw + TILE - 1) / TILE));
    hipLaunchKernelGGL(swin3d_attn_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, table, (bf16_t*)out, lse, g);
    AIM_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int aim_swin3d_attn_bwd(const aim_bf16* qkv, const float* table, const aim_bf16* dout, const float* lse, float* delta,
                                   aim_bf16* dqkv, float* dtable, int clips, int D, int G, int H, int wt, int wh, int ww, int st,
                                   int sh, int sw, int Wt, int Wh, int Ww, float* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "swin3d_attn_bwd";
    Geom3 g;
    if (int rc = make_geom(who, &g, clips, D, G, H, wt, wh, ww, st, sh, sw, Wt, Wh, Ww)) return rc;
    AIM_CHECK_ARG(qkv && table && dout && lse && delta && dqkv, "%s: null pointer", who);
    AIM_CHECK_ARG(aligned16(qkv) && aligned16(dout) && aligned16(dqkv), "%s: the bf16 buffers must be 16-byte aligned", who);
    AIM_CHECK_ARG(aligned4(table) && aligned4(lse) && aligned4(delta) && aligned4(dtable), "%s: the fp32 buffers must be 4-byte aligned", who);
    int per = 0;
    const int nwalks = walks_of(g.nboxes, g.H, &per);
    const long long n = (long long)g.H * g.Sw * g.Sw;
    if (dtable) {
        const long long need = ((long long)nwalks + 1) * n * 4;
        AIM_CHECK_ARG(workspace && workspace_bytes >= need, "%s: the table gradient needs a workspace of %lld bytes", who, need);
        AIM_CHECK_ARG(aligned4(workspace), "%s: the workspace must be 4-byte aligned", who);
    }
    float* partial = dtable ? workspace : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (partial) {
        const long long m = (long long)nwalks * n;
        hipLaunchKernelGGL(swin3d_zero_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, partial, m);
        AIM_CHECK_LAUNCH(who);
    }
    const dim3 grid1((unsigned)(g.nboxes * g.H), (unsigned)((g.Sw + TILE - 1) / TILE));
    hipLaunchKernelGGL(swin3d_attn_bwd_dq_kernel, grid1, dim3(256), 0, s, (const bf16_t*)qkv, table, (const bf16_t*)dout, lse, delta,
                       (bf16_t*)dqkv, g);
    AIM_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(swin3d_attn_bwd_dkv_kernel, dim3((unsigned)nwalks, (unsigned)g.H), dim3(256), 0, s, (const bf16_t*)qkv, table,
                       (const bf16_t*)dout, lse, (const float*)delta, (bf16_t*)dqkv, partial, per, g);
    AIM_CHECK_LAUNCH(who);
    if (partial) {
        float* dense = partial + (long long)nwalks * n;
        hipLaunchKernelGGL(swin3d_walk_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, partial, dense, nwalks, (int)n);
        AIM_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(swin3d_table_fold_kernel, dim3((unsigned)((g.ntab * g.H + 127) / 128)), dim3(128), 0, s, dense, dtable, Wt, Wh,
                           Ww, g);
        AIM_CHECK_LAUNCH(who);
    }
    return 0;
}
