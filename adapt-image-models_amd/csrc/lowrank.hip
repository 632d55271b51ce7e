// Fused low-rank (bottleneck) linear adapters: two chained bf16 MFMA products whose r-wide intermediate never leaves the
// workgroup.  gfx950 only.  ZeroI2V's Linear_Adapter (reference vit_clip_zeroI2V.py:15-38) is LA(x) = x + D_fc2(D_fc1(x)) with
// no activation between the two layers and r <= 256 hidden units beside D = 768 / 1024: as separate GEMMs both products are
// byte-bound (K or N = r), and the [M, D] input, the skip term and the output each cross memory once per call.
//
//   aim_lowrank_fwd   H_g = bf16(X W1_g^T + b1_g)               Y_g = alpha X + H_g W2_g^T + b2_g         g < G, G in {1, 3}
//   aim_lowrank_bwd   dH_g = bf16(dY_g W2_g)                    dX = bf16(alpha sum_g dY_g + sum_g dH_g W1_g)
//
// Both are ONE kernel template: per adapter a first product over K = D whose [rows, r] result is rounded to bf16, stored to
// memory (the weight gradients read it) and written into an LDS image, and a second product over K = r that reads that image
// as its A operand.  Every weight is taken K-contiguous ([n][k], the GEMMs' convention), so the backward is handed W2^T and
// W1^T (the copies the dgrad GEMMs of this library use anyway).
//
// A workgroup owns BM rows: 128 in the forward (one H image at a time: first product, second product, next adapter; 8 waves),
// 64 in the backward (all G images stay resident, because the second product sums over the adapters into one accumulator;
// 8 waves), 32 with 4 waves where three resident images of r > 192 leave no room for 64.  Every workgroup streams both weight
// matrices of an adapter from L2, so the rows per workgroup set the on-chip traffic per row.  First product: waves as
// NW / 4 (M) x 4 (N), a wave takes the 16-column tiles {w, w + 4, ...} of H.  Second product: a 64-column chunk of the output at
// a time, waves as NW / 2 (M) x 2 (N).  Both stream their tiles through a two-slot LDS ring (LDS-DMA, the XOR-swizzled
// 128-byte-row image of aim_common.h); the tile of step s + 1 is in flight while step s multiplies.
// LDS at r = 256: forward 64 KiB (H) + 2 x 48 KiB = the 160 KiB of a CU; backward at G = 3: 3 x 16 KiB (dH) + 2 x 36 KiB.
//
// Memory traffic: the X rows of a workgroup (at most 128 x D bf16 = 256 KiB) are staged once per adapter and read once more by
// the epilogue for the skip term; after the first pass they are served by the L2 of the workgroup's XCD, so X crosses HBM once
// for all G adapters.  The same holds for each dY_g in the backward.  No atomics, one fixed summation order: reruns give
// equal bits.
#include "aim_common.h"
#include "aim_kernels_internal.h"

namespace {

typedef aim_lowrank_args LrArgs;

template <typename T>
__device__ __forceinline__ T sel3(T const (&p)[3], int g) {
    return g == 0 ? p[0] : (g == 1 ? p[1] : p[2]);      // (a run-time index into the argument block would send it to scratch)
}

template <int MT, bool BWD, int NW>
__global__ __launch_bounds__(NW * 64) void lowrank_kernel(LrArgs a, int rk) {
    constexpr int BM = MT * 16;
    constexpr int MTW = MT / (NW / 4);                  // M tiles of a wave in the first product: waves as NW / 4 (M) x 4 (N)
    constexpr int MI = MT / (NW / 2);                   // ... and in the second: waves as NW / 2 (M) x 2 (N)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    AIM_LDS char* smem = (AIM_LDS char*)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fq = lane >> 4;
    const int wq = wave & 3, wh = wave >> 2;
    const int srow = lane >> 3, schunk = (lane & 7) ^ srow;
    const int D = a.D, r = a.r, G = a.G;
    const long long m0 = (long long)blockIdx.x * BM;
    const int rows = (a.M - m0) < BM ? (int)(a.M - m0) : BM;
    const int hbytes = BM * rk * 128;                   // one adapter's H image: rk K-chunks of [BM rows][128 B]
    const int stage_bytes = (BM + rk * 64) * 128;       // ring slot: a 64-wide K-step of the rows + of r (padded) weight rows
    AIM_LDS char* sH = smem;
    AIM_LDS char* sS = smem + (BWD ? G : 1) * hbytes;
    const int nk = D >> 6;

    for (int g = 0; g < G; ++g) {
        // ---------------- first product: H_g [BM, r] = X_g [BM, D] . Wa_g [r, D]^T ----------------
        AIM_LDS char* sHg = sH + (BWD ? g : 0) * hbytes;
        {
            const bf16_t* Xg = (const bf16_t*)(BWD ? sel3(a.x, g) : a.x[0]) + m0 * a.ldx;
            const __amdgpu_buffer_rsrc_t rX = make_rsrc(Xg, ((long long)(rows - 1) * a.ldx + D) * 2);
            const __amdgpu_buffer_rsrc_t rW = make_rsrc(sel3(a.wa, g), (long long)r * D * 2);
            const int npieces = MT * 2 + rk * 8;        // pieces of 8 rows x 128 B: the rows first, then the weight rows
            auto stage1 = [&](int slot, int kt) {
                const unsigned k0b = (unsigned)(kt * 128 + schunk * 16);
                for (int p = wave; p < npieces; p += NW) {
                    AIM_LDS char* dst = sS + slot * stage_bytes + p * 1024;
                    if (p < MT * 2) {
                        const int row = p * 8 + srow;
                        stage_piece(rX, dst, row < rows ? (unsigned)(row * a.ldx * 2) + k0b : AIM_OOB);
                    } else {
                        const int row = (p - MT * 2) * 8 + srow;
                        stage_piece(rW, dst, row < r ? (unsigned)(row * D * 2) + k0b : AIM_OOB);
                    }
                }
            };
            f32x4 acc[MTW][4];
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            stage1(0, 0);
            for (int kt = 0; kt < nk; ++kt) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();                        // step kt has landed; every wave is past its reads of the other slot
                if (kt + 1 < nk) stage1((kt + 1) & 1, kt + 1);
                const AIM_LDS char* sA = sS + (kt & 1) * stage_bytes;
                const AIM_LDS char* sW = sA + BM * 128;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 af[MTW];
#pragma unroll
                    for (int i = 0; i < MTW; ++i) af[i] = lds_read8(sA + swz_off((wh * MTW + i) * 16 + frow, ks * 4 + fq));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < rk) {
                            const bf16x8 wf = lds_read8(sW + swz_off((wq + 4 * j) * 16 + frow, ks * 4 + fq));
#pragma unroll
                            for (int i = 0; i < MTW; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[i], acc[i][j], 0, 0, 0);
                        }
                    }
                }
            }
            // H = bf16(acc + bias): into the LDS image (zero in the columns that pad r to 64s) and to memory
            const float* ba = BWD ? nullptr : sel3(a.ba, g);
            bf16_t* hg = (bf16_t*)sel3(a.h, g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= rk) continue;
                const int n = (wq + 4 * j) * 16 + fq * 4;
                const bool live = n < r;                // r is a multiple of 8: the four columns are in or out together
                const f32x4 b = (live && ba) ? *(const f32x4*)(ba + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < MTW; ++i) {
                    const int m = (wh * MTW + i) * 16 + frow;
                    const bf16x4 h4 = live ? pack4(acc[i][j][0] + b[0], acc[i][j][1] + b[1], acc[i][j][2] + b[2], acc[i][j][3] + b[3])
                                           : pack4(0.f, 0.f, 0.f, 0.f);
                    *(AIM_LDS bf16x4*)(sHg + (n >> 6) * (BM * 128) + swz_off(m, (n & 63) >> 3) + (n & 7) * 2) = h4;
                    if (hg && live && m < rows) *(bf16x4*)(hg + (m0 + m) * a.ldh + n) = h4;
                }
            }
            __syncthreads();                            // the image is whole; the ring is free
        }
        if (BWD && g + 1 < G) continue;                 // backward: every dH first, then one second product over all of them

        // ---------------- second product: out [BM, D] (+)= H [BM, r] . Wb [D, r]^T, 64 output columns per step ----------------
        const int ng = BWD ? G : 1;
        const int nsteps = nk * ng;
        const int wm = wave >> 1, wn = wave & 1;
        auto stage2 = [&](int slot, int s) {
            const int nc = s / ng, gi = BWD ? s - nc * ng : g;
            const __amdgpu_buffer_rsrc_t rB = make_rsrc(sel3(a.wb, gi), (long long)D * r * 2);
            for (int p = wave; p < rk * 8; p += NW) {  // piece p: K-chunk p / 8, weight rows 8 (p % 8) ..
                const int col = (p >> 3) * 64 + schunk * 8;
                const int row = nc * 64 + (p & 7) * 8 + srow;
                stage_piece(rB, sS + slot * stage_bytes + p * 1024, col < r ? (unsigned)((row * r + col) * 2) : AIM_OOB);
            }
        };
        f32x4 acc[MI][2];
        stage2(0, 0);
        for (int s = 0; s < nsteps; ++s) {
            const int nc = s / ng, gi = BWD ? s - nc * ng : g;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            // what this chunk's epilogue adds -- the skip rows (L2: this workgroup staged them), the fp32 residual -- is asked
            // for here, ahead of the next tile's DMA and of the MFMAs, so that its latency passes under them
            const bool last = !BWD || gi + 1 == ng;
            bf16x4 xs[BWD ? 3 : 1][MI][2];
            f32x4 rs[MI][2];
            if (last) {
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const int m = (wm * MI + i) * 16 + frow;
                    if (m >= rows) continue;
                    const long long mg = m0 + m;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int n = nc * 64 + wn * 32 + j * 16 + fq * 4;
#pragma unroll
                        for (int q = 0; q < (BWD ? 3 : 1); ++q)
                            if (q < G) xs[q][i][j] = *(const bf16x4*)((const bf16_t*)(BWD ? sel3(a.x, q) : a.x[0]) + mg * a.ldx + n);
                        if (!BWD && a.y32) rs[i][j] = *(const f32x4*)(a.resid + mg * a.ldr + n);
                    }
                }
            }
            if (s + 1 < nsteps) stage2((s + 1) & 1, s + 1);
            if (!BWD || gi == 0) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const AIM_LDS char* sB = sS + (s & 1) * stage_bytes;
            const AIM_LDS char* sA = sH + (BWD ? gi : 0) * hbytes;
            for (int kc = 0; kc < rk; ++kc) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 af[MI], wf[2];
#pragma unroll
                    for (int i = 0; i < MI; ++i) af[i] = lds_read8(sA + kc * (BM * 128) + swz_off((wm * MI + i) * 16 + frow, ks * 4 + fq));
#pragma unroll
                    for (int j = 0; j < 2; ++j) wf[j] = lds_read8(sB + kc * 8192 + swz_off(wn * 32 + j * 16 + frow, ks * 4 + fq));
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
                }
            }
            if (!last) continue;
            // epilogue of this 64-column chunk
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int m = (wm * MI + i) * 16 + frow;
                if (m >= rows) continue;
                const long long mg = m0 + m;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int n = nc * 64 + wn * 32 + j * 16 + fq * 4;
                    float v[4];
                    if constexpr (BWD) {
                        float sx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            if (q >= G) continue;
#pragma unroll
                            for (int e = 0; e < 4; ++e) sx[e] += (float)xs[q][i][j][e];
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(a.alpha, sx[e], acc[i][j][e]);
                        *(bf16x4*)((bf16_t*)a.y[0] + mg * a.ldy + n) = pack4(v[0], v[1], v[2], v[3]);
                    } else {
                        const bf16x4 x4 = xs[0][i][j];
                        const float* bb = sel3(a.bb, g);
                        const f32x4 b = bb ? *(const f32x4*)(bb + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(a.alpha, (float)x4[e], acc[i][j][e] + b[e]);
                        bf16_t* yg = (bf16_t*)sel3(a.y, g);
                        if (yg) *(bf16x4*)(yg + mg * a.ldy + n) = pack4(v[0], v[1], v[2], v[3]);
                        if (a.y32)
                            *(f32x4*)(a.y32 + mg * a.ld32 + n) =
                                f32x4{rs[i][j][0] + v[0], rs[i][j][1] + v[1], rs[i][j][2] + v[2], rs[i][j][3] + v[3]};
                    }
                }
            }
        }
        __syncthreads();                                // the next adapter's first product re-uses the image and the ring
    }
}

bool aligned(const void* p, int n) { return ((uintptr_t)p & (uintptr_t)(n - 1)) == 0; }

int check_common(const char* who, const LrArgs* a) {
    AIM_CHECK_ARG(a != nullptr, "%s: no arguments", who);
    AIM_CHECK_ARG(a->G == 1 || a->G == 3, "%s: G must be 1 or 3 (G=%d)", who, a->G);
    AIM_CHECK_ARG(a->M >= 1, "%s: M must be at least 1 (M=%d)", who, a->M);
    AIM_CHECK_ARG(a->D >= 64 && a->D % 64 == 0 && a->D <= 8192, "%s: D must be a multiple of 64 in [64, 8192] (D=%d)", who, a->D);
    AIM_CHECK_ARG(a->r >= 8 && a->r % 8 == 0 && a->r <= 256, "%s: r must be a multiple of 8 in [8, 256] (r=%d)", who, a->r);
    AIM_CHECK_ARG(a->ldx >= a->D && a->ldx % 8 == 0 && (long long)a->ldx * 2 * 128 < 0x7fffffffLL,
                  "%s: ldx must be a multiple of 8, at least D and below 2^22 (ldx=%d)", who, a->ldx);
    AIM_CHECK_ARG(a->ldh >= a->r && a->ldh % 4 == 0, "%s: ldh must be a multiple of 4 and at least r (ldh=%d)", who, a->ldh);
    AIM_CHECK_ARG(a->ldy >= a->D && a->ldy % 4 == 0, "%s: ldy must be a multiple of 4 and at least D (ldy=%d)", who, a->ldy);
    for (int g = 0; g < a->G; ++g) {
        AIM_CHECK_ARG(a->wa[g] && a->wb[g] && aligned(a->wa[g], 16) && aligned(a->wb[g], 16),
                      "%s: the weights of adapter %d must be 16-byte aligned device pointers", who, g);
        AIM_CHECK_ARG(aligned(a->h[g], 8) && aligned(a->y[g], 8), "%s: h / y of adapter %d must be 8-byte aligned", who, g);
    }
    return 0;
}

constexpr int LDS_MAX = 160 * 1024;

// LDS bytes of a workgroup of MT 16-row tiles: the H image(s) and the two ring slots
int lds_bytes(int MT, bool bwd, int G, int r) {
    const int BM = MT * 16, rk = (r + 63) / 64;
    return (bwd ? G : 1) * BM * rk * 128 + 2 * (BM + rk * 64) * 128;
}

template <int MT, bool BWD, int NW>
int launch(const LrArgs& a, hipStream_t st, const char* who) {
    constexpr int BM = MT * 16;
    const int lds = lds_bytes(MT, BWD, a.G, a.r);
    AIM_CHECK_ARG(lds <= LDS_MAX, "%s: %d bytes of LDS", who, lds);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)lowrank_kernel<MT, BWD, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        attr_set = true;
    }
    hipLaunchKernelGGL((lowrank_kernel<MT, BWD, NW>), dim3((a.M + BM - 1) / BM), dim3(NW * 64), lds, st, a, (a.r + 63) / 64);
    AIM_CHECK_LAUNCH(who);
    return 0;
}

}  // namespace

extern "C" int aim_lowrank_fwd(const aim_lowrank_args* a, void* stream) {
    const char* who = "aim_lowrank_fwd";
    if (check_common(who, a)) return 1;
    AIM_CHECK_ARG(a->alpha == 1.f || a->alpha == 2.f, "%s: alpha must be 1 or 2 (alpha=%g)", who, (double)a->alpha);
    AIM_CHECK_ARG(a->x[0] && aligned(a->x[0], 16), "%s: x must be a 16-byte aligned device pointer", who);
    if (a->y32) {
        AIM_CHECK_ARG(a->G == 1, "%s: the fp32 output form takes one adapter (G=%d)", who, a->G);
        AIM_CHECK_ARG(a->resid && aligned(a->y32, 16) && aligned(a->resid, 16) && a->ld32 >= a->D && a->ld32 % 4 == 0 &&
                          a->ldr >= a->D && a->ldr % 4 == 0,
                      "%s: the fp32 output form needs resid, 16-byte aligned pointers and row strides that are multiples of 4", who);
    }
    for (int g = 0; g < a->G; ++g) {
        AIM_CHECK_ARG(a->y[g] || (a->y32 && g == 0), "%s: adapter %d has no output", who, g);
        AIM_CHECK_ARG(aligned(a->ba[g], 16) && aligned(a->bb[g], 16), "%s: the biases of adapter %d must be 16-byte aligned", who, g);
    }
    return launch<8, false, 8>(*a, (hipStream_t)stream, who);
}

extern "C" int aim_lowrank_bwd(const aim_lowrank_args* a, void* stream) {
    const char* who = "aim_lowrank_bwd";
    if (check_common(who, a)) return 1;
    AIM_CHECK_ARG(a->alpha == 1.f || a->alpha == 2.f, "%s: alpha must be 1 or 2 (alpha=%g)", who, (double)a->alpha);
    AIM_CHECK_ARG(a->y[0] != nullptr, "%s: no dX", who);
    for (int g = 0; g < a->G; ++g) {
        AIM_CHECK_ARG(a->x[g] && aligned(a->x[g], 16), "%s: dY of adapter %d must be a 16-byte aligned device pointer", who, g);
        AIM_CHECK_ARG(a->h[g] != nullptr, "%s: dH of adapter %d is an output the weight gradients need", who, g);
    }
    // 64 rows per workgroup where the G resident dH images leave room for the ring (not at G = 3, r > 192), else 32
    if (lds_bytes(4, true, a->G, a->r) <= LDS_MAX) return launch<4, true, 8>(*a, (hipStream_t)stream, who);
    return launch<2, true, 4>(*a, (hipStream_t)stream, who);
}
