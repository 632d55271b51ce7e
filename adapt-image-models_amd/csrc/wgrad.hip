// Weight-gradient GEMM for the trainable adapters:  dW[n][k] += sum_m G[m][n] * A[m][k].  gfx950 only.
//
// Autograd counterpart of Adapter.D_fc1 / D_fc2 (reference vit_clip.py:57-58, 62-64); the reference
// gets it from torch autograd (addmm backward).  Both operands are row-major with the REDUCTION index
// m as the slow dimension, so neither can be read as a k-contiguous MFMA fragment.  The tiles are
// staged untransposed ([m][n] and [m][k], coalesced) into swizzled LDS images and the fragments are
// fetched with ds_read_b64_tr_b16, the hardware transposing read: no transposed copies in HBM.
//
// Block tile 256(n) x 256(k), 8 waves as 2x4, wave tile 128x64 = 8x4 MFMA 16x16x32 tiles, 4-stage LDS ring.
// The M dimension is split over blockIdx.y in chunks; partial tiles go to a caller-provided scratch slab and
// are summed by a second kernel (no atomics), or are combined with fp32 atomics when no scratch is given.
#include "aim_common.h"
#include <stdlib.h>
#include "aim_kernels_internal.h"
#include "wgrad_tile.h"

namespace {

using wgrad_tile::MSTEP;
using wgrad_tile::NST;
using wgrad_tile::STAGE_BYTES;
using wgrad_tile::TILE;

// One workgroup = one output tile x one M-chunk (wgrad_tile.h holds the body: the rider workgroups of the persistent GEMM
// run the same function).  row0: the row of the whole problem that G / A row 0 is (the `at` factors are at[(row0 + m) % ntok]).
__global__ __launch_bounds__(512) void wgrad_kernel(const bf16_t* __restrict__ G, int ldg, const bf16_t* __restrict__ A,
                                                    int lda, float* __restrict__ dW, int lddw, float* __restrict__ partial,
                                                    int M, int Nw, int Kw, int chunk, float* __restrict__ db,
                                                    float* __restrict__ bias_partial, const float* __restrict__ at, int ntok,
                                                    int row0) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    AIM_LDS char* smem = (AIM_LDS char*)smem_raw;
    const int tiles_k = (Kw + TILE - 1) / TILE;
    const int tiles = ((Nw + TILE - 1) / TILE) * tiles_k;
    const int cidx = blockIdx.x / tiles, tix = blockIdx.x - cidx * tiles;
    const int tn = tix / tiles_k, tk = tix - tn * tiles_k;
    const int mbeg = cidx * chunk;
    const int mend = min(M, mbeg + chunk);
    if (mbeg >= mend) return;
    wgrad_tile::run<false>(smem, G, ldg, A, lda, dW, lddw, partial ? partial + (long long)cidx * Nw * Kw : nullptr, Nw, Kw, tn, tk,
                           mbeg, mend, row0, db != nullptr, db, bias_partial ? bias_partial + (long long)cidx * Nw : nullptr, at, ntok);
}

// dW[n][k] += sum_c slab[c][n][k]  and  db[n] += sum_c bias_slab[c][n], both in chunk order (bitwise reproducible).
// A thread owns four consecutive outputs and walks the chunks with eight independent 16-byte loads in flight (the first
// version issued one dependent 4-byte load per chunk: latency-bound at 80 us for 50 MB).
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float* __restrict__ partial, float* __restrict__ dW,
                                                           int lddw, int nchunks, int Nw, int Kw,
                                                           const float* __restrict__ bias_partial, float* __restrict__ db) {
    const long long total = (long long)Nw * Kw;
    const long long idx = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (idx < total) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        int c = 0;
        for (; c + 8 <= nchunks; c += 8) {
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *(const f32x4*)(partial + (long long)(c + j) * total + idx);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];
        }
        for (; c < nchunks; ++c) acc += *(const f32x4*)(partial + (long long)c * total + idx);
        const int n = (int)(idx / Kw), k = (int)(idx - (long long)n * Kw);      // Kw % 8 == 0: the four outputs share a row
        f32x4* o = (f32x4*)(dW + (long long)n * lddw + k);
        *o = *o + acc;
    }
    if (bias_partial) {          // a wave per bias column, four columns per block: chunk-strided loads, fixed-order wave sum
        const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (n < Nw) {
            float a = 0.f;
            for (int c = lane; c < nchunks; c += 64) a += bias_partial[(long long)c * Nw + n];
            a = wave_sum(a);
            if (lane == 0) db[n] += a;
        }
    }
}

// (A/B reference, AIM_WGRAD_FINISH_V=0) one output per thread, one dependent load per chunk
__global__ __launch_bounds__(256) void wgrad_finish1_kernel(const float* __restrict__ partial, float* __restrict__ dW,
                                                            int lddw, int nchunks, int Nw, int Kw) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)Nw * Kw;
    if (idx >= total) return;
    float acc = 0.f;
    for (int c = 0; c < nchunks; ++c) acc += partial[(long long)c * total + idx];
    const int n = (int)(idx / Kw), k = (int)(idx - (long long)n * Kw);
    dW[(long long)n * lddw + k] += acc;
}

}  // namespace

static int wgrad_chunks(int M, int tiles, int* chunk_out) {
    // Target workgroup count.  256 = one per CU is fastest stand-alone; the framework runs these launches on a stream
    // of their own beside MFMA-bound GEMMs, where fewer, longer workgroups mean fewer partial slabs to write and sum.
    static const int target = [] { const char* e = getenv("AIM_WGRAD_WGS"); const int v = e ? atoi(e) : 256; return v > 0 ? v : 256; }();
    int nchunks = (target + tiles - 1) / tiles;
    const int maxchunks = (M + MSTEP - 1) / MSTEP;
    if (nchunks > maxchunks) nchunks = maxchunks;
    int chunk = (M + nchunks - 1) / nchunks;
    chunk = ((chunk + MSTEP - 1) / MSTEP) * MSTEP;
    if (chunk_out) *chunk_out = chunk;
    return (M + chunk - 1) / chunk;
}

extern "C" int64_t aim_wgrad_workspace_bytes(int M, int Nw, int Kw) {
    const int tiles = ((Nw + TILE - 1) / TILE) * ((Kw + TILE - 1) / TILE);
    const int nchunks = wgrad_chunks(M, tiles, nullptr);
    return nchunks > 1 ? (int64_t)nchunks * Nw * (Kw + 1) * 4 : 0;      // weight slabs + one bias row per chunk
}

extern "C" int aim_wgrad_bias_bf16(const aim_bf16* G, int ldg, const aim_bf16* A, int lda, float* dW, int lddw, float* db,
                                   const float* at, int ntok, int M, int Nw, int Kw, float* workspace, int64_t workspace_bytes,
                                   void* stream) {
    AIM_CHECK_ARG(M > 0 && Nw > 0 && Kw > 0 && (Nw % 8) == 0 && (Kw % 8) == 0, "wgrad: Nw/Kw must be positive multiples of 8 (Nw=%d Kw=%d)", Nw, Kw);
    AIM_CHECK_ARG((ldg % 8) == 0 && (lda % 8) == 0 && (lddw % 4) == 0, "wgrad: ldg/lda must be multiples of 8, lddw of 4");
    AIM_CHECK_ARG(ldg >= Nw && lda >= Kw && lddw >= Kw, "wgrad: ldg/lda/lddw must cover a row (ldg=%d lda=%d lddw=%d)", ldg, lda, lddw);
    AIM_CHECK_ARG(G && A && dW, "wgrad: null pointer");
    AIM_CHECK_ARG(!at || (db && ntok > 0 && ntok <= 4096), "wgrad: row factors need db and 0 < ntok <= 4096");
    const int tiles = ((Nw + TILE - 1) / TILE) * ((Kw + TILE - 1) / TILE);
    int chunk = 0;
    const int nchunks = wgrad_chunks(M, tiles, &chunk);
    const int lds_bytes = NST * STAGE_BYTES + (at ? ((ntok * 4 + 15) & ~15) : 0);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)wgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    AIM_CHECK_ARG((long long)chunk * (ldg > lda ? ldg : lda) * 2 < 0x7fffffffLL, "wgrad: chunk too large");
    float* slab = (workspace && nchunks > 1 && workspace_bytes >= (int64_t)nchunks * Nw * (Kw + 1) * 4) ? workspace : nullptr;
    static const bool fuse_bias = [] { const char* e = getenv("AIM_WGRAD_FUSE_BIAS"); return !e || atoi(e) != 0; }();
    static const bool finish_v = [] { const char* e = getenv("AIM_WGRAD_FINISH_V"); return !e || atoi(e) != 0; }();
    float* bias_slab = (slab && db && fuse_bias) ? slab + (long long)nchunks * Nw * Kw : nullptr;
    if (db && nchunks > 1 && !bias_slab) {       // no scratch: the bias through the stand-alone column sum (atomics inside)
        const int rc = aim_colsum_bf16(G, ldg, nullptr, at, ntok, db, M, Nw, nullptr, 0, stream);
        if (rc) return rc;
        db = nullptr;
    }
    hipLaunchKernelGGL(wgrad_kernel, dim3(tiles * nchunks), dim3(512), lds_bytes, (hipStream_t)stream,
                       (const bf16_t*)G, ldg, (const bf16_t*)A, lda, dW, lddw, slab, M, Nw, Kw, chunk, db, bias_slab, at, ntok, 0);
    AIM_CHECK_LAUNCH("aim_wgrad_bf16");
    if (slab) {
        const long long total = (long long)Nw * Kw;
        unsigned fgrid = (unsigned)((total / 4 + 255) / 256);
        if (bias_slab && (unsigned)((Nw + 3) / 4) > fgrid) fgrid = (unsigned)((Nw + 3) / 4);
        if (finish_v || bias_slab)
            hipLaunchKernelGGL(wgrad_finish_kernel, dim3(fgrid), dim3(256), 0, (hipStream_t)stream,
                               slab, dW, lddw, nchunks, Nw, Kw, bias_slab, db);
        else
            hipLaunchKernelGGL(wgrad_finish1_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                               slab, dW, lddw, nchunks, Nw, Kw);
        AIM_CHECK_LAUNCH("aim_wgrad_bf16(finish)");
    }
    return 0;
}

extern "C" int aim_wgrad_bf16(const aim_bf16* G, int ldg, const aim_bf16* A, int lda, float* dW, int lddw, float* db,
                              int M, int Nw, int Kw, float* workspace, int64_t workspace_bytes, void* stream) {
    return aim_wgrad_bias_bf16(G, ldg, A, lda, dW, lddw, db, nullptr, 0, M, Nw, Kw, workspace, workspace_bytes, stream);
}

static void wgrad_attr() {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)wgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
}

extern "C" int aim_wgrad_slabs_bf16(const aim_bf16* G, int ldg, const aim_bf16* A, int lda, const float* at, int ntok, int m_begin,
                                    int m_end, int Nw, int Kw, float* slabs, float* bias_slabs, int max_chunks, int* chunks_written,
                                    void* stream) {
    AIM_CHECK_ARG(Nw > 0 && Kw > 0 && (Nw % 8) == 0 && (Kw % 8) == 0, "wgrad_slabs: Nw/Kw must be positive multiples of 8 (Nw=%d Kw=%d)", Nw, Kw);
    AIM_CHECK_ARG((ldg % 8) == 0 && (lda % 8) == 0, "wgrad_slabs: ldg/lda must be multiples of 8");
    AIM_CHECK_ARG(ldg >= Nw && lda >= Kw, "wgrad_slabs: ldg/lda must cover a row (ldg=%d lda=%d)", ldg, lda);
    AIM_CHECK_ARG(G && A && slabs && chunks_written, "wgrad_slabs: null pointer");
    AIM_CHECK_ARG(m_begin >= 0 && m_end > m_begin, "wgrad_slabs: empty row range [%d, %d)", m_begin, m_end);
    AIM_CHECK_ARG(!at || (bias_slabs && ntok > 0 && ntok <= 4096), "wgrad_slabs: row factors need bias slabs and 0 < ntok <= 4096");
    const int rows = m_end - m_begin;
    const int tiles = ((Nw + TILE - 1) / TILE) * ((Kw + TILE - 1) / TILE);
    int chunk = 0;
    const int nchunks = max_chunks > 0 ? aim_wgrad_range_chunks(rows, max_chunks, &chunk) : wgrad_chunks(rows, tiles, &chunk);
    AIM_CHECK_ARG((long long)chunk * (ldg > lda ? ldg : lda) * 2 < 0x7fffffffLL, "wgrad_slabs: chunk too large");
    wgrad_attr();
    const int lds_bytes = NST * STAGE_BYTES + (at ? ((ntok * 4 + 15) & ~15) : 0);
    // db only says "sum the bias columns": with a bias slab the kernel never touches it
    hipLaunchKernelGGL(wgrad_kernel, dim3(tiles * nchunks), dim3(512), lds_bytes, (hipStream_t)stream,
                       (const bf16_t*)G + (long long)m_begin * ldg, ldg, (const bf16_t*)A + (long long)m_begin * lda, lda,
                       (float*)nullptr, 0, slabs, rows, Nw, Kw, chunk, bias_slabs, bias_slabs, at, ntok, m_begin);
    AIM_CHECK_LAUNCH("aim_wgrad_slabs_bf16");
    *chunks_written = nchunks;
    return 0;
}

extern "C" int aim_wgrad_finish(const float* slabs, const float* bias_slabs, int nchunks, float* dW, int lddw, float* db, int Nw,
                                int Kw, void* stream) {
    AIM_CHECK_ARG(slabs && dW && nchunks > 0, "wgrad_finish: null pointer or no slabs");
    AIM_CHECK_ARG(Nw > 0 && Kw > 0 && (Nw % 8) == 0 && (Kw % 8) == 0 && (lddw % 4) == 0, "wgrad_finish: Nw/Kw multiples of 8, lddw of 4");
    AIM_CHECK_ARG((bias_slabs != nullptr) == (db != nullptr), "wgrad_finish: bias slabs and db go together");
    const long long total = (long long)Nw * Kw;
    unsigned fgrid = (unsigned)((total / 4 + 255) / 256);
    if (bias_slabs && (unsigned)((Nw + 3) / 4) > fgrid) fgrid = (unsigned)((Nw + 3) / 4);
    hipLaunchKernelGGL(wgrad_finish_kernel, dim3(fgrid), dim3(256), 0, (hipStream_t)stream, slabs, dW, lddw, nchunks, Nw, Kw,
                       bias_slabs, db);
    AIM_CHECK_LAUNCH("aim_wgrad_finish");
    return 0;
}
