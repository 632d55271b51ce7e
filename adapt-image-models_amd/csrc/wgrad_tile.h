// One output tile x one M-chunk of the adapter weight gradient  dW[n][k] += sum_m G[m][n] * A[m][k]  as a device function:
// the body of wgrad_kernel (wgrad.hip), shared with the rider workgroups of the persistent GEMM (gemm256.hip).
#pragma once
#include "aim_common.h"

namespace wgrad_tile {

constexpr int MSTEP = 32;                 // reduction rows per stage
constexpr int NST = 4;                    // LDS ring depth: three stages in flight hide the HBM latency
constexpr int IMG = MSTEP * 128;          // one [32 m][64 col] image = 4 KiB
constexpr int OPER_BYTES = 4 * IMG;       // [32 m][256 col] = four images = 16 KiB
constexpr int STAGE_BYTES = 2 * OPER_BYTES;
constexpr int TILE = 256;                 // output tile 256 (n) x 256 (k)
constexpr int RING_BYTES = NST * STAGE_BYTES;      // 128 KiB; the `at` table (ntok floats) lives behind it

// A weight-gradient job of rider workgroups: rows [m_begin, m_end) of the whole problem (G, A point at its row 0) in
// chunks of `chunk` rows (a multiple of 32); chunk c of tile t belongs to rider c * tiles + t.  The chunk's partial tile goes
// to slabs[c][Nw][Kw], its bias column sums (bias_slabs != nullptr) to bias_slabs[c][Nw].
struct Job {
    const bf16_t* G;
    const bf16_t* A;
    float* slabs;
    float* bias_slabs;
    const float* at;
    int ldg, lda, Nw, Kw, m_begin, m_end, chunk, ntok;
};

// One workgroup = 8 waves as 2 (n) x 4 (k); a wave owns 128 x 64 outputs = 8 x 4 MFMA 16x16x32 tiles.
// The kernel is bound by the bytes a CU can pull per cycle (every output tile re-reads its M-chunk of G and
// A), so the tile is as large as the accumulators allow: [768 x 192] needs 3 tiles, 271 MB of operand reads
// for M = 100 864 instead of 620 MB with 128 x 128 tiles.
//
// Bias gradient in the same pass (want_bias): column sums of rs(m) G[m][n], rs(m) = at[(row0 + m) % ntok] (1 without `at`).  The
// workgroups of the first k-tile column (tk == 0) already hold every G row of their chunk in LDS: thread t sums column
// t & 255 over rows 16 (t >> 8) .. +15 of each stage beside the MFMAs (the kernel is bound by the CU's load path, not by LDS
// or VALU issue); the per-chunk column sums go to their own slab row and are added up, in chunk order, by the finish kernel.
// This replaces a separate column-sum launch that re-read all of G from HBM (155 MB for the MLP_Adapter's D_fc2 bias).
//
// Rows [mbeg, mend) of G / A (mbeg < mend); row m of G is row row0 + m of the whole problem (only `at` looks at that).
// slab: this chunk's partial tile [Nw][Kw], or nullptr -> fp32 atomics into dW.  bias_row: this chunk's [Nw] column sums, or
// nullptr -> db[n] += (one chunk: this workgroup is the column's only writer).  SLABS: both are given (no atomics compiled in).
template <bool SLABS>
__device__ __forceinline__ void run(AIM_LDS char* smem, const bf16_t* __restrict__ G, int ldg, const bf16_t* __restrict__ A, int lda,
                                    float* __restrict__ dW, int lddw, float* __restrict__ slab, int Nw, int Kw, int tn, int tk,
                                    int mbeg, int mend, int row0, bool want_bias, float* __restrict__ db,
                                    float* __restrict__ bias_row, const float* __restrict__ at, int ntok) {
    AIM_LDS float* sAt = (AIM_LDS float*)(smem + RING_BYTES);            // [ntok] row factors (only with `at`)
    const int n0 = tn * TILE, k0 = tk * TILE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 2, wk = wave & 3;
    const int frow = lane & 15, fq = lane >> 4;

    const bf16_t* Gb = G + (long long)mbeg * ldg + n0;
    const bf16_t* Ab = A + (long long)mbeg * lda + k0;
    const int rows = mend - mbeg;
    aim_rsrc_words rG = make_rsrc_words(Gb, ((long long)(rows - 1) * ldg + min(TILE, Nw - n0)) * 2);
    aim_rsrc_words rA = make_rsrc_words(Ab, ((long long)(rows - 1) * lda + min(TILE, Kw - k0)) * 2);

    // staging: per operand 16 pieces (4 column images x 4 row groups of 8); a wave takes 2 of each.  A piece's offset is its
    // stage-0 offset plus ms * (32 rows): one v_add per piece and step.  Rows past the chunk need no test -- the resources end
    // with the chunk's last row, so their offsets are out of range by themselves (zero fill); columns past Nw / Kw carry
    // AIM_OOB from the start (AIM_OOB + ms * step stays out of range).
    const int srow = lane >> 3, schunk = (lane & 7) ^ srow;
    unsigned vg0[2], va0[2];
    AIM_LDS char* pdst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int piece = wave * 2 + j;           // 0..15
        const int img = piece >> 2, rg = piece & 3;
        const int r = rg * 8 + srow;              // row inside stage 0
        const int col = img * 64 + schunk * 8;
        vg0[j] = n0 + col < Nw ? (unsigned)((r * ldg + col) * 2) : AIM_OOB;
        va0[j] = k0 + col < Kw ? (unsigned)((r * lda + col) * 2) : AIM_OOB;
        pdst[j] = smem + img * IMG + rg * 1024;
    }
    const unsigned gstep = (unsigned)(MSTEP * ldg * 2), astep = (unsigned)(MSTEP * lda * 2);
    auto stage = [&](int buf, int ms) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            stage_piece_asm(rG, pdst[j] + buf * STAGE_BYTES, vg0[j] + (unsigned)ms * gstep);
            stage_piece_asm(rA, pdst[j] + buf * STAGE_BYTES + OPER_BYTES, va0[j] + (unsigned)ms * astep);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposing fragment read: 16 columns c0..c0+15 of the operand's [32 m][256] stage, reduction rows
    // {4*fq + 0..3} and {16 + 4*fq + 0..3}; lane i = lane&15 supplies row (i>>2), cols 4*(i&3)..
    auto frag = [&](const AIM_LDS char* oper, int c0) -> bf16x8 {
        const AIM_LDS char* img = oper + (c0 >> 6) * IMG;
        const int ch = ((c0 & 63) >> 3) + ((frow & 3) >> 1), half8 = (frow & 1) * 8;
        const int r0 = fq * 4 + (frow >> 2);
        const bf16x4 a = lds_read_tr4(img + swz_off(r0, ch) + half8);
        const bf16x4 b = lds_read_tr4(img + swz_off(r0 + 16, ch) + half8);
        bf16x8 f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[e] = a[e];
            f[4 + e] = b[e];
        }
        return f;
    };

    // ring of NST stages; each wave issues 4 LDS-DMA loads per stage.  Iteration ms: vmcnt(8) retires
    // stage ms (stages ms+1, ms+2 stay in flight), one barrier, re-stage buffer (ms+3)%4 -- read in
    // iteration ms-1, which every wave finished before this barrier -- then 24 tr-reads + 32 MFMA.
    const int nsteps = (rows + MSTEP - 1) / MSTEP;
    const bool do_bias = want_bias && tk == 0;          // workgroup-uniform
    // bias column sums: thread t owns the 8 columns of 16-byte chunk (t & 31) in rows (t >> 5) and (t >> 5) + 16 of every stage
    // (two ds_read_b128 per step; the first version read sixteen 2-byte values per thread and step: +30 us per launch)
    float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int bcg = tid & 31, brow = tid >> 5;
    int btok0 = 0, btok1 = 0;
    if (do_bias && at) {
        for (int i = tid; i < ntok; i += 512) sAt[i] = at[i];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // written before the loop's first barrier publishes it
        btok0 = (row0 + mbeg + brow) % ntok;
        btok1 = (row0 + mbeg + brow + 16) % ntok;
    }
    const int bstep = MSTEP % (ntok > 0 ? ntok : 1);
    stage(0, 0); stage(1, 1); stage(2, 2);            // stages past the chunk are zero-fill, still counted
    for (int ms = 0; ms < nsteps; ++ms) {
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        stage((ms + 3) % NST, ms + 3);
        const AIM_LDS char* sG = smem + (ms % NST) * STAGE_BYTES;
        const AIM_LDS char* sA = sG + OPER_BYTES;
        if (do_bias) {
            // chunk bcg of the [32 m][256 n] stage: image bcg >> 3, 16-byte chunk bcg & 7 of rows brow and brow + 16
            const AIM_LDS char* img = sG + (bcg >> 3) * IMG;
            const bf16x8 v0 = lds_read8(img + swz_off(brow, bcg & 7));
            const bf16x8 v1 = lds_read8(img + swz_off(brow + 16, bcg & 7));
            float f0 = 1.0f, f1 = 1.0f;
            if (at) {
                f0 = sAt[btok0];
                f1 = sAt[btok1];
                btok0 += bstep; if (btok0 >= ntok) btok0 -= ntok;
                btok1 += bstep; if (btok1 >= ntok) btok1 -= ntok;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) bs[e] += f0 * (float)v0[e] + f1 * (float)v1[e];      // rows past the chunk are zero-filled
        }
        bf16x8 gf[8], af[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = frag(sA, wk * 64 + j * 16);
#pragma unroll
        for (int i = 0; i < 8; ++i) gf[i] = frag(sG, wn * 128 + i * 16);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[j], gf[i], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (do_bias) {          // the sixteen row groups of a column meet in LDS (the stage images are dead now), summed in order
        __syncthreads();
        AIM_LDS float* red = (AIM_LDS float*)smem;
#pragma unroll
        for (int e = 0; e < 8; ++e) red[brow * 256 + bcg * 8 + e] = bs[e];
        __syncthreads();
        if (tid < 256 && n0 + tid < Nw) {
            float v = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) v += red[r * 256 + tid];
            if (SLABS || bias_row) bias_row[n0 + tid] = v;
            else db[n0 + tid] += v;                    // one chunk: this workgroup is the column's only writer
        }
    }
    // The MFMA is issued with the A fragment FIRST (D[k][n]): the lane holds n = .. + (lane & 15) and the four consecutive
    // k = .. + 4 * (lane >> 4) + e, so a partial tile leaves as 16-byte stores (32 per wave; the 4-byte form, 128 per wave,
    // took 7.6 us of a 46 us workgroup).
    // With a scratch slab the chunk's partial tile is stored plainly (slab [chunk][Nw][Kw], summed by
    // wgrad_finish_kernel: no atomics, bitwise reproducible); otherwise fp32 atomics into dW.
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 128 + i * 16 + frow;
            const int k = k0 + wk * 64 + j * 16 + fq * 4;
            if (n >= Nw || k >= Kw) continue;          // Kw is a multiple of 8: a lane's four k are in range together
            if (SLABS || slab) *(f32x4*)(slab + (long long)n * Kw + k) = acc[i][j];
            else
#pragma unroll
                for (int e = 0; e < 4; ++e) atomicAdd(dW + (long long)n * lddw + k + e, acc[i][j][e]);
        }
}

// A rider workgroup's share of a Job: rider `rid` = chunk (rid / tiles) of tile (rid % tiles).  Empty chunks write nothing.
// The rider always writes slabs (no atomics).
__device__ __forceinline__ void run_job(AIM_LDS char* smem, const Job& j, int rid) {
    const int tiles_k = (j.Kw + TILE - 1) / TILE;
    const int tiles = ((j.Nw + TILE - 1) / TILE) * tiles_k;
    const int cidx = rid / tiles, tix = rid - cidx * tiles;
    const int tn = tix / tiles_k, tk = tix - tn * tiles_k;
    const int mbeg = j.m_begin + cidx * j.chunk;
    const int mend = min(j.m_end, mbeg + j.chunk);
    if (mbeg >= mend) return;
    run<true>(smem, j.G, j.ldg, j.A, j.lda, nullptr, 0, j.slabs + (long long)cidx * j.Nw * j.Kw, j.Nw, j.Kw, tn, tk, mbeg, mend, 0,
        j.bias_slabs != nullptr, nullptr, j.bias_slabs ? j.bias_slabs + (long long)cidx * j.Nw : nullptr, j.at, j.ntok);
}

}  // namespace wgrad_tile
