// Internal glue between the public C ABI (include/aim_kernels.h) and the kernel translation units.
#pragma once
#include <stdlib.h>
#include "../../include/aim_kernels.h"
#include <hip/hip_runtime.h>

typedef aim_gemm_args GemmArgs;
enum { EPI_BF16 = AIM_EPI_BF16, EPI_ACT = AIM_EPI_ACT, EPI_DACT = AIM_EPI_DACT, EPI_F32 = AIM_EPI_F32, EPI_EXPSUM = AIM_EPI_EXPSUM, EPI_ACT8 = AIM_EPI_ACT8, EPI_RES16 = AIM_EPI_RES16 };
enum { ACT_QGELU = AIM_ACT_QGELU, ACT_GELU = AIM_ACT_GELU };

// CUs of the current device (per-call query, no cache; CU-masked caller streams are not supported: capi.hip).  Persistent
// kernels size their grids by it.
int aim_device_cus();
// ride != nullptr: the launch also carries the rider workgroups of an adapter weight gradient (gemm256.hip); refused unless
// aim_gemm_hosts_riders(g, epi).  *chunks_written: the slabs the riders fill.
int aim_gemm_launch(const GemmArgs& g, int epi, int batch, hipStream_t st, const aim_wgrad_ride_args* ride = nullptr,
                    int* chunks_written = nullptr);
int aim_gemm256_launch(const GemmArgs& g, int epi, int nbatch, hipStream_t st);
bool aim_gemm_hosts_riders(const GemmArgs& g, int epi);
int aim_gemm256_ride_launch(const GemmArgs& g, int epi, const aim_wgrad_ride_args& r, int* chunks_written, hipStream_t st);
int aim_gemm256_ride_plan(const GemmArgs& g, int epi, int Nw, int Kw, int ntok, int M_total, int rows_left, int* chunks, int* rows);
// a row range as at most max_chunks chunks of whole 32-row steps: the chunk length and the number of non-empty chunks
int aim_wgrad_range_chunks(int rows, int max_chunks, int* chunk_out);
int aim_gemm256_fp8_launch(const GemmArgs& g, int epi, hipStream_t st);
int aim_gemm_small_launch(const GemmArgs& g, int epi, int batch, hipStream_t st);
int aim_gemm_small_fp8_launch(const GemmArgs& g, int epi, hipStream_t st);
// rows of a thin last tile round that go to the small-tile kernel (0: no peel); fills M0 = rows of the whole rounds
int aim_gemm_peel_rows(const GemmArgs& g, int* M0);
// Mini-batch blending fused into the patch gather.  Clip b of the batch pairs with clip partner[b].  mode 1 (mixup):
// lam * v(b) + oml * v(partner[b]); mode 2 (cutmix): v(partner[b]) for pixels in rows [y1, y2) x columns [x1, x2) of every
// frame and channel, v(b) elsewhere.
struct AimBlend {
    const int* partner;
    int mode;
    float lam, oml;
    int x1, y1, x2, y2;
};
// The launcher of the one patch-gather kernel (embed_misc.hip) behind the four aim_patchify* entry points, which keep their
// own shape and pointer checks and their own in_dtype refusal.  blend: null for a plain gather, else checked here; who: the
// prefix of the entry point's messages ("patchify_f32").  0: launched; -1, no error set: no gather for this in_dtype, which
// the entry point refuses in its own words; other nonzero: the error is set.  A must be 16-byte aligned.
int aim_patchify_launch(const char* who, bool f32_out, const void* imgs, int in_dtype, const float* mean3, const float* std3,
                        void* A, int B, int T, int H, int W, int p, int Kp, const AimBlend* blend, hipStream_t st);
// EXPSUM problems of one 256x256 tile per batch item run on the persistent kernel (8 partial slots per item)
static inline bool aim_expsum_use256(int M, int N) {
    static const bool on = [] { const char* e = getenv("AIM_EXPSUM_256"); return !e || atoi(e) != 0; }();
    return on && (M > 128 || N > 128) && M <= 256 && N <= 256;
}

// Head-shifted spatial attention (aim_attn_fwd_shift / aim_attn_bwd_shift): the queries of frame b T + t see, in head h, the K
// and V of frame b T + (t - s_h) mod T of the same clip.  The table travels in the kernel arguments, one byte per head,
// already reduced to [0, T): no device memory, no allocation, nothing kept between calls.  T == 0: no shift.
struct AttnShift {
    unsigned long long lo, hi;          // heads 0..7, 8..15
    int T;
};
// checks (B T == BT, H <= 16, T <= 256, |s_h| < T) and packs; nonzero: the error is set
int aim_attn_shift_pack(const char* who, AttnShift* sh, const int* shifts, int B, int T, int BT, int H);
#ifdef __HIPCC__
__device__ __forceinline__ int attn_shift_of(const AttnShift& sh, int h) {
    const unsigned long long w = h < 8 ? sh.lo : sh.hi;
    return (int)((w >> ((h & 7) * 8)) & 0xff);
}
// the frame whose K / V (and dK / dV) belong to the queries of frame bt in head h; t = bt mod T
__device__ __forceinline__ int attn_kv_frame_t(const AttnShift& sh, int bt, int t, int h) {
    const int s = attn_shift_of(sh, h);
    return bt - s + (t < s ? sh.T : 0);
}
__device__ __forceinline__ int attn_kv_frame(const AttnShift& sh, int bt, int h) { return attn_kv_frame_t(sh, bt, bt % sh.T, h); }
#endif
