// Temporal attention over the T frames of EVERY token position (stock-AIM block), forward and backward.  gfx950 only.
//
// Replaces reference mmaction/models/backbones/vitclip_aim.py:199-205: attention() (:148-187) applied to
// rearrange(x, 'n (b t) d -> t (b n) d'): sequence = the T frames, batch = B * N (every token position of every clip).
// (vit_clip.py's own block runs this attention on the class tokens only: cls_attn.hip.)
// Sequence length is T <= 32 and the batch is huge (B * N * H = 151 296 problems at 64 clips), so this is a
// bandwidth-bound kernel: one wave per (clip, token, head), lane = head-dim element, 4 problems per 256-thread workgroup;
// every global access of a wave is one whole 128-byte row segment of the frame-major fused qkv buffer
// (row (b*T + t)*N + n), so no transposed copy of the activations is ever made (the reference rearranges x twice).
#include "aim_common.h"
#include "aim_kernels_internal.h"

namespace {

constexpr int TMAX = 32;

// How q, k and v are staged in LDS: as fp32 in rows of 65 floats, or (LDS16) as the bf16 they arrive as in rows of 66
// elements (33 dwords: an odd dword stride again) and widened on read -- the same fp32 values, half the bytes.
template <bool LDS16> struct tattn_stage { typedef float elem; static constexpr int RS = 65, ROW_FLOATS = 65; };
template <> struct tattn_stage<true> { typedef bf16_t elem; static constexpr int RS = 66, ROW_FLOATS = 33; };

// LDS per wave: q, k, v [T][RS] + p [T][T+1] f32
template <bool LDS16>
__host__ __device__ __forceinline__ int tattn_lds_floats(int T) { return 3 * T * tattn_stage<LDS16>::ROW_FLOATS + T * (T + 1); }

// PROBS: the probabilities go to `probs` (what the backward reads).  OUT8: `out` is e4m3 bytes, the saturating cast of the
// fp32 accumulators, instead of bf16.  <true, false, false> is the training forward; the others are the inference forms
// (aim_tattn_fwd_infer).  The score, softmax and P.V arithmetic is one text for all of them, every sum in ascending index
// order, so the bf16 outputs agree bit for bit and the fp8 bytes are the cast of the very accumulators the bf16 form rounds.
template <bool PROBS, bool OUT8, bool LDS16>
__global__ __launch_bounds__(256) void tattn_fwd_kernel(const bf16_t* __restrict__ qkv, void* __restrict__ out,
                                                        float* __restrict__ probs, int B, int T, int N, int H) {
    typedef typename tattn_stage<LDS16>::elem S;
    constexpr int RS = tattn_stage<LDS16>::RS;
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long prob = (long long)blockIdx.x * (blockDim.x >> 6) + wave;          // (b, n, h)
    const long long nprob = (long long)B * N * H;
    if (prob >= nprob) return;          // (whole waves only: no barrier below spans waves)
    const int h = (int)(prob % H);
    const long long bn = prob / H;
    const int n = (int)(bn % N), b = (int)(bn / N);
    const int D = H * 64, ld = 3 * D;
    S* sq = (S*)(smem + wave * tattn_lds_floats<LDS16>(T));
    S* sk = sq + T * RS;
    S* sv = sk + T * RS;
    float* sp = (float*)(sv + T * RS);
    for (int t = 0; t < T; ++t) {
        const bf16_t* r = qkv + ((long long)(b * T + t) * N + n) * ld + h * 64 + lane;
        sq[t * RS + lane] = (S)r[0];
        sk[t * RS + lane] = (S)r[D];
        sv[t * RS + lane] = (S)r[2 * D];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): this wave's LDS writes are done
    for (int p = lane; p < T * T; p += 64) {
        const int tq = p / T, tk = p - tq * T;
        float acc = 0.f;
        if constexpr (LDS16) {      // two elements per 32-bit LDS read, summed in the same ascending order
            const bf16x2* q2 = (const bf16x2*)(sq + tq * RS);
            const bf16x2* k2 = (const bf16x2*)(sk + tk * RS);
#pragma unroll 8
            for (int d = 0; d < 32; ++d) {
                const bf16x2 a = q2[d], c = k2[d];
                acc += (float)a[0] * (float)c[0];
                acc += (float)a[1] * (float)c[1];
            }
        } else {
#pragma unroll 8
            for (int d = 0; d < 64; ++d) acc += sq[tq * RS + d] * sk[tk * RS + d];
        }
        sp[tq * (T + 1) + tk] = acc * 0.125f;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (int tq = lane; tq < T; tq += 64) {
        float mx = -INFINITY;
        for (int tk = 0; tk < T; ++tk) mx = fmaxf(mx, sp[tq * (T + 1) + tk]);
        float sum = 0.f;
        for (int tk = 0; tk < T; ++tk) {
            const float e = expf(sp[tq * (T + 1) + tk] - mx);
            sp[tq * (T + 1) + tk] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
        for (int tk = 0; tk < T; ++tk) {
            const float p = sp[tq * (T + 1) + tk] * inv;
            sp[tq * (T + 1) + tk] = p;
            if constexpr (PROBS) probs[(prob * T + tq) * T + tk] = p;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if constexpr (OUT8) {
        // a lane owns four consecutive head-dim elements (one packed 32-bit store) of query row tq0 + lane / 16: sixteen
        // lanes cover the head's 64 bytes of a row, the wave four rows per step
        const int sub = lane >> 4, d4 = (lane & 15) * 4;
        for (int tq0 = 0; tq0 < T; tq0 += 4) {
            const int tq = tq0 + sub;
            if (tq >= T) continue;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            for (int tk = 0; tk < T; ++tk) {
                const float p = sp[tq * (T + 1) + tk];
                float v0, v1, v2, v3;
                if constexpr (LDS16) {
                    const bf16x2* v = (const bf16x2*)(sv + tk * RS + d4);
                    const bf16x2 lo = v[0], hi = v[1];
                    v0 = (float)lo[0], v1 = (float)lo[1], v2 = (float)hi[0], v3 = (float)hi[1];
                } else {
                    v0 = sv[tk * RS + d4], v1 = sv[tk * RS + d4 + 1], v2 = sv[tk * RS + d4 + 2], v3 = sv[tk * RS + d4 + 3];
                }
                a0 += p * v0;
                a1 += p * v1;
                a2 += p * v2;
                a3 += p * v3;
            }
            *(unsigned*)((uint8_t*)out + ((long long)(b * T + tq) * N + n) * D + h * 64 + d4) = pack4_fp8(a0, a1, a2, a3);
        }
    } else {
        for (int tq = 0; tq < T; ++tq) {
            float acc = 0.f;
            for (int tk = 0; tk < T; ++tk) acc += sp[tq * (T + 1) + tk] * (float)sv[tk * RS + lane];
            ((bf16_t*)out)[((long long)(b * T + tq) * N + n) * D + h * 64 + lane] = (bf16_t)acc;
        }
    }
}

// LDS per wave: q, k, v, dO [T][65] + p, dS [T][T+1]
__device__ __forceinline__ int tattn_bwd_lds_floats(int T) { return 4 * T * 65 + 2 * T * (T + 1); }

__global__ __launch_bounds__(256) void tattn_bwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ probs,
                                                        const bf16_t* __restrict__ dout, bf16_t* __restrict__ dqkv, int B,
                                                        int T, int N, int H) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long prob = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    const long long nprob = (long long)B * N * H;
    if (prob >= nprob) return;
    const int h = (int)(prob % H);
    const long long bn = prob / H;
    const int n = (int)(bn % N), b = (int)(bn / N);
    const int D = H * 64, ld = 3 * D;
    float* sq = smem + wave * tattn_bwd_lds_floats(T);
    float* sk = sq + T * 65;
    float* sv = sk + T * 65;
    float* sdo = sv + T * 65;
    float* sp = sdo + T * 65;
    float* sds = sp + T * (T + 1);
    for (int t = 0; t < T; ++t) {
        const long long row = (long long)(b * T + t) * N + n;
        const bf16_t* r = qkv + row * ld + h * 64 + lane;
        sq[t * 65 + lane] = (float)r[0];
        sk[t * 65 + lane] = (float)r[D];
        sv[t * 65 + lane] = (float)r[2 * D];
        sdo[t * 65 + lane] = (float)dout[row * D + h * 64 + lane];
    }
    for (int p = lane; p < T * T; p += 64) {
        const int tq = p / T, tk = p - tq * T;
        sp[tq * (T + 1) + tk] = probs[(prob * T + tq) * T + tk];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (int p = lane; p < T * T; p += 64) {          // dP[tq][tk] = dO[tq] . V[tk]
        const int tq = p / T, tk = p - tq * T;
        float acc = 0.f;
#pragma unroll 8
        for (int d = 0; d < 64; ++d) acc += sdo[tq * 65 + d] * sv[tk * 65 + d];
        sds[tq * (T + 1) + tk] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (int tq = lane; tq < T; tq += 64) {
        float dot = 0.f;
        for (int tk = 0; tk < T; ++tk) dot += sp[tq * (T + 1) + tk] * sds[tq * (T + 1) + tk];
        for (int tk = 0; tk < T; ++tk) sds[tq * (T + 1) + tk] = sp[tq * (T + 1) + tk] * (sds[tq * (T + 1) + tk] - dot) * 0.125f;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (int t = 0; t < T; ++t) {
        float dq = 0.f, dk = 0.f, dv = 0.f;
        for (int u = 0; u < T; ++u) {
            dq += sds[t * (T + 1) + u] * sk[u * 65 + lane];
            dk += sds[u * (T + 1) + t] * sq[u * 65 + lane];
            dv += sp[u * (T + 1) + t] * sdo[u * 65 + lane];
        }
        bf16_t* r = dqkv + ((long long)(b * T + t) * N + n) * ld + h * 64 + lane;
        r[0] = (bf16_t)dq;
        r[D] = (bf16_t)dk;
        r[2 * D] = (bf16_t)dv;
    }
}

// out[r][c] = a[r][c] + b[r][c]  (bf16, row strides in elements; 8 elements per thread)
__global__ __launch_bounds__(256) void add_bf16_kernel(const bf16_t* __restrict__ a, long long lda, const bf16_t* __restrict__ b,
                                                       long long ldb, bf16_t* __restrict__ out, long long ldo, int R, int C8) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)R * C8) return;
    const int r = (int)(i / C8), c = (int)(i - (long long)r * C8) * 8;
    const bf16x8 x = *(const bf16x8*)(a + r * lda + c), y = *(const bf16x8*)(b + r * ldb + c);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (bf16_t)((float)x[e] + (float)y[e]);
    *(bf16x8*)(out + r * ldo + c) = o;
}

// x[r][c] += s[r][c]   (x f32 dense [R, C], s bf16 with row stride lds; 4 elements per thread)
__global__ __launch_bounds__(256) void acc_bf16_kernel(float* __restrict__ x, const bf16_t* __restrict__ s, long long lds, int R, int C4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)R * C4) return;
    const int r = (int)(i / C4), c = (int)(i - (long long)r * C4) * 4;
    f32x4* xp = (f32x4*)(x + (long long)r * C4 * 4 + c);
    const bf16x4 v = *(const bf16x4*)(s + r * lds + c);
    f32x4 o = *xp;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] += (float)v[e];
    *xp = o;
}

}  // namespace

template <bool PROBS, bool OUT8, bool LDS16>
static int tattn_fwd_launch(const char* name, const aim_bf16* qkv, void* out, float* probs, int B, int T, int N, int H, void* stream) {
    const long long nprob = (long long)B * N * H;
    const int wpb = T <= 16 ? 4 : 2;                // waves (problems) per workgroup: LDS per problem grows with T
    const size_t lds = (size_t)wpb * tattn_lds_floats<LDS16>(T) * 4;
    static bool attr_set_f = false;                 // (one per instantiation)
    if (!attr_set_f) {
        (void)hipFuncSetAttribute((const void*)tattn_fwd_kernel<PROBS, OUT8, LDS16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set_f = true;
    }
    hipLaunchKernelGGL((tattn_fwd_kernel<PROBS, OUT8, LDS16>), dim3((unsigned)((nprob + wpb - 1) / wpb)), dim3(64 * wpb), lds,
                       (hipStream_t)stream, (const bf16_t*)qkv, out, probs, B, T, N, H);
    AIM_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int aim_tattn_fwd(const aim_bf16* qkv, aim_bf16* out, float* probs, int B, int T, int N, int H, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && T <= TMAX && N > 0 && H > 0, "tattn_fwd: unsupported shape B=%d T=%d (T <= 32)", B, T);
    AIM_CHECK_ARG(qkv && out && probs, "tattn_fwd: null pointer");
    return tattn_fwd_launch<true, false, false>("aim_tattn_fwd", qkv, out, probs, B, T, N, H, stream);
}

extern "C" int aim_tattn_fwd_infer(const aim_bf16* qkv, aim_bf16* out, uint8_t* out_fp8, int B, int T, int N, int H, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && T <= TMAX && N > 0 && H > 0, "tattn_fwd_infer: unsupported shape B=%d T=%d (T <= 32)", B, T);
    AIM_CHECK_ARG(qkv, "tattn_fwd_infer: null pointer");
    AIM_CHECK_ARG((out != nullptr) != (out_fp8 != nullptr), "tattn_fwd_infer: exactly one of out / out_fp8 must be given");
    AIM_CHECK_ARG(((uintptr_t)out_fp8 & 3) == 0, "tattn_fwd_infer: out_fp8 must be 4-byte aligned (packed 32-bit stores)");
    // q, k, v staged as bf16: 16.5 KB instead of 28.5 KB per wave at T = 32, so twice the waves fit a CU and a score or P.V
    // step reads two elements per LDS access.  Measured at 3 views x 32 frames x 257 tokens x 16 heads (rocprofv3): bf16
    // form 415 -> 264 us, fp8 form 362 -> 209 us, same bits.  AIM_TATTN_LDS16=0: fp32 staging as in the training kernel (A/B runs)
    static const bool lds16 = [] { const char* e = getenv("AIM_TATTN_LDS16"); return !e || atoi(e) != 0; }();
    if (out_fp8) {
        if (lds16) return tattn_fwd_launch<false, true, true>("aim_tattn_fwd_infer", qkv, out_fp8, nullptr, B, T, N, H, stream);
        return tattn_fwd_launch<false, true, false>("aim_tattn_fwd_infer", qkv, out_fp8, nullptr, B, T, N, H, stream);
    }
    if (lds16) return tattn_fwd_launch<false, false, true>("aim_tattn_fwd_infer", qkv, out, nullptr, B, T, N, H, stream);
    return tattn_fwd_launch<false, false, false>("aim_tattn_fwd_infer", qkv, out, nullptr, B, T, N, H, stream);
}

extern "C" int aim_tattn_bwd(const aim_bf16* qkv, const float* probs, const aim_bf16* dout, aim_bf16* dqkv, int B, int T, int N,
                             int H, void* stream) {
    AIM_CHECK_ARG(B > 0 && T > 0 && T <= TMAX && N > 0 && H > 0, "tattn_bwd: unsupported shape B=%d T=%d (T <= 32)", B, T);
    AIM_CHECK_ARG(qkv && probs && dout && dqkv, "tattn_bwd: null pointer");
    const long long nprob = (long long)B * N * H;
    const int wpb = T <= 16 ? 4 : 2;
    const size_t lds = (size_t)wpb * (4 * T * 65 + 2 * T * (T + 1)) * 4;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)tattn_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(tattn_bwd_kernel, dim3((unsigned)((nprob + wpb - 1) / wpb)), dim3(64 * wpb), lds, (hipStream_t)stream, (const bf16_t*)qkv,
                       probs, (const bf16_t*)dout, (bf16_t*)dqkv, B, T, N, H);
    AIM_CHECK_LAUNCH("aim_tattn_bwd");
    return 0;
}

extern "C" int aim_add_bf16(const aim_bf16* a, int64_t lda, const aim_bf16* b, int64_t ldb, aim_bf16* out, int64_t ldo, int R, int C,
                            void* stream) {
    AIM_CHECK_ARG(a && b && out && R > 0 && C > 0 && (C % 8) == 0 && (lda % 8) == 0 && (ldb % 8) == 0 && (ldo % 8) == 0, "add_bf16: bad arguments");
    const long long n = (long long)R * (C / 8);
    hipLaunchKernelGGL(add_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a,
                       (long long)lda, (const bf16_t*)b, (long long)ldb, (bf16_t*)out, (long long)ldo, R, C / 8);
    AIM_CHECK_LAUNCH("aim_add_bf16");
    return 0;
}

extern "C" int aim_acc_bf16(float* x, const aim_bf16* s, int64_t lds, int R, int C, void* stream) {
    AIM_CHECK_ARG(x && s && R > 0 && C > 0 && (C % 4) == 0 && (lds % 4) == 0, "acc_bf16: bad arguments");
    const long long n = (long long)R * (C / 4);
    hipLaunchKernelGGL(acc_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)s,
                       (long long)lds, R, C / 4);
    AIM_CHECK_LAUNCH("aim_acc_bf16");
    return 0;
}
