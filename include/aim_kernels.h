/*
 * aim_kernels.h -- C ABI of libaim_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * AIM ViT-CLIP + Adapter forward/backward hot path.
 *
 * The reference (bobochow/adapt-image-models) is 100 % Python over PyTorch eager ops and has no
 * FFI of its own; each entry point below replaces the eager-op sequence at the cited lines of
 * mmaction/models/backbones/vit_clip.py.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success; non-zero -> aim_last_error() (thread-local text);
 *   - all pointers are DEVICE pointers unless said otherwise; the caller owns all memory
 *     (no allocation, no implicit synchronisation and no state that outlives a call inside the
 *     library -- the only statics are idempotent one-time initialisations (a kernel's dynamic-LDS
 *     attribute, environment switches read once); every knob of a launch is an argument of that
 *     call, so two host threads may drive two streams through the library at once);
 *   - `stream` is a hipStream_t passed as void*; launches are stream-ordered;
 *   - matrices are row-major; "bf16" is IEEE bfloat16 stored as uint16_t; "ld*" are row strides
 *     in ELEMENTS;
 *   - token rows are frame-major: row = (b*T + t)*N + n for clip b, frame t, token n
 *     (the reference's [N, BT, D] tensor transposed; N = (res/patch)^2 + 1, D = width);
 *   - head_dim is 64 for every supported model (ViT-B/16: 12x64, ViT-L/14: 16x64).
 */
#ifndef AIM_KERNELS_H
#define AIM_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t aim_bf16;

#define AIM_ABI_VERSION 19

int aim_version(void);                /* == AIM_ABI_VERSION */
const char* aim_last_error(void);     /* message of the last failing call on this thread */

/* ------------------------------------------------------------------------------------------
 * GEMM  C[m][n] = sum_k A[m][k] * W[n][k]  (bf16 operands, fp32 accumulate, MFMA 16x16x32)
 * replaces: q/k/v projections vit_clip.py:132-138,168-173; attn.out_proj :157,192;
 *           mlp.c_fc/QuickGELU/c_proj :93-97,286; Adapter.D_fc1/GELU/D_fc2 :62-64;
 *           residual combines :275,286; and (autograd) the dgrad of every frozen Linear
 *           (pass the transposed weight).
 * Requirements: K, lda, ldw multiples of 8; N, ldo (and ldo2/ldr/ldv/ldaux when used) multiples
 * of 4; pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
enum {
    AIM_EPI_BF16 = 0,  /* out(bf16) = rs * (acc + bias)                                         */
    AIM_EPI_ACT = 1,   /* out2(bf16) = pre = acc + bias ; out(bf16) = rs * act(pre)             */
    AIM_EPI_DACT = 2,  /* out(bf16) = rs * (acc + bias) * act'(aux)        (aux = saved pre)    */
    AIM_EPI_F32 = 3,   /* out(f32) = resid + rs*(acc + bias) + bt[tok]*vec[frame][n]
                          (rs_bias_only != 0: out = resid + acc + rs*bias + ...)               */
    AIM_EPI_EXPSUM = 4,/* out(f32)[batch][tile][2] = (max, sum exp(scale*acc - max)) over the
                          valid part of each tile (lambda statistics, :149-151): per batch item
                          aim_gemm_expsum_tiles(M, N) pairs, ldo = float stride between items
                          (0: packed).  Problems that function lays out as 8 slots per item
                          need K % 64 == 0; other K is refused.                                 */
    AIM_EPI_ACT8 = 5,  /* out(fp8 e4m3) = sat(rs * act(acc + bias)): inference only, nothing saved
                          for a backward (aim_gemm_fp8)                                         */
    AIM_EPI_RES16 = 6  /* out(bf16) = resid(bf16) + rs*(acc + bias) + bt[tok]*vec[frame][n]: AIM_EPI_F32's sum on
                          a bf16 residual stream (fp8 inference only, aim_gemm_fp8; ldr in bf16 elements)    */
};
enum { AIM_ACT_QGELU = 0, AIM_ACT_GELU = 1 };

typedef struct aim_gemm_args {
    const aim_bf16* A;      /* [batch][M, lda]                                                  */
    const aim_bf16* W;      /* [batch][N, ldw]                                                  */
    int32_t lda, ldw;
    int64_t strideA, strideW; /* batch strides in elements (0 for batch == 1)                   */
    int32_t M, N, K;
    const float* bias;      /* [N] or NULL                                                      */
    const float* resid;     /* [M, ldr] f32 or NULL (AIM_EPI_F32)                               */
    int32_t ldr;
    /* row factor rs = af[row / ntok] * at[row % ntok]  (either may be NULL -> 1)               */
    const float* af;        /* [M / ntok] per-frame factor, e.g. 1 - lamda                      */
    const float* at;        /* [ntok]     per-token factor, e.g. DropPath mask * adapter scale  */
    const float* vec;       /* [M / ntok, ldv] per-frame row vector added to every token        */
    const float* bt;        /* [ntok] factor on vec (NULL -> 1)                                 */
    int32_t ldv, ntok;
    const aim_bf16* aux;    /* [M, ldaux] saved pre-activation (AIM_EPI_DACT)                   */
    int32_t ldaux;
    void* out;  int32_t ldo;
    void* out2; int32_t ldo2;
    float scale;            /* logit scale (AIM_EPI_EXPSUM)                                     */
    int32_t act;            /* AIM_ACT_*                                                        */
    int32_t rs_bias_only;   /* AIM_EPI_F32: apply rs to the bias term only                      */
    /* column split for fused [frozen MLP | adapter] GEMMs (ACT / DACT): when n_split > 0, columns
       n < n_split use `act` with rs = 1, columns n >= n_split use `act2` with the row factor rs.
       n_split must be a multiple of 4 (8 for aim_gemm_fp8) and at most N; other values are refused. */
    int32_t n_split, act2;
    /* AIM_EPI_EXPSUM, one 256x256 tile per batch item (128 < max(M, N), N < 256) only: an EXTRA key.  Row N of W for batch
       item z is xrow + z * ldx (K elements); the scores against it (column N of the tile) are reduced apart into slots
       8..15 of the item's 16 (max, sum) slots -- lamda's `cw` rides along with its `ow` (vit_clip.py:149-151,184-186). */
    const aim_bf16* xrow;
    int32_t ldx;
    /* Scheduling knob of THIS launch (no reference counterpart): the large-tile GEMM is persistent (one workgroup per
       CU); with reserve_cus > 0 its grid leaves that many CUs free, so that kernels queued on ANOTHER stream (the
       class-token chain beside the QKV projection) are not starved. */
    int32_t reserve_cus;
    /* Diagnostics of THIS launch (tools/probe_gemm.py only): when probe != NULL (device memory, probe_cap x 4 uint64)
       the large-tile kernel records {workgroup | K-loop cycles, tile start, K-loop end, epilogue end} (100 MHz ticks)
       per processed tile. */
    void* probe;
    int32_t probe_cap;
    /* per-output-channel dequantisation scale of W (aim_gemm_fp8): acc is multiplied by wscale[n] before bias / act /
       row factors.  NULL -> 1.  */
    const float* wscale;
    /* AIM_EPI_ACT / AIM_EPI_DACT: what `out2` / `aux` hold.  0: the pre-activation (the DACT epilogue evaluates the
       derivative from it).  1: the activation's DERIVATIVE at the bf16-rounded pre-activation, computed by the ACT epilogue
       from the sigmoid / normal CDF it needs anyway -- the DACT epilogue is then dgrad x aux x row factor, no
       transcendentals (a pre-activation is saved for the backward only: vit_clip.py:80-82,93-97 under autograd). */
    int32_t aux_grad;
    /* AIM_EPI_ACT / AIM_EPI_DACT on the large-tile kernel (M >= 1024, batch 1): `out2` / `aux` is a FRAGMENT-ordered buffer,
       private to the pair of launches with the same M and N: (ceil(M/256) x ceil(N/256) tiles) x [8 waves][32 fragments]
       [64 lanes] x 4 bf16 -- each lane's own accumulator elements, so neither epilogue re-tiles it (ldo2 / ldaux are
       ignored; the buffer holds ceil(M/256) * ceil(N/256) * 65536 elements). */
    int32_t aux_frag;
    /* Row index, in the caller's whole problem, of row 0 of THIS launch's A / out / resid pointers: the row factors are read
       as af[(row0 + m) / ntok], at[(row0 + m) % ntok] (same for vec / bt).  0 for a whole problem.  The library uses it
       itself when it peels the thin last tile round of a large launch into a second, low-latency launch (AIM_GEMM_PEEL);
       the small-tile kernels honour it, the persistent 256 x 256 kernel requires 0. */
    int32_t row0;
    /* != 0 (ABI 9; bf16 GEMM, K % 64 == 0, not EXPSUM): run this launch on the 64 x 64 kernel whatever M is.  That kernel
       walks K in the persistent 256 x 256 kernel's order with the same epilogue arithmetic, so a launch over a SUBSET of the
       rows of a large problem gives those rows the bits the large launch gives them (the 128 x 128 kernel that M < 1024
       otherwise selects sums K in another order).  The last block's class-row launches set it. */
    int32_t small_tile;
} aim_gemm_args;

int aim_gemm_bf16(const aim_gemm_args* args, int epilogue, int batch, void* stream);

/* fp8 inference GEMM (BASELINE configs[4]; no reference counterpart -- the reference runs apex-O1 fp16):
 *   C[m][n] = wscale[n] * sum_k A8[m][k] * W8[n][k]
 * A and W hold OCP e4m3 bytes (K-contiguous; lda / ldw / K in elements, multiples of 16), products run on the
 * block-scaled MFMA v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (2x the bf16 MFMA rate), fp32 accumulate.
 * Weights are quantised once per output channel (wscale[n] = amax_n / 448), activations are saturating casts made by
 * the producing kernel (aim_layernorm_fwd y_fp8, AIM_EPI_ACT8, aim_attn_fwd out_fp8).  Epilogues: AIM_EPI_BF16,
 * AIM_EPI_F32, AIM_EPI_ACT8, AIM_EPI_RES16.  Large-M problems only (M >= 1024, N >= 64, N % 8 == 0). */
int aim_gemm_fp8(const aim_gemm_args* args, int epilogue, void* stream);
/* number of (max,sum) pairs AIM_EPI_EXPSUM writes per batch entry */
int aim_gemm_expsum_tiles(int M, int N);

/* ------------------------------------------------------------------------------------------
 * Weight-gradient GEMM for the (trainable) adapters:
 *   dW[n][k] += sum_m G[m][n] * A[m][k]      db[n] += sum_m G[m][n]
 * With a workspace the split-M partial slabs are summed in a fixed order by a second kernel (no atomics, bitwise
 * reproducible: the form the training step uses); workspace == NULL falls back to fp32 atomics.
 * autograd counterpart of Adapter.D_fc1 / D_fc2 (vit_clip.py:57-58).  Nw, Kw multiples of 8; ldg, lda multiples of 8 and
 * lddw a multiple of 4, each at least a row long (ldg >= Nw, lda >= Kw, lddw >= Kw: anything else is refused, here and by
 * aim_wgrad_slabs_bf16).
 * ------------------------------------------------------------------------------------------ */
int aim_wgrad_bf16(const aim_bf16* G, int ldg, const aim_bf16* A, int lda, float* dW, int lddw,
                   float* db, int M, int Nw, int Kw,
                   float* workspace /* optional: aim_wgrad_workspace_bytes(); NULL -> fp32 atomics (not reproducible) */,
                   int64_t workspace_bytes, void* stream);
int64_t aim_wgrad_workspace_bytes(int M, int Nw, int Kw);
/* the same with the bias gradient's row factor: db[n] += sum_m at[m % ntok] * G[m][n] (at == NULL: 1), summed inside the
 * weight-gradient kernel from the G rows it already holds in LDS (no separate pass over G).  The DropPath-scaled bias of
 * the MLP_Adapter's D_fc2 (vit_clip.py:286) is the user. */
int aim_wgrad_bias_bf16(const aim_bf16* G, int ldg, const aim_bf16* A, int lda, float* dW, int lddw, float* db,
                        const float* at, int ntok, int M, int Nw, int Kw, float* workspace, int64_t workspace_bytes, void* stream);

/* The two halves of aim_wgrad_bias_bf16 apart (ABI 14), for a gradient whose rows are summed by more than one launch:
 * aim_wgrad_slabs_bf16 writes the partial sums of rows [m_begin, m_end) of the problem (G, A point at its row 0; the row
 * factors are at[m % ntok] of that absolute row index) as at most max_chunks (<= 0: the library's choice) slabs
 * slabs[c][Nw][Kw] and, with bias_slabs != NULL, bias_slabs[c][Nw]; *chunks_written = the slabs it filled.  aim_wgrad_finish
 * adds nchunks consecutive slabs, in that order, into dW / db (bias_slabs, db NULL: weights only).  No atomics anywhere. */
int aim_wgrad_slabs_bf16(const aim_bf16* G, int ldg, const aim_bf16* A, int lda, const float* at, int ntok, int m_begin,
                         int m_end, int Nw, int Kw, float* slabs, float* bias_slabs, int max_chunks, int* chunks_written,
                         void* stream);
int aim_wgrad_finish(const float* slabs, const float* bias_slabs, int nchunks, float* dW, int lddw, float* db, int Nw, int Kw,
                     void* stream);

/* Rider workgroups (ABI 14; no reference counterpart -- scheduling).  The persistent large-tile GEMM sizes its grid so that
 * the last tile round is full, which leaves CUs idle for the whole launch (1 182 tiles: 237 workgroups on 256 CUs).
 * aim_gemm_bf16_ride is aim_gemm_bf16 (batch 1, AIM_EPI_BF16 or AIM_EPI_DACT, a problem the large-tile kernel runs in one
 * launch) whose launch carries tiles(Nw, Kw) * chunks more workgroups; each sums one 256 x 256 tile of a weight gradient
 * over one chunk of rows [m_begin, m_end) into slabs[c][Nw][Kw] (and bias_slabs[c][Nw]) as aim_wgrad_slabs_bf16 does;
 * *chunks_written slabs are filled.  The GEMM's output has the bits of the launch without riders; riders and GEMM
 * workgroups share nothing, a slab is complete when the launch is.  at needs bias_slabs and ntok <= 4096.
 * aim_wgrad_ride_plan is the policy: how many chunks and rows (from rows_left of a gradient of M_total rows) this host
 * launch should carry -- 0 / 0: none.  It depends on the shapes, the CU count, reserve_cus and AIM_WGRAD_RIDE (0: never)
 * only; AIM_WGRAD_RIDE_C overrides the measured ratio of a host K-step's time to a rider step's, AIM_WGRAD_RIDE_DACT=0 keeps
 * riders off AIM_EPI_DACT launches. */
typedef struct aim_wgrad_ride_args {
    const aim_bf16* G;      /* [M, ldg] gradient rows, row 0 of the whole problem                */
    const aim_bf16* A;      /* [M, lda] activation rows                                          */
    int32_t ldg, lda, Nw, Kw;
    int32_t m_begin, m_end; /* the rows the riders sum                                           */
    const float* at;        /* [ntok] bias row factor or NULL                                    */
    int32_t ntok;
    int32_t chunks;         /* row chunks per tile (riders = tiles * chunks; empty chunks are not launched) */
    float* slabs;           /* [chunks][Nw][Kw]                                                  */
    float* bias_slabs;      /* [chunks][Nw] or NULL: no bias gradient                            */
} aim_wgrad_ride_args;
int aim_gemm_bf16_ride(const aim_gemm_args* args, int epilogue, const aim_wgrad_ride_args* ride, int* chunks_written, void* stream);
int aim_wgrad_ride_plan(const aim_gemm_args* host, int epilogue, int Nw, int Kw, int ntok, int M_total, int rows_left,
                        int* chunks, int* rows);

/* ------------------------------------------------------------------------------------------
 * LayerNorm (fp32 statistics, eps inside rsqrt) -- vit_clip.py:71-77 (ln_1, ln_2, ln_pre, ln_post)
 *   fwd: y = (x - mean) * rstd * gamma + beta ; x fp32 rows with stride ldx; y as bf16 and/or f32
 *   bwd: dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma   (frozen gamma)
 *        optional: dgamma/dbeta accumulation for the trainable ln_post (rows <= 8192: one ordered column pass,
 *        no atomics; more rows: per-element fp32 atomics).
 * ------------------------------------------------------------------------------------------ */
int aim_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta,
                      aim_bf16* y_bf16, float* y_f32, int64_t ldy, float* mean, float* rstd,
                      int rows, int D, float eps, void* stream);
/* inference form: y as fp8 e4m3 bytes (saturating cast, row stride ldy bytes); no statistics are saved */
int aim_layernorm_fwd_fp8(const float* x, int64_t ldx, const float* gamma, const float* beta, uint8_t* y_fp8,
                          int64_t ldy, int rows, int D, float eps, void* stream);
/* the same LayerNorm over bf16 rows (the fp8 inference path keeps its residual stream in bf16: AIM_EPI_RES16);
 * any subset of the three outputs */
int aim_layernorm_fwd_x16(const aim_bf16* x, int64_t ldx, const float* gamma, const float* beta, aim_bf16* y_bf16,
                          float* y_f32, uint8_t* y_fp8, int64_t ldy, int rows, int D, float eps, void* stream);
int aim_layernorm_bwd(const void* dy, int dy_is_bf16 /* dy is bf16 (1) or f32 (0) */, int64_t lddy,
                      const float* x, int64_t ldx, const float* gamma,
                      const float* mean, const float* rstd, const void* dres, int dres_is_bf16,
                      int64_t lddres /* row stride of dres (ABI 9; it shared lddx before) */, float* dx,
                      aim_bf16* dx_bf16, int64_t lddx, float* dgamma, float* dbeta,
                      int rows, int D, void* stream);
/* The bf16 form of aim_layernorm_bwd (dy, dres, dx all bf16, rows = frames*ntok) that also emits per-frame weighted column
 * sums of the dx it stores: fsum_partial[frame][g][c] = sum over token group g (ceil(ntok/groups) tokens) of
 * w[n] * dx_bf16[frame*ntok + n][c]   (w NULL = 1).  aim_frame_sum(fsum_partial, f32, NULL, out, frames, groups, D) finishes
 * it: the backward's sum_n dms1[n] d(x1)[frame, n, :] (autograd of the broadcast S_Adapter term, vit_clip.py:272-275)
 * without a second pass over d(x1). */
int aim_layernorm_bwd_fsum(const aim_bf16* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                           const float* mean, const float* rstd, const aim_bf16* dres, aim_bf16* dx_bf16, int64_t lddx,
                           const float* w, float* fsum_partial, int groups, int frames, int ntok, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spatial multi-head self-attention over the N tokens of each frame (flash-style, scores never
 * leave the CU) -- vit_clip.py:139-156 (reshape, q k^T / sqrt(dh), softmax, @ v, merge heads).
 *   qkv [BT*N, 3*D] bf16 (q | k | v, D = H*64) ; out [BT*N, D] bf16 ; lse [BT, H, N] f32
 *   bwd: dqkv [BT*N, 3*D] bf16 from dout [BT*N, D] bf16 (recomputes the probabilities from lse).
 * ------------------------------------------------------------------------------------------ */
int aim_attn_fwd(const aim_bf16* qkv, aim_bf16* out, float* lse, int BT, int N, int H, void* stream);
/* inference form: out as fp8 e4m3 bytes [BT*N, D] (operand of the fp8 out_proj GEMM); lse may be NULL */
int aim_attn_fwd_fp8(const aim_bf16* qkv, uint8_t* out_fp8, float* lse, int BT, int N, int H, void* stream);
int aim_attn_bwd(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse,
                 float* delta /* scratch [BT, H, N] f32 */, aim_bf16* dqkv, int BT, int N, int H,
                 void* stream);
/* The class query (token 0) of every (frame, head) only (ABI 9): the last block of the backbone, whose other rows nobody
 * reads.  fwd: out_cls [BT, D] bf16, lse_cls [BT, H] f32 -- row 0 of aim_attn_fwd's results, bit for bit.
 * bwd: from dout_cls [BT, D] (the gradient of every other row of the attention output is zero) WRITES the whole
 * dqkv [BT*N, 3*D]: dk, dv of every key, dq in the class rows, zeros in every other dq row.  The q part of the other rows of
 * qkv is not read.  Same shapes as aim_attn_fwd (N <= 288, 64-wide heads); fixed summation order, no atomics. */
int aim_attn_fwd_cls(const aim_bf16* qkv, aim_bf16* out_cls, float* lse_cls, int BT, int N, int H, void* stream);
int aim_attn_bwd_cls(const aim_bf16* qkv, const aim_bf16* out_cls, const aim_bf16* dout_cls, const float* lse_cls,
                     aim_bf16* dqkv, int BT, int N, int H, void* stream);
/* Head-shifted form (ABI 10; ViT_CLIP_ZEROI2V's HeadShift, vit_clip_zeroI2V.py): BT = B*T frames, clips of T consecutive
 * frames.  In head h the queries of frame (b, t) attend to the K and V of frame (b, (t - shifts[h]) mod T) of the same clip --
 * torch.roll(k, shifts[h], dims=t) -- q, out, lse and dout stay in frame (b, t).  bwd: dq in the query's frame; dk, dv are
 * written to the frame the keys were read from (per head the map is a bijection on the clip: one writer per row, no atomics,
 * nothing is summed across items).  shifts: H ints in HOST memory, |shifts[h]| < T, read during the call and passed to the
 * kernels by value (H <= 16, T <= 256): nothing is allocated or kept.  Results are the bits of aim_attn_fwd / aim_attn_bwd on
 * a qkv whose K and V columns were rolled that way (dk, dv rolled back); an all-zero table gives the unshifted bits. */
int aim_attn_fwd_shift(const aim_bf16* qkv, aim_bf16* out, float* lse, int BT, int N, int H, int B, int T, const int* shifts,
                       void* stream);
int aim_attn_bwd_shift(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse,
                       float* delta /* scratch [BT, H, N] f32 */, aim_bf16* dqkv, int BT, int N, int H, int B, int T,
                       const int* shifts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Self-attention inside 3-D windows of the patch grid (ABI 11; AIM_FLASH_WIN's temporal branch,
 * vitclip_aim_flash_win.py:146-225: window_partition, attention, window_reverse on the patch tokens).
 *   B clips of T frames of N = G*G + 1 tokens, stored P >= N token rows per frame (P > N: spare rows behind a frame's
 *   tokens, e.g. the slot of a prompt token; never touched).  A window of (wt, wh, ww) holds the S = wt*wh*ww patch
 *   tokens (dt, dh, dw) whose row is (b*T + it*wt + dt)*P + 1 + (ih*wh + dh)*G + iw*ww + dw.  The gather and its inverse are
 *   addresses inside the kernels: no window-partitioned copy of anything exists.  An extent that reaches the grid's is
 *   clipped to it (the reference's get_window_size); the clipped extents must divide (T, G, G).
 *   qkv [B*T*P, 3*D] bf16 (q | k | v, D = H*64) ; out, dout [B*T*P, D] bf16 ; dqkv [B*T*P, 3*D] bf16 ;
 *   lse, delta [B*T, H, P] f32 (delta = dout . out per row and head: written by bwd, scratch for the caller).
 *   The class row (token 0) and the spare rows of every frame are never read, and never written in out, lse, delta, dqkv.
 * Streaming softmax: K and V pass through LDS in 64-key tiles under an online (max, sum) rescale, so S is bounded only by
 * AIM_WIN_ATTN_MAX_S; more, a non-square N - 1 or extents that do not divide are refused before any launch.
 * bwd recomputes the probabilities from lse in two kernels (delta + dQ with the queries resident, then dK + dV with the
 * keys resident): one writer per row, fixed summation order, no atomics, the same bits on every run.  Nothing is summed
 * across workgroups, so bwd takes no workspace; `delta` is its only scratch.
 * ------------------------------------------------------------------------------------------ */
#define AIM_WIN_ATTN_MAX_S 4096
int aim_win_attn_fwd(const aim_bf16* qkv, aim_bf16* out, float* lse, int B, int T, int N, int P, int H, int wt, int wh,
                     int ww, void* stream);
int aim_win_attn_bwd(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse, float* delta,
                     aim_bf16* dqkv, int B, int T, int N, int P, int H, int wt, int wh, int ww, void* stream);

/* Shifted-window form (ABI 12; AIM_FLASH's odd blocks, vitclip_aim_flash.py: roll by -shift, border strips, attention inside
 * each strip, stitch, roll back).  Buffers, layouts and guarantees are those of aim_win_attn_fwd / aim_win_attn_bwd; only the
 * grouping of the patch tokens into sequences differs.  With (wt, wh, ww) the clipped extents and (st, sh, sw) the shifts, in
 * ORIGINAL (unrolled) coordinates and each axis on its own:
 *   h (w alike), sh > 0: [0, G) is cut at 0, sh, sh + wh, sh + 2*wh, ..., G: a first segment of sh rows, whole windows, a last
 *     segment of wh - sh.  Nothing wraps.  sh = 0: the windows [ih*wh, (ih+1)*wh).
 *   t: whole windows in rolled coordinates; window k holds the frames (k*wt + st + dt) mod T, dt = 0 .. wt-1, of its own clip.
 * One sequence is one (t window, h segment, w segment) box with its tokens in (dt, dh, dw) row-major order; attention is
 * plain softmax self-attention inside the box, and every patch token lies in exactly one box.  The boxes and the t wrap are
 * addresses inside the kernels: no rolled or strip-ordered copy of anything exists, and all (box, head) items of every size
 * run in one launch (three for bwd).
 * Bit-for-bit: st = sh = sw = 0 gives the bits of aim_win_attn_fwd / aim_win_attn_bwd; sh = sw = 0, st > 0 gives the bits of
 * those entries on buffers whose frames were rolled by -st inside each clip, rolled back by +st.
 * Refused before any launch: a shift < 0 or >= its clipped extent, a non-zero shift on an axis whose clipped extent equals
 * the grid's, and everything aim_win_attn_* refuses. */
int aim_win_attn_fwd_shift(const aim_bf16* qkv, aim_bf16* out, float* lse, int B, int T, int N, int P, int H, int wt, int wh,
                           int ww, int st, int sh, int sw, void* stream);
int aim_win_attn_bwd_shift(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse, float* delta,
                           aim_bf16* dqkv, int B, int T, int N, int P, int H, int wt, int wh, int ww, int st, int sh, int sw,
                           void* stream);

/* Cut-window form (ABI 13; AIM's odd blocks, vitclip_aim.py:62-75 and :180-187: roll by -shift, whole windows of the rolled grid
 * under an additive -100 mask between compute_mask's regions, roll back).  Arguments, buffers, layouts, guarantees and refusals
 * are those of the *_shift entries; only the t axis is grouped differently: it is cut like h and w, at 0, st, st + wt, st + 2*wt,
 * ..., T (st = 0: the windows [it*wt, (it+1)*wt)), and no frame index is taken modulo T.  One sequence is one (t segment, h
 * segment, w segment) box, (T/wt + (st > 0)) * nh * nw of them per clip, tokens in (dt, dh, dw) row-major order, plain softmax
 * self-attention inside it; every patch token lies in exactly one box.  A pair of tokens the reference's mask separates gets a
 * weight of exactly 0 here, where the reference leaves at most (S - 1) e^(spread - 100) of probability mass (spread: the largest logit
 * difference inside a window).
 * Bit-for-bit: st = 0 gives the bits of aim_win_attn_fwd_shift / aim_win_attn_bwd_shift at the same (sh, sw), so the all-zero
 * shift gives those of aim_win_attn_fwd / aim_win_attn_bwd. */
int aim_win_attn_fwd_cut(const aim_bf16* qkv, aim_bf16* out, float* lse, int B, int T, int N, int P, int H, int wt, int wh,
                         int ww, int st, int sh, int sw, void* stream);
int aim_win_attn_bwd_cut(const aim_bf16* qkv, const aim_bf16* out, const aim_bf16* dout, const float* lse, float* delta,
                         aim_bf16* dqkv, int B, int T, int N, int P, int H, int wt, int wh, int ww, int st, int sh, int sw,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Temporal attention over the T class tokens of each clip -- vit_clip.py:220-224 with
 * attention() :139-156 at seq = T, batch = B.  Reads the class rows (token 0) of qkv.
 *   out_cls [B*T, D] bf16 ; probs [B, H, T, T] f32 (saved for backward)
 *   bwd: compact == 0: ADDS dq/dk/dv of the class rows into dqkv [BT*N, 3*D] (bf16, rows n == 0);
 *        compact != 0: WRITES them to dqkv [B*T, 3*D] (the class rows' share alone, for a separate dgrad).
 * ------------------------------------------------------------------------------------------ */
int aim_cls_attn_fwd(const aim_bf16* qkv, aim_bf16* out_cls, float* probs, int B, int T, int N, int H,
                     void* stream);
int aim_cls_attn_bwd(const aim_bf16* qkv, const float* probs, const aim_bf16* dout_cls, aim_bf16* dqkv, int compact,
                     int B, int T, int N, int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Temporal attention over the T frames of EVERY token position -- the stock-AIM block
 * (mmaction/models/backbones/vitclip_aim.py:199-205: attention() :148-187 on 'n (b t) d -> t (b n) d', seq = T, batch = B*N).
 *   qkv [B*T*N, 3*D] bf16 frame-major ; out [B*T*N, D] bf16 ; probs [B*N, H, T, T] f32 (saved for backward)
 *   bwd WRITES dqkv [B*T*N, 3*D] bf16.
 * aim_add_bf16: out = a + b (bf16, row strides) ; aim_acc_bf16: x (f32, dense) += s (bf16): the residual adds of that
 * block's S_Adapter branch (skip_connect=True, :211) that no GEMM epilogue of this library covers.
 * ------------------------------------------------------------------------------------------ */
int aim_tattn_fwd(const aim_bf16* qkv, aim_bf16* out, float* probs, int B, int T, int N, int H, void* stream);
int aim_tattn_bwd(const aim_bf16* qkv, const float* probs, const aim_bf16* dout, aim_bf16* dqkv, int B, int T, int N, int H,
                  void* stream);
/* inference forms of aim_tattn_fwd (ABI 15): no probabilities are stored (a forward without a backward has no reader for
 * them: at T = 32 they are 4 KB of stores per (token, head) beside 12 KB of loads).  Exactly one of out / out_fp8 is
 * non-NULL; both or neither is refused before any launch.  Same shapes as aim_tattn_fwd (T <= 32).
 *   out     [B*T*N, D] bf16 : the bits aim_tattn_fwd writes to `out`
 *   out_fp8 [B*T*N, D] e4m3 : the saturating cast (|x| clamped to 448) of the same fp32 accumulators -- the A operand of
 *                             the fp8 out_proj GEMM (aim_gemm_fp8); written as packed 32-bit stores, 4-byte aligned */
int aim_tattn_fwd_infer(const aim_bf16* qkv, aim_bf16* out, uint8_t* out_fp8, int B, int T, int N, int H, void* stream);
int aim_add_bf16(const aim_bf16* a, int64_t lda, const aim_bf16* b, int64_t ldb, aim_bf16* out, int64_t ldo, int R, int C,
                 void* stream);
int aim_acc_bf16(float* x, const aim_bf16* s, int64_t lds, int R, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused low-rank linear adapters (ABI 16) -- ZeroI2V's Linear_Adapter, vit_clip_zeroI2V.py:15-38: LA(x) = x + D_fc2(D_fc1(x)),
 * no activation, r hidden units.  Two chained MFMA products per adapter; the r-wide intermediate goes from the first to the
 * second through LDS and is also stored, rounded to bf16, because the other direction needs it.  G in {1, 3} adapters share
 * one input (forward) or one input gradient (backward).  Every weight is K-contiguous, dense:
 *   aim_lowrank_fwd   H_g  = bf16(X W1_g^T + b1_g)        wa[g] = W1_g   [r, D]   ba[g] = b1_g [r] f32 (NULL: none)
 *                     Y_g  = alpha X + H_g W2_g^T + b2_g  wb[g] = W2_g   [D, r]   bb[g] = b2_g [D] f32 (NULL: none)
 *                     x[0] = X [M, D] (ldx) ; h[g] = H_g [M, r] (ldh; NULL: not stored) ; y[g] = Y_g [M, D] bf16 (ldy).
 *                     G == 1 only: y32 [M, D] f32 (ld32) = resid (ldr) + Y_0 before its rounding; y[0] may then be NULL.
 *   aim_lowrank_bwd   dH_g = bf16(dY_g W2_g)              wa[g] = W2_g^T [r, D]
 *                     dX   = bf16(alpha sum_g dY_g + sum_g dH_g W1_g)      wb[g] = W1_g^T [D, r]
 *                     x[g] = dY_g [M, D] (one ldx) ; h[g] = dH_g [M, r] (ldh, required) ; y[0] = dX [M, D] (ldy).
 * The second product reads the ROUNDED intermediate.  alpha is 1 or 2.  No atomics and one summation order: equal bits on
 * every run.  Requirements: M >= 1; D a multiple of 64, at most 8192; r a multiple of 8, at most 256; ldx a multiple of 8,
 * ldh / ldy / ld32 / ldr multiples of 4; x and the weights 16-byte aligned, h and y 8-byte, biases / y32 / resid 16-byte.
 * Anything else is refused before any launch.
 * ------------------------------------------------------------------------------------------ */
typedef struct aim_lowrank_args {
    const aim_bf16* x[3];
    int32_t ldx;
    const aim_bf16* wa[3];
    const float* ba[3];
    aim_bf16* h[3];
    int32_t ldh;
    const aim_bf16* wb[3];
    const float* bb[3];
    aim_bf16* y[3];
    int32_t ldy;
    float* y32;
    const float* resid;
    int32_t ld32, ldr;
    int32_t M, D, r, G;
    float alpha;
} aim_lowrank_args;
int aim_lowrank_fwd(const aim_lowrank_args* a, void* stream);
int aim_lowrank_bwd(const aim_lowrank_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * lamda = cw / (cw + ow) per frame -- vit_clip.py:149-151, 184-186, 272.
 *   ow[bt] = sum_{i,j} exp(q_i . k_j / 8)  arrives as AIM_EPI_EXPSUM partial pairs
 *            partials [BT, ntiles, 2];  cw[bt] = sum_i exp(q_i . kx[bt] / 8) is computed here.
 *   Both sums share one max shift (identical ratio, no overflow).  lam [BT] f32; one_minus [BT].
 * ------------------------------------------------------------------------------------------ */
/* ss [BT, N] f32 = scale * q_i . kx[bt] (full width): the one pass over q that lamda's cw needs; aim_lambda accepts it so
 * that this pass can run as soon as q exists.  ss == NULL in aim_lambda: computed inside (one-call form). */
/* lamda from the 16 slots per frame of an AIM_EPI_EXPSUM launch with `xrow` (8 ow partials, 8 cw partials). */
int aim_lambda_partials(const float* partials, float* lam, float* one_minus_lam, int BT, void* stream);
int aim_qk_cross(const aim_bf16* qkv, const aim_bf16* kx, int ldkx, float* ss, int BT, int N, int D, float scale, void* stream);
int aim_lambda(const aim_bf16* qkv, const aim_bf16* kx, int ldkx, const float* ss, const float* partials, int ntiles,
               float* lam, float* one_minus_lam, int BT, int N, int D, float scale, void* stream);
/* lamda statistics when a frame has ONE token more than the large-tile GEMM's 256 rows (ViT-L/14, N = 257): the scores of tokens
 * 0 .. N-2 against each other are one full 256 x 256 tile per frame of aim_gemm_bf16(AIM_EPI_EXPSUM, M = N = 256, 8 slots
 * with a per-item slot stride of ldo floats); this adds the border -- (max, sum exp) of scale q_i . k_{N-1} (i < N-1) into
 * partials[bt][slot0] and of scale q_{N-1} . k_j (j < N) into partials[bt][slot0 + 1] -- and the cross scores
 * ss[bt][i] = scale q_i . kx[bt] in the same pass over q.  aim_lambda(ss, partials, nslots) finishes.  vit_clip.py:149-151,184-186 */
int aim_qk_border(const aim_bf16* qkv, const aim_bf16* kx, int ldkx, float* ss, float* partials /* [BT, nslots, 2] */, int slot0,
                  int nslots, int BT, int N, int D, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch embedding glue -- vit_clip.py:434-447.
 *   patchify: imgs [B,3,T,H,W] (f32, or uint8 with GPUNormalize mean/std fused:
 *             mmaction/utils/module_hooks.py:73-85) -> A [B*T*G*G, Kp] bf16, Kp = 3*p*p padded
 *             to a multiple of 64 with zeros (conv1 as a GEMM against conv1.weight.view(D,-1)).
 *   embed_ln: tok [B*T*G*G, D] bf16 + class/positional/temporal embeddings -> ln_pre ->
 *             x [B*T, N, D] f32 ; saves mean/rstd [B*T*N].
 *   embed_bwd: d(temporal_embedding)[T, D] += sum_{b,n} ln_pre_bwd(dx)  (two-stage ordered reduction through the
 *             workspace; workspace == NULL: fp32 atomics).
 * ------------------------------------------------------------------------------------------ */
int aim_patchify(const void* imgs, int in_dtype /* 0 f32, 1 uint8, 2 bf16 */, const float* mean3, const float* std3, aim_bf16* A,
                 int B, int T, int H, int W, int p, int Kp, void* stream);
/* patchify_blend: aim_patchify (in_dtype 0 f32 | 1 uint8) with a mini-batch blending applied while gathering, so no blended
 * copy of the clip batch is written (mmaction/datasets/blending_utils.py:74-152 after recognizers/base.py:254-255).  Clip b
 * pairs with clip partner[b] (int32 [B], device; b < B):
 *   mode 1 (MixupBlending) : lam * v(b) + oml * v(partner[b]), each product and the sum rounded separately (oml = 1 - lam in
 *                            f32, as torch computes it).  With mean3/std3 the clips are normalised first:
 *                            lam * norm(a) + oml * norm(b) (the reference's own Mixup cannot take uint8 into GPUNormalize).
 *   mode 2 (CutmixBlending): v(partner[b]) for pixels in rows [y1, y2) x columns [x1, x2) of every frame and channel, v(b)
 *                            elsewhere (0 <= x1 <= x2 <= W, 0 <= y1 <= y2 <= H; lam / oml unused). */
int aim_patchify_blend(const void* imgs, int in_dtype, const float* mean3, const float* std3, aim_bf16* A, int B, int T, int H,
                       int W, int p, int Kp, const int32_t* partner, int mode, float lam, float oml, int x1, int y1, int x2,
                       int y2, void* stream);
int aim_embed_ln(const aim_bf16* tok, const float* cls, const float* pos, const float* temporal,
                 const float* gamma, const float* beta, float* x, float* mean, float* rstd,
                 int B, int T, int N, int D, float eps, void* stream);
int aim_embed_bwd(const void* dx, int dx_is_bf16, const aim_bf16* tok, const float* cls, const float* pos,
                  const float* temporal, const float* gamma, const float* mean, const float* rstd,
                  float* dtemporal, int B, int T, int N, int D,
                  float* workspace /* optional scratch: two-stage, bitwise reproducible reduction */, int64_t workspace_bytes,
                  void* stream);
int64_t aim_embed_bwd_workspace_bytes(int B, int T, int N, int D);

/* ------------------------------------------------------------------------------------------
 * Small reductions / casts used by the block's backward and the optimizer boundary.
 *   frame_sum : out[frame][d] = sum_tok w[tok] * x[frame*ntok + tok][d]   (x f32, w may be NULL)
 *   colsum    : out[c] += sum_m rs(m) * X[m][c]   (X bf16; rs as in the GEMM).  C % 8 == 0, ldx % 8 == 0, C <= 2048:
 *               two-stage ordered reduction through the workspace (more than 64 rows and ceil(M / max(64, ceil(M/1024))) * C
 *               floats of workspace); without one, M <= 2048 runs as one block in a fixed order and a larger M adds one
 *               fp32 atomic per column per 64-row block.  Any other C or ldx: a scalar kernel that ignores the workspace and
 *               adds one fp32 atomic per column per row block (not reproducible above 64 rows).
 *   cast      : f32 -> bf16 (optionally transposed [R,C] -> [C,R]) for weight staging
 *   scale_rows: y[r][c] = s[r] * x[r][c]  (f32 x -> bf16 y), used for lamda * crs_attn
 * ------------------------------------------------------------------------------------------ */
int aim_frame_sum(const void* x, int x_is_bf16, const float* w, float* out, int frames, int ntok, int D, void* stream);
int aim_colsum_bf16(const aim_bf16* X, int ldx, const float* af, const float* at, int ntok,
                    float* out, int M, int C, float* workspace /* optional: >= 1024*C floats -> two-stage, no atomics */,
                    int64_t workspace_bytes, void* stream);
int aim_cast_bf16(const float* src, aim_bf16* dst, int R, int C, int transpose, int ldd /* dst row stride, 0 = dense */,
                  void* stream);
int aim_scale_rows(const float* x, const float* s, aim_bf16* y, float* y_f32, int R, int C, void* stream);
/* dst[r * dst_row_stride + c] += src[r * C + c] (bf16 += fp32): folds the class rows' gradient share, computed apart on
 * the side stream, into a token-major tensor (dst_row_stride = N * D selects the class rows). */
int aim_add_rows_bf16(aim_bf16* dst, int64_t dst_row_stride, const float* src, int R, int C, void* stream);

/* A table of casts in ONE launch: dst = bf16(src) or bf16(src^T) with row stride ldd, for the ~150 small
 * adapter tensors that must be re-staged as bf16 GEMM operands after every optimizer step.  The table
 * lives in DEVICE memory (built once; the pointers are stable). */
typedef struct aim_cast_desc {
    const float* src;   /* [R, C] dense fp32 */
    void* dst;          /* bf16 [R, ldd] or, transposed, [C, ldd]; transpose == 2: fp32 [R, ldd] plain copy */
    int32_t R, C, ldd, transpose;
} aim_cast_desc;
int aim_cast_multi(const aim_cast_desc* table_dev, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer boundary: AdamW (torch.optim.AdamW semantics, decoupled decay) on ONE flat fp32 buffer
 * per parameter group -- the reference steps 149 small tensors through mmcv's optimizer hook
 * (mmaction/utils/optimizer.py:22-33, configs/recognition/vit/vitclip_base_k400.py:96-102).
 * `step` is the 1-based update count (bias correction).  p, g, m and v must be 16-byte aligned (the kernel moves four
 * floats at a time): a misaligned pointer is refused.
 * `grad_scale` multiplies g on the fly: 1 / world_size turns the SUM all-reduce of the flat gradient buffer into
 * DDP's mean (mmaction/apis/train.py:106-110) without a separate pass over the buffer.
 * ------------------------------------------------------------------------------------------ */
int aim_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Classification tail -- the callers right after the backbone:
 *   head_fwd : I3DHead.forward (mmaction/models/heads/i3d_head.py:53-73): adaptive average pool over the T frames of
 *              feat [B, T, D] f32 (the backbone's [B, D, T, 1, 1] output stored frame-major), optional dropout as a
 *              caller-drawn factor table drop[B, D] (0 or 1/(1-p); NULL = eval), fc_cls:
 *              pooled[b][d] = drop[b][d] * mean_t feat[b][t][d]  (saved for backward) ; score = pooled W^T + bias.
 *   head_bwd : dW[C, D] += dscore^T pooled ; db[C] += colsum(dscore) ; dfeat[b][t][d] = drop[b][d]/T * (dscore W)[b][d].
 *              dW, db and dfeat are each optional (NULL: not computed, the others unchanged); all three NULL is refused.
 *   ce_topk  : CrossEntropyLoss hard-label path (mmaction/models/losses/cross_entropy_loss.py:78) + top-k accuracy
 *              (mmaction/core/evaluation/accuracy.py:90-109, numpy argsort tie order: a label is in the top k iff
 *              fewer than k classes score higher or tie with a larger index), all on the device:
 *              out3 = {mean over VALID b of -log softmax(score)[label], top1, top5} ; dscore[B, C] = (softmax - onehot) / n_valid.
 *              A label outside [0, C) is ignored exactly like F.cross_entropy's ignore_index (-100): no loss term, a zero
 *              dscore row, not counted in the CE mean (top1 / top5 keep the denominator B: such a sample is a miss).
 *              One workgroup per sample writes per-sample terms, the last pass sums them in sample order (no atomics).
 * ------------------------------------------------------------------------------------------ */
int aim_head_fwd(const float* feat, const float* drop, const float* W, const float* bias, float* pooled, float* score,
                 int B, int T, int D, int C, void* stream);
int aim_head_bwd(const float* dscore, const float* pooled, const float* drop, const float* W, float* dW, float* db,
                 float* dfeat, int B, int T, int D, int C, void* stream);
int aim_ce_topk(const float* score, const int64_t* label, float* dscore, float* per_sample /* [B, 4] scratch */,
                float* out3, int B, int C, int k2 /* second k of the accuracy pair, 5 */, void* stream);
/* ce_soft : CrossEntropyLoss with soft labels and/or class_weight (mmaction/models/losses/cross_entropy_loss.py:52-80):
 *           label [B, C] f32 (soft labels, or an on-device one-hot of hard labels with zero rows for ignored ones),
 *           w = class_weight [C] or NULL (all ones).  loss_b = -sum_c w_c y_bc log_softmax(score)_bc;
 *           out[0] = sum_b loss_b / denom with denom = B (w NULL: the plain mean) or sum_b sum_c w_c y_bc (weighted, as
 *           F.cross_entropy(weight=w) and the reference's soft branch normalise); dscore[B, C] (or NULL) =
 *           (softmax * sum_c w y - w y) / denom.  One workgroup per sample, then an ordered finish (bitwise reproducible). */
int aim_ce_soft(const float* score, const float* label, const float* class_weight, float* dscore,
                float* per_sample /* [B, 2] workspace */, float* out /* [1] */, int B, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reference-precision (fp32) path: `ViT_CLIP.set_precision('fp32')`, forward AND backward.  The product path
 * computes on bf16 MFMA operands; these entry points compute the SAME block from fp32 operands with fp32 accumulation
 * (v_mfma_f32_16x16x4_f32: exact f32 products, 1/16 of the bf16 rate), exact erf / exp, probabilities normalised before
 * P V -- the arithmetic of the reference's un-autocast run (vit_clip.py:433-458), so the GPU output is held DIRECTLY to
 * the reference's fixtures at 1e-5 (BASELINE north_star), with no bf16-emulating oracle in between.
 *   gemm_f32       : C = A W^T with A, W, bias, resid, out all f32 (aim_gemm_args with float operands); epilogues
 *                    AIM_EPI_BF16 (read: linear, out(f32) = rs * (acc + bias)), AIM_EPI_ACT (out(f32) = [rs *] act(acc + bias),
 *                    n_split / act2 as above; out2 != NULL receives the f32 pre-activation acc + bias, ldo2 floats per row),
 *                    AIM_EPI_DACT (out = [rs *] acc * act'(aux): aux = that f32 pre-activation, ldaux floats per row; exact
 *                    erf / exp derivative; aux_grad / aux_frag are ignored), AIM_EPI_F32; batch > 1 (linear only) writes
 *                    item z at out + z * M * ldo.  K, lda, ldw multiples of 4; lda, ldw >= K, ldo >= N, ldr >= N, and ldv
 *                    either 0 (one row for every frame) or >= N: anything else is refused.
 *                    replaces vit_clip.py:93-97,132-138,157,286,436.
 *   attn_fwd_f32   : softmax(q k^T / 8) v per (frame, head) on the fused f32 qkv rows [BT*N, 3D]; out [BT*N, D].  :139-156
 *   cls_attn_fwd_f32 : the same over the T class tokens of each clip (sequence T, batch B); qkv rows of the class tokens
 *                    are `row_stride` floats apart (N * 3D in the fused buffer); out [B*T, D].  :220-229
 *   lambda_f32     : scores [BT][N][lds] = RAW full-width q_i . k_j (a batched gemm_f32 of q against k); kx [BT, ldkx] the
 *                    cross-attention's single key; lam = cw / (cw + ow) with ow = sum_ij exp(scale s_ij), cw = sum_i
 *                    exp(scale q_i . kx), one shared max shift.  :149-151,184-186,272
 *   patchify_f32 / embed_ln_f32 : aim_patchify / aim_embed_ln with an f32 patch matrix / f32 tokens (in_dtype 0 | 1).  :434-447
 *                    embed_ln_f32: pre / mean / rstd (all three or none) receive ln_pre's input rows [B*T*N, D] and statistics
 *                    -- what aim_layernorm_bwd needs for the gradient of the trainable temporal_embedding (:344,446).
 * Backward (the reference gets it from torch autograd; these follow autograd's formulas: softmax backward
 * dS = P o (dP - rowsum(P o dP)) then the 1/sqrt(dh) of :147, addmm backward for the Adapter's Linear layers):
 *   attn_bwd_f32   : dqkv [BT*N, 3D] (all three thirds WRITTEN) from qkv and d(out) [BT*N, D]; probabilities recomputed;
 *                    workspace of aim_attn_bwd_f32_workspace_bytes (row log-sum-exp and rowsum(P o dP)).  :139-156
 *   cls_attn_bwd_f32 : d(out_cls) [B*T, D] -> ADDED into the class rows of dqkv (row_stride floats apart), which already
 *                    hold the spatial attention's share (call after attn_bwd_f32).  :220-229
 *   wgrad_f32      : dW [Nw, Kw] += sum_m G[m][n] A[m][k]; db [Nw] += sum_m at[m % ntok] G[m][n] (at NULL -> 1; db NULL -> no
 *                    bias); G [M, ldg], A [M, lda] f32.  M is reduced in chunks whose partial results are summed in chunk
 *                    order (workspace of aim_wgrad_f32_workspace_bytes; no atomics).  Adapter.D_fc1 / D_fc2, :57-58,62-64
 * LayerNorm backward, the per-frame sums and the row scaling of the fp32 backward are the f32 forms of aim_layernorm_bwd,
 * aim_frame_sum and aim_scale_rows above.
 * ------------------------------------------------------------------------------------------ */
int aim_gemm_f32(const aim_gemm_args* args, int epilogue, int batch, void* stream);
int aim_attn_fwd_f32(const float* qkv, float* out, int BT, int N, int H, void* stream);
int aim_cls_attn_fwd_f32(const float* qkv, int64_t row_stride, float* out_cls, int B, int T, int H, void* stream);
int aim_lambda_f32(const float* scores, int lds, const float* qkv, const float* kx, int ldkx, float* lam,
                   float* one_minus_lam, int BT, int N, int D, float scale, void* stream);
int aim_patchify_f32(const void* imgs, int in_dtype, const float* mean3, const float* std3, float* A, int B, int T,
                     int H, int W, int p, int Kp, void* stream);
int aim_patchify_blend_f32(const void* imgs, int in_dtype, const float* mean3, const float* std3, float* A, int B, int T,
                           int H, int W, int p, int Kp, const int32_t* partner, int mode, float lam, float oml, int x1, int y1,
                           int x2, int y2, void* stream);    /* aim_patchify_blend with an f32 patch matrix (Kp % 4 == 0, as
                                                                  aim_patchify_f32 and the GEMM behind it require) */
int aim_embed_ln_f32(const float* tok, const float* cls, const float* pos, const float* temporal, const float* gamma,
                     const float* beta, float* x, float* pre, float* mean, float* rstd, int B, int T, int N, int D, float eps,
                     void* stream);
int64_t aim_attn_bwd_f32_workspace_bytes(int BT, int N, int H);
int aim_attn_bwd_f32(const float* qkv, const float* dout, float* dqkv, int BT, int N, int H, float* workspace,
                     int64_t workspace_bytes, void* stream);
int aim_cls_attn_bwd_f32(const float* qkv, int64_t row_stride, const float* dout_cls, float* dqkv, int B, int T, int H,
                         void* stream);
/* stock-AIM block (vitclip_aim.py:199-204): attention over the T frames of EVERY token, on the frame-major fused f32 qkv rows
   [B*T*N, 3D]; out / dout [B*T*N, D]; the backward ADDS into dqkv (zero it first when nothing else wrote it) */
int aim_tattn_fwd_f32(const float* qkv, float* out, int B, int T, int N, int H, void* stream);
int aim_tattn_bwd_f32(const float* qkv, const float* dout, float* dqkv, int B, int T, int N, int H, void* stream);
int64_t aim_wgrad_f32_workspace_bytes(int M, int Nw, int Kw);
int aim_wgrad_f32(const float* G, int ldg, const float* A, int lda, float* dW, int M, int Nw, int Kw, float* db,
                  const float* at, int ntok, float* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * ViT_ImageNet (reference vit_imagenet.py; ABI 8): embedding without ln_pre and the LayerNorm gamma / beta gradients of the
 * full-parameter backward.
 *   embed_nopre_fwd : x[bt*N + n] = ((n == 0 ? cls : tok[bt*(N-1) + n-1]) + pos[n]) + temporal[t]   (tok f32 [B*T*(N-1), D]:
 *                     the patch conv as a GEMM with its bias, :241-251; x f32 [B*T*N, D])
 *   embed_nopre_bwd : from dx [B*T*N, D] (bf16 or f32): dcls += sum_bt dx[bt, 0]; dpos[n] += sum_bt dx[bt, n];
 *                     dtemporal[t] += sum_{b, n} dx[b*T + t, n]; dbias += sum_{bt, n >= 1} dx[bt, n]; dtok (dx's dtype,
 *                     [B*T*(N-1), D]) = the token rows of dx (the conv weight gradient's operand).  Every output is optional
 *                     (NULL: skipped).  Fixed-order sums through the workspace: bitwise reproducible.
 *   layernorm_gb_bwd: dgamma[d] += sum_m dy[m][d] * (x[m][d] - mean[m]) * rstd[m], dbeta[d] += sum_m dy[m][d] over any
 *                     number of rows (row-chunk partial slabs, then an ordered sum: no atomics, bitwise reproducible).
 * ------------------------------------------------------------------------------------------ */
int aim_embed_nopre_fwd(const float* tok, const float* cls, const float* pos, const float* temporal, float* x, int B, int T,
                        int N, int D, void* stream);
int64_t aim_embed_nopre_bwd_workspace_bytes(int B, int T, int N, int D);
int aim_embed_nopre_bwd(const void* dx, int dx_is_bf16, void* dtok, float* dcls, float* dpos, float* dtemporal, float* dbias,
                        int B, int T, int N, int D, float* workspace, int64_t workspace_bytes, void* stream);
int64_t aim_layernorm_gb_bwd_workspace_bytes(int rows, int D);
int aim_layernorm_gb_bwd(const void* dy, int dy_is_bf16, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                         const float* rstd, float* dgamma, float* dbeta, int rows, int D, float* workspace,
                         int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * TimeSformer (reference timesformer.py; ABI 17): the FULL backward of the fused stem aim_embed_ln / aim_embed_ln_f32,
 * x = ln_pre(u), u[bt*N + n] = ((n == 0 ? cls : tok[bt*(N-1) + n-1]) + pos[n]) + temporal[t], for a model whose stem trains
 * (aim_embed_bwd gives d temporal only).  With xhat = (u - mean) rstd and g = gamma dx per row:
 *   du = rstd (g - mean_d(g) - xhat mean_d(g xhat));  dtok = rows n >= 1 of du, WRITTEN;
 *   dcls += sum_bt du[bt, 0]; dpos[n] += sum_bt du[bt, n]; dtemporal[t] += sum_{b, n} du[b*T + t, n];
 *   dgamma += sum_rows dx xhat; dbeta += sum_rows dx        (all five f32, ADDED into).
 * is_bf16 != 0: dx, tok and dtok are bf16 (the bf16 path); 0: all three f32.  Every output is optional (NULL: untouched); all
 * six NULL is refused.  fp32 arithmetic, one wave per row.  Two ordered stages through the workspace (3 N T D floats: one
 * partial row per (token, frame-time) and quantity, then fixed-order sums over them): no atomics, equal bits on every run, and
 * dcls's increment has the bits of dpos[0]'s.  Refused before any launch: D not a multiple of 4 or above 2048, N < 2,
 * N + T > 65535, a short workspace, dx / tok / dtok not aligned to four elements, cls / pos / temporal / gamma / workspace
 * not 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int64_t aim_embed_ln_bwd_workspace_bytes(int B, int T, int N, int D);
int aim_embed_ln_bwd(const void* dx, int is_bf16, const void* tok, const float* cls, const float* pos, const float* temporal,
                     const float* gamma, const float* mean, const float* rstd, void* dtok, float* dcls, float* dpos,
                     float* dtemporal, float* dgamma, float* dbeta, int B, int T, int N, int D, float* workspace,
                     int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * SwinTransformer2D_Adapter (reference swin2d_adapter.py; ABI 18): attention at head width 32 over sequences of at most 64
 * tokens under a dense additive bias, on the fused qkv [rows, 3 C] bf16 (C = 32 H, frame-major rows (frame, h, w)).
 *   win   : the window x window tokens of each window of the res x res grid rolled by -shift (:372-395); roll, partition and
 *           their inverses are addresses.  A (query, key) pair that the reference's attn_mask gives -100 has the weight
 *           exactly 0.  bias [H, S, S] f32, S = window^2, in window-local token order.  frames = B T'.
 *   tattn : the T frame tokens of each (clip, position) (:361-366): token t of (b, n) is row (b T + t) L + n; bias [H, T, T].
 * fwd writes out [rows, C] bf16 and lse [sequences, H, CAP] f32 (base 2; CAP = 32 where S <= 32, else 64).  bwd (from qkv, dout [rows, C] and the forward's lse; delta = sum_j p_j dP_j) writes dqkv
 * [rows, 3 C] bf16 (all three parts of every row) and, where dbias is not NULL, the dense bias gradient dbias [H, S, S] =
 * sum over sequences of P o (dP - delta): per-chunk partial sums in the workspace, added in a fixed order (no atomics; equal
 * bits on every run).  The 32^-1/2 scale is applied to the fp32 score; p and dS are rounded to bf16 as MFMA operands only.
 * bias_scatter: dtable[t][h] += sum of dense[h][e] over the entries e of index [SS] (int32) equal to t, in ascending order.
 * Refused before any launch: window^2 > 64, a window that does not divide res, a shift outside [0, window) or on a window
 * that spans the grid, T > 32, buffers that are not 16-byte aligned, a short workspace.
 * ------------------------------------------------------------------------------------------ */
int aim_swin_win_attn_fwd(const aim_bf16* qkv, const float* bias, aim_bf16* out, float* lse, int frames, int res, int H, int window,
                          int shift, void* stream);
int aim_swin_win_attn_bwd(const aim_bf16* qkv, const float* bias, const aim_bf16* dout, const float* lse,
                          aim_bf16* dqkv, float* dbias, int frames, int res, int H, int window, int shift, float* workspace,
                          int64_t workspace_bytes, void* stream);
int aim_swin_tattn_fwd(const aim_bf16* qkv, const float* bias, aim_bf16* out, float* lse, int B, int T, int L, int H, void* stream);
int aim_swin_tattn_bwd(const aim_bf16* qkv, const float* bias, const aim_bf16* dout, const float* lse,
                       aim_bf16* dqkv, float* dbias, int B, int T, int L, int H, float* workspace, int64_t workspace_bytes,
                       void* stream);
int64_t aim_swin_attn_bwd_workspace_bytes(int sequences, int H, int S);
int aim_swin_bias_scatter(const float* dense, const int* index, float* dtable, int H, int SS, int ntable, void* stream);

/* ------------------------------------------------------------------------------------------
 * SwinTransformer3D (reference swin_transformer.py; ABI 19): attention at head width 32 inside 3-D windows under the learned
 * 3-D relative-position bias, on the fused qkv [rows, 3 C] bf16 (C = 32 H, rows (clip, d, y, x) of a (D, G, G) token grid, no
 * class row).  (wt, wh, ww) is the effective window (after the reference's get_window_size), (st, sh, sw) the shift and
 * (Wt, Wh, Ww) the full window of the constructor, which gives the strides of table [(2Wt-1)(2Wh-1)(2Ww-1), H] f32.
 * A sequence is one box of the partition that cuts each axis at 0, s, s + w, ... (0, w, 2w, ... where the shift is 0): the
 * reference's roll, window_partition, -100 mask and their inverses, a masked pair having the weight exactly 0.  The bias of
 * (query, key) is table[f(q) - f(k) + f(Wt-1, Wh-1, Ww-1)][h], f(t, h, w) = (t (2Wh-1) + h)(2Ww-1) + w.
 * Capacity: wt wh ww <= 1024 tokens per window and at most 5248 table entries; (16,7,7) has 784 and 5239.
 * fwd writes out [rows, C] bf16 and lse [rows, H] f32 (base 2).  bwd (from qkv, dout [rows, C] and the forward's lse) writes
 * delta [rows, H] f32 (sum_j p_j dP_j), dqkv [rows, 3 C] bf16 (all three parts of every row) and, where dtable is not NULL,
 * ADDS the table gradient (sum of the unrounded fp32 dS, no scale factor) onto dtable [table, H]: dense per-walk partial sums
 * in the workspace, added in a fixed order (no atomics; equal bits on every run; dqkv does not depend on dtable being asked for).
 * The 32^-1/2 scale is applied to the fp32 score; p and dS are rounded to bf16 as MFMA operands only.
 * Refused before any launch: a window that does not divide D or G, a shift outside [0, w) or non-zero on an axis its window
 * spans, a full window smaller than the effective one, more tokens or table entries than the capacity, rows that overflow
 * 32-bit offsets, null pointers, bf16 buffers off 16 bytes or fp32 buffers off 4, a short workspace.
 * ------------------------------------------------------------------------------------------ */
int aim_swin3d_attn_fwd(const aim_bf16* qkv, const float* table, aim_bf16* out, float* lse, int clips, int D, int G, int H, int wt,
                        int wh, int ww, int st, int sh, int sw, int Wt, int Wh, int Ww, void* stream);
int aim_swin3d_attn_bwd(const aim_bf16* qkv, const float* table, const aim_bf16* dout, const float* lse, float* delta,
                        aim_bf16* dqkv, float* dtable, int clips, int D, int G, int H, int wt, int wh, int ww, int st, int sh,
                        int sw, int Wt, int Wh, int Ww, float* workspace, int64_t workspace_bytes, void* stream);
int64_t aim_swin3d_attn_bwd_workspace_bytes(int clips, int D, int G, int H, int wt, int wh, int ww, int st, int sh, int sw);

#ifdef __cplusplus
}
#endif
#endif /* AIM_KERNELS_H */
