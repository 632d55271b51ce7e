"""Every call form of the reference-precision kernels of csrc/fp32.hip (`set_precision('fp32')`): aim_gemm_f32 with its four
epilogues, aim_attn_fwd_f32 / _bwd_f32, aim_cls_attn_fwd_f32 / _bwd_f32, aim_tattn_fwd_f32 / _bwd_f32, aim_lambda_f32,
aim_wgrad_f32, aim_embed_ln_f32, aim_patchify_f32 and aim_patchify_blend_f32, against float64 references with bounds
derived from the kernels' rounding points.

A plain module (no fixtures).  None of these kernels reads an environment switch, so `run(dev)` executes every case in the
calling process through ctypes (`load_library()`), with every workspace and every output buffer handed in filled with NaN;
`test_fp32_cases_gpu.py` reads its records and `test_fp32_cases_cpu.py` proves on the CPU that the bounds accept an fp32
evaluation of each kernel's arithmetic (`emulate`) and reject the same evaluation with one plausible bug (`emulate(.., mut)`).
Operands are full fp32 values (torch.randn and products of it), never bf16-representable.  The float64 references are
computed on the device the case runs on.

Notation: u = 2^-24.  Every bound is a worst-case sum over absolute values, so it holds for any summation order.  TINY =
2^-126 is added to every bound that has a transcendental in it: an fp32 result below the smallest normal may be flushed to
(signed) zero, e.g. QuickGELU at pre = -100 gives -0 against -1e-72.

gemm_f32 (gemm_f32_kernel: v_mfma_f32_16x16x4_f32, exact products, an fp32 chain over k with an internal order of 4):
    e_acc = (K + 2) u sum_k |a_k w_k|
    linear:  out = rs (acc + b), rs = af[frame] at[tok] (one more rounding):
             |rs| (e_acc + u (|acc| + |b|)) + 2 u |out|
    F32:     out = ((rs (acc + b) | acc + rs b) + resid) + bt vec: five IEEE operations on the magnitudes involved:
             max(|rs|, 1 if rs_bias_only) e_acc + 5 u (|rs| (|acc| + |b|) + |acc| + |resid| + |bt vec|)
    ACT:     pre = acc + b: e_pre = e_acc + u (|acc| + |b|) (`out2` is held to exactly this: the acc bound plus one u);
             out = [rs] act(pre): |rs| (E_ACT (1 + |pre|) + |act'(pre)| e_pre) + 2 u |out| + TINY
    DACT:    takes the `aux` it is handed, so the float64 derivative d is evaluated at that fp32 value:
             out = [rs] acc d(aux): |rs| (|acc| E_DACT (1 + |aux|) + |d| e_acc) + 3 u |out| + TINY
  QuickGELU's 1.702 is the fp32 constant (the model's own arithmetic is fp32); GELU is stated with the exact 1 / sqrt(2) and
  1 / sqrt(2 pi), whose fp32 roundings cost less than u in erf's argument and are inside E_ACT.
  E_ACT = E_DACT = 2^-20 = 16 u (EPS_ACT of gemm_cases.py: an activation evaluated in fp32).  Measured on MI355X by the K = 4
  probe of `run_probe` (pre = x exactly, 2^18 points over [-110, 110] and the `bigpre` points), worst error / (1 + |x|):
  ACT QuickGELU 9.27e-8 (1.56 u), ACT GELU 7.98e-8 (1.34 u), DACT QuickGELU 1.21e-7 (2.03 u), DACT GELU 5.85e-8 (0.98 u): the
  precedent 2^-20 = 9.54e-7 is 7.9 times the worst of them, so it stays (MEASURED_ACT below; test_activation_constants
  asserts on the GPU that each constant is at least twice what the probe shows).

attn_fwd_f32 (attn_f32_kernel: a 64-term fmaf chain per score, * 1/8 exact, wave max, expf, lane sums + butterfly, one division,
an N-term fmaf chain for the output):
    e_s = 66 u sum_d |q_d k_d| / 8
    z = s - max: r_exp = e_s + max_j e_s + u |z| + C_EXP u            (relative error of exp(z); C_EXP = 4 as attn_cases.py)
    sum: r_sum = max_j r_exp + (ceil(N/64) + 6 + 2) u ;  p = exp / sum: r_p = expm1(r_exp + r_sum + 2 u), e_p = p r_p + TINY
    out: sum_j e_p,j |v_j| + (N + 1) u sum_j p_j |v_j|
attn_bwd_f32 (attn_bwd_dq_f32_kernel, attn_bwd_dkv_f32_kernel).  The dq kernel recomputes p as the forward does; the dk / dv
kernel takes p = exp(s - L) with L = max + logf(sum) from `stats`: that costs C_LOG u + 3 u (|s| + |L|) more, and the one
larger relative error r_p' = expm1(r_exp + r_sum + 2 u + C_LOG u + 3 u (|s| + |L|)) is used for all three gradients:
    dP = dO . v:  e_dP = 66 u sum_d |dO_d v_d|
    del = sum_j p_j dP_j:  e_del = sum_j (e_p |dP| + p e_dP) + (ceil(N/64) + 6 + 2) u sum_j p_j |dP_j|
    dS = p (dP - del) / 8 (three roundings):  e_dS = (e_p |dP - del| + p (e_dP + e_del + u (|dP| + |del|))) / 8 + 2 u |dS|
    dq_i = sum_j dS_ij k_j:  sum_j e_dS |k_j| + (N + 1) u sum_j |dS_ij k_j|      (an N-chain of fmaf)
    dk_j = sum_i dS_ij q_i:  sum_i e_dS |q_i| + (N + 1) u sum_i |dS_ij q_i|
    dv_j = sum_i p_ij dO_i:  sum_i e_p |dO_i| + (N + 1) u sum_i p_ij |dO_i|
  dO = 0 gives dP = del = dS = 0 exactly: all three bounds collapse to 0 and the comparison demands exact zeros.

cls_attn / tattn f32 (seq_attn_f32_kernel, seq_attn_bwd_f32_kernel: sequences of T rows, one wave per (sequence, head); the
backward recomputes p as the forward does, there is no log and no stats buffer, so r_p is used, not r_p').  The
64-wide dot product is one product per lane and 6 butterfly steps: e_s = 8 u sum |q k| / 8, e_dP = 8 u sum |dO v|; the sum of
the T exponentials, del and dq are T-chains: the formulas above with (T + 2) for the sum and del, (T + 1) for out.  The backward
ADDS into a non-zero dqkv, whose initial value counts as a term: dq: |init| joins with one rounding; a key row is
accumulated T times, once per query (a T + 1 chain, every term ds q / p dO rounded once more):
    dk_tk: sum_tq e_dS |q| + (T + 2) u (|init| + sum_tq |dS q|) ;  dv_tk: sum_tq e_p |dO| + (T + 2) u (|init| + sum_tq p |dO|)
  `base_plus_zero`: the same call on zeroed gradient rows computes the same fp32 terms, so only the additions differ.  dq is
  added once: |base call - (zero call + base)| <= u |base call|, the one extra rounding.  A dk / dv element takes T additions
  in either call, each off by at most u of a partial sum that is at most |base| + sum |terms|: 2 T u (|base| + sum |terms|), where
  sum |terms| is the reference's sum_tq |dS q| (p |dO|) plus its error bound sum_tq e_dS |q| (e_p |dO|).

lambda_f32 (lambda_f32_kernel; scores are given):
    ss_i = scale (q_i . kx): e_ss = (ceil(D/64) + 6 + 1) u |scale| sum_d |q_d kx_d|
    both sums are taken under one fp32 shift mx, which cancels in the ratio whatever its value.  ow = sum_ij exp(scale s_ij - mx):
    argument error u |scale s| + u |scale s - mx|, so r_ow = max_ij(that) + C_EXP u + (ceil(N^2/256) + 6 + 3) u;
    cw = sum_i exp(ss_i - mx): r_cw = max_i(e_ss + u |ss - mx|) + C_EXP u + (ceil(N/256) + 6 + 3) u     (sums of positive terms)
    lam = cw / (cw + ow): relative, r_lam = expm1(r_cw + r_ow + 2 u) (+ N^2 TINY for flushed terms); one_minus = 1 - lam is
    held absolutely: u + e_lam.

wgrad_f32 (wgrad_f32_kernel + reduce_slabs_f32_kernel, colsum_f32_kernel): chunks = min(64, ceil(M/512)), chunk =
ceil16(ceil(M/chunks)); a partial is a `chunk`-long fmaf chain, the finish adds the partials in order, then into dW:
    dW: (chunk + chunks + 1) u (|dW_init| + sum_m |G_mn A_mk|)
    db: (chunk + chunks + 2) u (|db_init| + sum_m |at G|)            (one more rounding per term when `at` is given)

embed_ln_f32 (embed_ln_f32_kernel): pre = fp32((src + pos) + tmp), two IEEE additions: bound 0 against torch's fp32
evaluation.  x, mean and rstd: the LayerNorm-forward derivation of rowwise_cases.py with a lane chain of ceil(D/64), 6
butterfly steps, a division, and 1 / sqrtf:
    L = ceil(D/64) + 6 + 1;  e_mu = L u mean|v|;  e_d = e_mu + u |d|;  e_var = e_mu^2 + 2 mean(|d| e_d) + (L + 4) u var
    r_rs = e_var / (2 (var + eps)) + 4 u;  x: |gamma| rstd e_d + |gamma d rstd| (r_rs + 3 u) + u (|x| + |beta|)

patchify_f32 / patchify_blend_f32: the gather is a copy, the uint8 normalise is two IEEE operations ((v - mean) / std), mixup
is fp32(fp32(lam a) + fp32(oml b)) as aim_kernels.h states: bound 0 against torch's fp32 evaluation of the same operations;
the Kp padding columns are exactly 0.  The GPU shows no difference: division and the two mixup products are IEEE there.

Findings pinned by the cases: attn_f32_kernel stores V into LDS as 16-byte vectors at a base of N * 65 floats, 16-byte aligned
only when N % 4 = 0; every N from 1 to 317 (1 to 310 backward) runs and is inside its bound, so the unaligned vector stores
are handled by the hardware.  N = 317 / 310 are accepted and N = 318 / 311 refused, as the "(N <= 317)" / "(N <= 310)" of
fp32.hip say.  aim_gemm_f32 now refuses lda < K, ldw < K, ldr < N and 0 < ldv < N, and aim_patchify_blend_f32 refuses
Kp % 4 != 0 like aim_patchify_f32 (REFUSAL_TEXT).
"""
import math
import os
import re
import sys
import time
from dataclasses import dataclass, field
from typing import Dict

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import EPS_ACT, U24, _pad_intact, _padded, ratio  # noqa: E402

F32, F64 = torch.float32, torch.float64
U = U24
TINY = 2.0 ** -126
NAN = float("nan")
C_EXP = 4.0
C_LOG = 4.0
E_ACT = EPS_ACT
E_DACT = EPS_ACT
# worst |kernel - float64| / (1 + |x|) of the K = 4 probe on MI355X (run_probe), per activation: see test_activation_constants
MEASURED_ACT = {"act_qgelu": 9.27e-8, "act_gelu": 7.98e-8, "dact_qgelu": 1.21e-7, "dact_gelu": 5.85e-8}
QGELU, GELU = 0, 1
EPI = {"lin": 0, "act": 1, "dact": 2, "f32": 3}
C1702 = float(torch.tensor(1.702, dtype=F32))

# kind -> entry point(s) of include/aim_kernels.h it runs
ENTRY = {"gemm": ("aim_gemm_f32",), "attn_fwd": ("aim_attn_fwd_f32",),
         "attn_bwd": ("aim_attn_bwd_f32", "aim_attn_bwd_f32_workspace_bytes"),
         "cls_fwd": ("aim_cls_attn_fwd_f32",), "cls_bwd": ("aim_cls_attn_bwd_f32",), "tattn_fwd": ("aim_tattn_fwd_f32",),
         "tattn_bwd": ("aim_tattn_bwd_f32",), "lambda": ("aim_lambda_f32",),
         "wgrad": ("aim_wgrad_f32", "aim_wgrad_f32_workspace_bytes"), "embed_ln": ("aim_embed_ln_f32",),
         "patchify": ("aim_patchify_f32",), "patchify_blend": ("aim_patchify_blend_f32",)}


def header_symbols():
    """the fp32 entry points include/aim_kernels.h declares"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aim_kernels.h")
    return set(re.findall(r"^(?:int|int64_t) (aim_\w*_f32\w*)\(", open(path).read(), re.M))


@dataclass
class Case:
    name: str
    kind: str
    p: dict = field(default_factory=dict)
    family: str = "unit"
    seed: int = 0


def _cdiv(a, b):
    return (a + b - 1) // b


def _gen(case):
    return torch.Generator().manual_seed(7000 + case.seed)


def _rn(g, *shape):
    return torch.randn(shape, generator=g, dtype=F32)


# ------------------------------------------------------------------ mirrors of the host-side rules -------------------------
def wgrad_f32_chunks(M: int) -> int:
    """csrc/fp32.hip::wgrad_f32_chunks"""
    c = (M + 511) // 512
    return 1 if c < 1 else (64 if c > 64 else c)


def wgrad_f32_chunk(M: int) -> int:
    c = wgrad_f32_chunks(M)
    return _cdiv(_cdiv(M, c), 16) * 16


def wgrad_f32_workspace_bytes(M, Nw, Kw) -> int:
    return wgrad_f32_chunks(M) * (Nw * Kw + Nw) * 4


def attn_bwd_f32_workspace_bytes(BT, N, H) -> int:
    return BT * H * N * 2 * 4


def attn_fwd_accepts(N: int) -> bool:
    return 0 < N <= 320 and N * 129 * 4 <= 160 * 1024


def attn_bwd_accepts(N: int) -> bool:
    return 0 < N <= 320 and N * 132 * 4 <= 160 * 1024


ATTN_FWD_MAX, ATTN_BWD_MAX = 317, 310


def split_branch(n_split: int, N: int) -> str:
    return "none" if n_split <= 0 else ("all_first" if n_split >= N else "inside")


# ------------------------------------------------------------------ gemm_f32 ----------------------------------------------
def _act64(x, act):
    if act == QGELU:
        return x * torch.sigmoid(C1702 * x)
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def _dact64(x, act):
    if act == QGELU:
        sg = torch.sigmoid(C1702 * x)
        return sg * (1.0 + C1702 * x * (1.0 - sg))
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _act32(x, act):
    """the kernel's own expressions, in fp32"""
    if act == QGELU:
        return x / (1.0 + torch.exp(-1.702 * x))
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))


def _dact32(x, act):
    if act == QGELU:
        sg = 1.0 / (1.0 + torch.exp(-1.702 * x))
        return sg * (1.0 + 1.702 * x * (1.0 - sg))
    return 0.5 * (1.0 + torch.erf(x * 0.70710678118654752)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def gemm_inputs(case):
    p, g = case.p, _gen(case)
    M, N, K, batch, fam = p["M"], p["N"], p["K"], p.get("batch", 1), case.family
    lead = (batch,) if batch > 1 else ()
    A, W = _rn(g, *lead, M, K), _rn(g, *lead, N, K)
    if fam == "offset":
        A, W = A + 50.0, W + 50.0
    elif fam == "cancel":                      # second half of k repeats the first with the sign of a flipped: sum a w ~ 0
        h = K // 2
        A[..., h:2 * h] = -A[..., :h] * (1.0 + 1e-3 * _rn(g, *lead, M, h))
        W[..., h:2 * h] = W[..., :h]
    elif fam == "bigpre":                      # small products; the bias (ACT) or aux (DACT) spreads pre over +-100
        A, W = A * 0.1, W * (0.1 / math.sqrt(K))
    inp = {"A": A, "W": W}
    ntok = p.get("ntok", 0)
    frames = _cdiv(M, ntok) if ntok else 1
    if p.get("bias"):
        inp["bias"] = _rn(g, N) * 0.5
        if fam == "bigpre":
            inp["bias"] = (torch.linspace(-100.0, 100.0, N) + _rn(g, N) * 0.01)[torch.randperm(N, generator=g)]
    if p.get("resid"):
        inp["resid"] = _rn(g, M, N)
    if p.get("af"):
        inp["af"] = 0.5 + torch.rand(frames, generator=g)
    if p.get("at"):
        inp["at"] = 0.5 + torch.rand(ntok, generator=g)
    if p.get("bt"):
        inp["bt"] = _rn(g, ntok)
    if p.get("vec"):
        inp["vec"] = _rn(g, frames if p["vec"] == "frame" else 1, N)
    if p["epi"] == "dact":
        inp["aux"] = _rn(g, M, N) * 1.5
        if fam == "bigpre":
            inp["aux"] = (torch.linspace(-100.0, 100.0, M * N) + _rn(g, M * N) * 0.01)[torch.randperm(M * N, generator=g)].view(M, N)
    return inp


def _gemm_core(p, inp, dt, mut=None):
    """every intermediate of the epilogue in `dt`: float64 is the reference, float32 the emulation"""
    M, N, K, ntok, epi = p["M"], p["N"], p["K"], p.get("ntok", 0), p["epi"]
    dev = inp["A"].device
    A, W = inp["A"].to(dt), inp["W"].to(dt)
    if mut == "bf16_operands":
        A, W = inp["A"].bfloat16().to(dt), inp["W"].bfloat16().to(dt)
    if mut == "k_tail_dropped":
        A, W = A[..., :K - K % 16], W[..., :K - K % 16]
    acc = A @ W.transpose(-1, -2)
    rows = torch.arange(M, device=dev)
    frame, tok = (rows // ntok, rows % ntok) if ntok else (rows * 0, rows * 0)
    rs = torch.ones(M, dtype=dt, device=dev)
    if "af" in inp:
        rs = rs * inp["af"].to(dt)[frame]
    if "at" in inp:
        rs = rs * inp["at"].to(dt)[(frame % ntok) if mut == "at_row_div_ntok" else tok]
    rs = rs[:, None]
    b = inp["bias"].to(dt)[None, :] if "bias" in inp else torch.zeros((1, N), dtype=dt, device=dev)
    ns, act, act2 = p.get("n_split", 0), p.get("act", QGELU), p.get("act2", QGELU)
    if mut == "split_plus_4":
        ns += 4
    if mut == "act_swapped":
        act, act2 = act2, act
    cols = torch.arange(N, device=dev)
    second = (cols >= ns)[None, :] if ns > 0 else torch.zeros((1, N), dtype=torch.bool, device=dev)
    rs_eff = rs.expand(M, N) if ns <= 0 or mut == "rs_on_frozen" else torch.where(second, rs, torch.ones_like(rs)).expand(M, N)
    c = {"acc": acc, "rs": rs, "b": b, "rs_eff": rs_eff, "second": second, "act": act, "act2": act2}
    f_act, f_dact = (_act64, _dact64) if dt == F64 else (_act32, _dact32)
    if epi == "lin":
        c["out"] = rs * (acc + b)
    elif epi == "act":
        pre = acc + b
        y = torch.where(second, f_act(pre, act2), f_act(pre, act))
        c.update(pre=pre, y=y, out=rs_eff * y)
        c["d"] = torch.where(second, _dact64(pre.double(), act2), _dact64(pre.double(), act))
    elif epi == "dact":
        aux = inp["aux"].to(dt)
        d = torch.where(second, f_dact(aux, act2), f_dact(aux, act))
        c.update(aux=aux, d=d, out=acc * d * rs_eff)
    else:
        rbo = p.get("rbo", False) and mut != "rbo_ignored"
        o = acc + rs * b if rbo else rs * (acc + b)
        c["t_lin"] = o
        if "resid" in inp:
            o = o + inp["resid"].to(dt)
        if "vec" in inp:
            v = inp["vec"].to(dt)
            btf = inp["bt"].to(dt)[tok][:, None] if "bt" in inp else 1.0
            if p["vec"] == "frame":
                vv = v[frame]
            elif mut == "vec_frame_n":        # ldv = 0 taken as N: frame f reads the memory behind row 0 (here: zeros)
                vv = torch.where((frame == 0)[:, None], v.expand(M, N), torch.zeros((), dtype=dt, device=dev))
            else:
                vv = v.expand(M, N)
            c["t_vec"] = btf * vv
            o = o + c["t_vec"]
        c["out"] = o
    return c


def gemm_expected(case, inp, got=None):
    p = case.p
    K = p["K"]
    c = _gemm_core(p, inp, F64)
    S = inp["A"].double().abs() @ inp["W"].double().abs().transpose(-1, -2)
    e_acc = (K + 2) * U * S
    acc, rs, b, out = c["acc"], c["rs"].abs(), c["b"].abs(), c["out"]
    if p["epi"] == "lin":
        bound = rs * (e_acc + U * (acc.abs() + b)) + 2 * U * out.abs()
    elif p["epi"] == "f32":
        scale = torch.maximum(rs, torch.ones_like(rs)) if p.get("rbo") else rs
        mags = rs * (acc.abs() + b) + acc.abs()
        if "resid" in inp:
            mags = mags + inp["resid"].double().abs()
        if "t_vec" in c:
            mags = mags + c["t_vec"].abs()
        bound = scale * e_acc + 5 * U * mags
    elif p["epi"] == "act":
        e_pre = e_acc + U * (acc.abs() + b)
        bound = c["rs_eff"].abs() * (E_ACT * (1 + c["pre"].abs()) + c["d"].abs() * e_pre) + 2 * U * out.abs() + TINY
        exp = {"out": (out, bound)}
        if p.get("out2"):
            exp["out2"] = (c["pre"], e_pre)
        return exp
    else:
        bound = c["rs_eff"].abs() * (acc.abs() * E_DACT * (1 + c["aux"].abs()) + c["d"].abs() * e_acc) + 3 * U * out.abs() + TINY
    return {"out": (out, bound)}


GEMM_MUTANTS = ("bf16_operands", "k_tail_dropped", "split_plus_4", "act_swapped", "rs_on_frozen", "rbo_ignored", "vec_frame_n",
                "at_row_div_ntok", "batched_item_mn")


def gemm_emulate(case, inp, mut=None):
    p = case.p
    c = _gemm_core(p, inp, F32, mut)
    got = {"out": c["out"]}
    if p.get("out2"):
        got["out2"] = c["pre"]
    if mut == "batched_item_mn":              # item z stored M N floats after item z - 1 instead of M ldo
        M, N, batch, ldo = p["M"], p["N"], p["batch"], p["N"] + 3
        buf = torch.full((batch * M * ldo + 8,), NAN)
        for z in range(batch):
            buf[z * M * N:z * M * N + M * ldo].view(M, ldo)[:, :N] = c["out"][z]
        got["out"] = torch.stack([buf[z * M * ldo:(z + 1) * M * ldo].view(M, ldo)[:, :N] for z in range(batch)])
    return got


def _gemm_args(ctx, A, W, out, M, N, K, **kw):
    """aim_gemm_args from device tensors (2-D views: their row stride is the leading dimension)"""
    from aim_amd.lib import GemmArgs
    g = GemmArgs()
    g.A, g.W, g.out = A.data_ptr(), W.data_ptr(), out.data_ptr()
    g.M, g.N, g.K = M, N, K
    for name, t in (("lda", A), ("ldw", W), ("ldo", out)):
        setattr(g, name, kw.pop(name) if name in kw else t.stride(-2))
    g.scale = 1.0
    for name in ("bias", "af", "at", "bt"):
        t = kw.pop(name, None)
        if t is not None:
            setattr(g, name, t.data_ptr())
    for name, ld in (("resid", "ldr"), ("vec", "ldv"), ("aux", "ldaux"), ("out2", "ldo2")):
        t = kw.pop(name, None)
        if t is not None:
            setattr(g, name, t.data_ptr())
            setattr(g, ld, kw.pop(ld) if ld in kw else t.stride(-2))
    for name, v in kw.items():                # ntok, act, act2, n_split, rs_bias_only, strideA, strideW and raw overrides
        setattr(g, name, v)
    return g


def _gemm_run(ctx, epi, batch, A, W, out, M, N, K, **kw):
    from ctypes import byref
    g = _gemm_args(ctx, A, W, out, M, N, K, **kw)
    return ctx.lib.aim_gemm_f32(byref(g), epi, batch, ctx.stream())


def _nan_view(t, dev, off=0, pad=0, rows_extra=3):
    """`t` [R, C] as columns [off, off + C) of an NaN-filled [R + rows_extra, off + C + pad] device buffer"""
    R, C = t.shape
    buf = torch.full((R + rows_extra, off + C + pad), NAN, dtype=F32, device=dev)
    buf[:R, off:off + C] = t.to(dev)
    return buf[:R, off:off + C]


def _bits_eq(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def gemm_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    M, N, K, batch, epi = p["M"], p["N"], p["K"], p.get("batch", 1), p["epi"]
    d = {k: v.to(dev) for k, v in inp.items()}
    if batch > 1:                             # fp32_path.py:112: q against k inside the fused qkv rows, items N 3D floats apart
        qkv = torch.full((batch, M, 3 * K), NAN, dtype=F32, device=dev)
        qkv[:, :, :K], qkv[:, :, K:2 * K] = d["A"], d["W"]
        ldo = N + 3
        buf = torch.full((batch * M * ldo + 8,), NAN, dtype=F32, device=dev)
        ctx.check(_gemm_run(ctx, 0, batch, qkv[0], qkv[0][:, K:], buf, M, N, K, ldo=ldo, strideA=M * 3 * K, strideW=M * 3 * K),
                  "aim_gemm_f32")
        torch.cuda.synchronize()
        items = buf[:batch * M * ldo].view(batch, M, ldo)
        out = items[:, :, :N].clone()
        chk = torch.cat([items[:, :, N:].reshape(-1), buf[batch * M * ldo:]])
        rec["pad"]["out"] = bool(torch.isnan(chk).all())
        rec["finite"]["out"] = bool(torch.isfinite(out).all())
        return {"out": out}

    def operands(strided):
        if not strided:
            return d["A"].contiguous(), d["W"].contiguous()
        W = _nan_view(d["W"], dev, p.get("w_off", 0), p.get("w_pad", 0))
        if p.get("w_row_off"):                # W = rows [w_row_off:] of a taller weight (Wqkv[D:]); the rows above it are NaN
            tall = torch.full((p["w_row_off"] + N + 3, K), NAN, dtype=F32, device=dev)
            tall[p["w_row_off"]:p["w_row_off"] + N] = d["W"]
            W = tall[p["w_row_off"]:p["w_row_off"] + N]
        return _nan_view(d["A"], dev, p.get("a_off", 0), p.get("a_pad", 0)), W

    def call(A, W, rows=None, n_split=None, want_out2=None):
        r0, cnt = rows if rows else (0, M)
        kw = dict(ntok=p.get("ntok", 0), act=p.get("act", 0), act2=p.get("act2", 0),
                  n_split=p.get("n_split", 0) if n_split is None else n_split, rs_bias_only=int(p.get("rbo", False)))
        for k in ("bias", "af", "at", "bt"):
            if k in d:
                kw[k] = d[k]
        if "resid" in d:
            kw["resid"] = _nan_view(d["resid"], dev, 0, 4)[r0:r0 + cnt]
        if "aux" in d:
            kw["aux"] = _nan_view(d["aux"], dev, 0, 4)[r0:r0 + cnt]
        if "vec" in d:
            kw["vec"] = _nan_view(d["vec"], dev, 0, 8, rows_extra=0)
            if p["vec"] == "row0":
                kw["ldv"] = 0
        out, obuf = _padded(cnt, N, F32, dev)
        bufs = {"out": (out, obuf)}
        if p.get("out2") if want_out2 is None else want_out2:
            o2, o2buf = _padded(cnt, N, F32, dev)
            kw["out2"] = o2
            bufs["out2"] = (o2, o2buf)
        ctx.check(_gemm_run(ctx, EPI[epi], 1, A[r0:r0 + cnt], W, out, cnt, N, K, **kw), "aim_gemm_f32")
        return bufs

    strided = any(p.get(k) for k in ("a_off", "a_pad", "w_off", "w_pad", "w_row_off"))
    A, W = operands(strided)
    bufs = call(A, W)
    torch.cuda.synchronize()
    got = {}
    for k, (v, b) in bufs.items():
        got[k] = v
        rec["pad"][k] = _pad_intact(b, M, N)
        rec["finite"][k] = bool(torch.isfinite(v).all())
    ids = p.get("ident", ())
    if "repeat" in ids:
        rec["ident"]["repeat"] = all(_bits_eq(v, got[k]) for k, (v, _) in call(A, W).items())
    if "strided_eq_dense" in ids:
        assert strided, case.name
        rec["ident"]["strided_eq_dense"] = all(_bits_eq(v, got[k]) for k, (v, _) in call(*operands(False)).items())
    if "row_alone" in ids:                    # rows [16, 16 + min(33, M - 16)) launched alone: other tile phase, same bits
        assert not p.get("ntok") and M > 16, case.name
        cnt = min(33, M - 16)
        rec["ident"]["row_alone"] = all(_bits_eq(v, got[k][16:16 + cnt]) for k, (v, _) in call(A, W, rows=(16, cnt)).items())
    if "out2_split" in ids:
        assert p.get("out2") and p.get("n_split"), case.name
        rec["ident"]["out2_split"] = _bits_eq(call(A, W, n_split=0)["out2"][0], got["out2"])
    return got


# ------------------------------------------------------------------ softmax pieces shared by the attention kinds ------------
def _softmax_ref(s, e_s, chain, extra=None):
    """p = softmax(s) over the last axis in float64, with its absolute bound e_p (and the relative r_p)"""
    mx = s.max(-1, keepdim=True).values
    z = s - mx
    ex = torch.exp(z)
    sm = ex.sum(-1, keepdim=True)
    pr = ex / sm
    r_exp = e_s + e_s.max(-1, keepdim=True).values + U * z.abs() + C_EXP * U
    r_sum = r_exp.max(-1, keepdim=True).values + chain * U
    r = r_exp + r_sum + 2 * U
    if extra is not None:
        L = mx + torch.log(sm)
        r = r + C_LOG * U + 3 * U * (s.abs() + L.abs())
    return pr, pr * torch.expm1(r) + TINY


def _softmax32(s, mut=None):
    if mut == "no_max_shift":
        ex = torch.exp(s)
    else:
        ex = torch.exp(s - s.max(-1, keepdim=True).values)
    return ex / ex.sum(-1, keepdim=True)


ATTN_FAMILIES = ("unit", "peaked", "cls_sink", "diag", "neg40", "neg100", "big", "zero_do")


def _attn_family(fam, S, N, H, g):
    """q, k, v [S, N, H, 64] (S independent sequences of N rows)"""
    q, k, v = _rn(g, S, N, H, 64), _rn(g, S, N, H, 64), _rn(g, S, N, H, 64)
    if fam == "peaked":
        q, k = q * 3.0, k * 3.0
    elif fam == "big":                        # logits of a few hundred: exp overflows without the max shift
        q, k = q * 12.0, k * 12.0
    elif fam == "cls_sink":                   # every query attends key 0
        c = _rn(g, 64)
        q = q + c
        k[:, 0] = 2.0 * c + 0.1 * k[:, 0]
    elif fam == "diag":                       # every query attends its own key
        k = 2.0 * q + 0.1 * k
    elif fam in ("neg40", "neg100"):          # every second key sits 40 / 100 below the others
        a = -40.0 if fam == "neg40" else -100.0
        c = _rn(g, 64)
        c = c / c.norm() * math.sqrt(8.0)
        lvl = torch.where(torch.arange(N) % 2 == 1, a, 0.0).view(1, N, 1, 1)
        q = c + 0.1 * q
        k = lvl * c + 0.1 * k
    return q, k, v


def _attn_core(q, k, v, dO, dt, mut=None):
    """[..., N, 64] per (sequence, head); returns every intermediate in `dt`"""
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    N = q.shape[-2]
    if mut == "last_key_dropped" and N % 64 == 1 and N > 1:
        k, v = k[..., :-1, :], v[..., :-1, :]
    s = (q @ k.transpose(-1, -2)) * 0.125
    if mut == "scale_twice":
        s = s * 0.125
    pr = _softmax32(s, mut)
    c = {"s": s, "p": pr, "out": pr @ v}
    if dO is not None:
        dO = dO.to(dt)
        dP = dO @ v.transpose(-1, -2)
        dl = (dP if mut == "del_without_p" else pr * dP).sum(-1, keepdim=True)
        dS = pr * (dP - dl) * 0.125
        c.update(dq=dS @ k, dk=dS.transpose(-1, -2) @ q, dv=(dS if mut == "dv_from_ds" else pr).transpose(-1, -2) @ dO)
        if k.shape[-2] != N:                  # (the dropped key's gradients are never written)
            z = torch.zeros_like(q[..., :1, :])
            c["dk"], c["dv"] = torch.cat([c["dk"], z], -2), torch.cat([c["dv"], z], -2)
    return c


def _attn_expected(q, k, v, dO, dot_u, chain, init=None, acc_chain=None, from_stats=True, parts=None):
    """float64 references and bounds of out (dO None) or dq / dk / dv.  `dot_u`: roundings of a 64-wide dot product;
    `chain`: of the row sums; acc_chain / init [3 x [..., N, 64]]: the backward adds into non-zero gradients; from_stats:
    dk / dv take p = exp(s - L) from the saved log-sum-exp (attn_bwd_f32 only); parts: receives an upper bound of the sum of
    the |terms| the kernel adds into a dk / dv element (the reference's plus their error bound)"""
    q, k, v = q.double(), k.double(), v.double()
    N = q.shape[-2]
    s = (q @ k.transpose(-1, -2)) * 0.125
    e_s = dot_u * U * (q.abs() @ k.abs().transpose(-1, -2)) * 0.125
    if dO is None:
        pr, e_p = _softmax_ref(s, e_s, chain)
        out = pr @ v
        return {"out": (out, e_p @ v.abs() + (N + 1) * U * (pr @ v.abs()))}
    dO = dO.double()
    pr, e_p = _softmax_ref(s, e_s, chain, extra=True if from_stats else None)
    dP = dO @ v.transpose(-1, -2)
    e_dP = dot_u * U * (dO.abs() @ v.abs().transpose(-1, -2))
    dl = (pr * dP).sum(-1, keepdim=True)
    e_dl = (e_p * dP.abs() + pr * e_dP).sum(-1, keepdim=True) + chain * U * (pr * dP.abs()).sum(-1, keepdim=True)
    dS = pr * (dP - dl) * 0.125
    e_dS = (e_p * (dP - dl).abs() + pr * (e_dP + e_dl + U * (dP.abs() + dl.abs()))) * 0.125 + 2 * U * dS.abs()
    ch = (N + 1) if acc_chain is None else acc_chain
    T_ = lambda t: t.transpose(-1, -2)        # noqa: E731
    dq, bq = dS @ k, e_dS @ k.abs() + (N + 1) * U * (dS.abs() @ k.abs())
    dk, bk = T_(dS) @ q, T_(e_dS) @ q.abs() + ch * U * (T_(dS.abs()) @ q.abs())
    dv, bv = T_(pr) @ dO, T_(e_p) @ dO.abs() + ch * U * (T_(pr) @ dO.abs())
    if parts is not None:
        parts.update(dk=T_(dS.abs() + e_dS) @ q.abs(), dv=T_(pr + e_p) @ dO.abs())
    if init is not None:
        i = [t.double() for t in init]
        dq, bq = dq + i[0], bq + U * (i[0].abs() + dq.abs())
        dk, bk = dk + i[1], bk + ch * U * i[1].abs()
        dv, bv = dv + i[2], bv + ch * U * i[2].abs()
    return {"dq": (dq, bq), "dk": (dk, bk), "dv": (dv, bv)}


# ------------------------------------------------------------------ attn_fwd_f32 / attn_bwd_f32 -----------------------------
def _heads(t):
    """[S, N, H, 64] -> [S, H, N, 64]"""
    return t.permute(0, 2, 1, 3)


def attn_inputs(case):
    p, g = case.p, _gen(case)
    BT, N, H = p["BT"], p["N"], p["H"]
    q, k, v = _attn_family(case.family, BT, N, H, g)
    inp = {"q": q, "k": k, "v": v}
    if case.kind == "attn_bwd":
        inp["dO"] = torch.zeros(BT, N, H, 64) if case.family == "zero_do" else _rn(g, BT, N, H, 64)
    return inp


def _unheads(t):
    return t.permute(0, 2, 1, 3)


def attn_expected(case, inp, got=None):
    N = case.p["N"]
    e = _attn_expected(_heads(inp["q"]), _heads(inp["k"]), _heads(inp["v"]), _heads(inp["dO"]) if "dO" in inp else None, 66,
                       _cdiv(N, 64) + 6 + 2)
    return {k: (_unheads(r), _unheads(b)) for k, (r, b) in e.items()}


ATTN_FWD_MUTANTS = ("no_max_shift", "last_key_dropped", "scale_twice")
ATTN_BWD_MUTANTS = ATTN_FWD_MUTANTS + ("del_without_p", "dv_from_ds")


def attn_emulate(case, inp, mut=None):
    c = _attn_core(_heads(inp["q"]), _heads(inp["k"]), _heads(inp["v"]), _heads(inp["dO"]) if "dO" in inp else None, F32, mut)
    keys = ("dq", "dk", "dv") if "dO" in inp else ("out",)
    return {k: _unheads(c[k]) for k in keys}


def _qkv_rows(q, k, v):
    """[S, N, H, 64] x 3 -> the fused rows [S * N, 3 D]"""
    S, N, H, _ = q.shape
    return torch.cat([q.reshape(S * N, H * 64), k.reshape(S * N, H * 64), v.reshape(S * N, H * 64)], 1).contiguous()


def _nan_tail(t, extra=64):
    """a contiguous copy of `t` inside a flat buffer with `extra` NaN floats behind it: (view, whole buffer)"""
    buf = torch.full((t.numel() + extra,), NAN, dtype=t.dtype, device=t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf[:t.numel()].view(t.shape), buf


def _tail_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _attn_call(ctx, bwd, qkv, dout, BT, N, H, rec=None):
    dev, D = ctx.dev, H * 64
    if not bwd:
        out, obuf = _nan_tail(torch.full((BT * N, D), NAN, dtype=F32, device=dev))
        ctx.check(ctx.lib.aim_attn_fwd_f32(qkv.data_ptr(), out.data_ptr(), BT, N, H, ctx.stream()), "aim_attn_fwd_f32")
        return {"out": out.view(BT, N, H, 64)}, {"out": (obuf, out.numel())}, None
    dqkv, dbuf = _nan_tail(torch.full((BT * N, 3 * D), NAN, dtype=F32, device=dev))
    need = ctx.lib.aim_attn_bwd_f32_workspace_bytes(BT, N, H)
    ws = torch.full((need // 4 + 16,), NAN, dtype=F32, device=dev)
    ctx.check(ctx.lib.aim_attn_bwd_f32(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), BT, N, H, ws.data_ptr(), need, ctx.stream()),
              "aim_attn_bwd_f32")
    got = {k: dqkv[:, i * D:(i + 1) * D].reshape(BT, N, H, 64) for i, k in enumerate(("dq", "dk", "dv"))}
    return got, {k: (dbuf, dqkv.numel()) for k in got}, (ws, need)


def attn_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    BT, N, H = p["BT"], p["N"], p["H"]
    bwd = case.kind == "attn_bwd"
    d = {k: v.to(dev) for k, v in inp.items()}
    qkv = _qkv_rows(d["q"], d["k"], d["v"])
    dout = d["dO"].reshape(BT * N, H * 64).contiguous() if bwd else None
    got, bufs, ws = _attn_call(ctx, bwd, qkv, dout, BT, N, H)
    torch.cuda.synchronize()
    for k, (b, n) in bufs.items():
        rec["pad"][k] = _tail_intact(b, n)
        rec["finite"][k] = bool(torch.isfinite(got[k]).all())
    if bwd:
        w, need = ws
        rec["evidence"]["workspace_bytes_as_mirrored"] = need == attn_bwd_f32_workspace_bytes(BT, N, H)
        rec["evidence"]["stats_exactly_finite"] = bool(torch.isfinite(w[:need // 4]).all()) and bool(torch.isnan(w[need // 4:]).all())
    ids = p.get("ident", ())
    if "repeat" in ids:
        again = _attn_call(ctx, bwd, qkv, dout, BT, N, H)[0]
        rec["ident"]["repeat"] = all(_bits_eq(again[k], got[k]) for k in got)
    if "nan_neighbours" in ids:               # item (frame 1, head 1): every other frame's rows and head's columns are NaN
        b_, h_ = 1, 1
        one = lambda t: t[b_:b_ + 1, :, h_:h_ + 1]        # noqa: E731
        alone = _attn_call(ctx, bwd, _qkv_rows(one(d["q"]), one(d["k"]), one(d["v"])),
                           one(d["dO"]).reshape(N, 64).contiguous() if bwd else None, 1, N, 1)[0]

        def mask(t):
            m = torch.full_like(t, NAN)
            m[b_, :, h_] = t[b_, :, h_]
            return m

        noisy = _attn_call(ctx, bwd, _qkv_rows(mask(d["q"]), mask(d["k"]), mask(d["v"])),
                           mask(d["dO"]).reshape(BT * N, H * 64).contiguous() if bwd else None, BT, N, H)[0]
        torch.cuda.synchronize()
        rec["ident"]["nan_neighbours"] = all(bool(torch.isfinite(noisy[k][b_, :, h_]).all()) and
                                             _bits_eq(noisy[k][b_, :, h_], alone[k][0, :, 0]) and
                                             _bits_eq(noisy[k][b_, :, h_], got[k][b_, :, h_]) for k in got)
    return got


# ------------------------------------------------------------------ cls_attn / tattn (sequences of T rows) ------------------
SEQ_FAMILIES = ("unit", "peaked", "big")


def seq_inputs(case):
    """q, k, v, dO [S, T, H, 64]: S = B sequences (cls) or B * N (tattn, sequence b * N + n); dqkv0: the gradient rows' start"""
    p, g = case.p, _gen(case)
    S = p["B"] if case.kind.startswith("cls") else p["B"] * p["N"]
    q, k, v = _attn_family(case.family, S, p["T"], p["H"], g)
    inp = {"q": q, "k": k, "v": v}
    if case.kind.endswith("bwd"):
        inp["dO"] = _rn(g, S, p["T"], p["H"], 64)
        inp["init"] = torch.stack([_rn(g, S, p["T"], p["H"], 64) for _ in range(3)])
    return inp


def seq_expected(case, inp, got=None, parts=None):
    T = case.p["T"]
    bwd = "dO" in inp
    init = [_heads(inp["init"][i]) for i in range(3)] if bwd else None
    e = _attn_expected(_heads(inp["q"]), _heads(inp["k"]), _heads(inp["v"]), _heads(inp["dO"]) if bwd else None, 8, T + 2,
                       init=init, acc_chain=T + 2, from_stats=False, parts=parts)
    if parts is not None:
        parts.update({k: _unheads(v) for k, v in parts.items()})
    return {k: (_unheads(r), _unheads(b)) for k, (r, b) in e.items()}


SEQ_FWD_MUTANTS = ("no_max_shift", "scale_twice")
SEQ_BWD_MUTANTS = ("assign",)


def seq_emulate(case, inp, mut=None):
    bwd = "dO" in inp
    c = _attn_core(_heads(inp["q"]), _heads(inp["k"]), _heads(inp["v"]), _heads(inp["dO"]) if bwd else None, F32,
                   None if bwd else mut)
    if not bwd:
        return {"out": _unheads(c["out"])}
    return {k: _unheads(c[k]) + (0 if mut == "assign" else inp["init"][i]) for i, k in enumerate(("dq", "dk", "dv"))}


def _seq_place(case, dev, q, k, v, fill=NAN):
    """the fused rows the entry point reads, [B, T, N, 3D]; cls: only row 0 of every frame holds values, the rest is `fill`"""
    p = case.p
    B, T, N, H = p["B"], p["T"], p["N"], p["H"]
    D = H * 64
    rows = torch.cat([q.reshape(-1, T, D), k.reshape(-1, T, D), v.reshape(-1, T, D)], -1).to(dev)      # [S, T, 3D]
    if case.kind.startswith("cls"):
        buf = torch.full((B, T, N, 3 * D), fill, dtype=F32, device=dev)
        buf[:, :, 0] = rows
    else:
        buf = rows.view(B, N, T, 3 * D).permute(0, 2, 1, 3).contiguous()
    return buf


def _seq_take(case, buf, width):
    """the sequences' rows of a [B, T, N, width] buffer: [S, T, width]"""
    p = case.p
    if case.kind.startswith("cls"):
        return buf[:, :, 0]
    return buf.permute(0, 2, 1, 3).reshape(p["B"] * p["N"], p["T"], width)


def seq_launch(ctx, case, inp, rec):
    p, dev, lib = case.p, ctx.dev, ctx.lib
    B, T, N, H = p["B"], p["T"], p["N"], p["H"]
    D, cls, bwd = H * 64, case.kind.startswith("cls"), case.kind.endswith("bwd")
    S = B if cls else B * N
    qkv = _seq_place(case, dev, inp["q"], inp["k"], inp["v"])
    split = lambda t, w: {k: t[..., i * w:(i + 1) * w].reshape(S, T, H, 64) for i, k in enumerate(("dq", "dk", "dv"))}  # noqa: E731
    if not bwd:
        out, obuf = _nan_tail(torch.full((B * T, D) if cls else (B * T * N, D), NAN, dtype=F32, device=dev))
        if cls:
            ctx.check(lib.aim_cls_attn_fwd_f32(qkv.data_ptr(), N * 3 * D, out.data_ptr(), B, T, H, ctx.stream()), "aim_cls_attn_fwd_f32")
            got = {"out": out.view(B, T, H, 64)}
        else:
            ctx.check(lib.aim_tattn_fwd_f32(qkv.data_ptr(), out.data_ptr(), B, T, N, H, ctx.stream()), "aim_tattn_fwd_f32")
            got = {"out": _seq_take(case, out.view(B, T, N, D), D).reshape(S, T, H, 64)}
        torch.cuda.synchronize()
        rec["pad"]["out"], rec["finite"]["out"] = _tail_intact(obuf, out.numel()), bool(torch.isfinite(out).all())
        return got
    i = inp["init"]
    dO = inp["dO"].to(dev)
    dout = (dO.reshape(B * T, D) if cls else dO.reshape(B, N, T, D).permute(0, 2, 1, 3).reshape(B * T * N, D)).contiguous()

    def call(base):
        """base: the start of the sequences' rows [3, S, T, H, 64]; every other row of dqkv starts from random values"""
        start = _seq_place(case, dev, base[0], base[1], base[2], fill=0.0)
        if cls:
            start[:, :, 1:].uniform_(-1.0, 1.0)
        dq, dbuf = _nan_tail(start)
        before = dq.clone()
        if cls:
            ctx.check(lib.aim_cls_attn_bwd_f32(qkv.data_ptr(), N * 3 * D, dout.data_ptr(), dq.data_ptr(), B, T, H, ctx.stream()),
                      "aim_cls_attn_bwd_f32")
        else:
            ctx.check(lib.aim_tattn_bwd_f32(qkv.data_ptr(), dout.data_ptr(), dq.data_ptr(), B, T, N, H, ctx.stream()), "aim_tattn_bwd_f32")
        torch.cuda.synchronize()
        return dq, dbuf, before

    dq, dbuf, before = call(i)
    got = split(_seq_take(case, dq, 3 * D), D)
    for k in got:
        rec["pad"][k], rec["finite"][k] = _tail_intact(dbuf, dq.numel()), bool(torch.isfinite(got[k]).all())
    if cls:
        rec["ident"]["other_rows_kept"] = _bits_eq(dq[:, :, 1:], before[:, :, 1:])
    if "base_plus_zero" in p.get("ident", ()):
        # the same call on zeroed rows: every term is the same fp32 number in both calls, only the additions differ.  dq is
        # added once: |base call - (zero call + base)| <= u |base call|.  A dk / dv element takes T additions in either call,
        # each off by u of a partial sum that is at most |base| + sum |terms|: 2 T u (|base| + sum |terms|)
        zero = split(_seq_take(case, call(torch.zeros_like(i))[0], 3 * D), D)
        parts = {}
        seq_expected(case, {k: v.to(dev) for k, v in inp.items()}, parts=parts)
        ok = True
        for j, k in enumerate(("dq", "dk", "dv")):
            base = i[j].to(dev).double()
            diff = (got[k].double() - (zero[k].double() + base)).abs()
            tol = U * got[k].double().abs() if k == "dq" else 2 * T * U * (base.abs() + parts[k])
            ok = ok and bool((diff <= tol).all())
        rec["ident"]["base_plus_zero"] = ok
    return got


# ------------------------------------------------------------------ lambda_f32 ----------------------------------------------
LAMBDA_FAMILIES = ("unit", "cw_dominant", "ow_dominant", "huge")


def lambda_inputs(case):
    p, g = case.p, _gen(case)
    BT, N, D, fam = p["BT"], p["N"], p["D"], case.family
    scale = 0.125
    S = _rn(g, BT, N, N) * 8.0                               # scale s ~ N(0, 1)
    c = _rn(g, D)
    q = _rn(g, BT, N, D) * 0.1 + c
    kx = _rn(g, BT, D) / math.sqrt(D)                        # unit: ss = scale q . kx is O(1)
    n2 = float((c * c).sum())
    if fam == "cw_dominant":                                 # ss ~ +30: lam -> 1
        kx = kx + c * (30.0 / (scale * n2))
    elif fam == "ow_dominant":                               # lam ~ 1e-6
        kx = kx + c * (math.log(1e-6 * N) / (scale * n2))
    elif fam == "huge":                                      # scale s and ss spread over +-200
        S = (torch.rand((BT, N, N), generator=g) * 400.0 - 200.0) / scale
        kx = kx + c * (150.0 / (scale * n2)) * torch.where(torch.arange(BT) % 2 == 0, 1.0, -1.0)[:, None]
    return {"S": S, "q": q, "kx": kx, "scale": scale}


def _lambda_core(inp, dt, mut=None):
    S, q, kx, scale = inp["S"].to(dt), inp["q"].to(dt), inp["kx"].to(dt), inp["scale"]
    BT = S.shape[0]
    ss = (q * kx[:, None, :]).sum(-1) * scale                # [BT, N]
    a = S * scale
    m_ow, m_cw = a.reshape(BT, -1).max(1).values, ss.max(1).values
    mx = torch.maximum(m_ow, m_cw)
    if mut == "separate_shifts":
        ow, cw = torch.exp(a - m_ow[:, None, None]).sum((1, 2)), torch.exp(ss - m_cw[:, None]).sum(1)
    else:
        ow, cw = torch.exp(a - mx[:, None, None]).sum((1, 2)), torch.exp(ss - mx[:, None]).sum(1)
    if mut == "cw_ow_swapped":
        ow, cw = cw, ow
    lam = cw / (cw + ow)
    return {"ss": ss, "a": a, "mx": mx, "lam": lam, "one_minus": 1.0 - lam}


def lambda_expected(case, inp, got=None):
    p = case.p
    N, D = p["N"], p["D"]
    c = _lambda_core(inp, F64)
    BT = c["a"].shape[0]
    e_ss = (_cdiv(D, 64) + 7) * U * abs(inp["scale"]) * (inp["q"].double().abs() * inp["kx"].double().abs()[:, None, :]).sum(-1)
    mx = c["mx"]
    r_ow = (U * c["a"].abs() + U * (c["a"] - mx[:, None, None]).abs()).reshape(BT, -1).max(1).values + (C_EXP + _cdiv(N * N, 256) + 9) * U
    r_cw = (e_ss + U * (c["ss"] - mx[:, None]).abs()).max(1).values + (C_EXP + _cdiv(N, 256) + 9) * U
    e_lam = c["lam"] * (torch.expm1(r_ow + r_cw + 2 * U) + N * N * TINY) + TINY
    exp = {"lam": (c["lam"], e_lam)}
    if p.get("one_minus", True):
        exp["one_minus"] = (c["one_minus"], U + e_lam)
    return exp


LAMBDA_MUTANTS = ("separate_shifts", "lds_as_n", "cw_ow_swapped")


def lambda_emulate(case, inp, mut=None):
    p = case.p
    if mut == "lds_as_n" and p["lds"] > p["N"]:              # rows read N apart from a buffer whose rows are lds apart
        N, lds = p["N"], p["lds"]
        buf = torch.full((p["BT"], N, lds), NAN)
        buf[:, :, :N] = inp["S"]
        inp = dict(inp, S=buf.reshape(p["BT"], -1)[:, :N * N].reshape(p["BT"], N, N))
    c = _lambda_core(inp, F32, mut)
    return {k: c[k] for k in (("lam", "one_minus") if p.get("one_minus", True) else ("lam",))}


def lambda_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    BT, N, D, lds, ldkx = p["BT"], p["N"], p["D"], p["lds"], p["ldkx"]
    S = torch.full((BT, N, lds), NAN, dtype=F32, device=dev)
    S[:, :, :N] = inp["S"].to(dev)
    qkv = torch.full((BT * N, 3 * D), NAN, dtype=F32, device=dev)     # only q is read
    qkv[:, :D] = inp["q"].to(dev).reshape(BT * N, D)
    kx = torch.full((BT, ldkx), NAN, dtype=F32, device=dev)
    kx[:, :D] = inp["kx"].to(dev)
    lam, lbuf = _nan_tail(torch.full((BT,), NAN, dtype=F32, device=dev), 8)
    got, bufs = {"lam": lam}, {"lam": lbuf}
    om = None
    if p.get("one_minus", True):
        om, obuf = _nan_tail(torch.full((BT,), NAN, dtype=F32, device=dev), 8)
        got["one_minus"], bufs["one_minus"] = om, obuf
    ctx.check(ctx.lib.aim_lambda_f32(S.data_ptr(), lds, qkv.data_ptr(), kx.data_ptr(), ldkx, lam.data_ptr(),
                                     om.data_ptr() if om is not None else None, BT, N, D, inp["scale"], ctx.stream()), "aim_lambda_f32")
    torch.cuda.synchronize()
    for k in got:
        rec["pad"][k], rec["finite"][k] = _tail_intact(bufs[k], BT), bool(torch.isfinite(got[k]).all())
    return got


# ------------------------------------------------------------------ wgrad_f32 -----------------------------------------------
def wgrad_inputs(case):
    p, g = case.p, _gen(case)
    M, Nw, Kw = p["M"], p["Nw"], p["Kw"]
    inp = {"G": _rn(g, M, Nw), "A": _rn(g, M, Kw), "dW0": _rn(g, Nw, Kw)}
    if p.get("db"):
        inp["db0"] = _rn(g, Nw)
    if p.get("ntok"):
        inp["at"] = 0.5 + torch.rand(p["ntok"], generator=g)
    return inp


def _wgrad_core(p, inp, dt, mut=None):
    M = p["M"]
    G, A = inp["G"].to(dt), inp["A"].to(dt)
    rows = torch.arange(M, device=G.device)
    keep = torch.ones(M, dtype=torch.bool, device=G.device)
    if mut == "tail_rows_dropped":
        keep = rows < M - M % 16
    if mut == "last_chunk_dropped":
        keep = rows < (wgrad_f32_chunks(M) - 1) * wgrad_f32_chunk(M)
    Gk = G * keep[:, None].to(dt)
    out = {"dW": Gk.t() @ A + (0 if mut == "assign" else inp["dW0"].to(dt))}
    if "db0" in inp:
        w = torch.ones(M, dtype=dt, device=G.device)
        if "at" in inp:
            nt = p["ntok"]
            w = inp["at"].to(dt)[((rows // nt) % nt) if mut == "at_row_div_ntok" else rows % nt]
        out["db"] = (Gk * w[:, None]).sum(0) + (0 if mut == "assign" else inp["db0"].to(dt))
        out["w"] = w
    return out


def wgrad_expected(case, inp, got=None):
    p = case.p
    c = _wgrad_core(p, inp, F64)
    chain = wgrad_f32_chunk(p["M"]) + wgrad_f32_chunks(p["M"]) + 1
    G, A = inp["G"].double().abs(), inp["A"].double().abs()
    exp = {"dW": (c["dW"], chain * U * (inp["dW0"].double().abs() + G.t() @ A))}
    if "db0" in inp:
        exp["db"] = (c["db"], (chain + 1) * U * (inp["db0"].double().abs() + (G * c["w"].abs()[:, None]).sum(0)))
    return exp


WGRAD_MUTANTS = ("tail_rows_dropped", "assign", "at_row_div_ntok", "last_chunk_dropped")


def wgrad_emulate(case, inp, mut=None):
    c = _wgrad_core(case.p, inp, F32, mut)
    return {k: c[k] for k in ("dW", "db") if k in c}


def wgrad_launch(ctx, case, inp, rec):
    p, dev, lib = case.p, ctx.dev, ctx.lib
    M, Nw, Kw = p["M"], p["Nw"], p["Kw"]
    G = _nan_view(inp["G"], dev, 0, p.get("g_pad", 0))
    A = _nan_view(inp["A"], dev, 0, p.get("a_pad", 0))
    at = inp["at"].to(dev) if "at" in inp else None
    need = lib.aim_wgrad_f32_workspace_bytes(M, Nw, Kw)
    chunks, chunk, numel = wgrad_f32_chunks(M), wgrad_f32_chunk(M), Nw * Kw

    def call():
        dW, wbuf = _nan_tail(inp["dW0"].to(dev))
        db, bbuf = _nan_tail(inp["db0"].to(dev)) if "db0" in inp else (None, None)
        ws = torch.full((need // 4 + 16,), NAN, dtype=F32, device=dev)
        ctx.check(lib.aim_wgrad_f32(G.data_ptr(), G.stride(0), A.data_ptr(), A.stride(0), dW.data_ptr(), M, Nw, Kw,
                                    db.data_ptr() if db is not None else None, at.data_ptr() if at is not None else None,
                                    p.get("ntok", 0), ws.data_ptr(), need, ctx.stream()), "aim_wgrad_f32")
        torch.cuda.synchronize()
        got, bufs = {"dW": dW}, {"dW": (wbuf, numel)}
        if db is not None:
            got["db"], bufs["db"] = db, (bbuf, Nw)
        return got, bufs, ws

    got, bufs, ws = call()
    for k, (b, n) in bufs.items():
        rec["pad"][k], rec["finite"][k] = _tail_intact(b, n), bool(torch.isfinite(got[k]).all())
    used = chunks * numel + (chunks * Nw if "db0" in inp else 0)
    ev = rec["evidence"]
    ev["workspace_bytes_as_mirrored"] = need == wgrad_f32_workspace_bytes(M, Nw, Kw)
    ev["partials_exactly_finite"] = bool(torch.isfinite(ws[:used]).all()) and bool(torch.isnan(ws[used:]).all())
    part = ws[:chunks * numel].view(chunks, Nw, Kw)
    # the partial of chunk z is G[rows of z]^T A[rows of z] (so `chunk` is what the mirror says), an empty chunk holds zeros
    ok = True
    for z in sorted({0, chunks - 1}):
        lo, hi = z * chunk, min(M, (z + 1) * chunk)
        if hi <= lo:
            ok = ok and bool((part[z] == 0).all())
            ev["empty_chunk_is_zero"] = bool((part[z] == 0).all())
        else:
            g64, a64 = inp["G"][lo:hi].to(dev).double(), inp["A"][lo:hi].to(dev).double()
            ok = ok and ratio(part[z], g64.t() @ a64, (chunk + 1) * U * (g64.abs().t() @ a64.abs())) <= 1.0
    ev["partials_are_the_chunks"] = ok
    if "repeat" in p.get("ident", ()):
        again = call()[0]
        rec["ident"]["repeat"] = all(_bits_eq(again[k], got[k]) for k in got)
    return got


# ------------------------------------------------------------------ embed_ln_f32 --------------------------------------------
EMBED_FAMILIES = ("unit", "offset", "scaled", "const")


def embed_inputs(case):
    p, g = case.p, _gen(case)
    B, T, N, D, fam = p["B"], p["T"], p["N"], p["D"], case.family
    tok, cls = _rn(g, B * T * (N - 1), D), _rn(g, D)
    pos, tmp = _rn(g, N, D) * 0.3, _rn(g, T, D) * 0.3
    if fam == "offset":
        tok, cls = tok + 300.0, cls + 300.0
    elif fam == "scaled":                     # row scales from 1e-3 to 1e3
        sc = torch.logspace(-3, 3, N)
        pos, tmp = pos * sc[:, None], tmp * 0.0
        tok = (tok.view(B * T, N - 1, D) * sc[None, 1:, None]).reshape(-1, D)
        cls = cls * sc[0]
    elif fam == "const":                      # every row one constant: var = 0
        tok = torch.ones_like(tok) * _rn(g, B * T * (N - 1), 1)
        cls, pos, tmp = torch.ones(D) * 0.7, torch.ones(N, D) * _rn(g, N, 1), torch.ones(T, D) * _rn(g, T, 1)
    return {"tok": tok, "cls": cls, "pos": pos, "tmp": tmp, "gamma": 1.0 + 0.2 * _rn(g, D), "beta": 0.2 * _rn(g, D)}


def _embed_value(p, inp, mut=None):
    """ln_pre's input rows [B*T, N, D] in fp32, as the kernel adds them: (src + pos) + tmp"""
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    tok = inp["tok"].view(B * T, N - 1, D)
    first = tok[:, :1] if mut == "class_row_from_tok" else inp["cls"].view(1, 1, D).expand(B * T, 1, D)
    src = torch.cat([first, tok], 1)
    t = torch.arange(B * T, device=tok.device) % T
    return (src + inp["pos"][None]) + inp["tmp"][t][:, None, :]


def embed_expected(case, inp, got=None):
    p = case.p
    D, eps = p["D"], p["eps"]
    v32 = _embed_value(p, inp).reshape(-1, D)
    v = v32.double()
    G, Bt = inp["gamma"].double(), inp["beta"].double()
    mu = v.mean(1, keepdim=True)
    d = v - mu
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    L = _cdiv(D, 64) + 6 + 1
    e_mu = L * U * v.abs().mean(1, keepdim=True)
    e_d = e_mu + U * d.abs()
    e_var = e_mu ** 2 + 2 * (d.abs() * e_d).mean(1, keepdim=True) + (L + 4) * U * var
    r_rs = e_var / (2 * (var + eps)) + 4 * U
    x = d * rstd * G + Bt
    bx = G.abs() * rstd * e_d + (G * d * rstd).abs() * (r_rs + 3 * U) + U * (x.abs() + Bt.abs())
    exp = {"x": (x, bx)}
    if p.get("stats"):
        exp.update(pre=(v, torch.zeros_like(v)), mean=(mu[:, 0], e_mu[:, 0]), rstd=(rstd[:, 0], (rstd * r_rs)[:, 0]))
    return exp


EMBED_MUTANTS = ("eps_outside", "class_row_from_tok")


def embed_emulate(case, inp, mut=None):
    p = case.p
    D, eps = p["D"], p["eps"]
    v = _embed_value(p, inp, mut).reshape(-1, D)
    mu = v.mean(1, keepdim=True)
    d = v - mu
    var = (d * d).mean(1, keepdim=True)
    rs = 1.0 / (torch.sqrt(var) + eps) if mut == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    got = {"x": d * rs * inp["gamma"] + inp["beta"]}
    if p.get("stats"):
        got.update(pre=v, mean=mu[:, 0], rstd=rs[:, 0])
    return got


def embed_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    R = B * T * N
    d = {k: v.to(dev).contiguous() for k, v in inp.items()}
    got, bufs = {}, {}
    for k, shape in (("x", (R, D)),) + ((("pre", (R, D)), ("mean", (R,)), ("rstd", (R,))) if p.get("stats") else ()):
        got[k], bufs[k] = _nan_tail(torch.full(shape, NAN, dtype=F32, device=dev))
    ptr = lambda k: got[k].data_ptr() if k in got else None      # noqa: E731
    ctx.check(ctx.lib.aim_embed_ln_f32(d["tok"].data_ptr(), d["cls"].data_ptr(), d["pos"].data_ptr(), d["tmp"].data_ptr(),
                                       d["gamma"].data_ptr(), d["beta"].data_ptr(), ptr("x"), ptr("pre"), ptr("mean"), ptr("rstd"),
                                       B, T, N, D, p["eps"], ctx.stream()), "aim_embed_ln_f32")
    torch.cuda.synchronize()
    for k in got:
        rec["pad"][k], rec["finite"][k] = _tail_intact(bufs[k], got[k].numel()), bool(torch.isfinite(got[k]).all())
    return got


# ------------------------------------------------------------------ patchify_f32 / patchify_blend_f32 -----------------------
def patchify_inputs(case):
    p, g = case.p, _gen(case)
    B, T, H, W = p["B"], p["T"], p["H"], p["W"]
    if p["dtype"] == "u8":
        img = torch.randint(0, 256, (B, 3, T, H, W), generator=g, dtype=torch.uint8)
    else:
        img = _rn(g, B, 3, T, H, W)
    inp = {"img": img}
    if p.get("norm"):
        inp["mean"], inp["std"] = torch.tensor([123.675, 116.28, 103.53]), torch.tensor([58.395, 57.12, 57.375])
    if case.kind == "patchify_blend":
        inp["partner"] = torch.tensor(p["partner"], dtype=torch.int32)
    return inp


def _patch_index(p, dev, mut=None):
    """(channel, y, x, frame t, clip b) of every element [rows, 3 p p] of the patch matrix"""
    B, T, H, W, pp = p["B"], p["T"], p["H"], p["W"], p["p"]
    G, Gy, K = W // pp, H // pp, 3 * pp * pp
    row, k = torch.arange(B * T * Gy * G, device=dev)[:, None], torch.arange(K, device=dev)[None, :]
    gx, gy, bt = row % G, (row // G) % Gy, row // (G * Gy)
    t, b = bt % T, bt // T
    c = (k // pp) % 3 if mut == "channel_stride_p" else k // (pp * pp)
    rem = k % (pp * pp)
    return c, gy * pp + rem // pp, gx * pp + rem % pp, t, b


def _patchify_core(case, inp, mut=None):
    """torch's fp32 evaluation of the same operations"""
    p = case.p
    img = inp["img"]
    c, y, x, t, b = _patch_index(p, img.device, mut)

    def take(bb):
        v = img[bb, c, t, y, x].to(F32)
        if "mean" in inp:
            v = (v - inp["mean"][c]) / inp["std"][c]
        return v

    if case.kind == "patchify":
        v = take(b)
    else:
        pb = inp["partner"].long()[b]
        if p["mode"] == 1:
            lam, oml = torch.tensor(p["lam"], dtype=F32), torch.tensor(p["oml"], dtype=F32)
            v = (lam.to(img.device) * take(b)) + (oml.to(img.device) * take(pb))
        else:
            x1, y1, x2, y2 = p["box"]
            inside = (x >= y1) & (x < y2) & (y >= x1) & (y < x2) if mut == "box_axes_swapped" else \
                (y >= y1) & (y < y2) & (x >= x1) & (x < x2)
            v = take(torch.where(inside, pb, b))
    out = torch.zeros((v.shape[0], p["Kp"]), dtype=F32, device=img.device)
    out[:, :v.shape[1]] = v
    return out


def patchify_expected(case, inp, got=None):
    ref = _patchify_core(case, inp).double()
    return {"A": (ref, torch.zeros_like(ref))}


PATCHIFY_MUTANTS = ("channel_stride_p",)
BLEND_MUTANTS = ("channel_stride_p", "box_axes_swapped")


def patchify_emulate(case, inp, mut=None):
    return {"A": _patchify_core(case, inp, mut)}


def _patchify_rc(ctx, case_kind, p, img, mean, std, A, partner=None, **over):
    lib = ctx.lib
    a = dict(B=p["B"], T=p["T"], H=p["H"], W=p["W"], p=p["p"], Kp=p["Kp"], in_dtype=1 if p["dtype"] == "u8" else 0)
    a.update(over)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    if case_kind == "patchify":
        return lib.aim_patchify_f32(img.data_ptr(), a["in_dtype"], ptr(mean), ptr(std), A.data_ptr(), a["B"], a["T"], a["H"], a["W"],
                                    a["p"], a["Kp"], ctx.stream())
    x1, y1, x2, y2 = p.get("box", (0, 0, 0, 0))
    return lib.aim_patchify_blend_f32(img.data_ptr(), a["in_dtype"], ptr(mean), ptr(std), A.data_ptr(), a["B"], a["T"], a["H"],
                                      a["W"], a["p"], a["Kp"], ptr(partner), p["mode"], p.get("lam", 1.0), p.get("oml", 0.0),
                                      x1, y1, x2, y2, ctx.stream())


def patchify_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    d = {k: v.to(dev).contiguous() for k, v in inp.items()}
    rows = p["B"] * p["T"] * (p["H"] // p["p"]) * (p["W"] // p["p"])
    A, abuf = _nan_tail(torch.full((rows, p["Kp"]), NAN, dtype=F32, device=dev))
    ctx.check(_patchify_rc(ctx, case.kind, p, d["img"], d.get("mean"), d.get("std"), A, d.get("partner")), "aim_" + case.kind + "_f32")
    torch.cuda.synchronize()
    rec["pad"]["A"], rec["finite"]["A"] = _tail_intact(abuf, A.numel()), bool(torch.isfinite(A).all())
    if case.kind == "patchify_blend" and p.get("plain_twin"):       # identity partner / empty box / lam = 1: aim_patchify_f32's bits
        B_, bbuf = _nan_tail(torch.full((rows, p["Kp"]), NAN, dtype=F32, device=dev))
        ctx.check(_patchify_rc(ctx, "patchify", p, d["img"], d.get("mean"), d.get("std"), B_), "aim_patchify_f32")
        torch.cuda.synchronize()
        rec["ident"]["blend_noop_eq_patchify"] = _bits_eq(A, B_)
    return {"A": A}


# kind -> (inputs, expected, emulate, launch, mutants)
KINDS = {
    "gemm": (gemm_inputs, gemm_expected, gemm_emulate, gemm_launch, GEMM_MUTANTS),
    "attn_fwd": (attn_inputs, attn_expected, attn_emulate, attn_launch, ATTN_FWD_MUTANTS),
    "attn_bwd": (attn_inputs, attn_expected, attn_emulate, attn_launch, ATTN_BWD_MUTANTS),
    "cls_fwd": (seq_inputs, seq_expected, seq_emulate, seq_launch, SEQ_FWD_MUTANTS),
    "cls_bwd": (seq_inputs, seq_expected, seq_emulate, seq_launch, SEQ_BWD_MUTANTS),
    "tattn_fwd": (seq_inputs, seq_expected, seq_emulate, seq_launch, SEQ_FWD_MUTANTS),
    "tattn_bwd": (seq_inputs, seq_expected, seq_emulate, seq_launch, SEQ_BWD_MUTANTS),
    "lambda": (lambda_inputs, lambda_expected, lambda_emulate, lambda_launch, LAMBDA_MUTANTS),
    "wgrad": (wgrad_inputs, wgrad_expected, wgrad_emulate, wgrad_launch, WGRAD_MUTANTS),
    "embed_ln": (embed_inputs, embed_expected, embed_emulate, embed_launch, EMBED_MUTANTS),
    "patchify": (patchify_inputs, patchify_expected, patchify_emulate, patchify_launch, PATCHIFY_MUTANTS),
    "patchify_blend": (patchify_inputs, patchify_expected, patchify_emulate, patchify_launch, BLEND_MUTANTS),
}

# ------------------------------------------------------------------ the case table ------------------------------------------
GEMM_MN = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 197, 257)
GEMM_K = (4, 8, 12, 16, 20, 28, 36, 64, 588, 768)
GEMM_FAMILIES = ("unit", "offset", "cancel", "bigpre")
NTOKS = (5, 7, 197)
LAMBDA_N = (1, 5, 63, 64, 65, 197, 255, 256, 257, 317)
LAMBDA_D = (64, 100, 768, 1024)
WGRAD_M = (1, 15, 16, 17, 511, 512, 513, 1025, 32769, 40000)
WGRAD_NK = (1, 3, 52, 63, 64, 65, 100, 192)
PATCH_SHAPES = ((16, 32, 32), (14, 28, 42), (2, 4, 6))
EMBED_SHAPES = ((1, 1, 2, 64), (2, 3, 5, 128), (1, 2, 197, 768), (1, 1, 5, 100))
TATTN_SHAPES = ((1, 1, 3, 1), (2, 8, 5, 2), (1, 32, 7, 2), (2, 4, 197, 12))


def _gemm_cases(add):
    K_cycle = list(GEMM_K)
    i = 0
    # every M and N value against a small (20) and a large (129) partner; K, strides, offsets and families cycle through
    for v in GEMM_MN:
        for other in (20, 129):
            for M, N in ((v, other), (other, v)):
                K = K_cycle[i % len(K_cycle)]
                fam = GEMM_FAMILIES[i % 3]                                  # (bigpre goes with ACT / DACT below)
                p = dict(epi="lin", M=M, N=N, K=K, bias=i % 2 == 0, a_pad=4 * (i % 3), w_pad=4 * ((i + 1) % 3),
                         a_off=K if i % 4 == 1 else 0, w_off=K if i % 4 == 2 else 0)
                ids = ["repeat"] if i % 6 == 0 else []
                if any(p[k] for k in ("a_pad", "w_pad", "a_off", "w_off")) and i % 3 == 0:
                    ids.append("strided_eq_dense")
                if M > 17 and i % 5 == 0:
                    ids.append("row_alone")
                add(f"gemm/lin/M{M}N{N}K{K}/{fam}/{i}", "gemm", dict(p, ident=tuple(ids)), fam)
                i += 1
    # every K at one odd shape, every family
    for K in GEMM_K:
        for fam in ("unit", "offset", "cancel"):
            if fam == "cancel" and K < 8:
                continue
            add(f"gemm/lin/M65N17K{K}/{fam}", "gemm", dict(epi="lin", M=65, N=17, K=K, bias=True, a_pad=4, w_pad=8,
                                                          ident=("strided_eq_dense", "row_alone")), fam)
    # linear: bias or none x af / at / both, frames crossing the 16-row groups
    for ntok in NTOKS:
        for bias in (False, True):
            for af, at in ((True, False), (False, True), (True, True)):
                M = ntok * (3 if ntok < 100 else 1) if not (af and at) else ntok * (7 if ntok < 100 else 2)
                add(f"gemm/lin/ntok{ntok}/b{int(bias)}af{int(af)}at{int(at)}", "gemm",
                    dict(epi="lin", M=M, N=36, K=20, ntok=ntok, bias=bias, af=af, at=at), "unit")
    # F32: resid, vec (ldv > N | ldv = 0), bt, rs_bias_only
    n = 0
    for resid in (False, True):
        for vec in ("", "frame", "row0"):
            for bt in ((False, True) if vec else (False,)):
                for rbo in (False, True):
                    ntok = NTOKS[n % 3]
                    M = ntok * (4 if ntok < 100 else 2)
                    add(f"gemm/f32/r{int(resid)}v{vec or 'none'}bt{int(bt)}rbo{int(rbo)}/ntok{ntok}", "gemm",
                        dict(epi="f32", M=M, N=(33, 65, 130)[n % 3], K=(36, 64, 12)[n % 3], ntok=ntok, bias=True, resid=resid, vec=vec,
                             bt=bt, rbo=rbo, af=n % 2 == 0, at=n % 2 == 1 or rbo, a_pad=4 * (n % 2),
                             ident=("repeat",) if n % 4 == 0 else ()), ("unit", "offset", "cancel")[n % 3])
                    n += 1
    # ACT: both activations, n_split 0 / 4 / 36 / N - 4 / N, out2 given or NULL; DACT: both activations, split, at and af
    N = 68
    for a1, a2 in ((QGELU, GELU), (GELU, QGELU)):
        for ns in (0, 4, 36, N - 4, N):
            for out2 in (False, True):
                for fam in ("unit", "bigpre"):
                    add(f"gemm/act/a{a1}{a2}/split{ns}/out2_{int(out2)}/{fam}", "gemm",
                        dict(epi="act", M=35, N=N, K=28, ntok=7, bias=True, at=True, af=ns == 36, act=a1, act2=a2, n_split=ns, out2=out2,
                             ident=("out2_split",) if out2 and ns == 36 else ()), fam)
        for ns in (0, 36, N):
            for rows in ("at", "af", "both"):
                for fam in ("unit", "bigpre"):
                    add(f"gemm/dact/a{a1}{a2}/split{ns}/{rows}/{fam}", "gemm",
                        dict(epi="dact", M=35, N=N, K=28, ntok=5, at=rows != "af", af=rows != "at", act=a1, act2=a2, n_split=ns), fam)
    add("gemm/act/plain/M130N129", "gemm", dict(epi="act", M=130, N=129, K=64, bias=True, act=GELU, out2=True, ident=("repeat", "row_alone")))
    add("gemm/dact/plain/M130N129", "gemm", dict(epi="dact", M=130, N=129, K=64, act=GELU, ident=("repeat", "row_alone")))
    # the product's forms (fp32_path.py) at the tiny geometry D = 128, r = 32, ntok = 5 (2 frames), once at ntok = 197
    D, r = 128, 32
    H4, C = 4 * D, 4 * D + r
    for ntok, fr in ((5, 2), (197, 1)):
        M = ntok * fr
        tag = f"ntok{ntok}"
        if ntok == 197:
            D, r = 64, 16
            H4, C = 4 * D, 4 * D + r
        add(f"gemm/site/x1/{tag}", "gemm", dict(epi="f32", M=M, N=D, K=D, ntok=ntok, bias=True, resid=True, af=True, vec="frame", bt=True))
        add(f"gemm/site/mlp_act/{tag}", "gemm", dict(epi="act", M=M, N=C, K=D, ntok=ntok, bias=True, at=True, act=QGELU, act2=GELU,
                                                    n_split=H4, out2=True))
        add(f"gemm/site/x2/{tag}", "gemm", dict(epi="f32", M=M, N=D, K=C, ntok=ntok, bias=True, resid=True, vec="row0", bt=True))
        add(f"gemm/site/mlp_dact/{tag}", "gemm", dict(epi="dact", M=M, N=C, K=D, ntok=ntok, at=True, act=QGELU, act2=GELU, n_split=H4))
        add(f"gemm/site/dgrad_o/{tag}", "gemm", dict(epi="lin", M=M, N=D, K=D, ntok=ntok, af=True))
        add(f"gemm/site/crs_kv_view/{tag}", "gemm", dict(epi="lin", M=fr, N=D, K=D, bias=True, a_off=D, ident=("strided_eq_dense",)))
        add(f"gemm/site/kv_wqkv_rows/{tag}", "gemm", dict(epi="lin", M=fr, N=2 * D, K=D, bias=True, w_row_off=D, a_pad=4,
                                                      ident=("strided_eq_dense",)))
    # batched linear: the raw scores of lamda (fp32_path.py:112)
    for n_ in (5, 197):
        add(f"gemm/batched/N{n_}", "gemm", dict(epi="lin", M=n_, N=n_, K=64, batch=3))


def cases():
    out, seen = [], [0]

    def add(name, kind, p, family="unit"):
        out.append(Case(name, kind, p, family, seen[0]))
        seen[0] += 1

    _gemm_cases(add)
    # attention: every N in rising order; all families on every 7th
    for kind, top, fams in (("attn_fwd", ATTN_FWD_MAX, ATTN_FAMILIES[:-1]), ("attn_bwd", ATTN_BWD_MAX, ATTN_FAMILIES)):
        for N in range(1, top + 1):
            for fam in (fams if N % 7 == 0 or N in (1, top) else ("unit",)):
                add(f"{kind}/N{N}/{fam}", kind, dict(BT=2, N=N, H=2, ident=("repeat",) if N % 50 == 0 and fam == "unit" else ()), fam)
        for N, H in ((197, 12), (257, 16)):
            for BT in (1, 2):
                add(f"{kind}/site/N{N}H{H}BT{BT}", kind, dict(BT=BT, N=N, H=H))
        for N in (20, 65, 130):
            add(f"{kind}/independent/N{N}", kind, dict(BT=3, N=N, H=2, ident=("nan_neighbours",)))
    # cls attention: every T, (B, H, N) cycling through all twelve combinations; tattn: the four shapes
    combos = [(B, H, N) for B in (1, 3) for H in (1, 12) for N in (2, 5, 197)]
    for kind in ("cls_fwd", "cls_bwd"):
        for T in range(1, 33):
            for j in range(2 if T not in (1, 8, 32) else 12):
                B, H, N = combos[(2 * T + j) % 12] if T not in (1, 8, 32) else combos[j]
                fam = SEQ_FAMILIES[(T + j) % 3]
                add(f"{kind}/T{T}/B{B}H{H}N{N}/{fam}", kind,
                    dict(B=B, T=T, H=H, N=N, ident=("base_plus_zero",) if kind == "cls_bwd" and j == 0 else ()), fam)
    for kind in ("tattn_fwd", "tattn_bwd"):
        for B, T, N, H in TATTN_SHAPES:
            for fam in SEQ_FAMILIES:
                add(f"{kind}/B{B}T{T}N{N}H{H}/{fam}", kind,
                    dict(B=B, T=T, N=N, H=H, ident=("base_plus_zero",) if kind == "tattn_bwd" and fam == "unit" else ()), fam)
    # lamda: every N at D = 64 in every family; every D; strides; the product's batch of 24 frames
    for j, N in enumerate(LAMBDA_N):
        for k, fam in enumerate(LAMBDA_FAMILIES):
            add(f"lambda/N{N}/D64/{fam}", "lambda",
                dict(BT=24 if (j + k) % 4 == 0 and N < 200 else 1, N=N, D=64, lds=N + 3 * ((j + k) % 2), ldkx=64 * (1 + (j + k) % 2),
                     one_minus=(j + k) % 3 != 0), fam)
    for j, D in enumerate(LAMBDA_D):
        for N in (5, 65):
            for fam in ("unit", "cw_dominant"):
                add(f"lambda/N{N}/D{D}/{fam}/strides", "lambda", dict(BT=2, N=N, D=D, lds=N + 3 * (j % 2), ldkx=D * (2 - j % 2),
                                                                     one_minus=True), fam)
    add("lambda/site/N197D768BT24", "lambda", dict(BT=24, N=197, D=768, lds=200, ldkx=768, one_minus=True))
    add("lambda/site/N257D1024BT2", "lambda", dict(BT=2, N=257, D=1024, lds=257, ldkx=2048, one_minus=True))
    # wgrad
    j = 0
    for m, M in enumerate(WGRAD_M):
        big = M > 2000
        for Nw, Kw in ((8, 8),) if big else ((WGRAD_NK[m % 8], WGRAD_NK[(m + 3) % 8]), (WGRAD_NK[(m + 5) % 8], WGRAD_NK[(m + 2) % 8])):
            for form in ("nodb", "db", "at5", "at197"):
                ntok = {"at5": 5, "at197": 197}.get(form, 0)
                add(f"wgrad/M{M}/Nw{Nw}Kw{Kw}/{form}", "wgrad",
                    dict(M=M, Nw=Nw, Kw=Kw, db=form != "nodb", ntok=ntok, g_pad=4 * (j % 2) + 1, a_pad=3 * ((j + 1) % 2),
                         ident=("repeat",) if form == "at5" else ()))
            j += 1
    for Nw, Kw in ((192, 64), (65, 192), (100, 100)):
        add(f"wgrad/M513/Nw{Nw}Kw{Kw}/at5/wide", "wgrad", dict(M=513, Nw=Nw, Kw=Kw, db=True, ntok=5, g_pad=8, a_pad=0))
    # embed_ln
    for B, T, N, D in EMBED_SHAPES:
        for j, fam in enumerate(EMBED_FAMILIES):
            for stats in (False, True):
                add(f"embed_ln/B{B}T{T}N{N}D{D}/{fam}/stats{int(stats)}", "embed_ln",
                    dict(B=B, T=T, N=N, D=D, stats=stats, eps=(1e-5, 1e-6)[(j + int(stats)) % 2]), fam)
    # patchify and its blend
    for pp, H, W in PATCH_SHAPES:
        K = 3 * pp * pp
        for Kp in (K, K + 8):
            for dtype in ("f32", "u8"):
                for norm in (False, True):
                    base = dict(B=3, T=2, H=H, W=W, p=pp, Kp=Kp, dtype=dtype, norm=norm)
                    add(f"patchify/p{pp}H{H}W{W}/Kp{Kp}/{dtype}/norm{int(norm)}", "patchify", base)
        base = dict(B=3, T=2, H=H, W=W, p=pp, Kp=K + 4, dtype="u8", norm=True)
        ident, cycle = [0, 1, 2], [1, 2, 0]
        for lam in (0.0, 1.0, 0.3):
            for partner in (ident, cycle):
                add(f"patchify_blend/p{pp}H{H}W{W}/mixup/lam{lam}/{'cycle' if partner == cycle else 'identity'}", "patchify_blend",
                    dict(base, mode=1, lam=lam, oml=1.0 - lam, partner=partner, plain_twin=lam == 1.0,
                         dtype="u8" if lam != 0.3 else "f32"))
        for tag, box in (("empty", (3, 2, 3, 2)), ("full", (0, 0, W, H)), ("offgrid", (1, 2, W - 2, H - 1))):
            for partner in (ident, cycle):
                add(f"patchify_blend/p{pp}H{H}W{W}/cutmix/{tag}/{'cycle' if partner == cycle else 'identity'}", "patchify_blend",
                    dict(base, mode=2, box=box, partner=partner, plain_twin=tag == "empty" or partner == ident,
                         norm=tag != "full", dtype="f32" if tag == "full" else "u8"))
    return out


# ------------------------------------------------------------------ running -------------------------------------------------
def build_inputs(case):
    return KINDS[case.kind][0](case)


def compare(case, inp, got) -> Dict[str, float]:
    exp = KINDS[case.kind][1](case, inp, got)
    assert set(exp) == set(got), (case.name, sorted(exp), sorted(got))
    return {k: ratio(got[k].double().reshape(exp[k][0].shape), *exp[k]) for k in exp}


def emulate(case, inp, mut=None):
    return KINDS[case.kind][2](case, inp, mut)


def _split_in(c):
    return 0 < c.p.get("n_split", 0) < c.p["N"]


def _has_rs(c):
    return bool(c.p.get("af") or c.p.get("at"))


def _seq_len(c):
    return c.p["N"] if c.kind.startswith("attn") else c.p["T"]


def _last_chunk_has_rows(c):
    return (wgrad_f32_chunks(c.p["M"]) - 1) * wgrad_f32_chunk(c.p["M"]) < c.p["M"]


# mutant -> the cases (of the kinds that list it in KINDS) on which it must fall outside the bound, with the reason for
# leaving the others out: there the mutant changes nothing
MUST_SEE = {
    # 2^-9 per operand against (K + 2) 2^-24 sum |a w|: a kernel that truncates an operand to bf16 fails on every case
    "bf16_operands": lambda c: True,
    "k_tail_dropped": lambda c: c.p["K"] % 16 != 0 and c.family in ("unit", "offset"),
    # the four columns behind the split take the other activation (and lose rs): visible where the two differ
    "split_plus_4": lambda c: c.p["epi"] in ("act", "dact") and _split_in(c) and c.p["n_split"] + 4 <= c.p["N"] and c.family == "unit",
    "act_swapped": lambda c: (c.p["epi"] in ("act", "dact") and c.p.get("act", 0) != c.p.get("act2", 0) and c.family == "unit"
                              and (_split_in(c) or c.p.get("n_split", 0) == 0)),
    "rs_on_frozen": lambda c: c.p["epi"] in ("act", "dact") and _split_in(c) and _has_rs(c) and c.family == "unit",
    "rbo_ignored": lambda c: bool(c.p.get("rbo")) and _has_rs(c) and bool(c.p.get("bias")),
    "vec_frame_n": lambda c: c.p.get("vec") == "row0" and c.p["M"] > c.p["ntok"],
    # (rs_bias_only: at multiplies the bias alone, small next to an `offset` product; n_split = N: no column takes rs;
    # wgrad: one row has m / ntok = m % ntok = 0)
    "at_row_div_ntok": lambda c: (bool(c.p.get("ntok")) and c.p["M"] > 1 if c.kind == "wgrad" else
                                  bool(c.p.get("at")) and c.p["M"] > 1 and c.family != "bigpre" and not c.p.get("rbo")
                                  and c.p.get("n_split", 0) < c.p["N"]),
    "batched_item_mn": lambda c: c.p.get("batch", 1) > 1,
    # exp overflows without the shift only where the logits pass 88 (one key: softmax is 1 whatever the logits)
    "no_max_shift": lambda c: c.family == "big" and _seq_len(c) > 1,
    "last_key_dropped": lambda c: c.p["N"] % 64 == 1 and c.p["N"] > 1 and c.family == "unit",
    # (zero_do: every gradient is 0)
    "scale_twice": lambda c: _seq_len(c) > 1 and c.family == "unit",
    "del_without_p": lambda c: c.p["N"] > 1 and c.family == "unit",
    "dv_from_ds": lambda c: c.family == "unit",
    # (lam = 1/2 is its own mirror image; one shared maximum makes the two shifts equal)
    "separate_shifts": lambda c: c.family in ("cw_dominant", "ow_dominant"),
    "lds_as_n": lambda c: c.p["lds"] > c.p["N"] and c.p["N"] > 1,
    "cw_ow_swapped": lambda c: c.family in ("cw_dominant", "ow_dominant"),
    "tail_rows_dropped": lambda c: c.p["M"] % 16 != 0,
    "assign": lambda c: True,
    "last_chunk_dropped": _last_chunk_has_rows,
    # eps outside the root: visible where var is far from 1 (scaled rows, constant rows)
    "eps_outside": lambda c: c.family in ("scaled", "const"),
    "class_row_from_tok": lambda c: c.family != "const",
    "channel_stride_p": lambda c: True,
    "box_axes_swapped": lambda c: c.p["mode"] == 2 and "offgrid" in c.name and "cycle" in c.name,
}


def mutants(case):
    """the mutants of the case's kind that must fall outside the bound on this case"""
    return tuple(m for m in KINDS[case.kind][4] if MUST_SEE[m](case))


class _Ctx:
    def __init__(self, dev):
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from aim_amd import ops
        from aim_amd.lib import check, load_library
        self.ops, self.lib, self.check, self.stream, self.dev = ops, load_library(), check, ops._stream, torch.device(dev)


_FATAL = ("illegal memory access", "HIP error", "hipError", "unspecified launch failure")


def _to(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}


def run_case(ctx, case):
    rec = {"kind": case.kind, "checks": {}, "finite": {}, "pad": {}, "ident": {}, "evidence": {}}
    inp = build_inputs(case)
    got = KINDS[case.kind][3](ctx, case, inp, rec)
    if ctx.dev.type == "cuda":
        torch.cuda.synchronize()
    rec["checks"] = compare(case, _to(inp, ctx.dev), got)
    return rec


def run_probe(ctx, points=2 ** 18):
    """the activations alone: aim_gemm_f32(ACT / DACT) with K = 4, A = [x, 0, 0, 0] (DACT: [1, 0, 0, 0] and aux = x), W = [1, 0, 0,
    0], no bias, so pre = x exactly; worst |kernel - float64| / (1 + |x|) per activation over a dense grid of [-110, 110] and the
    points of the `bigpre` family"""
    dev = ctx.dev
    big = torch.cat([gemm_inputs(c)["bias"] for c in cases() if c.kind == "gemm" and c.family == "bigpre" and c.p["epi"] == "act"][:2])
    x = torch.cat([torch.linspace(-110.0, 110.0, points, dtype=F64).to(F32), big]).to(dev)
    M = x.numel()
    A = torch.zeros((M, 4), dtype=F32, device=dev)
    W = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=F32, device=dev)
    out, res = torch.empty((M, 1), dtype=F32, device=dev), {}
    x64 = x.double()[:, None]
    for act, name in ((QGELU, "qgelu"), (GELU, "gelu")):
        A[:, 0] = x
        ctx.check(_gemm_run(ctx, EPI["act"], 1, A, W, out, M, 1, 4, act=act), "aim_gemm_f32")
        torch.cuda.synchronize()
        res["act_" + name] = float(((out.double() - _act64(x64, act)).abs() / (1 + x64.abs())).max())
        A[:, 0] = 1.0
        ctx.check(_gemm_run(ctx, EPI["dact"], 1, A, W, out, M, 1, 4, act=act, aux=x[:, None], ldaux=1), "aim_gemm_f32")
        torch.cuda.synchronize()
        res["dact_" + name] = float(((out.double() - _dact64(x64, act)).abs() / (1 + x64.abs())).max())
    return res


REFUSAL_TEXT = {
    "gemm_f32/null_args": "null args / bad batch", "gemm_f32/batch0": "null args / bad batch",
    "gemm_f32/null_out": "null operand or empty problem", "gemm_f32/M0": "null operand or empty problem",
    "gemm_f32/K%4": "multiples of 4", "gemm_f32/lda%4": "multiples of 4", "gemm_f32/A_misaligned": "16-byte aligned",
    "gemm_f32/ldo<N": "ldo < N", "gemm_f32/lda<K": "lda < K or ldw < K", "gemm_f32/ldw<K": "lda < K or ldw < K",
    "gemm_f32/ldr<N": "ldr < N", "gemm_f32/ldv<N": "ldr < N", "gemm_f32/row_factors_without_ntok": "ntok required",
    "gemm_f32/batched_act": "linear epilogue only", "gemm_f32/out2_with_f32": "out2", "gemm_f32/ldo2<N": "out2",
    "gemm_f32/dact_without_aux": "AIM_EPI_DACT needs", "gemm_f32/ldaux<N": "AIM_EPI_DACT needs", "gemm_f32/epilogue4": "unsupported epilogue",
    "attn_fwd_f32/N318": "unsupported shape", "attn_bwd_f32/N311": "unsupported shape", "attn_bwd_f32/workspace": "workspace too small",
    "cls_attn_fwd_f32/T33": "unsupported shape", "cls_attn_bwd_f32/T33": "unsupported shape", "tattn_fwd_f32/T33": "unsupported shape",
    "tattn_bwd_f32/T33": "unsupported shape", "lambda_f32/lds<N": "bad arguments",
    "patchify_f32/Kp<3pp": "multiple of 4", "patchify_f32/Kp%4": "multiple of 4", "patchify_f32/H%p": "bad shape",
    "patchify_f32/in_dtype2": "in_dtype must be", "patchify_f32/mean_without_std": "null pointer",
    "patchify_blend_f32/Kp<3pp": "multiple of 4", "patchify_blend_f32/Kp%4": "multiple of 4", "patchify_blend_f32/H%p": "bad shape",
    "patchify_blend_f32/in_dtype2": "in_dtype must be", "patchify_blend_f32/mean_without_std": "null pointer",
    "embed_ln_f32/N1": "bad arguments", "embed_ln_f32/pre_without_mean": "go together",
    "wgrad_f32/ldg<Nw": "bad arguments", "wgrad_f32/lda<Kw": "bad arguments", "wgrad_f32/at_without_ntok": "ntok required", "wgrad_f32/workspace": "workspace too small",
}


def run_refusals(ctx):
    """at least one call per AIM_CHECK_ARG of csrc/fp32.hip (test_fp32_cases_cpu.py ties REFUSAL_TEXT to the macros of the file) and
    per in_dtype / epilogue switch, each decided on the host before any launch:
    {name: {"rc", "message", "untouched": every output and workspace, prefilled with NaN, still NaN}}"""
    dev, lib = ctx.dev, ctx.lib
    out = {}

    def attempt(name, fn, watched):
        rc = fn()
        msg = lib.aim_last_error()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        out[name] = {"rc": rc, "message": msg.decode() if rc and msg else None,
                     "untouched": all(bool(torch.isnan(t).all()) for t in watched)}

    def nanf(*shape):
        return torch.full(shape, NAN, dtype=F32, device=dev)

    def zf(*shape):
        return torch.zeros(shape, dtype=F32, device=dev)

    M, N, K = 8, 12, 16
    A, W, vec8 = zf(M + 1, K + 8), zf(N, K + 8), zf(2, N)

    def gemm(name, epi=0, batch=1, a=None, o=None, Kk=K, Mm=M, **kw):
        o_ = nanf(M, N + 4) if o is None else o
        watched = [o_] + [kw[k] for k in ("out2",) if k in kw]
        attempt("gemm_f32/" + name, lambda: _gemm_run(ctx, epi, batch, A if a is None else a, W, o_, Mm, N, Kk, **kw), watched)

    attempt("gemm_f32/null_args", lambda: lib.aim_gemm_f32(None, 0, 1, ctx.stream()), ())
    gemm("batch0", batch=0)

    def null_out():
        from ctypes import byref
        g = _gemm_args(ctx, A, W, zf(M, N), M, N, K)
        g.out = None
        return lib.aim_gemm_f32(byref(g), 0, 1, ctx.stream())

    attempt("gemm_f32/null_out", null_out, ())
    gemm("M0", Mm=0)
    gemm("K%4", Kk=14)
    gemm("lda%4", lda=K + 2)
    gemm("A_misaligned", a=A.view(-1)[1:1 + M * (K + 8)].view(M, K + 8))
    gemm("ldo<N", ldo=N - 1)
    gemm("lda<K", lda=K - 4)
    gemm("ldw<K", ldw=K - 4)
    gemm("ldr<N", epi=3, resid=zf(M, N), ldr=N - 1)
    gemm("ldv<N", epi=3, vec=vec8, ldv=N - 1, ntok=4)
    gemm("row_factors_without_ntok", af=zf(2))
    gemm("batched_act", epi=1, batch=2)
    o2 = nanf(M, N)
    gemm("out2_with_f32", epi=3, out2=o2)
    gemm("ldo2<N", epi=1, out2=o2, ldo2=N - 1)
    gemm("dact_without_aux", epi=2)
    gemm("ldaux<N", epi=2, aux=zf(M, N), ldaux=N - 1)
    gemm("epilogue4", epi=4)

    H, D = 1, 64
    for name, n, bwd in (("attn_fwd_f32/N318", 318, False), ("attn_bwd_f32/N311", 311, True), ("attn_bwd_f32/workspace", 8, True)):
        qkv, o = zf(n, 3 * D), nanf(n, 3 * D if bwd else D)
        need = attn_bwd_f32_workspace_bytes(1, n, H)
        ws = nanf(need // 4)
        if bwd:
            short = 1 if name.endswith("workspace") else 0
            attempt(name, lambda: lib.aim_attn_bwd_f32(qkv.data_ptr(), zf(n, D).data_ptr(), o.data_ptr(), 1, n, H, ws.data_ptr(),
                                                       need - short, ctx.stream()), (o, ws))
        else:
            attempt(name, lambda: lib.aim_attn_fwd_f32(qkv.data_ptr(), o.data_ptr(), 1, n, H, ctx.stream()), (o,))
    T, Nn = 33, 2
    qkv, dq, oc, of = zf(T * Nn, 3 * D), nanf(T * Nn, 3 * D), nanf(T, D), nanf(T * Nn, D)
    attempt("cls_attn_fwd_f32/T33", lambda: lib.aim_cls_attn_fwd_f32(qkv.data_ptr(), Nn * 3 * D, oc.data_ptr(), 1, T, H, ctx.stream()), (oc,))
    attempt("cls_attn_bwd_f32/T33", lambda: lib.aim_cls_attn_bwd_f32(qkv.data_ptr(), Nn * 3 * D, zf(T, D).data_ptr(), dq.data_ptr(), 1, T, H,
                                                                     ctx.stream()), (dq,))
    attempt("tattn_fwd_f32/T33", lambda: lib.aim_tattn_fwd_f32(qkv.data_ptr(), of.data_ptr(), 1, T, Nn, H, ctx.stream()), (of,))
    attempt("tattn_bwd_f32/T33", lambda: lib.aim_tattn_bwd_f32(qkv.data_ptr(), zf(T * Nn, D).data_ptr(), dq.data_ptr(), 1, T, Nn, H,
                                                               ctx.stream()), (dq,))
    lam, om = nanf(2), nanf(2)
    attempt("lambda_f32/lds<N", lambda: lib.aim_lambda_f32(zf(2, 5, 5).data_ptr(), 4, zf(10, 3 * D).data_ptr(), zf(2, D).data_ptr(), D,
                                                           lam.data_ptr(), om.data_ptr(), 2, 5, D, 0.125, ctx.stream()), (lam, om))
    base = dict(B=2, T=1, H=4, W=6, p=2, Kp=12, dtype="f32", mode=2, box=(0, 0, 2, 2))
    img, m3 = zf(2, 3, 1, 4, 6), zf(3)
    partner = torch.zeros(2, dtype=torch.int32, device=dev)
    for kind in ("patchify", "patchify_blend"):
        for name, over, mean, std in (("Kp<3pp", dict(Kp=8), None, None), ("Kp%4", dict(Kp=14), None, None), ("H%p", dict(H=5), None, None),
                                      ("in_dtype2", dict(in_dtype=2), None, None), ("mean_without_std", {}, m3, None)):
            Ap = nanf(2 * 6, 16)
            attempt(f"{kind}_f32/{name}", lambda: _patchify_rc(ctx, kind, base, img, mean, std, Ap, partner, **over), (Ap,))
    x, pre, rs = nanf(6, D), nanf(6, D), nanf(6)
    z = zf(6, D)
    emb = lambda N_, pre_, mean_, rstd_: lib.aim_embed_ln_f32(  # noqa: E731
        z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), x.data_ptr(), pre_, mean_, rstd_, 2, 1, N_, D,
        1e-5, ctx.stream())
    attempt("embed_ln_f32/N1", lambda: emb(1, None, None, None), (x,))
    attempt("embed_ln_f32/pre_without_mean", lambda: emb(3, pre.data_ptr(), None, rs.data_ptr()), (x, pre, rs))
    Mw, Nw, Kw = 20, 8, 8
    G, Aw, dW, db = zf(Mw, Nw), zf(Mw, Kw), nanf(Nw, Kw), nanf(Nw)
    need = wgrad_f32_workspace_bytes(Mw, Nw, Kw)
    ws = nanf(need // 4)
    wg = lambda ldg=Nw, lda=Kw, at=None, ntok=0, wb=need: lib.aim_wgrad_f32(  # noqa: E731
        G.data_ptr(), ldg, Aw.data_ptr(), lda, dW.data_ptr(), Mw, Nw, Kw, db.data_ptr(), at, ntok, ws.data_ptr(), wb, ctx.stream())
    attempt("wgrad_f32/ldg<Nw", lambda: wg(ldg=Nw - 1), (dW, db, ws))
    attempt("wgrad_f32/lda<Kw", lambda: wg(lda=Kw - 1), (dW, db, ws))
    attempt("wgrad_f32/at_without_ntok", lambda: wg(at=zf(5).data_ptr()), (dW, db, ws))
    attempt("wgrad_f32/workspace", lambda: wg(wb=need - 4), (dW, db, ws))
    return out


def run(dev="cuda"):
    """every case, the refusals and the activation probe on `dev`: {"cases": {name: record}, "refusals", "probe", "seconds"}"""
    ctx = _Ctx(dev)
    t0 = time.time()
    res = {"cases": {}, "errors": {}}
    with torch.no_grad():
        for case in cases():
            try:
                res["cases"][case.name] = run_case(ctx, case)
            except Exception as e:      # a refused or failed call is a finding of the test; after a GPU fault nothing more runs
                res["errors"][case.name] = f"{type(e).__name__}: {e}"
                if any(s in str(e) for s in _FATAL):
                    res["fatal"] = case.name
                    return res
        res["seconds"] = time.time() - t0
        res["refusals"] = run_refusals(ctx)
        res["probe"] = run_probe(ctx)
    res["seconds_all"] = time.time() - t0
    return res
