"""Every call form of the kernels at the two ends of a training step -- pixels in, loss out, weights updated: the head and
the losses (aim_head_fwd / aim_head_bwd / aim_ce_topk / aim_ce_soft, csrc/head.hip), the lamda statistic (aim_qk_cross /
aim_qk_border / aim_lambda / aim_lambda_partials, csrc/cls_attn.hip), the patch gather (aim_patchify) and the optimizer
(aim_adamw_flat, csrc/embed_misc.hip); float64 references on the same fp32 / bf16 / uint8 operand values and element-wise
bounds derived from each kernel's summation order.

A plain module (no fixtures), in the manner of rowwise_cases.py.  `run(dev)` calls libaim_hip.so through ctypes, every case
once in the calling process; test_ends_cases_gpu.py reads its records and test_ends_cases_cpu.py proves on the CPU that the
bounds accept an fp32 emulation of each kernel's arithmetic in its summation order (`emulate`) and reject the same emulation
with one plausible bug (`emulate(..., mut)`).  Every output, every workspace and eight guard elements behind every buffer
(inputs too) go in as NaN.

Notation: u = 2^-24 (one fp32 rounding, relative), FL = 2^-126 (a result below the normal range may be flushed).  A sum of
terms: (longest addition chain + roundings per term) u sum|terms| (`_sum_bound`), an accumulated output's initial value
counting as a term.  A 256-thread strided block sum of n terms has the chain ceil(n/256) + 6 (butterfly) + 3 (waves).

head_fwd.  pooled = drop * (sum_t feat) / T: T - 1 adds, 1/T (one rounding) and its product, the drop factor:
    e_p = (T + 2) u |drop| mean_t|feat|.
  score = pooled . w + bias: a lane adds ceil(D/64) products (one rounding each), 6 butterfly steps, the bias:
    e_s = (ceil(D/64) + 6 + 1 + 1) u (sum|w pooled| + |bias|) + sum_d |w_d| e_p[d]     (reference on the float64 pooled).
head_bwd.  dW += sum_b dscore pooled: chain B, one rounding per product, dW's initial value a term.  db += sum_b dscore:
  chain B.  dfeat = drop / T * sum_c dscore W: a class group adds ceil(C/4) products, (g0 + g1) + (g2 + g3), the division
  by T and the drop factor: (ceil(C/4) + 2 + 1 + 2) u |drop| / T sum|dscore W|.
ce_topk.  __expf(x) is modelled as exp2(fl(x log2e)) with a 1-ulp exp2: fl(x log2e) carries the rounding of the constant
  and of the product, 2 u |x| in the result, and the 1-ulp exp2 2 u: 2 u (1 + |x|).  __logf(y) as fl(log2(y) ln2) with a
  1-ulp log2: 4 u |log y|.  The hardware's rounding is not documented, so both intrinsic terms get a factor of 4:
    E(x) = 8 u (1 + |x|),  L(y) = 16 u |log y|.
  The maximum is exact.  d = s - max (u |d|); sum = block sum of __expf(d):
    r_sum = sum e^d (E(d) + u |d|) / sum e^d + (ceil(C/256) + 9) u + C FL / sum
    e_lse = r_sum + L(sum) + u |lse|;  loss_b = lse - s[label]: e_lse + u |loss_b|
    out[0] = sum_valid loss_b / n_valid in sample order: sum e_loss / n_valid + (B + 1) u sum|loss_b| / n_valid
    p = __expf(s - lse): e_p = p (e_lse + u |x| + E(x)) + FL;  dscore = (p - onehot) / n_valid: (e_p + u |p - onehot|) /
    n_valid + 2 u |dscore| (1 / n_valid is rounded, then the product).
  Exact: an ignored sample's dscore row and loss term are zero; the accuracy columns are float32(count) / float32(B) with
  the count by numpy's stable argsort (a label is in the top k iff fewer than k classes score higher or tie with a larger
  index).  All labels ignored: 0 / 0, out[0] is NaN, as F.cross_entropy(ignore_index=-100) returns on the CPU
  (test_ends_cases_cpu.py::test_torch_agrees_on_the_nan_cases); the record says which it saw.
  The mutant "softmax without the max shift" cannot be seen on logits of +-80: C e^80 <= 5.5e37 stays finite in fp32 and
  the rounding of 80 log2e (about 1e-6 in the result) is below the one rounding of lse = 80 (4.8e-6) that every correct
  kernel is allowed.  The +-80 family stays in the comparison and a +-100 family is added, where an unshifted e^100
  overflows: the mutant must be seen there.
  The mutant "k2 not clamped to C" is listed and cannot be seen: at most C - 1 classes are ahead of a valid label, fewer
  than min(k2, C) and than k2 alike whenever k2 >= C; the CPU test holds the mutant to the unmutated bits instead.
ce_soft.  expf / logf are libm-accurate: 2 u each.  Block sums with the waves joined pairwise: chain ceil(C/256) + 6 + 2.
    r_sum = sum e^d (u |d| + 2 u) / sum + chain u;  e_lse = r_sum + 2 u |log sum| + u |lse|
    t = w y (u when w is given);  loss_b = sum t (lse - s): sum|t| e_lse + (chain + 3) u sum|t (lse - s)|
    wy_b = sum t: (chain + 1) u sum|t|;  den = B, or the sample-ordered sum of wy_b: sum e_wy + B u sum|wy|
    out = sum_b loss_b / den: (sum e_loss + B u sum|loss_b|) / den + |out| (e_den / den + u)
    dscore = (p wy - t) / den, p = expf(s - lse): e_p = p (e_lse + u |x| + 2 u) + FL;
      (wy e_p + p e_wy + u |p wy| + u |t| + u |p wy - t|) / den + |dscore| (e_den / den + u).
  Weighted with sum w y = 0 over the whole batch: 0 / 0, out and dscore are NaN, as F.cross_entropy(weight=w) returns on the
  CPU for hard labels that are all ignored (the zero one-hot rows this kernel is handed for them) and as the weighted
  soft-label formula sum(-w y log_softmax) / sum(w y) evaluates in torch (same CPU test).
qk_cross.  bf16 products are exact in fp32.  A lane adds ceil(D/512) 8 products, the butterfly, the scale:
    (8 ceil(D/512) + 6 + 1) u |scale| sum|q k|.   lambda with ss == NULL: (4 ceil(D/256) + 6 + 1) u |scale| sum|q k|.
qk_border.  16 fused multiply-adds per lane (two 512-column chunks, the second all zeros at D = 512), the butterfly, the
  scale: (16 + 6 + 1) u |scale| sum|q k| =: e_s.  A (max, sum) pair: the maximum is the exact maximum of the fp32 scores and
  is held to the float64 maximum within max e_s; max + log(sum) is held to the float64 log-sum-exp within
    max e_s + sum e^d (u |d| + 2 u) / sum + (ceil(cnt/256) + 9) u + cnt FL / sum.
lambda / lambda_partials.  cw = sum_i exp(ss_i - M), ow = sum_t sum_t exp(max_t - M) with ONE shift M (any common shift
  cancels in the ratio, so the float64 reference takes its own).  Absolute errors
    a_c = sum e^d (e_ss + u |d| + 2 u) + chain u cw + N FL,   a_o = sum o_t (u |d_t| + 3 u) + chain u ow + ntiles FL max sum_t
    lam = cw / (cw + ow): (ow a_c + cw a_o) / (cw + ow)^2 + 2 u lam;   1 - lam: that + u |1 - lam|.
  (lambda: block sums, chain ceil(n/256) + 9; lambda_partials: 8 slots in order, chain 8.)  When ow leads by more than
  104 in the exponent cw underflows to 0: the FL terms make the bound absolute there.
patchify.  A gather, a subtraction and a division by std (two correctly rounded operations with nothing to contract: there
  is no multiply next to an add, and the build has no fast-math) and one round-to-nearest-even to bf16: bound 0 against torch's
  float32 arithmetic on the CPU, padding columns K .. Kp are +0 (`exact_bits` compares the bit patterns).
adamw.  Reference in float64 on the fp32 values of p, g, m, v and of lr, beta1, beta2, eps, weight_decay, grad_scale; the
  bias corrections are exact in the reference, the host's are bc1 = 1 - powf(beta1, step), bc2s = sqrtf(1 - powf(beta2,
  step)) in fp32 with a 1-ulp powf: r_bc1 = 2 u beta1^s / bc1 + u,  r_bc2s = (2 u beta2^s / bc2 + u) / 2 + u.
    g' = g gs (u);  m' = fma(1 - b1, g', fl(b1 m)): e_m = u (|b1 m| + |m'| + (1 - b1) |g'|) + FL
    v' = fma(b2, v, fl(fl((1 - b2) g') g')): e_v = u (4 (1 - b2) g'^2 + |v'|) + FL
    den = sqrt(v') / bc2s + eps: r_den = (e_v / (2 v') + 2 u + r_bc2s) (sqrt(v') / bc2s) / den + u
    U = (lr / bc1) m' / den: r_U = r_bc1 + u + e_m / |m'| + r_den + 2 u
    p' = fma(c, p, -U), c = fl(1 - lr wd): the bound is stated on the UPDATE p' - p (1 - lr wd) against -U:
      |U| r_U + (1 + [wd != 0]) u |p|       (the rounding of c, when it is not 1, and of the result).
  An fp32 intermediate that overflows is infinite in the kernel and in torch's fp32 AdamW alike; the reference maps every
  float64 intermediate beyond the fp32 range to infinity (|g| = 1e20: v' = inf, the update is 0, m' stays finite), and one
  below it may be flushed (|g| = 1e-25: g^2 contributes nothing; the FL terms).
"""
import math
import os
import sys
import time
from dataclasses import dataclass, field
from typing import Dict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import U24, ratio  # noqa: E402
from rowwise_cases import _FATAL, _XOR, _groups4, _seq, _sum_bound  # noqa: E402
from rowwise_cases import _bits_eq as _bits_eq32  # noqa: E402

BF16, F32, F64, I64, U8T = torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.uint8
NAN, INF = float("nan"), float("inf")
u = U24
FL = 2.0 ** -126
F32MAX = 3.4028234663852886e38
LOG2E32 = torch.tensor(1.4426950408889634, dtype=F32)
LN2_32 = torch.tensor(0.6931471805599453, dtype=F32)


@dataclass
class Case:
    name: str
    kind: str
    p: dict = field(default_factory=dict)
    family: str = "unit"
    seed: int = 0


def _bits_eq(a, b):
    """rowwise_cases._bits_eq, also for the float64 values derived from a (max, sum) pair"""
    if a.dtype == F64:
        return a.shape == b.shape and bool((a.contiguous().view(I64) == b.contiguous().view(I64)).all())
    return _bits_eq32(a, b)


def _cdiv(a, b):
    return (a + b - 1) // b


def _gen(case):
    return torch.Generator().manual_seed(1000 + case.seed)


def _rn(g, *shape):
    return torch.randn(shape, generator=g, dtype=F32)


def eratio(got, ref, bound) -> float:
    """gemm_cases.ratio where the reference is finite; where it is NaN or infinite the result must be the same"""
    got, ref = got.double().reshape(ref.shape), ref.double()
    fin = torch.isfinite(ref)
    same = (torch.isnan(ref) & torch.isnan(got)) | (ref == got)
    if not bool((fin | same).all()):
        return INF
    if not bool(fin.any()):
        return 0.0
    return ratio(got[fin], ref[fin], bound.double().expand(ref.shape)[fin])


# ---- fp32 emulation pieces ------------------------------------------------------------------------------------------------
def _butterfly(acc):
    """[..., 64] -> [...]: wave_sum"""
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., _XOR[o]]
    return acc[..., 0]


def _lanes(t, per, width):
    """[..., D] f32 -> wave sum where lane l adds elements l*per + e + width*i (i outer, e inner) one by one"""
    D = t.shape[-1]
    n = _cdiv(D, width)
    pad = torch.zeros(t.shape[:-1] + (n * width,), dtype=F32)
    pad[..., :D] = t
    v = pad.view(t.shape[:-1] + (n, width // per, per))
    acc = torch.zeros(t.shape[:-1] + (64,), dtype=F32)
    for i in range(n):
        for e in range(per):
            acc = acc + v[..., i, :, e]
    return _butterfly(acc)


def _block256(t, pairwise):
    """[R, n] f32 -> [R]: thread tid adds elements tid, tid + 256, ...; wave_sum; the four waves in order or pairwise"""
    R, n = t.shape
    k = max(1, _cdiv(n, 256))
    pad = torch.zeros((R, k * 256), dtype=F32)
    pad[:, :n] = t
    w = _butterfly(_seq(pad.view(R, k, 256).transpose(0, 1)).view(R, 4, 64))
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]) if pairwise else ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _fma(a, b, c):
    """fl32(a b + c) for fp32 operands (the product is exact in float64)"""
    return (a.double() * b.double() + c.double()).float()


def _fast_exp(x):
    return torch.exp2(x * LOG2E32)


def _fast_log(y):
    return torch.log2(y) * LN2_32


# ---- kinds: inputs(case) -> CPU tensors; expected(case, inp, got) -> {output: (float64 value, bound)};
#      emulate(case, inp, mut) -> {output: tensor}; launch(ctx, case, inp, **variant) -> ({output: cpu tensor}, {output: guard ok})
KINDS: Dict[str, tuple] = {}


# ================================================================== head_fwd =================================================
def head_fwd_inputs(case):
    p, g = case.p, _gen(case)
    B, T, D, C = p["B"], p["T"], p["D"], p["C"]
    feat = _rn(g, B, T, D)
    if case.family == "frame1e4":
        feat[:, 0] *= 1e4
    elif case.family == "equal":
        feat = torch.full((B, T, D), 0.7, dtype=F32)
    inp = {"feat": feat, "W": _rn(g, C, D) / math.sqrt(D), "bias": _rn(g, C)}
    drop = (torch.rand((B, D), generator=g) < 0.5).float() * 2.0
    drop[:, 0] = 2.0
    drop[:, -1] = 0.0 if D > 1 else 2.0
    inp["drop"] = drop
    return inp


def head_fwd_expected(case, inp, got=None):
    p = case.p
    T, D = p["T"], p["D"]
    feat, W = inp["feat"].double(), inp["W"].double()
    drop = inp["drop"].double() if p["drop"] else torch.ones_like(feat[:, 0])
    bias = inp["bias"].double() if p["bias"] else torch.zeros(p["C"], dtype=F64)
    pooled = feat.sum(1) / T * drop
    e_p = (T + 2) * u * drop.abs() * feat.abs().mean(1)
    score = pooled @ W.T + bias
    e_s = _sum_bound(_cdiv(D, 64) + 7, 1, pooled.abs() @ W.abs().T, bias.expand_as(score)) + e_p @ W.abs().T
    return {"pooled": (pooled, e_p), "score": (score, e_s)}


HEAD_FWD_MUTANTS = ("mean_Tm1", "bias_next", "pooled_nodrop", "last_class_unwritten")


def head_fwd_emulate(case, inp, mut=None):
    p = case.p
    T = p["T"]
    feat = inp["feat"]
    Tn = T - 1 if mut == "mean_Tm1" else T
    s = torch.zeros_like(feat[:, 0])
    for t in range(Tn):
        s = s + feat[:, t]
    s = s * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(max(Tn, 1)), dtype=F32))
    saved = s
    if p["drop"]:
        s = s * inp["drop"]
        if mut != "pooled_nodrop":
            saved = s
    acc = _lanes(inp["W"][None] * s[:, None, :], 1, 64)
    if p["bias"]:
        acc = acc + (inp["bias"].roll(-1) if mut == "bias_next" else inp["bias"])
    else:
        acc = acc + 0.0
    if mut == "last_class_unwritten":
        acc[:, -1] = NAN
    return {"pooled": saved, "score": acc}


def head_fwd_launch(ctx, case, inp, drop="case", bias="case", rows=None):
    p = case.p
    B, T, D, C = p["B"], p["T"], p["D"], p["C"]
    feat = inp["feat"]
    dr = inp["drop"] if p["drop"] else None
    bi = inp["bias"] if p["bias"] else None
    if drop == "ones":
        dr = torch.ones((B, D), dtype=F32)
    if bias == "zeros":
        bi = torch.zeros(C, dtype=F32)
    if rows is not None:
        feat, B = feat[rows], len(rows)
        dr = dr[rows] if dr is not None else None
    d = ctx.put(feat=feat, W=inp["W"], drop=dr, bias=bi)
    o = ctx.outs(pooled=(B, D), score=(B, C))
    ctx.call("aim_head_fwd", d["feat"], d["drop"], d["W"], d["bias"], o["pooled"], o["score"], B, T, D, C)
    return ctx.collect(o)


def head_fwd_idents(ctx, case, inp, got, rec):
    p = case.p
    if p["B"] > 1:
        g1, _ = head_fwd_launch(ctx, case, inp, rows=[1])
        rec["ident"]["row_alone"] = all(_bits_eq(got[k][1:2], g1[k]) for k in got)
    if not p["drop"]:
        g1, _ = head_fwd_launch(ctx, case, inp, drop="ones")
        rec["ident"]["null_eq_ones"] = all(_bits_eq(got[k], g1[k]) for k in got)
    if not p["bias"]:
        g1, _ = head_fwd_launch(ctx, case, inp, bias="zeros")
        rec["ident"]["null_eq_ones"] = rec["ident"].get("null_eq_ones", True) and all(_bits_eq(got[k], g1[k]) for k in got)


KINDS["head_fwd"] = (head_fwd_inputs, head_fwd_expected, head_fwd_emulate, head_fwd_launch, HEAD_FWD_MUTANTS, head_fwd_idents)


# ================================================================== head_bwd =================================================
HEAD_BWD_SUBSETS = (("dW", "db", "dfeat"), ("dW", "db"), ("dW",), ("dfeat",), ("db",))


def head_bwd_inputs(case):
    p, g = case.p, _gen(case)
    B, D, C = p["B"], p["D"], p["C"]
    drop = (torch.rand((B, D), generator=g) < 0.5).float() * 2.0
    drop[:, 0] = 2.0
    return {"dscore": _rn(g, B, C) / C, "pooled": _rn(g, B, D), "drop": drop, "W": _rn(g, C, D) / math.sqrt(D),
            "dW0": _rn(g, C, D), "db0": _rn(g, C)}


def head_bwd_expected(case, inp, got=None):
    p = case.p
    B, T, C = p["B"], p["T"], p["C"]
    ds, po, W = inp["dscore"].double(), inp["pooled"].double(), inp["W"].double()
    drop = inp["drop"].double() if p["drop"] else torch.ones_like(po)
    out = {}
    if "dW" in p["outs"]:
        out["dW"] = (inp["dW0"].double() + ds.T @ po, _sum_bound(B, 1, ds.abs().T @ po.abs(), inp["dW0"].double()))
    if "db" in p["outs"]:
        out["db"] = (inp["db0"].double() + ds.sum(0), _sum_bound(B, 0, ds.abs().sum(0), inp["db0"].double()))
    if "dfeat" in p["outs"]:
        v = (ds @ W) / T * drop
        bv = (_cdiv(C, 4) + 5) * u * (ds.abs() @ W.abs()) / T * drop.abs()
        out["dfeat"] = (v[:, None, :].expand(B, T, -1).contiguous(), bv[:, None, :].expand(B, T, -1).contiguous())
    return out


HEAD_BWD_MUTANTS = ("assign", "no_invT", "drop_next", "db_Bm1")


def head_bwd_emulate(case, inp, mut=None):
    p = case.p
    B, T = p["B"], p["T"]
    ds, po, W = inp["dscore"], inp["pooled"], inp["W"]
    out = {}
    if "dW" in p["outs"]:
        acc = _seq(ds[:, :, None] * po[:, None, :])
        out["dW"] = acc if mut == "assign" else inp["dW0"] + acc
    if "db" in p["outs"]:
        nb = B - 1 if mut == "db_Bm1" else B
        out["db"] = inp["db0"] + (_seq(ds[:nb]) if nb else torch.zeros_like(ds[0]))
    if "dfeat" in p["outs"]:
        v = torch.stack([_groups4(ds[b][:, None] * W) for b in range(B)])
        if mut != "no_invT":
            v = v / torch.tensor(float(T), dtype=F32)
        if p["drop"]:
            v = v * (inp["drop"].roll(-1, 1) if mut == "drop_next" else inp["drop"])
        out["dfeat"] = v[:, None, :].expand(B, T, -1).contiguous()
    return out


def head_bwd_launch(ctx, case, inp, outs=None):
    p = case.p
    B, T, D, C = p["B"], p["T"], p["D"], p["C"]
    outs = p["outs"] if outs is None else outs
    d = ctx.put(dscore=inp["dscore"], pooled=inp["pooled"], drop=inp["drop"] if p["drop"] else None, W=inp["W"])
    shapes, init = {}, {}
    if "dW" in outs:
        shapes["dW"], init["dW"] = (C, D), inp["dW0"]
    if "db" in outs:
        shapes["db"], init["db"] = (C,), inp["db0"]
    if "dfeat" in outs:
        shapes["dfeat"] = (B, T, D)
    o = ctx.outs(init=init, **shapes)
    ctx.call("aim_head_bwd", d["dscore"], d["pooled"], d["drop"], d["W"], o.get("dW"), o.get("db"), o.get("dfeat"), B, T, D, C)
    return ctx.collect(o)


def head_bwd_idents(ctx, case, inp, got, rec):
    if case.p["outs"] != HEAD_BWD_SUBSETS[0]:
        full, _ = head_bwd_launch(ctx, case, inp, outs=HEAD_BWD_SUBSETS[0])
        rec["ident"]["subset_eq_full"] = all(_bits_eq(got[k], full[k]) for k in got)


KINDS["head_bwd"] = (head_bwd_inputs, head_bwd_expected, head_bwd_emulate, head_bwd_launch, HEAD_BWD_MUTANTS, head_bwd_idents)


# ================================================================== ce_topk ==================================================
CE_FAMILIES = ("unit", "pm80", "spike", "neginf", "ties", "pm100")
TIE_VARIANTS = 8        # (4 | 5 | 6 ties) x (at larger | at smaller indices), an all-equal row, duplicates of the maximum


def _ce_scores(case, g):
    """-> (score [B, C] f32, label [B] int64, all valid)"""
    p, fam = case.p, case.family
    B, C = p["B"], p["C"]
    lab = torch.randint(0, C, (B,), generator=g)
    s = _rn(g, B, C)
    if fam in ("pm80", "pm100"):
        s = torch.where(torch.rand((B, C), generator=g) < 0.5, 1.0, -1.0).float() * float(fam[2:])
    elif fam == "spike":
        s[torch.arange(B), torch.randint(0, C, (B,), generator=g)] += 1e4
    elif fam == "neginf":
        hole = torch.rand((B, C), generator=g) < 0.2
        hole[torch.arange(B), lab] = False
        s[hole] = -INF
    elif fam == "ties":
        s = -1.0 - torch.rand((B, C), generator=g)
        for b in range(B):
            v = b % TIE_VARIANTS
            if C < 16 or v == 6:
                s[b] = 0.25
            elif v == 7:                    # the maximum three times; the label is the middle one
                lab[b] = C // 2
                s[b, [1, C // 2, C - 2]] = 3.0
            else:
                n, larger = 4 + v % 3, v < 3
                lab[b] = 2 if larger else C - 3
                other = torch.arange(3, 3 + n) if larger else torch.arange(C - 3 - n, C - 3)
                s[b, other] = 1.0
                s[b, lab[b]] = 1.0
    return s, lab


def ce_topk_inputs(case):
    p, g = case.p, _gen(case)
    B, C = p["B"], p["C"]
    s, lab = _ce_scores(case, g)
    if p["labels"] == "mix":
        bad = torch.tensor([-100, -1, C, 2 ** 40])
        for i in range(0, B, 2):
            lab[i] = bad[(i // 2) % 4]
        if B == 1:
            lab[0] = -100
    elif p["labels"] == "ignored":
        lab[:] = torch.tensor([-100, -1, C, 2 ** 40])[torch.arange(B) % 4]
    return {"score": s, "label": lab.to(I64)}


def _k2(p):
    return {"1": 1, "5": 5, "C+3": p["C"] + 3}[p["k2"]]


def _ce_valid(inp, C):
    lab = inp["label"]
    valid = (lab >= 0) & (lab < C)
    return valid, torch.where(valid, lab, torch.zeros_like(lab))


def ce_topk_expected(case, inp, got=None):
    p = case.p
    B, C = p["B"], p["C"]
    s = inp["score"].double()
    valid, labc = _ce_valid(inp, C)
    nv = int(valid.sum())
    mx = s.max(1, keepdim=True).values
    d = s - mx
    e = d.exp()
    S = e.sum(1)
    lse = mx[:, 0] + S.log()
    ad = torch.where(torch.isinf(d), torch.zeros_like(d), d.abs())
    r_sum = (e * (8 * u * (1 + ad) + u * ad)).sum(1) / S + (_cdiv(C, 256) + 9) * u + C * FL / S
    e_lse = r_sum + 16 * u * S.log().abs() + u * lse.abs()
    tgt = s[torch.arange(B), labc]
    zero = torch.zeros(B, dtype=F64)
    loss_b = torch.where(valid, lse - tgt, zero)
    e_loss = torch.where(valid, e_lse + u * loss_b.abs(), zero)
    if nv:
        out0, b0 = loss_b.sum() / nv, e_loss.sum() / nv + (B + 1) * u * loss_b.abs().sum() / nv
    else:
        out0, b0 = torch.tensor(NAN, dtype=F64), torch.tensor(0.0, dtype=F64)
    order = np.argsort(inp["score"].numpy(), axis=1, kind="stable")
    k2 = _k2(p)
    hit = torch.zeros((B, 2), dtype=F64)
    for b in range(B):
        if valid[b]:
            hit[b, 0] = float(int(labc[b]) in order[b, -1:])
            hit[b, 1] = float(int(labc[b]) in order[b, -k2:])
    acc = torch.tensor([float(np.float32(hit[:, j].sum().item()) / np.float32(B)) for j in range(2)], dtype=F64)
    ps = torch.stack([loss_b, hit[:, 0], hit[:, 1], valid.double()], 1)
    bps = torch.stack([e_loss, zero, zero, zero], 1)
    out = {"loss": (out0.reshape(1), b0.reshape(1)), "acc": (acc, torch.zeros(2, dtype=F64)), "per_sample": (ps, bps)}
    if p["dscore"]:
        x = s - lse[:, None]
        pr = x.exp()
        ax = torch.where(torch.isinf(x), torch.zeros_like(x), x.abs())
        e_p = pr * (e_lse[:, None] + u * ax + 8 * u * (1 + ax)) + FL
        oh = torch.zeros_like(s)
        oh[torch.arange(B), labc] = 1.0
        n1 = max(nv, 1)
        ds = (pr - oh) / n1
        bd = (e_p + u * (pr - oh).abs()) / n1 + 2 * u * ds.abs()
        out["dscore"] = (torch.where(valid[:, None], ds, torch.zeros_like(ds)), torch.where(valid[:, None], bd, torch.zeros_like(bd)))
    return out


CE_TOPK_MUTANTS = ("mean_over_B", "tie_lt", "k2_unclamped", "no_max_shift", "onehot_next")


def ce_topk_emulate(case, inp, mut=None):
    p = case.p
    B, C = p["B"], p["C"]
    s = inp["score"]
    valid, labc = _ce_valid(inp, C)
    nv = valid.float().sum()
    mx = torch.zeros(B) if mut == "no_max_shift" else s.max(1).values
    tgt = s[torch.arange(B), labc]
    sm = _block256(_fast_exp(s - mx[:, None]), False)
    cidx = torch.arange(C)[None]
    tie = (cidx < labc[:, None]) if mut == "tie_lt" else (cidx > labc[:, None])
    ahead = ((s > tgt[:, None]) | ((s == tgt[:, None]) & tie)).float().sum(1)
    lse = mx + _fast_log(sm)
    k2 = _k2(p)
    kk = float(k2 if mut == "k2_unclamped" else min(k2, C))
    zero = torch.zeros(B)
    ps = torch.stack([torch.where(valid, lse - tgt, zero), (valid & (ahead < 1)).float(), (valid & (ahead < kk)).float(), valid.float()], 1)
    tot = _seq(ps)
    den = torch.tensor(float(B)) if mut == "mean_over_B" else tot[3]
    out = {"loss": (tot[0] / den).reshape(1), "acc": tot[1:3] / torch.tensor(float(B)), "per_sample": ps}
    if p["dscore"]:
        inv = torch.tensor(1.0) / (torch.tensor(float(B)) if mut == "mean_over_B" else nv)
        oh = torch.zeros_like(s)
        oh[torch.arange(B), (labc + 1) % C if mut == "onehot_next" else labc] = 1.0
        ds = (_fast_exp(s - lse[:, None]) - oh) * inv
        out["dscore"] = torch.where(valid[:, None], ds, torch.zeros_like(ds))
    return out


def ce_topk_launch(ctx, case, inp, rows=None):
    p = case.p
    B, C = p["B"], p["C"]
    s, lab = inp["score"], inp["label"]
    if rows is not None:
        s, lab, B = s[rows], lab[rows], len(rows)
    d = ctx.put(score=s, label=lab)
    shapes = {"per_sample": (B, 4), "out3": (3,)}
    if p["dscore"]:
        shapes["dscore"] = (B, C)
    o = ctx.outs(**shapes)
    ctx.call("aim_ce_topk", d["score"], d["label"], o.get("dscore"), o["per_sample"], o["out3"], B, C, _k2(p))
    got, pad = ctx.collect(o)
    o3 = got.pop("out3")
    got["loss"], got["acc"] = o3[:1], o3[1:]
    pad["loss"] = pad["acc"] = pad.pop("out3")
    return got, pad


def ce_topk_idents(ctx, case, inp, got, rec):
    p = case.p
    if p["B"] > 1:
        g1, _ = ce_topk_launch(ctx, case, inp, rows=[1])
        ok = _bits_eq(got["per_sample"][1:2], g1["per_sample"])
        if p["dscore"] and p["labels"] == "valid" and p["B"] in (2, 64):      # n_valid a power of two: the scaling is exact
            big = g1["dscore"].abs() > 2.0 ** -100
            ok = ok and bool(((got["dscore"][1:2] * float(p["B"]))[big] == g1["dscore"][big]).all())
        rec["ident"]["row_alone"] = ok


KINDS["ce_topk"] = (ce_topk_inputs, ce_topk_expected, ce_topk_emulate, ce_topk_launch, CE_TOPK_MUTANTS, ce_topk_idents)


# ================================================================== ce_soft ==================================================
SOFT_LABELS = ("onehot", "twohot", "uniform", "somezero", "allzero")


def ce_soft_inputs(case):
    p, g = case.p, _gen(case)
    B, C = p["B"], p["C"]
    s = _rn(g, B, C) * 3.0
    y = torch.zeros((B, C), dtype=F32)
    a = torch.randint(0, C, (B,), generator=g)
    if p["labels"] in ("onehot", "somezero"):
        y[torch.arange(B), a] = 1.0
        if p["labels"] == "somezero":
            y[::2] = 0.0
    elif p["labels"] == "twohot":
        lam = torch.rand(B, generator=g)
        y[torch.arange(B), a] += lam
        y[torch.arange(B), (a + 1) % C] += 1.0 - lam
    elif p["labels"] == "uniform":
        y[:] = 1.0 / C
    return {"score": s, "label": y, "w": 0.5 + torch.rand(C, generator=g)}


def ce_soft_expected(case, inp, got=None):
    p = case.p
    B, C = p["B"], p["C"]
    s, y = inp["score"].double(), inp["label"].double()
    w = inp["w"].double() if p["weighted"] else torch.ones(C, dtype=F64)
    chain = _cdiv(C, 256) + 8
    mx = s.max(1, keepdim=True).values
    d = s - mx
    e = d.exp()
    S = e.sum(1)
    lse = mx[:, 0] + S.log()
    r_sum = (e * (u * d.abs() + 2 * u)).sum(1) / S + chain * u
    e_lse = r_sum + 2 * u * S.log().abs() + u * lse.abs()
    t = w * y
    term = t * (lse[:, None] - s)
    loss_b = term.sum(1)
    e_loss = t.abs().sum(1) * e_lse + (chain + 3) * u * term.abs().sum(1)
    wy = t.sum(1)
    e_wy = (chain + 1) * u * t.abs().sum(1)
    if p["weighted"]:
        den, e_den = wy.sum(), e_wy.sum() + B * u * wy.abs().sum()
    else:
        den, e_den = torch.tensor(float(B), dtype=F64), torch.tensor(0.0, dtype=F64)
    r_den = e_den / den + u
    out = loss_b.sum() / den
    b_out = (e_loss.sum() + B * u * loss_b.abs().sum()) / den + out.abs() * r_den
    res = {"out": (out.reshape(1), b_out.reshape(1)), "per_sample": (torch.stack([loss_b, wy], 1), torch.stack([e_loss, e_wy], 1))}
    if p["dscore"]:
        x = s - lse[:, None]
        pr = x.exp()
        e_p = pr * (e_lse[:, None] + u * x.abs() + 2 * u) + FL
        num = pr * wy[:, None] - t
        e_num = wy[:, None].abs() * e_p + pr * e_wy[:, None] + u * (pr * wy[:, None]).abs() + u * t.abs() + u * num.abs()
        ds = num / den
        res["dscore"] = (ds, e_num / den + ds.abs() * r_den)
    if not bool(torch.isfinite(out)):                  # 0 / 0: NaN expected, nothing to bound
        res = {k: (torch.full_like(v, NAN) if k != "per_sample" else v, b.nan_to_num(0.0)) for k, (v, b) in res.items()}
    return res


CE_SOFT_MUTANTS = ("den_B_weighted", "no_wy", "w_next")


def ce_soft_emulate(case, inp, mut=None):
    p = case.p
    B, C = p["B"], p["C"]
    s, y = inp["score"], inp["label"]
    w = (inp["w"].roll(-1) if mut == "w_next" else inp["w"]) if p["weighted"] else torch.ones(C)
    mx = s.max(1).values
    sm = _block256(torch.exp(s - mx[:, None]), True)
    t = w * y
    wy = _block256(t, True)
    lse = mx + torch.log(sm)
    loss = _block256(t * (lse[:, None] - s), True)
    den = _seq(wy) if p["weighted"] and mut != "den_B_weighted" else torch.tensor(float(B))
    out = {"out": (_seq(loss) / den).reshape(1), "per_sample": torch.stack([loss, wy], 1)}
    if p["dscore"]:
        pr = torch.exp(s - lse[:, None])
        out["dscore"] = ((pr if mut == "no_wy" else pr * wy[:, None]) - t) / den
    return out


def ce_soft_launch(ctx, case, inp, rows=None, w="case"):
    p = case.p
    B, C = p["B"], p["C"]
    s, y = inp["score"], inp["label"]
    if rows is not None:
        s, y, B = s[rows], y[rows], len(rows)
    wt = inp["w"] if p["weighted"] else None
    if w == "ones":
        wt = torch.ones(C, dtype=F32)
    d = ctx.put(score=s, label=y, w=wt)
    shapes = {"per_sample": (B, 2), "out": (1,)}
    if p["dscore"]:
        shapes["dscore"] = (B, C)
    o = ctx.outs(**shapes)
    ctx.call("aim_ce_soft", d["score"], d["label"], d["w"], o.get("dscore"), o["per_sample"], o["out"], B, C)
    return ctx.collect(o)


def ce_soft_idents(ctx, case, inp, got, rec):
    p = case.p
    if p["B"] > 1:
        g1, _ = ce_soft_launch(ctx, case, inp, rows=[1])
        rec["ident"]["row_alone"] = _bits_eq(got["per_sample"][1:2], g1["per_sample"])
    if not p["weighted"] and p["labels"] == "onehot":           # wy = 1 per row: both denominators are B
        g1, _ = ce_soft_launch(ctx, case, inp, w="ones")
        rec["ident"]["null_eq_ones"] = all(_bits_eq(got[k], g1[k]) for k in got)


KINDS["ce_soft"] = (ce_soft_inputs, ce_soft_expected, ce_soft_emulate, ce_soft_launch, CE_SOFT_MUTANTS, ce_soft_idents)


# ================================================================== qk_cross / qk_border =====================================
SCALE = 0.125


def _qkv(g, BT, N, D, q_only):
    """[BT, N, 3D] bf16; the parts the kernel must not read are NaN"""
    t = _rn(g, BT, N, 3 * D).to(BF16)
    t[..., (D if q_only else 2 * D):] = NAN
    return t


def qk_cross_inputs(case):
    p, g = case.p, _gen(case)
    return {"qkv": _qkv(g, p["BT"], p["N"], p["D"], True), "kx": _rn(g, p["BT"], p["D"]).to(BF16)}


def _cross64(inp, D, chain):
    q, kx = inp["qkv"][..., :D].double(), inp["kx"].double()
    ss = SCALE * torch.einsum("bnd,bd->bn", q, kx)
    return ss, (chain + 1) * u * SCALE * torch.einsum("bnd,bd->bn", q.abs(), kx.abs())


def qk_cross_expected(case, inp, got=None):
    D = case.p["D"]
    return {"ss": _cross64(inp, D, 8 * _cdiv(D, 512) + 6)}


QK_CROSS_MUTANTS = ("no_scale", "kx_next")


def qk_cross_emulate(case, inp, mut=None):
    D = case.p["D"]
    kx = inp["kx"].roll(-1, 0) if mut == "kx_next" else inp["kx"]
    acc = _lanes(inp["qkv"][..., :D].float() * kx.float()[:, None, :], 8, 512)
    return {"ss": acc if mut == "no_scale" else acc * SCALE}


def _put_kx(ctx, kx, ldkx):
    """kx rows at stride ldkx inside a NaN buffer"""
    BT, D = kx.shape
    buf = torch.full((BT * ldkx + 8,), NAN, dtype=BF16, device=ctx.dev)
    buf[:BT * ldkx].view(BT, ldkx)[:, :D] = kx.to(ctx.dev)
    return buf


def qk_cross_launch(ctx, case, inp, rows=None):
    p = case.p
    BT, N, D = p["BT"], p["N"], p["D"]
    qkv, kx = inp["qkv"], inp["kx"]
    if rows is not None:
        qkv, kx, BT = qkv[rows], kx[rows], len(rows)
    d = ctx.put(qkv=qkv)
    kxb = _put_kx(ctx, kx, p["ldkx"])
    o = ctx.outs(ss=(BT, N))
    ctx.call("aim_qk_cross", d["qkv"], kxb, p["ldkx"], o["ss"], BT, N, D, SCALE)
    return ctx.collect(o)


def _row_alone(launch):
    def idents(ctx, case, inp, got, rec):
        if case.p["BT"] > 1:
            g1, _ = launch(ctx, case, inp, rows=[1])
            rec["ident"]["row_alone"] = all(_bits_eq(got[k][1:2], g1[k]) for k in got)
    return idents


KINDS["qk_cross"] = (qk_cross_inputs, qk_cross_expected, qk_cross_emulate, qk_cross_launch, QK_CROSS_MUTANTS, _row_alone(qk_cross_launch))


def qk_border_inputs(case):
    """q_{N-1} lies along k_{N-1}: the corner score (8) weighs in both pairs, so that a pass which counts it wrongly shows"""
    p, g = case.p, _gen(case)
    N, D = p["N"], p["D"]
    qkv = _qkv(g, p["BT"], N, D, False)
    k = qkv[:, N - 1, D:2 * D].float()
    qkv[:, N - 1, :D] = (k * (8.0 / (SCALE * k.pow(2).sum(1, keepdim=True)))).to(BF16)
    return {"qkv": qkv, "kx": _rn(g, p["BT"], D).to(BF16)}


def _pair64(sc, e_s):
    """float64 scores [R, cnt] and their bounds -> (max, bound), (log-sum-exp, bound)"""
    cnt = sc.shape[1]
    mx = sc.max(1, keepdim=True).values
    d = sc - mx
    e = d.exp()
    S = e.sum(1)
    em = e_s.max(1).values
    return (mx[:, 0], em), (mx[:, 0] + S.log(), em + (e * (u * d.abs() + 2 * u)).sum(1) / S + (_cdiv(cnt, 256) + 9) * u + cnt * FL / S)


def _border_scores(inp, D, N):
    q, k = inp["qkv"][..., :D].double(), inp["qkv"][..., D:2 * D].double()
    a = SCALE * torch.einsum("bnd,bd->bn", q[:, :N - 1], k[:, N - 1])
    ea = 23 * u * SCALE * torch.einsum("bnd,bd->bn", q[:, :N - 1].abs(), k[:, N - 1].abs())
    b = SCALE * torch.einsum("bd,bnd->bn", q[:, N - 1], k)
    eb = 23 * u * SCALE * torch.einsum("bd,bnd->bn", q[:, N - 1].abs(), k.abs())
    return (a, ea), (b, eb)


def qk_border_expected(case, inp, got=None):
    p = case.p
    D, N = p["D"], p["N"]
    (a, ea), (b, eb) = _border_scores(inp, D, N)
    (ma, lsa), (mb, lsb) = _pair64(a, ea), _pair64(b, eb)
    st = lambda x, y: torch.stack([x, y], 1)                    # noqa: E731
    return {"ss": _cross64(inp, D, 22), "max": (st(ma[0], mb[0]), st(ma[1], mb[1])), "lse": (st(lsa[0], lsb[0]), st(lsa[1], lsb[1]))}


QK_BORDER_MUTANTS = ("no_scale", "kx_next", "corner_both", "corner_neither", "slot_swapped")


def _pair32(sc):
    mx = sc.max(1).values
    sm = _block256(torch.exp(sc - mx[:, None]), False)
    return torch.stack([mx, sm], 1)


def _border_lanes(x, v):
    """sum over D of x v with 16 fma per lane (c*512 + lane*8 + e), the butterfly"""
    return _lanes(x.float() * v.float(), 8, 512)       # (bf16 products are exact: an fma is the product and the addition)


def qk_border_emulate(case, inp, mut=None):
    p = case.p
    D, N = p["D"], p["N"]
    sc = 1.0 if mut == "no_scale" else SCALE
    q, k = inp["qkv"][..., :D], inp["qkv"][..., D:2 * D]
    kx = inp["kx"].roll(-1, 0) if mut == "kx_next" else inp["kx"]
    ss = _border_lanes(q, kx[:, None, :]) * sc
    a = _border_lanes(q, k[:, N - 1:N]) * sc
    b = _border_lanes(k, q[:, N - 1:N]) * sc
    na = N if mut == "corner_both" else N - 1
    nb = N - 1 if mut == "corner_neither" else N
    pa = _pair32(a[:, :na])
    pb = _pair32(b[:, :nb]) if nb else torch.tensor([[-INF, 0.0]]).expand(p["BT"], 2)
    if mut == "slot_swapped":
        pa, pb = pb, pa
    return _border_keys(ss, torch.stack([pa, pb], 1))


def _border_keys(ss, pairs):
    """pairs [BT, 2, 2] f32 -> the compared outputs (max + log(sum) in float64)"""
    pd = pairs.double()
    return {"ss": ss, "max": pairs[..., 0], "lse": pd[..., 0] + pd[..., 1].log()}


def qk_border_launch(ctx, case, inp, rows=None):
    p = case.p
    BT, N, D, s0, ns = p["BT"], p["N"], p["D"], p["slot0"], p["nslots"]
    qkv, kx = inp["qkv"], inp["kx"]
    if rows is not None:
        qkv, kx, BT = qkv[rows], kx[rows], len(rows)
    d = ctx.put(qkv=qkv)
    kxb = _put_kx(ctx, kx, p["ldkx"])
    o = ctx.outs(ss=(BT, N), part=(BT, ns, 2))
    ctx.call("aim_qk_border", d["qkv"], kxb, p["ldkx"], o["ss"], o["part"], s0, ns, BT, N, D, SCALE)
    got, pad = ctx.collect(o)
    part = got.pop("part")
    rest = part.clone()
    rest[:, s0:s0 + 2] = NAN
    ok = pad.pop("part") and bool(torch.isnan(rest).all())           # the other slots stay NaN
    got = _border_keys(got["ss"], part[:, s0:s0 + 2])
    pad["max"] = pad["lse"] = ok
    return got, pad


KINDS["qk_border"] = (qk_border_inputs, qk_border_expected, qk_border_emulate, qk_border_launch, QK_BORDER_MUTANTS, _row_alone(qk_border_launch))


# ================================================================== lambda / lambda_partials =================================
LAM_FAMILIES = ("unit", "cw_dom", "ow_dom", "near200")


def _synth_partials(g, centre, nt, hole_from=2):
    """per-tile (max, sum exp) pairs of float64 scores around centre [BT]; every third slot from `hole_from` is (-inf, 0)"""
    BT = centre.shape[0]
    sc = centre.double()[:, None, None] + torch.randn((BT, nt, 6), generator=g, dtype=F64)
    mx = sc.max(2).values
    part = torch.stack([mx, (sc - mx[..., None]).exp().sum(2)], 2).float()
    part[:, hole_from::3, 0] = -INF
    part[:, hole_from::3, 1] = 0.0
    return part


def _centre(fam, ss):
    if fam == "cw_dom":
        return ss.min(1).values - 30.0
    if fam == "ow_dom":
        return ss.max(1).values + 110.0
    return ss.mean(1)


def lambda_inputs(case):
    p, g, fam = case.p, _gen(case), case.family
    BT, N, D, nt = p["BT"], p["N"], p["D"], p["ntiles"]
    inp = {}
    if p["form"] == "ss":
        ss = _rn(g, BT, N) * 2.0 + (200.0 if fam == "near200" else 0.0)
        inp["ss"] = ss
    else:
        kx = _rn(g, BT, D).to(BF16)
        qkv = _qkv(g, BT, N, D, True)
        if fam in ("cw_dom", "near200"):         # kx aligned with every query: q_i = a_i kx
            tgt = (200.0 if fam == "near200" else 20.0) + _rn(g, BT, N)
            a = tgt / (SCALE * kx.float().pow(2).sum(1, keepdim=True))
            qkv[..., :D] = (a[..., None] * kx.float()[:, None, :]).to(BF16)
        inp["qkv"], inp["kx"] = qkv, kx
        ss = _cross64(inp, D, 0)[0].float()
    inp["partials"] = _synth_partials(g, _centre(fam, ss), nt)
    return inp


def _lam64(ss, e_ss, part, chain_c, chain_o):
    p0, p1 = part[..., 0].double(), part[..., 1].double()
    N, nt = ss.shape[1], p0.shape[1]
    M = torch.maximum(ss.max(1).values, p0.max(1).values)[:, None]
    ec = (ss - M).exp()
    live = p0 > -INF
    zero = torch.zeros_like(p0)
    eo = torch.where(live, p1 * (p0 - M).exp(), zero)
    cw, ow = ec.sum(1), eo.sum(1)
    a_c = (ec * (e_ss + u * (ss - M).abs() + 2 * u)).sum(1) + chain_c * u * cw + N * FL
    a_o = (eo * (u * torch.where(live, (p0 - M).abs(), zero) + 3 * u)).sum(1) + chain_o * u * ow + nt * FL * p1.max(1).values
    lam = cw / (cw + ow)
    e_lam = (ow * a_c + cw * a_o) / (cw + ow) ** 2 + 2 * u * lam
    return lam, e_lam, 1.0 - lam, e_lam + u * (1.0 - lam).abs()


def lambda_expected(case, inp, got=None):
    p = case.p
    if p["form"] == "ss":
        ss, e_ss = inp["ss"].double(), torch.zeros(inp["ss"].shape, dtype=F64)
    else:
        ss, e_ss = _cross64(inp, p["D"], 4 * _cdiv(p["D"], 256) + 6)
    lam, e_lam, oml, e_oml = _lam64(ss, e_ss, inp["partials"], _cdiv(p["N"], 256) + 9, _cdiv(p["ntiles"], 256) + 9)
    out = {"lam": (lam, e_lam)}
    if p["oml"]:
        out["oml"] = (oml, e_oml)
    return out


LAMBDA_MUTANTS = ("diff_max", "neginf_nan", "ntiles_256", "swap")


def _lam32(ss, part, mut, block):
    p0, p1 = part[..., 0], part[..., 1]
    mc = ss.max(1).values
    mo = p0.max(1).values
    mx = torch.maximum(mc, mo)
    if mut != "diff_max":
        mc = mo = mx
    live = p0 > -INF
    ec = torch.exp(ss - mc[:, None])
    eo = torch.where(live, p1 * torch.exp(torch.where(live, p0, torch.zeros_like(p0)) - mo[:, None]), torch.zeros_like(p0))
    if block:
        c, o = _block256(ec, False), _block256(eo, False)
    else:
        c, o = _seq(ec.T.contiguous()), _seq(eo.T.contiguous())
    lam = c / (c + o)
    if mut == "neginf_nan":
        lam = torch.where((~live).any(1), torch.full_like(lam, NAN), lam)
    oml = 1.0 - lam
    return (oml, lam) if mut == "swap" else (lam, oml)


def lambda_emulate(case, inp, mut=None):
    p = case.p
    if p["form"] == "ss":
        ss = inp["ss"]
    else:
        D = p["D"]
        pr = inp["qkv"][..., :D].float() * inp["kx"].float()[:, None, :]
        n = _cdiv(D, 256)
        pad = torch.zeros(pr.shape[:-1] + (n * 256,), dtype=F32)
        pad[..., :D] = pr
        v = pad.view(pr.shape[:-1] + (n, 64, 4))
        acc = torch.zeros(pr.shape[:-1] + (64,), dtype=F32)
        for i in range(n):
            acc = acc + (((v[..., i, :, 0] + v[..., i, :, 1]) + v[..., i, :, 2]) + v[..., i, :, 3])
        ss = _butterfly(acc) * SCALE
    part = inp["partials"][:, :256] if mut == "ntiles_256" else inp["partials"]
    lam, oml = _lam32(ss, part, mut, True)
    return {"lam": lam, "oml": oml} if p["oml"] else {"lam": lam}


def lambda_launch(ctx, case, inp, rows=None):
    p = case.p
    BT, N, D, nt = p["BT"], p["N"], p["D"], p["ntiles"]
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    BT = BT if rows is None else len(rows)
    d = ctx.put(partials=sel(inp["partials"]), ss=sel(inp["ss"]) if p["form"] == "ss" else None,
                qkv=sel(inp["qkv"]) if p["form"] == "qk" else None)
    kxb = _put_kx(ctx, sel(inp["kx"]), p["ldkx"]) if p["form"] == "qk" else None
    shapes = {"lam": (BT,)}
    if p["oml"]:
        shapes["oml"] = (BT,)
    o = ctx.outs(**shapes)
    ctx.call("aim_lambda", d["qkv"], kxb, p.get("ldkx", 0), d["ss"], d["partials"], nt, o["lam"], o.get("oml"), BT, N, D, SCALE)
    return ctx.collect(o)


KINDS["lambda"] = (lambda_inputs, lambda_expected, lambda_emulate, lambda_launch, LAMBDA_MUTANTS, _row_alone(lambda_launch))


def lam_part_inputs(case):
    p, g, fam = case.p, _gen(case), case.family
    BT = p["BT"]
    base = _rn(g, BT, 1) * 2.0 + (200.0 if fam == "near200" else 0.0)
    cw = _synth_partials(g, base[:, 0], 8, hole_from=1)
    ow = _synth_partials(g, _centre(fam, cw[..., 0][:, ::3]), 8)
    return {"partials": torch.cat([ow, cw], 1)}


def lam_part_expected(case, inp, got=None):
    part = inp["partials"].double()
    p0, p1 = part[..., 0], part[..., 1]
    M = p0.max(1).values[:, None]
    live = p0 > -INF
    zero = torch.zeros_like(p0)
    e = torch.where(live, p1 * (p0 - M).exp(), zero)
    a = e * (u * torch.where(live, (p0 - M).abs(), zero) + 3 * u)
    o, c = e[:, :8].sum(1), e[:, 8:].sum(1)
    fl = 8 * FL * p1.max(1).values
    a_o, a_c = a[:, :8].sum(1) + 8 * u * o + fl, a[:, 8:].sum(1) + 8 * u * c + fl
    lam = c / (c + o)
    e_lam = (o * a_c + c * a_o) / (c + o) ** 2 + 2 * u * lam
    out = {"lam": (lam, e_lam)}
    if case.p["oml"]:
        out["oml"] = (1.0 - lam, e_lam + u * (1.0 - lam).abs())
    return out


LAM_PART_MUTANTS = ("diff_max", "neginf_nan", "swap")


def lam_part_emulate(case, inp, mut=None):
    part = inp["partials"]
    p0, p1 = part[..., 0], part[..., 1]
    mo, mc = p0[:, :8].max(1).values, p0[:, 8:].max(1).values
    mx = torch.maximum(mo, mc)
    if mut != "diff_max":
        mo = mc = mx
    live = p0 > -INF
    safe = torch.where(live, p0, torch.zeros_like(p0))
    e = torch.where(live, p1 * torch.exp(safe - torch.cat([mo[:, None].expand(-1, 8), mc[:, None].expand(-1, 8)], 1)), torch.zeros_like(p0))
    o, c = _seq(e[:, :8].T.contiguous()), _seq(e[:, 8:].T.contiguous())
    lam = c / (c + o)
    if mut == "neginf_nan":
        lam = torch.full_like(lam, NAN)
    oml = 1.0 - lam
    if mut == "swap":
        lam, oml = oml, lam
    return {"lam": lam, "oml": oml} if case.p["oml"] else {"lam": lam}


def lam_part_launch(ctx, case, inp, rows=None):
    p = case.p
    part = inp["partials"] if rows is None else inp["partials"][rows]
    BT = part.shape[0]
    d = ctx.put(partials=part)
    shapes = {"lam": (BT,)}
    if p["oml"]:
        shapes["oml"] = (BT,)
    o = ctx.outs(**shapes)
    ctx.call("aim_lambda_partials", d["partials"], o["lam"], o.get("oml"), BT)
    return ctx.collect(o)


KINDS["lam_part"] = (lam_part_inputs, lam_part_expected, lam_part_emulate, lam_part_launch, LAM_PART_MUTANTS, _row_alone(lam_part_launch))


# ================================================================== patchify =================================================
IN_DT = {0: F32, 1: U8T, 2: BF16}
PATCH_B, PATCH_T = 2, 3
MEAN3 = torch.tensor([123.675, 116.28, 103.53], dtype=F32)
STD3 = torch.tensor([58.395, 57.12, 57.375], dtype=F32)


def patchify_inputs(case):
    p, g = case.p, _gen(case)
    shape = (PATCH_B, 3, PATCH_T, p["H"], p["W"])
    if p["in_dtype"] == 1:
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(U8T)
        x.view(-1)[0::7] = 255
        x.view(-1)[3::11] = 0
    else:
        x = (_rn(g, *shape) * (60.0 if p["norm"] else 1.0) + (110.0 if p["norm"] else 0.0)).to(IN_DT[p["in_dtype"]])
    return {"x": x}


def _patch_gather(v, p, Kp, mut=None, pad=0.0):
    """v [B, 3, T, H, W] (any dtype) -> [rows, Kp]"""
    B, _, T, H, W = v.shape
    Gy, G, K = H // p, W // p, 3 * p * p
    if mut == "h_stride":               # the row stride taken from H: flat index ((.. * H + y) * H + x), wrapped into the buffer
        b, c, t, y, x = torch.meshgrid(*[torch.arange(n) for n in (B, 3, T, H, W)], indexing="ij")
        v = v.reshape(-1)[((((b * 3 + c) * T + t) * H + y) * H + x) % v.numel()]
    t = v.view(B, 3, T, Gy, p, G, p)
    t = t.permute(0, 2, 3, 5, 4, 1, 6) if mut == "swap_c_py" else t.permute(0, 2, 3, 5, 1, 4, 6)
    out = torch.full((B * T * Gy * G, Kp), pad, dtype=v.dtype)
    out[:, :K] = t.reshape(-1, K)
    return out


def _patch_values(case, inp, mut=None):
    p = case.p
    x = inp["x"]
    v = (x.view(torch.int8) if mut == "u8_signed" and x.dtype == U8T else x).float()
    if p["norm"]:
        v = (v - MEAN3.view(1, 3, 1, 1, 1)) / STD3.view(1, 3, 1, 1, 1)
    if mut == "truncate":
        return (v.view(torch.int32) & -65536).view(F32).to(BF16)
    return v.to(BF16)


def patchify_expected(case, inp, got=None):
    ref = _patch_gather(_patch_values(case, inp), case.p["p"], case.p["Kp"])
    return {"A": (ref.double(), torch.zeros(ref.shape, dtype=F64))}


PATCHIFY_MUTANTS = ("swap_c_py", "h_stride", "u8_signed", "truncate", "pad_unwritten")


def patchify_emulate(case, inp, mut=None):
    return {"A": _patch_gather(_patch_values(case, inp, mut), case.p["p"], case.p["Kp"], mut, NAN if mut == "pad_unwritten" else 0.0)}


def patchify_fast_path(p):
    """csrc/embed_misc.hip::patchify_kernel: the 8-pixel loads are taken by the threads with k0 + 8 <= K of such a case"""
    return p["p"] % 8 == 0 and p["W"] % 8 == 0


def patchify_launch(ctx, case, inp, offset=0):
    p = case.p
    x = inp["x"]
    rows = PATCH_B * PATCH_T * (p["H"] // p["p"]) * (p["W"] // p["p"])
    buf = torch.zeros(x.numel() + offset + 16, dtype=x.dtype, device=ctx.dev)
    if x.dtype != U8T:
        buf.fill_(NAN)
    buf[offset:offset + x.numel()] = x.reshape(-1).to(ctx.dev)
    ptr = buf.data_ptr() + offset * x.element_size()
    d = ctx.put(mean=MEAN3 if p["norm"] else None, std=STD3 if p["norm"] else None)
    o = ctx.outs(dtype=BF16, A=(rows, p["Kp"]))
    ctx.call("aim_patchify", ptr, p["in_dtype"], d["mean"], d["std"], o["A"], PATCH_B, PATCH_T, p["H"], p["W"], p["p"], p["Kp"])
    return ctx.collect(o)


def patchify_idents(ctx, case, inp, got, rec):
    rec["ident"]["exact_bits"] = _bits_eq(got["A"], patchify_expected(case, inp)["A"][0].to(BF16))
    if patchify_fast_path(case.p):
        g1, _ = patchify_launch(ctx, case, inp, offset=1)
        rec["ident"]["fast_eq_scalar"] = _bits_eq(got["A"], g1["A"])


KINDS["patchify"] = (patchify_inputs, patchify_expected, patchify_emulate, patchify_launch, PATCHIFY_MUTANTS, patchify_idents)


# ================================================================== adamw ====================================================
ADAM_FAMILIES = ("unit", "g0", "g0v0", "g1e-25", "g1e20")
LR = 3e-4


def adamw_inputs(case):
    p, g, fam = case.p, _gen(case), case.family
    n = p["n"]
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    gr = {"unit": _rn(g, n), "g0": torch.zeros(n), "g0v0": torch.zeros(n), "g1e-25": 1e-25 * sign, "g1e20": 1e20 * sign}[fam]
    m = _rn(g, n) * 0.1
    m = torch.where(m.abs() < 1e-3, torch.full_like(m, 0.05), m)
    v = torch.zeros(n) if fam == "g0v0" else torch.rand(n, generator=g) * 0.01 + 1e-4
    return {"p": _rn(g, n), "g": gr.float(), "m": m.float(), "v": v.float()}


def _hyp(p):
    f = lambda x: float(torch.tensor(x, dtype=F32))             # noqa: E731
    return {"lr": f(LR), "b1": f(p["betas"][0]), "b2": f(p["betas"][1]), "eps": f(p["betas"][2]), "wd": f(p["wd"]), "gs": f(p["gs"])}


def _over(t):
    return torch.where(t.abs() > F32MAX, torch.sign(t) * INF, t)


def adamw_expected(case, inp, got=None):
    p, h = case.p, _hyp(case.p)
    s = p["step"]
    P, G, M, V = (inp[k].double() for k in ("p", "g", "m", "v"))
    bc1, bc2 = 1.0 - h["b1"] ** s, 1.0 - h["b2"] ** s
    r_bc1 = 2 * u * h["b1"] ** s / bc1 + u
    r_bc2s = (2 * u * h["b2"] ** s / bc2 + u) / 2 + u
    g1 = G * h["gs"]
    m1 = (1 - h["b1"]) * g1 + h["b1"] * M
    e_m = u * ((h["b1"] * M).abs() + m1.abs() + (1 - h["b1"]) * g1.abs()) + FL
    g2 = _over((1 - h["b2"]) * g1 * g1)
    v1 = _over(h["b2"] * V + g2)
    e_v = u * (4 * g2 + v1.abs()) + FL
    root = v1.sqrt() / math.sqrt(bc2)
    den = root + h["eps"]
    r_den = ((e_v / (2 * v1)).nan_to_num(0.0, 0.0, 0.0) + 2 * u + r_bc2s) * (root / den).nan_to_num(1.0, 1.0, 1.0) + u
    U = h["lr"] / bc1 * m1 / den
    r_U = r_bc1 + u + (e_m / m1.abs()).nan_to_num(0.0, 0.0, 0.0) + r_den + 2 * u
    c = 1.0 - h["lr"] * h["wd"]
    b_up = U.abs() * r_U + (2 if h["wd"] else 1) * u * P.abs()
    out = {"m": (m1, e_m), "v": (v1, torch.where(torch.isfinite(v1), e_v, torch.zeros_like(v1))), "update": (-U, b_up)}
    if got is not None:
        got["update"] = got.pop("p").double() - P * c
    return out


ADAMW_MUTANTS = ("eps_inside", "bc_step_m1", "l2_decay", "gs_not_squared", "tail_skipped")


def adamw_emulate(case, inp, mut=None):
    p, h = case.p, _hyp(case.p)
    t = lambda x: torch.tensor(x, dtype=F32)                    # noqa: E731
    s = p["step"] - 1 if mut == "bc_step_m1" else p["step"]
    lr, b1, b2, eps, wd, gs = (t(h[k]) for k in ("lr", "b1", "b2", "eps", "wd", "gs"))
    bc1 = 1.0 - torch.pow(b1, t(float(s)))
    bc2 = 1.0 - torch.pow(b2, t(float(s)))
    bc2s = bc2.sqrt()
    P, G, M, V = inp["p"], inp["g"], inp["m"], inp["v"]
    c = t(1.0) if mut == "l2_decay" else _fma(-lr, wd, t(1.0))
    g1 = G * gs
    if mut == "l2_decay":
        g1 = g1 + wd * P
    m1 = _fma(1.0 - b1, g1, b1 * M)
    sq = (1.0 - b2) * g1 * (G if mut == "gs_not_squared" else g1)
    v1 = _fma(b2, V, sq)
    den = (v1 / bc2 + eps).sqrt() if mut == "eps_inside" else v1.sqrt() / bc2s + eps
    p1 = _fma(c, P, -((lr / bc1) * m1 / den))
    if mut == "tail_skipped":
        k = p["n"] - p["n"] % 4
        p1[k:], m1[k:], v1[k:] = P[k:], M[k:], V[k:]
    return {"p": p1, "m": m1, "v": v1}


def adamw_launch(ctx, case, inp, n=None):
    p, h = case.p, _hyp(case.p)
    n = p["n"] if n is None else n
    d = ctx.put(g=inp["g"][:n])
    o = ctx.outs(init={k: inp[k][:n] for k in ("p", "m", "v")}, p=(n,), m=(n,), v=(n,))
    ctx.call("aim_adamw_flat", o["p"], d["g"], o["m"], o["v"], n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], p["step"], h["gs"])
    return ctx.collect(o)


def adamw_idents(ctx, case, inp, got, rec):
    wide = adamw_inputs(Case("tail", "adamw", dict(case.p, n=8), case.family, case.seed))
    a, _ = adamw_launch(ctx, case, wide, n=7)
    b, _ = adamw_launch(ctx, case, wide, n=8)
    rec["ident"]["tail_eq_vector"] = all(_bits_eq(a[k], b[k][:7]) for k in a)


KINDS["adamw"] = (adamw_inputs, adamw_expected, adamw_emulate, adamw_launch, ADAMW_MUTANTS, adamw_idents)


# ================================================================== the catalogue ============================================
HEAD_B, HEAD_T = (1, 3), (1, 2, 8)
HEAD_D = (4, 63, 64, 65, 255, 256, 257, 768)
HEAD_FWD_C = (1, 3, 4, 5, 31, 32, 33, 65, 400)
HEAD_BWD_C = (1, 3, 4, 5, 255, 256, 257, 400)
HEAD_FAMILIES = ("unit", "frame1e4", "equal")
CE_B = (1, 2, 64, 257)
CE_C = (1, 2, 5, 6, 255, 256, 257, 400, 1000)
CE_K2 = ("1", "5", "C+3")
CE_LABELS = ("valid", "mix", "ignored")
QKC_N, QKC_D = (1, 2, 3, 4, 5, 197), (8, 64, 504, 512, 520, 768, 1024)
LAM_N, LAM_D = (1, 2, 255, 256, 257, 320), (4, 252, 256, 260, 768)
LAM_NT = (1, 4, 9, 10, 255, 256, 257)
BORDER_N = (2, 9, 33, 257, 320)
PART_BT = (1, 63, 64, 65)
PATCH_GEOMS = ((8, 16, 24, 192), (8, 16, 16, 200), (16, 32, 48, 768), (16, 32, 32, 832), (14, 28, 42, 592), (14, 28, 28, 640),
               (12, 24, 36, 432), (4, 8, 12, 48), (4, 8, 8, 64))
ADAM_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099)
ADAM_STEP = (1, 2, 1000, 100000)
ADAM_BETAS = ((0.9, 0.999, 1e-8), (0.8, 0.95, 1e-6))


def cases():
    out = []

    def add(kind, name, p, family="unit"):
        out.append(Case(f"{kind}/{name}", kind, p, family, len(out)))

    for i in range(36):
        p = dict(B=HEAD_B[(i // 3) % 2], T=HEAD_T[(i // 2) % 3], D=HEAD_D[i % 8], C=HEAD_FWD_C[i % 9], drop=bool(i % 2), bias=bool((i // 2) % 2))
        fam = HEAD_FAMILIES[(i // 4) % 3]
        add("head_fwd", f"B{p['B']}T{p['T']}D{p['D']}C{p['C']}d{int(p['drop'])}b{int(p['bias'])}-{fam}", p, fam)
    add("head_fwd", "limit-D16384C5", dict(B=1, T=2, D=16384, C=5, drop=True, bias=True))
    for i in range(40):
        p = dict(B=HEAD_B[(i // 3) % 2], T=HEAD_T[(i // 2) % 3], D=HEAD_D[i % 8], C=HEAD_BWD_C[(i // 5) % 8], outs=HEAD_BWD_SUBSETS[i % 5],
                 drop=bool((i // 5) % 2))
        add("head_bwd", f"B{p['B']}T{p['T']}D{p['D']}C{p['C']}d{int(p['drop'])}-{'+'.join(p['outs'])}", p)
    add("head_bwd", "limit-C16128D8", dict(B=3, T=2, D=8, C=16128, outs=HEAD_BWD_SUBSETS[0], drop=True))
    for i in range(45):
        p = dict(B=CE_B[i % 4], C=CE_C[i % 9], k2=CE_K2[(i // 2) % 3], dscore=bool((i // 3) % 2), labels=CE_LABELS[(i // 5) % 3])
        fam = CE_FAMILIES[i % 6]
        add("ce_topk", f"B{p['B']}C{p['C']}k{p['k2']}g{int(p['dscore'])}-{p['labels']}-{fam}", p, fam)
    for j, (B, C, k2, lab, fam) in enumerate(((64, 255, "5", "valid", "ties"), (257, 400, "5", "valid", "ties"), (64, 256, "1", "mix", "ties"),
                                              (64, 1000, "5", "valid", "pm80"), (64, 1000, "5", "valid", "pm100"), (2, 6, "C+3", "valid", "unit"), (64, 5, "C+3", "mix", "unit"),
                                              (64, 400, "5", "valid", "unit"), (2, 257, "5", "valid", "neginf"))):
        add("ce_topk", f"x{j}-B{B}C{C}k{k2}-{lab}-{fam}", dict(B=B, C=C, k2=k2, dscore=True, labels=lab), fam)
    for i in range(40):
        p = dict(B=CE_B[i % 4], C=CE_C[i % 9], weighted=bool((i // 2) % 2), dscore=bool((i // 3) % 2), labels=SOFT_LABELS[i % 5])
        add("ce_soft", f"B{p['B']}C{p['C']}w{int(p['weighted'])}g{int(p['dscore'])}-{p['labels']}", p)
    for j, (B, w, lab) in enumerate(((64, False, "onehot"), (2, True, "allzero"), (64, True, "somezero"), (64, False, "somezero"), (2, True, "twohot"))):
        add("ce_soft", f"x{j}-B{B}C400w{int(w)}-{lab}", dict(B=B, C=400, weighted=w, dscore=True, labels=lab))
    for i in range(14):
        D = QKC_D[i % 7]
        p = dict(BT=(1, 3)[(i // 2) % 2], N=QKC_N[i % 6], D=D, ldkx=D + 8 * (i % 2))
        add("qk_cross", f"BT{p['BT']}N{p['N']}D{D}ld{p['ldkx']}", p)
    for i in range(10):
        D = (512, 1024)[i % 2]
        s0, ns = ((0, 2), (8, 10))[(i // 2) % 2]
        p = dict(BT=(1, 3)[(i // 3) % 2], N=BORDER_N[i % 5], D=D, ldkx=D + 8 * ((i // 5) % 2), slot0=s0, nslots=ns)
        add("qk_border", f"BT{p['BT']}N{p['N']}D{D}s{s0}of{ns}", p)
    for i in range(42):
        form = ("ss", "qk")[i % 2]
        D = LAM_D[i % 5]
        p = dict(BT=(1, 3)[(i // 2) % 2], N=LAM_N[i % 6], D=D, ntiles=LAM_NT[i % 7], form=form, oml=bool((i // 3) % 2))
        if form == "qk":
            p["ldkx"] = D + 4 * ((i // 4) % 2)
        fam = LAM_FAMILIES[(i // 2) % 4]
        add("lambda", f"{form}-BT{p['BT']}N{p['N']}D{D}nt{p['ntiles']}o{int(p['oml'])}-{fam}", p, fam)
    for i in range(8):
        p = dict(BT=PART_BT[i % 4], oml=bool((i // 4) % 2))
        fam = LAM_FAMILIES[(i + i // 4) % 4]
        add("lam_part", f"BT{p['BT']}o{int(p['oml'])}-{fam}", p, fam)
    for pp, H, W, Kp in PATCH_GEOMS:
        for dt in (0, 1, 2):
            for norm in (False, True):
                add("patchify", f"p{pp}H{H}W{W}Kp{Kp}t{dt}n{int(norm)}", dict(p=pp, H=H, W=W, Kp=Kp, in_dtype=dt, norm=norm))
    for i in range(45):
        p = dict(n=ADAM_N[i % 9], step=ADAM_STEP[i % 4], wd=(0.0, 0.05)[(i // 3) % 2], gs=(1.0, 0.125)[(i // 2) % 2], betas=ADAM_BETAS[(i // 7) % 2])
        fam = ADAM_FAMILIES[i % 5]
        add("adamw", f"n{p['n']}s{p['step']}wd{p['wd']}gs{p['gs']}b{p['betas'][0]}-{fam}", p, fam)
    return out


# ================================================================== running ==================================================
def build_inputs(case):
    return KINDS[case.kind][0](case)


def compare(case, inp, got) -> Dict[str, float]:
    got = dict(got)
    exp = KINDS[case.kind][1](case, inp, got)
    assert set(exp) == set(got), (case.name, sorted(exp), sorted(got))
    return {k: eratio(got[k], *exp[k]) for k in exp}


def finite_where_expected(case, inp, got) -> Dict[str, bool]:
    """every element finite wherever the reference is; and what the NaN-expecting cases saw"""
    got = dict(got)
    exp = KINDS[case.kind][1](case, inp, got)
    return {k: bool((torch.isfinite(got[k].double().reshape(exp[k][0].shape)) | ~torch.isfinite(exp[k][0])).all()) for k in exp}


def expects_nan(case, inp) -> bool:
    exp = KINDS[case.kind][1](case, inp, None if case.kind != "adamw" else {"p": inp["p"]})
    return any(bool(torch.isnan(v).any()) for v, _ in exp.values())


def emulate(case, inp, mut=None):
    return KINDS[case.kind][2](case, inp, mut)


def mutants(kind):
    return KINDS[kind][4]


class _Ctx:
    """ctypes calls into libaim_hip.so; inputs and outputs live in NaN-guarded device buffers"""

    def __init__(self, dev):
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from aim_amd import ops
        from aim_amd.lib import check, load_library
        self.lib, self.check, self.stream, self.dev = load_library(), check, ops._stream, torch.device(dev)

    def put(self, **tensors):
        out = {}
        for k, t in tensors.items():
            if t is None:
                out[k] = None
            elif t.dtype.is_floating_point:
                buf = torch.full((t.numel() + 8,), NAN, dtype=t.dtype, device=self.dev)
                buf[:t.numel()] = t.reshape(-1).to(self.dev)
                out[k] = buf
            else:
                out[k] = t.contiguous().to(self.dev)
        return out

    def outs(self, init=None, dtype=F32, **shapes):
        o = _Outs()
        for k, shape in shapes.items():
            n = int(np.prod(shape))
            buf = torch.full((n + 8,), NAN, dtype=dtype, device=self.dev)
            if init and k in init:
                buf[:n] = init[k].reshape(-1).to(self.dev)
            o[k] = buf
            o.shapes[k] = tuple(shape)
        return o

    def call(self, name, *args):
        a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
        self.check(getattr(self.lib, name)(*a, self.stream()), name)

    def collect(self, o):
        torch.cuda.synchronize()
        got, pad = {}, {}
        for k, buf in o.items():
            n = int(np.prod(o.shapes[k]))
            host = buf.cpu()
            got[k] = host[:n].view(o.shapes[k]).clone()
            pad[k] = bool(torch.isnan(host[n:]).all())
        return got, pad


class _Outs(dict):
    def __init__(self):
        super().__init__()
        self.shapes = {}


def run_case(ctx, case):
    rec = {"kind": case.kind, "checks": {}, "finite": {}, "pad": {}, "ident": {}, "nan": None}
    inp = build_inputs(case)
    launch, idents = KINDS[case.kind][3], KINDS[case.kind][5]
    got, pad = launch(ctx, case, inp)
    again, _ = launch(ctx, case, inp)
    rec["ident"]["repeat"] = all(_bits_eq(got[k], again[k]) for k in got)
    idents(ctx, case, inp, got, rec)
    rec["checks"] = compare(case, inp, got)
    rec["finite"] = finite_where_expected(case, inp, got)
    rec["pad"] = {("update" if case.kind == "adamw" and k == "p" else k): v for k, v in pad.items()}
    if expects_nan(case, inp):
        rec["nan"] = {k: bool(torch.isnan(v.float()).any()) for k, v in got.items()}
    return rec


# ---- refusals: name -> the text of the AIM_CHECK_ARG that must answer (test_ends_cases_cpu.py holds them to the sources) ------
REFUSAL_TEXT = {
    "head_fwd/D16388": "head_fwd: D=", "head_fwd/null_pooled": "head_fwd: bad arguments",
    "head_bwd/C16129": "head_bwd: C=", "head_bwd/all_null": "head_bwd: no output requested",
    "lambda/N321": "lambda: unsupported shape", "lambda/ntiles0": "lambda: bad arguments", "lambda/neither": "lambda: needs either",
    "qk_border/D768": "qk_border: unsupported shape", "qk_border/N321": "qk_border: unsupported shape",
    "qk_border/slot0+2>nslots": "qk_border: bad arguments",
    "patchify/H%p": "patchify: bad shape", "patchify/Kp<3pp": "patchify: Kp=", "patchify/Kp%8": "patchify: Kp=",
    "patchify/mean_without_std": "patchify: null pointer", "patchify/in_dtype3": "patchify: in_dtype must be",
    "adamw/misaligned": "adamw: p, g, m and v must be 16-byte aligned",
}
REFUSAL_SOURCE = {"head_fwd": "head.hip", "head_bwd": "head.hip", "lambda": "cls_attn.hip", "qk_border": "cls_attn.hip",
                  "patchify": "embed_misc.hip", "adamw": "embed_misc.hip"}


def run_refusals(ctx):
    """calls the library must refuse: {name: {message, every output still NaN}}"""
    dev, out = ctx.dev, {}

    def nanf(*shape, dtype=F32):
        return torch.full(shape, NAN, dtype=dtype, device=dev)

    def zf(*shape, dtype=F32):
        return torch.zeros(shape, dtype=dtype, device=dev)

    def attempt(name, fn, args, watched):
        try:
            ctx.call(fn, *args)
            msg = None
        except RuntimeError as e:
            msg = str(e)
        torch.cuda.synchronize()
        out[name] = {"message": msg, "untouched": all(bool(torch.isnan(t).all()) for t in watched)}

    D = 16388
    po, sc = nanf(1, D), nanf(1, 5)
    attempt("head_fwd/D16388", "aim_head_fwd", (zf(1, 1, D), None, zf(5, D), None, po, sc, 1, 1, D, 5), (po, sc))
    attempt("head_fwd/null_pooled", "aim_head_fwd", (zf(1, 1, 8), None, zf(5, 8), None, None, sc, 1, 1, 8, 5), (sc,))
    C = 16129
    dW, db, df = nanf(C, 8), nanf(C), nanf(1, 1, 8)
    attempt("head_bwd/C16129", "aim_head_bwd", (zf(1, C), zf(1, 8), None, zf(C, 8), dW, db, df, 1, 1, 8, C), (dW, db, df))
    attempt("head_bwd/all_null", "aim_head_bwd", (zf(1, 5), zf(1, 8), None, zf(5, 8), None, None, None, 1, 1, 8, 5), ())
    lam, part = nanf(1), zf(1, 4, 2)
    attempt("lambda/N321", "aim_lambda", (None, None, 0, zf(1, 321), part, 4, lam, None, 1, 321, 64, SCALE), (lam,))
    attempt("lambda/ntiles0", "aim_lambda", (None, None, 0, zf(1, 8), part, 0, lam, None, 1, 8, 64, SCALE), (lam,))
    attempt("lambda/neither", "aim_lambda", (None, None, 0, None, part, 4, lam, None, 1, 8, 64, SCALE), (lam,))
    ss, pt = nanf(1, 321), nanf(1, 2, 2)
    for name, (N, D, s0, ns) in {"D768": (9, 768, 0, 2), "N321": (321, 512, 0, 2), "slot0+2>nslots": (9, 512, 1, 2)}.items():
        attempt(f"qk_border/{name}", "aim_qk_border", (zf(1, N, 3 * D, dtype=BF16), zf(1, D, dtype=BF16), D, ss, pt, s0, ns, 1, N, D, SCALE), (ss, pt))
    A, img, m3 = nanf(64, 200, dtype=BF16), zf(1, 3, 1, 20, 16), zf(3)
    for name, (H, Kp, dt, mean, std) in {"H%p": (20, 192, 0, None, None), "Kp<3pp": (16, 184, 0, None, None), "Kp%8": (16, 196, 0, None, None),
                                         "mean_without_std": (16, 192, 0, m3, None), "in_dtype3": (16, 192, 3, None, None)}.items():
        attempt(f"patchify/{name}", "aim_patchify", (img, dt, mean, std, A, 1, 1, H, 16, 8, Kp), (A,))
    buf = nanf(4 * 16)
    p, g, m, v = (buf[16 * i:16 * i + 9] for i in range(4))
    attempt("adamw/misaligned", "aim_adamw_flat", (p.data_ptr() + 4, g, m, v, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0), (buf,))
    return out


def run(dev="cuda"):
    """every case and the refusals on `dev`: {"cases": {name: record}, "errors", "refusals", "seconds"}"""
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
        try:
            res["refusals"] = run_refusals(ctx)
        except Exception as e:
            res["errors"]["refusals"] = f"{type(e).__name__}: {e}"
            if any(s in str(e) for s in _FATAL):
                res["fatal"] = "refusals"
                return res
    res["seconds"] = time.time() - t0
    return res
