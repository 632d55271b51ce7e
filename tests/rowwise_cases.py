"""Every call form of the kernels between the GEMMs: the LayerNorms (aim_layernorm_fwd / _fwd_x16 / _fwd_fp8 / _bwd /
_bwd_fsum / _gb_bwd), the embedding glue (aim_embed_ln, aim_embed_bwd, aim_embed_nopre_fwd / _bwd), the ordered column and
frame reductions (aim_frame_sum, aim_colsum_bf16), the row adds and scales (aim_scale_rows, aim_add_rows_bf16, aim_add_bf16,
aim_acc_bf16) and the casts (aim_cast_bf16, aim_cast_multi); float64 references and bounds derived from the kernels'
rounding points.

A plain module (no fixtures).  None of these kernels reads an environment switch, so `run(dev)` executes every case in
the calling process; `test_rowwise_gpu.py` reads its records and `test_rowwise_cases_cpu.py` proves on the CPU that the
bounds accept an fp32 emulation of each kernel's arithmetic in its summation order (`emulate`) and reject the same
emulation with one plausible bug (`emulate(..., mut)`).

Notation: u = 2^-24 (one fp32 rounding, relative), U8 = 2^-8 (one bf16 rounding).  A result stored as bf16 from an fp32
value that is off by b is off by at most U8 |ref| + (1 + U8) b.  A sum of terms: (longest addition chain of the kernel's
summation tree + roundings per term) u sum |terms|, the initial value of an accumulating output counting as a term; on an
atomic route the order is free and the chain is the number of addends.

LayerNorm forward (csrc/norm.hip::ln_fwd_kernel, embed_misc.hip::embed_ln_kernel).  A lane sums its NC float4 chunks
((a+b)+(c+d) each), 6 butterfly steps, one division:
    L    = 2 + (NC-1) + 6 + 1
    e_mu = L u mean|x| ;  e_d = e_mu + u |d|   (d = x - mu)
    e_var = e_mu^2 + 2 mean(|d| e_d) + (L+4) u var           (4 sequential squares per chunk instead of the pair sum)
    r_rs = e_var / (2 (var+eps)) + 4u                         (rsqrtf: within two ulps, the addition and the division)
    |y' - y| <= |gamma| rstd e_d + |gamma d rstd| (r_rs + 3u) + u |y|
  mean and rstd are held to e_mu and rstd r_rs.  e4m3: half an ulp is 2^-4 of the binade, 2^-10 below 2^-6, values clamped
  to +-448.  embed_ln normalises v = fp32((tok|cls + pos) + temporal): the additions are single IEEE operations, so the
  reference takes them in fp32 in the same order and the bound above applies unchanged; embed_nopre_fwd is exactly that sum.

LayerNorm backward (ln_bwd_kernel, ln_bwd_fsum_kernel, embed_bwd_kernel), on the mean / rstd it is handed:
    xh = (x - mu) rs: two roundings;  g = dy gamma: one;  a lane adds its 4 NC elements one by one, 6 butterfly steps:
    L1 = 4 NC + 6;  e_m1 = (L1+1) u mean|g| + u|m1|;  e_m2 = (L1+4) u mean|g xh| + u|m2|
    t = g - m1 - xh m2:  e_t = e_m1 + |xh| e_m2 + 3u|g| + 2u|m1| + 4u|xh m2|
    o = rs t:  e_o = |rs| e_t + u|o|;   dx = o + dres: + u|dx|;   bf16 dx: U8|dx| + (1 + U8) (that)
  (ln_bwd_elem fuses xh m2 into the subtraction: one rounding fewer than the bound counts; rs t and + dres stay two operations
  in both ln_bwd_kernel and ln_bwd_fsum_kernel, which is what `dx_eq_layernorm_bwd` holds them to, bit for bit.)
  dy = 0 gives g = m1 = m2 = 0 exactly: the bound collapses to the one rounding of dres, and `zero_dy_exact` records the
  bit identity.  dgamma / dbeta: ln_dparam_kernel walks rows g, g+4, ... (chain ceil(rows/4)), joins four groups pairwise
  (2) and adds into the output (1); a term dy xh carries 3 roundings, a term dy none.  Above 8192 rows the main kernel
  adds every element atomically: chain = rows.  layernorm_gb_bwd: a slab of `rps` rows in order (fma: xh 2 + 1), slot s adds
  slabs s, s+16, ... (ceil(P/16)), the 16 slots in order, the output: chain rps + ceil(P/16) + 16 + 1.
  layernorm_bwd_fsum adds w[n] * (the bf16 dx it stored): the reference is stated on the kernel's own dx_bf16, chain
  ceil(rg/4) + 2, one rounding per term.  (So the mutant "sum of the unrounded dx" differs by 2^-8 |dx| per term against a
  bound of a few u: the bound separates it, see test_rowwise_cases_cpu.py.)
  embed_bwd: dtemporal[t] += sum_{b,n} o: sum e_o over the rows + chain u (|init| + sum|o|), chain = ceil(B N / (4 chunks))
  + 3 (waves) + ceil(chunks/4) + 2 + 1 with a workspace, ceil(B N / (4 chunks)) + 4 chunks + 1 with atomics.

Reductions.  frame_sum: chain ceil(ntok/4) + 2, one rounding per term (w x).  colsum: a term af at x carries 2 roundings;
  8-wide kernel: a row slot walks ceil(rpb/nrs) rows, slot 0 adds the other nrs - 1 in order, then one block adds into
  `out` (1), or the finish adds ceil(P/16) + 16 + 1, or P blocks add atomically (P + 1); scalar kernel: rpb + blocks + 1.
  embed_nopre_bwd: exact terms; dpos: BT + 1; dcls: BT + 1; dbias: BT + (N-1) + 1; dtemporal: N + B + 1.
Casts, add_bf16, add_rows, acc_bf16, scale_rows, the dtok copy: one IEEE operation and / or one round-to-nearest-even:
  bound 0 against torch's fp32 arithmetic and its bf16 conversion.
"""
import os
import sys
import time
from dataclasses import dataclass, field
from typing import Dict

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import U8, U24, _digest, _pad_intact, _padded, ratio  # noqa: E402

BF16, F32, F64, FP8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
DT = {"f32": F32, "bf16": BF16}
FAMILIES = ("unit", "offset", "scaled", "const", "zero_dy")
EPS = (1e-5, 1e-6)
NAN = float("nan")


@dataclass
class Case:
    name: str
    kind: str
    p: dict = field(default_factory=dict)
    family: str = "unit"
    eps: float = 1e-5
    seed: int = 0


# ------------------------------------------------------------------ mirrors of the host-side selection rules ----------------
def _cdiv(a, b):
    return (a + b - 1) // b


def ln_nc(D: int) -> int:
    """csrc/ln_row.h::nc_dispatch, the one ladder behind every launch of the wave-per-row kernels: float4 chunks per lane."""
    nc = (D + 255) // 256
    return nc if nc <= 4 else 8


def ln_dparam_route(rows: int, has_dgamma: bool):
    """csrc/norm.hip::aim_layernorm_bwd (AIM_LN_DPARAM_ROWS = 8192): who adds dgamma / dbeta."""
    if not has_dgamma:
        return None
    return "ordered" if rows <= 8192 else "atomic"


def colsum_route(M: int, C: int, ldx: int, workspace_bytes: int):
    """csrc/embed_misc.hip::aim_colsum_bf16: (route, row blocks, rows per block)."""
    if C % 8 == 0 and C <= 2048 and ldx % 8 == 0:
        rpb = max(64, (M + 1023) // 1024)
        P = _cdiv(M, rpb)
        if workspace_bytes >= P * C * 4 and P > 1:
            return ("two_stage", P, rpb)
        if M <= 2048:
            return ("one_block", 1, M)
        return ("atomic8", P, rpb)
    rpb = max(64, (M + 511) // 512)
    return ("scalar", _cdiv(M, rpb), rpb)


def embed_bwd_chunks(B: int, T: int, N: int) -> int:
    """csrc/embed_misc.hip::aim_embed_bwd (and aim_embed_bwd_workspace_bytes): row chunks (grid y) of embed_bwd_kernel."""
    return min((B * N + 3) // 4, (2048 + T - 1) // T)


def gb_slabs(rows: int):
    """csrc/vit_imagenet.hip::gb_rows_per_slab and aim_layernorm_gb_bwd: (rows per slab, slabs)."""
    rps = max(16, (rows + 1023) // 1024)
    return rps, _cdiv(rows, rps)


def cast_route(transpose: bool, ldd: int, C: int) -> str:
    """csrc/embed_misc.hip::aim_cast_bf16."""
    if transpose:
        return "transpose"
    return "strided" if ldd and ldd != C else "dense"


def cast_multi_route(desc) -> str:
    """csrc/embed_misc.hip::cast_multi_kernel; desc = (transpose, R, C, ldd, src 16-byte aligned, dst 8-byte aligned)."""
    tr, R, C, ldd, s16, d8 = desc
    if tr == 0 and C % 4 == 0 and ldd % 4 == 0 and s16 and d8:
        return "wide4"
    if tr == 1 and R % 32 == 0 and C % 32 == 0:
        return "tile32"
    return "copy32" if tr == 2 else "scalar"


# ------------------------------------------------------------------ helpers -------------------------------------------------
def _gen(case):
    return torch.Generator().manual_seed(case.seed)


def _family_x(fam, rows, D, g):
    x = torch.randn((rows, D), generator=g)
    if fam == "offset":
        x = x + 300.0
    elif fam == "scaled":
        x = x * torch.logspace(-3, 3, max(rows, 2))[:rows, None]
    elif fam == "const":
        x = (torch.arange(rows, dtype=F32)[:, None] * 0.75 + 3.25).expand(rows, D).clone()
        x[rows // 2] = 0.0
    return x.float().contiguous()


def _gb(D, g):
    return (1.0 + 0.1 * torch.randn(D, generator=g)).float(), (0.1 * torch.randn(D, generator=g)).float()


def _bf_bound(ref, b):
    return U8 * ref.abs() + (1 + U8) * b


def _fp8_half_ulp(a):
    e = torch.floor(torch.log2(a.abs().clamp(2.0 ** -6, 448.0)))
    return torch.pow(2.0, e - 4)


def _stats64(x, eps):
    mu = x.mean(1, keepdim=True)
    d = x - mu
    var = (d * d).mean(1, keepdim=True)
    return mu, d, var, (var + eps).rsqrt()


def ln_fwd_expected(x, G, B, eps, NC):
    """x, G, B float64 -> {y, mean, rstd: (value, bound)} (module docstring)"""
    L = 2 + (NC - 1) + 6 + 1
    mu, d, var, rs = _stats64(x, eps)
    y = d * rs * G + B
    e_mu = L * U24 * x.abs().mean(1, keepdim=True)
    e_d = e_mu + U24 * d.abs()
    e_var = e_mu ** 2 + 2 * (d.abs() * e_d).mean(1, keepdim=True) + (L + 4) * U24 * var
    r_rs = e_var / (2 * (var + eps)) + 4 * U24
    by = G.abs() * rs * e_d + (G * d * rs).abs() * (r_rs + 3 * U24) + U24 * y.abs()
    return {"y": (y, by), "mean": (mu[:, 0], e_mu[:, 0]), "rstd": (rs[:, 0], (rs * r_rs)[:, 0])}


def ln_bwd_expected(dy, x, G, mu, rs, dres, NC):
    """float64 dx and its fp32 bound on the statistics handed in (mu, rs: [rows, 1])"""
    xh = (x - mu) * rs
    g = dy * G
    L1 = 4 * NC + 6
    m1 = g.mean(1, keepdim=True)
    m2 = (g * xh).mean(1, keepdim=True)
    e_m1 = (L1 + 1) * U24 * g.abs().mean(1, keepdim=True) + U24 * m1.abs()
    e_m2 = (L1 + 4) * U24 * (g * xh).abs().mean(1, keepdim=True) + U24 * m2.abs()
    t = g - m1 - xh * m2
    e_t = e_m1 + xh.abs() * e_m2 + 3 * U24 * g.abs() + 2 * U24 * m1.abs() + 4 * U24 * (xh * m2).abs()
    o = rs * t
    e_o = rs.abs() * e_t + U24 * o.abs()
    if dres is None:
        return o, e_o
    dx = o + dres
    return dx, e_o + U24 * dx.abs()


def _sum_bound(chain, per_term, terms_abs_sum, init):
    return (chain + per_term) * U24 * (init.abs() + terms_abs_sum)


# ---- fp32 emulation pieces (CPU, IEEE single operations, the kernels' orders) ------------------------------------------------
def _lanes(v, NC):
    rows, D = v.shape
    out = torch.zeros((rows, NC * 256), dtype=F32)
    out[:, :D] = v
    return out.view(rows, NC, 64, 4)


_XOR = {o: torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)}


def _wave_seq(v, NC, pair=False):
    l = _lanes(v, NC)
    acc = torch.zeros((v.shape[0], 64), dtype=F32)
    for c in range(NC):
        if pair:
            acc = acc + ((l[:, c, :, 0] + l[:, c, :, 1]) + (l[:, c, :, 2] + l[:, c, :, 3]))
        else:
            for e in range(4):
                acc = acc + l[:, c, :, e]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, _XOR[o]]
    return acc[:, 0]


def _f32(v):
    return torch.tensor(v, dtype=F32)


def emu_ln_fwd(x, G, B, eps, NC, mut=None):
    D = x.shape[1]
    mu = _wave_seq(x, NC, pair=True) / _f32(float(NC * 256 if mut == "mean_padded" else D))
    d = x - mu[:, None]
    if mut == "one_pass":
        var = (_wave_seq(x * x, NC) / _f32(float(D)) - mu * mu).clamp_min(0.0)
    else:
        var = _wave_seq(d * d, NC) / _f32(float(D - 1 if mut == "unbiased" else D))
    rs = 1.0 / (var.sqrt() + _f32(eps)) if mut == "eps_outside" else torch.rsqrt(var + _f32(eps))
    return d * rs[:, None] * G + B, mu, rs


def emu_ln_bwd(dy, x, G, mu, rs, dres, NC, mut=None):
    D = x.shape[1]
    xh = (x - mu[:, None]) * rs[:, None]
    g = dy * G
    m1 = _wave_seq(g, NC) / _f32(float(D))
    m2 = _wave_seq(g * xh, NC) / _f32(float(D))
    if mut == "no_m1":
        m1 = torch.zeros_like(m1)
    if mut == "no_m2":
        m2 = torch.zeros_like(m2)
    # csrc/ln_row.h::ln_bwd_elem: fma(-xh, m2, g - m1) (an exact product in float64, rounded once), the scale, then the residual
    t = ((g - m1[:, None]).double() - xh.double() * m2[:, None].double()).float()
    if dres is not None and mut == "dres_before_scale":
        return rs[:, None] * (t + dres), xh
    o = rs[:, None] * t
    return (o if dres is None else o + dres), xh


def _groups4(t):
    """rows g, g + 4, ... in order per group g, then (0 + 1) + (2 + 3): ln_dparam, frame_sum, embed_bwd_finish"""
    n = t.shape[0]
    pad = torch.zeros((_cdiv(n, 4) * 4,) + tuple(t.shape[1:]), dtype=F32)
    pad[:n] = t
    v = pad.view(-1, 4, *t.shape[1:])
    acc = torch.zeros_like(v[0])
    for i in range(v.shape[0]):
        acc = acc + v[i]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def _seq(t):
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def _slots16(part):
    """finish kernels: slot s adds rows s, s + 16, ... in order, then the 16 slots in order"""
    P = part.shape[0]
    pad = torch.zeros((_cdiv(P, 16) * 16,) + tuple(part.shape[1:]), dtype=F32)
    pad[:P] = part
    return _seq(_seq(pad.view(-1, 16, *part.shape[1:])))


# ------------------------------------------------------------------ kinds ---------------------------------------------------
# Every kind has: inputs(case) -> CPU tensors; expected(case, inp, got) -> {output: (float64 value, bound)};
# emulate(case, inp, mut) -> {output: tensor of the output's dtype}; launch(ctx, case, inp) -> (got, rec) on the GPU.
KINDS: Dict[str, tuple] = {}


def _stats_for(case, inp, x, form, fwd=None):
    """mean / rstd [rows] f32 handed to a backward: (a) fp32 of the float64 ones, (b) the forward's own (fwd callable)"""
    if form == "b" and fwd is not None:
        return fwd()
    mu, _, _, rs = _stats64(x.double(), case.eps)
    return mu[:, 0].float(), rs[:, 0].float()


# ---- layernorm_fwd / _x16 / _fp8 ---------------------------------------------------------------------------------------------
def ln_fwd_inputs(case):
    p, g = case.p, _gen(case)
    x = _family_x(case.family, p["rows"], p["D"], g)
    if p["variant"] == "x16":
        x = x.to(BF16)
    G, B = _gb(p["D"], g)
    return {"x": x, "gamma": G, "beta": B}


def ln_fwd_expected_case(case, inp, got=None):
    NC = ln_nc(case.p["D"])
    e = ln_fwd_expected(inp["x"].double(), inp["gamma"].double(), inp["beta"].double(), case.eps, NC)
    y, by = e["y"]
    yc = y.clamp(-448.0, 448.0)
    out = {"y": (y, by), "yb": (y, _bf_bound(y, by)), "y8": (yc, by + _fp8_half_ulp(y.abs() + by)),
           "mean": e["mean"], "rstd": e["rstd"]}
    have = {"f32": ("y", "yb", "mean", "rstd"), "x16": ("y", "yb", "y8"), "fp8": ("y8",)}[case.p["variant"]]
    return {k: out[k] for k in have}


LN_FWD_MUTANTS = ("eps_outside", "unbiased", "one_pass", "mean_padded")


def ln_fwd_emulate(case, inp, mut=None):
    y, mu, rs = emu_ln_fwd(inp["x"].float(), inp["gamma"], inp["beta"], case.eps, ln_nc(case.p["D"]), mut)
    out = {"y": y, "yb": y.to(BF16), "y8": y.clamp(-448.0, 448.0).to(FP8), "mean": mu, "rstd": rs}
    return {k: out[k] for k in ln_fwd_expected_case(case, inp)}


def _nan_in(t, dev, extra_cols=8):
    """t inside a NaN-filled [R + 1, C + extra] device buffer: a strided input whose padding must not leak"""
    R, C = t.shape
    buf = torch.full((R + 1, C + extra_cols), NAN, dtype=t.dtype, device=dev)
    buf[:R, :C] = t.to(dev)
    return buf[:R, :C]


def _out8(R, C, dev):
    buf = torch.full((R + 3, C + 8), 0x7F, dtype=torch.uint8, device=dev)      # 0x7F: e4m3 NaN
    return buf[:R, :C], buf


def _pad8_intact(buf, R, C):
    b = buf.clone()
    b[:R, :C] = 0x7F
    return bool((b == 0x7F).all())


def _bits_eq(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and bool((a.view(iv) == b.view(iv)).all())


def _ln_fwd_call(ctx, variant, x, G, B, rows, D, eps, outs, stats=True):
    """one launch; outs: name -> [rows, D] view (all with the same row stride)"""
    ops = ctx.ops
    ldy = next(iter(outs.values())).stride(0)
    if variant == "f32":
        ops.layernorm_fwd(x, G, B, rows, D, x.stride(0), y_bf16=outs.get("yb"), y_f32=outs.get("y"), ldy=ldy,
                          mean=outs.get("mean"), rstd=outs.get("rstd"), eps=eps)
    elif variant == "x16":
        ops.layernorm_fwd_x16(x, G, B, rows, D, x.stride(0), y_bf16=outs.get("yb"), y_f32=outs.get("y"), y8=outs.get("y8"),
                              ldy=ldy, eps=eps)
    else:
        ops.layernorm_fwd_fp8(x, G, B, rows, D, x.stride(0), outs["y8"], ldy=ldy, eps=eps)


def _ln_fwd_outs(variant, rows, D, dev, dense=False):
    outs, bufs = {}, {}
    names = {"f32": ("y", "yb"), "x16": ("y", "yb", "y8"), "fp8": ("y8",)}[variant]
    for k in names:
        if k == "y8":
            outs[k], bufs[k] = _out8(rows, D, dev)
        else:
            outs[k], bufs[k] = _padded(rows, D, F32 if k == "y" else BF16, dev)
        if dense:
            outs[k] = torch.empty((rows, D), dtype=outs[k].dtype, device=dev)
    if variant == "f32":
        for k in ("mean", "rstd"):
            v, b = _padded(1, rows, F32, dev)
            outs[k], bufs[k] = v[0], b
    return outs, bufs


def _collect(rec, got, bufs, shapes):
    for k, v in got.items():
        f = v.view(FP8).float() if v.dtype == torch.uint8 else v.float()
        rec["finite"][k] = bool(torch.isfinite(f).all())
        R, C = shapes[k]
        rec["pad"][k] = _pad8_intact(bufs[k], R, C) if v.dtype == torch.uint8 else _pad_intact(bufs[k], R, C)


def _cpu(got):
    return {k: (v.cpu().view(FP8) if v.dtype == torch.uint8 else v.cpu()) for k, v in got.items()}


def ln_fwd_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    rows, D, var = p["rows"], p["D"], p["variant"]
    G, B = inp["gamma"].to(dev), inp["beta"].to(dev)
    xs = _nan_in(inp["x"], dev)
    outs, bufs = _ln_fwd_outs(var, rows, D, dev)
    _ln_fwd_call(ctx, var, xs, G, B, rows, D, case.eps, outs)
    shapes = {k: ((1, rows) if k in ("mean", "rstd") else (rows, D)) for k in outs}
    _collect(rec, outs, bufs, shapes)
    ident = rec["ident"]
    o2, _ = _ln_fwd_outs(var, rows, D, dev)
    _ln_fwd_call(ctx, var, xs, G, B, rows, D, case.eps, o2)
    ident["repeat"] = all(_bits_eq(outs[k], o2[k]) for k in outs)
    o3, _ = _ln_fwd_outs(var, rows, D, dev, dense=True)
    _ln_fwd_call(ctx, var, inp["x"].to(dev), G, B, rows, D, case.eps, o3)
    ident["strided_eq_dense"] = all(_bits_eq(outs[k], o3[k]) for k in outs)
    if "y" in outs and "yb" in outs:
        ident["yb_is_bf16_of_y"] = _bits_eq(outs["yb"], outs["y"].cpu().to(BF16))
    if "y" in outs and "y8" in outs:
        ident["y8_is_e4m3_of_y"] = _bits_eq(outs["y8"], outs["y"].cpu().clamp(-448.0, 448.0).to(FP8).view(torch.uint8))
    if var == "x16":          # the same rows as fp32 values through aim_layernorm_fwd
        o4, _ = _ln_fwd_outs("f32", rows, D, dev)
        _ln_fwd_call(ctx, "f32", inp["x"].float().to(dev), G, B, rows, D, case.eps, o4)
        ident["x16_eq_f32_of_bf16"] = _bits_eq(outs["y"], o4["y"]) and _bits_eq(outs["yb"], o4["yb"])
    if rows > 1 and case.family == "unit":
        r = rows - 1
        o5, _ = _ln_fwd_outs(var, 1, D, dev)
        _ln_fwd_call(ctx, var, xs[r:r + 1], G, B, 1, D, case.eps, o5)
        ident["row_alone"] = all(_bits_eq(outs[k][r:r + 1], o5[k]) for k in outs)
        xn = torch.full_like(xs, NAN)
        xn[r] = xs[r]
        o6, _ = _ln_fwd_outs(var, rows, D, dev)
        _ln_fwd_call(ctx, var, xn, G, B, rows, D, case.eps, o6)
        ident["nan_neighbours"] = all(_bits_eq(outs[k][r:r + 1], o6[k][r:r + 1]) for k in outs)
    return _cpu(outs)


KINDS["ln_fwd"] = (ln_fwd_inputs, ln_fwd_expected_case, ln_fwd_emulate, ln_fwd_launch, LN_FWD_MUTANTS)


# ---- embed_ln ------------------------------------------------------------------------------------------------------------------
def _embed_inputs(case, tok_dtype):
    p, g = case.p, _gen(case)
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    tok = _family_x(case.family, B * T * (N - 1), D, g).to(tok_dtype)
    sc = 300.0 if case.family == "offset" else 1.0
    cls = (torch.randn(D, generator=g) + (sc if sc > 1 else 0)).float()
    pos = (0.5 * torch.randn((N, D), generator=g)).float()
    tmp = (0.5 * torch.randn((T, D), generator=g)).float()
    if case.family == "const":
        cls, pos, tmp = torch.full((D,), 2.0), torch.full((N, D), 0.5), torch.full((T, D), 0.25)
    G, Bt = _gb(D, g)
    return {"tok": tok, "cls": cls, "pos": pos, "temporal": tmp, "gamma": G, "beta": Bt}


def _embed_value(inp, B, T, N, D, mut=None):
    """fp32 ((tok | cls) + pos) + temporal[t], the kernels' order: [B*T*N, D]"""
    a = torch.empty((B * T, N, D), dtype=F32)
    a[:, 0] = inp["cls"]
    a[:, 1:] = inp["tok"].float().view(B * T, N - 1, D)
    bt = torch.arange(B * T)
    tmp = inp["temporal"][bt.clamp_max(T - 1) if mut == "temporal_bt" else bt % T]
    return ((a + inp["pos"][None]) + tmp[:, None, :]).view(B * T * N, D)


def embed_ln_inputs(case):
    return _embed_inputs(case, BF16)


def embed_ln_expected(case, inp, got=None):
    p = case.p
    v = _embed_value(inp, p["B"], p["T"], p["N"], p["D"])
    e = ln_fwd_expected(v.double(), inp["gamma"].double(), inp["beta"].double(), case.eps, ln_nc(p["D"]))
    return {"x": e["y"], "mean": e["mean"], "rstd": e["rstd"]}


def embed_ln_emulate(case, inp, mut=None):
    p = case.p
    v = _embed_value(inp, p["B"], p["T"], p["N"], p["D"], mut)
    y, mu, rs = emu_ln_fwd(v, inp["gamma"], inp["beta"], case.eps, ln_nc(p["D"]), mut)
    return {"x": y, "mean": mu, "rstd": rs}


def _dense_out(R, C, dtype, dev, fill=NAN):
    """contiguous [R, C] at the head of a NaN-filled [R + 3, C] buffer"""
    buf = torch.full((R + 3, C), fill, dtype=dtype, device=dev)
    return buf[:R], buf


def embed_ln_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    M = B * T * N
    d = {k: v.to(dev) for k, v in inp.items()}

    def once():
        x, xb = _dense_out(M, D, F32, dev)
        mean, mb = _dense_out(1, M, F32, dev)
        rstd, rb = _dense_out(1, M, F32, dev)
        ctx.ops.embed_ln(d["tok"], d["cls"], d["pos"], d["temporal"], d["gamma"], d["beta"], x, mean[0], rstd[0], B, T, N, D,
                         eps=case.eps)
        return {"x": x, "mean": mean[0], "rstd": rstd[0]}, {"x": xb, "mean": mb, "rstd": rb}

    outs, bufs = once()
    _collect(rec, outs, bufs, {"x": (M, D), "mean": (1, M), "rstd": (1, M)})
    o2, _ = once()
    rec["ident"]["repeat"] = all(_bits_eq(outs[k], o2[k]) for k in outs)
    return _cpu(outs)


KINDS["embed_ln"] = (embed_ln_inputs, embed_ln_expected, embed_ln_emulate, embed_ln_launch,
                     ("eps_outside", "unbiased", "mean_padded", "temporal_bt"))


# ---- layernorm_bwd -------------------------------------------------------------------------------------------------------------
# forms: "strided" (every operand in a wider buffer, lddres != lddx), "dense", "classrow" (backbone.py:813-815: all rows
# without dres, then the class rows again at stride N*D with dres at stride D), "zshift" (zeroi2v.py:144: row 1 of every
# frame, inputs at stride P*D from a pointer one row in, dx at stride D)
def _bwd_geom(p):
    form = p["form"]
    if form in ("classrow", "zshift"):
        return p["BT"] * p["N"], p["BT"]
    return p["rows"], p["rows"]


def ln_bwd_inputs(case):
    p, g = case.p, _gen(case)
    M, R = _bwd_geom(p)
    D = p["D"]
    x = _family_x(case.family, M, D, g)
    dy = torch.randn((M, D), generator=g)
    if case.family == "zero_dy":
        dy = torch.zeros((M, D))
    G, _ = _gb(D, g)
    inp = {"x": x, "dy": dy.to(DT[p["dy"]]), "gamma": G}
    if p.get("dres"):
        inp["dres"] = torch.randn((R, D), generator=g).to(DT[p["dres"]])
    if p.get("dparam"):
        inp["dgamma0"] = torch.randn(D, generator=g).float()
        inp["dbeta0"] = torch.randn(D, generator=g).float()
    return inp


def _bwd_rows(p):
    """rows of x / dy that the (last) call reads"""
    M, R = _bwd_geom(p)
    if p["form"] == "classrow":
        return torch.arange(R) * p["N"]
    if p["form"] == "zshift":
        return torch.arange(R) * p["N"] + 1
    return torch.arange(R)


def _bwd_stats(case, inp, own=False):
    x = inp["x"]
    if own:
        G = inp["gamma"]
        _, mu, rs = emu_ln_fwd(x, G, torch.zeros_like(G), case.eps, ln_nc(case.p["D"]))
        return mu, rs
    mu, _, _, rs = _stats64(x.double(), case.eps)
    return mu[:, 0].float(), rs[:, 0].float()


def ln_bwd_expected_case(case, inp, got=None):
    p = case.p
    NC = ln_nc(p["D"])
    mu, rs = inp["mean"].double()[:, None], inp["rstd"].double()[:, None]
    x, dy, G = inp["x"].double(), inp["dy"].double(), inp["gamma"].double()
    rows = _bwd_rows(p)
    dres = inp["dres"].double() if "dres" in inp else None
    dx, b = ln_bwd_expected(dy[rows], x[rows], G, mu[rows], rs[rows], dres, NC)
    if p["form"] == "classrow":
        dxa, ba = ln_bwd_expected(dy, x, G, mu, rs, None, NC)
        dxa[rows], ba[rows] = dx, b
        dx, b = dxa, ba
    out = {}
    if p["outs"] in ("dx", "both"):
        out["dx"] = (dx, b)
    if p["outs"] in ("dxb", "both"):
        out["dxb"] = (dx, _bf_bound(dx, b))
    if p.get("dparam"):
        n = len(rows)
        chain = (_cdiv(n, 4) + 2 + 1) if ln_dparam_route(n, True) == "ordered" else n
        xh = (x[rows] - mu[rows]) * rs[rows]
        tg = dy[rows] * xh
        g0, b0 = inp["dgamma0"].double(), inp["dbeta0"].double()
        out["dgamma"] = (g0 + tg.sum(0), _sum_bound(chain, 3, tg.abs().sum(0), g0))
        out["dbeta"] = (b0 + dy[rows].sum(0), _sum_bound(chain, 0, dy[rows].abs().sum(0), b0))
    return out


LN_BWD_MUTANTS = ("no_m1", "no_m2", "dres_before_scale", "dres_at_lddx", "assign")


def ln_bwd_emulate(case, inp, mut=None):
    p = case.p
    D, NC = p["D"], ln_nc(p["D"])
    mu, rs = inp["mean"], inp["rstd"]
    x, dy, G = inp["x"], inp["dy"].float(), inp["gamma"]
    rows = _bwd_rows(p)
    dres = inp["dres"].float() if "dres" in inp else None
    if dres is not None and mut == "dres_at_lddx" and p["form"] == "classrow":
        flat = torch.zeros(len(rows) * p["N"] * D)
        flat[:dres.numel()] = dres.reshape(-1)
        dres = flat.view(len(rows), p["N"] * D)[:, :D].contiguous()
    dx, xh = emu_ln_bwd(dy[rows], x[rows], G, mu[rows], rs[rows], dres, NC, mut)
    out = {}
    if p["form"] == "classrow":
        dxa, _ = emu_ln_bwd(dy, x, G, mu, rs, None, NC, mut)
        dxa = dxa.to(BF16).float() if p["outs"] == "dxb" else dxa
        dxa[rows] = dx
        dx = dxa
    if p["outs"] in ("dx", "both"):
        out["dx"] = dx
    if p["outs"] in ("dxb", "both"):
        out["dxb"] = dx.to(BF16)
    if p.get("dparam"):
        tg, tb = dy[rows] * xh, dy[rows]
        red = _groups4 if ln_dparam_route(len(rows), True) == "ordered" else _seq
        z = 0.0 if mut == "assign" else 1.0
        out["dgamma"] = z * inp["dgamma0"] + red(tg)
        out["dbeta"] = z * inp["dbeta0"] + red(tb)
    return out


def _acc_out(init, dev):
    """an accumulating [C] output: row 0 of a NaN-padded buffer, set to `init`"""
    v, buf = _padded(1, init.numel(), F32, dev)
    v[0].copy_(init.to(dev))
    return v[0], buf


def ln_bwd_launch(ctx, case, inp, rec):
    p, dev, ops = case.p, ctx.dev, ctx.ops
    D, form = p["D"], p["form"]
    M, R = _bwd_geom(p)
    G = inp["gamma"].to(dev)
    mean, rstd = inp["mean"].to(dev), inp["rstd"].to(dev)
    strided = form == "strided"
    put = (lambda t, e=8: _nan_in(t, dev, e)) if strided else (lambda t, e=8: t.to(dev))
    x, dy = put(inp["x"]), put(inp["dy"])
    dres = put(inp["dres"], 16) if "dres" in inp else None
    rows_idx = _bwd_rows(p)

    def outs_for(nrows, dense):
        o, b = {}, {}
        for k, dt in (("dx", F32), ("dxb", BF16)):
            if p["outs"] in (k, "both"):
                o[k], b[k] = _dense_out(nrows, D, dt, dev) if dense else _padded(nrows, D, dt, dev)
        return o, b

    def params():
        if not p.get("dparam"):
            return {}, {}
        dg, dgb = _acc_out(inp["dgamma0"], dev)
        db, dbb = _acc_out(inp["dbeta0"], dev)
        return {"dgamma": dg, "dbeta": db}, {"dgamma": dgb, "dbeta": dbb}

    def call(dy_, x_, mean_, rstd_, dres_, o, pr, nrows, lddy, ldx, lddx, lddres=None):
        ops.layernorm_bwd(dy_, x_, G, mean_, rstd_, nrows, D, lddy=lddy, ldx=ldx, lddx=lddx, dres=dres_, dx=o.get("dx"),
                          dx_bf16=o.get("dxb"), dgamma=pr.get("dgamma"), dbeta=pr.get("dbeta"), lddres=lddres)

    ident = rec["ident"]
    if form in ("strided", "dense"):
        def once(dense=False):
            o, b = outs_for(R, dense or form == "dense")
            pr, pb = params()
            if dense and strided:
                call(inp["dy"].to(dev), inp["x"].to(dev), mean, rstd, inp["dres"].to(dev) if dres is not None else None, o, pr,
                     R, D, D, D, D)
            else:
                lddx = next(iter(o.values())).stride(0)
                call(dy, x, mean, rstd, dres, o, pr, R, dy.stride(0), x.stride(0), lddx,
                     dres.stride(0) if dres is not None else None)
            return {**o, **pr}, {**b, **pb}
        outs, bufs = once()
        o2, _ = once()
        fixed = [k for k in outs if k in ("dx", "dxb") or ln_dparam_route(R, True) == "ordered"]
        ident["repeat"] = all(_bits_eq(outs[k], o2[k]) for k in fixed)
        if strided:
            o3, _ = once(dense=True)
            ident["strided_eq_dense"] = all(_bits_eq(outs[k], o3[k]) for k in fixed)
        if R > 1 and case.family == "unit" and not p.get("dparam"):
            r = R - 1
            o5, _ = outs_for(1, False)
            call(dy[r:r + 1], x[r:r + 1], mean[r:r + 1], rstd[r:r + 1], dres[r:r + 1] if dres is not None else None, o5, {}, 1,
                 dy.stride(0), x.stride(0), next(iter(o5.values())).stride(0), dres.stride(0) if dres is not None else None)
            ident["row_alone"] = all(_bits_eq(outs[k][r:r + 1], o5[k]) for k in o5)
    elif form == "classrow":
        N = p["N"]
        o, b = outs_for(M, True)
        call(dy, x, mean, rstd, None, o, {}, M, D, D, D)
        first = {k: v.clone() for k, v in o.items()}
        mc, rc = mean[::N].contiguous(), rstd[::N].contiguous()
        call(dy, x, mc, rc, dres, o, {}, R, N * D, N * D, N * D, D)
        outs, bufs = o, b
        other = torch.ones(M, dtype=torch.bool)
        other[rows_idx] = False
        ident["other_rows_kept"] = all(_bits_eq(o[k][other.to(dev)], first[k][other.to(dev)]) for k in o)
    else:                               # zshift
        P = p["N"]
        o, b = outs_for(R, True)
        ms, rs_ = mean.view(R, P)[:, 1].contiguous(), rstd.view(R, P)[:, 1].contiguous()
        call(dy[1:], x[1:], ms, rs_, dres, o, {}, R, P * D, P * D, D, D if dres is not None else None)
        outs, bufs = o, b
    nrows_out = M if form == "classrow" else R
    _collect(rec, outs, bufs, {k: ((1, D) if k in ("dgamma", "dbeta") else (nrows_out, D)) for k in outs})
    got = _cpu(outs)
    if case.family == "zero_dy" and form in ("strided", "dense"):
        want = inp["dres"].float() if "dres" in inp else torch.zeros((R, D))
        ok = all(_bits_eq(got[k], want.to(got[k].dtype)) or ("dres" not in inp and bool((got[k] == 0).all()))
                 for k in ("dx", "dxb") if k in got)
        if p.get("dparam"):
            ok = ok and _bits_eq(got["dgamma"], inp["dgamma0"]) and _bits_eq(got["dbeta"], inp["dbeta0"])
        ident["zero_dy_exact"] = ok
    if p.get("dparam"):
        rec["route"] = ln_dparam_route(R, True)
    return got


KINDS["ln_bwd"] = (ln_bwd_inputs, ln_bwd_expected_case, ln_bwd_emulate, ln_bwd_launch, LN_BWD_MUTANTS)


# ---- layernorm_bwd_fsum --------------------------------------------------------------------------------------------------------
def ln_fsum_inputs(case):
    p, g = case.p, _gen(case)
    F, ntok, D = p["frames"], p["ntok"], p["D"]
    M = F * ntok
    inp = {"x": _family_x(case.family, M, D, g), "gamma": _gb(D, g)[0],
           "dy": (torch.zeros((M, D)) if case.family == "zero_dy" else torch.randn((M, D), generator=g)).to(BF16),
           "dres": torch.randn((M, D), generator=g).to(BF16)}
    if p["w"] != "none":
        w = torch.rand(ntok, generator=g) + 0.25
        w[1::3] = 0.0
        inp["w"] = w.float()
    return inp


def _fsum_groups(ntok, G, shift=0):
    rg = _cdiv(ntok, G)
    return [(min(ntok, g * rg + shift), min(ntok, (g + 1) * rg + shift)) for g in range(G)], rg


def ln_fsum_expected(case, inp, got=None):
    p = case.p
    F, ntok, D, G = p["frames"], p["ntok"], p["D"], p["groups"]
    dx, b = ln_bwd_expected(inp["dy"].double(), inp["x"].double(), inp["gamma"].double(), inp["mean"].double()[:, None],
                            inp["rstd"].double()[:, None], inp["dres"].double(), ln_nc(D))
    out = {"dxb": (dx, _bf_bound(dx, b))}
    stored = (got["dxb"] if got is not None and "dxb" in got else dx.to(BF16)).double().view(F, ntok, D)
    w = inp["w"].double() if "w" in inp else torch.ones(ntok, dtype=F64)
    terms = stored * w[None, :, None]
    groups, rg = _fsum_groups(ntok, G)
    ref = torch.stack([terms[:, a:e].sum(1) for a, e in groups], 1)
    mag = torch.stack([terms[:, a:e].abs().sum(1) for a, e in groups], 1)
    out["partial"] = (ref.view(F * G, D), ((_cdiv(rg, 4) + 2 + 1) * U24 * mag).view(F * G, D))
    return out


LN_FSUM_MUTANTS = ("no_m2", "group_off_by_one", "w_next", "fsum_unrounded")


def ln_fsum_emulate(case, inp, mut=None):
    p = case.p
    F, ntok, D, G = p["frames"], p["ntok"], p["D"], p["groups"]
    o, _ = emu_ln_bwd(inp["dy"].float(), inp["x"], inp["gamma"], inp["mean"], inp["rstd"], inp["dres"].float(), ln_nc(D), mut)
    ob = o.to(BF16)
    w = inp["w"] if "w" in inp else torch.ones(ntok)
    if mut == "w_next":
        w = w.roll(-1)
    terms = (w[None, :, None] * (o if mut == "fsum_unrounded" else ob.float()).view(F, ntok, D))
    groups, _ = _fsum_groups(ntok, G, 1 if mut == "group_off_by_one" else 0)
    part = torch.stack([_groups4(terms[:, a:e].transpose(0, 1)) if e > a else torch.zeros((F, D)) for a, e in groups], 1)
    return {"dxb": ob, "partial": part.reshape(F * G, D)}


def ln_fsum_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    F, ntok, D, G = p["frames"], p["ntok"], p["D"], p["groups"]
    M = F * ntok
    d = {k: v.to(dev) for k, v in inp.items()}

    def once():
        dxb, b1 = _dense_out(M, D, BF16, dev)
        part, b2 = _dense_out(F * G, D, F32, dev)
        ctx.check(ctx.lib.aim_layernorm_bwd_fsum(d["dy"].data_ptr(), D, d["x"].data_ptr(), D, d["gamma"].data_ptr(),
                                                 d["mean"].data_ptr(), d["rstd"].data_ptr(), d["dres"].data_ptr(), dxb.data_ptr(), D,
                                                 d["w"].data_ptr() if "w" in d else None, part.data_ptr(), G, F, ntok, D,
                                                 ctx.stream()), "aim_layernorm_bwd_fsum")
        return {"dxb": dxb, "partial": part}, {"dxb": b1, "partial": b2}

    outs, bufs = once()
    _collect(rec, outs, bufs, {"dxb": (M, D), "partial": (F * G, D)})
    o2, _ = once()
    rec["ident"]["repeat"] = all(_bits_eq(outs[k], o2[k]) for k in outs)
    # the same rows through aim_layernorm_bwd (bf16 dy, bf16 dres): "the per-row arithmetic is ln_bwd_kernel's, bit for bit"
    dx2, _ = _dense_out(M, D, BF16, dev)
    ctx.ops.layernorm_bwd(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], M, D, lddy=D, ldx=D, lddx=D, dres=d["dres"],
                          dx_bf16=dx2)
    rec["ident"]["dx_eq_layernorm_bwd"] = _bits_eq(outs["dxb"], dx2)
    got = _cpu(outs)
    if case.family == "zero_dy":
        rec["ident"]["zero_dy_exact"] = _bits_eq(got["dxb"], inp["dres"])
    return got


KINDS["ln_fsum"] = (ln_fsum_inputs, ln_fsum_expected, ln_fsum_emulate, ln_fsum_launch, LN_FSUM_MUTANTS)


# ---- layernorm_gb_bwd ------------------------------------------------------------------------------------------------------------
def ln_gb_inputs(case):
    p, g = case.p, _gen(case)
    rows, D = p["rows"], p["D"]
    dy = torch.zeros((rows, D)) if case.family == "zero_dy" else torch.randn((rows, D), generator=g)
    return {"x": _family_x(case.family, rows, D, g), "dy": dy.to(DT[p["dy"]]), "gamma": torch.ones(D),
            "dgamma0": torch.randn(D, generator=g).float(), "dbeta0": torch.randn(D, generator=g).float()}


def ln_gb_expected(case, inp, got=None):
    p = case.p
    rps, P = gb_slabs(p["rows"])
    chain = min(rps, p["rows"]) + _cdiv(P, 16) + 16 + 1
    x, dy = inp["x"].double(), inp["dy"].double()
    tg = dy * (x - inp["mean"].double()[:, None]) * inp["rstd"].double()[:, None]
    g0, b0 = inp["dgamma0"].double(), inp["dbeta0"].double()
    out = {"dgamma": (g0 + tg.sum(0), _sum_bound(chain, 3, tg.abs().sum(0), g0)),
           "dbeta": (b0 + dy.sum(0), _sum_bound(chain, 0, dy.abs().sum(0), b0))}
    return {k: v for k, v in out.items() if p["which"] in (k, "both")}


def ln_gb_emulate(case, inp, mut=None):
    p = case.p
    rows, D = p["rows"], p["D"]
    rps, P = gb_slabs(rows)
    dy = inp["dy"].float()
    xh = (inp["x"] - inp["mean"][:, None]) * inp["rstd"][:, None]
    out = {}
    for k, t, init in (("dgamma", dy * xh, inp["dgamma0"]), ("dbeta", dy, inp["dbeta0"])):
        if p["which"] not in (k, "both"):
            continue
        pad = torch.zeros((P * rps, D))
        pad[:rows] = t
        part = _seq(pad.view(P, rps, D).transpose(0, 1))
        out[k] = (0.0 if mut == "assign" else 1.0) * init + _slots16(part)
    return out


def ln_gb_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    rows, D = p["rows"], p["D"]
    mean, rstd = inp["mean"].to(dev), inp["rstd"].to(dev)
    x = _nan_in(inp["x"], dev, 2 * D) if p.get("strided") else inp["x"].to(dev)
    dy = _nan_in(inp["dy"], dev) if p.get("strided") else inp["dy"].to(dev)
    need = ctx.lib.aim_layernorm_gb_bwd_workspace_bytes(rows, D)
    rps, P = gb_slabs(rows)
    rec["route"] = f"slab{rps}"
    rec["ident"]["workspace_bytes_as_mirrored"] = need == 2 * P * D * 4

    def once():
        ws = torch.full((need // 4 + 64,), NAN, device=dev)
        o, b = {}, {}
        for k in ("dgamma", "dbeta"):
            if p["which"] in (k, "both"):
                o[k], b[k] = _acc_out(inp[k + "0"], dev)
        ctx.check(ctx.lib.aim_layernorm_gb_bwd(dy.data_ptr(), int(dy.dtype == BF16), dy.stride(0), x.data_ptr(), x.stride(0),
                                               mean.data_ptr(), rstd.data_ptr(), o["dgamma"].data_ptr() if "dgamma" in o else None,
                                               o["dbeta"].data_ptr() if "dbeta" in o else None, rows, D, ws.data_ptr(), need,
                                               ctx.stream()), "aim_layernorm_gb_bwd")
        return o, b, ws

    outs, bufs, ws = once()
    _collect(rec, outs, bufs, {k: (1, D) for k in outs})
    rec["evidence"] = {"slabs_written": bool(torch.isfinite(ws[:need // 4]).all()), "rest_untouched": bool(torch.isnan(ws[need // 4:]).all())}
    o2, _, _ = once()
    rec["ident"]["repeat"] = all(_bits_eq(outs[k], o2[k]) for k in outs)
    got = _cpu(outs)
    if case.family == "zero_dy":
        rec["ident"]["zero_dy_exact"] = all(_bits_eq(got[k], inp[k + "0"]) for k in got)
    return got


KINDS["ln_gb"] = (ln_gb_inputs, ln_gb_expected, ln_gb_emulate, ln_gb_launch, ("assign",))


# ---- embed_bwd -------------------------------------------------------------------------------------------------------------------
def embed_bwd_inputs(case):
    inp = _embed_inputs(case, BF16)
    p, g = case.p, torch.Generator().manual_seed(case.seed + 1)
    M = p["B"] * p["T"] * p["N"]
    dx = torch.zeros((M, p["D"])) if case.family == "zero_dy" else torch.randn((M, p["D"]), generator=g)
    inp["dx"] = dx.to(DT[p["dx"]])
    inp["dtemporal0"] = torch.randn((p["T"], p["D"]), generator=g).float()
    inp["x"] = _embed_value(inp, p["B"], p["T"], p["N"], p["D"])          # ln_pre's input: what the statistics are taken of
    return inp


def _embed_bwd_chain(p):
    B, T, N = p["B"], p["T"], p["N"]
    chunks = embed_bwd_chunks(B, T, N)
    walk = _cdiv(B * N, 4 * chunks)
    return chunks, (walk + 3 + _cdiv(chunks, 4) + 2 + 1) if p["ws"] else (walk + 4 * chunks + 1)


def embed_bwd_expected(case, inp, got=None):
    p = case.p
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    o, e_o = ln_bwd_expected(inp["dx"].double(), inp["x"].double(), inp["gamma"].double(), inp["mean"].double()[:, None],
                             inp["rstd"].double()[:, None], None, ln_nc(D))
    o, e_o = o.view(B, T, N, D), e_o.view(B, T, N, D)
    _, chain = _embed_bwd_chain(p)
    t0 = inp["dtemporal0"].double()
    return {"dtemporal": (t0 + o.sum((0, 2)), e_o.sum((0, 2)) + chain * U24 * (t0.abs() + o.abs().sum((0, 2))))}


def embed_bwd_emulate(case, inp, mut=None):
    p = case.p
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    v = _embed_value(inp, B, T, N, D, mut)
    o, _ = emu_ln_bwd(inp["dx"].float(), v, inp["gamma"], inp["mean"], inp["rstd"], None, ln_nc(D), mut)
    o = o.view(B, T, N, D).permute(1, 0, 2, 3).reshape(T, B * N, D)
    chunks, _ = _embed_bwd_chain(p)
    K = _cdiv(B * N, 4 * chunks)
    pad = torch.zeros((T, K * chunks * 4, D))
    pad[:, :B * N] = o
    acc = _seq(pad.view(T, K, chunks, 4, D).transpose(0, 1))             # [T, chunks, 4, D]: every wave's walk
    if p["ws"]:
        part = ((acc[:, :, 0] + acc[:, :, 1]) + acc[:, :, 2]) + acc[:, :, 3]
        tot = _groups4(part.transpose(0, 1))
    else:
        tot = _seq(acc.reshape(T, chunks * 4, D).transpose(0, 1))
    return {"dtemporal": (0.0 if mut == "assign" else 1.0) * inp["dtemporal0"] + tot}


def embed_bwd_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    d = {k: v.to(dev) for k, v in inp.items()}
    need = ctx.lib.aim_embed_bwd_workspace_bytes(B, T, N, D)
    chunks = embed_bwd_chunks(B, T, N)
    rec["ident"]["workspace_bytes_as_mirrored"] = need == T * chunks * D * 4
    rec["route"] = "two_stage" if p["ws"] else "atomic"

    # dtemporal is dense [T, D] by contract: it sits at the head of a NaN-filled buffer
    def padded_once():
        ws = torch.full((need // 4 + 64,), NAN, device=dev)
        dt, buf = _dense_out(T, D, F32, dev)
        dt.copy_(d["dtemporal0"])
        ctx.check(ctx.lib.aim_embed_bwd(d["dx"].data_ptr(), int(d["dx"].dtype == BF16), d["tok"].data_ptr(), d["cls"].data_ptr(),
                                        d["pos"].data_ptr(), d["temporal"].data_ptr(), d["gamma"].data_ptr(), d["mean"].data_ptr(),
                                        d["rstd"].data_ptr(), dt.data_ptr(), B, T, N, D, ws.data_ptr() if p["ws"] else None,
                                        need if p["ws"] else 0, ctx.stream()), "aim_embed_bwd")
        return dt, buf, ws

    dt, buf, ws = padded_once()
    _collect(rec, {"dtemporal": dt}, {"dtemporal": buf}, {"dtemporal": (T, D)})
    if p["ws"]:
        rec["evidence"] = {"partials_written": bool(torch.isfinite(ws[:need // 4]).all()),
                           "rest_untouched": bool(torch.isnan(ws[need // 4:]).all())}
        dt2, _, _ = padded_once()
        rec["ident"]["repeat"] = _bits_eq(dt, dt2)
    else:
        rec["evidence"] = {"workspace_untouched": bool(torch.isnan(ws).all())}
    got = {"dtemporal": dt.cpu()}
    if case.family == "zero_dy":
        rec["ident"]["zero_dy_exact"] = _bits_eq(got["dtemporal"], inp["dtemporal0"])
    return got


KINDS["embed_bwd"] = (embed_bwd_inputs, embed_bwd_expected, embed_bwd_emulate, embed_bwd_launch, ("assign", "temporal_bt", "no_m1"))


# ---- frame_sum -----------------------------------------------------------------------------------------------------------------
def frame_sum_inputs(case):
    p, g = case.p, _gen(case)
    F, ntok, D = p["frames"], p["ntok"], p["D"]
    inp = {"x": _family_x(case.family, F * ntok, D, g).to(DT[p["x"]])}
    if p["w"]:
        w = torch.rand(ntok, generator=g) + 0.25
        w[2::5] = 0.0
        inp["w"] = w.float()
    return inp


def frame_sum_expected(case, inp, got=None):
    p = case.p
    F, ntok, D = p["frames"], p["ntok"], p["D"]
    w = inp["w"].double() if "w" in inp else torch.ones(ntok, dtype=F64)
    t = inp["x"].double().view(F, ntok, D) * w[None, :, None]
    return {"out": (t.sum(1), (_cdiv(ntok, 4) + 2 + 1) * U24 * t.abs().sum(1))}


def frame_sum_emulate(case, inp, mut=None):
    p = case.p
    F, ntok, D = p["frames"], p["ntok"], p["D"]
    w = inp["w"] if "w" in inp else torch.ones(ntok)
    if mut == "w_next":
        w = w.roll(-1)
    t = inp["x"].float().view(F, ntok, D) * w[None, :, None]
    return {"out": _groups4(t.transpose(0, 1))}


def frame_sum_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    F, ntok, D = p["frames"], p["ntok"], p["D"]
    x = inp["x"].to(dev)
    w = inp["w"].to(dev) if "w" in inp else None

    def once():
        out, buf = _dense_out(F, D, F32, dev)
        ctx.ops.frame_sum(x, w, out, F, ntok, D)
        return out, buf

    out, buf = once()
    _collect(rec, {"out": out}, {"out": buf}, {"out": (F, D)})
    rec["ident"]["repeat"] = _bits_eq(out, once()[0])
    if F > 1:
        o1, _ = _dense_out(1, D, F32, dev)
        ctx.ops.frame_sum(x[(F - 1) * ntok:], w, o1, 1, ntok, D)
        rec["ident"]["row_alone"] = _bits_eq(out[F - 1:], o1)
    return {"out": out.cpu()}


KINDS["frame_sum"] = (frame_sum_inputs, frame_sum_expected, frame_sum_emulate, frame_sum_launch, ("w_next",))


# ---- colsum --------------------------------------------------------------------------------------------------------------------
def _colsum_ws_bytes(p):
    M, C = p["M"], p["C"]
    if p["ws"] == "none":
        return 0
    _, P, _ = colsum_route(M, C, p.get("ldx") or C, 1 << 60)
    return P * C * 4 - (4 if p["ws"] == "short" else 0)


def colsum_plan(p):
    return colsum_route(p["M"], p["C"], p.get("ldx") or p["C"], _colsum_ws_bytes(p))


def colsum_inputs(case):
    p, g = case.p, _gen(case)
    M, C, ntok = p["M"], p["C"], p.get("ntok", 0)
    inp = {"X": _family_x("unit" if case.family == "zero_dy" else case.family, M, C, g).to(BF16),
           "out0": torch.randn(C, generator=g).float()}
    if p.get("af"):
        inp["af"] = (torch.rand(_cdiv(M, ntok), generator=g) * 0.7 + 0.3).float()
    if p.get("at"):
        at = (torch.rand(ntok, generator=g) < 0.7).float() * (0.5 / 0.7)
        at[0] = 0.5
        inp["at"] = at
    return inp


def _colsum_rs(inp, M, ntok, mut=None, dtype=F32):
    rs = torch.ones(M, dtype=dtype)
    if ntok:
        m = torch.arange(M)
        f, tk = m // ntok, m % ntok
        if "af" in inp:
            af = inp["af"].to(dtype)
            rs = rs * af[(tk if mut == "af_mod" else f).clamp_max(len(af) - 1)]
        if "at" in inp:
            at = inp["at"].to(dtype)
            rs = rs * at[(f if mut == "at_div" else tk).clamp_max(len(at) - 1)]
    return rs


def colsum_expected(case, inp, got=None):
    p = case.p
    M, C = p["M"], p["C"]
    route, P, rpb = colsum_plan(p)
    if route == "scalar":
        chain = min(rpb, M) + P + 1
    else:
        nrs = max(1, 256 // (C // 8))
        walk = _cdiv(min(rpb, M), nrs) + nrs - 1
        chain = walk + {"one_block": 1, "two_stage": _cdiv(P, 16) + 16 + 1, "atomic8": P + 1}[route]
    t = inp["X"].double() * _colsum_rs(inp, M, p.get("ntok", 0), dtype=F64)[:, None]
    o0 = inp["out0"].double()
    return {"out": (o0 + t.sum(0), _sum_bound(chain, 2, t.abs().sum(0), o0))}


def colsum_emulate(case, inp, mut=None):
    p = case.p
    M, C = p["M"], p["C"]
    route, P, rpb = colsum_plan(p)
    t = _colsum_rs(inp, M, p.get("ntok", 0), mut)[:, None] * inp["X"].float()
    rpb = min(rpb, M) if route != "one_block" else M
    nrs = 1 if route == "scalar" else max(1, 256 // (C // 8))
    K = _cdiv(rpb, nrs)
    pad = torch.zeros((P, K * nrs, C))
    for b in range(P):
        blk = t[b * rpb:(b + 1) * rpb]
        pad[b, :blk.shape[0]] = blk
    slots = _seq(pad.view(P, K, nrs, C).transpose(0, 1))                  # [P, nrs, C]
    blocks = _seq(slots.transpose(0, 1))                                  # slot 0 adds the others in order
    tot = _slots16(blocks) if route == "two_stage" else _seq(blocks)
    return {"out": (0.0 if mut == "assign" else 1.0) * inp["out0"] + tot}


def colsum_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    M, C, ldx = p["M"], p["C"], p.get("ldx") or p["C"]
    route, P, rpb = colsum_plan(p)
    rec["route"] = route
    X = _nan_in(inp["X"], dev, ldx - C) if ldx > C else inp["X"].to(dev)
    af = inp["af"].to(dev) if "af" in inp else None
    at = inp["at"].to(dev) if "at" in inp else None
    nbytes = _colsum_ws_bytes(p)

    def once():
        ws = torch.full((nbytes // 4 + 32,), NAN, device=dev)
        out, buf = _acc_out(inp["out0"], dev)
        ctx.check(ctx.lib.aim_colsum_bf16(X.data_ptr(), X.stride(0), af.data_ptr() if af is not None else None,
                                          at.data_ptr() if at is not None else None, p.get("ntok", 0), out.data_ptr(), M, C,
                                          ws.data_ptr() if nbytes else None, nbytes, ctx.stream()), "aim_colsum_bf16")
        return out, buf, ws

    out, buf, ws = once()
    _collect(rec, {"out": out}, {"out": buf}, {"out": (1, C)})
    if route == "two_stage":
        rec["evidence"] = {"partials_written": bool(torch.isfinite(ws[:P * C]).all()), "rest_untouched": bool(torch.isnan(ws[P * C:]).all())}
    else:
        rec["evidence"] = {"workspace_untouched": bool(torch.isnan(ws).all())}
    if route in ("two_stage", "one_block") or P == 1:
        rec["ident"]["repeat"] = _bits_eq(out, once()[0])
    return {"out": out.cpu()}


KINDS["colsum"] = (colsum_inputs, colsum_expected, colsum_emulate, colsum_launch, ("at_div", "af_mod", "assign"))


# ---- embed_nopre_fwd / _bwd --------------------------------------------------------------------------------------------------
def nopre_fwd_inputs(case):
    return _embed_inputs(case, F32)


def nopre_fwd_expected(case, inp, got=None):
    p = case.p
    v = _embed_value(inp, p["B"], p["T"], p["N"], p["D"]).double()
    return {"x": (v, torch.zeros_like(v))}


def nopre_fwd_emulate(case, inp, mut=None):
    p = case.p
    return {"x": _embed_value(inp, p["B"], p["T"], p["N"], p["D"], mut)}


def nopre_fwd_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    d = {k: v.to(dev) for k, v in inp.items()}
    x, buf = _dense_out(B * T * N, D, F32, dev)
    ctx.ops.embed_nopre_fwd(d["tok"], d["cls"], d["pos"], d["temporal"], x, B, T, N, D)
    _collect(rec, {"x": x}, {"x": buf}, {"x": (B * T * N, D)})
    return {"x": x.cpu()}


KINDS["nopre_fwd"] = (nopre_fwd_inputs, nopre_fwd_expected, nopre_fwd_emulate, nopre_fwd_launch, ("temporal_bt",))
NOPRE_OUTS = ("dtok", "dcls", "dpos", "dtemporal", "dbias")


def nopre_bwd_inputs(case):
    p, g = case.p, _gen(case)
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    inp = {"dx": _family_x("unit" if case.family == "zero_dy" else case.family, B * T * N, D, g).to(DT[p["dx"]])}
    for k, shape in (("dcls", (1, D)), ("dpos", (N, D)), ("dtemporal", (T, D)), ("dbias", (1, D))):
        inp[k + "0"] = torch.randn(shape, generator=g).float()
    return inp


def nopre_bwd_expected(case, inp, got=None):
    p = case.p
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    dx = inp["dx"].double().view(B, T, N, D)
    a = dx.abs()
    i0 = {k: inp[k + "0"].double() for k in ("dcls", "dpos", "dtemporal", "dbias")}
    out = {"dtok": (dx[:, :, 1:].reshape(-1, D), torch.zeros((B * T * (N - 1), D), dtype=F64)),
           "dcls": (i0["dcls"] + dx[:, :, 0].sum((0, 1))[None], _sum_bound(B * T + 1, 0, a[:, :, 0].sum((0, 1))[None], i0["dcls"])),
           "dpos": (i0["dpos"] + dx.sum((0, 1)), _sum_bound(B * T + 1, 0, a.sum((0, 1)), i0["dpos"])),
           "dtemporal": (i0["dtemporal"] + dx.sum((0, 2)), _sum_bound(N + B + 1, 0, a.sum((0, 2)), i0["dtemporal"])),
           "dbias": (i0["dbias"] + dx[:, :, 1:].sum((0, 1, 2))[None],
                     _sum_bound(B * T + N - 1 + 1, 0, a[:, :, 1:].sum((0, 1, 2))[None], i0["dbias"]))}
    return {k: out[k] for k in p["outs"]}


def nopre_bwd_emulate(case, inp, mut=None):
    p = case.p
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    dxt = inp["dx"]
    dx = dxt.float().view(B * T, N, D)
    fsum = _seq(dx.transpose(0, 1))                                       # [BT, D], n ascending
    psum = _seq(dx)                                                       # [N, D], f ascending
    z = 0.0 if mut == "assign" else 1.0
    tok = dxt.view(B * T, N, D)[:, :-1] if mut == "dtok_shift" else dxt.view(B * T, N, D)[:, 1:]
    out = {"dtok": tok.reshape(-1, D).clone(), "dcls": z * inp["dcls0"] + psum[0][None], "dpos": z * inp["dpos0"] + psum,
           "dbias": z * inp["dbias0"] + _seq(psum[0 if mut == "dbias_with_cls" else 1:])[None],
           "dtemporal": z * inp["dtemporal0"] + _seq(fsum.view(B, T, D))}
    return {k: out[k] for k in p["outs"]}


def nopre_bwd_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    B, T, N, D = p["B"], p["T"], p["N"], p["D"]
    dx = inp["dx"].to(dev)
    need = ctx.lib.aim_embed_nopre_bwd_workspace_bytes(B, T, N, D)
    rec["ident"]["workspace_bytes_as_mirrored"] = need == (B * T + N) * D * 4
    shapes = {"dtok": (B * T * (N - 1), D), "dcls": (1, D), "dpos": (N, D), "dtemporal": (T, D), "dbias": (1, D)}

    def once():
        ws = torch.full((need // 4 + 64,), NAN, device=dev)
        o, b = {}, {}
        for k in p["outs"]:
            o[k], b[k] = _dense_out(*shapes[k], dx.dtype if k == "dtok" else F32, dev)
            if k != "dtok":
                o[k].copy_(inp[k + "0"].to(dev))
        ptr = lambda k: o[k].data_ptr() if k in o else None
        ctx.check(ctx.lib.aim_embed_nopre_bwd(dx.data_ptr(), int(dx.dtype == BF16), ptr("dtok"), ptr("dcls"), ptr("dpos"),
                                              ptr("dtemporal"), ptr("dbias"), B, T, N, D, ws.data_ptr(), need, ctx.stream()),
                  "aim_embed_nopre_bwd")
        return o, b, ws

    outs, bufs, ws = once()
    _collect(rec, outs, bufs, {k: shapes[k] for k in outs})
    rec["evidence"] = {"sums_written": bool(torch.isfinite(ws[:need // 4]).all()), "rest_untouched": bool(torch.isnan(ws[need // 4:]).all())}
    o2, _, _ = once()
    rec["ident"]["repeat"] = all(_bits_eq(outs[k], o2[k]) for k in outs)
    return _cpu(outs)


KINDS["nopre_bwd"] = (nopre_bwd_inputs, nopre_bwd_expected, nopre_bwd_emulate, nopre_bwd_launch,
                      ("assign", "dbias_with_cls", "dtok_shift"))


# ---- casts -----------------------------------------------------------------------------------------------------------------------
def _cast_src(R, C, g):
    src = torch.randn((R, C), generator=g) * torch.logspace(-4, 4, R)[:, None]
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 3.0e38, 2.0 ** -100])
    flat = src.view(-1)
    n = min(len(ties), flat.numel())
    flat[:n] = ties[:n]                                                    # exact ties: nearest-even, not up, not truncated
    return src.float().contiguous()


def _truncate(t):
    return (t.float().view(torch.int32) & -65536).view(F32).to(BF16)


def cast_inputs(case):
    return {"src": _cast_src(case.p["R"], case.p["C"], _gen(case))}


def cast_expected(case, inp, got=None):
    s = inp["src"].T if case.p["mode"].startswith("transpose") else inp["src"]
    v = s.to(BF16).double().contiguous()
    return {"dst": (v, torch.zeros_like(v))}


def cast_emulate(case, inp, mut=None):
    tr = case.p["mode"].startswith("transpose") and mut != "no_transpose"
    s = (inp["src"].T if tr else inp["src"]).contiguous()
    return {"dst": _truncate(s) if mut == "truncate" else s.to(BF16)}


def _cast_dst(mode, R, C, dev):
    if mode == "dense":
        return _dense_out(R, C, BF16, dev)
    if mode == "strided":
        return _padded(R, C, BF16, dev)
    if mode == "transpose":
        return _dense_out(C, R, BF16, dev)
    return _padded(C, R, BF16, dev)                                        # transpose_ldd: ldd > R


def cast_launch(ctx, case, inp, rec):
    p, dev = case.p, ctx.dev
    R, C, mode = p["R"], p["C"], p["mode"]
    src = inp["src"].to(dev)
    dst, buf = _cast_dst(mode, R, C, dev)
    tr = mode.startswith("transpose")
    rec["route"] = cast_route(tr, dst.stride(0), C)
    ctx.ops.cast_bf16(src, dst, transpose=tr)
    _collect(rec, {"dst": dst}, {"dst": buf}, {"dst": tuple(dst.shape)})
    return {"dst": dst.cpu()}


KINDS["cast"] = (cast_inputs, cast_expected, cast_emulate, cast_launch, ("truncate", "no_transpose"))
CAST_SHAPES = ((1, 4), (33, 7), (32, 32), (64, 96), (100, 36))
CAST_MODES = ("dense", "strided", "transpose", "transpose_ldd")


def cast_multi_entries():
    """(R, C, mode, misaligned source); mode "copy": the fp32 copy (transpose = 2)"""
    ent = [(R, C, m, False) for R, C in CAST_SHAPES for m in CAST_MODES]
    return ent + [(64, 96, "dense", True), (33, 7, "copy", False), (64, 96, "copy", False)]


def cast_multi_desc(R, C, mode, mis):
    tr = 2 if mode == "copy" else int(mode.startswith("transpose"))
    ldd = {"dense": C, "strided": C + 8, "transpose": R, "transpose_ldd": R + 8, "copy": C}[mode]
    return (tr, R, C, ldd, not mis, True)


def cast_multi_inputs(case):
    g = _gen(case)
    return {f"src{i}": _cast_src(R, C, g) for i, (R, C, _, _) in enumerate(cast_multi_entries())}


def cast_multi_expected(case, inp, got=None):
    out = {}
    for i, (R, C, mode, _) in enumerate(cast_multi_entries()):
        s = inp[f"src{i}"]
        v = (s if mode == "copy" else (s.T if mode.startswith("transpose") else s).to(BF16)).double().contiguous()
        out[f"dst{i}"] = (v, torch.zeros_like(v))
    return out


def cast_multi_emulate(case, inp, mut=None):
    out = {}
    for i, (R, C, mode, _) in enumerate(cast_multi_entries()):
        s = inp[f"src{i}"]
        if mode == "copy":
            out[f"dst{i}"] = s.clone()
            continue
        s = (s.T if mode.startswith("transpose") and mut != "no_transpose" else s).contiguous()
        out[f"dst{i}"] = _truncate(s) if mut == "truncate" else s.to(BF16)
    return out


def cast_multi_launch(ctx, case, inp, rec):
    dev = ctx.dev
    entries, outs, bufs, routes, same = [], {}, {}, {}, True
    for i, (R, C, mode, mis) in enumerate(cast_multi_entries()):
        if mis:                       # a source 4 bytes past a 16-byte boundary
            flat = torch.empty(R * C + 1, device=dev)
            src = flat[1:].view(R, C)
            src.copy_(inp[f"src{i}"].to(dev))
        else:
            src = inp[f"src{i}"].to(dev)
        if mode == "copy":
            dst, buf = _dense_out(R, C, F32, dev)
        else:
            dst, buf = _cast_dst(mode, R, C, dev)
        desc = (2 if mode == "copy" else int(mode.startswith("transpose")), R, C, dst.stride(0), src.data_ptr() % 16 == 0,
                dst.data_ptr() % 8 == 0)
        routes[f"dst{i}"] = cast_multi_route(desc)
        same = same and routes[f"dst{i}"] == cast_multi_route(cast_multi_desc(R, C, mode, mis))
        entries.append((src, dst, 2 if mode == "copy" else mode.startswith("transpose")))
        outs[f"dst{i}"], bufs[f"dst{i}"] = dst, buf
    table = ctx.ops.CastTable(entries, dev)
    table.run()
    _collect(rec, outs, bufs, {k: tuple(v.shape) for k, v in outs.items()})
    rec["route"] = sorted(set(routes.values()))
    rec["ident"]["routes_as_mirrored"] = same
    ok = True
    for i, (R, C, mode, mis) in enumerate(cast_multi_entries()):
        if mode == "copy":
            continue
        d2, _ = _cast_dst(mode, R, C, dev)
        ctx.ops.cast_bf16(inp[f"src{i}"].to(dev), d2, transpose=mode.startswith("transpose"))
        ok = ok and _bits_eq(outs[f"dst{i}"], d2)
    rec["ident"]["cast_multi_eq_cast_bf16"] = ok
    return _cpu(outs)


KINDS["cast_multi"] = (cast_multi_inputs, cast_multi_expected, cast_multi_emulate, cast_multi_launch, ("truncate", "no_transpose"))


# ---- scale_rows, add_rows_bf16, add_bf16, acc_bf16 -----------------------------------------------------------------------------
def elem_inputs(case):
    p, g = case.p, _gen(case)
    R, C, op = p["R"], p["C"], p["op"]
    a = _cast_src(R, C, g) if case.family == "unit" else _family_x(case.family, R, C, g)
    b = torch.randn((R, C), generator=g).float()
    if op == "scale_rows":
        return {"x": a, "s": (torch.rand(R, generator=g) * 0.9 + 0.1).float()}
    if op == "add_rows":
        return {"dst0": b.to(BF16), "src": a.clamp(-1e30, 1e30)}
    if op == "add_bf16":
        return {"a": a.clamp(-1e30, 1e30).to(BF16), "b": b.to(BF16)}
    return {"x0": b, "s": a.clamp(-1e30, 1e30).to(BF16)}


def _elem_f32(case, inp, mut=None):
    op = case.p["op"]
    z = 0.0 if mut == "assign" else 1.0
    if op == "scale_rows":
        s = inp["s"].roll(-1) if mut == "s_next" else inp["s"]
        return inp["x"] * s[:, None]
    if op == "add_rows":
        return z * inp["dst0"].float() + inp["src"]
    if op == "add_bf16":
        return inp["a"].float() + z * inp["b"].float()
    return z * inp["x0"] + inp["s"].float()


def _elem_outs(op):
    return {"scale_rows": {"y": BF16, "yf": F32}, "add_rows": {"dst": BF16}, "add_bf16": {"out": BF16}, "acc_bf16": {"x": F32}}[op]


def elem_expected(case, inp, got=None):
    v = _elem_f32(case, inp)
    return {k: (v.to(dt).double(), torch.zeros(v.shape, dtype=F64)) for k, dt in _elem_outs(case.p["op"]).items()}


def elem_emulate(case, inp, mut=None):
    v = _elem_f32(case, inp, mut)
    return {k: (_truncate(v) if mut == "truncate" and dt == BF16 else v.to(dt)) for k, dt in _elem_outs(case.p["op"]).items()}


def elem_launch(ctx, case, inp, rec):
    p, dev, ops = case.p, ctx.dev, ctx.ops
    R, C, op = p["R"], p["C"], p["op"]
    d = {k: v.to(dev) for k, v in inp.items()}
    outs, bufs = {}, {}
    if op == "scale_rows":
        outs["y"], bufs["y"] = _dense_out(R, C, BF16, dev)
        outs["yf"], bufs["yf"] = _dense_out(R, C, F32, dev)
        ops.scale_rows(d["x"], d["s"], outs["y"], outs["yf"])
    elif op == "add_rows":
        outs["dst"], bufs["dst"] = _padded(R, C, BF16, dev)
        outs["dst"].copy_(d["dst0"])
        ops.add_rows(outs["dst"], outs["dst"].stride(0), d["src"])
    elif op == "add_bf16":
        outs["out"], bufs["out"] = _padded(R, C, BF16, dev)
        ops.add_bf16(_nan_in(inp["a"], dev), _nan_in(inp["b"], dev, 16), outs["out"])
    else:
        outs["x"], bufs["x"] = _dense_out(R, C, F32, dev)
        outs["x"].copy_(d["x0"])
        ops.acc_bf16(outs["x"], _nan_in(inp["s"], dev))
    _collect(rec, outs, bufs, {k: (R, C) for k in outs})
    return _cpu(outs)


KINDS["elem"] = (elem_inputs, elem_expected, elem_emulate, elem_launch, ("truncate", "assign", "s_next"))


# ------------------------------------------------------------------ the case table ------------------------------------------
LN_D = (4, 252, 256, 260, 512, 768, 1024, 1028, 1280, 2048)       # NC 1 1 1 2 2 3 4 8 8 8
LN_D_CORE = (4, 260, 768, 1028)
LN_ROWS = (1, 3, 4, 5, 2 * 197)
STAT_KINDS = ("ln_bwd", "ln_fsum", "ln_gb", "embed_bwd")
NC_KINDS = ("ln_fwd", "embed_ln", "ln_bwd", "ln_fsum", "embed_bwd")
DPARAM_ROWS = (1, 12, 13, 16, 17, 29, 8192, 8193)
GB_ROWS = (1, 15, 16, 17, 33, 16384 + 1)
FSUM_NTOK = (1, 3, 13, 14, 197, 257)
FRAME_NTOK = (1, 4, 28, 29, 32, 33, 61, 197)
COLSUM_M = (1, 63, 64, 65, 2048, 2049, 5000)
COLSUM_C = (8, 24, 768, 2048, 2056, 20)


def cases():
    out = []

    def add(kind, name, p, family="unit", eps=1e-5):
        out.append(Case(f"{kind}/{name}/{family}/eps{eps:g}", kind, p, family, eps, 5000 + len(out)))

    # ---- forward
    for D in LN_D:
        for rows in LN_ROWS:
            if rows in (1, 5) or D in LN_D_CORE:
                add("ln_fwd", f"f32/D{D}/r{rows}", dict(variant="f32", rows=rows, D=D))
        for var in ("x16", "fp8"):
            add("ln_fwd", f"{var}/D{D}/r5", dict(variant=var, rows=5, D=D))
    for D in LN_D_CORE + (2048,):
        for fam in ("unit", "offset", "scaled", "const"):
            for eps in EPS:
                if (fam, eps) != ("unit", 1e-5):
                    add("ln_fwd", f"f32/D{D}/r5", dict(variant="f32", rows=5, D=D), fam, eps)
    for var in ("x16", "fp8"):
        for fam in ("offset", "scaled", "const"):
            add("ln_fwd", f"{var}/D768/r5", dict(variant=var, rows=5, D=768), fam, 1e-6)
    for D in LN_D:
        add("embed_ln", f"B2T3N3/D{D}", dict(B=2, T=3, N=3, D=D))
    for fam in ("offset", "const"):
        add("embed_ln", "B2T3N3/D260", dict(B=2, T=3, N=3, D=260), fam, 1e-6)
    add("embed_ln", "B1T2N198/D768", dict(B=1, T=2, N=198, D=768), "unit", 1e-6)
    # ---- backward
    pairs = (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"), ("f32", None), ("bf16", None))
    for D in LN_D_CORE:
        for i, (dy, dres) in enumerate(pairs):
            add("ln_bwd", f"strided/{dy}+{dres}/D{D}/r5", dict(form="strided", rows=5, D=D, dy=dy, dres=dres,
                                                              outs=("dx", "dxb", "both")[i % 3]))
        for outs in ("dx", "dxb", "both"):
            add("ln_bwd", f"strided/bf16+bf16/{outs}/D{D}/r5", dict(form="strided", rows=5, D=D, dy="bf16", dres="bf16", outs=outs,
                                                                  stats="b"))
        add("ln_bwd", f"dense/f32+None/dx/D{D}/r5", dict(form="dense", rows=5, D=D, dy="f32", dres=None, outs="dx"))
        add("ln_bwd", f"classrow/bf16+bf16/D{D}", dict(form="classrow", BT=3, N=3, D=D, dy="bf16", dres="bf16", outs="dxb"))
        add("ln_bwd", f"classrow/bf16+f32/D{D}", dict(form="classrow", BT=3, N=3, D=D, dy="bf16", dres="f32", outs="dxb"))
        add("ln_bwd", f"zshift/bf16+None/D{D}", dict(form="zshift", BT=3, N=4, D=D, dy="bf16", dres=None, outs="dxb"))
    for D in (252, 256, 512, 1024, 1280, 2048):
        add("ln_bwd", f"strided/bf16+bf16/D{D}/r5", dict(form="strided", rows=5, D=D, dy="bf16", dres="bf16", outs="dxb"))
    for rows in (1, 3, 4, 2 * 197):
        add("ln_bwd", f"strided/bf16+bf16/D768/r{rows}", dict(form="strided", rows=rows, D=768, dy="bf16", dres="bf16", outs="both"))
    for D in (260, 768):
        for fam in ("offset", "scaled", "const", "zero_dy"):
            for eps, stats in ((1e-5, "a"), (1e-6, "b")):
                add("ln_bwd", f"strided/bf16+bf16/D{D}/r5/{stats}", dict(form="strided", rows=5, D=D, dy="bf16", dres="bf16",
                                                                       outs="both", stats=stats), fam, eps)
        add("ln_bwd", f"strided/f32+f32/D{D}/r5", dict(form="strided", rows=5, D=D, dy="f32", dres="f32", outs="both"), "zero_dy")
        add("ln_bwd", f"dense/f32+None/D{D}/r5", dict(form="dense", rows=5, D=D, dy="f32", dres=None, outs="dx"), "zero_dy")
    for rows in DPARAM_ROWS:
        for dy in ("f32", "bf16"):
            D = 64 if rows > 100 else (260 if dy == "f32" else 768)
            add("ln_bwd", f"dparam/{dy}/D{D}/r{rows}", dict(form="strided", rows=rows, D=D, dy=dy, dres=None, outs="dx", dparam=True,
                                                          stats="b" if rows == 13 else "a"))
    add("ln_bwd", "dparam/bf16/D260/r13", dict(form="strided", rows=13, D=260, dy="bf16", dres="bf16", outs="dxb", dparam=True),
        "zero_dy")
    add("ln_bwd", "dparam/f32/D1028/r17", dict(form="dense", rows=17, D=1028, dy="f32", dres=None, outs="dx", dparam=True), "offset")
    # ---- layernorm_bwd_fsum
    for ntok in FSUM_NTOK:
        add("ln_fsum", f"F3/n{ntok}/G13/D260", dict(frames=3, ntok=ntok, groups=13, D=260, w="zeros"))
    for G in (1, 4):
        add("ln_fsum", f"F3/n14/G{G}/D260", dict(frames=3, ntok=14, groups=G, D=260, w="zeros"))
    add("ln_fsum", "F1/n197/G13/D768", dict(frames=1, ntok=197, groups=13, D=768, w="none"))
    for D in (4, 512, 768, 1024, 1028):
        add("ln_fsum", f"F3/n14/G13/D{D}", dict(frames=3, ntok=14, groups=13, D=D, w="none" if D == 512 else "zeros", stats="b"))
    for fam in ("offset", "scaled", "zero_dy"):
        add("ln_fsum", "F3/n14/G13/D260", dict(frames=3, ntok=14, groups=13, D=260, w="zeros"), fam, 1e-6)
    # ---- layernorm_gb_bwd
    for rows in GB_ROWS:
        for dy in ("f32", "bf16"):
            add("ln_gb", f"{dy}/D64/r{rows}", dict(rows=rows, D=64, dy=dy, which="both"))
    add("ln_gb", "bf16/D1028/r33", dict(rows=33, D=1028, dy="bf16", which="both", stats="b"))
    add("ln_gb", "bf16/D260/r33/strided", dict(rows=33, D=260, dy="bf16", which="both", strided=True))
    for which in ("dgamma", "dbeta"):
        add("ln_gb", f"f32/D260/r17/{which}", dict(rows=17, D=260, dy="f32", which=which))
    for fam in ("offset", "zero_dy"):
        add("ln_gb", "f32/D260/r33", dict(rows=33, D=260, dy="f32", which="both"), fam, 1e-6)
    # ---- frame_sum
    for ntok in FRAME_NTOK:
        for xt in ("f32", "bf16"):
            add("frame_sum", f"{xt}/F3/n{ntok}/D260", dict(frames=3, ntok=ntok, D=260, x=xt, w=True))
    add("frame_sum", "f32/F3/n33/D260/now", dict(frames=3, ntok=33, D=260, x="f32", w=False))
    add("frame_sum", "bf16/F1/n1970/D768", dict(frames=1, ntok=1970, D=768, x="bf16", w=False))
    add("frame_sum", "f32/F2/n13/D4", dict(frames=2, ntok=13, D=4, x="f32", w=False))
    add("frame_sum", "f32/F2/n5/D6144", dict(frames=2, ntok=5, D=6144, x="f32", w=True))
    add("frame_sum", "f32/F3/n33/D260", dict(frames=3, ntok=33, D=260, x="f32", w=True), "offset")
    # ---- colsum: every route, both sides of its thresholds
    for M in COLSUM_M:
        for ws in ("exact", "none"):
            add("colsum", f"M{M}/C24/{ws}", dict(M=M, C=24, ws=ws, af=True, at=True, ntok=7))
    for C in (8, 768, 2048):
        for M, ws in ((65, "exact"), (65, "none"), (2049, "exact"), (2049, "none")):
            add("colsum", f"M{M}/C{C}/{ws}", dict(M=M, C=C, ws=ws, at=True, ntok=7))
    add("colsum", "M5000/C2048/exact", dict(M=5000, C=2048, ws="exact"))
    add("colsum", "M5000/C768/short", dict(M=5000, C=768, ws="short", af=True, ntok=197))
    add("colsum", "M65/C24/short", dict(M=65, C=24, ws="short"))
    for C, ldx in ((20, 0), (2056, 0), (24, 28)):
        for M in (1, 65, 5000):
            add("colsum", f"M{M}/C{C}/ldx{ldx}/exact", dict(M=M, C=C, ldx=ldx, ws="exact", af=True, at=True, ntok=7))
    add("colsum", "M2049/C24/ldx32/exact", dict(M=2049, C=24, ldx=32, ws="exact", af=True, ntok=7))
    add("colsum", "M65/C768/exact", dict(M=65, C=768, ws="exact", af=True, at=True, ntok=7), "offset")
    # ---- embed_bwd: chunks below / at / above ceil(2048 / T); the finish loop's seam at 28 | 29 chunks
    for B, T, N in ((31, 64, 4), (32, 64, 4), (33, 64, 4), (33, 62, 4), (29, 2, 4), (28, 2, 4), (1, 2, 4), (2, 3, 2)):
        for dx, ws in (("f32", True), ("bf16", False)):
            add("embed_bwd", f"B{B}T{T}N{N}/D64/{dx}/ws{int(ws)}", dict(B=B, T=T, N=N, D=64, dx=dx, ws=ws))
    for D in (4, 260, 512, 768, 1024, 1028):
        add("embed_bwd", f"B2T3N3/D{D}/bf16/ws1", dict(B=2, T=3, N=3, D=D, dx="bf16", ws=True, stats="b"))
    add("embed_bwd", "B29T2N4/D64/bf16/ws1", dict(B=29, T=2, N=4, D=64, dx="bf16", ws=True))
    add("embed_bwd", "B2T3N3/D260/f32/ws0", dict(B=2, T=3, N=3, D=260, dx="f32", ws=False))
    for fam in ("offset", "zero_dy"):
        add("embed_bwd", "B2T3N3/D260/f32/ws1", dict(B=2, T=3, N=3, D=260, dx="f32", ws=True), fam, 1e-6)
    # ---- embed_nopre
    for D in (4, 260, 1028):
        add("nopre_fwd", f"B2T3N3/D{D}", dict(B=2, T=3, N=3, D=D))
    for dx in ("f32", "bf16"):
        add("nopre_bwd", f"B2T3N5/D260/{dx}/all", dict(B=2, T=3, N=5, D=260, dx=dx, outs=NOPRE_OUTS))
        for k in NOPRE_OUTS:
            add("nopre_bwd", f"B2T3N5/D260/{dx}/{k}", dict(B=2, T=3, N=5, D=260, dx=dx, outs=(k,)))
    add("nopre_bwd", "B2T3N5/D1028/bf16/all", dict(B=2, T=3, N=5, D=1028, dx="bf16", outs=NOPRE_OUTS))
    # ---- casts and row operations
    for R, C in CAST_SHAPES:
        for mode in CAST_MODES:
            add("cast", f"{R}x{C}/{mode}", dict(R=R, C=C, mode=mode))
    add("cast_multi", "table", {})
    for op in ("scale_rows", "add_rows", "add_bf16", "acc_bf16"):
        for R, C in ((1, 8), (5, 24), (300, 40)):
            add("elem", f"{op}/{R}x{C}", dict(op=op, R=R, C=C))
    return out


# ------------------------------------------------------------------ running -------------------------------------------------
def build_inputs(case):
    inp = KINDS[case.kind][0](case)
    if case.kind in STAT_KINDS:
        inp["mean"], inp["rstd"] = _bwd_stats(case, inp, own=case.p.get("stats") == "b")
    return inp


def _as_f64(t):
    return (t.float() if t.dtype == FP8 else t).double()


def compare(case, inp, got) -> Dict[str, float]:
    exp = KINDS[case.kind][1](case, inp, got)
    assert set(exp) == set(got), (case.name, sorted(exp), sorted(got))
    return {k: ratio(_as_f64(got[k]).reshape(exp[k][0].shape), *exp[k]) for k in exp}


def emulate(case, inp, mut=None):
    return KINDS[case.kind][2](case, inp, mut)


def mutants(case):
    return KINDS[case.kind][4]


class _Ctx:
    def __init__(self, dev):
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from aim_amd import ops
        from aim_amd.lib import check, load_library
        self.ops, self.lib, self.check, self.stream, self.dev = ops, load_library(), check, ops._stream, torch.device(dev)


_FATAL = ("illegal memory access", "HIP error", "hipError", "unspecified launch failure")


def run_case(ctx, case):
    rec = {"kind": case.kind, "checks": {}, "finite": {}, "pad": {}, "ident": {}, "evidence": {}, "route": None}
    inp = build_inputs(case)
    if case.kind in STAT_KINDS and case.p.get("stats") == "b":        # the forward kernel's own statistics
        x = inp["x"].to(ctx.dev)
        M, D = x.shape
        mean, rstd, y = torch.empty(M, device=ctx.dev), torch.empty(M, device=ctx.dev), torch.empty((M, D), device=ctx.dev)
        G = inp["gamma"].to(ctx.dev)
        ctx.ops.layernorm_fwd(x, G, torch.zeros_like(G), M, D, D, y_f32=y, mean=mean, rstd=rstd, eps=case.eps)
        inp["mean"], inp["rstd"] = mean.cpu(), rstd.cpu()
    got = KINDS[case.kind][3](ctx, case, inp, rec)
    torch.cuda.synchronize()
    rec["checks"] = compare(case, inp, got)
    rec["hash"] = {k: _digest(v.view(torch.uint8) if v.dtype == FP8 else v) for k, v in got.items()}
    return rec


def run_large(ctx):
    """layernorm_fwd and layernorm_bwd over 2 rows whose stride puts row 1 beyond 2^32 bytes: one uninitialised fp32 buffer,
    x / dy / y / dx at different column offsets; row 1 must give the bits of the same row launched densely"""
    dev, ops, D = ctx.dev, ctx.ops, 260
    ld = 2 ** 30 + 64
    n = ld + 4 * D + 64
    free = torch.cuda.mem_get_info()[0]
    rec = {"ran": False, "need": n * 4, "free": free}
    if free < n * 4 + 2 ** 29:
        return rec
    g = torch.Generator().manual_seed(77)
    x, dy = torch.randn((2, D), generator=g), torch.randn((2, D), generator=g)
    G, B = _gb(D, g)
    Gd, Bd = G.to(dev), B.to(dev)
    buf = torch.empty(n, dtype=F32, device=dev)
    for r in range(2):
        buf[r * ld:r * ld + D] = x[r].to(dev)
        buf[r * ld + D:r * ld + 2 * D] = dy[r].to(dev)
    mean, rstd = torch.empty(2, device=dev), torch.empty(2, device=dev)
    ops.layernorm_fwd(buf, Gd, Bd, 2, D, ld, y_f32=buf[2 * D:], ldy=ld, mean=mean, rstd=rstd)
    ops.layernorm_bwd(buf[D:], buf, Gd, mean, rstd, 2, D, lddy=ld, ldx=ld, lddx=ld, dx=buf[3 * D:])
    y1, dx1 = torch.empty((1, D), device=dev), torch.empty((1, D), device=dev)
    m1, r1 = torch.empty(1, device=dev), torch.empty(1, device=dev)
    ops.layernorm_fwd(x[1:].to(dev), Gd, Bd, 1, D, D, y_f32=y1, mean=m1, rstd=r1)
    ops.layernorm_bwd(dy[1:].to(dev), x[1:].to(dev), Gd, m1, r1, 1, D, lddy=D, ldx=D, lddx=D, dx=dx1)
    torch.cuda.synchronize()
    y = torch.stack([buf[r * ld + 2 * D:r * ld + 3 * D] for r in range(2)]).cpu()
    dx = torch.stack([buf[r * ld + 3 * D:r * ld + 4 * D] for r in range(2)]).cpu()
    e = ln_fwd_expected(x.double(), G.double(), B.double(), 1e-5, ln_nc(D))
    mu, rs = mean.cpu(), rstd.cpu()
    dref, db = ln_bwd_expected(dy.double(), x.double(), G.double(), mu.double()[:, None], rs.double()[:, None], None, ln_nc(D))
    rec.update(ran=True, bytes=(ld + 4 * D) * 4, identical=_bits_eq(y[1:], y1) and _bits_eq(dx[1:], dx1),
               checks={"y": ratio(y, *e["y"]), "mean": ratio(mu, *e["mean"]), "rstd": ratio(rs, *e["rstd"]), "dx": ratio(dx, dref, db)},
               finite={"y": bool(torch.isfinite(y).all()), "dx": bool(torch.isfinite(dx).all())})
    del buf
    return rec


def run_refusals(ctx):
    """calls the library must refuse: {name: (message, every output still untouched)}"""
    dev, ops, lib = ctx.dev, ctx.ops, ctx.lib
    out = {}

    def attempt(name, fn, watched):
        try:
            fn()
            msg = None
        except RuntimeError as e:
            msg = str(e)
        torch.cuda.synchronize()
        out[name] = {"message": msg, "untouched": all(bool(torch.isnan(t).all()) for t in watched)}

    def nanf(*shape, dtype=F32):
        return torch.full(shape, NAN, dtype=dtype, device=dev)

    for D in (2052, 6):
        x, G, y = torch.zeros((4, D + 2), device=dev), torch.ones(D + 2, device=dev), nanf(4, D + 2)
        m, r = nanf(4), nanf(4)
        attempt(f"layernorm_fwd/D{D}", lambda: ops.layernorm_fwd(x, G, G, 4, D, D + 2, y_f32=y, ldy=D + 2, mean=m, rstd=r), (y, m, r))
        dx = nanf(4, D + 2)
        attempt(f"layernorm_bwd/D{D}", lambda: ops.layernorm_bwd(x, x, G, m.nan_to_num(), m.nan_to_num(), 4, D, lddy=D + 2, ldx=D + 2,
                                                                 lddx=D + 2, dx=dx), (dx,))
    D = 64
    x, G, y = torch.zeros((4, D + 2), device=dev), torch.ones(D, device=dev), nanf(4, D + 4)
    z4 = torch.zeros(4, device=dev)
    attempt("layernorm_fwd/ldx%4", lambda: ops.layernorm_fwd(x, G, G, 4, D, D + 2, y_f32=y, ldy=D + 4), (y,))
    attempt("layernorm_fwd/ldy%4", lambda: ops.layernorm_fwd(x, G, G, 4, D, D, y_f32=y, ldy=D + 2), (y,))
    dx, dg = nanf(4, D + 4), nanf(D)
    attempt("layernorm_bwd/lddres%4", lambda: ops.layernorm_bwd(x, x, G, z4, z4, 4, D, lddy=D, ldx=D, lddx=D + 4, dres=x, lddres=D + 2,
                                                               dx=dx), (dx,))
    attempt("layernorm_bwd/dgamma_without_dbeta", lambda: ops.layernorm_bwd(x, x, G, z4, z4, 4, D, lddy=D, ldx=D, lddx=D + 4, dx=dx,
                                                                            dgamma=dg), (dx, dg))
    need = lib.aim_layernorm_gb_bwd_workspace_bytes(33, D)
    ws, db = nanf(need // 4), nanf(D)
    xs = torch.zeros((33, D), device=dev)
    z33 = torch.zeros(33, device=dev)
    attempt("layernorm_gb_bwd/workspace", lambda: ctx.check(lib.aim_layernorm_gb_bwd(
        xs.data_ptr(), 0, D, xs.data_ptr(), D, z33.data_ptr(), z33.data_ptr(), dg.data_ptr(), db.data_ptr(), 33, D, ws.data_ptr(),
        need - 4, ctx.stream()), "aim_layernorm_gb_bwd"), (ws, dg, db))
    B, T, N = 2, 3, 5
    need = lib.aim_embed_nopre_bwd_workspace_bytes(B, T, N, D)
    ws, dpos = nanf(need // 4), nanf(N, D)
    dxs = torch.zeros((B * T * N, D), device=dev)
    attempt("embed_nopre_bwd/workspace", lambda: ctx.check(lib.aim_embed_nopre_bwd(
        dxs.data_ptr(), 0, None, None, dpos.data_ptr(), None, None, B, T, N, D, ws.data_ptr(), need - 4, ctx.stream()),
        "aim_embed_nopre_bwd"), (ws, dpos))
    return out


REFUSAL_TEXT = {"layernorm_fwd/D2052": "bad shape", "layernorm_fwd/D6": "bad shape", "layernorm_bwd/D2052": "bad shape",
                "layernorm_bwd/D6": "bad shape", "layernorm_fwd/ldx%4": "strides must be multiples of 4",
                "layernorm_fwd/ldy%4": "strides must be multiples of 4", "layernorm_bwd/lddres%4": "strides must be multiples of 4",
                "layernorm_bwd/dgamma_without_dbeta": "dgamma and dbeta go together",
                "layernorm_gb_bwd/workspace": "workspace of", "embed_nopre_bwd/workspace": "workspace of"}


def run(dev="cuda"):
    """every case, the large-offset case and the refusals on `dev`: {"cases": {name: record}, "large", "refusals", "seconds"}"""
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
        res["refusals"] = run_refusals(ctx)
        res["large"] = run_large(ctx)
    res["seconds"] = time.time() - t0
    return res
