"""Every call form of the attention kernels (aim_attn_fwd, aim_attn_fwd_fp8, aim_attn_bwd, aim_attn_fwd_cls / aim_attn_bwd_cls,
aim_cls_attn_fwd/bwd, aim_tattn_fwd/bwd, aim_tattn_fwd_infer), float64 closed-form references of their values and gradients,
and bounds derived from the kernels' rounding points.

A plain module (no fixtures): `test_attn_routes_gpu.py` runs `route_cases()` on every route, one child process per route
(`python attn_cases.py ROUTE OUT.json`; the switches are read once per process), `test_attn_lengths_gpu.py` runs
`length_cases()` -- kernels that no route switch reaches, at every length they accept -- in one child and the inference
forms of tattn once more in a child with AIM_TATTN_LDS16=0, and `test_attn_cases_cpu.py` proves on the CPU that the bounds
accept an emulation of the kernels' arithmetic and reject the bugs they are meant to catch.

Kinds.  `spatial`: aim_attn_fwd / _fp8 / aim_attn_bwd.  `clsq`: the class query of the last block, aim_attn_fwd_cls /
aim_attn_bwd_cls (compact out, dO [BT, D] and lse [BT, H]; dO is zero outside the class rows, which is the situation they
are built for).  `cls`: the temporal class-token kernels aim_cls_attn_*.  `tattn`: aim_tattn_*.

Routes.  `default`; `xt0` (AIM_ATTN_PIPE_XT=0: the left-over queries get a tick of their own); `two` (AIM_ATTN_BWD_PIPE=0:
the two-kernel backward at every N); `grid1`, `grid3` (AIM_ATTN_PIPE_GRID: one persistent workgroup walks every item /
three walk unequal shares); `reserve0` (AIM_ATTN_PIPE_RESERVE=0).  `bwd_plan` restates the selection rule of
csrc/attn_bwd.hip::aim_attn_bwd.  What can be proven from outside is proven: `delta` is handed in filled with NaN; the
two-kernel form writes it, the pipelined form leaves it.  Whether the extra-tile form of the pipelined kernel ran, and how
many workgroups walked the items, cannot be seen from outside: there the proof rests on `bwd_plan` being a faithful
restatement, and on test_attn_cases_cpu.py asserting that every branch of it has cases on the routes that select it.

Notation: one item = one (frame, head): q, k, v [N, 64] (bf16 values), z = q k^T / 8, p = softmax(z), O = p v,
lse = log sum exp z; dP = dO v^T, delta = rowsum(dO o O), dS = p o (dP - delta), dQ = dS k / 8, dK = dS^T q / 8, dV = p^T dO.
u = 2^-24 (fp32), U8 = 2^-8: a bf16 result is off by at most 2^-8 of its value (half an ulp).

Bounds of the spatial kernels, from the rounding points of csrc/attn_fwd.hip and csrc/attn_bwd.hip:
  S and dP are fp32 MFMA sums of 64 exact bf16 products:        eS = 2 . 64 u sum |q||k|,  edP = 2 . 64 u sum |dO||v|
  forward: p' = exp2(s C2 - max C2) in fp32, unnormalised (max 1): the exponent carries eS / 8 and three fp32 roundings of
    numbers no larger than |z| + |z|max, v_exp_f32 one ulp more:  rp = eS / 8 + 4 u (|z| + |z|max) + 4 u   (relative)
  p' is rounded to bf16, O accumulates in fp32 over the keys (2 N u), is scaled by 1 / sum (a sum of N fp32 terms, each off
    by rp: (N / 4 + 16) u + the p-weighted mean of rp =: rsum) and rounded once:
      |out - O| <= U8 A + E + U8 (|O| + U8 A + E),   A = sum_j p_j |v_j|,   E = sum_j p_j rp_j |v_j| + 2 N u A + rsum |O|
    (the same first-order shape as normalising before the rounding).  fp8 output: the last rounding is e4m3 of the fp32
    value: half an ulp is 2^-4 relative, 2^-10 absolute below 2^-6, saturating at +-448.
  lse = max / 8 + logf(sum) in fp32:   |lse' - lse| <= sum_j p_j rp_j + (N / 4 + 16) u + 32 u + 4 u (|lse| + |z|max)
  backward: p' = exp2(s C2 - lse log2e) in fp32:  rp = eS / 8 + elog + 4 u (|z| + |lse|) + 4 u, with elog the error of the
    lse it is given; delta' = fp32 rowsum(dO o out) of the bf16 `out` it is given: edelta = sum_d |dO| eout + 66 u sum |dO||O|.
    Form (a) hands in out = bf16(O), lse = fp32(lse): eout = U8 |O|, elog = u |lse|.  Form (b) hands in the forward kernel's
    own results: eout, elog are the forward bounds above.
    P = bf16(p') for dV, dS' = bf16(p' (dP' - delta')) for dQ and dK, 1/8 applied once in fp32, results rounded to bf16:
      ePb = p (U8 + (1 + U8) rp)
      eDS = U8 |dS| + (1 + U8) p (rp |dP - delta| + edP + edelta) + 2 u |dS|
      |dQ' - dQ| <= U8 |dQ| + (1 + U8) (sum_j eDS |k_j| + 2 N u sum_j |dS||k_j|) / 8        (dK alike, over the queries)
      |dV' - dV| <= U8 |dV| + (1 + U8) (sum_i ePb |dO_i| + 2 N u sum_i p |dO_i|)
clsq: the spatial references and bounds above with a dO that is zero outside the class rows, restricted to query row 0 for
    out, lse and dq and taken over every key for dk and dv.  The kernels' arithmetic for that query is the full kernels' (the
    forward is the full kernel's first query tile; the backward runs the dq kernel's key-pair step on a tile whose other
    fifteen queries are zero, and a key's dK = bf16(dS) q / 8, dV = bf16(p) dO are single exact products where the matrix
    kernels hold fp32 sums of one non-zero term), so no rounding point is added and the bounds carry over unchanged.
cls_attn / tattn keep fp32 probabilities (sequence T <= 32): z is an fp32 sum of 64 products, expf and one division:
      ep = p (2 . 64 u sum |q||k| / 8 . 2 + (T + 16) u);   out: U8 |O| + sum ep |v| + 2 T u A
    the backward takes the probabilities it is given (fp32 of the float64 ones, or the forward kernel's) and stays in fp32
    up to the one bf16 rounding of dq, dk, dv (cls_attn non-compact: of dqkv + d).
aim_tattn_fwd_infer: the bf16 form has the bits of aim_tattn_fwd's `out` (itself held to float64 above); every byte of the
    fp8 form is the e4m3 cast of the float64 result or its neighbour on the grid, and over all T of one (geometry, family)
    at most 1e-3 of the bytes are neighbours (test_aim_fp8_gpu.py's cap; its argument: an fp32 sum over T <= 32 terms errs by
    ~2e-6 relative and e4m3's rounding boundaries lie 2^-4 .. 2^-3 apart, so ~6e-5 of the values may flip).  Pooled because
    the smallest cases have fewer than 1000 bytes, where the cap would allow no neighbour at all.
"""
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # the repository root: oracle, aim_amd
from gemm_cases import U8, U24, _digest, _pad_intact, _padded, ratio  # noqa: E402

BF16, F32, F64, FP8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
_BITS = {BF16: torch.int16, F32: torch.int32}
NMAX = 288
ROUTES = ("default", "xt0", "two", "grid1", "grid3", "reserve0")
ROUTE_ENV = {"default": {}, "xt0": {"AIM_ATTN_PIPE_XT": "0"}, "two": {"AIM_ATTN_BWD_PIPE": "0"},
             "grid1": {"AIM_ATTN_PIPE_GRID": "1"}, "grid3": {"AIM_ATTN_PIPE_GRID": "3"},
             "reserve0": {"AIM_ATTN_PIPE_RESERVE": "0"}}
ROUTE_VARS = ("AIM_ATTN_PIPE_XT", "AIM_ATTN_BWD_PIPE", "AIM_ATTN_PIPE_GRID", "AIM_ATTN_PIPE_RESERVE")
FAMILIES = ("unit", "peaked", "cls_sink", "diag", "neg40", "neg100", "zero_do")
PRODUCT = ((197, 12), (257, 16))
PRODUCT_BT = (1, 2, 9)
SWEEP_BT, SWEEP_H = 2, 2
FAMILY_STRIDE = 7                      # the other families on every 7th N of the sweep (all residues mod 32 and mod 64)
SMALL_SHAPES = ((8, 8, 197, 12), (2, 32, 257, 16), (3, 1, 197, 12), (1, 31, 5, 2), (2, 16, 197, 12))    # B, T, N, H
CLSQ_SHAPES = ((16, 197, 12), (8, 257, 16), (4, 5, 2), (1, 288, 1), (3, 64, 1))                         # BT, N, H
TMAX = 32
# B, N, H of the sweep over T = 1 .. 32.  tattn runs one wave per (b, n, h) item, 4 waves per workgroup up to T = 16 and 2
# above: 3 and 30 items leave a partial last workgroup at 4 waves (3 % 4, 30 % 4) and at 2 (3 % 2).  cls_attn runs one
# 64-thread workgroup per (b, h) at every T: it has one wave count and no partial workgroup.
SWEEP_GEOMS = ((1, 3, 1), (2, 5, 3))
LENGTH_MODES = ("lengths", "lds32")          # children of test_attn_lengths_gpu.py
LENGTH_ENV = {"lengths": {}, "lds32": {"AIM_TATTN_LDS16": "0"}}
INFER_CAP = 1e-3                             # share of fp8 bytes that may be the neighbour of the float64 cast, per pool
SAT_T = (17, 32)                             # |v| = 600 saturates to +-448 on either side of the 4 / 2 wave switch


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                 # spatial | clsq | cls | tattn
    BT: int
    N: int
    H: int
    family: str = "unit"
    seed: int = 0
    B: int = 0                # cls / tattn: clips, frames per clip (BT = B T)
    T: int = 0
    alone: bool = False       # spatial: every frame also launched alone, must give the same bits
    poison: bool = False      # spatial: the frame / head independence case (BT = 3)
    sweep: bool = False       # cls / tattn: a case of the sweep over T (tattn: also run through aim_tattn_fwd_infer)


def tattn_wpb(T: int) -> int:
    """Mirror of csrc/tattn.hip: waves (items) per workgroup of aim_tattn_fwd / _infer / _bwd"""
    return 4 if T <= 16 else 2


def route_cases():
    """what every route of the spatial backward runs (test_attn_routes_gpu.py)"""
    out, seed = [], 1000
    for N, H in PRODUCT:
        for BT in PRODUCT_BT:
            for fam in FAMILIES:
                out.append(Case(f"attn/{N}x{H}/BT{BT}/{fam}", "spatial", BT, N, H, fam, seed, alone=BT == 9 and fam == "unit"))
                seed += 1
    for fam in FAMILIES:
        out.append(Case(f"attn/5x2/BT4/{fam}", "spatial", 4, 5, 2, fam, seed))
        seed += 1
    for N in range(1, NMAX + 1):
        fams = FAMILIES if N % FAMILY_STRIDE == 1 else ("unit",)
        for fam in fams:
            out.append(Case(f"attn/sweep/N{N}/{fam}", "spatial", SWEEP_BT, N, SWEEP_H, fam, seed))
            seed += 1
    for N, H in PRODUCT + ((5, 2),):
        out.append(Case(f"attn/{N}x{H}/independence", "spatial", 3, N, H, "unit", seed, poison=True))
        seed += 1
    for B, T, N, H in SMALL_SHAPES:
        for kind in ("cls", "tattn"):
            for fam in ("unit", "peaked"):
                out.append(Case(f"{kind}/B{B}T{T}N{N}H{H}/{fam}", kind, B * T, N, H, fam, seed, B=B, T=T))
                seed += 1
    return out


def length_cases():
    """the kernels no route switch reaches, at every length they accept (test_attn_lengths_gpu.py)"""
    out, seed = [], 5000
    for BT, N, H in CLSQ_SHAPES:
        for fam in FAMILIES:
            out.append(Case(f"clsq/{N}x{H}/BT{BT}/{fam}", "clsq", BT, N, H, fam, seed))
            seed += 1
    for N in range(1, NMAX + 1):
        fams = FAMILIES if N % FAMILY_STRIDE == 1 else ("unit",)
        for fam in fams:
            out.append(Case(f"clsq/sweep/N{N}/{fam}", "clsq", SWEEP_BT, N, SWEEP_H, fam, seed))
            seed += 1
    for B, N, H in SWEEP_GEOMS:
        for T in range(1, TMAX + 1):
            for kind in ("cls", "tattn"):
                for fam in ("unit", "peaked"):
                    out.append(Case(f"{kind}/sweep/B{B}N{N}H{H}/T{T}/{fam}", kind, B * T, N, H, fam, seed, B=B, T=T, sweep=True))
                    seed += 1
    return out


def cases():
    return route_cases() + length_cases()


def bwd_plan(N: int, route: str):
    """Mirror of the selection in csrc/attn_bwd.hip::aim_attn_bwd under `route`'s environment:
    ("two", False) or ("pipe", extra tile)."""
    if route == "two" or not 65 <= N <= 224:
        return ("two", False)
    xt = route != "xt0" and N >= 129 and ((N - 1) & 63) < 16
    return ("pipe", xt)


def pipe_grid(items: int, cus: int, route: str) -> int:
    """workgroups of the persistent pipelined kernel (same function)"""
    reserve = 0 if route == "reserve0" else 32
    if reserve > 0 and items > cus - reserve and cus - reserve >= 8:
        cus -= reserve
    cap = {"grid1": 1, "grid3": 3}.get(route, 0)
    if 0 < cap < cus:
        cus = cap
    return min(items, cus)


def fwd_plan(N: int):
    """Mirror of csrc/attn_fwd.hip::aim_attn_fwd: (key tiles of the LDS image, tiles known to lie below N)."""
    nkt = 2 if N <= 32 else 4 if N <= 64 else 14 if N <= 224 else 18
    return nkt, (nkt - 2 if (N >> 4) >= nkt - 2 else 0)


# ------------------------------------------------------------------ inputs (CPU, fixed seeds) ------------------------------
SINK_ROWS = 3            # neg40 / neg100: every third query row (and the last one) is anti-aligned


def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    """qkv [BT N, 3 D] and dO [BT N, D] as bf16, frame-major rows, heads side by side: the product's layout"""
    g = torch.Generator().manual_seed(case.seed)
    BT, N, H, fam = case.BT, case.N, case.H, case.family
    q, k, v = (torch.randn((BT, N, H, 64), generator=g) for _ in range(3))
    do = torch.randn((BT, N, H, 64), generator=g)
    if case.kind in ("cls", "tattn"):
        sc = 2.5 if fam == "peaked" else 0.8
        q, k = q * sc, k * sc
    elif fam == "peaked":
        q, k = q * 2.5, k * 2.5
    elif fam == "cls_sink":             # u = ones / 8: q.u ~ 8, k_0 = 16 u -> z_i0 ~ 16, every other logit ~ +-2
        q = 0.5 * q + 1.0
        k = 0.5 * k
        k[:, 0] = 2.0
    elif fam == "diag":
        k = q.clone()
    elif fam in ("neg40", "neg100"):    # k = small noise + 8 u; chosen rows q = noise - c u: every logit ~ -c
        c = 5.0 if fam == "neg40" else 13.0
        k = 0.1 * k + 1.0
        q = 0.5 * q
        rows = torch.zeros(N, dtype=torch.bool)
        rows[::SINK_ROWS] = True
        rows[-1] = True
        q[:, rows] = q[:, rows] - c
    elif fam == "zero_do":
        do[:, :, min(1, H - 1)] = 0.0
    D = H * 64
    qkv = torch.cat([t.reshape(BT * N, D) for t in (q, k, v)], dim=1).to(BF16)
    return {"qkv": qkv, "do": do.reshape(BT * N, D).to(BF16)}


def sink_rows(N: int):
    rows = torch.zeros(N, dtype=torch.bool)
    rows[::SINK_ROWS] = True
    rows[-1] = True
    return rows


def split(x, BT, N, H, parts=1):
    """[BT N, parts D] rows -> `parts` tensors [BT, H, N, 64] (float64)"""
    t = x.double().reshape(BT, N, parts, H, 64).permute(2, 0, 3, 1, 4)
    return [t[i] for i in range(parts)] if parts > 1 else t[0]


def merge(*ts):
    """[BT, H, N, 64] tensors -> [BT N, len(ts) D] rows"""
    BT, H, N, _ = ts[0].shape
    return torch.stack(ts, dim=0).permute(1, 3, 0, 2, 4).reshape(BT * N, len(ts) * H * 64)


# ------------------------------------------------------------------ float64 references and bounds: spatial -----------------
def forward_ref(q, k, v):
    """float64 forward of items [..., N, 64] and the bounds of `out`, `out8`, `lse` -> dict name: (ref, bound), plus parts"""
    N = q.shape[-2]
    z = q @ k.transpose(-1, -2) / 8.0
    eS = 2 * 64 * U24 * (q.abs() @ k.abs().transpose(-1, -2))
    lse = torch.logsumexp(z, dim=-1)
    p = torch.exp(z - lse[..., None])
    O = p @ v
    zmax = z.abs().amax(dim=-1, keepdim=True)
    rp = eS / 8 + 4 * U24 * (z.abs() + zmax) + 4 * U24
    A = p @ v.abs()
    wrp = (p * rp).sum(dim=-1)
    rsum = (N / 4 + 16) * U24 + wrp
    E = (p * rp) @ v.abs() + 2 * N * U24 * A + rsum[..., None] * O.abs()
    b_out = U8 * A + E + U8 * (O.abs() + U8 * A + E)
    O8 = O.clamp(-448.0, 448.0)
    b_out8 = U8 * A + E + torch.maximum(2.0 ** -4 * (O8.abs() + U8 * A + E), torch.full_like(O, 2.0 ** -10))
    b_lse = wrp + (N / 4 + 16) * U24 + 32 * U24 + 4 * U24 * (lse.abs() + zmax[..., 0])
    return {"out": (O, b_out), "out8": (O8, b_out8), "lse": (lse, b_lse), "_z": z, "_p": p, "_eS": eS}


def backward_ref(q, k, v, do, fw, eout, elog):
    """float64 gradients (closed form) and their bounds, given the error bounds of the `out` and `lse` handed to the kernel"""
    N = q.shape[-2]
    z, p, eS = fw["_z"], fw["_p"], fw["_eS"]
    O, lse = fw["out"][0], fw["lse"][0]
    dP = do @ v.transpose(-1, -2)
    edP = 2 * 64 * U24 * (do.abs() @ v.abs().transpose(-1, -2))
    delta = (do * O).sum(dim=-1, keepdim=True)
    edelta = (do.abs() * eout).sum(dim=-1, keepdim=True) + 66 * U24 * (do.abs() * O.abs()).sum(dim=-1, keepdim=True)
    dS = p * (dP - delta)
    rp = eS / 8 + elog[..., None] + 4 * U24 * (z.abs() + lse.abs()[..., None]) + 4 * U24
    ePb = p * (U8 + (1 + U8) * rp)
    eDS = U8 * dS.abs() + (1 + U8) * p * (rp * (dP - delta).abs() + edP + edelta) + 2 * U24 * dS.abs()
    dQ, dK, dV = dS @ k / 8, dS.transpose(-1, -2) @ q / 8, p.transpose(-1, -2) @ do
    acc = 2 * N * U24
    bQ = U8 * dQ.abs() + (1 + U8) * (eDS @ k.abs() + acc * (dS.abs() @ k.abs())) / 8
    bK = U8 * dK.abs() + (1 + U8) * (eDS.transpose(-1, -2) @ q.abs() + acc * (dS.abs().transpose(-1, -2) @ q.abs())) / 8
    bV = U8 * dV.abs() + (1 + U8) * (ePb.transpose(-1, -2) @ do.abs() + acc * (p.transpose(-1, -2) @ do.abs()))
    return {"dq": (dQ, bQ), "dk": (dK, bK), "dv": (dV, bV)}


def handed_in(fw):
    """form (a): what the backward is given when it is judged alone, and the error bounds of those inputs"""
    O, lse = fw["out"][0], fw["lse"][0]
    return O.to(BF16), lse.to(F32), U8 * O.abs(), U24 * lse.abs()


def spatial_expected(case: Case, inp):
    """-> (forward dict, backward dict of form a, backward dict of form b); references as [BT, H, N, 64] / [BT, H, N]"""
    q, k, v = split(inp["qkv"], case.BT, case.N, case.H, 3)
    do = split(inp["do"], case.BT, case.N, case.H)
    fw = forward_ref(q, k, v)
    _, _, eo, el = handed_in(fw)
    bw_a = backward_ref(q, k, v, do, fw, eo, el)
    bw_b = backward_ref(q, k, v, do, fw, fw["out"][1], fw["lse"][1])
    return fw, bw_a, bw_b


def emulate(case: Case, inp, mut: Optional[str] = None, own: bool = False):
    """The kernels' arithmetic restated in float64 with their rounding points inserted (fp32 scores and probabilities,
    bf16 P and dS, one final rounding); `mut` inserts one defect (MUTANTS).  own: the backward takes the emulated forward's
    out and lse (form b) instead of the rounded float64 ones (form a).  -> dict of [BT, H, N, ...] tensors"""
    BT, N, H = case.BT, case.N, case.H
    q, k, v = split(inp["qkv"], BT, N, H, 3)
    do = split(inp["do"], BT, N, H)
    r32 = lambda t: t.to(F32).double()
    r16 = lambda t: t.to(F32).to(BF16).double()
    s = r32(q @ k.transpose(-1, -2))
    z = s / 8
    mx = z.amax(dim=-1, keepdim=True)
    if mut == "pad_key":                            # one zero-filled key past N takes part in the softmax
        mx = mx.clamp_min(0.0)
    pu = r32(torch.exp(z - mx))
    if mut == "last_key_last_tile":                 # the last 16-query tile does not see the last key
        pu[..., 16 * ((N - 1) // 16):, N - 1] = 0.0
    tot = pu.sum(dim=-1, keepdim=True) + (torch.exp(-mx) if mut == "pad_key" else 0.0)
    lse = r32(mx + torch.log(r32(tot)))[..., 0]
    o32 = r32(r32(r16(pu) @ v) / tot)
    if mut == "out_scale":
        o32 = o32 * (1 + 2.0 ** -7)
    got = {"out": o32.to(BF16), "lse": lse.to(F32),
           "out8": o32.clamp(-448, 448).to(F32).to(FP8).to(F32)}
    if own:
        out_in, lse_in = got["out"].double(), got["lse"].double()
    else:
        fw = forward_ref(q, k, v)
        o_, l_, _, _ = handed_in(fw)
        out_in, lse_in = o_.double(), l_.double()
    nxt = lambda t, d: t.roll(-1, dims=d)
    delta = r32((do * out_in).sum(dim=-1, keepdim=True))
    L = lse_in[..., None]
    if mut == "no_delta":
        delta = torch.zeros_like(delta)
    if mut == "delta_next_head":
        delta = nxt(delta, 1)
    if mut == "lse_next_head":
        L = nxt(L, 1)
    if mut == "lse_next_query":
        L = nxt(L, 2)
    pb = r32(torch.exp(z - L))
    dP = r32(do @ v.transpose(-1, -2))
    dsb = r16(pb * (dP - delta))
    dq = r32(dsb @ k) * (1.0 if mut == "dq_no_eighth" else 0.125)
    dk = r32(dsb.transpose(-1, -2) @ q) / 8
    dv = r32(r16(pb).transpose(-1, -2) @ do)
    if mut == "leftover_dq_zero" and 1 <= N % 64 <= 16:
        dq[..., 64 * (N // 64):, :] = 0.0
    if mut == "dkv_next_item":                      # dK, dV of item k stored in item k + 1 (heads are the fast index)
        fl = lambda t: t.reshape(BT * H, N, 64).roll(1, dims=0).reshape(BT, H, N, 64)
        dk, dv = fl(dk), fl(dv)
    got.update(dq=dq.to(BF16), dk=dk.to(BF16), dv=dv.to(BF16))
    return got


FWD_MUTANTS = ("pad_key", "last_key_last_tile", "out_scale")
BWD_MUTANTS = ("no_delta", "delta_next_head", "lse_next_head", "lse_next_query", "dkv_next_item", "dq_no_eighth",
               "leftover_dq_zero")


def compare_spatial(case: Case, inp, got, form: str = "a") -> Dict[str, float]:
    """worst error / bound of every output in `got` ([BT, H, N, ...] tensors); form: which backward bounds apply"""
    fw, bw_a, bw_b = spatial_expected(case, inp)
    exp = dict(fw, **(bw_a if form == "a" else bw_b))
    return {k: ratio(got[k], *exp[k]) for k in got if k in exp}


# ------------------------------------------------------------------ the class query of the last block (clsq) ---------------
def clsq_inputs(case: Case) -> Dict[str, torch.Tensor]:
    """make_inputs with dO zero outside the class rows; the kernels get the compact rows `do_cls` [BT, D]"""
    inp = make_inputs(case)
    D = case.H * 64
    inp["do"].view(case.BT, case.N, D)[:, 1:] = 0
    inp["do_cls"] = inp["do"].view(case.BT, case.N, D)[:, 0].contiguous()
    return inp


def clsq_expected(case: Case, inp):
    """(reference, bound) of out, lse [query row 0] and of dq [row 0], dk, dv [every key] in both backward forms, and what
    form (a) hands in: `_out_a` [BT, D] bf16, `_lse_a` [BT, H] f32"""
    BT, N, H = case.BT, case.N, case.H
    q, k, v = split(inp["qkv"], BT, N, H, 3)
    do = split(inp["do"], BT, N, H)
    fw = forward_ref(q, k, v)
    o_a, l_a, eo, el = handed_in(fw)
    row0 = lambda pair: (pair[0][:, :, 0], pair[1][:, :, 0])
    exp = {"out": row0(fw["out"]), "lse": row0(fw["lse"])}
    for form, (eo_, el_) in (("a", (eo, el)), ("b", (fw["out"][1], fw["lse"][1]))):
        bw = backward_ref(q, k, v, do, fw, eo_, el_)
        exp[f"dq@{form}"], exp[f"dk@{form}"], exp[f"dv@{form}"] = row0(bw["dq"]), bw["dk"], bw["dv"]
    exp["_out_a"] = o_a[:, :, 0].reshape(BT, H * 64).contiguous()
    exp["_lse_a"] = l_a[:, :, 0].contiguous()
    return exp


def compare_clsq(case: Case, exp, got, form: str) -> Dict[str, float]:
    """worst error / bound of out [BT, H, 64], lse [BT, H] and dq, dk, dv [BT, H, N, 64] (those present in `got`)"""
    r = {k: ratio(got[k], *exp[k]) for k in ("out", "lse") if k in got}
    if "dq" in got:
        r["dq"] = ratio(got["dq"][:, :, 0], *exp[f"dq@{form}"])
        r["dk"] = ratio(got["dk"], *exp[f"dk@{form}"])
        r["dv"] = ratio(got["dv"], *exp[f"dv@{form}"])
    return r


def clsq_exact(case: Case, got) -> Dict[str, bool]:
    """the exact properties of one backward result: everything finite, every non-class dQ row zero, a zero_do head zero"""
    dq, dk, dv = got["dq"], got["dk"], got["dv"]
    res = {"finite": bool(all(torch.isfinite(t.float()).all() for t in (dq, dk, dv))),
           "other_dq_zero": bool((dq[:, :, 1:] == 0).all())}
    if case.family == "zero_do":
        h = min(1, case.H - 1)
        res["zero_head"] = bool(all((t[:, h] == 0).all() for t in (dq, dk, dv)))
    return res


CLSQ_MUTANTS = ("lse_transposed", "do_full_stride", "delta_next_head", "dk_no_eighth", "keys_past_64_unwritten",
                "other_dq_untouched", "out_row_stride")


def emulate_clsq(case: Case, inp, mut: Optional[str] = None, own: bool = False, exp=None):
    """aim_attn_fwd_cls / aim_attn_bwd_cls restated in float64 with their rounding points: fp32 scores, exp2 against the max
    (forward) or the lse handed in (backward), delta = dO . O as one fp32 dot, bf16 p and dS, dK = bf16(bf16(dS) q / 8) and
    dV = bf16(bf16(p) dO) as single products, explicit zeros in every other dQ row.  `mut` inserts one defect
    (CLSQ_MUTANTS); what a defect leaves unwritten keeps the NaN the buffers are filled with, what it reads outside the
    compact dO is the NaN around a guarded input.  own: form (b).  -> out [BT, H, 64], lse [BT, H], dq, dk, dv [BT, H, N, 64],
    spare_intact (of `out`, in gemm_cases._padded's layout)"""
    BT, N, H = case.BT, case.N, case.H
    D = H * 64
    exp = exp or clsq_expected(case, inp)
    q, k, v = split(inp["qkv"], BT, N, H, 3)
    q0 = q[:, :, 0]
    do0 = inp["do_cls"].double().reshape(BT, H, 64)
    r32 = lambda t: t.to(F32).double()
    r16 = lambda t: t.to(F32).to(BF16).double()
    nan = float("nan")
    z = r32(torch.einsum("bhd,bhnd->bhn", q0, k)) / 8
    mx = z.amax(dim=-1, keepdim=True)
    pu = r32(torch.exp(z - mx))
    tot = pu.sum(dim=-1, keepdim=True)
    lse = r32(mx + torch.log(r32(tot)))[..., 0]
    out = r32(r32(torch.einsum("bhn,bhnd->bhd", r16(pu), v)) / tot).to(BF16)
    spare_intact = True
    if mut == "out_row_stride":                       # the forward stores frame bt's row at bt N instead of bt
        n = BT * D
        flat = torch.full((n + 8 + 3 * (n + 8),), nan, dtype=F64)
        for bt in range(BT):
            if (bt * N + 1) * D <= flat.numel():      # (past the buffer: nothing the test can look at)
                flat[bt * N * D:(bt * N + 1) * D] = out[bt].double().reshape(D)
        out, spare_intact = flat[:n].reshape(BT, H, 64).to(BF16), bool(torch.isnan(flat[n:]).all())
    got = {"out": out, "lse": lse.to(F32), "spare_intact": spare_intact}
    if own:
        out_in, lse_in = out.double(), got["lse"].double()
    else:
        out_in, lse_in = exp["_out_a"].double().reshape(BT, H, 64), exp["_lse_a"].double()
    if mut == "lse_transposed":                       # item (bt, h) reads element h BT + bt of the [BT, H] array
        idx = torch.arange(H)[None, :] * BT + torch.arange(BT)[:, None]
        lse_in = lse_in.reshape(-1)[idx]
    if mut == "do_full_stride":                       # item (bt, h) reads row bt N of the [BT, D] array
        rows = torch.arange(BT) * N
        do0 = torch.where((rows < BT)[:, None, None], do0[rows.clamp_max(BT - 1)], torch.full_like(do0, nan))
    delta = r32((do0 * out_in).sum(dim=-1, keepdim=True))
    if mut == "delta_next_head":
        delta = delta.roll(-1, dims=1)
    pb = r32(torch.exp(z - lse_in[..., None]))
    dP = r32(torch.einsum("bhd,bhnd->bhn", do0, v))
    dsb, pbb = r16(pb * (dP - delta)), r16(pb)
    dq = torch.zeros((BT, H, N, 64), dtype=F64)
    dq[:, :, 0] = r32(torch.einsum("bhn,bhnd->bhd", dsb, k)) * 0.125
    dk = r32(dsb[..., None] * q0[:, :, None, :]) * (1.0 if mut == "dk_no_eighth" else 0.125)
    dv = r32(pbb[..., None] * do0[:, :, None, :])
    if mut == "other_dq_untouched":
        dq[:, :, 1:] = nan
    if mut == "keys_past_64_unwritten":               # the write loop's second trip (j = tid >> 3; j < N; j += 64) never runs
        dq[:, :, 64:], dk[:, :, 64:], dv[:, :, 64:] = nan, nan, nan
    got.update(dq=dq.to(BF16), dk=dk.to(BF16), dv=dv.to(BF16))
    return got


# ------------------------------------------------------------------ aim_tattn_fwd_infer ------------------------------------
def tattn_ref64(qkv, B, T, N, H):
    """float64 attention over the frame axis of the bf16 values -> rows [B*T*N, D]"""
    D = H * 64
    x = qkv.double().reshape(B, T, N, 3, H, 64).permute(3, 0, 2, 4, 1, 5)      # [3, B, N, H, T, 64]
    p = ((x[0] @ x[1].transpose(-1, -2)) / 8.0).softmax(-1)
    return (p @ x[2]).permute(0, 3, 1, 2, 4).reshape(B * T * N, D)


def e4m3_code(b):
    """signed position of an e4m3 byte on its grid (+0 and -0 share position 0)"""
    b = b.to(torch.int32)
    mag = b & 0x7F
    return torch.where(b >= 0x80, -mag, mag)


def e4m3_bytes(x):
    """the saturating e4m3 cast of a result (the oracle's q8 of its fp32 value) as bytes"""
    from oracle import vit_clip_oracle as O
    return O.q8(x.float()).to(FP8).view(torch.uint8)


def tattn_infer_emulate(qkv, B, T, N, H):
    """the arithmetic of aim_tattn_fwd_infer's fp8 form in fp32: scores as fp32 sums of exact bf16 products, fp32 softmax
    (expf, one reciprocal), fp32 P.V over T terms, saturating e4m3 cast -> bytes [B*T*N, D]"""
    D = H * 64
    x = qkv.float().reshape(B, T, N, 3, H, 64).permute(3, 0, 2, 4, 1, 5)
    z = (x[0] @ x[1].transpose(-1, -2)) * 0.125
    e = torch.exp(z - z.amax(dim=-1, keepdim=True))
    p = e * (1.0 / e.sum(dim=-1, keepdim=True))
    return e4m3_bytes((p @ x[2]).permute(0, 3, 1, 2, 4).reshape(B * T * N, D))


def infer_pool(case: Case) -> str:
    return f"B{case.B}N{case.N}H{case.H}/{case.family}"


def saturating_qkv(case: Case):
    """every frame's v is +-600 (sign by column): the attention's average is +-600 whatever the weights -> qkv, wanted bytes"""
    D = case.H * 64
    qkv = make_inputs(case)["qkv"].float()
    sign = torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0)
    qkv[:, 2 * D:] = 600.0 * sign
    return qkv.to(BF16), torch.where(sign < 0, 0xFE, 0x7E).to(torch.uint8).expand(case.BT * case.N, D)


# ------------------------------------------------------------------ float64 references and bounds: cls_attn / tattn --------
def small_ref(q, k, v, do, probs_in=None, ep_in=None):
    """attention over a sequence of T <= 32 in fp32 with stored probabilities: items [..., T, 64].
    probs_in / ep_in: the probabilities the backward is given and their error bound (default: fp32 of the float64 ones)."""
    T = q.shape[-2]
    z = q @ k.transpose(-1, -2) / 8.0
    ez = 2 * 64 * U24 * (q.abs() @ k.abs().transpose(-1, -2)) / 8
    p = torch.softmax(z, dim=-1)
    ep = p * (ez + ez.amax(dim=-1, keepdim=True) + (T + 16) * U24)
    O = p @ v
    A = p @ v.abs()
    b_out = U8 * O.abs() + (1 + U8) * (ep @ v.abs() + 2 * T * U24 * A)
    if ep_in is None:
        ep_in = U24 * p
    dP = do @ v.transpose(-1, -2)
    edP = 2 * 64 * U24 * (do.abs() @ v.abs().transpose(-1, -2))
    dot = (p * dP).sum(dim=-1, keepdim=True)
    edot = (ep_in * dP.abs() + p * edP).sum(dim=-1, keepdim=True) + 2 * T * U24 * (p * dP.abs()).sum(dim=-1, keepdim=True)
    dS = p * (dP - dot) / 8
    eDS = (ep_in * (dP - dot).abs() + p * (edP + edot)) / 8 + 4 * U24 * (p * (dP.abs() + dot.abs())) / 8
    acc = 2 * T * U24
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do
    eq = eDS @ k.abs() + acc * (dS.abs() @ k.abs())
    ek = eDS.transpose(-1, -2) @ q.abs() + acc * (dS.abs().transpose(-1, -2) @ q.abs())
    ev = ep_in.transpose(-1, -2) @ do.abs() + acc * (p.transpose(-1, -2) @ do.abs())
    return {"probs": (p, ep), "out": (O, b_out), "dq": (dq, eq), "dk": (dk, ek), "dv": (dv, ev)}


def small_rows(case: Case, inp):
    """the q, k, v, dO of the small kernels' items as [..., T, 64] and the rows of qkv / dO they come from.
    cls: items (B, H) over the class rows; tattn: items (B, N, H) over every token position."""
    B, T, N, H = case.B, case.T, case.N, case.H
    D = H * 64
    x = inp["qkv"].double().reshape(B, T, N, 3, H, 64)
    if case.kind == "cls":
        x = x[:, :, 0]                                                   # [B, T, 3, H, 64]
        q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))     # [B, H, T, 64]
        do = inp["do_small"].double().reshape(B, T, H, 64).permute(0, 2, 1, 3)
    else:
        q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))   # [B, N, H, T, 64]
        do = inp["do"].double().reshape(B, T, N, H, 64).permute(0, 2, 3, 1, 4)
    return q, k, v, do


def small_to_rows(case: Case, t):
    """items [..., T, 64] back to output rows: cls [B T, D]; tattn [B T N, D]"""
    B, T, N, H = case.B, case.T, case.N, case.H
    if case.kind == "cls":
        return t.permute(0, 2, 1, 3).reshape(B * T, H * 64)
    return t.permute(0, 3, 1, 2, 4).reshape(B * T * N, H * 64)


# ------------------------------------------------------------------ the child: one route, every case ------------------------
def _flat(n, dtype, dev):
    """n elements inside a NaN-filled buffer (gemm_cases._padded: spare elements behind, spare rows below)"""
    v, buf = _padded(1, n, dtype, dev)
    return v[0], buf


def _guarded(t, dev):
    """an input tensor copied into the middle of a NaN-filled buffer: a read before its first or past its last element
    poisons the result"""
    n = t.numel()
    if t.dtype == FP8:
        raise TypeError("no fp8 inputs")
    buf = torch.full((n + 512,), float("nan"), dtype=t.dtype, device=dev)
    view = buf[256:256 + n].view(t.shape)
    view.copy_(t)
    return view


class Runner:
    def __init__(self, ops, route, cus, dev):
        self.ops, self.route, self.cus, self.dev = ops, route, cus, dev

    # -- raw launches: every output in a NaN-filled buffer, returns views + buffers
    def fwd(self, qkv, BT, N, H, fp8=False):
        D = H * 64
        lse, lbuf = _flat(BT * H * N, F32, self.dev)
        if fp8:
            o16, obuf = _flat(BT * N * D // 2, BF16, self.dev)          # the fp8 bytes inside a bf16 NaN buffer
            out = o16.view(torch.uint8).view(FP8).view(BT * N, D)
            self.ops.attn_fwd_fp8(qkv, out, BT, N, H, lse=lse)
            return {"out8": out, "lse8": lse.view(BT, H, N)}, {"out8": (obuf, BT * N * D // 2), "lse8": (lbuf, BT * H * N)}
        out, obuf = _flat(BT * N * D, BF16, self.dev)
        out = out.view(BT * N, D)
        self.ops.attn_fwd(qkv, out, lse, BT, N, H)
        return {"out": out, "lse": lse.view(BT, H, N)}, {"out": (obuf, BT * N * D), "lse": (lbuf, BT * H * N)}

    def bwd(self, qkv, out, do, lse, BT, N, H):
        D = H * 64
        dqkv, dbuf = _flat(BT * N * 3 * D, BF16, self.dev)
        dqkv = dqkv.view(BT * N, 3 * D)
        delta, ebuf = _flat(BT * H * N, F32, self.dev)
        self.ops.attn_bwd(qkv, out, do, lse.reshape(-1), delta, dqkv, BT, N, H)
        return {"dqkv": dqkv, "delta": delta}, {"dqkv": (dbuf, BT * N * 3 * D), "delta": (ebuf, BT * H * N)}

    def spatial_all(self, qkv, do, out_a, lse_a, BT, N, H):
        """forward, fp8 forward, backward of form a and of form b -> views, buffers"""
        got, bufs = {}, {}
        g, b = self.fwd(qkv, BT, N, H)
        got.update(g), bufs.update(b)
        g, b = self.fwd(qkv, BT, N, H, fp8=True)
        got.update(g), bufs.update(b)
        for form, o, l in (("a", out_a, lse_a), ("b", got["out"], got["lse"])):
            if o is None:
                continue
            g, b = self.bwd(qkv, o, do, l, BT, N, H)
            got.update({f"{k}@{form}": t for k, t in g.items()}), bufs.update({f"{k}@{form}": t for k, t in b.items()})
        return got, bufs

    def run_spatial(self, case: Case):
        if case.poison:
            return self.run_poison(case)
        dev, BT, N, H = self.dev, case.BT, case.N, case.H
        inp = make_inputs(case)
        q, k, v = split(inp["qkv"], BT, N, H, 3)
        fw = forward_ref(q, k, v)
        o_a, l_a, _, _ = handed_in(fw)
        qkv, do = _guarded(inp["qkv"], dev), _guarded(inp["do"], dev)
        out_a = _guarded(merge(o_a.double()).to(BF16), dev)
        lse_a = _guarded(l_a, dev)
        got, bufs = self.spatial_all(qkv, do, out_a, lse_a, BT, N, H)
        again, _ = self.spatial_all(qkv, do, out_a, lse_a, BT, N, H)
        torch.cuda.synchronize()
        rec = {"plan": list(bwd_plan(N, self.route)), "checks": {}, "pad": {}, "finite": {}, "hash": {}, "repeat": {}}
        for name in got:
            raw = lambda t: t.view(torch.uint8) if t.dtype == FP8 else t.view(_BITS[t.dtype])
            rec["repeat"][name] = bool(torch.equal(raw(got[name]), raw(again[name])))
            rec["pad"][name] = _pad_intact(bufs[name][0], 1, bufs[name][1])
            rec["hash"][name] = _digest(raw(got[name]))
        # the route: the two-kernel form writes delta (finite everywhere), the pipelined form leaves the NaN fill
        for form in "ab":
            d = got[f"delta@{form}"]
            rec[f"delta_written@{form}"] = bool(torch.isfinite(d).all())
            rec[f"delta_untouched@{form}"] = bool(torch.isnan(d).all())
        host = {k_: (t.float() if t.dtype == FP8 else t).cpu() for k_, t in got.items()}
        do64 = split(inp["do"], BT, N, H)
        _, _, eo, el = handed_in(fw)
        bw = {"a": backward_ref(q, k, v, do64, fw, eo, el), "b": backward_ref(q, k, v, do64, fw, fw["out"][1], fw["lse"][1])}
        chk, fin = rec["checks"], rec["finite"]
        chk["out"] = ratio(split(host["out"], BT, N, H), *fw["out"])
        chk["out8"] = ratio(split(host["out8"], BT, N, H), *fw["out8"])
        chk["lse"] = ratio(host["lse"], *fw["lse"])
        chk["lse8"] = ratio(host["lse8"], *fw["lse"])
        for name in ("out", "out8", "lse", "lse8"):
            fin[name] = bool(torch.isfinite(host[name].float()).all())
        for form in "ab":
            d = split(host[f"dqkv@{form}"], BT, N, H, 3)
            for i, name in enumerate(("dq", "dk", "dv")):
                chk[f"{name}@{form}"] = ratio(d[i], *bw[form][name])
            fin[f"dqkv@{form}"] = bool(torch.isfinite(host[f"dqkv@{form}"].float()).all())
        if case.family == "zero_do":                  # dO = 0 for one head: its dq, dk, dv are exactly zero
            h = min(1, H - 1)
            for form in "ab":
                d = split(host[f"dqkv@{form}"], BT, N, H, 3)
                rec[f"zero_head@{form}"] = bool(all((t[:, h] == 0).all() for t in d))
        if case.alone:                                # every frame launched alone gives the bits it has in the whole launch
            same = True
            D = H * 64
            for b in range(BT):
                rows = slice(b * N, (b + 1) * N)
                one, _ = self.spatial_all(qkv[rows], do[rows], out_a[rows], lse_a.view(BT, H, N)[b], 1, N, H)
                torch.cuda.synchronize()
                for name in ("out", "dqkv@a", "dqkv@b"):
                    same &= bool(torch.equal(one[name], got[name][rows]))
                same &= bool(torch.equal(one["out8"].view(torch.uint8), got["out8"][rows].view(torch.uint8)))
                same &= bool(torch.equal(one["lse"][0], got["lse"][b]))
            rec["alone_identical"] = same
        return rec

    def run_poison(self, case: Case):
        """frames 0 and 2 and every odd head of frame 1 hold NaN in qkv, dO, out and lse: the even heads of frame 1 must be
        finite and the bits of the same data launched as BT = 1 with clean neighbours"""
        dev, N, H = self.dev, case.N, case.H
        D = H * 64
        inp = make_inputs(Case(case.name, "spatial", 1, N, H, "unit", case.seed))
        q, k, v = split(inp["qkv"], 1, N, H, 3)
        fw = forward_ref(q, k, v)
        o_a, l_a, _, _ = handed_in(fw)
        clean = {"qkv": inp["qkv"], "do": inp["do"], "out": merge(o_a.double()).to(BF16), "lse": l_a.reshape(H, N)}
        odd = torch.arange(H) % 2 == 1
        big = {}
        for name, t in clean.items():
            if name == "lse":
                mid = t.clone()
                mid[odd] = float("nan")
                big[name] = torch.stack([torch.full_like(t, float("nan")), mid, torch.full_like(t, float("nan"))])
            else:
                mid = t.clone().reshape(N, -1, H, 64)
                mid[:, :, odd] = float("nan")
                mid = mid.reshape(t.shape)
                big[name] = torch.cat([torch.full_like(t, float("nan")), mid, torch.full_like(t, float("nan"))])
        c = {n_: _guarded(t, dev) for n_, t in clean.items()}
        p = {n_: _guarded(t, dev) for n_, t in big.items()}
        one, _ = self.spatial_all(c["qkv"], c["do"], c["out"], c["lse"], 1, N, H)
        # form b of the poisoned launch: the forward's own out / lse are NaN where the inputs are, by construction
        got, bufs = self.spatial_all(p["qkv"], p["do"], p["out"], p["lse"], 3, N, H)
        torch.cuda.synchronize()
        rec = {"plan": list(bwd_plan(N, self.route)), "checks": {}, "pad": {}, "finite": {}, "hash": {}, "repeat": {}}
        even = (~odd).to(dev)
        rows = slice(N, 2 * N)
        same, finite = True, True
        for name in ("out", "out8", "dqkv@a", "dqkv@b"):
            f = lambda t: (t.view(torch.uint8) if t.dtype == FP8 else t.view(torch.int16)).reshape(N, -1, H, 64)[:, :, even]
            a, b = f(got[name][rows]), f(one[name])
            same &= bool(torch.equal(a, b))
            finite &= bool(torch.isfinite(got[name][rows].float().reshape(N, -1, H, 64)[:, :, even]).all())
        for name in ("lse", "lse8"):
            same &= bool(torch.equal(got[name][1][even], one[name][0][even]))
            finite &= bool(torch.isfinite(got[name][1][even]).all())
        rec["independent"] = same
        rec["finite"]["clean_heads"] = finite
        for name in got:
            rec["pad"][name] = _pad_intact(bufs[name][0], 1, bufs[name][1])
        return rec

    def run_small(self, case: Case):
        dev, ops = self.dev, self.ops
        B, T, N, H, BT = case.B, case.T, case.N, case.H, case.BT
        D = H * 64
        inp = make_inputs(case)
        g = torch.Generator().manual_seed(case.seed + 1)
        inp["do_small"] = torch.randn((BT, D), generator=g).to(BF16)
        base = torch.randn((BT * N, 3 * D), generator=g).to(BF16)                # cls non-compact accumulates into this
        q, k, v, do = small_rows(case, inp)
        ref = small_ref(q, k, v, do)
        qkv = _guarded(inp["qkv"], dev)
        cls = case.kind == "cls"
        nprob = B * H if cls else B * N * H
        rows_out = BT if cls else BT * N
        dout = _guarded(inp["do_small"] if cls else inp["do"], dev)
        probs_a = _guarded(ref["probs"][0].to(F32).reshape(-1), dev)

        def run():
            got, bufs = {}, {}

            def new(name, n, dtype, shape):
                vw, buf = _flat(n, dtype, dev)
                got[name], bufs[name] = vw.view(shape), (buf, n)
                return got[name]

            out = new("out", rows_out * D, BF16, (rows_out, D))
            probs = new("probs", nprob * T * T, F32, (nprob * T * T,))
            (ops.cls_attn_fwd if cls else ops.tattn_fwd)(qkv, out, probs, B, T, N, H)
            for form, pr in (("a", probs_a), ("b", probs)):
                if cls:
                    comp = new(f"dcompact@{form}", BT * 3 * D, BF16, (BT, 3 * D))
                    ops.cls_attn_bwd(qkv, pr, dout, comp, B, T, N, H, compact=True)
                    full = new(f"dfull@{form}", BT * N * 3 * D, BF16, (BT * N, 3 * D))
                    full.copy_(base)
                    ops.cls_attn_bwd(qkv, pr, dout, full, B, T, N, H, compact=False)
                else:
                    dq = new(f"dqkv@{form}", BT * N * 3 * D, BF16, (BT * N, 3 * D))
                    ops.tattn_bwd(qkv, pr, dout, dq, B, T, N, H)
            return got, bufs

        got, bufs = run()
        again, _ = run()
        torch.cuda.synchronize()
        rec = {"checks": {}, "pad": {}, "finite": {}, "hash": {}, "repeat": {}}
        for name in got:
            rec["repeat"][name] = bool(torch.equal(got[name].view(_BITS[got[name].dtype]), again[name].view(_BITS[got[name].dtype])))
            rec["pad"][name] = _pad_intact(bufs[name][0], 1, bufs[name][1])
            rec["hash"][name] = _digest(got[name])
            rec["finite"][name] = bool(torch.isfinite(got[name].float()).all())
        host = {k_: t.cpu() for k_, t in got.items()}
        chk = rec["checks"]
        chk["out"] = ratio(host["out"], small_to_rows(case, ref["out"][0]), small_to_rows(case, ref["out"][1]))
        pshape = ref["probs"][0].shape
        chk["probs"] = ratio(host["probs"].reshape(pshape), *ref["probs"])
        ref_b = small_ref(q, k, v, do, ep_in=ref["probs"][1])
        for form, r in (("a", ref), ("b", ref_b)):
            d = torch.cat([small_to_rows(case, r[n_][0]) for n_ in ("dq", "dk", "dv")], dim=1)
            e = torch.cat([small_to_rows(case, r[n_][1]) for n_ in ("dq", "dk", "dv")], dim=1)
            if cls:
                chk[f"dcompact@{form}"] = ratio(host[f"dcompact@{form}"], d, U8 * d.abs() + (1 + U8) * e)
                full = host[f"dfull@{form}"].reshape(BT, N, 3 * D)
                want = base.double().reshape(BT, N, 3 * D)[:, 0] + d
                chk[f"dfull@{form}"] = ratio(full[:, 0], want, (U8 + 2 * U24) * want.abs() + (1 + U8) * e)
                # only the class rows change: every other row keeps its bits
                rec[f"other_rows_kept@{form}"] = bool(torch.equal(full[:, 1:].view(torch.int16),
                                                                  base.reshape(BT, N, 3 * D)[:, 1:].view(torch.int16)))
            else:
                chk[f"dqkv@{form}"] = ratio(host[f"dqkv@{form}"], d, U8 * d.abs() + (1 + U8) * e)
        return rec

    def clsq_all(self, qkv, do_cls, out_a, lse_a, BT, N, H):
        """class-query forward, backward of form a (rounded float64 out / lse handed in) and of form b (the forward's own),
        every output in a NaN-filled buffer -> views, buffers"""
        D, dev, ops = H * 64, self.dev, self.ops
        got, bufs = {}, {}

        def new(name, n, dtype, shape):
            vw, buf = _flat(n, dtype, dev)
            got[name], bufs[name] = vw.view(shape), (buf, n)
            return got[name]

        out = new("out", BT * D, BF16, (BT, D))
        lse = new("lse", BT * H, F32, (BT, H))
        ops.attn_fwd_cls(qkv, out, lse, BT, N, H)
        for form, o, l in (("a", out_a, lse_a), ("b", out, lse)):
            dqkv = new(f"dqkv@{form}", BT * N * 3 * D, BF16, (BT * N, 3 * D))
            ops.attn_bwd_cls(qkv, o, do_cls, l, dqkv, BT, N, H)
        return got, bufs

    def run_clsq(self, case: Case):
        dev, BT, N, H = self.dev, case.BT, case.N, case.H
        D = H * 64
        inp = clsq_inputs(case)
        exp = clsq_expected(case, inp)
        qkv, do_cls = _guarded(inp["qkv"], dev), _guarded(inp["do_cls"], dev)
        out_a, lse_a = _guarded(exp["_out_a"], dev), _guarded(exp["_lse_a"], dev)
        got, bufs = self.clsq_all(qkv, do_cls, out_a, lse_a, BT, N, H)
        again, _ = self.clsq_all(qkv, do_cls, out_a, lse_a, BT, N, H)
        # row 0 of the full forward kernel on the same input
        full_out = torch.empty((BT * N, D), dtype=BF16, device=dev)
        full_lse = torch.empty((BT, H, N), dtype=F32, device=dev)
        self.ops.attn_fwd(qkv, full_out, full_lse.view(-1), BT, N, H)
        # NaN in the q part of every non-class row: nothing the class query's result depends on
        poisoned = inp["qkv"].clone()
        poisoned.view(BT, N, 3 * D)[:, 1:, :D] = float("nan")
        pois, _ = self.clsq_all(_guarded(poisoned, dev), do_cls, out_a, lse_a, BT, N, H)
        torch.cuda.synchronize()
        rec = {"checks": {}, "pad": {}, "finite": {}, "hash": {}, "repeat": {}, "poison": {}}
        bits = lambda t: t.view(_BITS[t.dtype])
        for name in got:
            rec["repeat"][name] = bool(torch.equal(bits(got[name]), bits(again[name])))
            rec["poison"][name] = bool(torch.equal(bits(got[name]), bits(pois[name])))
            rec["pad"][name] = _pad_intact(bufs[name][0], 1, bufs[name][1])
            rec["finite"][name] = bool(torch.isfinite(got[name].float()).all())
            rec["hash"][name] = _digest(bits(got[name]))
        rec["row0_of_attn_fwd"] = bool(torch.equal(bits(got["out"]), bits(full_out.view(BT, N, D)[:, 0].contiguous()))
                                       and torch.equal(bits(got["lse"]), bits(full_lse[:, :, 0].contiguous())))
        host = {k_: t.cpu() for k_, t in got.items()}
        fwd = {"out": host["out"].view(BT, H, 64), "lse": host["lse"]}
        rec["checks"].update(compare_clsq(case, exp, fwd, "a"))
        for form in "ab":
            dq, dk, dv = split(host[f"dqkv@{form}"], BT, N, H, 3)
            bwd = {"dq": dq, "dk": dk, "dv": dv}
            rec["checks"].update({f"{k_}@{form}": r for k_, r in compare_clsq(case, exp, bwd, form).items()})
            for k_, ok in clsq_exact(case, bwd).items():
                rec[f"{k_}@{form}"] = ok
        return rec

    def run_infer(self, case: Case):
        """aim_tattn_fwd_infer on a tattn sweep case under this process's LDS staging: the bf16 form against aim_tattn_fwd's
        bits, the fp8 form byte by byte against the e4m3 cast of the float64 result"""
        dev, ops = self.dev, self.ops
        B, T, N, H, M = case.B, case.T, case.N, case.H, case.BT * case.N
        D = H * 64
        qkv_h = make_inputs(case)["qkv"]
        qkv = _guarded(qkv_h, dev)
        want16 = torch.empty((M, D), dtype=BF16, device=dev)
        probs = torch.empty((B * N * H * T * T,), dtype=F32, device=dev)
        ops.tattn_fwd(qkv, want16, probs, B, T, N, H)
        rec = {"pad": {}, "repeat": {}}

        def infer(src, fp8):
            o16, buf = _flat(M * D // 2 if fp8 else M * D, BF16, dev)          # (the fp8 bytes inside a bf16 NaN buffer)
            out = o16.view(torch.uint8).view(M, D) if fp8 else o16.view(M, D)
            ops.tattn_fwd_infer(src, out, B, T, N, H)
            return out, buf, o16.numel()

        o16, b16, n16 = infer(qkv, False)
        o8, b8, n8 = infer(qkv, True)
        o16_2, _, _ = infer(qkv, False)
        o8_2, _, _ = infer(qkv, True)
        torch.cuda.synchronize()
        rec["bf16_is_tattn_fwd"] = bool(torch.equal(o16.view(torch.int16), want16.view(torch.int16)))
        rec["repeat"] = {"out": bool(torch.equal(o16.view(torch.int16), o16_2.view(torch.int16))), "out8": bool(torch.equal(o8, o8_2))}
        rec["pad"] = {"out": _pad_intact(b16, 1, n16), "out8": _pad_intact(b8, 1, n8)}
        got = o8.cpu()
        step = (e4m3_code(got) - e4m3_code(e4m3_bytes(tattn_ref64(qkv_h, B, T, N, H)))).abs()
        rec.update(bytes=got.numel(), neighbours=int((step == 1).sum()), farther=int((step > 1).sum()), hash8=_digest(got),
                   pool=infer_pool(case))
        if T in SAT_T and case.family == "unit":
            sat, want = saturating_qkv(case)
            s8, sb, sn = infer(_guarded(sat, dev), True)
            torch.cuda.synchronize()
            rec["saturates"] = bool(torch.equal(s8.cpu(), want)) and _pad_intact(sb, 1, sn)
        return rec

    def run_large(self, BT, tag):
        """BT x 197 x 12 with the qkv buffer above 2^31 (2^32) bytes: float64 on the first two and last two frames, the bits of
        those frames against a four-frame launch, finiteness everywhere"""
        dev, N, H = self.dev, 197, 12
        D = H * 64
        need = BT * N * D * 2 * (3 + 3 + 1 + 1 + 1 + 1) * 1.15
        free = torch.cuda.mem_get_info()[0]
        if free < need + (4 << 30):
            return {"ran": False, "free": free, "need": need}
        g = torch.Generator(device=dev).manual_seed(77)
        qkv = torch.empty((BT * N, 3 * D), dtype=BF16, device=dev)
        do = torch.empty((BT * N, D), dtype=BF16, device=dev)
        step = 200 * N
        for r in range(0, BT * N, step):
            n = min(step, BT * N - r)
            qkv[r:r + n] = torch.randn((n, 3 * D), generator=g, device=dev).to(BF16)
            do[r:r + n] = torch.randn((n, D), generator=g, device=dev).to(BF16)
        rec = {"ran": True, "bytes": qkv.numel() * 2, "checks": {}, "finite": {}}
        out = torch.full((BT * N, D), float("nan"), dtype=BF16, device=dev)
        out8 = torch.zeros((BT * N, D), dtype=torch.uint8, device=dev).view(FP8)
        lse = torch.full((BT * H * N,), float("nan"), dtype=F32, device=dev)
        dqkv = torch.full((BT * N, 3 * D), float("nan"), dtype=BF16, device=dev)
        delta = torch.empty((BT * H * N,), dtype=F32, device=dev)
        self.ops.attn_fwd(qkv, out, lse, BT, N, H)
        self.ops.attn_fwd_fp8(qkv, out8, BT, N, H)
        self.ops.attn_bwd(qkv, out, do, lse, delta, dqkv, BT, N, H)
        torch.cuda.synchronize()
        for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv)):
            rec["finite"][name] = bool(torch.isfinite(t).all())
        rec["finite"]["out8"] = bool(torch.isfinite(out8[:2 * N].float()).all() and torch.isfinite(out8[-2 * N:].float()).all())
        fr = torch.cat([torch.arange(0, 2 * N), torch.arange((BT - 2) * N, BT * N)]).to(dev)
        q4, d4 = qkv[fr].contiguous(), do[fr].contiguous()
        lfr = torch.cat([torch.arange(0, 2 * H * N), torch.arange((BT - 2) * H * N, BT * H * N)]).to(dev)
        big = {"out": out[fr].clone(), "out8": out8.view(torch.uint8)[fr].clone(), "lse": lse[lfr].clone(), "dqkv": dqkv[fr].clone()}
        del out, out8, lse, dqkv, delta, qkv, do
        torch.cuda.empty_cache()
        c4 = Case(f"attn/large/{tag}", "spatial", 4, N, H, "unit")
        one, _ = self.spatial_all(q4, d4, None, None, 4, N, H)
        torch.cuda.synchronize()
        rec["identical"] = bool(torch.equal(one["out"], big["out"]) and torch.equal(one["out8"].view(torch.uint8), big["out8"])
                                and torch.equal(one["lse"].reshape(-1), big["lse"]) and torch.equal(one["dqkv@b"], big["dqkv"]))
        inp = {"qkv": q4.cpu(), "do": d4.cpu()}
        fw, _, bw_b = spatial_expected(c4, inp)
        rec["checks"]["out"] = ratio(split(big["out"].cpu(), 4, N, H), *fw["out"])
        rec["checks"]["out8"] = ratio(split(big["out8"].view(FP8).float().cpu(), 4, N, H), *fw["out8"])
        rec["checks"]["lse"] = ratio(big["lse"].cpu().reshape(4, H, N), *fw["lse"])
        d = split(big["dqkv"].cpu(), 4, N, H, 3)
        for i, name in enumerate(("dq", "dk", "dv")):
            rec["checks"][f"{name}@b"] = ratio(d[i], *bw_b[name])
        return rec

    def refusals(self):
        """unsupported shapes are refused with a message through aim_last_error (ops.check raises it)"""
        dev, ops, out = self.dev, self.ops, {}
        t16 = torch.zeros(64, dtype=BF16, device=dev)
        t32 = torch.zeros(64, dtype=F32, device=dev)
        t8 = torch.zeros(64, dtype=torch.uint8, device=dev).view(FP8)
        calls = {"attn_fwd N=289": lambda: ops.attn_fwd(t16, t16, t32, 1, NMAX + 1, 1),
                 "attn_fwd_fp8 N=289": lambda: ops.attn_fwd_fp8(t16, t8, 1, NMAX + 1, 1),
                 "attn_bwd N=289": lambda: ops.attn_bwd(t16, t16, t16, t32, t32, t16, 1, NMAX + 1, 1),
                 "cls_attn_fwd T=33": lambda: ops.cls_attn_fwd(t16, t16, t32, 1, 33, 1, 1),
                 "cls_attn_bwd T=33": lambda: ops.cls_attn_bwd(t16, t32, t16, t16, 1, 33, 1, 1),
                 "tattn_fwd T=33": lambda: ops.tattn_fwd(t16, t16, t32, 1, 33, 1, 1),
                 "tattn_bwd T=33": lambda: ops.tattn_bwd(t16, t32, t16, t16, 1, 33, 1, 1)}
        for name, f in calls.items():
            try:
                f()
                out[name] = None
            except RuntimeError as e:
                out[name] = str(e)
        # the class-query kernels, through the library itself (a null pointer cannot pass ops): buffers large enough for the
        # largest refused shape, outputs filled with NaN that must survive
        import aim_amd
        lib, st, n = aim_amd.load_library(), ops._stream(), NMAX + 1
        qkv = torch.zeros((n, 192), dtype=BF16, device=dev)
        o16, d16 = torch.zeros(64, dtype=BF16, device=dev), torch.zeros(64, dtype=BF16, device=dev)
        l32 = torch.zeros(1, dtype=F32, device=dev)
        outs = {"out_cls": torch.full((64,), float("nan"), dtype=BF16, device=dev),
                "lse_cls": torch.full((1,), float("nan"), dtype=F32, device=dev),
                "dqkv": torch.full((n, 192), float("nan"), dtype=BF16, device=dev)}
        p = lambda t: t.data_ptr()
        fwd = lambda BT, N, lse: lib.aim_attn_fwd_cls(p(qkv), p(outs["out_cls"]), lse, BT, N, 1, st)
        bwd = lambda BT, N, lse: lib.aim_attn_bwd_cls(p(qkv), p(o16), p(d16), lse, p(outs["dqkv"]), BT, N, 1, st)
        for kernel, f, lse in (("attn_fwd_cls", fwd, p(outs["lse_cls"])), ("attn_bwd_cls", bwd, p(l32))):
            for tag, args in (("N=289", (1, n, lse)), ("N=0", (1, 0, lse)), ("BT=0", (0, 1, lse)), ("null lse_cls", (1, 1, None))):
                rc = f(*args)
                msg = lib.aim_last_error()
                out[f"{kernel} {tag}"] = (msg.decode() if msg else "") if rc != 0 else None
        torch.cuda.synchronize()
        self.refusals_untouched = {k: bool(torch.isnan(t).all()) for k, t in outs.items()}
        return out


def main(argv):
    route, path = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    dev = torch.device("cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"route": route, "cus": cus, "cases": {}, "large": {}}
    run = Runner(ops, route, cus, dev)
    if route in LENGTH_MODES:          # lengths: every length case, then the inference forms; lds32: the inference forms alone
        assert (os.environ.get("AIM_TATTN_LDS16") == "0") == (route == "lds32"), "the staging switch does not match the mode"
        res["infer"] = {}
        with torch.no_grad():
            res["refusals"] = run.refusals()
            res["refusals_untouched"] = run.refusals_untouched
            for case in length_cases():
                if route == "lengths":
                    res["cases"][case.name] = run.run_clsq(case) if case.kind == "clsq" else run.run_small(case)
                if case.kind == "tattn":
                    res["infer"][case.name] = run.run_infer(case)
        with open(path, "w") as f:
            json.dump(res, f)
        return
    with torch.no_grad():
        res["refusals"] = run.refusals()
        res["refusals_untouched"] = run.refusals_untouched
        for case in route_cases():
            res["cases"][case.name] = run.run_spatial(case) if case.kind == "spatial" else run.run_small(case)
        torch.cuda.empty_cache()
        res["large"]["2^31"] = run.run_large(2400, "2^31")
        torch.cuda.empty_cache()
        res["large"]["2^32"] = run.run_large(4800, "2^32")
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
