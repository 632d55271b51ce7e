"""The product's fp8 GEMM call forms (`ops.gemm_fp8`: the 256 x 256 block-scaled-MFMA kernel and the fp8 form of the
64 x 64 kernel that takes its peeled tail), rebuilt with their exact options, the edges of the entry point, and a float64
restatement of the four epilogues BF16, F32, ACT8 and RES16.

A plain module (no fixtures): `test_fp8_gemm_routes_gpu.py` runs every case on both routes, one child process per route
(`python fp8_gemm_cases.py ROUTE OUT.json`), and `test_fp8_gemm_cases_cpu.py` proves on the CPU that the comparison rejects
the bugs it is meant to catch.

Two input families.

`exact` removes the accumulation error instead of bounding it.  A holds integers in [-4, 4] and W8 integers in [-8, 8]
(exact in e4m3), so every product and every partial sum of any subset is an integer below 2^24: the fp32 accumulation is
exact in any order, inside or outside the MFMA.  wscale[n] is 2^-8 {1/2, 1, 2}, bias and vec are k / 256, af / at / bt come
from {0, 1/4, 1/2, 1, 2}, resid is k / 256 (F32, |resid| <= 4) or k / 16 (RES16, |k| <= 128: exact in bf16).  Every term of
the epilogue's sum is a multiple of 2^-11 and the sum of absolute terms stays far below 2^13, so any association (and any
fma contraction) of it is exact in fp32.  Hence
  * F32 is `ref.float()` and BF16 / RES16 are one round-to-nearest-even of an exactly representable value,
    `ref.float().to(bfloat16)`: the bound is 0 and the check counts unequal elements (compared as numbers, so that a zero
    of either sign equals a zero);
  * ACT8's pre-activation `acc * wscale + bias` is exact and the only error is the activation in fp32 and one product
    with the row factor: e = |rs| EPS_ACT (1 + |pre|) + 2 u |y|.  The byte must lie between the e4m3 roundings of y - e
    and y + e on the signed code grid (`code`: +0 and -0 share position 0) and is never a NaN code (0x7F, 0xFF).  No
    exclusions, no cap on mismatches: where the two ends agree, the byte is determined.  The share of outputs whose ends
    differ (`ambiguous`, from the reference alone) is held below AMBIGUOUS_MAX by the CPU test, so the check cannot
    become vacuous.

`random` is `gemm_cases.make_inputs`' fp8 recipe (normal activations, weights quantised per output row).  BF16, F32 and
RES16 are held to the bound `gemm_cases.expected` derives (error / bound <= 1).  ACT8 is held to the same byte interval
with e enlarged by 1.13 |rs| e_pre (1.13 bounds |GELU'|, whose maximum is about 1.129, and |QuickGELU'|; e_pre is the
accumulation bound): for ACT8 this family checks realistic magnitudes and saturation only -- under the worst-case
accumulation bound about half of all e4m3 roundings are undecided -- and the exact family carries the discriminating power.

Every output is a view into a wider buffer (ldo > N, spare rows) filled with NaN (bf16 / fp32) or the byte 0xA5 (fp8: NaN
bytes there would look like a kernel fault); the residual is such a view too (ldr > N), and the edge forms read A and W
out of buffers with lda, ldw > K whose spare bytes are the e4m3 NaN 0x7F.
"""
import json
import os
import sys
import time
from dataclasses import dataclass
from typing import Dict, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import (EPS_ACT, U8, U24, _digest, _pad_intact, _padded, gelu, peel_frames, peel_rows, qgelu,  # noqa: E402
                        ratio)

QGELU, GELU = 0, 1
BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
OUT_DTYPE = {"bf16": BF16, "f32": F32, "res16": BF16, "act8": torch.uint8}
GEOMS = {"b16": (768, 192, 197, 6), "l14": (1024, 256, 257, 4)}        # D, adapter width r, tokens per frame, frames
ROUTES = ("whole", "peel")
ROUTE_ENV = {"whole": {"AIM_GEMM_PEEL": "0"}, "peel": {}}
ROUTE_VARS = ("AIM_GEMM_PEEL",)
FAMILIES = ("exact", "random")
FACTORS = (0.0, 0.25, 0.5, 1.0, 2.0)          # af / at / bt of the exact family
AMBIGUOUS_MAX = 2e-3
CANARY = 0xA5


@dataclass(frozen=True)
class Spec:
    epi: str                  # bf16 | f32 | res16 | act8
    M: int
    N: int
    K: int
    ntok: int = 0
    bias: bool = False
    resid: bool = False
    af: bool = False
    at: bool = False
    vec: str = ""             # "frame": one row per frame (ldv = N); "row0": ldv = 0, rows >= 1 are decoys
    bt: bool = False
    act: int = QGELU
    act2: int = QGELU
    n_split: int = 0
    ldo_pad: int = 8          # ldo = N + ldo_pad (ACT8: 16 keeps the sixteen-byte stores, 8 selects the eight-byte ones)
    ld_pad: int = 0           # lda = ldw = K + ld_pad
    sat: bool = False         # ACT8: a few columns with bias +-1024, one token with row factor -1, one with 1/4
    w_scale: float = 1.0      # random family
    bias_scale: float = 1.0


@dataclass(frozen=True)
class Case:
    name: str
    form: str
    site: str                 # the call site (product forms) or the edge the case is for
    spec: Spec
    family: str = "exact"
    seed: int = 0
    reserve: bool = False     # also reserve_cus = 16 and 64: must give the same bits


# ------------------------------------------------------------------ the case table ----------------------------------------
def forms(geom: str, M: int) -> Dict[str, tuple]:
    """form -> (Spec, call site, Case options) at M rows of geometry `geom`."""
    D, r, ntok, _ = GEOMS[geom]
    H4, C = 4 * D, 4 * D + r
    res = dict(bias=True, resid=True, bt=True)
    return {
        "qkv": (Spec("bf16", M, 3 * D, D, bias=True), "backbone.py:486, aim_variant.py:150,163", dict(reserve=True)),
        "o_aim": (Spec("bf16", M, D, D, bias=True), "aim_variant.py:154,167", {}),
        "x1_f32": (Spec("f32", M, D, D, ntok, af=True, vec="frame", **res), "backbone.py:557", {}),
        "x1_res16": (Spec("res16", M, D, D, ntok, af=True, vec="frame", **res), "backbone.py:557", {}),
        "cat1": (Spec("act8", M, C, D, ntok, bias=True, at=True, act=QGELU, act2=GELU, n_split=H4, ldo_pad=16, w_scale=1.5,
                      bias_scale=0.3), "backbone.py:633", {}),
        "x2_f32": (Spec("f32", M, D, C, ntok, vec="row0", **res), "backbone.py:636", {}),
        "x2_res16": (Spec("res16", M, D, C, ntok, vec="row0", **res), "backbone.py:636", {}),
    }


PRODUCT_FORMS = ("qkv", "o_aim", "x1_f32", "x1_res16", "cat1", "x2_f32", "x2_res16")
# forms that also run at a row count whose last tile round the library peels (exact family, ViT-L/14)
PEEL_FORMS = ("qkv", "o_aim", "x1_res16")
EPIS = ("bf16", "f32", "res16", "act8")


def edge_spec(epi: str, M: int, N: int, K: int, ntok: int = 129, **kw) -> Spec:
    """the richest call of epilogue `epi` at an edge shape: every optional input the epilogue reads"""
    if epi == "bf16":
        base = dict(bias=True, af=True)
    elif epi == "act8":
        base = dict(bias=True, at=True, act=QGELU, act2=GELU, n_split=(N // 16) * 8)
    else:
        base = dict(bias=True, resid=True, af=True, vec="frame", bt=True)
    base.update(ld_pad=16)
    base.update(kw)
    return Spec(epi, M, N, K, ntok, **base)


def edge_cases():
    """[(name, the edge it is for, Spec)], exact family only: the smallest shapes the entry point accepts (M >= 1024,
    N >= 64, N % 8 == 0)."""
    out = []
    for epi in EPIS:
        out.append((f"edge_M/{epi}/M1024", "M: whole row tiles", edge_spec(epi, 1024, 264, 256)))
        out.append((f"edge_M/{epi}/M1031", "M: 7 rows in the last row tile, no multiple of the 8- / 16-row store groups",
                    edge_spec(epi, 1031, 264, 256)))
        for N, why in ((64, "one 64-column wave tile"), (72, "N % 16 == 8: ACT8's eight-byte store path"),
                       (264, "one full column tile plus 8 columns")):
            for pad in (16, 8):
                out.append((f"edge_N/{epi}/N{N}+{pad}", f"N = {N} ({why}), ldo = N + {pad}",
                            edge_spec(epi, 1031, N, 256, ldo_pad=pad)))
        for K, why in ((144, "two K-steps, the second 16 bytes long"), (256, "two whole K-steps"),
                       (400, "four K-steps, the last 16 bytes long")):
            out.append((f"edge_K/{epi}/K{K}", f"K = {K}: {why}", edge_spec(epi, 1031, 72, K)))
    for at in (False, True):
        for ns, why in ((0, "n_split = 0: `act` and the row factor on every column"),
                        (264, "n_split = N: `act` on every column, no row factor"),
                        (200, "n_split % 16 == 8 inside the wave tile of columns 192..255: that wave takes the "
                              "mixed-activation branch, columns 0..191 the all-QuickGELU one")):
            out.append((f"edge_split/act8/ns{ns}/{'at' if at else 'noat'}", why,
                        edge_spec("act8", 1031, 264, 256, ntok=129 if at else 0, at=at, n_split=ns)))
    out.append(("edge_sat/act8", "saturation: bias +-1024, row factors -1 and 1/4",
                edge_spec("act8", 1031, 72, 256, n_split=0, act=GELU, sat=True)))
    for epi in ("f32", "res16"):
        for ntok, why in ((128, "a 128-row wave tile meets exactly one frame"), (129, "a wave tile meets two frames"),
                          (1000, "a partial last frame: af and vec have ceil(M / ntok) rows")):
            out.append((f"edge_vec/{epi}/ntok{ntok}", f"ntok = {ntok}: {why}", edge_spec(epi, 1031, 72, 256, ntok=ntok)))
    return out


def cases(cus: int = 256):
    out = []
    seed = 500
    for geom in GEOMS:
        ntok, frames = GEOMS[geom][2:]
        for name in PRODUCT_FORMS:
            for fam in FAMILIES:
                spec, site, opt = forms(geom, frames * ntok)[name]
                out.append(Case(f"{name}/{geom}/M{spec.M}/{fam}", name, site, spec, fam, seed, **opt))
                seed += 1
    for name, why, spec in edge_cases():
        out.append(Case(name, name.split("/")[0], why, spec, "exact", seed))
        seed += 1
    # the peel route: row counts whose thin last tile round goes to the 64 x 64 kernel on a device of `cus` CUs
    ntok = GEOMS["l14"][2]
    for name in PEEL_FORMS:
        M = peel_frames(forms("l14", ntok)[name][0].N, ntok, cus) * ntok
        spec, site, _ = forms("l14", M)[name]
        out.append(Case(f"{name}/l14/M{M}/peel", name, site, spec, "exact", seed))
        seed += 1
    M = peel_frames(64, 197, cus) * 197
    out.append(Case(f"peel_smallN/M{M}/peel", "peel_smallN", "the peeled tail is a single column of 64 x 64 tiles",
                    Spec("bf16", M, 64, 256, bias=True), "exact", seed))
    return out


def route_plan(case: Case, route: str, cus: int):
    """(kernel, tiles the persistent 256 x 256 kernel processes) for `case` under `route`'s environment: a mirror of
    capi.hip::aim_gemm_fp8 -- only BF16 and RES16 peel, with K % 128 == 0 and aim_gemm_peel_rows > 0; F32 and ACT8 never
    do.  None: the case does not run there (route `peel` runs only what it peels)."""
    s = case.spec
    tn = (s.N + 255) // 256
    m0 = peel_rows(s.M, s.N, cus) if s.epi in ("bf16", "res16") and s.K % 128 == 0 else 0
    if route == "peel":
        return ("peel", (m0 // 256) * tn) if m0 else None
    return ("256", ((s.M + 255) // 256) * tn)


# ------------------------------------------------------------------ inputs (CPU, fixed seeds) ------------------------------
def _frames(s: Spec) -> int:
    return (s.M + s.ntok - 1) // s.ntok if s.ntok else 1


def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    s = case.spec
    g = torch.Generator().manual_seed(case.seed)
    frames = _frames(s)
    inp = {}

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def rn(*shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale

    if case.family == "exact":
        fac = torch.tensor(FACTORS)
        inp["A"] = ri(-4, 4, s.M, s.K).to(FP8)
        inp["W"] = ri(-8, 8, s.N, s.K).to(FP8)
        inp["wscale"] = 2.0 ** (-8 + ri(-1, 1, s.N))
        if s.bias:
            inp["bias"] = ri(-256, 256, s.N) / 256
        if s.resid:
            inp["resid"] = (ri(-128, 128, s.M, s.N) / 16).to(BF16) if s.epi == "res16" else ri(-1024, 1024, s.M, s.N) / 256
        if s.af:
            # (consecutive frames never share a factor: the next frame's is always a different number)
            inp["af"] = fac[(torch.randint(0, 5, (1,), generator=g) + 2 * torch.arange(frames)) % 5]
        if s.at:
            inp["at"] = fac[torch.randint(0, 5, (s.ntok,), generator=g)]
        if s.bt:
            inp["bt"] = fac[torch.randint(0, 5, (s.ntok,), generator=g)]
        if s.vec:
            inp["vec"] = ri(-256, 256, max(frames, 2), s.N) / 256
        if s.sat:
            # (the other tokens' factors stay <= 1/2: at -1024 the interval's half width |rs| EPS_ACT 1025 then stays below
            # the first tie 2^-10 of the e4m3 grid, and the zeros there are determined)
            inp["at"] = inp["at"].clamp(max=0.5)
            inp["bias"][[3, 10, 40]] = 1024.0
            inp["bias"][[5, 41]] = -1024.0
            inp["at"][0], inp["at"][1], inp["at"][2] = -1.0, 0.25, 1.0
        return inp
    # random: gemm_cases.make_inputs' fp8 branch (ops.quantize_fp8_rows on the weight)
    inp["A"] = rn(s.M, s.K).clamp(-448, 448).to(FP8)
    w = rn(s.N, s.K, scale=s.w_scale * s.K ** -0.5)
    sc = w.abs().amax(dim=1).clamp_min(1e-12) / 448.0
    inp["W"] = (w / sc[:, None]).clamp(-448.0, 448.0).to(FP8)
    inp["wscale"] = sc.float()
    if s.bias:
        inp["bias"] = rn(s.N, scale=s.bias_scale)
    if s.resid:
        inp["resid"] = rn(s.M, s.N).to(BF16 if s.epi == "res16" else F32)
    if s.af:                                         # 1 - lamda: differs per frame
        inp["af"] = torch.rand(frames, generator=g) * 0.7 + 0.3
    if s.at:                                         # DropPath mask * adapter scale / keep: dropped tokens are 0
        keep = torch.rand(s.ntok, generator=g) < 0.7
        keep[0], keep[-1] = True, False
        inp["at"] = keep.float() * (0.5 / 0.7)
    if s.bt:
        bt = torch.rand(s.ntok, generator=g) + 0.25
        bt[1::7] = 0.0
        inp["bt"] = bt
    if s.vec:
        inp["vec"] = rn(max(frames, 2), s.N)
    return inp


# ------------------------------------------------------------------ e4m3 on the signed code grid --------------------------
def _code(b):
    """signed position of an e4m3 byte on its grid (+0 and -0 share position 0): test_aim_fp8_gpu._code"""
    b = b.to(torch.int32)
    mag = b & 0x7F
    return torch.where(b >= 0x80, -mag, mag)


def q8_code(x):
    """code(q8(x)): the signed grid position of the saturating round-to-nearest-even cast of float64 `x` to e4m3, worked out
    on the 127 finite magnitudes themselves (no device cast involved)."""
    grid = torch.arange(127, dtype=torch.uint8).view(FP8).double().to(x.device)
    mids = (grid[:-1] + grid[1:]) / 2                          # exact in float64
    mag = x.abs().clamp(max=448.0)
    idx = torch.bucketize(mag, mids)                           # mids[idx - 1] < mag <= mids[idx]
    tie = (idx < 126) & (mag == mids[idx.clamp(max=125)])
    idx = idx + (tie & (idx % 2 == 1)).to(idx.dtype)           # a tie goes to the even code
    return torch.where(x < 0, -idx, idx).to(torch.int32)


def code_bytes(c):
    return torch.where(c < 0, 0x80 | (-c), c).to(torch.uint8)


# ------------------------------------------------------------------ float64 restatement -----------------------------------
MUTANTS = ("ws_col+4", "ws_ignored", "split+8", "at_next", "af_next", "vec_ldvN", "bt_ignored", "resid_ldrN", "sat_nan",
           "nosat_wrap", "bf16_trunc", "ktail_dropped")


def mutants(case: Case):
    s = case.spec
    on = {"ws_col+4": True, "ws_ignored": True, "split+8": s.epi == "act8" and s.n_split > 0,
          "at_next": s.at and not (s.epi == "act8" and s.n_split == s.N),          # (n_split = N: no column takes it)
          "af_next": s.af, "vec_ldvN": s.vec == "row0", "bt_ignored": s.bt, "resid_ldrN": s.resid, "sat_nan": s.sat,
          "nosat_wrap": s.sat, "bf16_trunc": s.epi in ("bf16", "res16"), "ktail_dropped": s.K % 128 != 0}
    return [m for m in MUTANTS if on[m]]


def accumulate(case: Case, inp, kdrop: bool = False):
    """(sum_k a w in float64, the bound's sum_k |a w| -- None for the exact family, whose accumulation has no error)"""
    s = case.spec
    K = s.K - (s.K % 128 if kdrop else 0)
    A, W = inp["A"][:, :K].double(), inp["W"][:, :K].double()
    acc = A @ W.T
    return acc, (None if case.family == "exact" else 2 * s.K * U24 * (A.abs() @ W.abs().T))


def _act_cols(s: Spec, x, n_split):
    f = {QGELU: qgelu, GELU: gelu}
    if n_split <= 0:
        return f[s.act](x)                               # no split: `act` on every column
    sec = torch.arange(s.N, device=x.device) >= n_split
    return torch.where(sec[None, :], f[s.act2](x), f[s.act](x))


def epilogue_terms(case: Case, inp, mut: Optional[str] = None, cache: Optional[dict] = None):
    """The float64 terms of the epilogue's sum (F32 / RES16: resid, rs * acc * wscale, rs * bias, vs * vec; BF16 and ACT8's
    pre-activation: acc * wscale, bias) with the row factors, and the accumulation bound."""
    s = case.spec
    dev = inp["A"].device
    cache = {} if cache is None else cache
    key = "kdrop" if mut == "ktail_dropped" else "acc"
    if key not in cache:
        cache[key] = accumulate(case, inp, key == "kdrop")
    acc, eabs = cache[key]
    ws = inp["wscale"].double()
    if mut == "ws_col+4":
        ws = ws.roll(-4)
    elif mut == "ws_ignored":
        ws = torch.ones_like(ws)
    accs = acc * ws[None, :]
    eacc = torch.zeros((), dtype=torch.float64, device=dev) if eabs is None else eabs * ws[None, :] + 2 * U24 * accs.abs()
    m = torch.arange(s.M, device=dev)
    rs = torch.ones(s.M, dtype=torch.float64, device=dev)
    vs = torch.zeros(s.M, dtype=torch.float64, device=dev)
    vrow = None
    if s.ntok:
        frame, tok = m // s.ntok, m % s.ntok
        if s.af:
            af = inp["af"].double()
            rs = rs * (af.roll(-1) if mut == "af_next" else af)[frame]
        if s.at:
            at = inp["at"].double()
            rs = rs * (at.roll(-1) if mut == "at_next" else at)[tok]
        if s.vec:
            vs = inp["bt"].double()[tok] if s.bt and mut != "bt_ignored" else torch.ones_like(vs)
            vec = inp["vec"].double()
            vrow = vec[frame] if (s.vec == "frame" or mut == "vec_ldvN") else vec[0].expand(s.M, s.N)
    bias = inp["bias"].double()[None, :] if s.bias else torch.zeros((1, s.N), dtype=torch.float64, device=dev)
    resid = None
    if s.resid:
        resid = inp["resid"].double()
        if mut == "resid_ldrN":            # the rows of the [M + 3, N + 8] buffer the residual lies in, read with ldr = N
            buf = torch.zeros((s.M + 3, s.N + 8), dtype=torch.float64, device=dev)
            buf[:s.M, :s.N] = resid
            resid = buf.flatten()[:s.M * s.N].view(s.M, s.N)
    return dict(accs=accs, eacc=eacc, rs=rs[:, None], vs=vs[:, None], vrow=vrow, bias=bias, resid=resid)


def expected(case: Case, inp, mut: Optional[str] = None, cache: Optional[dict] = None):
    """(float64 value, bound): what the kernel must write and how far it may be off (exact family, BF16 / F32 / RES16: the
    bound is not used, the value is exact in fp32).  ACT8: (y, e) before the cast.  `mut` names a deliberately wrong
    restatement (MUTANTS)."""
    s = case.spec
    t = epilogue_terms(case, inp, mut, cache)
    accs, eacc, rs, bias = t["accs"], t["eacc"], t["rs"], t["bias"]
    if s.epi == "bf16":
        ref = rs * (accs + bias)
        return ref, U8 * ref.abs() + rs.abs() * (eacc + 2 * U24 * (accs + bias).abs())
    if s.epi in ("f32", "res16"):
        resid = t["resid"] if t["resid"] is not None else torch.zeros_like(accs)
        vterm = t["vs"] * t["vrow"] if t["vrow"] is not None else torch.zeros_like(accs)
        ref = resid + rs * accs + rs * bias + vterm
        b = rs.abs() * eacc + 4 * U24 * ((rs * accs).abs() + (rs * bias).abs() + resid.abs() + vterm.abs())
        return ref, (b + U8 * ref.abs() if s.epi == "res16" else b)
    ns = s.n_split
    if mut == "split+8" and ns > 0:
        ns = ns + 8 if ns + 8 <= s.N else ns - 8
    cols = torch.arange(s.N, device=accs.device)
    rson = (cols >= ns) if ns > 0 else torch.ones_like(cols, dtype=torch.bool)
    rsc = torch.where(rson[None, :], rs, torch.ones_like(rs))
    pre = accs + bias
    y = rsc * _act_cols(s, pre, ns)
    e = rsc.abs() * EPS_ACT * (1 + pre.abs()) + 2 * U24 * y.abs()
    if case.family != "exact":
        e = e + 1.13 * rsc.abs() * (eacc + 2 * U24 * pre.abs())
    return y, e


def reassociations(case: Case, inp, cache: Optional[dict] = None):
    """(the float64 value, [the epilogue's sum in every order of its terms and with the row factor inside or outside the
    bracket, each partial result rounded to fp32]): on the exact family all of them must equal the float64 value."""
    import itertools
    s = case.spec
    t = epilogue_terms(case, inp, None, cache)

    def f(x):
        return x.float().double()

    accs, rs, bias = f(t["accs"]), t["rs"], t["bias"]
    if s.epi == "act8":                                      # the pre-activation
        return t["accs"] + bias, [f(accs + bias)]
    want = expected(case, inp, None, cache)[0]
    if s.epi == "bf16":
        return want, [f(rs * f(accs + bias)), f(f(rs * accs) + f(rs * bias))]
    rest = [x for x in (t["resid"], None if t["vrow"] is None else f(t["vs"] * t["vrow"])) if x is not None]
    out = []
    for head in ([f(rs * accs), f(rs * bias)], [f(rs * f(accs + bias))]):
        terms = head + rest
        for order in itertools.permutations(range(len(terms))):
            v = terms[order[0]]
            for i in order[1:]:
                v = f(v + terms[i])
            out.append(v)
    return want, out


def simulate(case: Case, inp, mut: Optional[str] = None, cache: Optional[dict] = None):
    """the output of a kernel that computes `expected(..., mut)` exactly and rounds once to the output dtype"""
    s = case.spec
    v, _ = expected(case, inp, mut, cache)
    if s.epi == "act8":
        b = code_bytes(q8_code(v))
        over = v.abs() > 448.0
        sign = torch.where(v < 0, 0x80, 0).to(torch.uint8)
        if mut == "sat_nan":                   # the cast's own overflow result instead of the clamp
            b = torch.where(over, sign | 0x7F, b)
        elif mut == "nosat_wrap":              # no clamp, and the largest finite code comes out with the wrong sign
            b = torch.where(over, (sign ^ 0x80) | 0x7E, b)
        return b
    v = v.float()
    if mut == "bf16_trunc":
        v = (v.view(torch.int32) & -65536).view(F32)
    return v.to(OUT_DTYPE[s.epi])


def check(case: Case, inp, got, cache: Optional[dict] = None) -> Dict[str, float]:
    """The figures the tests assert on: `unequal` (exact family, BF16 / F32 / RES16) or `ratio` = worst error / bound
    (random family); ACT8: `outside` the byte interval, `nan_codes`, and the `ambiguous` share of the reference."""
    s = case.spec
    cache = {} if cache is None else cache
    if "ref" not in cache:
        cache["ref"] = expected(case, inp, None, cache)
    ref, bound = cache["ref"]
    if s.epi == "act8":
        lo, hi = q8_code(ref - bound), q8_code(ref + bound)
        b = got.view(torch.uint8)
        c = _code(b)
        return {"outside": int(((c < lo) | (c > hi)).sum()), "nan_codes": int(((b & 0x7F) == 0x7F).sum()),
                "ambiguous": float((lo != hi).double().mean())}
    if case.family == "exact":
        want = ref.float().to(OUT_DTYPE[s.epi])
        return {"unequal": int((~(got == want)).sum())}
    return {"ratio": ratio(got, ref, bound)}


def passes(fig: Dict[str, float]) -> bool:
    return (fig.get("unequal", 0) == 0 and fig.get("ratio", 0.0) <= 1.0 and fig.get("outside", 0) == 0
            and fig.get("nan_codes", 0) == 0)


# ------------------------------------------------------------------ the child: one route, every case ------------------------
def _wide(M, N, dtype, dev, pad):
    """[M, N] view into a canary-filled [M + 3, N + pad] buffer: NaN, or the byte 0xA5 for an fp8 output"""
    if dtype == torch.uint8:
        buf = torch.full((M + 3, N + pad), CANARY, dtype=torch.uint8, device=dev)
    elif pad == 8:
        return _padded(M, N, dtype, dev)
    else:
        buf = torch.full((M + 3, N + pad), float("nan"), dtype=dtype, device=dev)
    return buf[:M, :N], buf


def _wide_intact(buf, M, N) -> bool:
    if buf.dtype != torch.uint8:
        return _pad_intact(buf, M, N)
    b = buf.clone()
    b[:M, :N] = CANARY
    return bool((b == CANARY).all())


def _operand(t, pad, dev):
    """the fp8 operand on the device; with `pad`, as the first K columns of a buffer whose spare bytes are the e4m3 NaN"""
    t = t.to(dev)
    if not pad:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + pad), 0x7F, dtype=torch.uint8, device=dev)
    buf[:, :t.shape[1]] = t.view(torch.uint8)
    return buf.view(FP8)[:, :t.shape[1]]


def call_kwargs(ops, s: Spec, inp, dev):
    """the keyword arguments of `ops.gemm_fp8` for `s` (the residual a view with ldr = N + 8)"""
    kw = dict(bias=inp.get("bias"), af=inp.get("af"), at=inp.get("at"), bt=inp.get("bt"), ntok=s.ntok)
    if s.resid:
        kw["resid"], _ = _padded(s.M, s.N, inp["resid"].dtype, dev)
        kw["resid"].copy_(inp["resid"])
    if s.vec:
        kw.update(vec=inp["vec"], ldv=0 if s.vec == "row0" else None)
    if s.epi == "act8":
        kw.update(act=s.act, act2=s.act2, n_split=s.n_split)
    epi = {"bf16": ops.EPI_BF16, "f32": ops.EPI_F32, "res16": ops.EPI_RES16, "act8": ops.EPI_ACT8}[s.epi]
    return epi, kw


def run_case(ops, case: Case, route: str, cus: int, dev):
    s = case.spec
    plan = route_plan(case, route, cus)
    inp = {k: v.to(dev) for k, v in make_inputs(case).items()}
    rec = {"kernel": plan[0], "probe_expected": plan[1], "family": case.family, "epi": s.epi, "checks": {}, "hash": {},
           "pad": {}}
    tiles = ((s.M + 255) // 256) * ((s.N + 255) // 256)
    probe = torch.zeros((tiles + 2 * cus + 64, 4), dtype=torch.int64, device=dev)
    A, W = _operand(inp["A"], s.ld_pad, dev), _operand(inp["W"], s.ld_pad, dev)
    epi, kw = call_kwargs(ops, s, inp, dev)
    got, bufs = {}, {}
    for name, extra in [("out", dict(probe=probe))] + ([(f"out@rc{rc}", dict(reserve_cus=rc)) for rc in (16, 64)]
                                                       if case.reserve else []):
        got[name], bufs[name] = _wide(s.M, s.N, OUT_DTYPE[s.epi], dev, s.ldo_pad)
        out = got[name].view(FP8) if s.epi == "act8" else got[name]
        ops.gemm_fp8(A, W, inp["wscale"], epi, out, **kw, **extra)
    torch.cuda.synchronize()
    rec["probe_written"] = int((probe != 0).any(dim=1).sum())
    cache = {}
    for k in got:
        rec["pad"][k] = _wide_intact(bufs[k], s.M, s.N)
        rec["hash"][k] = _digest(got[k])
        rec["checks"][k] = check(case, inp, got[k], cache)
    return rec


def main(argv):
    route, path = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    dev = torch.device("cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"route": route, "cus": cus, "cases": {}}
    t0 = time.time()
    with torch.no_grad():
        for case in cases(cus):
            if route_plan(case, route, cus) is None:
                continue
            res["cases"][case.name] = run_case(ops, case, route, cus, dev)
    res["seconds"] = time.time() - t0
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
