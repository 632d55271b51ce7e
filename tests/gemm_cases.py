"""The product's GEMM call forms, rebuilt with their exact options, and a float64 restatement of every epilogue.

A plain module (no fixtures): `test_gemm_routes_gpu.py` runs each case on every kernel route it can take, one child process
per route (`python gemm_cases.py ROUTE OUT.json`), and `test_gemm_cases_cpu.py` proves on the CPU that the comparison
rejects the bugs it is meant to catch.

Bounds (`expected`): u = 2^-24 (fp32), a bf16 result is off by at most 2^-8 of its value (half an ulp), and the fp32
accumulation of K exact bf16 (or e4m3) products is off by at most K u sum_k |a_k w_k| (taken twice, for the rounding of a
result that is itself off).  The activation epilogues evaluate sigmoid / a 1.5e-7-accurate erf in fp32: EPS_ACT (1 + |x|).
"""
import hashlib
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, Optional

import torch

U24 = 2.0 ** -24
U8 = 2.0 ** -8
EPS_ACT = 2.0 ** -20
QGELU, GELU = 0, 1
BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn

# D, adapter width r, tokens per frame
GEOMS = {"b16": (768, 192, 197), "l14": (1024, 256, 257), "tiny": (128, 32, 5)}     # tiny: tests/golden/make_golden.py
ROUTES = ("256", "peel", "128", "small", "expsum128")
ROUTE_ENV = {"256": {"AIM_GEMM_PEEL": "0"}, "peel": {},
             "128": {"AIM_GEMM_TILE": "128", "AIM_GEMM_SMALL": "0"},
             "small": {"AIM_GEMM_TILE": "128", "AIM_GEMM_SMALL": "1000000000"},
             "expsum128": {"AIM_EXPSUM_256": "0"}}
ROUTE_VARS = ("AIM_GEMM_PEEL", "AIM_GEMM_TILE", "AIM_GEMM_SMALL", "AIM_EXPSUM_256")


@dataclass(frozen=True)
class Spec:
    epi: str                  # bf16 | act | dact | f32 | fp8_f32 | fp8_res16
    M: int
    N: int
    K: int
    ntok: int = 0
    lda: int = 0              # A = columns [a_off, a_off + K) of an [M, lda] buffer (0: lda = K)
    a_off: int = 0
    ldw: int = 0              # W = columns [w_off, w_off + K) of an [N, ldw] buffer
    w_off: int = 0
    bias: bool = False
    resid: bool = False
    af: bool = False
    at: bool = False
    vec: str = ""             # "frame": one row per frame (ldv = N); "row0": ldv = 0, one row for every frame
    bt: bool = False
    act: int = QGELU
    act2: int = QGELU
    n_split: int = 0
    rs_bias_only: bool = False
    w_scale: float = 1.0      # ACT: 1.5 -> pre-activations over about [-4, 4]
    bias_scale: float = 1.0


@dataclass(frozen=True)
class Case:
    name: str
    form: str
    site: str
    spec: Spec
    seed: int = 0
    frag: bool = False        # ACT: also the fragment-ordered side buffer and its DACT twin (256 routes, M >= 1024)
    reserve: bool = False     # also reserve_cus = 16 and 64: must give the same bits
    batch: int = 1            # EXPSUM
    slot_stride: int = 0      # EXPSUM: floats between batch items' slots (0: packed)
    rows: int = 0             # EXPSUM: rows per item in the qkv buffer (>= M)


# ------------------------------------------------------------------ the case table ----------------------------------------
def forms(geom: str, M: int) -> Dict[str, tuple]:
    """form -> (Spec, call site, Case options) at M rows of geometry `geom`."""
    D, r, ntok = GEOMS[geom]
    H4, C = 4 * D, 4 * D + r
    act_in = dict(w_scale=1.5, bias_scale=0.3)
    return {
        "qkv": (Spec("bf16", M, 3 * D, D, bias=True), "backbone.py:504", dict(reserve=True)),
        "x1": (Spec("f32", M, D, D, ntok, bias=True, resid=True, af=True, vec="frame", bt=True), "backbone.py:599", {}),
        "mlp_act": (Spec("act", M, C, D, ntok, bias=True, at=True, act=QGELU, act2=GELU, n_split=H4, **act_in),
                    "backbone.py:628", dict(frag=True)),
        "x2": (Spec("f32", M, D, C, ntok, bias=True, resid=True, vec="row0", bt=True), "backbone.py:631", {}),
        "mlp_dact": (Spec("dact", M, C, D, ntok, at=True, act=QGELU, act2=GELU, n_split=H4), "backbone.py:652",
                     dict(reserve=True)),
        "dgrad_cat": (Spec("bf16", M, D, C), "backbone.py:659", {}),
        "dgrad_o": (Spec("bf16", M, D, D, ntok, af=True), "backbone.py:735", {}),
        "aim_t_act": (Spec("act", M, r, D, ntok, bias=True, at=True, act=GELU, **act_in), "aim_variant.py:49", {}),
        "aim_t_f32": (Spec("f32", M, D, r, ntok, resid=True, vec="row0", bt=True), "aim_variant.py:51", {}),
        "aim_t_dact": (Spec("dact", M, r, D, ntok, at=True, act=GELU), "aim_variant.py:114", {}),
        "f32_rs_bias_only": (Spec("f32", M, D, D, ntok, bias=True, resid=True, at=True, rs_bias_only=True),
                             "aim_kernels.h AIM_EPI_F32 rs_bias_only", {}),
        # class-token chain: M = B*T rows
        "cls_strided_a": (Spec("f32", M, D, D, lda=2 * D, a_off=D, bias=True), "backbone.py:475", {}),
        "cls_strided_w": (Spec("bf16", M, D, D, ldw=3 * D, w_off=2 * D), "backbone.py:714", {}),
        "ad_small_act": (Spec("act", M, r, D, bias=True, act=GELU, **act_in), "backbone.py:440", {}),
        "ad_small_dact": (Spec("dact", M, r, D, act=GELU), "backbone.py:673", {}),
        # fp8 inference (large M only)
        "fp8_x2_f32": (Spec("fp8_f32", M, D, C, ntok, bias=True, resid=True, vec="row0", bt=True), "backbone.py:596", {}),
        "fp8_x2_res16": (Spec("fp8_res16", M, D, C, ntok, bias=True, resid=True, vec="row0", bt=True), "backbone.py:586,596",
                         {}),
    }


TOKEN_FORMS = ("qkv", "x1", "mlp_act", "x2", "mlp_dact", "dgrad_cat", "dgrad_o", "aim_t_act", "aim_t_f32", "aim_t_dact",
               "f32_rs_bias_only")
CLS_FORMS = ("cls_strided_a", "cls_strided_w", "ad_small_act", "ad_small_dact")
FP8_FORMS = ("fp8_x2_f32", "fp8_x2_res16")
# frames per geometry: natural small (M <= 256), 128 (257 <= M < 1024) and 256 (M >= 1024) routes
FRAMES = {"b16": (1, 2, 6), "l14": (1, 2, 4), "tiny": (40, 100, 256)}
CLS_ROWS = (96, 512, 1200)
# BF16 / F32 forms (and the fp8 RES16 form) also at a row count whose last tile round the library peels
PEEL_FORMS = (("qkv", "b16"), ("x1", "b16"), ("dgrad_o", "l14"), ("aim_t_f32", "l14"), ("fp8_x2_res16", "l14"))


def peel_rows(M: int, N: int, cus: int, reserve: int = 0) -> int:
    """Mirror of csrc/gemm.hip::aim_gemm_peel_rows: rows of the whole tile rounds (0: no peel)."""
    c = cus - reserve if cus - reserve > 8 else 8
    tn, tm = (N + 255) // 256, (M + 255) // 256
    tiles = tm * tn
    full, left = tiles // c, tiles % c
    lrt = (left + tn - 1) // tn
    if full >= 2 and left > 0 and lrt <= 2 and left * 8 <= c and (tm - lrt) * tn <= full * c:
        return (tm - lrt) * 256
    return 0


def peel_frames(N: int, ntok: int, cus: int) -> int:
    f0 = (2 * cus // ((N + 255) // 256)) * 256 // ntok
    for f in range(f0, f0 + 4 * 256 // ntok + 16):
        if peel_rows(f * ntok, N, cus):
            return f
    raise AssertionError(f"no peeled row count near {f0} frames (N={N}, ntok={ntok}, {cus} CUs)")


def cases(cus: int = 256):
    out = []
    seed = 100
    for geom in GEOMS:
        ntok = GEOMS[geom][2]
        sizes = [(f, f * ntok) for f in FRAMES[geom]]
        for name in TOKEN_FORMS + FP8_FORMS:
            for f, M in sizes:
                spec, site, opt = forms(geom, M)[name]
                if name in FP8_FORMS and (M < 1024 or ntok < 128):
                    continue
                out.append(Case(f"{name}/{geom}/M{M}", name, site, spec, seed, **opt))
                seed += 1
        for name in CLS_FORMS:
            for M in CLS_ROWS:
                spec, site, opt = forms(geom, M)[name]
                out.append(Case(f"{name}/{geom}/M{M}", name, site, spec, seed, **opt))
                seed += 1
    for name, geom in PEEL_FORMS:
        ntok = GEOMS[geom][2]
        M = peel_frames(forms(geom, ntok)[name][0].N, ntok, cus) * ntok
        spec, site, opt = forms(geom, M)[name]
        out.append(Case(f"{name}/{geom}/M{M}/peel", name, site, spec, seed, **dict(opt, reserve=False, frag=False)))
        seed += 1
    # EXPSUM (lamda's `ow`, backbone.py:518,539,542): batch of frames, scale 1/8
    for tag, n, rows, D, ss in (("n197", 197, 197, 768, 0), ("n257", 257, 257, 1024, 0),
                                ("border256", 256, 257, 1024, 20)):       # border: 10 slots per frame, 8 from the GEMM
        out.append(Case(f"expsum/{tag}", "expsum", "backbone.py:518-543", Spec("expsum", n, n, D), seed, batch=3,
                        slot_stride=ss, rows=rows))
        seed += 1
    return out


def route_plan(case: Case, route: str, cus: int):
    """(kernel, tiles the persistent 256 x 256 kernel processes) for `case` under `route`'s environment: a mirror of the
    dispatch in csrc/gemm.hip::aim_gemm_launch and capi.hip::aim_gemm_fp8.  None: the case does not run there."""
    s = case.spec
    tiles = ((s.M + 255) // 256) * ((s.N + 255) // 256)
    if s.epi == "expsum":
        if route not in ("256", "expsum128"):
            return None
        use256 = route != "expsum128" and (s.M > 128 or s.N > 128) and s.M <= 256 and s.N <= 256
        return ("256", case.batch) if use256 and s.K % 64 == 0 else ("128", 0)
    if s.epi.startswith("fp8"):
        if route not in ("256", "peel"):
            return None
        m0 = peel_rows(s.M, s.N, cus) if s.epi == "fp8_res16" and s.K % 128 == 0 else 0
        if route == "peel":
            return ("peel", (m0 // 256) * ((s.N + 255) // 256)) if m0 else None
        return ("256", tiles)
    if route == "expsum128":
        return None
    wide_ok = s.N % 8 == 0 and s.n_split % 8 == 0 and s.K % 64 == 0 and (s.epi != "f32" or not s.vec or s.ntok >= 128)
    on256 = s.M >= 1024 and s.N >= 64 and wide_ok
    if route == "peel":                   # the default environment: only where it differs from route "256"
        m0 = peel_rows(s.M, s.N, cus) if on256 and s.epi in ("bf16", "f32") else 0
        return ("peel", (m0 // 256) * ((s.N + 255) // 256)) if m0 else None
    if route == "256":                    # (and problems below 1024 rows on their natural kernel)
        if on256:
            return ("256", tiles)
        return ("small", 0) if s.M <= 256 and s.K % 64 == 0 else ("128", 0)
    if route == "128":
        return ("128", 0)
    return ("small", 0) if s.K % 64 == 0 else ("128", 0)


# ------------------------------------------------------------------ inputs (CPU, fixed seeds) ------------------------------
def _frames(s: Spec) -> int:
    return (s.M + s.ntok - 1) // s.ntok if s.ntok else 1


def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    s = case.spec
    g = torch.Generator().manual_seed(case.seed)

    def rn(*shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale

    inp = {}
    if s.epi == "expsum":
        inp["qkv"] = (rn(case.batch * case.rows, 3 * s.K) * 0.5).to(BF16)
        return inp
    lda, ldw = s.lda or s.K, s.ldw or s.K
    if s.epi.startswith("fp8"):
        inp["A_buf"] = rn(s.M, lda).clamp(-448, 448).to(FP8)
        w = rn(s.N, ldw, scale=s.K ** -0.5)
        sc = w.abs().amax(dim=1).clamp_min(1e-12) / 448.0                 # ops.quantize_fp8_rows
        inp["W_buf"] = (w / sc[:, None]).clamp(-448.0, 448.0).to(FP8)
        inp["wscale"] = sc.float()
    else:
        inp["A_buf"] = rn(s.M, lda).to(BF16)
        inp["W_buf"] = rn(s.N, ldw, scale=s.w_scale * s.K ** -0.5).to(BF16)
    frames = _frames(s)
    if s.bias:
        inp["bias"] = rn(s.N, scale=s.bias_scale)
    if s.resid:
        inp["resid"] = rn(s.M, s.N).to(BF16 if s.epi == "fp8_res16" else F32)
    if s.af:                                         # 1 - lamda: differs per frame
        inp["af"] = torch.rand(frames, generator=g) * 0.7 + 0.3
    if s.at:                                         # DropPath mask * adapter scale / keep: dropped tokens are 0
        keep = torch.rand(s.ntok, generator=g) < 0.7
        keep[0], keep[-1] = True, False
        inp["at"] = keep.float() * (0.5 / 0.7)
    if s.bt:                                         # differs per token, some dropped
        bt = torch.rand(s.ntok, generator=g) + 0.25
        bt[1::7] = 0.0
        inp["bt"] = bt
    if s.vec:                                        # "row0": rows >= 1 are decoys the kernel must not read
        inp["vec"] = rn(max(frames, 2), s.N)
    if s.epi == "dact":                              # saved pre-activations over about [-4, 4], and their derivative
        pre = rn(s.M, s.N, scale=1.6).to(BF16)
        inp["aux_pre"] = pre
        inp["aux_d"] = act_grad_cols(s, pre.double(), s.n_split).to(BF16)
    return inp


def operands(s: Spec, inp):
    A = inp["A_buf"][:, s.a_off:s.a_off + s.K]
    W = inp["W_buf"][:, s.w_off:s.w_off + s.K]
    return A, W


# ------------------------------------------------------------------ float64 restatement -----------------------------------
def qgelu(x):
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad(x):
    sg = torch.sigmoid(1.702 * x)
    return sg * (1 + 1.702 * x * (1 - sg))


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _second(s: Spec, n_split: int, device):
    """columns that take act2 and the row factor (all of them without a split)"""
    cols = torch.arange(s.N, device=device)
    return cols >= n_split if n_split > 0 else torch.ones(s.N, dtype=torch.bool, device=device)


def _act_cols(s: Spec, x, n_split, grad=False):
    sec = _second(s, n_split, x.device)
    f = {QGELU: qgelu_grad if grad else qgelu, GELU: gelu_grad if grad else gelu}
    a1, a2 = f[s.act](x), f[s.act2](x)
    if n_split <= 0:
        return a1                                       # no split: `act` on every column
    return torch.where(sec[None, :], a2, a1)


def act_grad_cols(s: Spec, x, n_split):
    return _act_cols(s, x, n_split, grad=True)


def _row_factors(s: Spec, inp, mut, device):
    m = torch.arange(s.M, device=device)
    rs = torch.ones(s.M, dtype=torch.float64, device=device)
    vs = torch.zeros(s.M, dtype=torch.float64, device=device)
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
            vs = inp["bt"].double()[tok] if s.bt else torch.ones_like(vs)
            vec = inp["vec"].double()
            vrow = vec[frame] if (s.vec == "frame" or mut == "vec_ldvN") else vec[0].expand(s.M, s.N)
    return rs[:, None], vs[:, None], vrow


def expected(case: Case, inp, got=None, mut: Optional[str] = None):
    """{output: (float64 value, bound)}: what the kernel must write, and how far it may be off.  ACT's `post` / `d` are
    stated on the kernel's own bf16 `pre` (got["pre"]).  `mut` names a deliberately wrong restatement (MUTANTS)."""
    s = case.spec
    dev = inp["A_buf"].device
    A, W = operands(s, inp)
    acc = A.double() @ W.double().T
    eacc = 2 * s.K * U24 * (A.double().abs() @ W.double().abs().T)      # fp32 accumulation of K exact products
    if s.epi.startswith("fp8"):
        ws = inp["wscale"].double()[None, :]
        acc, eacc = acc * ws, eacc * ws + 2 * U24 * (acc * ws).abs()
    rs, vs, vrow = _row_factors(s, inp, mut, dev)
    bias = inp["bias"].double()[None, :] if s.bias else torch.zeros((1, s.N), dtype=torch.float64, device=dev)
    out = {}
    if s.epi == "bf16":
        ref = rs * (acc + bias)
        out["out"] = (ref, U8 * ref.abs() + rs.abs() * (eacc + 2 * U24 * (acc + bias).abs()))
    elif s.epi in ("f32", "fp8_f32", "fp8_res16"):
        resid = inp["resid"].double() if s.resid else torch.zeros_like(acc)
        vterm = vs * vrow if vrow is not None else torch.zeros_like(acc)
        ms = rs if not s.rs_bias_only or mut == "rs_bias_only_ignored" else torch.ones_like(rs)
        ref = resid + ms * acc + rs * bias + vterm
        # fp32: the accumulation, then a handful of multiply / fma / add roundings on terms no larger than these
        b = ms.abs() * eacc + 4 * U24 * ((ms * acc).abs() + (rs * bias).abs() + resid.abs() + vterm.abs())
        if s.epi == "fp8_res16":
            b = b + U8 * ref.abs()
        out["out"] = (ref, b)
    elif s.epi == "act":
        ns = s.n_split + (4 if mut == "split+4" and s.n_split else 0)
        sec = _second(s, ns, dev)[None, :]
        rsc = torch.where(sec, rs, torch.ones_like(rs))
        pre_ref = acc + bias
        out["pre"] = (pre_ref, U8 * pre_ref.abs() + eacc + 2 * U24 * pre_ref.abs())
        if got is None or "pre" not in got:
            return out
        pre = got["pre"].double()
        post = rsc * _act_cols(s, pre, ns)
        bpost = U8 * post.abs() + rsc.abs() * EPS_ACT * (1 + pre.abs())
        out["post"] = (post, bpost)
        out["post_ag"] = (post, bpost)
        d = act_grad_cols(s, pre, ns)
        out["d"] = (pre if mut == "aux_grad_swap" else d, U8 * d.abs() + 2 * EPS_ACT * (1 + pre.abs()))
    elif s.epi == "dact":
        ns = s.n_split + (4 if mut == "split+4" and s.n_split else 0)
        sec = _second(s, ns, dev)[None, :]
        rsc = torch.where(sec, rs, torch.ones_like(rs))
        v = acc + bias
        ev = eacc + 2 * U24 * v.abs()
        for name, aux, ag in (("g", inp["aux_pre"], False), ("g_ag", inp["aux_d"], True)):
            aux = aux.double()
            dv = aux if ag != (mut == "aux_grad_swap") else act_grad_cols(s, aux, ns)
            ref = rsc * v * dv
            b = U8 * ref.abs() + rsc.abs() * (dv.abs() * ev + (0 if ag else 2 * EPS_ACT) * v.abs() * (1 + aux.abs())) \
                + 4 * U24 * ref.abs()
            out[name] = (ref, b)
    return out


MUTANTS = ("split+4", "at_next", "af_next", "vec_ldvN", "aux_grad_swap", "rs_bias_only_ignored")


def mutants(s: Spec):
    on = {"split+4": s.n_split > 0, "at_next": s.at, "af_next": s.af, "vec_ldvN": s.vec == "row0",
          "aux_grad_swap": s.epi in ("act", "dact"), "rs_bias_only_ignored": s.rs_bias_only}
    return [m for m in MUTANTS if on[m]]


def out_dtype(case: Case, name: str):
    return F32 if case.spec.epi in ("f32", "fp8_f32") else BF16


def ratio(got, ref, bound) -> float:
    """worst |got - ref| / bound (0 / 0 = 0; non-finite -> inf)"""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
    r = torch.nan_to_num(r, nan=math.inf)
    return float(r.max()) if r.numel() else 0.0


def compare(case: Case, inp, got) -> Dict[str, float]:
    exp = expected(case, inp, got)
    return {k: ratio(got[k], *exp[k]) for k in exp if k in got}


def simulate(case: Case, inp, mut: Optional[str] = None):
    """the outputs of a kernel that computes `expected(..., mut)` exactly and rounds once to the output dtype"""
    got = {}
    if case.spec.epi == "act":
        got["pre"] = expected(case, inp, None, mut)["pre"][0].to(BF16)
    for k, (v, _) in expected(case, inp, got, mut).items():
        if k != "pre":
            got[k] = v.to(out_dtype(case, k))
    return got


# ------------------------------------------------------------------ the child: one route, every case ------------------------
def _digest(t) -> str:
    t = t.contiguous()
    return hashlib.sha1(t.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def _padded(M, N, dtype, dev):
    """[M, N] view into an NaN-filled [M + 3, N + 8] buffer (ldo > N, spare rows)"""
    buf = torch.full((M + 3, N + 8), float("nan"), dtype=dtype, device=dev)
    return buf[:M, :N], buf


def _pad_intact(buf, M, N) -> bool:
    iv = {2: torch.int16, 4: torch.int32}[buf.element_size()]
    fill = torch.full((1,), float("nan"), dtype=buf.dtype).view(iv).item()
    bits = buf.view(iv).clone()
    bits[:M, :N] = fill
    return bool((bits == fill).all())


def run_case(ops, case: Case, route: str, cus: int, dev):
    s = case.spec
    plan = route_plan(case, route, cus)
    inp = {k: v.to(dev) for k, v in make_inputs(case).items()}
    rec = {"kernel": plan[0], "probe_expected": plan[1], "checks": {}, "hash": {}, "pad": {}, "finite": {}}
    tiles = ((s.M + 255) // 256) * ((s.N + 255) // 256) * case.batch
    probe = torch.zeros((tiles + 2 * cus + 64, 4), dtype=torch.int64, device=dev)
    got, bufs = {}, {}

    def new(name, dtype):
        v, b = _padded(s.M, s.N, dtype, dev)
        got[name], bufs[name] = v, b
        return v

    if s.epi == "expsum":
        return run_expsum(ops, case, inp, rec, probe, dev)
    A, W = operands(s, inp)
    kw = dict(bias=inp.get("bias"), resid=inp.get("resid"), af=inp.get("af"), at=inp.get("at"), bt=inp.get("bt"),
              ntok=s.ntok)
    if s.vec:
        kw.update(vec=inp["vec"], ldv=0 if s.vec == "row0" else None)
    sp = dict(act=s.act, act2=s.act2, n_split=s.n_split)
    if s.epi == "bf16":
        ops.gemm(A, W, ops.EPI_BF16, new("out", BF16), probe=probe, **kw)
        if case.reserve:
            for rc in (16, 64):
                ops.gemm(A, W, ops.EPI_BF16, new(f"out@rc{rc}", BF16), reserve_cus=rc, **kw)
    elif s.epi == "f32":
        ops.gemm(A, W, ops.EPI_F32, new("out", F32), probe=probe, rs_bias_only=s.rs_bias_only, **kw)
    elif s.epi.startswith("fp8"):
        epi = ops.EPI_F32 if s.epi == "fp8_f32" else ops.EPI_RES16
        ops.gemm_fp8(A, W, inp["wscale"], epi, new("out", F32 if s.epi == "fp8_f32" else BF16), probe=probe, **kw)
    elif s.epi == "act":
        ops.gemm(A, W, ops.EPI_ACT, new("post", BF16), out2=new("pre", BF16), probe=probe, **kw, **sp)
        ops.gemm(A, W, ops.EPI_ACT, new("post_ag", BF16), out2=new("d", BF16), aux_grad=True, **kw, **sp)
        if case.frag and plan[0] in ("256", "peel"):
            # the fragment-ordered side buffer: same `post`, and the DACT twin reads it back to the same bits
            g2 = torch.Generator().manual_seed(case.seed + 7)
            G = torch.randn((s.M, s.K), generator=g2).to(BF16).to(dev)
            W2 = (torch.randn((s.N, s.K), generator=g2) * s.K ** -0.5).to(BF16).to(dev)
            dkw = dict(at=kw["at"], ntok=s.ntok, **sp)
            for ag, aux in ((False, got["pre"]), (True, got["d"])):
                t = "_ag" if ag else ""
                fb = ops.frag_buffer(s.M, s.N, dev)
                ops.gemm(A, W, ops.EPI_ACT, new("post_frag" + t, BF16), out2=fb, aux_grad=ag, aux_frag=True, **kw, **sp)
                ops.gemm(G, W2, ops.EPI_DACT, new("dact_rowmajor" + t, BF16), aux=aux, aux_grad=ag, **dkw)
                ops.gemm(G, W2, ops.EPI_DACT, new("dact_frag" + t, BF16), aux=fb, aux_grad=ag, aux_frag=True, **dkw)
    elif s.epi == "dact":
        kw = dict(at=kw["at"], ntok=s.ntok, bias=kw["bias"])
        auxes = {}
        for k in ("aux_pre", "aux_d"):                   # saved rows with a row stride > N
            v, _ = _padded(s.M, s.N, BF16, dev)
            v.copy_(inp[k])
            auxes[k] = v
        ops.gemm(A, W, ops.EPI_DACT, new("g", BF16), aux=auxes["aux_pre"], probe=probe, **kw, **sp)
        ops.gemm(A, W, ops.EPI_DACT, new("g_ag", BF16), aux=auxes["aux_d"], aux_grad=True, **kw, **sp)
        if case.reserve:
            for rc in (16, 64):
                ops.gemm(A, W, ops.EPI_DACT, new(f"g@rc{rc}", BF16), aux=auxes["aux_pre"], reserve_cus=rc, **kw, **sp)
    torch.cuda.synchronize()
    rec["probe_written"] = int((probe != 0).any(dim=1).sum())
    for k in got:
        rec["finite"][k] = bool(torch.isfinite(got[k].float()).all())
        rec["pad"][k] = _pad_intact(bufs[k], s.M, s.N)
        rec["hash"][k] = _digest(got[k])
    rec["checks"] = compare(case, inp, got)
    return rec


def run_expsum(ops, case: Case, inp, rec, probe, dev):
    s = case.spec
    B, D, n, rows = case.batch, s.K, s.M, case.rows
    nt = ops.expsum_tiles(n, n)                     # pairs per item, as the library reports them
    stride = case.slot_stride or 2 * nt
    buf = torch.full((B + 1, stride + 8), float("nan"), device=dev)        # a spare item and room behind each
    part = buf.view(-1)[:B * stride]
    qkv = inp["qkv"]
    ops.gemm(qkv[:, :D], qkv[:, D:], ops.EPI_EXPSUM, part, M=n, N=n, K=D, batch=B, stride_a=rows * 3 * D,
             stride_w=rows * 3 * D, scale=0.125, slot_stride=case.slot_stride, probe=probe)
    torch.cuda.synchronize()
    rec["probe_written"] = int((probe != 0).any(dim=1).sum())
    flat = buf.view(-1)
    idx = (torch.arange(B, device=dev)[:, None] * stride + torch.arange(2 * nt, device=dev)[None, :]).reshape(-1)
    slots = flat[idx].reshape(B, nt, 2)
    rec["finite"]["part"] = bool(not torch.isnan(slots).any() and (slots[..., 1] >= 0).all())     # (an empty part: (-inf, 0))
    rest = torch.ones_like(flat, dtype=torch.bool)
    rest[idx] = False
    rec["pad"]["part"] = bool(torch.isnan(flat[rest]).all())
    rec["hash"]["part"] = _digest(slots)
    q = qkv[:, :D].double().reshape(B, rows, D)[:, :n]
    k = qkv[:, D:2 * D].double().reshape(B, rows, D)[:, :n]
    sc = torch.einsum("bik,bjk->bij", q, k) * 0.125
    err = torch.einsum("bik,bjk->bij", q.abs(), k.abs()) * 0.125 * 2 * D * U24       # fp32 accumulation of the scores
    ref = torch.logsumexp(sc.reshape(B, -1), dim=1)
    got = torch.logsumexp(slots[..., 0].double() + torch.log(slots[..., 1].double()), dim=1)
    # lse of a tiled (max, sum exp) in fp32: the score error, plus exp and ~100 sequential / tree additions per tile
    bound = 2 * err.reshape(B, -1).amax(dim=1) + 256 * U24 + 2 * U24 * ref.abs()
    rec["checks"]["lse"] = ratio(got, ref, bound)
    return rec


def main(argv):
    route, path = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    dev = torch.device("cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"route": route, "cus": cus, "cases": {}}
    with torch.no_grad():
        for case in cases(cus):
            if route_plan(case, route, cus) is None:
                continue
            res["cases"][case.name] = run_case(ops, case, route, cus, dev)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
