"""The call forms of the fused low-rank adapter kernels (aim_lowrank_fwd / aim_lowrank_bwd, csrc/lowrank.hip), and a float64
restatement of both with bounds.

A plain module (no fixtures): `test_lowrank_gpu.py` runs every case on the kernels, `test_lowrank_cases_cpu.py` proves on the
CPU that the comparison rejects the bugs it is meant to catch.  Two tables: cases() (real widths, few sizes) and
sweep_groups() (every r, every last-tile row count, the narrowest and the widest D, the rarer call forms).

  forward    H_g = bf16(X W1_g^T + b1_g)           Y_g = alpha X + H_g W2_g^T + b2_g       (fp32 form, G = 1: resid + the same)
  backward   dH_g = bf16(dY_g W2_g)                dX = bf16(alpha sum_g dY_g + sum_g dH_g W1_g)

Bounds, derived as in gemm_cases.py: u = 2^-24 (fp32), a bf16 result is off by at most 2^-8 of its value, and the fp32
accumulation of K exact bf16 products is off by at most K u sum_k |a_k w_k| (taken twice, for the rounding of a result that is
itself off).  H and dH are checked against the inputs.  Y and dX are checked against the kernel's OWN stored H / dH: the second
product reads the rounded intermediate, so nothing of the first product's error enters their bound and it stays sharp.
"""
import os
import sys
from dataclasses import dataclass
from typing import Dict, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import BF16, F32, U8, U24, _digest, _pad_intact, _padded, ratio  # noqa: E402,F401

# one row; one short of / one past a forward tile of 128 (two backward tiles of 64, four of 32); 8 forward tiles (16 / 32
# backward tiles) and 5 rows
ROWS = (1, 127, 129, 1029)
WIDTHS = ((128, 32), (256, 8), (768, 192), (1024, 256))     # the tiny fixtures' width, the smallest r, ViT-B/16, ViT-L/14


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    D: int
    r: int
    G: int
    alpha: float
    seed: int = 0
    bias: str = "both"          # both | b1 | b2 | none: the biases that are passed; the wrapper gets None for the rest
    form: str = "std"           # std | y_y32 (G = 1: also y[0] and y32 from one call) | h1 (G = 3: also H of adapter 1 alone)


def cases():
    out, seed = [], 500
    for M in ROWS:
        for D, r in WIDTHS:
            for G in (1, 3):
                for alpha in (1.0, 2.0):
                    out.append(Case(f"M{M}/D{D}/r{r}/G{G}/a{int(alpha)}", M, D, r, G, alpha, seed))
                    seed += 1
    return out


SWEEP_M = 161                       # 128 + 33 forward rows; 2 x 64 + 33 and 5 x 32 + 1 in the two backward kernels
SWEEP_R = tuple(range(8, 257, 8))
SWEEP_D = (64, 192)                 # nk = 1 (the first product's ring never prefetches) and nk = 3
# (D, r, G): forward and 64-row backward at their smallest; the 32-row backward with rk = 4 and a partial last chunk
ROW_SWEEP = ((64, 8, 1), (64, 200, 3))
ROW_SWEEP_M = tuple(range(1, 131))          # every last-tile row count of the 128-, 64- and 32-row workgroups, and two past
FORMS_AT = (161, 192, 72)           # (M, D, r) of the call forms: rk = 2 with a partial chunk


def _name(M, D, r, G, alpha, bias="both", form="std"):
    tail = (f"/bias-{bias}" if bias != "both" else "") + (f"/{form}" if form != "std" else "")
    return f"M{M}/D{D}/r{r}/G{G}/a{int(alpha)}" + tail


def sweep_groups():
    """{group: [Case]}: every r; every last-tile row count on the three instantiations; the widest D; the call forms that
    cases() leaves out (a NULL b1 and / or b2, y[0] beside y32, H asked of one adapter of three)"""
    out, seed = {}, [1000]

    def add(group, M, D, r, G, alpha, **kw):
        out.setdefault(group, []).append(Case(_name(M, D, r, G, alpha, **kw), M, D, r, G, float(alpha), seed[0], **kw))
        seed[0] += 1

    for G in (1, 3):
        for D in SWEEP_D:
            for r in SWEEP_R:                   # alpha alternates along r; the two widths of an (r, G) take the two values
                add(f"r/G{G}/D{D}", SWEEP_M, D, r, G, 1 + (r // 8 + (D == SWEEP_D[1])) % 2)
    for D, r, G in ROW_SWEEP:
        for M in ROW_SWEEP_M:
            add(f"rows/D{D}/r{r}/G{G}", M, D, r, G, 1)
    add("wide", 129, 8192, 256, 3, 1)
    add("wide", 129, 8192, 136, 1, 2)
    M, D, r = FORMS_AT
    for G in (1, 3):
        for k, bias in enumerate(("b1", "b2", "none")):
            add("forms", M, D, r, G, 1 + (k + G // 3) % 2, bias=bias)
    add("forms", M, D, r, 1, 2, form="y_y32")
    add("forms", M, D, r, 3, 1, form="h1")
    return out


def sweep_cases():
    return [c for group in sweep_groups().values() for c in group]


def make_inputs(c: Case) -> Dict[str, torch.Tensor]:
    """X inside a wider buffer (row stride D + 64); per adapter W1 [r, D], b1, W2 [D, r], b2; an fp32 residual; and for the
    backward one dY_g per adapter as column slabs of ONE [M, G D] buffer (the q, k, v slabs of a fused gradient)."""
    g = torch.Generator().manual_seed(c.seed)
    rn = lambda *shape, scale=1.0: torch.randn(shape, generator=g) * scale
    inp = {"X_buf": rn(c.M, c.D + 64).to(BF16), "resid": rn(c.M, c.D), "dY_buf": rn(c.M, c.G * c.D).to(BF16)}
    for i in range(c.G):
        inp[f"W1_{i}"] = rn(c.r, c.D, scale=c.D ** -0.5).to(BF16)
        inp[f"b1_{i}"] = rn(c.r, scale=0.3)
        inp[f"W2_{i}"] = rn(c.D, c.r, scale=c.r ** -0.5).to(BF16)
        inp[f"b2_{i}"] = rn(c.D, scale=0.3)
    return inp


def x_of(c: Case, inp):
    return inp["X_buf"][:, 32:32 + c.D]


def dy_of(c: Case, inp, i: int):
    return inp["dY_buf"][:, i * c.D:(i + 1) * c.D]


MUTANTS = ("alpha_other", "no_b1", "no_b2", "permuted", "h_unrounded", "dx_no_skip", "dx_one_dy", "r_tail", "d_last_step",
           "bias_ignored_null")


def mutants(c: Case):
    """r_tail: the second product leaves out the hidden units of the last, partial 64-chunk of r; d_last_step: the first
    product leaves out the last 64 columns of D; bias_ignored_null: a bias that was not passed is added all the same"""
    on = {"alpha_other": True, "no_b1": c.bias in ("both", "b1"), "no_b2": c.bias in ("both", "b2"), "permuted": c.G == 3,
          "h_unrounded": True, "dx_no_skip": True, "dx_one_dy": c.G == 3, "r_tail": c.r % 64 != 0, "d_last_step": True,
          "bias_ignored_null": c.bias != "both"}
    return [m for m in MUTANTS if on[m]]


def expected(c: Case, inp, got=None, mut: Optional[str] = None):
    """{output: (float64 value, bound)}.  Without `got` only what follows from the inputs alone (H_g, dH_g); with the kernel's
    own got["H{g}"] / got["dH{g}"] also Y_g, Y32 (G = 1) and dX.  `mut` names a deliberately wrong restatement (MUTANTS)."""
    X = x_of(c, inp).double()
    alpha = c.alpha if mut != "alpha_other" else 3.0 - c.alpha
    src = (lambda i: (i + 1) % c.G) if mut == "permuted" else (lambda i: i)       # output i computed with adapter src(i)
    with_b1 = (c.bias in ("both", "b1") or mut == "bias_ignored_null") and mut != "no_b1"
    with_b2 = (c.bias in ("both", "b2") or mut == "bias_ignored_null") and mut != "no_b2"
    Dk = c.D - 64 if mut == "d_last_step" else c.D                  # the columns of D the first product sums over
    ru = c.r // 64 * 64 if mut == "r_tail" else c.r                 # the hidden units the second product sums over
    out = {}
    for i in range(c.G):
        W1, b1 = inp[f"W1_{src(i)}"].double(), inp[f"b1_{src(i)}"].double()
        ref = X[:, :Dk] @ W1[:, :Dk].T + (b1[None, :] if with_b1 else 0)
        e = 2 * c.D * U24 * (X.abs() @ W1.abs().T)
        out[f"H{i}"] = (ref, U8 * ref.abs() + e + 2 * U24 * ref.abs())
        dY, W2 = dy_of(c, inp, i).double(), inp[f"W2_{i}"].double()
        ref = dY[:, :Dk] @ W2[:Dk]
        e = 2 * c.D * U24 * (dY.abs() @ W2.abs())
        out[f"dH{i}"] = (ref, U8 * ref.abs() + e + 2 * U24 * ref.abs())
    if got is None:
        return out
    for i in range(c.G):
        if f"H{i}" not in got:
            continue
        H = got[f"H{i}"].double() if mut != "h_unrounded" else got["_H_exact"][i]
        W2, b2 = inp[f"W2_{src(i)}"].double(), inp[f"b2_{src(i)}"].double()
        acc = H[:, :ru] @ W2[:, :ru].T
        b2v = b2 if with_b2 else torch.zeros_like(b2)
        ref = alpha * X + acc + b2v[None, :]
        e = 2 * c.r * U24 * (H.abs() @ W2.abs().T) + 4 * U24 * ((alpha * X).abs() + acc.abs() + b2v.abs()[None, :])
        out[f"Y{i}"] = (ref, U8 * ref.abs() + e)
        if c.G == 1:
            resid = inp["resid"].double()
            out["Y32"] = (resid + ref, e + 4 * U24 * (resid.abs() + ref.abs()))
    if all(f"dH{i}" in got for i in range(c.G)):
        dYs = [dy_of(c, inp, i).double() for i in range(c.G)]
        skip = dYs[0] if mut == "dx_one_dy" else sum(dYs)
        acc, eacc = 0, 0
        for i in range(c.G):
            dH, W1 = got[f"dH{i}"].double(), inp[f"W1_{i}"].double()
            acc = acc + dH[:, :ru] @ W1[:ru]
            eacc = eacc + dH.abs() @ W1.abs()
        ref = (0 if mut == "dx_no_skip" else alpha * skip) + acc
        e = 2 * c.G * c.r * U24 * eacc + (c.G + 3) * U24 * (alpha * sum(d.abs() for d in dYs) + acc.abs())
        out["dX"] = (ref, U8 * ref.abs() + e)
    return out


def compare(c: Case, inp, got) -> Dict[str, float]:
    exp = expected(c, inp, got)
    return {k: ratio(got[k], *exp[k]) for k in exp if k in got}


def simulate(c: Case, inp, mut: Optional[str] = None):
    """the outputs of a kernel that computes `expected(..., mut)` exactly and rounds once to each output's dtype"""
    first = expected(c, inp, None, mut)
    got = {k: v.to(BF16) for k, (v, _) in first.items()}
    got["_H_exact"] = [first[f"H{i}"][0] for i in range(c.G)]
    for k, (v, _) in expected(c, inp, got, mut).items():
        if k not in got:
            got[k] = v.to(F32 if k == "Y32" else BF16)
    del got["_H_exact"]
    return got


# ------------------------------------------------------------------ the kernels, every call form of one case ----------------
def run_case(ops, c: Case, dev):
    """Both kernels on `c`: X row-strided, the Y_g as column slabs of one buffer (G = 3) or row-strided (G = 1), H stored and
    not, the fp32 form with its residual (G = 1), every dY_g a slab; each call twice; the biases that c.bias names (None for
    the rest).  c.form adds one call: y_y32 writes y[0] and y32 together, h1 asks for the H of adapter 1 alone; their outputs
    must have the bits of the calls above.  Every output lies in a NaN-filled buffer with spare rows and columns.
    -> dict(checks, pad, finite, same: rerun / H-NULL / form outputs with equal bits)."""
    inp = {k: v.to(dev) for k, v in make_inputs(c).items()}
    M, D, r, G = c.M, c.D, c.r, c.G
    X = x_of(c, inp)
    w1 = [inp[f"W1_{i}"] for i in range(G)]
    w2 = [inp[f"W2_{i}"] for i in range(G)]
    b1 = [inp[f"b1_{i}"] if c.bias in ("both", "b1") else None for i in range(G)]
    b2 = [inp[f"b2_{i}"] if c.bias in ("both", "b2") else None for i in range(G)]
    w1t = [w.T.contiguous() for w in w1]
    w2t = [w.T.contiguous() for w in w2]
    rec = {"pad": {}, "finite": {}, "same": {}}

    def forward(store_h, f32_form: bool, with_y: Optional[bool] = None):
        """store_h: True, False, or the indices of the adapters whose H is asked for; with_y: y[g] passed (default: exactly
        where y32 is not)"""
        got, bufs = {}, {}
        with_y = (not f32_form) if with_y is None else with_y
        stored = [i for i in range(G) if (store_h is True or (store_h is not False and i in store_h))]
        yv, ybuf = _padded(M, G * D, BF16, dev)
        ys = [yv[:, i * D:(i + 1) * D] for i in range(G)]
        hv, hbuf = _padded(M, G * r, BF16, dev)
        hs = [hv[:, i * r:(i + 1) * r] for i in range(G)]
        kw = {}
        if f32_form:
            got["Y32"], bufs["Y32"] = _padded(M, D, F32, dev)
            kw = dict(y32=got["Y32"], resid=inp["resid"])
        ops.lowrank_fwd(X, w1, b1, w2, b2, h=[hs[i] if i in stored else None for i in range(G)] if stored else None,
                        y=ys if with_y else None, alpha=c.alpha, **kw)
        if with_y:
            for i in range(G):
                got[f"Y{i}"] = ys[i]
            bufs["Y"] = (ybuf, G * D)
        for i in stored:
            got[f"H{i}"] = hs[i]
        if len(stored) == G:
            bufs["H"] = (hbuf, G * r)
        elif stored:                            # the slabs that were not asked for must still hold their NaNs
            bufs["H"] = (hbuf, stored)
        return got, bufs

    def backward():
        got, bufs = {}, {}
        got["dX"], dxbuf = _padded(M, D, BF16, dev)
        hv, hbuf = _padded(M, G * r, BF16, dev)
        hs = [hv[:, i * r:(i + 1) * r] for i in range(G)]
        ops.lowrank_bwd([dy_of(c, inp, i) for i in range(G)], w2t, w1t, hs, got["dX"], alpha=c.alpha)
        for i in range(G):
            got[f"dH{i}"] = hs[i]
        bufs["dX"], bufs["dH"] = (dxbuf, D), (hbuf, G * r)
        return got, bufs

    def pads(tag, bufs):
        for k, b in bufs.items():
            buf, cols = b if isinstance(b, tuple) else (b, D)
            if isinstance(cols, list):          # H slabs `cols` written, the others not: NaN everywhere else
                bits = buf.view(torch.int16).clone()
                fill = torch.full((1,), float("nan"), dtype=BF16).view(torch.int16).item()
                for i in cols:
                    bits[:M, i * r:(i + 1) * r] = fill
                rec["pad"][f"{tag}:{k}"] = bool((bits == fill).all())
            else:
                rec["pad"][f"{tag}:{k}"] = _pad_intact(buf, M, cols)

    def same(a, b):
        return all(torch.equal(a[k].view(torch.int16 if a[k].dtype == BF16 else torch.int32),
                               b[k].view(torch.int16 if b[k].dtype == BF16 else torch.int32)) for k in a if k in b)

    got, bufs = forward(True, False)
    again, _ = forward(True, False)
    no_h, bufs_nh = forward(False, False)
    pads("fwd", bufs), pads("fwd_noH", bufs_nh)
    rec["same"]["fwd_rerun"] = same(got, again)
    rec["same"]["fwd_H_NULL"] = same(no_h, got) and all(f"Y{i}" in no_h for i in range(G))
    if G == 1:
        g32, b32 = forward(True, True)
        g32b, _ = forward(True, True)
        pads("fwd32", b32)
        rec["same"]["fwd32_rerun"] = same(g32, g32b)
        rec["same"]["fwd32_H"] = same({"H0": g32["H0"]}, got)
        got["Y32"] = g32["Y32"]
    if c.form == "y_y32":
        both, bboth = forward(True, True, with_y=True)
        pads("fwd_y_y32", bboth)
        rec["same"]["fwd_y_y32"] = same(both, got) and {"Y0", "Y32", "H0"} <= set(both)
    elif c.form == "h1":
        part, bpart = forward([1], False)
        pads("fwd_h1", bpart)
        rec["same"]["fwd_h1"] = same(part, got) and set(part) == {"Y0", "Y1", "Y2", "H1"}
    else:
        assert c.form == "std", c.form
    gb, bb = backward()
    gb2, _ = backward()
    pads("bwd", bb)
    rec["same"]["bwd_rerun"] = same(gb, gb2)
    got.update(gb)
    torch.cuda.synchronize()
    for k in got:
        rec["finite"][k] = bool(torch.isfinite(got[k].float()).all())
    rec["checks"] = compare(c, inp, got)
    return rec


# ------------------------------------------------------------------ what the entry points refuse -----------------------------
def refused(lib):
    """[(what, return code, message)]: argument blocks both entry points must refuse before any launch -- every pointer in
    them is a small fake address that no kernel may touch."""
    import ctypes

    from aim_amd.lib import LowrankArgs

    def block(**kw):
        a = LowrankArgs()
        for g in range(3):
            a.x[g], a.wa[g], a.wb[g], a.h[g], a.y[g], a.ba[g], a.bb[g] = (0x1000,) * 7
        a.ldx, a.ldh, a.ldy, a.M, a.D, a.r, a.G, a.alpha = 768, 192, 768, 64, 768, 192, 3, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = {"r not a multiple of 8": dict(r=100, ldh=100), "r above 256": dict(r=264, ldh=264), "r = 0": dict(r=0),
           "D not a multiple of 64": dict(D=96, ldx=96, ldy=96), "G = 2": dict(G=2), "G = 4": dict(G=4), "M = 0": dict(M=0),
           "alpha = 0.5": dict(alpha=0.5), "ldx below D": dict(ldx=512), "ldx odd": dict(ldx=771), "ldy below D": dict(ldy=760),
           "ldh below r": dict(ldh=96)}
    out = []
    for what, kw in bad.items():
        for fn in (lib.aim_lowrank_fwd, lib.aim_lowrank_bwd):
            rc = fn(ctypes.byref(block(**kw)), None)
            out.append((what, rc, lib.aim_last_error() if rc else None))
    a = block(G=3)
    a.y32, a.resid = 0x1000, 0x1000
    rc = lib.aim_lowrank_fwd(ctypes.byref(a), None)
    out.append(("fp32 form with G = 3", rc, lib.aim_last_error() if rc else None))
    a = block(G=1)
    a.x[0] = 0x1002
    rc = lib.aim_lowrank_fwd(ctypes.byref(a), None)
    out.append(("misaligned x", rc, lib.aim_last_error() if rc else None))
    a = block(G=1)
    a.h[0] = None
    rc = lib.aim_lowrank_bwd(ctypes.byref(a), None)
    out.append(("backward without dH", rc, lib.aim_last_error() if rc else None))
    return out
