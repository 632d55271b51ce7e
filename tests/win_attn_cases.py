"""Every call form of the 3-D window attention kernels (aim_win_attn_fwd / aim_win_attn_bwd, csrc/win_attn.hip), float64
closed forms of out, lse, dQ, dK, dV per window, and bounds derived from the kernels' rounding points.

A plain module in the manner of attn_cases.py: `test_win_attn_gpu.py` runs `python win_attn_cases.py OUT.json` once (one child
process for the whole list) and `test_win_attn_cases_cpu.py` proves on the CPU that the bounds accept an emulation of the
kernels' arithmetic and reject the defects they are meant to catch (MUTANTS).

Geometry.  B clips of T frames of N = G G + 1 tokens; a window of (wt, wh, ww) (each extent clipped to the grid's) holds the
S = wt wh ww patch tokens (dt, dh, dw), token i = (dt wh + dh) ww + dw, whose frame-major row is
    (b T + it wt + dt) N + 1 + (ih wh + dh) G + iw ww + dw                                    (`window_rows`)
One item = one (window, head): q, k, v [S, 64], and everything of attn_cases.py's notation with N -> S.

Bounds.  Inside a window the kernels have the rounding points of the spatial kernels (fp32 MFMA sums of 64 exact bf16
products for S and dP, exp2 in fp32, bf16 P and dS operands, fp32 accumulation over the keys / queries, one final bf16
rounding; the backward recomputes p from lse and forms delta = fp32 rowsum(dO o out) itself), so the backward bounds ARE
attn_cases.backward_ref with N -> S, and the forward bounds are attn_cases.forward_ref's expressions with one more term:

  the online rescale.  The keys arrive in nT = ceil(S / 64) tiles.  Tile t is weighted with p' = exp2((s - m_t) c) against
  the running maximum m_t (p' <= 1: the bf16 rounding of P stays RELATIVE, U8 p', whatever follows), and every later tile u
  multiplies the accumulated O and l by alpha_u = exp2((m_{u-1} - m_u) c).  In exact arithmetic the exponents telescope to
  (s - m_final) c.  In fp32 each alpha carries three roundings of numbers no larger than 2 |z|max (difference, product with
  c, v_exp_f32's ulp) and the product with O / l one more: a relative 4 u . 2 |z|max + 5 u per rescale, on at most nT - 1
  rescales.  The same floats multiply O and l, but tiles differ in how many they see, so nothing cancels in O / l:
      resc = (nT - 1) (8 u |z|max + 5 u)            is added to rp of every key (forward only)
  and flows into E, rsum and the lse bound through rp exactly as eS does.  nT = 1 gives the spatial bounds unchanged.
"""
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_cases import backward_ref, handed_in, sink_rows  # noqa: E402
from gemm_cases import U8, U24, _digest, ratio  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MAX_S = 4096                      # AIM_WIN_ATTN_MAX_S
TILE = 64                         # keys per LDS tile
# B, T, G, H, window
SHAPES = ((1, 32, 14, 2, (16, 7, 7)),     # S = 784: 12 full tiles + 16, the hmdb51 / diving48 / sthv2 form
          (2, 32, 14, 1, (32, 1, 1)),     # S = 32: 196 windows per clip, the ucf101 form
          (1, 4, 4, 2, (2, 2, 2)),        # S = 8
          (1, 8, 4, 1, (8, 4, 4)),        # S = 128: exact tiles, one window
          (1, 6, 6, 1, (3, 3, 2)))        # S = 18, unequal extents
FAMILIES = ("unit", "peaked", "neg100", "late_max")
SENTINEL = -7.0                   # exact in bf16 and fp32


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    T: int
    G: int
    H: int
    window: tuple
    family: str = "unit"
    seed: int = 0

    @property
    def N(self):
        return self.G * self.G + 1


def cases():
    out, seed = [], 5000
    for B, T, G, H, w in SHAPES:
        for fam in FAMILIES:
            out.append(Case(f"win/B{B}T{T}G{G}H{H}/{w[0]}x{w[1]}x{w[2]}/{fam}", B, T, G, H, w, fam, seed))
            seed += 1
    return out


def clip_window(window, T, G):
    """the reference's get_window_size: an extent that reaches the grid's is clipped to it"""
    return min(window[0], T), min(window[1], G), min(window[2], G)


def window_rows(B, T, G, window, swap_hw=False):
    """[B nW, S] frame-major rows of every window's tokens: the kernels' address rule (swap_hw: the h <-> w defect)"""
    wt, wh, ww = clip_window(window, T, G)
    assert T % wt == 0 and G % wh == 0 and G % ww == 0
    N = G * G + 1
    b, it, ih, iw, dt, dh, dw = torch.meshgrid(torch.arange(B), torch.arange(T // wt), torch.arange(G // wh), torch.arange(G // ww),
                                               torch.arange(wt), torch.arange(wh), torch.arange(ww), indexing="ij")
    hh, wc = ih * wh + dh, iw * ww + dw
    if swap_hw:
        hh, wc = wc, hh
    rows = (b * T + it * wt + dt) * N + 1 + hh * G + wc
    return rows.reshape(-1, wt * wh * ww)


# ------------------------------------------------------------------ inputs (CPU, fixed seeds) ------------------------------
def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    """qkv [B T N, 3 D] and dO [B T N, D] as bf16, frame-major.  The families shape the logits INSIDE each window; the class
    rows hold unit noise (the kernels never read them)."""
    g = torch.Generator().manual_seed(case.seed)
    B, T, G, H, N, fam = case.B, case.T, case.G, case.H, case.N, case.family
    idx = window_rows(B, T, G, case.window)
    nWt, S = idx.shape
    q, k, v, do = (torch.randn((nWt, S, H, 64), generator=g) for _ in range(4))
    if fam == "peaked":
        q, k = q * 2.5, k * 2.5
    elif fam == "neg100":               # attn_cases: every logit of the chosen query rows ~ -104
        k = 0.1 * k + 1.0
        q = 0.5 * q
        rows = sink_rows(S)
        q[:, rows] = q[:, rows] - 13.0
    elif fam == "late_max":             # the row maximum sits at the window's LAST key, in the last tile (its tail when S % 64)
        q = 0.5 * q + 1.0
        k = 0.5 * k
        k[:, S - 1] = 2.0
    D, M = H * 64, B * T * N
    full = [torch.randn((M, H, 64), generator=g) for _ in range(4)]
    for f, w in zip(full, (q, k, v, do)):
        f[idx.reshape(-1)] = w.reshape(nWt * S, H, 64)
    qkv = torch.cat([t.reshape(M, D) for t in full[:3]], dim=1).to(BF16)
    return {"qkv": qkv, "do": full[3].reshape(M, D).to(BF16)}


def gather(x, idx, H, parts=1):
    """[M, parts D] rows -> `parts` tensors [nW, H, S, 64] (float64) of the windows `idx`"""
    nWt, S = idx.shape
    t = x.double()[idx.reshape(-1)].reshape(nWt, S, parts, H, 64).permute(2, 0, 3, 1, 4)
    return [t[i] for i in range(parts)] if parts > 1 else t[0]


def gather_stat(x, idx, BT, H, N):
    """[BT, H, N] statistics -> [nW, H, S]"""
    nWt, S = idx.shape
    return x.double().reshape(BT, H, N).permute(0, 2, 1).reshape(BT * N, H)[idx.reshape(-1)].reshape(nWt, S, H).permute(0, 2, 1)


def scatter(t, idx, M):
    """[nW, H, S, 64] -> [M, D] rows (class rows zero)"""
    nWt, H, S, _ = t.shape
    out = torch.zeros((M, H * 64), dtype=t.dtype)
    out[idx.reshape(-1)] = t.permute(0, 2, 1, 3).reshape(nWt * S, H * 64)
    return out


# ------------------------------------------------------------------ float64 references and bounds --------------------------
def forward_ref(q, k, v):
    """attn_cases.forward_ref with N -> S and the online-rescale term (module docstring) -> dict name: (ref, bound), parts"""
    S = q.shape[-2]
    nT = (S + TILE - 1) // TILE
    z = q @ k.transpose(-1, -2) / 8.0
    eS = 2 * 64 * U24 * (q.abs() @ k.abs().transpose(-1, -2))
    lse = torch.logsumexp(z, dim=-1)
    p = torch.exp(z - lse[..., None])
    O = p @ v
    zmax = z.abs().amax(dim=-1, keepdim=True)
    resc = (nT - 1) * (8 * U24 * zmax + 5 * U24)
    rp = eS / 8 + 4 * U24 * (z.abs() + zmax) + 4 * U24 + resc
    A = p @ v.abs()
    wrp = (p * rp).sum(dim=-1)
    rsum = (S / 4 + 16) * U24 + wrp
    E = (p * rp) @ v.abs() + 2 * S * U24 * A + rsum[..., None] * O.abs()
    b_out = U8 * A + E + U8 * (O.abs() + U8 * A + E)
    b_lse = wrp + (S / 4 + 16) * U24 + 32 * U24 + 4 * U24 * (lse.abs() + zmax[..., 0])
    return {"out": (O, b_out), "lse": (lse, b_lse), "_z": z, "_p": p, "_eS": eS}


def expected(case: Case, inp, idx=None):
    """-> (forward dict, backward dict of form a, backward dict of form b) over the windows [nW, H, S, ...]"""
    idx = window_rows(case.B, case.T, case.G, case.window) if idx is None else idx
    q, k, v = gather(inp["qkv"], idx, case.H, 3)
    do = gather(inp["do"], idx, case.H)
    fw = forward_ref(q, k, v)
    _, _, eo, el = handed_in(fw)
    return fw, backward_ref(q, k, v, do, fw, eo, el), backward_ref(q, k, v, do, fw, fw["out"][1], fw["lse"][1])


MUTANTS = ("swap_hw", "wt1", "tail_unmasked", "no_sum_rescale", "lse_last_tile")


def emulate(case: Case, inp, mut: Optional[str] = None, own: bool = False):
    """The kernels' arithmetic restated in float64 with their rounding points inserted (fp32 scores, running maximum, alpha,
    probabilities and sums; bf16 P and dS; one final rounding); `mut` inserts one defect.  own: the backward takes the
    emulated forward's out and lse (form b).  -> frame-major tensors as the kernels write them (class rows: SENTINEL)."""
    B, T, G, H, N = case.B, case.T, case.G, case.H, case.N
    M, BT = B * T * N, B * T
    window = (1,) + tuple(case.window[1:]) if mut == "wt1" else case.window
    idx = window_rows(B, T, G, window, swap_hw=mut == "swap_hw")
    nWt, S = idx.shape
    q, k, v = gather(inp["qkv"], idx, H, 3)
    do = gather(inp["do"], idx, H)
    r32 = lambda t: t.to(F32).double()
    r16 = lambda t: t.to(F32).to(BF16).double()
    z = r32(q @ k.transpose(-1, -2)) / 8
    m = torch.full((nWt, H, S, 1), -math.inf, dtype=F64)
    l = torch.zeros((nWt, H, S, 1), dtype=F64)
    O = torch.zeros((nWt, H, S, 64), dtype=F64)
    nT = (S + TILE - 1) // TILE
    for t in range(nT):
        lo, hi = t * TILE, min(S, (t + 1) * TILE)
        zt, vt = z[..., lo:hi], v[..., lo:hi, :]
        if mut == "tail_unmasked" and hi - lo < TILE:        # zero-filled keys past S take part: logit 0, value 0
            pad = TILE - (hi - lo)
            zt = torch.cat([zt, torch.zeros((nWt, H, S, pad), dtype=F64)], dim=-1)
            vt = torch.cat([vt, torch.zeros((nWt, H, pad, 64), dtype=F64)], dim=-2)
        mn = torch.maximum(m, zt.amax(dim=-1, keepdim=True))
        alpha = r32(torch.exp(m - mn))
        pu = r32(torch.exp(zt - mn))
        tile_sum = r32(pu.sum(dim=-1, keepdim=True))
        if mut == "lse_last_tile":
            l_last = tile_sum
        l = r32(l + tile_sum) if mut == "no_sum_rescale" else r32(r32(l * alpha) + tile_sum)
        O = r32(r32(O * alpha) + r16(pu) @ vt)
        m = mn
    lse = r32(m + torch.log(l_last if mut == "lse_last_tile" else l))[..., 0]
    o32 = r32(O / l)
    out_w, lse_w = o32.to(BF16), lse.to(F32)
    if own:
        out_in, lse_in = out_w.double(), lse_w.double()
    else:
        fw = forward_ref(q, k, v)
        o_, l_, _, _ = handed_in(fw)
        out_in, lse_in = o_.double(), l_.double()
    delta = r32((do * out_in).sum(dim=-1, keepdim=True))
    pb = r32(torch.exp(z - lse_in[..., None]))
    dP = r32(do @ v.transpose(-1, -2))
    dsb = r16(pb * (dP - delta))
    dq = r32(dsb @ k) / 8
    dk = r32(dsb.transpose(-1, -2) @ q) / 8
    dv = r32(r16(pb).transpose(-1, -2) @ do)
    got = {"out": scatter(out_w, idx, M),
           "dqkv": torch.cat([scatter(t.to(BF16), idx, M) for t in (dq, dk, dv)], dim=1)}
    ls = torch.zeros((BT * N, H), dtype=F32)
    ls[idx.reshape(-1)] = lse_w.permute(0, 2, 1).reshape(nWt * S, H)
    got["lse"] = ls.reshape(BT, N, H).permute(0, 2, 1).contiguous()
    return got


def compare(case: Case, inp, got, form: str = "a") -> Dict[str, float]:
    """worst error / bound of out, lse, dq, dk, dv given frame-major results (the TRUE windows are read back out of them)"""
    idx = window_rows(case.B, case.T, case.G, case.window)
    fw, bw_a, bw_b = expected(case, inp, idx)
    bw = bw_a if form == "a" else bw_b
    res = {}
    if "out" in got:
        res["out"] = ratio(gather(got["out"], idx, case.H), *fw["out"])
    if "lse" in got:
        res["lse"] = ratio(gather_stat(got["lse"], idx, case.B * case.T, case.H, case.N), *fw["lse"])
    if "dqkv" in got:
        d = gather(got["dqkv"], idx, case.H, 3)
        for i, name in enumerate(("dq", "dk", "dv")):
            res[name] = ratio(d[i], *bw[name])
    return res


def class_rows(t, BT, N):
    """the class rows of a frame-major [BT N, C] tensor / the class column of a [BT, H, N] statistic"""
    return t.reshape(BT, N, -1)[:, 0] if t.dim() == 2 else t[..., 0]


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Runner:
    def __init__(self, ops, dev):
        self.ops, self.dev = ops, dev

    def launch(self, case: Case, qkv, do, out_in=None, lse_in=None):
        """forward, then the backward on (out_in, lse_in) or on the forward's own results; every result buffer is pre-filled
        with SENTINEL and followed by 64 spare elements"""
        ops, dev = self.ops, self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        M, D, BT = B * T * N, case.H * 64, B * T
        got, bufs = {}, {}

        def new(name, shape, dtype):
            n = math.prod(shape)
            buf = torch.full((n + 64,), SENTINEL, dtype=dtype, device=dev)
            got[name], bufs[name] = buf[:n].view(shape), buf
            return got[name]

        out, lse = new("out", (M, D), BF16), new("lse", (BT, H, N), F32)
        ops.win_attn_fwd(qkv, out, lse, B, T, N, H, case.window)
        dqkv, delta = new("dqkv", (M, 3 * D), BF16), new("delta", (BT, H, N), F32)
        ops.win_attn_bwd(qkv, out if out_in is None else out_in, do, lse if lse_in is None else lse_in, delta, dqkv, B, T, N, H,
                         case.window)
        return got, bufs

    def handed(self, case: Case, inp, idx):
        """form (a): bf16 of the float64 out and fp32 of the float64 lse, frame-major (class rows: SENTINEL)"""
        B, T, H, N = case.B, case.T, case.H, case.N
        q, k, v = gather(inp["qkv"], idx, H, 3)
        fw = forward_ref(q, k, v)
        o_a, l_a, _, _ = handed_in(fw)
        out = scatter(o_a, idx, B * T * N)
        ls = torch.full((B * T * N, H), SENTINEL, dtype=F32)
        ls[idx.reshape(-1)] = l_a.permute(0, 2, 1).reshape(-1, H)
        return out, ls.reshape(B * T, N, H).permute(0, 2, 1).contiguous()

    def run_case(self, case: Case):
        dev = self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        BT = B * T
        inp = make_inputs(case)
        idx = window_rows(B, T, case.G, case.window)
        out_a, lse_a = self.handed(case, inp, idx)
        qkv, do = inp["qkv"].to(dev), inp["do"].to(dev)
        got_b, bufs = self.launch(case, qkv, do)
        got_a, _ = self.launch(case, qkv, do, out_a.to(dev), lse_a.to(dev))
        again, _ = self.launch(case, qkv, do)
        torch.cuda.synchronize()
        rec = {"checks": {}, "repeat": {}, "class_intact": {}, "spare_intact": {}, "finite": {}, "hash": {}}
        for name, t in got_b.items():
            rec["repeat"][name] = bool(torch.equal(_bits(t), _bits(again[name])))
            rec["class_intact"][name] = bool((class_rows(t, BT, N) == SENTINEL).all())
            n = t.numel()
            rec["spare_intact"][name] = bool((bufs[name][n:] == SENTINEL).all())
            rec["hash"][name] = _digest(_bits(t))
            patch = t.reshape(BT, N, -1)[:, 1:] if t.dim() == 2 else t[..., 1:]
            rec["finite"][name] = bool(torch.isfinite(patch.float()).all())
        host_b = {k_: t.cpu() for k_, t in got_b.items()}
        host_a = {k_: t.cpu() for k_, t in got_a.items()}
        for k_, r in compare(case, inp, host_b, "b").items():
            rec["checks"][f"{k_}@b" if k_[0] == "d" else k_] = r
        for k_, r in compare(case, inp, {"dqkv": host_a["dqkv"]}, "a").items():
            rec["checks"][f"{k_}@a"] = r
        # delta is the fp32 row sum of dO o out of the rows it was given
        dl = (do.double().reshape(BT, N, H, 64) * got_b["out"].double().reshape(BT, N, H, 64)).sum(-1).permute(0, 2, 1)[..., 1:]
        mag = (do.double().reshape(BT, N, H, 64) * got_b["out"].double().reshape(BT, N, H, 64)).abs().sum(-1).permute(0, 2, 1)[..., 1:]
        rec["checks"]["delta"] = ratio(got_b["delta"][..., 1:].cpu(), dl.cpu(), (66 * U24 * mag).cpu())
        return rec

    def run_poison(self, case: Case):
        """window 1's rows of qkv and dO hold NaN: every other window's results are the bits of a clean run, and finite.  The
        class rows of qkv hold NaN in BOTH runs."""
        dev = self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        BT, D = B * T, H * 64
        inp = make_inputs(case)
        idx = window_rows(B, T, case.G, case.window)
        cls = torch.arange(BT) * N
        qkv, do = inp["qkv"].clone(), inp["do"].clone()
        qkv[cls] = float("nan")
        bad_q, bad_do = qkv.clone(), do.clone()
        bad_q[idx[1]] = float("nan")
        bad_do[idx[1]] = float("nan")
        clean, _ = self.launch(case, qkv.to(dev), do.to(dev))
        bad, _ = self.launch(case, bad_q.to(dev), bad_do.to(dev))
        torch.cuda.synchronize()
        others = torch.cat([idx[:1].reshape(-1), idx[2:].reshape(-1)]).to(dev)
        same, finite = True, True
        for name in ("out", "dqkv"):
            same &= bool(torch.equal(_bits(clean[name][others]), _bits(bad[name][others])))
            finite &= bool(torch.isfinite(clean[name][others].float()).all())
        for name in ("lse", "delta"):
            f = lambda t: t.permute(0, 2, 1).reshape(BT * N, H)[others]
            same &= bool(torch.equal(_bits(f(clean[name]).contiguous()), _bits(f(bad[name]).contiguous())))
            finite &= bool(torch.isfinite(f(clean[name])).all())
        poisoned = bool(torch.isnan(bad["out"][idx[1].to(dev)].float()).all())
        return {"independent": same, "finite_with_nan_class_rows": finite, "poisoned_window_is_nan": poisoned}

    def run_stride(self, case: Case, spare: int = 3):
        """the same data stored P = N + spare token rows per frame (NaN in the spare rows of the inputs, SENTINEL in those
        of the results): the bits of the N-row launch in every token row, the spare rows untouched"""
        ops, dev = self.ops, self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        BT, D, P = B * T, H * 64, case.N + spare
        inp = make_inputs(case)
        base, _ = self.launch(case, inp["qkv"].to(dev), inp["do"].to(dev))

        def wide(t, fill):
            w = torch.full((BT, P, t.shape[-1]), fill, dtype=t.dtype)
            w[:, :N] = t.reshape(BT, N, -1)
            return w.reshape(BT * P, -1).to(dev)

        qkv, do = wide(inp["qkv"], float("nan")), wide(inp["do"], float("nan"))
        out = torch.full((BT * P, D), SENTINEL, dtype=BF16, device=dev)
        dqkv = torch.full((BT * P, 3 * D), SENTINEL, dtype=BF16, device=dev)
        lse, delta = (torch.full((BT, H, P), SENTINEL, dtype=F32, device=dev) for _ in range(2))
        ops.win_attn_fwd(qkv, out, lse, B, T, N, H, case.window, P=P)
        ops.win_attn_bwd(qkv, out, do, lse, delta, dqkv, B, T, N, H, case.window, P=P)
        torch.cuda.synchronize()
        same, spare_ok = True, True
        for name, t in (("out", out), ("dqkv", dqkv)):
            v = t.reshape(BT, P, -1)
            same &= bool(torch.equal(_bits(v[:, :N].contiguous()), _bits(base[name].reshape(BT, N, -1).contiguous())))
            spare_ok &= bool((v[:, N:] == SENTINEL).all())
        for name, t in (("lse", lse), ("delta", delta)):
            same &= bool(torch.equal(_bits(t[..., :N].contiguous()), _bits(base[name].contiguous())))
            spare_ok &= bool((t[..., N:] == SENTINEL).all())
        return {"identical": same, "spare_rows_intact": spare_ok}

    def refusals(self):
        """S over the cap, extents that do not divide, a non-square N - 1: an error through aim_last_error and nothing
        written (the buffers are far too small for these shapes: a launch would be out of bounds)"""
        dev, ops, out = self.dev, self.ops, {}
        shapes = {"S over the cap": (1, 17, 257, 1, (17, 16, 16)),          # S = 4352
                  "wt does not divide": (1, 6, 17, 1, (4, 2, 2)),
                  "wh does not divide": (1, 4, 17, 1, (2, 3, 2)),
                  "N - 1 not a square": (1, 4, 18, 1, (2, 2, 2))}
        for name, (B, T, N, H, w) in shapes.items():
            t16 = torch.full((256,), SENTINEL, dtype=BF16, device=dev)
            o16, d16 = t16.clone(), t16.clone()
            l32, e32 = (torch.full((256,), SENTINEL, dtype=F32, device=dev) for _ in range(2))
            msgs = []
            for f in (lambda: ops.win_attn_fwd(t16, o16, l32, B, T, N, H, w),
                      lambda: ops.win_attn_bwd(t16, t16, t16, l32, e32, d16, B, T, N, H, w)):
                try:
                    f()
                    msgs.append(None)
                except RuntimeError as e:
                    msgs.append(str(e))
            torch.cuda.synchronize()
            intact = all(bool((t == SENTINEL).all()) for t in (o16, d16, l32, e32))
            out[name] = {"fwd": msgs[0], "bwd": msgs[1], "nothing_written": intact}
        return out


def main(argv):
    (path,) = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    dev = torch.device("cuda")
    run = Runner(ops, dev)
    res = {"cases": {}, "poison": {}, "stride": {}}
    with torch.no_grad():
        res["refusals"] = run.refusals()
        for case in cases():
            res["cases"][case.name] = run.run_case(case)
        for case in cases():
            if case.family == "unit" and window_rows(case.B, case.T, case.G, case.window).shape[0] >= 3:
                res["poison"][case.name] = run.run_poison(case)
            if case.family == "unit":
                res["stride"][case.name] = run.run_stride(case)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
