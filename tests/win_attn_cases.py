"""Every call form of the 3-D window attention kernels (aim_win_attn_fwd / aim_win_attn_bwd, csrc/win_attn.hip), float64
closed forms of out, lse, dQ, dK, dV per window, and bounds derived from the kernels' rounding points.

A plain module in the manner of attn_cases.py: `test_win_attn_gpu.py` runs `python win_attn_cases.py OUT.json` once (one child
process for the whole list) and `test_win_attn_cases_cpu.py` proves on the CPU that the bounds accept an emulation of the
kernels' arithmetic and reject the defects they are meant to catch (MUTANTS).

This module also holds what the three tables of win_attn.hip share (win_attn_shift_cases.py and win_attn_cut_cases.py are the
other two).  Every shared function is handed the sequences it works on: an [n, S] index of frame-major rows, or a list of
`groups` (idx, forward dict, backward dict of form a, of form b), one per index.  This table has one group, the windows of
`window_rows`; the other two have one group per size of box.  `Runner` launches any of the three entry pairs.

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
NAN = float("nan")


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
def background(g, M, H):
    """unit noise for q, k, v, dO of all M rows; the class rows keep it (the kernels never read them)"""
    return [torch.randn((M, H, 64), generator=g) for _ in range(4)]


def draw_group(g, idx, H, fam):
    """q, k, v, dO [n, S, H, 64] of the sequences `idx`; the families shape the logits INSIDE each sequence (its own S: the
    sink rows and the late maximum sit where its tile loop ends)"""
    n, S = idx.shape
    q, k, v, do = (torch.randn((n, S, H, 64), generator=g) for _ in range(4))
    if fam == "peaked":
        q, k = q * 2.5, k * 2.5
    elif fam == "neg100":               # attn_cases: every logit of the chosen query rows ~ -104
        k = 0.1 * k + 1.0
        q = 0.5 * q
        rows = sink_rows(S)
        q[:, rows] = q[:, rows] - 13.0
    elif fam == "late_max":             # the row maximum sits at the sequence's LAST key, in the last tile (its tail when S % 64)
        q = 0.5 * q + 1.0
        k = 0.5 * k
        k[:, S - 1] = 2.0
    return idx, (q, k, v, do)


def assemble(full, drawn, H):
    """the drawn groups written over the background -> qkv [M, 3 D] and dO [M, D] as bf16, frame-major"""
    for idx, group in drawn:
        for f, w in zip(full, group):
            f[idx.reshape(-1)] = w.reshape(idx.numel(), H, 64)
    M, D = full[0].shape[0], H * 64
    qkv = torch.cat([t.reshape(M, D) for t in full[:3]], dim=1).to(BF16)
    return {"qkv": qkv, "do": full[3].reshape(M, D).to(BF16)}


def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(case.seed)
    # the windows are drawn BEFORE the background and the box tables draw it first: merged, one of them would change its bits
    drawn = draw_group(g, window_rows(case.B, case.T, case.G, case.window), case.H, case.family)
    return assemble(background(g, case.B * case.T * case.N, case.H), [drawn], case.H)


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


def scatter_stat(groups, BT, N, H, fill=0.0):
    """(idx, [nW, H, S] fp32) pairs -> one [BT, H, N] statistic (untouched columns: `fill`)"""
    ls = torch.full((BT * N, H), fill, dtype=F32)
    for idx, t in groups:
        ls[idx.reshape(-1)] = t.permute(0, 2, 1).reshape(-1, H)
    return ls.reshape(BT, N, H).permute(0, 2, 1).contiguous()


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


def expected(case, inp, idx=None):
    """-> (forward dict, backward dict of form a, backward dict of form b) over the sequences `idx` [nW, H, S, ...] (default:
    this table's windows)"""
    idx = window_rows(case.B, case.T, case.G, case.window) if idx is None else idx
    q, k, v = gather(inp["qkv"], idx, case.H, 3)
    do = gather(inp["do"], idx, case.H)
    fw = forward_ref(q, k, v)
    _, _, eo, el = handed_in(fw)
    return fw, backward_ref(q, k, v, do, fw, eo, el), backward_ref(q, k, v, do, fw, fw["out"][1], fw["lse"][1])


def expected_groups(case: Case, inp):
    """-> [(idx, forward dict, backward dict of form a, backward dict of form b)]: this table's one group, the true windows"""
    idx = window_rows(case.B, case.T, case.G, case.window)
    return [(idx,) + tuple(expected(case, inp, idx))]


ARITHMETIC = ("tail_unmasked", "no_sum_rescale", "lse_last_tile")        # defects of emulate_rows
MUTANTS = ("swap_hw", "wt1") + ARITHMETIC                                 # the first two: defects of the index


def emulate_rows(idx, inp, BT, N, H, mut: Optional[str] = None, own: bool = False):
    """The kernels' arithmetic on the sequences `idx` [n, S], restated in float64 with their rounding points inserted (fp32
    scores, running maximum, alpha, probabilities and sums; bf16 P and dS; one final rounding); `mut` inserts one defect of
    ARITHMETIC.  own: the backward takes the emulated forward's out and lse (form b).  -> frame-major tensors as the kernels
    write them, zero in every row outside `idx`."""
    M = BT * N
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
    return {"out": scatter(out_w, idx, M),
            "dqkv": torch.cat([scatter(t.to(BF16), idx, M) for t in (dq, dk, dv)], dim=1),
            "lse": scatter_stat([(idx, lse_w)], BT, N, H)}


def emulate(case: Case, inp, mut: Optional[str] = None, own: bool = False):
    """emulate_rows on the windows: the true ones, or those of a defect of the index (`swap_hw`, `wt1`)"""
    window = (1,) + tuple(case.window[1:]) if mut == "wt1" else case.window
    idx = window_rows(case.B, case.T, case.G, window, swap_hw=mut == "swap_hw")
    return emulate_rows(idx, inp, case.B * case.T, case.N, case.H, mut if mut in ARITHMETIC else None, own)


def compare(case, inp, got, form: str = "a", groups=None) -> Dict[str, float]:
    """worst error / bound of out, lse, dq, dk, dv over `groups` (default: expected_groups, the true windows), given
    frame-major results: the true sequences are read back out of them"""
    res: Dict[str, float] = {}
    worst = lambda name, r: res.__setitem__(name, max(res.get(name, 0.0), r))      # ratio: never NaN (non-finite -> inf)
    for idx, fw, bw_a, bw_b in (expected_groups(case, inp) if groups is None else groups):
        bw = bw_a if form == "a" else bw_b
        if "out" in got:
            worst("out", ratio(gather(got["out"], idx, case.H), *fw["out"]))
        if "lse" in got:
            worst("lse", ratio(gather_stat(got["lse"], idx, case.B * case.T, case.H, case.N), *fw["lse"]))
        if "dqkv" in got:
            d = gather(got["dqkv"], idx, case.H, 3)
            for i, name in enumerate(("dq", "dk", "dv")):
                worst(name, ratio(d[i], *bw[name]))
    return res


def class_rows(t, BT, N):
    """the class rows of a frame-major [BT N, C] tensor / the class column of a [BT, H, N] statistic"""
    return t.reshape(BT, N, -1)[:, 0] if t.dim() == 2 else t[..., 0]


def patch_rows(t, BT, N):
    """the patch rows of a frame-major [BT N, C] tensor / the patch columns of a [BT, H, N] statistic"""
    return t.reshape(BT, N, -1)[:, 1:] if t.dim() == 2 else t[..., 1:]


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def holds(t, fill):
    """is every element of t still the value its buffer was filled with (SENTINEL or NaN)"""
    return bool((torch.isnan(t.float()) if fill != fill else t == fill).all())


def wide(t, BT, N, P, fill=NAN):
    """frame-major rows [BT N, C] (or a [BT, H, N] statistic) stored P >= N token rows per frame, `fill` in the spare rows"""
    if t.dim() == 3:
        w = torch.full(tuple(t.shape[:2]) + (P,), fill, dtype=t.dtype)
        w[..., :N] = t
        return w
    w = torch.full((BT, P, t.shape[-1]), fill, dtype=t.dtype)
    w[:, :N] = t.reshape(BT, N, -1)
    return w.reshape(BT * P, -1)


def narrow(got, BT, N, P):
    """the N token rows of every frame of results stored P rows per frame"""
    return {name: (t.reshape(BT, P, -1)[:, :N].reshape(BT * N, -1) if t.dim() == 2 else t[..., :N]).contiguous()
            for name, t in got.items()}


def untouched(got, bufs, BT, N, P, fill):
    """do the class rows, the spare rows of every frame and the elements behind each buffer still hold `fill`"""
    ok = True
    for name, t in got.items():
        v = t.reshape(BT, P, -1) if t.dim() == 2 else t.permute(0, 2, 1)          # [BT, P, C]
        ok &= holds(v[:, 0], fill) and holds(v[:, N:], fill) and holds(bufs[name][t.numel():], fill)
    return ok


def delta_ratio(do, out, delta, BT, N, H):
    """delta is the fp32 row sum of dO o out of the rows it was given: worst error / (66 u sum |dO o out|) over the patch rows"""
    prod = do.double().reshape(BT, N, H, 64) * out.double().reshape(BT, N, H, 64)
    dl, mag = prod.sum(-1).permute(0, 2, 1)[..., 1:], prod.abs().sum(-1).permute(0, 2, 1)[..., 1:]
    return ratio(delta[..., 1:].cpu(), dl.cpu(), (66 * U24 * mag).cpu())


ENTRIES = {"plain": ("win_attn_fwd", "win_attn_bwd"),                 # no shift argument
           "shift": ("win_attn_fwd_shift", "win_attn_bwd_shift"),
           "cut": ("win_attn_fwd_cut", "win_attn_bwd_cut")}


class Runner:
    """the launches and checks the three tables share; a table's runner names its own entry pair and the value its result
    buffers are pre-filled with, and adds the runs only that table has"""
    entry, fill = "plain", SENTINEL

    def __init__(self, ops, dev):
        self.ops, self.dev = ops, dev

    def launch(self, case, qkv, do, out_in=None, lse_in=None, *, entry=None, shift=None, P=None, fill=None):
        """forward, then the backward on (out_in, lse_in) or on the forward's own results, through the pair ENTRIES[entry]
        with `shift` (default: the case's) on buffers of P (default N) token rows per frame; every result buffer is pre-filled
        with `fill` and followed by 64 spare elements"""
        dev = self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        entry, fill, P = entry or self.entry, self.fill if fill is None else fill, N if P is None else P
        M, D, BT = B * T * P, H * 64, B * T
        fwd, bwd = (getattr(self.ops, name) for name in ENTRIES[entry])
        geom = (B, T, N, H, case.window) + (() if entry == "plain" else (case.shift if shift is None else shift,))
        got, bufs = {}, {}

        def new(name, shape, dtype):
            n = math.prod(shape)
            buf = torch.full((n + 64,), fill, dtype=dtype, device=dev)
            got[name], bufs[name] = buf[:n].view(shape), buf
            return got[name]

        out, lse = new("out", (M, D), BF16), new("lse", (BT, H, P), F32)
        dqkv, delta = new("dqkv", (M, 3 * D), BF16), new("delta", (BT, H, P), F32)
        fwd(qkv, out, lse, *geom, P=P)
        bwd(qkv, out if out_in is None else out_in, do, lse if lse_in is None else lse_in, delta, dqkv, *geom, P=P)
        return got, bufs

    def handed(self, case, groups):
        """form (a): bf16 of the float64 out and fp32 of the float64 lse, frame-major (class rows: out 0, lse SENTINEL)"""
        B, T, H, N = case.B, case.T, case.H, case.N
        out, stats = torch.zeros((B * T * N, H * 64), dtype=BF16), []
        for idx, fw, _, _ in groups:
            o_a, l_a, _, _ = handed_in(fw)
            out += scatter(o_a, idx, B * T * N)            # disjoint rows, zeros elsewhere
            stats.append((idx, l_a))
        return out, scatter_stat(stats, B * T, N, H, SENTINEL)

    def run_case(self, case, inp, groups):
        """forward and both backward forms against the fp64 bounds of `groups`; a second run has the same bits; class rows and
        the elements behind each buffer keep their SENTINEL"""
        dev = self.dev
        BT, H, N = case.B * case.T, case.H, case.N
        out_a, lse_a = self.handed(case, groups)
        qkv, do = inp["qkv"].to(dev), inp["do"].to(dev)
        got_b, bufs = self.launch(case, qkv, do)
        got_a, _ = self.launch(case, qkv, do, out_a.to(dev), lse_a.to(dev))
        again, _ = self.launch(case, qkv, do)
        torch.cuda.synchronize()
        rec = {"checks": {}, "repeat": {}, "class_intact": {}, "spare_intact": {}, "finite": {}, "hash": {}}
        for name, t in got_b.items():
            rec["repeat"][name] = bool(torch.equal(_bits(t), _bits(again[name])))
            rec["class_intact"][name] = holds(class_rows(t, BT, N), SENTINEL)
            rec["spare_intact"][name] = holds(bufs[name][t.numel():], SENTINEL)
            rec["hash"][name] = _digest(_bits(t))
            rec["finite"][name] = bool(torch.isfinite(patch_rows(t, BT, N).float()).all())
        host_b = {k_: t.cpu() for k_, t in got_b.items()}
        for k_, r in compare(case, inp, host_b, "b", groups).items():
            rec["checks"][f"{k_}@b" if k_[0] == "d" else k_] = r
        for k_, r in compare(case, inp, {"dqkv": got_a["dqkv"].cpu()}, "a", groups).items():
            rec["checks"][f"{k_}@a"] = r
        rec["checks"]["delta"] = delta_ratio(do, got_b["out"], got_b["delta"], BT, N, H)
        return rec

    def _same_rows(self, clean, bad, rows, BT, N, H):
        """are the rows `rows` of every result of two launches the same bits, and finite in the first"""
        same, finite = True, True
        for name in ("out", "dqkv"):
            same &= bool(torch.equal(_bits(clean[name][rows]), _bits(bad[name][rows])))
            finite &= bool(torch.isfinite(clean[name][rows].float()).all())
        for name in ("lse", "delta"):
            f = lambda t: t.permute(0, 2, 1).reshape(BT * N, H)[rows].contiguous()
            same &= bool(torch.equal(_bits(f(clean[name])), _bits(f(bad[name]))))
            finite &= bool(torch.isfinite(f(clean[name])).all())
        return same, finite

    def run_poison(self, case, inp):
        """window 1's rows of qkv and dO hold NaN: every other window's results are the bits of a clean run, and finite.  The
        class rows of qkv hold NaN in BOTH runs."""
        dev = self.dev
        BT, H, N = case.B * case.T, case.H, case.N
        idx = window_rows(case.B, case.T, case.G, case.window)
        qkv, do = inp["qkv"].clone(), inp["do"].clone()
        qkv[torch.arange(BT) * N] = NAN
        bad_q, bad_do = qkv.clone(), do.clone()
        bad_q[idx[1]] = NAN
        bad_do[idx[1]] = NAN
        clean, _ = self.launch(case, qkv.to(dev), do.to(dev))
        bad, _ = self.launch(case, bad_q.to(dev), bad_do.to(dev))
        torch.cuda.synchronize()
        others = torch.cat([idx[:1].reshape(-1), idx[2:].reshape(-1)]).to(dev)
        same, finite = self._same_rows(clean, bad, others, BT, N, H)
        poisoned = bool(torch.isnan(bad["out"][idx[1].to(dev)].float()).all())
        return {"independent": same, "finite_with_nan_class_rows": finite, "poisoned_window_is_nan": poisoned}

    def run_stride(self, case, inp, spare: int = 3):
        """the same data stored P = N + spare token rows per frame (NaN in the spare rows of the inputs, SENTINEL in those
        of the results): the bits of the N-row launch in every token row; the spare rows, the class rows and the 64 elements
        behind each buffer untouched"""
        dev = self.dev
        BT, N, P = case.B * case.T, case.N, case.N + spare
        base, _ = self.launch(case, inp["qkv"].to(dev), inp["do"].to(dev))
        got, bufs = self.launch(case, wide(inp["qkv"], BT, N, P).to(dev), wide(inp["do"], BT, N, P).to(dev), P=P)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(_bits(t), _bits(base[name]))) for name, t in narrow(got, BT, N, P).items())
        return {"identical": same, "spare_rows_intact": untouched(got, bufs, BT, N, P, SENTINEL)}

    def refusals(self, shapes):
        """every geometry of `shapes` (name: B, T, N, H, window[, shift]) through this runner's entry pair: an error through
        aim_last_error and nothing written (the buffers are far too small for these shapes: a launch would be out of bounds)"""
        dev, out = self.dev, {}
        fwd, bwd = (getattr(self.ops, name) for name in ENTRIES[self.entry])
        for name, geom in shapes.items():
            t16 = torch.full((256,), self.fill, dtype=BF16, device=dev)
            o16, d16 = t16.clone(), t16.clone()
            l32, e32 = (torch.full((256,), self.fill, dtype=F32, device=dev) for _ in range(2))
            msgs = []
            for f in (lambda: fwd(t16, o16, l32, *geom), lambda: bwd(t16, t16, t16, l32, e32, d16, *geom)):
                try:
                    f()
                    msgs.append(None)
                except RuntimeError as e:
                    msgs.append(str(e))
            torch.cuda.synchronize()
            intact = all(holds(t, self.fill) for t in (o16, d16, l32, e32))
            out[name] = {"fwd": msgs[0], "bwd": msgs[1], "nothing_written": intact}
        return out


# S over the cap, extents that do not divide, a non-square N - 1
REFUSAL_SHAPES = {"S over the cap": (1, 17, 257, 1, (17, 16, 16)),          # S = 4352
                  "wt does not divide": (1, 6, 17, 1, (4, 2, 2)),
                  "wh does not divide": (1, 4, 17, 1, (2, 3, 2)),
                  "N - 1 not a square": (1, 4, 18, 1, (2, 2, 2))}
REFUSALS = tuple(REFUSAL_SHAPES)


def main(argv):
    (path,) = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    run = Runner(ops, torch.device("cuda"))
    res = {"cases": {}, "poison": {}, "stride": {}}
    with torch.no_grad():
        res["refusals"] = run.refusals(REFUSAL_SHAPES)
        for case in cases():
            inp = make_inputs(case)
            res["cases"][case.name] = run.run_case(case, inp, expected_groups(case, inp))
        for case in cases():
            if case.family != "unit":
                continue
            inp = make_inputs(case)
            if window_rows(case.B, case.T, case.G, case.window).shape[0] >= 3:
                res["poison"][case.name] = run.run_poison(case, inp)
            res["stride"][case.name] = run.run_stride(case, inp)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
