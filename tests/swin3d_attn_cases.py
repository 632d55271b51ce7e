"""Every call form of the 3-D Swin attention kernels (aim_swin3d_attn_fwd / _bwd, csrc/swin3d_attn.hip), float64 closed forms
per (window, head) built from the reference's own construction, and bounds derived from the kernels' rounding points.

A plain module in the manner of swin_attn_cases.py: `test_swin3d_attn_gpu.py` runs `python swin3d_attn_cases.py OUT.json` once
(one child process for the whole list) and `test_swin3d_attn_cases_cpu.py` proves on the CPU that the bounds accept an
emulation of the kernels' arithmetic and reject the defects they are meant to catch (MUTANTS).

Geometry.  `clips` clips of a (D, G, G) token grid, rows ((b D + t) G + y) G + x.  The float64 reference does NOT use the
kernels' box rule: `rolled_geometry` restates swin_transformer.py on row numbers -- torch.roll by -shift, window_partition,
compute_mask's three slices per axis (a pair of different regions, -100 in the reference, has the weight exactly 0) -- and
`relative_position_index` is WindowAttention3D's buffer of the FULL window, sliced [:S, :S] as its forward does.  A sequence
of the reference is therefore a whole rolled window of S = wt wh ww tokens under an allow mask; the kernels' boxes are the
mask's connected pieces.

Notation and bounds are those of swin_attn_cases.py (same rounding points: bf16 q, k, v, dO; fp32 scores with the scale and
the bias log2 e folded by one fma; exp2 in fp32; bf16 p and dS as MFMA operands; fp32 everything else), with the one more
forward term of win_attn_cases.py for the online rescale over nT = ceil(S / 64) key tiles,
    resc = (nT - 1) (8 u |z|max + 5 u)     added to rp of every key (forward only),
nT taken from the window (a box has no more tiles than its window).  The backward's delta is the fp32 sum_j p_j dP_j of
swin_attn.hip, accumulated across the tiles (the (S + 2) u term covers it), and the table gradient is the fp32 sum of the
unrounded dS over boxes (walk partials), walks and the pairs of one table row: swin_attn_cases.py's dbias and dtable bounds
with nseq = the number of windows.
"""
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_attn_cases as S2  # noqa: E402
import win_attn_cases as W3  # noqa: E402
from gemm_cases import U8, U24, _digest, ratio  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HD, SCALE, LN2, SENTINEL = S2.HD, S2.SCALE, S2.LN2, S2.SENTINEL
BIAS_BIG, HOT_Q, HOT_K = S2.BIAS_BIG, S2.HOT_Q, S2.HOT_K
TILE = W3.TILE
MAX_S, TAB_CAP = 1024, 5248          # the kernels' stated capacity
gather, scatter, fold, _bits = S2.gather, S2.scatter, S2.fold, S2._bits

# clips, D, G, window, shift, heads, full window (None: the window)
SHAPES = ((2, 4, 6, (2, 3, 3), (1, 1, 1), 1, None),        # S 18, one partial tile, boxes down to a single token, two clips
          (1, 4, 14, (2, 7, 7), (1, 3, 3), 3, None),       # S 98, two key tiles with a tail of 34, three heads (Swin-T)
          (2, 6, 7, (3, 7, 7), (1, 0, 0), 2, None),        # window spans the grid, shift t only, S 147
          (1, 8, 14, (4, 7, 7), (2, 3, 3), 2, None),       # S 196, three full tiles and 4 tokens
          (1, 8, 16, (4, 8, 8), (2, 4, 4), 1, None),       # S 256, exact tiles
          (2, 4, 6, (4, 3, 3), (0, 1, 1), 2, (8, 3, 3)),   # t clipped: the table stride differs from the window
          (1, 16, 7, (8, 7, 7), (4, 0, 0), 2, None),       # the recipes' own windows, S 392 and 784, at 784 rows
          (1, 16, 7, (16, 7, 7), (0, 0, 0), 1, None))
# the backward's walk over several boxes per workgroup: 243 boxes, 4 per walk, 61 walks, the last one of 3
WALK_SHAPE = (9, 4, 6, (2, 3, 3), (1, 1, 1), 16, None)
FAMILIES = ("unit", "peaked", "bias_big", "zero_do")
HOT_SHAPE = SHAPES[0]                # cross_hot needs at most 32 regions and a mask


@dataclass(frozen=True)
class Case:
    name: str
    dims: tuple
    family: str = "unit"
    seed: int = 0

    @property
    def clips(self):
        return self.dims[0]

    @property
    def D(self):
        return self.dims[1]

    @property
    def G(self):
        return self.dims[2]

    @property
    def window(self):
        return self.dims[3]

    @property
    def shift(self):
        return self.dims[4]

    @property
    def H(self):
        return self.dims[5]

    @property
    def full(self):
        return self.dims[6] or self.dims[3]

    @property
    def S(self):
        return math.prod(self.window)

    @property
    def rows(self):
        return self.clips * self.D * self.G * self.G

    @property
    def nwin(self):
        return self.rows // self.S

    @property
    def ntable(self):
        return math.prod(2 * w - 1 for w in self.full)

    @property
    def nboxes(self):
        n = self.clips
        for ext, w, s in zip((self.D, self.G, self.G), self.window, self.shift):
            n *= ext // w + (1 if s else 0)
        return n


def _tag(d):
    w, s = "".join(map(str, d[3])), "".join(map(str, d[4]))
    return f"c{d[0]}D{d[1]}G{d[2]}w{w}s{s}h{d[5]}" + (f"W{''.join(map(str, d[6]))}" if d[6] else "")


def cases():
    """every shape under every family, and once more at zero shift (`unit`); the walk shape; cross_hot on the first shape"""
    out, seed, seen = [], 7500, set()
    for d in SHAPES:
        for fam in FAMILIES:
            out.append(Case(f"{_tag(d)}/{fam}", d, fam, seed))
            seed += 1
        seen.add(_tag(d))
    for d in SHAPES:
        z = d[:4] + ((0, 0, 0),) + d[5:]
        if _tag(z) not in seen:
            out.append(Case(f"{_tag(z)}/unit", z, "unit", seed))
            seed += 1
    for fam in ("unit", "peaked"):
        out.append(Case(f"walk/{_tag(WALK_SHAPE)}/{fam}", WALK_SHAPE, fam, seed))
        seed += 1
    out.append(Case(f"{_tag(HOT_SHAPE)}/cross_hot", HOT_SHAPE, "cross_hot", seed))
    return out


def walks(nboxes, H):
    """walks_of of csrc/swin3d_attn.hip restated -> (nwalks, per): the grid of the key-owning backward pass is (nwalks, H) and
    a workgroup walks the boxes [walk per, min((walk + 1) per, nboxes)) in ascending order"""
    n = min(nboxes, (1024 + H - 1) // H)
    per = (nboxes + n - 1) // n
    return (nboxes + per - 1) // per, per


# ------------------------------------------------------------------ geometry and bias ---------------------------------------
def _partition(t, window):
    """window_partition (swin_transformer.py:38-50) on a [B, D, G, G] tensor -> [B nW, S]"""
    B, D, Hh, Ww = t.shape
    wt, wh, ww = window
    return t.view(B, D // wt, wt, Hh // wh, wh, Ww // ww, ww).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, wt * wh * ww)


def mask_regions(D, G, window, shift):
    """compute_mask's img_mask (swin_transformer.py:317-324) -> [1, D, G, G]"""
    img = torch.zeros((1, D, G, G))
    cnt = 0
    for d in slice(-window[0]), slice(-window[0], -shift[0]), slice(-shift[0], None):
        for h in slice(-window[1]), slice(-window[1], -shift[1]), slice(-shift[1], None):
            for w in slice(-window[2]), slice(-window[2], -shift[2]), slice(-shift[2], None):
                img[:, d, h, w] = cnt
                cnt += 1
    return img


def rolled_geometry(case: Case, mut: Optional[str] = None):
    """the reference's own construction on row numbers (forward_part1 :227-235 and compute_mask restated): roll the grid of row
    numbers by -shift, partition it into windows, allow = (region difference == 0).  -> (idx [nwin, S], allow [nwin, S, S])"""
    B, D, G, window, shift = case.clips, case.D, case.G, case.window, case.shift
    rows = torch.arange(B * D * G * G).view(B, D, G, G)
    if any(shift):
        sgn = 1 if mut == "shift_sign" else -1
        rows = torch.roll(rows, shifts=tuple(sgn * s for s in shift), dims=(1, 2, 3))
    idx = _partition(rows, window)
    S = idx.shape[1]
    if not any(shift) or mut == "cross_box":
        return idx, torch.ones((idx.shape[0], S, S), dtype=torch.bool)
    img = mask_regions(D, G, window, shift)
    if mut == "t_wrap":          # the t axis not cut: its regions joined
        img = mask_regions(D, G, window, (0,) + tuple(shift[1:]))
    mw = _partition(img, window)
    allow = (mw[:, None, :] - mw[:, :, None]) == 0
    return idx, allow.repeat(B, 1, 1)


def row_regions(case: Case):
    """-> [rows] compute_mask's region of every row, in original coordinates"""
    idx, _ = rolled_geometry(case)
    reg = _partition(mask_regions(case.D, case.G, case.window, case.shift), case.window).repeat(case.clips, 1)
    out = torch.zeros(case.rows, dtype=torch.long)
    out[idx.reshape(-1)] = reg.reshape(-1).long()
    return out


def relative_position_index(full):
    """WindowAttention3D's buffer (swin_transformer.py:113-127) -> [N, N], N = Wt Wh Ww"""
    c = torch.stack(torch.meshgrid(torch.arange(full[0]), torch.arange(full[1]), torch.arange(full[2]), indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += full[0] - 1
    rel[:, :, 1] += full[1] - 1
    rel[:, :, 2] += full[2] - 1
    rel[:, :, 0] *= (2 * full[1] - 1) * (2 * full[2] - 1)
    rel[:, :, 1] *= 2 * full[2] - 1
    return rel.sum(-1)


def arithmetic_index(window, full, mut: Optional[str] = None):
    """the kernels' rule: index(q, k) = f(q) - f(k) + const over the tokens of an effective window -> [S, S]"""
    fh, fw = 2 * full[1] - 1, 2 * full[2] - 1
    t, h, w = (x.reshape(-1) for x in torch.meshgrid(*(torch.arange(n) for n in window), indexing="ij"))
    if mut == "swap_hw_f":
        h, w = w, h
    f = (t * fh + h) * fw + w
    Wt = window[0] if mut == "clipped_const" else full[0]
    const = ((Wt - 1) * fh + full[1] - 1) * fw + full[2] - 1
    return f[:, None] - f[None, :] + const


def bias_index(case: Case, mut: Optional[str] = None):
    """-> [S S] the table row of every (query, key) of a window: the reference's buffer sliced [:S, :S] (forward :151)"""
    S = case.S
    if mut in ("swap_hw_f", "clipped_const"):
        return arithmetic_index(case.window, case.full, mut).reshape(-1)
    idx = relative_position_index(case.full)[:S, :S]
    return (idx.t() if mut == "bias_T" else idx).reshape(-1)


def dense_bias(table, index, S):
    """table [ntable, H] -> [H, S, S]"""
    return table[index].view(S, S, -1).permute(2, 0, 1).contiguous()


# ------------------------------------------------------------------ inputs (CPU, fixed seeds) ------------------------------
def zero_head(case: Case):
    return min(1, case.H - 1)


def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(case.seed)
    M, H = case.rows, case.H
    q, k, v, do = (torch.randn((M, H * HD), generator=g) for _ in range(4))
    if case.family == "peaked":
        q, k = q * 2.5, k * 2.5
    table = (0.75 * torch.randn((case.ntable, H), generator=g)).to(F32)
    if case.family == "bias_big":        # the max and the lse come from the bias, not from q k
        table = (table * (BIAS_BIG / float(table.abs().amax()))).to(F32)
    elif case.family == "cross_hot":
        # swin_attn_cases.py's family on compute_mask's 27 regions: c q.k gets exactly 0 from the first 27 features on a pair
        # of one region and c HOT_Q HOT_K = 135.8 on a pair of different regions
        assert any(case.shift)
        hot = torch.nn.functional.one_hot(row_regions(case), 27).to(q.dtype)[:, None, :]
        q, k = q.view(M, H, HD), k.view(M, H, HD)
        q[:, :, :27] = HOT_Q * hot
        k[:, :, :27] = HOT_K * (1.0 - hot)
        q, k = q.reshape(M, H * HD), k.reshape(M, H * HD)
    elif case.family == "zero_do":       # dO = 0 for one head: its dq, dk, dv and its table gradient are exactly zero
        do.view(M, H, HD)[:, zero_head(case)] = 0.0
    return {"qkv": torch.cat([q, k, v], dim=1).to(BF16), "do": do.to(BF16), "table": table}


# ------------------------------------------------------------------ float64 references and bounds --------------------------
def expected(case: Case, inp):
    """-> dict name: (ref, bound) over out / dq / dk / dv [nwin, H, S, 32], lse [nwin, H, S], dtable [ntable, H]"""
    idx, allow = rolled_geometry(case)
    H, S, n = case.H, case.S, idx.shape[0]
    nT = (S + TILE - 1) // TILE
    q, k, v = gather(inp["qkv"], idx, H, 3)
    do = gather(inp["do"], idx, H)
    index = bias_index(case)
    bias = dense_bias(inp["table"].double(), index, S)[None]
    al = allow[:, None]
    zf = torch.where(al, q @ k.transpose(-1, -2) * SCALE + bias, torch.zeros((), dtype=F64))       # finite everywhere
    z = torch.where(al, zf, torch.full((), -math.inf, dtype=F64))
    eS = 2 * HD * U24 * (q.abs() @ k.abs().transpose(-1, -2))
    lse = torch.logsumexp(z, dim=-1)
    p = torch.exp(z - lse[..., None])
    O = p @ v
    zmax = zf.abs().amax(dim=-1, keepdim=True)
    resc = (nT - 1) * (8 * U24 * zmax + 5 * U24)
    rp = SCALE * eS + 4 * U24 * (zf.abs() + zmax) + 2 * U24 * bias.abs() + 4 * U24 + resc
    A = p @ v.abs()
    wrp = (p * rp).sum(dim=-1)
    rsum = (S / 4 + 16) * U24 + wrp
    E = (p * rp) @ v.abs() + 2 * S * U24 * A + rsum[..., None] * O.abs()
    b_out = U8 * A + E + U8 * (O.abs() + U8 * A + E)
    b_lse = wrp + (S / 4 + 16) * U24 + 32 * U24 + 4 * U24 * (lse.abs() + zmax[..., 0])
    # backward on the forward's own lse
    dP = do @ v.transpose(-1, -2)
    edP = 2 * HD * U24 * (do.abs() @ v.abs().transpose(-1, -2))
    delta = (p * dP).sum(dim=-1, keepdim=True)
    dS = p * (dP - delta)
    rpb = SCALE * eS + b_lse[..., None] + 4 * U24 * (zf.abs() + lse.abs()[..., None]) + 2 * U24 * bias.abs() + 4 * U24
    edelta = (p * (rpb * dP.abs() + edP)).sum(dim=-1, keepdim=True) + (S + 2) * U24 * (p * dP.abs()).sum(dim=-1, keepdim=True)
    ePb = p * (U8 + (1 + U8) * rpb)
    eDS32 = p * (rpb * (dP - delta).abs() + edP + edelta) + 2 * U24 * dS.abs()
    eDS = U8 * dS.abs() + (1 + U8) * eDS32
    dQ, dK, dV = dS @ k * SCALE, dS.transpose(-1, -2) @ q * SCALE, p.transpose(-1, -2) @ do
    acc = 2 * S * U24
    bQ = U8 * dQ.abs() + (1 + U8) * SCALE * (eDS @ k.abs() + acc * (dS.abs() @ k.abs()))
    bK = U8 * dK.abs() + (1 + U8) * SCALE * (eDS.transpose(-1, -2) @ q.abs() + acc * (dS.abs().transpose(-1, -2) @ q.abs()))
    bV = U8 * dV.abs() + (1 + U8) * (ePb.transpose(-1, -2) @ do.abs() + acc * (p.transpose(-1, -2) @ do.abs()))
    dB = dS.sum(dim=0)
    bB = eDS32.sum(dim=0) + 2 * n * U24 * dS.abs().sum(dim=0)
    cnt = torch.bincount(index, minlength=case.ntable).double()[:, None]
    dT = fold(dB, index, case.ntable)
    bT = fold(bB, index, case.ntable) + 2 * cnt * U24 * fold(dB.abs() + bB, index, case.ntable)
    return {"out": (O, b_out), "lse": (lse, b_lse), "dq": (dQ, bQ), "dk": (dK, bK), "dv": (dV, bV), "dtable": (dT, bT)}


# defects of the index, of the partition, of the mask's weight 0 and of the table gradient
MUTANTS = ("bias_T", "no_bias", "swap_hw_f", "clipped_const", "cross_box", "t_wrap", "shift_sign", "penalty_mask",
           "dtable_restart", "dtable_scaled")


def emulate(case: Case, inp, mut: Optional[str] = None):
    """The kernels' arithmetic restated in float64 with their rounding points inserted (fp32 scores, logits, running maximum,
    alpha, probabilities and sums under the online rescale over 64-key tiles; bf16 P and dS operands; one final rounding), on
    the windows of `rolled_geometry` (a masked key has p = 0, so a window's tiles carry its boxes' keys); `mut` inserts one
    defect.  -> what the kernels write, in the layout `compare` takes"""
    idx, allow = rolled_geometry(case, mut)
    H, S, M = case.H, case.S, case.rows
    q, k, v = gather(inp["qkv"], idx, H, 3)
    do = gather(inp["do"], idx, H)
    index = bias_index(case, mut)
    ntab = inp["table"].shape[0]
    table = inp["table"].double()
    bias = dense_bias(table, index.clamp(0, ntab - 1), S)[None]
    if mut == "no_bias":
        bias = torch.zeros_like(bias)
    r32 = lambda t: t.to(F32).double()
    r16 = lambda t: t.to(F32).to(BF16).double()
    al = allow[:, None]
    ninf = torch.full((), -math.inf, dtype=F64)
    xa = r32(r32(q @ k.transpose(-1, -2)) * SCALE + bias)
    if mut == "penalty_mask":          # the reference's -100 instead of the weight 0
        xa, al = torch.where(al, xa, r32(xa - 100.0)), torch.ones_like(al)
    x = torch.where(al, xa, ninf)
    m = torch.full(x.shape[:-1] + (1,), -math.inf, dtype=F64)
    l = torch.zeros_like(m)
    O = torch.zeros(x.shape[:-1] + (HD,), dtype=F64)
    for k0 in range(0, S, TILE):
        xt, vt = x[..., k0:k0 + TILE], v[..., k0:k0 + TILE, :]
        mn = torch.maximum(m, xt.amax(dim=-1, keepdim=True))
        safe = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)      # a tile with no key of the query's region yet
        alpha = r32(torch.exp(torch.where(torch.isinf(m), ninf, m - safe)))
        pu = r32(torch.exp(xt - safe))
        l = r32(r32(l * alpha) + pu.sum(dim=-1, keepdim=True))
        O = r32(r32(O * alpha) + r16(pu) @ vt)
        m = mn
    lse = r32(m + torch.log(l))
    out = r16(O / l)
    pb = torch.where(al, r32(torch.exp(x - lse)), torch.zeros((), dtype=F64))
    dP = r32(do @ v.transpose(-1, -2))
    delta = r32((pb * dP).sum(dim=-1, keepdim=True))
    ds32 = r32(pb * (dP - delta))
    dsb = r16(ds32)
    dq = r32(dsb @ k) * SCALE
    dk = r32(dsb.transpose(-1, -2) @ q) * SCALE
    dv = r32(r16(pb).transpose(-1, -2) @ do)
    # the table gradient: a workgroup's sum over its walk, the sum over the walks, the fold along the index
    n = idx.shape[0]
    nw, per = walks(n, H)
    per = max(per, 2) if mut == "dtable_restart" else per
    nw = (n + per - 1) // per
    dsc = torch.cat([ds32, torch.zeros((nw * per - n, H, S, S), dtype=F64)]).view(nw, per, H, S, S)
    if mut == "dtable_restart":        # the sum restarted at every window: the walk's last window alone
        last = torch.tensor([min((c + 1) * per, n) - 1 - c * per for c in range(nw)])
        partial = dsc[torch.arange(nw), last]
    else:
        partial = r32(dsc.sum(dim=1))
    dB = r32(partial.sum(dim=0))
    if mut == "dtable_scaled":
        dB = r32(dB * SCALE)
    keep = (index >= 0) & (index < ntab)
    dT = torch.zeros((ntab, H), dtype=F64)
    dT.index_add_(0, index[keep], dB.reshape(H, -1).t()[keep])
    return {"out": scatter(out.to(BF16), idx, M), "dqkv": torch.cat([scatter(t.to(BF16), idx, M) for t in (dq, dk, dv)], dim=1),
            "lse": scatter_stat(lse[..., 0], idx, M).to(F32), "dtable": dT.to(F32)}


def scatter_stat(t, idx, M):
    """[nwin, H, S] -> [M, H] rows"""
    n, H, S = t.shape
    out = torch.zeros((M, H), dtype=t.dtype)
    out[idx.reshape(-1)] = t.permute(0, 2, 1).reshape(n * S, H)
    return out


def gather_stat(x, idx):
    """[M, H] rows -> [nwin, H, S] (float64)"""
    n, S = idx.shape
    return x.double()[idx.reshape(-1)].reshape(n, S, -1).permute(0, 2, 1)


def compare(case: Case, inp, got, exp=None) -> Dict[str, float]:
    """worst error / bound of every result in `got`: out [M, C], dqkv [M, 3 C], lse [M, H] (natural log), dtable"""
    idx, _ = rolled_geometry(case)
    exp = exp or expected(case, inp)
    res = {}
    if "out" in got:
        res["out"] = ratio(gather(got["out"], idx, case.H), *exp["out"])
    if "dqkv" in got:
        d = gather(got["dqkv"], idx, case.H, 3)
        for i, name in enumerate(("dq", "dk", "dv")):
            res[name] = ratio(d[i], *exp[name])
    if "lse" in got:
        res["lse"] = ratio(gather_stat(got["lse"], idx), *exp["lse"])
    if "dtable" in got:
        res["dtable"] = ratio(got["dtable"], *exp["dtable"])
    return res


def lone_rows(case: Case):
    """-> the rows of the tokens that are alone in their box (a one-key softmax)"""
    idx, allow = rolled_geometry(case)
    return idx[allow.sum(dim=-1) == 1]


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
class Runner:
    def __init__(self, ops, dev):
        self.ops, self.dev = ops, dev

    def launch(self, case: Case, inp, start=None):
        """forward, backward on the forward's own results; every result buffer is pre-filled with SENTINEL (dtable with
        `start` or zeros: the backward adds) and followed by 64 spare elements"""
        ops, dev = self.ops, self.dev
        H, M, C = case.H, case.rows, case.H * HD
        got, bufs = {}, {}

        def new(name, shape, dtype, fill=SENTINEL):
            n = math.prod(shape)
            buf = torch.full((n + 64,), SENTINEL, dtype=dtype, device=dev)
            buf[:n] = fill if not torch.is_tensor(fill) else fill.reshape(-1).to(dev)
            got[name], bufs[name] = buf[:n].view(shape), buf
            return got[name]

        qkv, do, table = inp["qkv"].to(dev), inp["do"].to(dev), inp["table"].to(dev)
        out, lse2, delta = new("out", (M, C), BF16), new("lse2", (M, H), F32), new("delta", (M, H), F32)
        dqkv = new("dqkv", (M, 3 * C), BF16)
        dtable = new("dtable", (case.ntable, H), F32, 0.0 if start is None else start)
        geom = (case.clips, case.D, case.G, H, case.window, case.shift, case.full)
        ops.swin3d_attn_fwd(qkv, table, out, lse2, *geom)
        ops.swin3d_attn_bwd(qkv, table, do, lse2, delta, dqkv, dtable, *geom)
        # the same backward without a table gradient: the bits of dqkv must not depend on it
        dq2, de2 = torch.full_like(dqkv, SENTINEL), torch.full_like(delta, SENTINEL)
        ops.swin3d_attn_bwd(qkv, table, do, lse2, de2, dq2, None, *geom)
        got["dqkv_notable"] = dq2
        return got, bufs

    def run_case(self, case: Case):
        inp = make_inputs(case)
        exp = expected(case, inp)
        got, bufs = self.launch(case, inp)
        again, _ = self.launch(case, inp)
        torch.cuda.synchronize()
        H, C = case.H, case.H * HD
        rec = {"checks": {}, "repeat": {}, "spare_intact": {}, "finite": {}, "hash": {}}
        for name, t in got.items():
            rec["repeat"][name] = bool(torch.equal(_bits(t), _bits(again[name])))
            if name in bufs:
                rec["spare_intact"][name] = bool((bufs[name][t.numel():] == SENTINEL).all())
            rec["hash"][name] = _digest(_bits(t))
        rec["dqkv_without_dtable_same_bits"] = bool(torch.equal(_bits(got["dqkv"]), _bits(got["dqkv_notable"])))
        host = {"out": got["out"].cpu(), "dqkv": got["dqkv"].cpu(), "lse": got["lse2"].cpu().double() * LN2, "dtable": got["dtable"].cpu()}
        for name, t in host.items():
            rec["finite"][name] = bool(torch.isfinite(t.float()).all())
        rec["checks"] = compare(case, inp, host, exp)
        # the table gradient ADDS: from dyadic non-zero values; one more fp32 rounding of start + sum
        g = torch.Generator().manual_seed(case.seed + 50000)
        start = (torch.randint(-32, 33, (case.ntable, H), generator=g).double() / 8).to(F32)
        start[start == 0] = 0.125
        got3, _ = self.launch(case, inp, start)
        torch.cuda.synchronize()
        dT, bT = exp["dtable"]
        ref = start.double() + dT
        rec["checks"]["dtable_added"] = ratio(got3["dtable"].cpu(), ref, bT + U24 * (ref.abs() + bT))
        rec["walks"] = list(walks(case.nboxes, H))
        if case.family == "zero_do":
            zh = zero_head(case)
            cols = slice(zh * HD, (zh + 1) * HD)
            d = host["dqkv"].view(case.rows, 3, C)
            rec["zero_head"] = {"dq": not d[:, 0, cols].any(), "dk": not d[:, 1, cols].any(), "dv": not d[:, 2, cols].any(),
                                "dtable": not host["dtable"][:, zh].any(), "other_heads_live": bool(host["dtable"].any()) or H == 1}
        rows = lone_rows(case)
        if rows.numel():
            # a token alone in its box: p = 1, so out = v, dv = dO, dq = dk = 0, bit for bit
            qkv, d = inp["qkv"].view(case.rows, 3, C), host["dqkv"].view(case.rows, 3, C)
            rec["one_key"] = {"tokens": int(rows.numel()), "out_is_v": bool(torch.equal(_bits(host["out"][rows]), _bits(qkv[rows, 2]))),
                              "dv_is_do": bool(torch.equal(_bits(d[rows, 2]), _bits(inp["do"][rows]))),
                              "dq_zero": not d[rows, 0].any(), "dk_zero": not d[rows, 1].any()}
        return rec

    # ---- refusals
    def refusals(self):
        """geometry outside the limits: an error through aim_last_error and nothing written (the buffers are far too small for
        these shapes: a launch would be out of bounds)"""
        import ctypes
        dev, lib, out = self.dev, self.ops.load_library(), {}
        # clips, D, G, H, window, shift, full
        table = {"window does not divide D": (1, 6, 6, 1, (4, 3, 3), (0, 0, 0), (4, 3, 3)),
                 "window does not divide G": (1, 4, 14, 1, (2, 4, 7), (0, 0, 0), (2, 4, 7)),
                 "shift outside the window": (1, 4, 14, 1, (2, 7, 7), (1, 7, 3), (2, 7, 7)),
                 "negative shift": (1, 4, 14, 1, (2, 7, 7), (-1, 3, 3), (2, 7, 7)),
                 "shift on a window that spans its axis": (1, 4, 7, 1, (2, 7, 7), (1, 3, 0), (2, 7, 7)),
                 "too many tokens": (1, 16, 9, 1, (16, 9, 9), (0, 0, 0), (16, 9, 9)),
                 "too many table entries": (1, 16, 8, 1, (16, 8, 8), (0, 0, 0), (16, 8, 8)),
                 "full window smaller than the window": (1, 4, 6, 1, (4, 3, 3), (0, 0, 0), (2, 3, 3)),
                 "rows overflow 32-bit offsets": (40000, 16, 56, 4, (8, 7, 7), (4, 3, 3), (8, 7, 7))}
        for name, (B, D, G, H, w, s, f) in table.items():
            t16 = torch.full((256,), SENTINEL, dtype=BF16, device=dev)
            o16, d16 = t16.clone(), t16.clone()
            l32, b32, e32 = (torch.full((256,), SENTINEL, dtype=F32, device=dev) for _ in range(3))
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc_f = lib.aim_swin3d_attn_fwd(t16.data_ptr(), b32.data_ptr(), o16.data_ptr(), l32.data_ptr(), B, D, G, H, *w, *s, *f, st)
            msg_f = lib.aim_last_error().decode() if rc_f else None
            rc_b = lib.aim_swin3d_attn_bwd(t16.data_ptr(), b32.data_ptr(), t16.data_ptr(), l32.data_ptr(), e32.data_ptr(), d16.data_ptr(),
                                           None, B, D, G, H, *w, *s, *f, None, 0, st)
            msg_b = lib.aim_last_error().decode() if rc_b else None
            torch.cuda.synchronize()
            intact = all(bool((t == SENTINEL).all()) for t in (o16, d16, l32, b32, e32))
            out[name] = {"fwd": msg_f, "bwd": msg_b, "nothing_written": intact}
        return out

    def _entry_buffers(self, case: Case):
        """correctly sized buffers of one case, each followed by 64 spare elements, all filled with SENTINEL"""
        H, M, C = case.H, case.rows, case.H * HD
        nbytes = int(self.ops.load_library().aim_swin3d_attn_bwd_workspace_bytes(case.clips, case.D, case.G, H, *case.window, *case.shift))
        sizes = {"qkv": (M * 3 * C, BF16), "out": (M * C, BF16), "dout": (M * C, BF16), "dqkv": (M * 3 * C, BF16),
                 "table": (case.ntable * H, F32), "lse": (M * H, F32), "delta": (M * H, F32), "dtable": (case.ntable * H, F32),
                 "workspace": (nbytes // 4, F32)}
        return {k: torch.full((n + 64,), SENTINEL, dtype=dt, device=self.dev) for k, (n, dt) in sizes.items()}, nbytes

    def _call(self, lib, case: Case, which, ptr, nbytes):
        import ctypes
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        geom = (case.clips, case.D, case.G, case.H, *case.window, *case.shift, *case.full)
        if which == "fwd":
            rc = lib.aim_swin3d_attn_fwd(ptr["qkv"], ptr["table"], ptr["out"], ptr["lse"], *geom, st)
        else:
            rc = lib.aim_swin3d_attn_bwd(ptr["qkv"], ptr["table"], ptr["dout"], ptr["lse"], ptr["delta"], ptr["dqkv"], ptr["dtable"],
                                         *geom, ptr["workspace"], nbytes, st)
        return rc, (lib.aim_last_error().decode() if rc else None)

    def pointer_refusals(self):
        """null pointers, bf16 pointers off by 2 bytes, fp32 pointers off by 2 bytes and a short or missing workspace: a
        non-zero return, a message and nothing written"""
        lib, out = self.ops.load_library(), {}
        case = Case("r", SHAPES[0])
        bufs, nbytes = self._entry_buffers(case)
        good = {k: (t.data_ptr() or None) for k, t in bufs.items()}
        forms = {"fwd": [(f"null {k}", {k: None}, nbytes) for k in ("qkv", "table", "out", "lse")] +
                        [(f"{k} off by 2 bytes", {k: good[k] + 2}, nbytes) for k in ("qkv", "out", "table", "lse")],
                 "bwd": [(f"null {k}", {k: None}, nbytes) for k in ("qkv", "table", "dout", "lse", "delta", "dqkv")] +
                        [(f"{k} off by 2 bytes", {k: good[k] + 2}, nbytes) for k in ("qkv", "dout", "dqkv", "delta", "dtable", "workspace")] +
                        [("workspace 4 bytes short", {}, nbytes - 4), ("null workspace", {"workspace": None}, nbytes)]}
        for which, table in forms.items():
            for name, change, nb in table:
                rc, msg = self._call(lib, case, which, {**good, **change}, nb)
                torch.cuda.synchronize()
                intact = all(bool((t == SENTINEL).all()) for t in bufs.values())
                out[f"swin3d_attn_{which}: {name}"] = {"rc": rc, "message": msg, "nothing_written": intact}
        return out

    def workspace_guard(self, case: Case):
        """the backward called directly with a workspace of exactly the reported size: the 64 floats behind it are intact, and
        the results have the bits that ops' own call gives"""
        lib = self.ops.load_library()
        inp = make_inputs(case)
        got, _ = self.launch(case, inp)
        bufs, nbytes = self._entry_buffers(case)
        for k, t in (("qkv", inp["qkv"]), ("dout", inp["do"]), ("table", inp["table"]), ("lse", got["lse2"])):
            bufs[k][:t.numel()] = t.reshape(-1).to(self.dev)
        bufs["dtable"][:-64] = 0.0
        rc, msg = self._call(lib, case, "bwd", {k: t.data_ptr() for k, t in bufs.items()}, nbytes)
        torch.cuda.synchronize()
        n = nbytes // 4
        nw, per = walks(case.nboxes, case.H)
        return {"rc": rc, "message": msg, "workspace_bytes": [nbytes, (nw + 1) * case.H * case.S ** 2 * 4],
                "sentinels_intact": bool((bufs["workspace"][n:] == SENTINEL).all()),
                "workspace_written": bool((bufs["workspace"][:n] != SENTINEL).any()),
                "other_spares_intact": all(bool((bufs[k][-64:] == SENTINEL).all()) for k in ("dqkv", "dtable", "delta")),
                "dtable_same_bits": bool(torch.equal(_bits(bufs["dtable"][:-64]), _bits(got["dtable"].reshape(-1)))),
                "dqkv_same_bits": bool(torch.equal(_bits(bufs["dqkv"][:-64]), _bits(got["dqkv"].reshape(-1))))}


def main(argv):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    import time
    (path,) = argv
    run, res, t0 = Runner(ops, torch.device("cuda")), {"cases": {}}, time.time()
    with torch.no_grad():
        res["refusals"] = run.refusals()
        res["pointer_refusals"] = run.pointer_refusals()
        res["workspace_guard"] = run.workspace_guard(Case("guard", WALK_SHAPE, "unit", 7499))
        for case in cases():
            res["cases"][case.name] = run.run_case(case)
    res["seconds"] = time.time() - t0
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
