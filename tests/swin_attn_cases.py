"""Every call form of the Swin attention kernels (aim_swin_win_attn_fwd / _bwd, aim_swin_tattn_fwd / _bwd and
aim_swin_bias_scatter, csrc/swin_attn.hip), float64 closed forms per (window, head) and per (sequence, head), and bounds
derived from the kernels' rounding points.

A plain module in the manner of win_attn_cases.py: `test_swin_attn_gpu.py` runs `python swin_attn_cases.py OUT.json` once (one
child process for the whole list) and `test_swin_attn_cases_cpu.py` proves on the CPU that the bounds accept an emulation of
the kernels' arithmetic and reject the defects they are meant to catch (MUTANTS).

Two more lists run in a second child (`python swin_attn_cases.py --sweep OUT.json`, tests/test_swin_attn_sweep_gpu.py) under the
same references and bounds, which do not depend on how the backward splits its work:
  chunk_cases()  the backward's walk over several sequences per workgroup.  `chunks` restates the kernels' chunks_of; every case
                 of `cases()` has one sequence per workgroup, these have 3 (windows of 49, 64 and 16 tokens, T' = 5 and 32) and 8,
                 a short last chunk, and a walk length coprime to the windows of a frame, so one workgroup meets different
                 region patterns in turn.  The second launch replaces one mid-chunk sequence: no other row may change.
  sweep_cases()  every T' from 1 to 32 and every window side from 1 to 8 at every shift, three more input families (bias_big:
                 |bias| up to 40; cross_hot: every masked score 126 or more above every allowed one; zero_do: one head of dO
                 zero, that head's gradients exactly zero), and on the shifts 1 and w - 1 the tokens that are alone in their
                 region: out = v, dv = dO, dq = dk = 0 bit for bit, and nothing of them in the bias gradients.
The child also asks for the refusal of null and misaligned pointers and of a short or missing workspace, checks the floats
behind a workspace of exactly the reported size, and adds a scatter onto a non-zero table.  NEW_MUTANTS are the defects of
that ground: a stale region table, a bias-gradient sum restarted per sequence, a dropped short chunk, a max over masked keys, the
reference's -100 in place of the weight 0, a scaled bias gradient.

Geometry.  Window cases: `frames` frames of a res x res grid, frame-major rows f res^2 + y res + x.  Token i = (iy, ix) of
window (wy, wx) has ROLLED coordinates (wy w + iy, wx w + ix) and lies at row ((wy w + iy + s) mod res, (wx w + ix + s) mod res):
the reference's roll by -s, window_partition, window_reverse and roll back.  With s > 0 each rolled axis has the regions
[0, res - w), [res - w, res - s), [res - s, res); a pair of different regions (attn_mask = -100 in the reference) has the
weight exactly 0 (`geometry`; `rolled_geometry` restates the reference's own construction with torch.roll on row numbers).
Temporal cases: token t of sequence (b, n) is row (b T + t) L + n; nothing is masked.
The dense bias [H, S, S] is table[index] with the reference's relative_position_index / t_relative_coords.

Notation: one item = one (sequence, head): q, k, v [S, 32] (bf16 values), c = 32^-1/2, z = c q k^T + bias on the allowed
pairs, p = softmax(z), O = p v, lse = log sum exp z; dP = dO v^T, delta = rowsum(dO o O), dS = p o (dP - delta), dQ = c dS k,
dK = c dS^T q, dV = p^T dO, dbias = sum over sequences of dS, dtable[t] = sum of dbias over the index entries equal to t.
u = 2^-24 (fp32), U8 = 2^-8 (half a bf16 ulp, relative).

Bounds, from the rounding points of csrc/swin_attn.hip (those of attn_cases.py with 64 -> 32, 1/8 -> c and the bias term):
  S and dP are fp32 MFMA sums of 32 exact bf16 products:       eS = 2 . 32 u sum |q||k|,  edP = 2 . 32 u sum |dO||v|
  forward: x = fma(s, c log2 e, bias log2 e), p' = exp2(x - max) in fp32, unnormalised (max 1): the exponent carries c eS, the
    rounding of bias log2 e (u |bias|, twice with the fma's own), three fp32 roundings of numbers no larger than |z| + |z|max
    and v_exp_f32's ulp:                  rp = c eS + 4 u (|z| + |z|max) + 2 u |bias| + 4 u          (relative)
  p' is rounded to bf16, O accumulates in fp32 over the keys (2 S u), is scaled by 1 / sum (S fp32 terms, each off by rp:
    (S / 4 + 16) u + the p-weighted mean of rp =: rsum) and rounded once:
      |out - O| <= U8 A + E + U8 (|O| + U8 A + E),   A = sum_j p_j |v_j|,   E = sum_j p_j rp_j |v_j| + 2 S u A + rsum |O|
  lse = (max + log2 sum) ln 2:  |lse' - lse| <= sum_j p_j rp_j + (S / 4 + 16) u + 32 u + 4 u (|lse| + |z|max)
  backward (given the forward kernel's own lse, whose error elog is the bound above):
    p' = exp2(x - lse2): rp_b = c eS + elog + 4 u (|z| + |lse|) + 2 u |bias| + 4 u;  delta' = fp32 sum_j p'_j dP'_j:
    edelta = sum_j p_j (rp_b |dP_j| + edP_j) + (S + 2) u sum_j p_j |dP_j|;  dS32 = p' (dP' - delta') in fp32:
      eDS32 = p (rp_b |dP - delta| + edP + edelta) + 2 u |dS|
    dbias sums dS32 over the nseq sequences in fp32 (chunk partials, then the chunks):
      |dbias' - dbias| <= sum_seq eDS32 + 2 nseq u sum_seq |dS|
    dtable adds the n_t entries of a table row in fp32:  fold(bound) + 2 n_t u fold(|dbias| + bound)
    P = bf16(p') for dV, bf16(dS32) for dQ and dK, c applied once in fp32, results rounded to bf16:
      ePb = p (U8 + (1 + U8) rp_b),  eDS = U8 |dS| + (1 + U8) eDS32
      |dQ' - dQ| <= U8 |dQ| + (1 + U8) c (sum_j eDS |k_j| + 2 S u sum_j |dS||k_j|)        (dK alike, over the queries)
      |dV' - dV| <= U8 |dV| + (1 + U8) (sum_i ePb |dO_i| + 2 S u sum_i p |dO_i|)
"""
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import U8, U24, _digest, ratio  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HD = 32
SCALE = 32.0 ** -0.5
LN2 = math.log(2.0)
# frames, res, window, shift, heads
WIN_SHAPES = ((2, 14, 7, 3, 1),      # 1 / 2 / 2 / 4-region windows
              (1, 7, 7, 0, 2),       # one window spans the grid
              (1, 16, 8, 4, 2),      # S = 64: the exact tile
              (3, 8, 4, 2, 3),       # S = 16 on the 32-slot kernel
              (1, 56, 7, 3, 4))      # the first stage's grid
# B, T', L, heads
T_SHAPES = ((1, 1, 5, 1), (2, 2, 49, 2), (1, 3, 10, 1), (1, 16, 64, 4), (1, 32, 8, 1))
FAMILIES = ("unit", "peaked")
# families of the new case lists only (chunk_cases, sweep_cases); `cases()` keeps FAMILIES
NEW_FAMILIES = ("bias_big", "cross_hot", "zero_do")
ALL_FAMILIES = FAMILIES + NEW_FAMILIES
BIAS_BIG = 40.0                      # bias_big: the largest |bias|
HOT_Q, HOT_K = 16.0, 48.0            # cross_hot: exact in bf16; c HOT_Q HOT_K = 135.8 on a pair of different regions
# backward with per >= 2 sequences per workgroup.  windows (frames, res, w, s, H), temporal (B, T', L, H)
CHUNK_WIN = ((35, 14, 7, 3, 16),     # (a) CAP 64, S 49: nseq 140, per 3, 47 chunks, the last one of 2
             (35, 16, 8, 4, 16),     # (b) CAP 64, S 64
             (35, 8, 4, 2, 16))      # (c) CAP 32, S 16
CHUNK_T = ((1, 5, 140, 16),          # (d) a partial wave: nseq 140, per 3, 47 chunks, the last one of 2
           (1, 32, 70, 32))          #     T' 32: nseq 70, per 3, 24 chunks, the last one of 1
CHUNK_DEEP = (227, 6, 2, 1, 4)       # (e) nseq 2043, per 8, 256 chunks, the last one of 3; s = w - 1: one-key regions
SENTINEL = -7.0


@dataclass(frozen=True)
class Case:
    name: str
    kind: str            # "win" | "t"
    dims: tuple
    family: str = "unit"
    seed: int = 0

    @property
    def H(self):
        return self.dims[-1]

    @property
    def S(self):
        return self.dims[2] ** 2 if self.kind == "win" else self.dims[1]

    @property
    def rows(self):
        return self.dims[0] * self.dims[1] ** 2 if self.kind == "win" else self.dims[0] * self.dims[1] * self.dims[2]

    @property
    def nseq(self):
        if self.kind == "win":
            return self.dims[0] * (self.dims[1] // self.dims[2]) ** 2
        return self.dims[0] * self.dims[2]

    @property
    def ntable(self):
        return (2 * self.dims[2] - 1) ** 2 if self.kind == "win" else 2 * self.dims[1] - 1


def cap(S):
    return 32 if S <= 32 else 64


def cases():
    out, seed = [], 7000
    for d in WIN_SHAPES:
        for fam in FAMILIES:
            out.append(Case(f"win/f{d[0]}r{d[1]}w{d[2]}s{d[3]}h{d[4]}/{fam}", "win", d, fam, seed))
            seed += 1
    for d in T_SHAPES:
        for fam in FAMILIES:
            out.append(Case(f"t/B{d[0]}T{d[1]}L{d[2]}h{d[3]}/{fam}", "t", d, fam, seed))
            seed += 1
    return out


def chunks(nseq, H):
    """chunks_of of csrc/swin_attn.hip restated -> (nchunks, per): the backward grid is (nchunks, H) and a workgroup walks
    the `per` sequences [chunk per, min((chunk + 1) per, nseq)) in ascending order"""
    n = min(nseq, (1024 + H - 1) // H)
    per = (nseq + n - 1) // n
    return (nseq + per - 1) // per, per


def chunk_cases():
    """the backward's walk over several sequences per workgroup (per >= 3; per >= 8 in the deep case), both FAMILIES"""
    out, seed = [], 7100
    for kind, shapes in (("win", CHUNK_WIN), ("t", CHUNK_T), ("win", (CHUNK_DEEP,))):
        for d in shapes:
            for fam in FAMILIES:
                tag = f"f{d[0]}r{d[1]}w{d[2]}s{d[3]}h{d[4]}" if kind == "win" else f"B{d[0]}T{d[1]}L{d[2]}h{d[3]}"
                out.append(Case(f"chunk/{kind}/{tag}/{fam}", kind, d, fam, seed))
                seed += 1
    return out


def sweep_families(kind, dims):
    if kind == "t":
        return tuple(f for f in ALL_FAMILIES if f != "cross_hot") if dims[1] % 7 == 0 else ("unit",)
    w, s = dims[2], dims[3]
    return ALL_FAMILIES if w >= 5 and s in (1, w - 1) else ("unit",)


def sweep_cases():
    """every T' from 1 to 32 (B 2, L 5, H 2) and every window side from 1 to 8 at every shift (2 frames of a 3 w x 3 w grid,
    H 2: interior, edge and corner windows); `unit` everywhere, ALL_FAMILIES on every seventh T' (cross_hot needs a mask:
    windows only) and on w in 5..8 with s in {1, w - 1}"""
    out, seed = [], 7200
    for T in range(1, 33):
        d = (2, T, 5, 2)
        for fam in sweep_families("t", d):
            out.append(Case(f"sweep/t/T{T}/{fam}", "t", d, fam, seed))
            seed += 1
    for w in range(1, 9):
        for s in range(w):
            d = (2, 3 * w, w, s, 2)
            for fam in sweep_families("win", d):
                out.append(Case(f"sweep/win/w{w}s{s}/{fam}", "win", d, fam, seed))
                seed += 1
    return out


# ------------------------------------------------------------------ geometry and bias ---------------------------------------
def _regions(c, res, w, s):
    return torch.where(c < res - w, 0, torch.where(c < res - s, 1, 2)) if s else torch.zeros_like(c)


def geometry(case: Case, mut: Optional[str] = None):
    """-> (idx [nseq, S] rows, allow [nseq, S, S] bool): the kernels' address and mask rule (mut: one defect of it)"""
    if case.kind == "t":
        B, T, L, _ = case.dims
        b, n, t = torch.meshgrid(torch.arange(B), torch.arange(L), torch.arange(T), indexing="ij")
        idx = ((b * T + t) * L + n).reshape(B * L, T)
        return idx, torch.ones((B * L, T, T), dtype=torch.bool)
    frames, res, w, s, _ = case.dims
    nw = res // w
    f, wy, wx, iy, ix = torch.meshgrid(torch.arange(frames), torch.arange(nw), torch.arange(nw), torch.arange(w), torch.arange(w),
                                       indexing="ij")
    y, x = wy * w + iy, wx * w + ix
    sh = -s if mut == "shift_sign" else s
    oy, ox = (y + sh) % res, (x + sh) % res
    if mut == "swap_hw":
        oy, ox = ox, oy
    idx = (f * res * res + oy * res + ox).reshape(-1, w * w)
    reg = (_regions(y, res, w, s) * 3 + _regions(x, res, w, s)).reshape(-1, w * w)
    allow = reg[:, :, None] == reg[:, None, :]
    if mut == "no_mask":
        allow = torch.ones_like(allow)
    if mut == "stale_region":      # the region table of the chunk's first sequence kept for all of its sequences
        per = chunks(case.nseq, case.H)[1]
        allow = allow[torch.arange(case.nseq) // per * per]
    return idx, allow


def row_regions(case: Case):
    """-> [rows] the mask region of every row of a window case (0 where nothing is masked)"""
    frames, res, w, s, _ = case.dims
    idx, _ = geometry(case)
    nw = res // w
    _, wy, wx, iy, ix = torch.meshgrid(torch.arange(frames), torch.arange(nw), torch.arange(nw), torch.arange(w), torch.arange(w),
                                       indexing="ij")
    reg = _regions(wy * w + iy, res, w, s) * 3 + _regions(wx * w + ix, res, w, s)
    out = torch.zeros(case.rows, dtype=torch.long)
    out[idx.reshape(-1)] = reg.reshape(-1)
    return out


def lone_tokens(case: Case):
    """-> [nseq, S] bool: the tokens that are alone in their mask region (a one-key softmax inside a masked window)"""
    return geometry(case)[1].sum(dim=-1) == 1


def rolled_geometry(frames, res, w, s):
    """the reference's own construction on row numbers (swin2d_adapter.py:331-350 and :372-380 restated): roll the grid of
    row numbers by -s, partition it into windows, mask = (region difference != 0) from the three slices per axis"""
    rows = torch.arange(frames * res * res).view(frames, res, res)
    if s:
        rows = torch.roll(rows, shifts=(-s, -s), dims=(1, 2))
    part = lambda t: t.view(t.shape[0], res // w, w, res // w, w).permute(0, 1, 3, 2, 4).reshape(-1, w * w)
    idx = part(rows)
    nW = (res // w) ** 2
    if not s:
        return idx, torch.ones((idx.shape[0], w * w, w * w), dtype=torch.bool)
    img = torch.zeros((1, res, res))
    cnt = 0
    for hs in (slice(0, -w), slice(-w, -s), slice(-s, None)):
        for ws in (slice(0, -w), slice(-w, -s), slice(-s, None)):
            img[:, hs, ws] = cnt
            cnt += 1
    mw = part(img)
    allow = (mw[:, None, :] - mw[:, :, None]) == 0
    return idx, allow.repeat(frames, 1, 1).reshape(frames * nW, w * w, w * w)


def relative_position_index(w):
    """the reference's buffer (swin2d_adapter.py:187-196) -> [S*S]"""
    c = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(w), indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += w - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * w - 1
    return rel.sum(-1).reshape(-1)


def t_relative_coords(T):
    c = torch.arange(T)
    return (c[:, None] - c[None, :] + T - 1).reshape(-1)


def bias_index(case: Case, mut: Optional[str] = None):
    if case.kind == "win":
        return relative_position_index(case.dims[2])
    T = case.dims[1]
    c = torch.arange(T)
    return ((c[None, :] - c[:, None]) if mut == "t_neg" else (c[:, None] - c[None, :])).add(T - 1).reshape(-1)


def dense_bias(table, index, S, mut: Optional[str] = None):
    """table [ntable, H] -> [H, S, S]"""
    b = table[index].view(S, S, -1).permute(2, 0, 1)
    out = torch.empty((table.shape[1], S, S), dtype=table.dtype)      # (dense strides whatever the sizes)
    out.copy_(b.transpose(1, 2) if mut == "bias_T" else b)
    return out


# ------------------------------------------------------------------ inputs (CPU, fixed seeds) ------------------------------
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
        # The first nine features hold a region one-hot: HOT_Q e_r in q, HOT_K (1 - e_r) in k, so c q.k gets exactly 0 from
        # them on a pair of one region and c HOT_Q HOT_K = 135.8 on a pair of different regions: every masked score is far
        # above every allowed one.  The float64 reference masks with -inf and never sees them.  (At +60 an fp32 kernel
        # that took its max over the masked keys, or masked with the reference's -100, would still pass: e^-60 is a
        # normal fp32 number and e^(60 - 100) is below every bound.  The gain has to exceed 100 + the spread of the scores
        # for the -100 mask and 2^-149 for the max, hence 135.8.)  On such inputs the reference project's -100 mask
        # differs from the weight 0 BY DESIGN: this family tests the kernels' documented contract only.
        assert case.kind == "win" and case.dims[3] > 0, "cross_hot needs a shifted window case"
        hot = torch.nn.functional.one_hot(row_regions(case), 9).to(q.dtype)[:, None, :]
        q, k = q.view(M, H, HD), k.view(M, H, HD)
        q[:, :, :9] = HOT_Q * hot
        k[:, :, :9] = HOT_K * (1.0 - hot)
        q, k = q.reshape(M, H * HD), k.reshape(M, H * HD)
    elif case.family == "zero_do":       # dO = 0 for one head: its dq, dk, dv and its bias gradients are exactly zero
        do.view(M, H, HD)[:, zero_head(case)] = 0.0
    return {"qkv": torch.cat([q, k, v], dim=1).to(BF16), "do": do.to(BF16), "table": table}


def zero_head(case: Case):
    return min(1, case.H - 1)


def gather(x, idx, H, parts=1):
    """[M, parts C] rows -> `parts` tensors [nseq, H, S, 32] (float64)"""
    n, S = idx.shape
    t = x.double()[idx.reshape(-1)].reshape(n, S, parts, H, HD).permute(2, 0, 3, 1, 4)
    return [t[i] for i in range(parts)] if parts > 1 else t[0]


def scatter(t, idx, M):
    """[nseq, H, S, 32] -> [M, C] rows"""
    n, H, S, _ = t.shape
    out = torch.zeros((M, H * HD), dtype=t.dtype)
    out[idx.reshape(-1)] = t.permute(0, 2, 1, 3).reshape(n * S, H * HD)
    return out


def fold(dense, index, ntable):
    """[H, S, S] -> [ntable, H]: sum over the index entries of each table row"""
    H = dense.shape[0]
    out = torch.zeros((ntable, H), dtype=dense.dtype)
    out.index_add_(0, index, dense.reshape(H, -1).t().contiguous())
    return out


# ------------------------------------------------------------------ float64 references and bounds --------------------------
def expected(case: Case, inp):
    """-> dict name: (ref, bound) over out / dq / dk / dv [nseq, H, S, 32], lse [nseq, H, S], dbias [H, S, S], dtable"""
    idx, allow = geometry(case)
    H, S, n = case.H, case.S, idx.shape[0]
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
    rp = SCALE * eS + 4 * U24 * (zf.abs() + zmax) + 2 * U24 * bias.abs() + 4 * U24
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
    return {"out": (O, b_out), "lse": (lse, b_lse), "dq": (dQ, bQ), "dk": (dK, bK), "dv": (dV, bV), "dbias": (dB, bB),
            "dtable": (dT, bT)}


MUTANTS = ("bias_T", "no_mask", "shift_sign", "swap_hw", "t_neg")
# defects of the walk over several sequences per workgroup, of the mask's weight 0 and of the bias gradient's scale
NEW_MUTANTS = ("stale_region", "db_last_only", "drop_ragged_chunk", "max_before_mask", "penalty_mask", "dbias_scaled")


def emulate(case: Case, inp, mut: Optional[str] = None):
    """The kernels' arithmetic restated in float64 with their rounding points inserted (fp32 scores, logits, probabilities and
    sums; bf16 P and dS operands; one final rounding); `mut` inserts one defect.  -> what the kernels write, in `results`'
    layout (the backward takes the emulated forward's out and lse)."""
    idx, allow = geometry(case, mut)
    H, S, M = case.H, case.S, case.rows
    q, k, v = gather(inp["qkv"], idx, H, 3)
    do = gather(inp["do"], idx, H)
    index = bias_index(case, mut)
    bias = dense_bias(inp["table"].double(), index, S, mut)[None]
    r32 = lambda t: t.to(F32).double()
    r16 = lambda t: t.to(F32).to(BF16).double()
    al = allow[:, None]
    ninf = torch.full((), -math.inf, dtype=F64)
    xa = r32(r32(q @ k.transpose(-1, -2)) * SCALE + bias)
    if mut == "penalty_mask":          # the reference's -100 instead of the weight 0
        xa, al = torch.where(al, xa, r32(xa - 100.0)), torch.ones_like(al)
    x = torch.where(al, xa, ninf)
    mx = (xa if mut == "max_before_mask" else x).amax(dim=-1, keepdim=True)
    pu = r32(torch.exp(x - mx))        # (fp32: below 2^-149 it is 0)
    tot = r32(pu.sum(dim=-1, keepdim=True))
    lse = r32(mx + torch.log(tot))
    out = r16(r32(r16(pu) @ v) / tot)
    pb = torch.where(al, r32(torch.exp(x - lse)), torch.zeros((), dtype=F64))
    dP = r32(do @ v.transpose(-1, -2))
    delta = r32((pb * dP).sum(dim=-1, keepdim=True))
    ds32 = r32(pb * (dP - delta))
    dsb = r16(ds32)
    dq = r32(dsb @ k) * SCALE
    dk = r32(dsb.transpose(-1, -2) @ q) * SCALE
    dv = r32(r16(pb).transpose(-1, -2) @ do)
    # the two stages of the bias gradient: a workgroup's sum over the sequences of its chunk, then the sum over the chunks
    n = idx.shape[0]
    nch, per = chunks(n, H)
    dsc = torch.cat([ds32, torch.zeros((nch * per - n, H, S, S), dtype=F64)]).view(nch, per, H, S, S)
    if mut == "db_last_only":          # the sum restarted at every sequence: the chunk's last sequence alone
        last = torch.tensor([min((c + 1) * per, n) - 1 - c * per for c in range(nch)])
        partial = dsc[torch.arange(nch), last]
    else:
        partial = r32(dsc.sum(dim=1))
    if mut == "drop_ragged_chunk" and n % per:
        partial = partial[:-1]
    dB = r32(partial.sum(dim=0))
    if mut == "dbias_scaled":
        dB = r32(dB * SCALE)
    return {"out": scatter(out.to(BF16), idx, M), "dqkv": torch.cat([scatter(t.to(BF16), idx, M) for t in (dq, dk, dv)], dim=1),
            "lse": lse[..., 0].to(F32), "dbias": dB.to(F32), "dtable": fold(dB, bias_index(case, mut), case.ntable).to(F32)}


def compare(case: Case, inp, got) -> Dict[str, float]:
    """worst error / bound of every result in `got`: out [M, C], dqkv [M, 3 C], lse [nseq, H, S] (natural log), dbias, dtable
    (the TRUE sequences are read back out of the row tensors)"""
    idx, _ = geometry(case)
    exp = expected(case, inp)
    res = {}
    if "out" in got:
        res["out"] = ratio(gather(got["out"], idx, case.H), *exp["out"])
    if "dqkv" in got:
        d = gather(got["dqkv"], idx, case.H, 3)
        for i, name in enumerate(("dq", "dk", "dv")):
            res[name] = ratio(d[i], *exp[name])
    for name in ("lse", "dbias", "dtable"):
        if name in got:
            res[name] = ratio(got[name], *exp[name])
    return res


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Runner:
    def __init__(self, ops, dev):
        self.ops, self.dev = ops, dev

    def launch(self, case: Case, inp):
        """forward, backward on the forward's own results, scatter; every result buffer is pre-filled with SENTINEL (dtable
        with zeros: the scatter adds) and followed by 64 spare elements"""
        ops, dev = self.ops, self.dev
        H, S, M, C = case.H, case.S, case.rows, case.H * HD
        got, bufs = {}, {}

        def new(name, shape, dtype, fill=SENTINEL):
            n = math.prod(shape)
            buf = torch.full((n + 64,), SENTINEL, dtype=dtype, device=dev)
            buf[:n] = fill
            got[name], bufs[name] = buf[:n].view(shape), buf
            return got[name]

        qkv, do = inp["qkv"].to(dev), inp["do"].to(dev)
        index = bias_index(case).to(torch.int32).to(dev)
        bias = dense_bias(inp["table"], bias_index(case), S).to(dev)
        out, lse2 = new("out", (M, C), BF16), new("lse2", (case.nseq, H, cap(S)), F32)
        dqkv, dbias = new("dqkv", (M, 3 * C), BF16), new("dbias", (H, S, S), F32)
        dtable = new("dtable", (case.ntable, H), F32, 0.0)
        if case.kind == "win":
            geom = (case.dims[0], case.dims[1], H, case.dims[2], case.dims[3])
            ops.swin_win_attn_fwd(qkv, bias, out, lse2, *geom)
            ops.swin_win_attn_bwd(qkv, bias, do, lse2, dqkv, dbias, *geom)
        else:
            geom = (case.dims[0], case.dims[1], case.dims[2], H)
            ops.swin_tattn_fwd(qkv, bias, out, lse2, *geom)
            ops.swin_tattn_bwd(qkv, bias, do, lse2, dqkv, dbias, *geom)
        ops.swin_bias_scatter(dbias, index, dtable)
        # the same backward without a bias gradient: the bits of dqkv must not depend on it
        dq2 = torch.full_like(dqkv, SENTINEL)
        (ops.swin_win_attn_bwd if case.kind == "win" else ops.swin_tattn_bwd)(qkv, bias, do, lse2, dq2, None, *geom)
        got["dqkv_nobias"] = dq2
        return got, bufs

    def run_case(self, case: Case, extras=False):
        inp = make_inputs(case)
        got, bufs = self.launch(case, inp)
        again, _ = self.launch(case, inp)
        torch.cuda.synchronize()
        S = case.S
        rec = {"checks": {}, "repeat": {}, "spare_intact": {}, "finite": {}, "hash": {}}
        for name, t in got.items():
            rec["repeat"][name] = bool(torch.equal(_bits(t), _bits(again[name])))
            if name in bufs:
                rec["spare_intact"][name] = bool((bufs[name][t.numel():] == SENTINEL).all())
            rec["hash"][name] = _digest(_bits(t))
        rec["slots_past_S_intact"] = bool((got["lse2"][..., S:] == SENTINEL).all())
        rec["dqkv_without_dbias_same_bits"] = bool(torch.equal(_bits(got["dqkv"]), _bits(got["dqkv_nobias"])))
        host = {"out": got["out"].cpu(), "dqkv": got["dqkv"].cpu(), "lse": got["lse2"][..., :S].cpu().double() * LN2,
                "dbias": got["dbias"].cpu(), "dtable": got["dtable"].cpu()}
        for name, t in host.items():
            rec["finite"][name] = bool(torch.isfinite(t.float()).all())
        rec["checks"] = compare(case, inp, host)
        if extras:
            self.exact_properties(case, inp, got, host, rec)
        return rec

    # ---- the exact properties of the new case lists
    def _other_rows_keep_their_bits(self, case, got, got2, rows):
        """`rows` of the inputs were replaced in the second launch: every other row of out and dqkv has the same bits"""
        keep = torch.ones(case.rows, dtype=torch.bool)
        keep[rows] = False
        keep = keep.to(self.dev)
        return {name: bool(torch.equal(_bits(got[name])[keep], _bits(got2[name])[keep])) for name in ("out", "dqkv", "dqkv_nobias")}

    def _replaced(self, case, inp, rows):
        g = torch.Generator().manual_seed(case.seed + 100000)
        qkv, do = inp["qkv"].clone(), inp["do"].clone()
        qkv[rows] = (1.5 * torch.randn((rows.numel(), qkv.shape[1]), generator=g)).to(BF16)
        do[rows] = (1.5 * torch.randn((rows.numel(), do.shape[1]), generator=g)).to(BF16)
        return {"qkv": qkv, "do": do, "table": inp["table"]}

    def exact_properties(self, case: Case, inp, got, host, rec):
        H, S, C = case.H, case.S, case.H * HD
        idx, _ = geometry(case)
        nch, per = chunks(case.nseq, H)
        rec["workspace_bytes"] = [int(self.ops.load_library().aim_swin_attn_bwd_workspace_bytes(case.nseq, H, S)), nch * H * S * S * 4]
        if case.family == "zero_do":
            cols = slice(zero_head(case) * HD, (zero_head(case) + 1) * HD)
            d = host["dqkv"].view(case.rows, 3, C)
            rec["zero_head"] = {"dq": not d[:, 0, cols].any(), "dk": not d[:, 1, cols].any(), "dv": not d[:, 2, cols].any(),
                                "dbias": not host["dbias"][zero_head(case)].any(), "dtable": not host["dtable"][:, zero_head(case)].any(),
                                "other_heads_live": bool(host["dbias"].any()) or H == 1}
        if case.kind == "win" and case.dims[2] > 1 and case.dims[3] in (1, case.dims[2] - 1):
            # a token alone in its region: p = 1, so out = v, dv = dO, dq = dk = 0, bit for bit, and dS = 0: nothing of it
            # reaches the bias gradient -- with its q, k, v and dO rows replaced the dense gradient keeps all its bits
            rows = idx[lone_tokens(case)]
            qkv, do, d = inp["qkv"].view(case.rows, 3, C), inp["do"], host["dqkv"].view(case.rows, 3, C)
            got2, _ = self.launch(case, self._replaced(case, inp, rows))
            torch.cuda.synchronize()
            others = self._other_rows_keep_their_bits(case, got, got2, rows)
            rec["one_key"] = {"tokens": int(rows.numel()), "out_is_v": bool(torch.equal(_bits(host["out"][rows]), _bits(qkv[rows, 2]))),
                              "dv_is_do": bool(torch.equal(_bits(d[rows, 2]), _bits(do[rows]))),
                              "dq_zero": not d[rows, 0].any(), "dk_zero": not d[rows, 1].any(),
                              "dbias_same_bits_with_the_token_replaced": bool(torch.equal(_bits(got["dbias"]), _bits(got2["dbias"]))),
                              "dtable_same_bits_with_the_token_replaced": bool(torch.equal(_bits(got["dtable"]), _bits(got2["dtable"]))),
                              "replaced_rows_differ": not torch.equal(_bits(got["out"])[rows.to(self.dev)], _bits(got2["out"])[rows.to(self.dev)]),
                              **{f"other_rows_{k}": v for k, v in others.items()}}
        if per > 1:
            # no leak between the sequences of one workgroup: the rows of one mid-chunk sequence replaced, every other
            # sequence's out, lse and dqkv rows keep their bits
            seq = (nch // 2) * per + 1
            assert seq % per == 1 and seq + 1 < min((nch // 2 + 1) * per, case.nseq)
            got2, _ = self.launch(case, self._replaced(case, inp, idx[seq]))
            torch.cuda.synchronize()
            sk = torch.ones(case.nseq, dtype=torch.bool, device=self.dev)
            sk[seq] = False
            rec["no_leak"] = {"sequence": seq, "chunk": nch // 2, "per": per,
                              "lse2": bool(torch.equal(_bits(got["lse2"])[sk], _bits(got2["lse2"])[sk])),
                              "replaced_sequence_differs": not torch.equal(_bits(got["lse2"])[seq], _bits(got2["lse2"])[seq]),
                              **self._other_rows_keep_their_bits(case, got, got2, idx[seq])}

    def refusals(self):
        """geometry outside the limits: an error through aim_last_error and nothing written (the buffers are far too small for
        these shapes: a launch would be out of bounds)"""
        dev, ops, out = self.dev, self.ops, {}
        lib = self.ops.load_library()
        import ctypes
        win = {"window over 64 tokens": (1, 18, 1, 9, 0), "window does not divide": (1, 14, 1, 4, 0),
               "shift outside the window": (1, 14, 1, 7, 7), "shift on a window that spans the grid": (1, 7, 1, 7, 3)}
        tmp = {"more than 32 frame tokens": (1, 33, 4, 1)}
        for table, fwd, bwd in ((win, "aim_swin_win_attn_fwd", "aim_swin_win_attn_bwd"), (tmp, "aim_swin_tattn_fwd", "aim_swin_tattn_bwd")):
            for name, geom in table.items():
                t16 = torch.full((256,), SENTINEL, dtype=BF16, device=dev)
                o16, d16 = t16.clone(), t16.clone()
                l32, b32 = (torch.full((256,), SENTINEL, dtype=F32, device=dev) for _ in range(2))
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                rc_f = getattr(lib, fwd)(t16.data_ptr(), b32.data_ptr(), o16.data_ptr(), l32.data_ptr(), *geom, st)
                msg_f = lib.aim_last_error().decode() if rc_f else None
                rc_b = getattr(lib, bwd)(t16.data_ptr(), b32.data_ptr(), t16.data_ptr(), l32.data_ptr(), d16.data_ptr(),
                                         None, *geom, None, 0, st)
                msg_b = lib.aim_last_error().decode() if rc_b else None
                torch.cuda.synchronize()
                intact = all(bool((t == SENTINEL).all()) for t in (o16, d16, l32, b32))
                out[name] = {"fwd": msg_f, "bwd": msg_b, "nothing_written": intact}
        return out

    def _entry_buffers(self, case: Case):
        """correctly sized buffers of one case, each followed by 64 spare elements, all filled with SENTINEL"""
        H, S, M, C = case.H, case.S, case.rows, case.H * HD
        nbytes = int(self.ops.load_library().aim_swin_attn_bwd_workspace_bytes(case.nseq, H, S))
        sizes = {"qkv": (M * 3 * C, BF16), "out": (M * C, BF16), "dout": (M * C, BF16), "dqkv": (M * 3 * C, BF16), "bias": (H * S * S, F32),
                 "lse": (case.nseq * H * cap(S), F32), "dbias": (H * S * S, F32), "workspace": (nbytes // 4, F32)}
        return {k: torch.full((n + 64,), SENTINEL, dtype=dt, device=self.dev) for k, (n, dt) in sizes.items()}, nbytes

    def _call(self, lib, case: Case, which, ptr, nbytes, dbias=True):
        import ctypes
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        geom = (case.dims[0], case.dims[1], case.H, case.dims[2], case.dims[3]) if case.kind == "win" else case.dims
        name = ("aim_swin_win_attn_" if case.kind == "win" else "aim_swin_tattn_") + which
        if which == "fwd":
            rc = getattr(lib, name)(ptr["qkv"], ptr["bias"], ptr["out"], ptr["lse"], *geom, st)
        else:
            rc = getattr(lib, name)(ptr["qkv"], ptr["bias"], ptr["dout"], ptr["lse"], ptr["dqkv"], ptr["dbias"] if dbias else None,
                                    *geom, ptr["workspace"], nbytes, st)
        return rc, (lib.aim_last_error().decode() if rc else None)

    def pointer_refusals(self):
        """null pointers, bf16 pointers off by 2 bytes and a short or missing workspace, on every entry that takes them: a
        non-zero return, a message and nothing written.  The buffers have the call's true sizes and 64 spare elements, so
        a pointer off by 2 bytes stays inside its buffer."""
        lib, out = self.ops.load_library(), {}
        for case in (Case("r", "win", (1, 8, 4, 2, 1)), Case("r", "t", (1, 4, 4, 1))):
            bufs, nbytes = self._entry_buffers(case)
            good = {k: (t.data_ptr() or None) for k, t in bufs.items()}
            forms = {"fwd": [(f"null {k}", {k: None}, nbytes) for k in ("qkv", "bias", "out", "lse")] +
                            [(f"{k} off by 2 bytes", {k: good[k] + 2}, nbytes) for k in ("qkv", "out")],
                     "bwd": [(f"null {k}", {k: None}, nbytes) for k in ("qkv", "bias", "dout", "lse", "dqkv")] +
                            [(f"{k} off by 2 bytes", {k: good[k] + 2}, nbytes) for k in ("qkv", "dout", "dqkv")] +
                            [("workspace 4 bytes short", {}, nbytes - 4), ("null workspace", {"workspace": None}, nbytes)]}
            for which, table in forms.items():
                for name, change, nb in table:
                    rc, msg = self._call(lib, case, which, {**good, **change}, nb)
                    torch.cuda.synchronize()
                    intact = all(bool((t == SENTINEL).all()) for t in bufs.values())
                    out[f"{'swin_win_attn_' if case.kind == 'win' else 'swin_tattn_'}{which}: {name}"] = \
                        {"rc": rc, "message": msg, "nothing_written": intact}
        return out

    def workspace_guard(self, case: Case):
        """the backward called directly with a workspace of exactly the reported size: the 64 floats behind it are intact,
        and the bias gradient has the bits that ops' own call gives"""
        lib = self.ops.load_library()
        inp = make_inputs(case)
        got, _ = self.launch(case, inp)
        bufs, nbytes = self._entry_buffers(case)
        for k, t in (("qkv", inp["qkv"]), ("dout", inp["do"]), ("bias", dense_bias(inp["table"], bias_index(case), case.S)), ("lse", got["lse2"])):
            bufs[k][:t.numel()] = t.reshape(-1).to(self.dev)
        rc, msg = self._call(lib, case, "bwd", {k: t.data_ptr() for k, t in bufs.items()}, nbytes)
        torch.cuda.synchronize()
        n = nbytes // 4
        return {"rc": rc, "message": msg, "workspace_bytes": nbytes, "sentinels_intact": bool((bufs["workspace"][n:] == SENTINEL).all()),
                "workspace_written": bool((bufs["workspace"][:n] != SENTINEL).any()),
                "other_spares_intact": all(bool((bufs[k][-64:] == SENTINEL).all()) for k in ("dqkv", "dbias")),
                "dbias_same_bits": bool(torch.equal(_bits(bufs["dbias"][:-64]), _bits(got["dbias"].reshape(-1)))),
                "dqkv_same_bits": bool(torch.equal(_bits(bufs["dqkv"][:-64]), _bits(got["dqkv"].reshape(-1))))}

    def scatter_adds(self):
        """aim_swin_bias_scatter ADDS: from a non-zero dtable of dyadic values, with 4 table rows that no index entry names
        (they keep their bits) and ntable H no multiple of the 128-thread block.  The dense gradient is given exactly, so the
        bound is the dtable bound's own fp32 sum term, 2 n_t u fold(|dense|), plus one rounding of start + sum."""
        out, H = {}, 3
        for name, index in (("window", relative_position_index(7)), ("temporal", t_relative_coords(16))):
            g = torch.Generator().manual_seed(7900 + len(out))
            SS, ntable = index.numel(), int(index.max()) + 1 + 4
            dense = torch.randn((H, SS), generator=g).to(F32)
            start = (torch.randint(-32, 33, (ntable, H), generator=g).double() / 8).to(F32)
            buf = torch.full((ntable * H + 64,), SENTINEL, dtype=F32, device=self.dev)
            dtable = buf[:ntable * H].view(ntable, H)
            dtable.copy_(start)
            S = int(math.isqrt(SS))
            self.ops.swin_bias_scatter(dense.view(H, S, S).to(self.dev), index.to(torch.int32).to(self.dev), dtable)
            torch.cuda.synchronize()
            got = dtable.cpu()
            cnt = torch.bincount(index, minlength=ntable).double()[:, None]
            add = fold(dense.double().view(H, S, S), index, ntable)
            ref = start.double() + add
            e_sum = 2 * cnt * U24 * fold(dense.double().abs().view(H, S, S), index, ntable)
            bound = e_sum + U24 * (ref.abs() + e_sum)
            named = cnt[:, 0] > 0
            out[name] = {"ratio": ratio(got[named], ref[named], bound[named]), "ntable_H": ntable * H, "unnamed_rows": int((~named).sum()),
                         "unnamed_rows_keep_their_bits": bool(torch.equal(_bits(got[~named]), _bits(start[~named]))),
                         "spare_intact": bool((buf[ntable * H:] == SENTINEL).all()), "start_nonzero": bool((start != 0).float().mean() > 0.9)}
        return out


def main(argv):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    dev = torch.device("cuda")
    run = Runner(ops, dev)
    res = {"cases": {}}
    if argv[0] == "--sweep":
        import time
        path, t0 = argv[1], time.time()
        with torch.no_grad():
            res["pointer_refusals"] = run.pointer_refusals()
            res["scatter_adds"] = run.scatter_adds()
            res["workspace_guard"] = run.workspace_guard(chunk_cases()[0])
            for case in chunk_cases() + sweep_cases():
                res["cases"][case.name] = run.run_case(case, extras=True)
        res["seconds"] = time.time() - t0
        with open(path, "w") as f:
            json.dump(res, f)
        return
    (path,) = argv
    with torch.no_grad():
        res["refusals"] = run.refusals()
        for case in cases():
            res["cases"][case.name] = run.run_case(case)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
