"""Every call form of the shifted 3-D window attention kernels (aim_win_attn_fwd_shift / aim_win_attn_bwd_shift,
csrc/win_attn.hip), float64 closed forms per box, and the bounds of win_attn_cases.py with S and nT of each box.

A plain module in the manner of win_attn_cases.py, whose references, bounds, gather / scatter and emulation it imports:
`test_win_attn_shift_gpu.py` runs `python win_attn_shift_cases.py OUT.json` once (one child process for the whole list) and
`test_win_attn_shift_cases_cpu.py` proves on the CPU that the bounds accept an emulation of the kernels' arithmetic on the
boxes and reject the addressing defects of MUTANTS.

Geometry.  B clips of T frames of N = G G + 1 tokens, a window (wt, wh, ww) clipped to the grid, a shift (st, sh, sw).  Each
axis on its own, in ORIGINAL (unrolled) coordinates:
  h (w alike), sh > 0: [0, G) is cut at 0, sh, sh + wh, sh + 2 wh, ..., G;  sh = 0: whole windows
  t: window k holds the frames (k wt + st + dt) mod T of its own clip
One box = one (t window, h segment, w segment); its tokens (dt, dh, dw) in row-major order have the frame-major rows
    (b T + (k wt + st + dt) mod T) N + 1 + (h0 + dh) G + w0 + dw                                   (`box_rows`)
One item = one (box, head): q, k, v [S, 64] with S = wt eh ew, which differs from box to box; `box_rows` returns the boxes
grouped by S so that each group is a dense [n, S] index like win_attn_cases.window_rows.

Bounds.  Inside a box the kernels are the unshifted kernels with S -> the box's S (the tile loop runs to the box's own S,
the rounding points do not move), so the bounds are win_attn_cases.forward_ref / attn_cases.backward_ref evaluated per
group.  No tolerance is introduced here.
"""
import contextlib
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cases as W  # noqa: E402
from attn_cases import handed_in, sink_rows  # noqa: E402
from gemm_cases import U24, _digest, ratio  # noqa: E402
from win_attn_cases import BF16, F32, FAMILIES, SENTINEL, _bits, class_rows, clip_window, gather, gather_stat, scatter  # noqa: E402

# B, T, G, H, window, shift
SHAPES = ((1, 32, 14, 2, (16, 7, 7), (8, 3, 3)),     # the hmdb51 form: S 144 ... 784, tails 16 and 0 mod 64
          (1, 32, 14, 1, (32, 2, 2), (0, 1, 1)),     # the diving48 / ucf101 form: 64 boxes, S 32 / 64 / 128
          (1, 4, 4, 2, (2, 2, 2), (1, 1, 1)),        # boxes smaller than one 16-token wave chunk; two wrapping t windows
          (2, 12, 8, 1, (6, 4, 4), (3, 2, 2)),       # S 96 / 48 / 24; two clips
          (1, 8, 6, 1, (4, 3, 2), (2, 1, 1)),        # unequal extents
          (1, 8, 4, 1, (4, 2, 4), (2, 1, 0)))        # shift on t and h only (kernel level: the model class refuses it)


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    T: int
    G: int
    H: int
    window: tuple
    shift: tuple
    family: str = "unit"
    seed: int = 0

    @property
    def N(self):
        return self.G * self.G + 1


def cases():
    out, seed = [], 6000
    for B, T, G, H, w, s in SHAPES:
        for fam in FAMILIES:
            out.append(Case(f"winshift/B{B}T{T}G{G}H{H}/{w[0]}x{w[1]}x{w[2]}/s{s[0]}.{s[1]}.{s[2]}/{fam}", B, T, G, H, w, s, fam,
                            seed))
            seed += 1
    return out


# ------------------------------------------------------------------ the address rule ---------------------------------------
MUTANTS = ("shift_ignored", "wrong_sign", "strips_not_cut", "t_cut_into_strips", "wrap_mod_BT")


def axis_segments(G, w, s):
    """coordinates of the segments of [0, G) cut at 0, s, s + w, ... (s = 0: whole windows)"""
    cuts = ([0] if s else []) + list(range(s, G, w)) + [G]
    return [torch.arange(a, b) for a, b in zip(cuts[:-1], cuts[1:])]


def axis_rolled(G, w, s):
    """whole windows in rolled coordinates: window k holds (k w + s + d) mod G"""
    return [(k * w + s + torch.arange(w)) % G for k in range(G // w)]


def boxes(B, T, G, window, shift, mut: Optional[str] = None):
    """-> list of ((b, kt, jh, jw), rows): the frame-major rows of every box's tokens in (dt, dh, dw) order.  `mut`: one of
    MUTANTS, an addressing defect."""
    wt, wh, ww = clip_window(window, T, G)
    assert T % wt == 0 and G % wh == 0 and G % ww == 0
    st, sh, sw = shift
    if mut == "shift_ignored":
        st = sh = sw = 0
    elif mut == "wrong_sign":
        st, sh, sw = (wt - st) % wt, (wh - sh) % wh, (ww - sw) % ww
    N = G * G + 1
    hs, ws = (axis_rolled if mut == "strips_not_cut" else axis_segments)(G, wh, sh), \
        (axis_rolled if mut == "strips_not_cut" else axis_segments)(G, ww, sw)
    out = []
    for b in range(B):
        if mut == "t_cut_into_strips":
            ts = [b * T + f for f in axis_segments(T, wt, st)]
        elif mut == "wrap_mod_BT":
            ts = [(b * T + f + st) % (B * T) for f in axis_segments(T, wt, 0)]
        else:
            ts = [b * T + f for f in axis_rolled(T, wt, st)]
        for kt, f in enumerate(ts):
            for jh, hh in enumerate(hs):
                for jw, wc in enumerate(ws):
                    rows = f[:, None, None] * N + 1 + hh[None, :, None] * G + wc[None, None, :]
                    out.append(((b, kt, jh, jw), rows.reshape(-1)))
    return out


def box_rows(B, T, G, window, shift, mut: Optional[str] = None) -> List[torch.Tensor]:
    """the boxes grouped by their token count: a list of [n, S] row indices, S ascending, boxes in (b, kt, jh, jw) order"""
    by_S: Dict[int, list] = {}
    for _, rows in boxes(B, T, G, window, shift, mut):
        by_S.setdefault(rows.numel(), []).append(rows)
    return [torch.stack(by_S[S]) for S in sorted(by_S)]


def case_rows(case: Case, mut: Optional[str] = None):
    return box_rows(case.B, case.T, case.G, case.window, case.shift, mut)


# ------------------------------------------------------------------ inputs (CPU, fixed seeds) ------------------------------
def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    """win_attn_cases.make_inputs with the families shaping the logits INSIDE each box (its own S: the sink rows and the late
    maximum sit where the box's tile loop ends)."""
    g = torch.Generator().manual_seed(case.seed)
    B, T, H, N, fam = case.B, case.T, case.H, case.N, case.family
    D, M = H * 64, B * T * N
    full = [torch.randn((M, H, 64), generator=g) for _ in range(4)]
    for idx in case_rows(case):
        n, S = idx.shape
        q, k, v, do = (torch.randn((n, S, H, 64), generator=g) for _ in range(4))
        if fam == "peaked":
            q, k = q * 2.5, k * 2.5
        elif fam == "neg100":
            k = 0.1 * k + 1.0
            q = 0.5 * q
            rows = sink_rows(S)
            q[:, rows] = q[:, rows] - 13.0
        elif fam == "late_max":
            q = 0.5 * q + 1.0
            k = 0.5 * k
            k[:, S - 1] = 2.0
        for f, w in zip(full, (q, k, v, do)):
            f[idx.reshape(-1)] = w.reshape(n * S, H, 64)
    qkv = torch.cat([t.reshape(M, D) for t in full[:3]], dim=1).to(BF16)
    return {"qkv": qkv, "do": full[3].reshape(M, D).to(BF16)}


# ------------------------------------------------------------------ emulation and comparison -------------------------------
@contextlib.contextmanager
def _rows_as(idx):
    """win_attn_cases.emulate takes its sequences from win_attn_cases.window_rows: hand it one group of boxes instead"""
    saved = W.window_rows
    W.window_rows = lambda *a, **k: idx
    try:
        yield
    finally:
        W.window_rows = saved


def emulate(case: Case, inp, mut: Optional[str] = None, own: bool = False):
    """win_attn_cases.emulate (the kernels' arithmetic in float64 with their rounding points) run on the boxes of
    `box_rows(..., mut)` group by group -> frame-major tensors as the kernels write them (untouched rows: 0)"""
    got = None
    for idx in case_rows(case, mut):
        with _rows_as(idx):
            part = W.emulate(case, inp, None, own=own)
        got = part if got is None else {k_: got[k_] + part[k_] for k_ in got}       # disjoint rows, zeros elsewhere
    return got


def expected_groups(case: Case, inp):
    """-> list of (idx, forward dict, backward dict of form a, backward dict of form b), one per group of the TRUE boxes"""
    return [(idx,) + tuple(W.expected(case, inp, idx)) for idx in case_rows(case)]


def compare(case: Case, inp, got, form: str = "a", groups=None) -> Dict[str, float]:
    """worst error / bound of out, lse, dq, dk, dv over the true boxes, given frame-major results"""
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


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
def roll_frames(t, B, T, by):
    """frame-major rows [B T n, C] (or a [B T, H, n] statistic) with the frames of every clip rolled by `by`"""
    if t.dim() == 2:
        return t.reshape(B, T, -1, t.shape[-1]).roll(by, dims=1).reshape(t.shape)
    return t.reshape((B, T) + tuple(t.shape[1:])).roll(by, dims=1).reshape(t.shape)


class Runner:
    def __init__(self, ops, dev):
        self.ops, self.dev = ops, dev

    def launch(self, case: Case, qkv, do, out_in=None, lse_in=None, shift="case", P=None):
        """forward, then the backward on (out_in, lse_in) or on the forward's own results; every result buffer is pre-filled
        with SENTINEL and followed by 64 spare elements.  shift: "case", a triple, or None for the UNSHIFTED entry points."""
        ops, dev = self.ops, self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        P = N if P is None else P
        M, D, BT = B * T * P, case.H * 64, B * T
        shift = case.shift if shift == "case" else shift
        got, bufs = {}, {}

        def new(name, shape, dtype):
            n = math.prod(shape)
            buf = torch.full((n + 64,), SENTINEL, dtype=dtype, device=dev)
            got[name], bufs[name] = buf[:n].view(shape), buf
            return got[name]

        out, lse = new("out", (M, D), BF16), new("lse", (BT, H, P), F32)
        dqkv, delta = new("dqkv", (M, 3 * D), BF16), new("delta", (BT, H, P), F32)
        o_in, l_in = out if out_in is None else out_in, lse if lse_in is None else lse_in
        if shift is None:
            ops.win_attn_fwd(qkv, out, lse, B, T, N, H, case.window, P=P)
            ops.win_attn_bwd(qkv, o_in, do, l_in, delta, dqkv, B, T, N, H, case.window, P=P)
        else:
            ops.win_attn_fwd_shift(qkv, out, lse, B, T, N, H, case.window, shift, P=P)
            ops.win_attn_bwd_shift(qkv, o_in, do, l_in, delta, dqkv, B, T, N, H, case.window, shift, P=P)
        return got, bufs

    def handed(self, case: Case, inp, groups):
        """form (a): bf16 of the float64 out and fp32 of the float64 lse, frame-major (class rows: SENTINEL)"""
        B, T, H, N = case.B, case.T, case.H, case.N
        out = torch.zeros((B * T * N, H * 64), dtype=BF16)
        ls = torch.full((B * T * N, H), SENTINEL, dtype=F32)
        for idx, fw, _, _ in groups:
            o_a, l_a, _, _ = handed_in(fw)
            out += scatter(o_a, idx, B * T * N)
            ls[idx.reshape(-1)] = l_a.permute(0, 2, 1).reshape(-1, H)
        return out, ls.reshape(B * T, N, H).permute(0, 2, 1).contiguous()

    def run_case(self, case: Case):
        dev = self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        BT = B * T
        inp = make_inputs(case)
        groups = expected_groups(case, inp)
        out_a, lse_a = self.handed(case, inp, groups)
        qkv, do = inp["qkv"].to(dev), inp["do"].to(dev)
        got_b, bufs = self.launch(case, qkv, do)
        got_a, _ = self.launch(case, qkv, do, out_a.to(dev), lse_a.to(dev))
        again, _ = self.launch(case, qkv, do)
        torch.cuda.synchronize()
        rec = {"checks": {}, "repeat": {}, "class_intact": {}, "spare_intact": {}, "finite": {}, "hash": {}}
        for name, t in got_b.items():
            rec["repeat"][name] = bool(torch.equal(_bits(t), _bits(again[name])))
            rec["class_intact"][name] = bool((class_rows(t, BT, N) == SENTINEL).all())
            rec["spare_intact"][name] = bool((bufs[name][t.numel():] == SENTINEL).all())
            rec["hash"][name] = _digest(_bits(t))
            patch = t.reshape(BT, N, -1)[:, 1:] if t.dim() == 2 else t[..., 1:]
            rec["finite"][name] = bool(torch.isfinite(patch.float()).all())
        host_b = {k_: t.cpu() for k_, t in got_b.items()}
        for k_, r in compare(case, inp, host_b, "b", groups).items():
            rec["checks"][f"{k_}@b" if k_[0] == "d" else k_] = r
        for k_, r in compare(case, inp, {"dqkv": got_a["dqkv"].cpu()}, "a", groups).items():
            rec["checks"][f"{k_}@a"] = r
        # delta is the fp32 row sum of dO o out of the rows it was given
        prod = do.double().reshape(BT, N, H, 64) * got_b["out"].double().reshape(BT, N, H, 64)
        dl, mag = prod.sum(-1).permute(0, 2, 1)[..., 1:], prod.abs().sum(-1).permute(0, 2, 1)[..., 1:]
        rec["checks"]["delta"] = ratio(got_b["delta"][..., 1:].cpu(), dl.cpu(), (66 * U24 * mag).cpu())
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

    def run_poison(self, case: Case):
        """(a) the rows of box (0, 0, 0, 0) of qkv and dO hold NaN: every other box's results are the bits of a clean run, in
        particular the boxes that share its rolled window (the last h / w segments of the same t window); (b) all of clip 1
        holds NaN: clip 0 keeps its bits.  The class rows of qkv hold NaN in every run."""
        dev = self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        BT = B * T
        inp = make_inputs(case)
        bx = boxes(B, T, case.G, case.window, case.shift)
        nh, nw = 1 + max(k[2] for k, _ in bx), 1 + max(k[3] for k, _ in bx)
        qkv, do = inp["qkv"].clone(), inp["do"].clone()
        qkv[torch.arange(BT) * N] = float("nan")
        clean, _ = self.launch(case, qkv.to(dev), do.to(dev))

        def poisoned(rows):
            bq, bd = qkv.clone(), do.clone()
            bq[rows] = float("nan")
            bd[rows] = float("nan")
            return self.launch(case, bq.to(dev), bd.to(dev))[0]

        target = bx[0][1]
        bad = poisoned(target)
        torch.cuda.synchronize()
        others = torch.cat([r for _, r in bx[1:]]).to(dev)
        mates = [r for k, r in bx[1:] if k[:2] == (0, 0) and k[2] in (0, nh - 1) and k[3] in (0, nw - 1)]
        same, finite = self._same_rows(clean, bad, others, BT, N, H)
        rec = {"independent": same, "finite_with_nan_class_rows": finite, "window_mates": len(mates),
               "window_mates_independent": self._same_rows(clean, bad, torch.cat(mates).to(dev), BT, N, H)[0],
               "poisoned_box_is_nan": bool(torch.isnan(bad["out"][target.to(dev)].float()).all())}
        if B > 1:
            clip1 = torch.cat([r for k, r in bx if k[0] == 1])
            bad1 = poisoned(clip1)
            torch.cuda.synchronize()
            clip0 = torch.cat([r for k, r in bx if k[0] == 0]).to(dev)
            rec["clip0_independent_of_clip1"] = self._same_rows(clean, bad1, clip0, BT, N, H)[0]
        return rec

    def run_stride(self, case: Case, spare: int = 3):
        """the same data stored P = N + spare token rows per frame (NaN in the spare rows of the inputs, SENTINEL in those
        of the results): the bits of the N-row launch in every token row, the spare rows untouched"""
        dev = self.dev
        B, T, N = case.B, case.T, case.N
        BT, P = B * T, case.N + spare
        inp = make_inputs(case)
        base, _ = self.launch(case, inp["qkv"].to(dev), inp["do"].to(dev))

        def wide(t, fill):
            w = torch.full((BT, P, t.shape[-1]), fill, dtype=t.dtype)
            w[:, :N] = t.reshape(BT, N, -1)
            return w.reshape(BT * P, -1).to(dev)

        got, bufs = self.launch(case, wide(inp["qkv"], float("nan")), wide(inp["do"], float("nan")), P=P)
        torch.cuda.synchronize()
        same, spare_ok = True, True
        for name in ("out", "dqkv"):
            v = got[name].reshape(BT, P, -1)
            same &= bool(torch.equal(_bits(v[:, :N].contiguous()), _bits(base[name].reshape(BT, N, -1).contiguous())))
            spare_ok &= bool((v[:, N:] == SENTINEL).all())
        for name in ("lse", "delta"):
            same &= bool(torch.equal(_bits(got[name][..., :N].contiguous()), _bits(base[name].contiguous())))
            spare_ok &= bool((got[name][..., N:] == SENTINEL).all())
        spare_ok &= all(bool((bufs[name][got[name].numel():] == SENTINEL).all()) for name in got)
        return {"identical": same, "spare_rows_intact": spare_ok}

    def run_zero_shift(self, case: Case):
        """shift (0, 0, 0): every result has the bits of the unshifted entry points"""
        inp = make_inputs(case)
        qkv, do = inp["qkv"].to(self.dev), inp["do"].to(self.dev)
        a, _ = self.launch(case, qkv, do, shift=(0, 0, 0))
        b, _ = self.launch(case, qkv, do, shift=None)
        torch.cuda.synchronize()
        return {name: bool(torch.equal(_bits(a[name]), _bits(b[name]))) for name in a}

    def run_t_shift(self, case: Case):
        """shift (st, 0, 0): the bits of the unshifted entry points on buffers whose frames were rolled by -st inside each
        clip, the results rolled back by +st"""
        B, T = case.B, case.T
        st = case.shift[0]
        inp = make_inputs(case)
        qkv, do = inp["qkv"].to(self.dev), inp["do"].to(self.dev)
        a, _ = self.launch(case, qkv, do, shift=(st, 0, 0))
        b, _ = self.launch(case, roll_frames(qkv, B, T, -st).contiguous(), roll_frames(do, B, T, -st).contiguous(), shift=None)
        torch.cuda.synchronize()
        moved = not torch.equal(_bits(a["out"]), _bits(b["out"]))          # the roll is not a no-op on these inputs
        rec = {name: bool(torch.equal(_bits(a[name]), _bits(roll_frames(b[name], B, T, st).contiguous()))) for name in a}
        rec["roll_matters"] = moved
        return rec

    def refusals(self):
        """what aim_win_attn_* refuses, a negative shift, a shift that reaches its clipped extent, a shift on an axis whose
        window spans the grid: an error through aim_last_error and nothing written (the buffers are far too small for
        these shapes: a launch would be out of bounds)"""
        dev, ops, out = self.dev, self.ops, {}
        shapes = {"S over the cap": (1, 17, 257, 1, (17, 16, 16), (0, 0, 0)),
                  "wt does not divide": (1, 6, 17, 1, (4, 2, 2), (1, 1, 1)),
                  "wh does not divide": (1, 4, 17, 1, (2, 3, 2), (1, 1, 1)),
                  "N - 1 not a square": (1, 4, 18, 1, (2, 2, 2), (1, 1, 1)),
                  "negative shift": (1, 4, 17, 1, (2, 2, 2), (1, -1, 1)),
                  "shift reaches the window": (1, 4, 17, 1, (2, 2, 2), (1, 2, 1)),
                  "shift reaches the clipped window": (1, 8, 17, 1, (4, 2, 8), (2, 1, 4)),
                  "t shift on a window that spans the clip": (1, 4, 17, 1, (4, 2, 2), (1, 1, 1)),
                  "w shift on a window that spans the grid": (1, 4, 17, 1, (2, 2, 4), (1, 1, 1))}
        for name, (B, T, N, H, w, s) in shapes.items():
            t16 = torch.full((256,), SENTINEL, dtype=BF16, device=dev)
            o16, d16 = t16.clone(), t16.clone()
            l32, e32 = (torch.full((256,), SENTINEL, dtype=F32, device=dev) for _ in range(2))
            msgs = []
            for f in (lambda: ops.win_attn_fwd_shift(t16, o16, l32, B, T, N, H, w, s),
                      lambda: ops.win_attn_bwd_shift(t16, t16, t16, l32, e32, d16, B, T, N, H, w, s)):
                try:
                    f()
                    msgs.append(None)
                except RuntimeError as e:
                    msgs.append(str(e))
            torch.cuda.synchronize()
            intact = all(bool((t == SENTINEL).all()) for t in (o16, d16, l32, e32))
            out[name] = {"fwd": msgs[0], "bwd": msgs[1], "nothing_written": intact}
        return out


REFUSALS = ("S over the cap", "wt does not divide", "wh does not divide", "N - 1 not a square", "negative shift",
            "shift reaches the window", "shift reaches the clipped window", "t shift on a window that spans the clip",
            "w shift on a window that spans the grid")


def main(argv):
    (path,) = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    dev = torch.device("cuda")
    run = Runner(ops, dev)
    res = {"cases": {}, "poison": {}, "stride": {}, "zero_shift": {}, "t_shift": {}}
    with torch.no_grad():
        res["refusals"] = run.refusals()
        for case in cases():
            res["cases"][case.name] = run.run_case(case)
        for case in cases():
            if case.family != "unit":
                continue
            res["poison"][case.name] = run.run_poison(case)
            res["stride"][case.name] = run.run_stride(case)
            res["zero_shift"][case.name] = run.run_zero_shift(case)
            if case.shift[0]:
                res["t_shift"][case.name] = run.run_t_shift(case)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
