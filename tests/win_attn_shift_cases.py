"""Every call form of the shifted 3-D window attention kernels (aim_win_attn_fwd_shift / aim_win_attn_bwd_shift,
csrc/win_attn.hip), float64 closed forms per box, and the bounds of win_attn_cases.py with S and nT of each box.

A table in the manner of win_attn_cases.py, whose references, bounds, emulation core, comparison and runner it calls with its
own sequences as arguments: the boxes of `boxes`, grouped by size.  `boxes` is the address rule of win_attn_cut_cases.py too:
how the t axis is treated is its `t_axis` argument, which a Case carries.  `test_win_attn_shift_gpu.py` runs
`python win_attn_shift_cases.py OUT.json` once (one child process for the whole list) and `test_win_attn_shift_cases_cpu.py`
proves on the CPU that the bounds accept an emulation of the kernels' arithmetic on the boxes and reject the addressing
defects of MUTANTS.

Geometry.  B clips of T frames of N = G G + 1 tokens, a window (wt, wh, ww) clipped to the grid, a shift (st, sh, sw).  Each
axis on its own, in ORIGINAL (unrolled) coordinates:
  h (w alike), sh > 0: [0, G) is cut at 0, sh, sh + wh, sh + 2 wh, ..., G;  sh = 0: whole windows          (`axis_segments`)
  t: window k holds the frames (k wt + st + dt) mod T of its own clip                                      (`axis_rolled`)
One box = one (t window, h segment, w segment); its tokens (dt, dh, dw) in row-major order have the frame-major rows
    (b T + (k wt + st + dt) mod T) N + 1 + (h0 + dh) G + w0 + dw                                   (`box_rows`)
One item = one (box, head): q, k, v [S, 64] with S = wt eh ew, which differs from box to box; `box_rows` returns the boxes
grouped by S so that each group is a dense [n, S] index like win_attn_cases.window_rows.

Bounds.  Inside a box the kernels are the unshifted kernels with S -> the box's S (the tile loop runs to the box's own S,
the rounding points do not move), so the bounds are win_attn_cases.forward_ref / attn_cases.backward_ref evaluated per
group.  No tolerance is introduced here.
"""
import json
import os
import sys
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cases as W  # noqa: E402
from win_attn_cases import FAMILIES, NAN, _bits, clip_window  # noqa: E402

# B, T, G, H, window, shift
SHAPES = ((1, 32, 14, 2, (16, 7, 7), (8, 3, 3)),     # the hmdb51 form: S 144 ... 784, tails 16 and 0 mod 64
          (1, 32, 14, 1, (32, 2, 2), (0, 1, 1)),     # the diving48 / ucf101 form: 64 boxes, S 32 / 64 / 128
          (1, 4, 4, 2, (2, 2, 2), (1, 1, 1)),        # boxes smaller than one 16-token wave chunk; two wrapping t windows
          (2, 12, 8, 1, (6, 4, 4), (3, 2, 2)),       # S 96 / 48 / 24; two clips
          (1, 8, 6, 1, (4, 3, 2), (2, 1, 1)),        # unequal extents
          (1, 8, 4, 1, (4, 2, 4), (2, 1, 0)))        # shift on t and h only (kernel level: the model class refuses it)


# ------------------------------------------------------------------ the address rule ---------------------------------------
MUTANTS = ("shift_ignored", "wrong_sign", "strips_not_cut", "t_cut_into_strips", "wrap_mod_BT")


def axis_segments(G, w, s):
    """coordinates of the segments of [0, G) cut at 0, s, s + w, ... (s = 0: whole windows)"""
    cuts = ([0] if s else []) + list(range(s, G, w)) + [G]
    return [torch.arange(a, b) for a, b in zip(cuts[:-1], cuts[1:])]


def axis_rolled(G, w, s):
    """whole windows in rolled coordinates: window k holds (k w + s + d) mod G"""
    return [(k * w + s + torch.arange(w)) % G for k in range(G // w)]


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
    t_axis: Callable = axis_rolled          # the *_shift entries; axis_segments: the *_cut entries

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


def boxes(B, T, G, window, shift, mut: Optional[str] = None, t_axis=axis_rolled):
    """-> list of ((b, kt, jh, jw), rows): the frame-major rows of every box's tokens in (dt, dh, dw) order.  h and w are cut
    into segments; t_axis: axis_rolled (whole t windows that start at st and wrap round the clip's end, the *_shift entries)
    or axis_segments (t cut like h and w, the *_cut entries).  `mut`: an addressing defect, one of this module's MUTANTS or
    of win_attn_cut_cases.MUTANTS."""
    wt, wh, ww = clip_window(window, T, G)
    assert T % wt == 0 and G % wh == 0 and G % ww == 0
    st, sh, sw = shift
    hw_axis, wrap = axis_segments, 0
    if mut == "shift_ignored":
        st = sh = sw = 0
    elif mut == "wrong_sign":
        st, sh, sw = (wt - st) % wt, (wh - sh) % wh, (ww - sw) % ww
    elif mut == "cut_at_s_plus_1":
        st, sh, sw = (s + 1 if s else 0 for s in (st, sh, sw))
    elif mut == "cut_at_s_minus_1":
        st, sh, sw = (s - 1 if s else 0 for s in (st, sh, sw))
    elif mut == "hw_shifts_swapped":
        sh, sw = sw, sh
    elif mut == "strips_not_cut":           # h and w in whole rolled windows
        hw_axis = axis_rolled
    elif mut == "t_cut_into_strips":        # the *_cut entries' rule where the *_shift entries' is due
        t_axis = axis_segments
    elif mut == "t_wraps":                  # the *_shift entries' rule where the *_cut entries' is due
        t_axis = axis_rolled
    elif mut == "t_not_cut":                # h and w cut, t left in plain windows
        t_axis, st = axis_segments, 0
    elif mut == "wrap_mod_BT":              # plain t windows moved by st and wrapped round the end of the BATCH
        t_axis, st, wrap = axis_segments, 0, st
    N = G * G + 1
    out = []
    for b in range(B):
        for kt, f in enumerate(t_axis(T, wt, st)):
            f = (b * T + f + wrap) % (B * T) if wrap else b * T + f
            for jh, hh in enumerate(hw_axis(G, wh, sh)):
                for jw, wc in enumerate(hw_axis(G, ww, sw)):
                    rows = f[:, None, None] * N + 1 + hh[None, :, None] * G + wc[None, None, :]
                    out.append(((b, kt, jh, jw), rows.reshape(-1)))
    return out


def box_rows(B, T, G, window, shift, mut: Optional[str] = None, t_axis=axis_rolled) -> List[torch.Tensor]:
    """the boxes grouped by their token count: a list of [n, S] row indices, S ascending, boxes in (b, kt, jh, jw) order"""
    by_S: Dict[int, list] = {}
    for _, rows in boxes(B, T, G, window, shift, mut, t_axis):
        by_S.setdefault(rows.numel(), []).append(rows)
    return [torch.stack(by_S[S]) for S in sorted(by_S)]


def case_rows(case: Case, mut: Optional[str] = None):
    return box_rows(case.B, case.T, case.G, case.window, case.shift, mut, case.t_axis)


# ------------------------------------------------------------------ inputs, emulation and comparison -----------------------
def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    """qkv [B T N, 3 D] and dO [B T N, D] as bf16, frame-major: the background, then the boxes group by group"""
    g = torch.Generator().manual_seed(case.seed)
    full = W.background(g, case.B * case.T * case.N, case.H)
    return W.assemble(full, [W.draw_group(g, idx, case.H, case.family) for idx in case_rows(case)], case.H)


def emulate(case: Case, inp, mut: Optional[str] = None, own: bool = False):
    """win_attn_cases.emulate_rows (the kernels' arithmetic in float64 with their rounding points) on the boxes of
    `case_rows(case, mut)` group by group -> frame-major tensors as the kernels write them (untouched rows: 0)"""
    got = None
    for idx in case_rows(case, mut):
        part = W.emulate_rows(idx, inp, case.B * case.T, case.N, case.H, None, own)
        got = part if got is None else {k_: got[k_] + part[k_] for k_ in got}       # disjoint rows, zeros elsewhere
    return got


def expected_groups(case: Case, inp):
    """-> list of (idx, forward dict, backward dict of form a, backward dict of form b), one per group of the TRUE boxes"""
    return [(idx,) + tuple(W.expected(case, inp, idx)) for idx in case_rows(case)]


def compare(case: Case, inp, got, form: str = "a", groups=None) -> Dict[str, float]:
    """worst error / bound of out, lse, dq, dk, dv over the true boxes, given frame-major results"""
    return W.compare(case, inp, got, form, expected_groups(case, inp) if groups is None else groups)


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
def roll_frames(t, B, T, by):
    """frame-major rows [B T n, C] (or a [B T, H, n] statistic) with the frames of every clip rolled by `by`"""
    if t.dim() == 2:
        return t.reshape(B, T, -1, t.shape[-1]).roll(by, dims=1).reshape(t.shape)
    return t.reshape((B, T) + tuple(t.shape[1:])).roll(by, dims=1).reshape(t.shape)


class Runner(W.Runner):
    entry = "shift"

    def run_poison(self, case: Case, inp):
        """(a) the rows of box (0, 0, 0, 0) of qkv and dO hold NaN: every other box's results are the bits of a clean run, in
        particular the boxes that share its rolled window (the last h / w segments of the same t window); (b) all of clip 1
        holds NaN: clip 0 keeps its bits.  The class rows of qkv hold NaN in every run."""
        dev = self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        BT = B * T
        bx = boxes(B, T, case.G, case.window, case.shift, None, case.t_axis)
        nh, nw = 1 + max(k[2] for k, _ in bx), 1 + max(k[3] for k, _ in bx)
        qkv, do = inp["qkv"].clone(), inp["do"].clone()
        qkv[torch.arange(BT) * N] = NAN
        clean, _ = self.launch(case, qkv.to(dev), do.to(dev))

        def poisoned(rows):
            bq, bd = qkv.clone(), do.clone()
            bq[rows] = NAN
            bd[rows] = NAN
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

    def run_zero_shift(self, case: Case, inp):
        """shift (0, 0, 0): every result has the bits of the unshifted entry points"""
        qkv, do = inp["qkv"].to(self.dev), inp["do"].to(self.dev)
        a, _ = self.launch(case, qkv, do, shift=(0, 0, 0))
        b, _ = self.launch(case, qkv, do, entry="plain")
        torch.cuda.synchronize()
        return {name: bool(torch.equal(_bits(a[name]), _bits(b[name]))) for name in a}

    def run_t_shift(self, case: Case, inp):
        """shift (st, 0, 0): the bits of the unshifted entry points on buffers whose frames were rolled by -st inside each
        clip, the results rolled back by +st"""
        B, T = case.B, case.T
        st = case.shift[0]
        qkv, do = inp["qkv"].to(self.dev), inp["do"].to(self.dev)
        a, _ = self.launch(case, qkv, do, shift=(st, 0, 0))
        b, _ = self.launch(case, roll_frames(qkv, B, T, -st).contiguous(), roll_frames(do, B, T, -st).contiguous(), entry="plain")
        torch.cuda.synchronize()
        moved = not torch.equal(_bits(a["out"]), _bits(b["out"]))          # the roll is not a no-op on these inputs
        rec = {name: bool(torch.equal(_bits(a[name]), _bits(roll_frames(b[name], B, T, st).contiguous()))) for name in a}
        rec["roll_matters"] = moved
        return rec


# what aim_win_attn_* refuses, a negative shift, a shift that reaches its clipped extent, a shift on an axis whose window
# spans the grid
REFUSAL_SHAPES = {"S over the cap": (1, 17, 257, 1, (17, 16, 16), (0, 0, 0)),
                  "wt does not divide": (1, 6, 17, 1, (4, 2, 2), (1, 1, 1)),
                  "wh does not divide": (1, 4, 17, 1, (2, 3, 2), (1, 1, 1)),
                  "N - 1 not a square": (1, 4, 18, 1, (2, 2, 2), (1, 1, 1)),
                  "negative shift": (1, 4, 17, 1, (2, 2, 2), (1, -1, 1)),
                  "shift reaches the window": (1, 4, 17, 1, (2, 2, 2), (1, 2, 1)),
                  "shift reaches the clipped window": (1, 8, 17, 1, (4, 2, 8), (2, 1, 4)),
                  "t shift on a window that spans the clip": (1, 4, 17, 1, (4, 2, 2), (1, 1, 1)),
                  "w shift on a window that spans the grid": (1, 4, 17, 1, (2, 2, 4), (1, 1, 1))}
REFUSALS = tuple(REFUSAL_SHAPES)


def main(argv):
    (path,) = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    run = Runner(ops, torch.device("cuda"))
    res = {"cases": {}, "poison": {}, "stride": {}, "zero_shift": {}, "t_shift": {}}
    with torch.no_grad():
        res["refusals"] = run.refusals(REFUSAL_SHAPES)
        for case in cases():
            inp = make_inputs(case)
            res["cases"][case.name] = run.run_case(case, inp, expected_groups(case, inp))
        for case in cases():
            if case.family != "unit":
                continue
            inp = make_inputs(case)
            res["poison"][case.name] = run.run_poison(case, inp)
            res["stride"][case.name] = run.run_stride(case, inp)
            res["zero_shift"][case.name] = run.run_zero_shift(case, inp)
            if case.shift[0]:
                res["t_shift"][case.name] = run.run_t_shift(case, inp)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
