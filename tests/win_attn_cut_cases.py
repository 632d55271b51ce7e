"""Every call form of the cut 3-D window attention kernels (aim_win_attn_fwd_cut / aim_win_attn_bwd_cut, csrc/win_attn.hip),
float64 closed forms per box, and the bounds of win_attn_cases.py with S and nT of each box.

A plain module in the manner of win_attn_shift_cases.py, which it imports and does not change: inputs, emulation, references
and comparison are that module's, run on THIS module's boxes (`_cut_rule` hands them over for the duration of a call, as
win_attn_shift_cases._rows_as does with win_attn_cases).  `test_win_attn_cut_gpu.py` runs `python win_attn_cut_cases.py OUT.json`
once (one child process for the whole list) and `test_win_attn_cut_cases_cpu.py` proves on the CPU that the bounds accept an
emulation of the kernels' arithmetic on the boxes and reject the addressing defects of MUTANTS.

Geometry.  B clips of T frames of N = G G + 1 tokens, a window (wt, wh, ww) clipped to the grid, a shift (st, sh, sw).  EVERY
axis on its own, t included, in ORIGINAL (unrolled) coordinates: [0, extent) is cut at 0, s, s + w, s + 2 w, ..., extent
(s = 0: whole windows).  One box = one (t segment, h segment, w segment); its tokens (dt, dh, dw) in row-major order have the
frame-major rows (b T + t0 + dt) N + 1 + (h0 + dh) G + w0 + dw; no frame index is taken modulo T.

Bounds.  Inside a box the kernels are the unshifted kernels with S -> the box's S, so the bounds are
win_attn_cases.forward_ref / attn_cases.backward_ref evaluated per group of equal S.  No tolerance is introduced here.
"""
import contextlib
import json
import math
import os
import sys
from typing import Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_shift_cases as WS  # noqa: E402
from gemm_cases import U24, _digest, ratio  # noqa: E402,F401
from win_attn_cases import BF16, F32, FAMILIES, _bits, clip_window  # noqa: E402
from win_attn_shift_cases import Case, axis_rolled, axis_segments  # noqa: E402

NAN = float("nan")
# B, T, G, H, window, shift
SHAPES = ((2, 4, 4, 2, (2, 2, 2), (1, 1, 1)),        # boxes of 1 ... 8 tokens: smaller than one 16-token wave chunk
          (2, 8, 6, 2, (4, 3, 3), (2, 1, 1)),        # boxes of 2 ... 36 tokens
          (2, 16, 6, 2, (8, 6, 6), (4, 0, 0)),       # t cut alone: 144 / 288 / 144 tokens, several 64-key tiles with tails of 16
                                                     # and 32, more than one chunk of own tokens
          (2, 8, 8, 2, (4, 4, 2), (2, 2, 1)))        # unequal h and w shifts (the swapped-shift defect is visible here)


def cases():
    out, seed = [], 7000
    for B, T, G, H, w, s in SHAPES:
        for fam in FAMILIES:
            out.append(Case(f"wincut/B{B}T{T}G{G}H{H}/{w[0]}x{w[1]}x{w[2]}/s{s[0]}.{s[1]}.{s[2]}/{fam}", B, T, G, H, w, s, fam, seed))
            seed += 1
    return out


# ------------------------------------------------------------------ the address rule ---------------------------------------
MUTANTS = ("shift_ignored", "t_wraps", "t_not_cut", "cut_at_s_plus_1", "cut_at_s_minus_1", "hw_shifts_swapped")


def boxes(B, T, G, window, shift, mut: Optional[str] = None):
    """-> list of ((b, jt, jh, jw), rows): the frame-major rows of every box's tokens in (dt, dh, dw) order.  `mut`: one of
    MUTANTS, an addressing defect."""
    wt, wh, ww = clip_window(window, T, G)
    assert T % wt == 0 and G % wh == 0 and G % ww == 0
    st, sh, sw = shift
    if mut == "shift_ignored":
        st = sh = sw = 0
    elif mut == "cut_at_s_plus_1":
        st, sh, sw = (s + 1 if s else 0 for s in (st, sh, sw))
    elif mut == "cut_at_s_minus_1":
        st, sh, sw = (s - 1 if s else 0 for s in (st, sh, sw))
    elif mut == "hw_shifts_swapped":
        sh, sw = sw, sh
    N = G * G + 1
    if mut == "t_wraps":            # whole t windows that start at st and wrap round the clip's end: the *_shift entries' rule
        tsegs = axis_rolled(T, wt, st)
    elif mut == "t_not_cut":        # h and w cut, t left in plain windows
        tsegs = axis_segments(T, wt, 0)
    else:
        tsegs = axis_segments(T, wt, st)
    out = []
    for b in range(B):
        for jt, f in enumerate(tsegs):
            for jh, hh in enumerate(axis_segments(G, wh, sh)):
                for jw, wc in enumerate(axis_segments(G, ww, sw)):
                    rows = (b * T + f)[:, None, None] * N + 1 + hh[None, :, None] * G + wc[None, None, :]
                    out.append(((b, jt, jh, jw), rows.reshape(-1)))
    return out


@contextlib.contextmanager
def _cut_rule():
    """win_attn_shift_cases takes its sequences from its own `boxes`: hand it this module's for the duration of a call"""
    saved = WS.boxes
    WS.boxes = boxes
    try:
        yield
    finally:
        WS.boxes = saved


def _with_cut_rule(f):
    def g(*a, **k):
        with _cut_rule():
            return f(*a, **k)
    g.__doc__ = f"win_attn_shift_cases.{f.__name__} on the boxes of this module"
    return g


box_rows, case_rows, make_inputs, emulate = (_with_cut_rule(f) for f in (WS.box_rows, WS.case_rows, WS.make_inputs, WS.emulate))
expected_groups, compare = _with_cut_rule(WS.expected_groups), _with_cut_rule(WS.compare)


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
class Runner(WS.Runner):
    """win_attn_shift_cases.Runner with the *_cut entry points and every result buffer pre-filled with NaN: a row that must not
    be written (class rows, spare rows behind a frame's tokens, the 64 elements behind a buffer) still holds NaN afterwards"""

    def launch(self, case: Case, qkv, do, out_in=None, lse_in=None, shift="case", P=None, entry="cut"):
        """entry: "cut", "shift" (aim_win_attn_*_shift) or "plain" (aim_win_attn_fwd / _bwd, no shift argument)"""
        ops, dev = self.ops, self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        P = N if P is None else P
        M, D, BT = B * T * P, H * 64, B * T
        shift = case.shift if shift == "case" else shift
        got, bufs = {}, {}

        def new(name, shape, dtype):
            n = math.prod(shape)
            buf = torch.full((n + 64,), NAN, dtype=dtype, device=dev)
            got[name], bufs[name] = buf[:n].view(shape), buf
            return got[name]

        out, lse = new("out", (M, D), BF16), new("lse", (BT, H, P), F32)
        dqkv, delta = new("dqkv", (M, 3 * D), BF16), new("delta", (BT, H, P), F32)
        o_in, l_in = out if out_in is None else out_in, lse if lse_in is None else lse_in
        if entry == "plain":
            ops.win_attn_fwd(qkv, out, lse, B, T, N, H, case.window, P=P)
            ops.win_attn_bwd(qkv, o_in, do, l_in, delta, dqkv, B, T, N, H, case.window, P=P)
        else:
            fwd, bwd = (ops.win_attn_fwd_cut, ops.win_attn_bwd_cut) if entry == "cut" else (ops.win_attn_fwd_shift, ops.win_attn_bwd_shift)
            fwd(qkv, out, lse, B, T, N, H, case.window, shift, P=P)
            bwd(qkv, o_in, do, l_in, delta, dqkv, B, T, N, H, case.window, shift, P=P)
        return got, bufs

    @staticmethod
    def _untouched(got, bufs, BT, N, P):
        """are the class rows, the spare rows of every frame and the elements behind each buffer still NaN"""
        ok = True
        for name, t in got.items():
            v = t.reshape(BT, P, -1) if t.dim() == 2 else t.permute(0, 2, 1)          # [BT, P, C]
            ok &= bool(torch.isnan(v[:, 0].float()).all()) and bool(torch.isnan(v[:, N:].float()).all())
            ok &= bool(torch.isnan(bufs[name][t.numel():].float()).all())
        return ok

    @staticmethod
    def _narrow(got, BT, N, P):
        """the N token rows of every frame of results stored P rows per frame"""
        out = {}
        for name, t in got.items():
            out[name] = (t.reshape(BT, P, -1)[:, :N].reshape(BT * N, -1) if t.dim() == 2 else t[..., :N]).contiguous()
        return out

    def run_case(self, case: Case):
        """forward and backward against the fp64 bounds, at P = N and at P = N + 1 (NaN in the spare rows of the inputs)"""
        dev = self.dev
        B, T, H, N = case.B, case.T, case.H, case.N
        BT = B * T
        inp = make_inputs(case)
        groups = expected_groups(case, inp)
        out_a, lse_a = self.handed(case, inp, groups)
        rec = {"checks": {}, "repeat": {}, "untouched": {}, "finite": {}, "hash": {}}
        for P in (N, N + 1):
            def wide(t, fill=NAN):
                if t.dim() == 3:                                    # a [BT, H, N] statistic
                    w = torch.full((BT, H, P), fill, dtype=t.dtype)
                    w[..., :N] = t
                    return w.to(dev)
                w = torch.full((BT, P, t.shape[-1]), fill, dtype=t.dtype)
                w[:, :N] = t.reshape(BT, N, -1)
                return w.reshape(BT * P, -1).to(dev)

            tag = "N" if P == N else "N+1"
            qkv, do = wide(inp["qkv"]), wide(inp["do"])
            got_b, bufs_b = self.launch(case, qkv, do, P=P)
            got_a, bufs_a = self.launch(case, qkv, do, wide(out_a), wide(lse_a), P=P)
            again, _ = self.launch(case, qkv, do, P=P)
            torch.cuda.synchronize()
            rec["untouched"][tag] = self._untouched(got_b, bufs_b, BT, N, P) and self._untouched(got_a, bufs_a, BT, N, P)
            nb, na, ng = self._narrow(got_b, BT, N, P), self._narrow(got_a, BT, N, P), self._narrow(again, BT, N, P)
            rec["repeat"][tag] = all(bool(torch.equal(_bits(nb[k][..., 1:] if nb[k].dim() == 3 else nb[k].reshape(BT, N, -1)[:, 1:]),
                                                      _bits(ng[k][..., 1:] if ng[k].dim() == 3 else ng[k].reshape(BT, N, -1)[:, 1:])))
                                     for k in nb)
            rec["finite"][tag] = all(bool(torch.isfinite((t.reshape(BT, N, -1)[:, 1:] if t.dim() == 2 else t[..., 1:]).float()).all())
                                     for t in nb.values())
            rec["hash"][tag] = {k: _digest(_bits((t.reshape(BT, N, -1)[:, 1:] if t.dim() == 2 else t[..., 1:]).contiguous()))
                                for k, t in nb.items()}
            host_b = {k_: t.cpu() for k_, t in nb.items()}
            for k_, r in compare(case, inp, host_b, "b", groups).items():
                rec["checks"][f"{k_}@b/{tag}" if k_[0] == "d" else f"{k_}/{tag}"] = r
            for k_, r in compare(case, inp, {"dqkv": na["dqkv"].cpu()}, "a", groups).items():
                rec["checks"][f"{k_}@a/{tag}"] = r
            # delta is the fp32 row sum of dO o out of the rows it was given
            prod = inp["do"].double().reshape(BT, N, H, 64) * host_b["out"].double().reshape(BT, N, H, 64)
            dl, mag = prod.sum(-1).permute(0, 2, 1)[..., 1:], prod.abs().sum(-1).permute(0, 2, 1)[..., 1:]
            rec["checks"][f"delta/{tag}"] = ratio(host_b["delta"][..., 1:], dl, 66 * U24 * mag)
        rec["same_bits_at_both_strides"] = rec["hash"]["N"] == rec["hash"]["N+1"]
        return rec

    def _equal_patch_rows(self, a, b, case):
        BT, N = case.B * case.T, case.N
        f = lambda t: _bits((t.reshape(BT, N, -1)[:, 1:] if t.dim() == 2 else t[..., 1:]).contiguous())
        return {name: bool(torch.equal(f(a[name]), f(b[name]))) for name in a}

    def run_bit_identity(self, case: Case):
        """st = 0: the bits of the *_shift entries at the same (sh, sw); all-zero shift: the bits of the unshifted entries"""
        inp = make_inputs(case)
        qkv, do = inp["qkv"].to(self.dev), inp["do"].to(self.dev)
        s0 = (0,) + tuple(case.shift[1:])
        cut0, _ = self.launch(case, qkv, do, shift=s0, entry="cut")
        shf0, _ = self.launch(case, qkv, do, shift=s0, entry="shift")
        zero, _ = self.launch(case, qkv, do, shift=(0, 0, 0), entry="cut")
        plain, _ = self.launch(case, qkv, do, entry="plain")
        full, _ = self.launch(case, qkv, do, entry="cut")
        torch.cuda.synchronize()
        rec = {"st0_vs_shift": self._equal_patch_rows(cut0, shf0, case), "zero_vs_plain": self._equal_patch_rows(zero, plain, case)}
        if case.shift[0]:          # the t cut is live: it moves the output against st = 0
            rec["t_cut_matters"] = not all(self._equal_patch_rows(full, cut0, case).values())
        return rec

    def refusals(self):
        """what the *_shift entries refuse, one by one: an error through aim_last_error and nothing written (the buffers are far
        too small for these shapes: a launch would be out of bounds)"""
        dev, ops, out = self.dev, self.ops, {}
        for name, (B, T, N, H, w, s) in REFUSAL_SHAPES.items():
            t16 = torch.full((256,), NAN, dtype=BF16, device=dev)
            o16, d16 = t16.clone(), t16.clone()
            l32, e32 = (torch.full((256,), NAN, dtype=F32, device=dev) for _ in range(2))
            msgs = []
            for f in (lambda: ops.win_attn_fwd_cut(t16, o16, l32, B, T, N, H, w, s),
                      lambda: ops.win_attn_bwd_cut(t16, t16, t16, l32, e32, d16, B, T, N, H, w, s)):
                try:
                    f()
                    msgs.append(None)
                except RuntimeError as e:
                    msgs.append(str(e))
            torch.cuda.synchronize()
            intact = all(bool(torch.isnan(t.float()).all()) for t in (o16, d16, l32, e32))
            out[name] = {"fwd": msgs[0], "bwd": msgs[1], "nothing_written": intact}
        return out


REFUSAL_SHAPES = {"S over the cap": (1, 17, 257, 1, (17, 16, 16), (0, 0, 0)),
                  "wt does not divide": (1, 6, 17, 1, (4, 2, 2), (1, 1, 1)),
                  "wh does not divide": (1, 4, 17, 1, (2, 3, 2), (1, 1, 1)),
                  "ww does not divide": (1, 4, 17, 1, (2, 2, 3), (1, 1, 1)),
                  "N - 1 not a square": (1, 4, 18, 1, (2, 2, 2), (1, 1, 1)),
                  "negative t shift": (1, 4, 17, 1, (2, 2, 2), (-1, 1, 1)),
                  "negative h shift": (1, 4, 17, 1, (2, 2, 2), (1, -1, 1)),
                  "t shift reaches the window": (1, 4, 17, 1, (2, 2, 2), (2, 1, 1)),
                  "shift reaches the clipped window": (1, 8, 17, 1, (4, 2, 8), (2, 1, 4)),
                  "t shift on a window that spans the clip": (1, 4, 17, 1, (4, 2, 2), (1, 1, 1)),
                  "w shift on a window that spans the grid": (1, 4, 17, 1, (2, 2, 4), (1, 1, 1))}
REFUSALS = tuple(REFUSAL_SHAPES)


def main(argv):
    (path,) = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    dev = torch.device("cuda")
    run = Runner(ops, dev)
    res = {"cases": {}, "bits": {}}
    with torch.no_grad():
        res["refusals"] = run.refusals()
        for case in cases():
            res["cases"][case.name] = run.run_case(case)
            for k, r in res["cases"][case.name]["checks"].items():
                print(f"{case.name} {k}: {r:.3f}", flush=True)
        for case in cases():
            if case.family == "unit":
                res["bits"][case.name] = run.run_bit_identity(case)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
