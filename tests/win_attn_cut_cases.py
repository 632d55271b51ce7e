"""Every call form of the cut 3-D window attention kernels (aim_win_attn_fwd_cut / aim_win_attn_bwd_cut, csrc/win_attn.hip),
float64 closed forms per box, and the bounds of win_attn_cases.py with S and nT of each box.

A table in the manner of win_attn_shift_cases.py.  Its cases carry `t_axis=axis_segments`, and that module's `boxes`, inputs,
emulation, references and comparison take the rule from the case they are given (or from their `t_axis` argument), so they
ARE this table's; only the runs on the GPU are its own.  `test_win_attn_cut_gpu.py` runs `python win_attn_cut_cases.py OUT.json`
once (one child process for the whole list) and `test_win_attn_cut_cases_cpu.py` proves on the CPU that the bounds accept an
emulation of the kernels' arithmetic on the boxes and reject the addressing defects of MUTANTS.

Geometry.  B clips of T frames of N = G G + 1 tokens, a window (wt, wh, ww) clipped to the grid, a shift (st, sh, sw).  EVERY
axis on its own, t included, in ORIGINAL (unrolled) coordinates: [0, extent) is cut at 0, s, s + w, s + 2 w, ..., extent
(s = 0: whole windows).  One box = one (t segment, h segment, w segment); its tokens (dt, dh, dw) in row-major order have the
frame-major rows (b T + t0 + dt) N + 1 + (h0 + dh) G + w0 + dw; no frame index is taken modulo T.

Bounds.  Inside a box the kernels are the unshifted kernels with S -> the box's S, so the bounds are
win_attn_cases.forward_ref / attn_cases.backward_ref evaluated per group of equal S.  No tolerance is introduced here.
"""
import functools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cases as W  # noqa: E402
import win_attn_shift_cases as WS  # noqa: E402
from gemm_cases import _digest  # noqa: E402
from win_attn_cases import FAMILIES, NAN, _bits, patch_rows  # noqa: E402
from win_attn_shift_cases import Case, axis_segments, case_rows, compare, emulate, expected_groups, make_inputs  # noqa: E402,F401

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
            out.append(Case(f"wincut/B{B}T{T}G{G}H{H}/{w[0]}x{w[1]}x{w[2]}/s{s[0]}.{s[1]}.{s[2]}/{fam}", B, T, G, H, w, s, fam, seed,
                            t_axis=axis_segments))
            seed += 1
    return out


# ------------------------------------------------------------------ the address rule ---------------------------------------
MUTANTS = ("shift_ignored", "t_wraps", "t_not_cut", "cut_at_s_plus_1", "cut_at_s_minus_1", "hw_shifts_swapped")
# boxes(B, T, G, window, shift[, mut]) -> list of ((b, jt, jh, jw), rows), and the same grouped by token count
boxes = functools.partial(WS.boxes, t_axis=axis_segments)
box_rows = functools.partial(WS.box_rows, t_axis=axis_segments)


# ------------------------------------------------------------------ the GPU run (one child process) ------------------------
def equal_patch_rows(a, b, BT, N):
    return {name: bool(torch.equal(_bits(patch_rows(a[name], BT, N).contiguous()), _bits(patch_rows(b[name], BT, N).contiguous())))
            for name in a}


class Runner(W.Runner):
    """the *_cut entry points with every result buffer pre-filled with NaN: a row that must not be written (class rows, spare
    rows behind a frame's tokens, the 64 elements behind a buffer) still holds NaN afterwards"""
    entry, fill = "cut", NAN

    def run_case(self, case: Case, inp, groups):
        """forward and backward against the fp64 bounds, at P = N and at P = N + 1 (NaN in the spare rows of the inputs)"""
        dev = self.dev
        BT, H, N = case.B * case.T, case.H, case.N
        out_a, lse_a = self.handed(case, groups)
        rec = {"checks": {}, "repeat": {}, "untouched": {}, "finite": {}, "hash": {}}
        for P in (N, N + 1):
            tag = "N" if P == N else "N+1"
            qkv, do, o_in, l_in = (W.wide(t, BT, N, P).to(dev) for t in (inp["qkv"], inp["do"], out_a, lse_a))
            got_b, bufs_b = self.launch(case, qkv, do, P=P)
            got_a, bufs_a = self.launch(case, qkv, do, o_in, l_in, P=P)
            again, _ = self.launch(case, qkv, do, P=P)
            torch.cuda.synchronize()
            rec["untouched"][tag] = W.untouched(got_b, bufs_b, BT, N, P, NAN) and W.untouched(got_a, bufs_a, BT, N, P, NAN)
            nb, na, ng = (W.narrow(got, BT, N, P) for got in (got_b, got_a, again))
            rec["repeat"][tag] = all(equal_patch_rows(nb, ng, BT, N).values())
            rec["finite"][tag] = all(bool(torch.isfinite(patch_rows(t, BT, N).float()).all()) for t in nb.values())
            rec["hash"][tag] = {k: _digest(_bits(patch_rows(t, BT, N).contiguous())) for k, t in nb.items()}
            host_b = {k_: t.cpu() for k_, t in nb.items()}
            for k_, r in compare(case, inp, host_b, "b", groups).items():
                rec["checks"][f"{k_}@b/{tag}" if k_[0] == "d" else f"{k_}/{tag}"] = r
            for k_, r in compare(case, inp, {"dqkv": na["dqkv"].cpu()}, "a", groups).items():
                rec["checks"][f"{k_}@a/{tag}"] = r
            rec["checks"][f"delta/{tag}"] = W.delta_ratio(inp["do"], host_b["out"], host_b["delta"], BT, N, H)
        rec["same_bits_at_both_strides"] = rec["hash"]["N"] == rec["hash"]["N+1"]
        return rec

    def run_bit_identity(self, case: Case, inp):
        """st = 0: the bits of the *_shift entries at the same (sh, sw); all-zero shift: the bits of the unshifted entries"""
        BT, N = case.B * case.T, case.N
        qkv, do = inp["qkv"].to(self.dev), inp["do"].to(self.dev)
        s0 = (0,) + tuple(case.shift[1:])
        cut0, _ = self.launch(case, qkv, do, shift=s0)
        shf0, _ = self.launch(case, qkv, do, shift=s0, entry="shift")
        zero, _ = self.launch(case, qkv, do, shift=(0, 0, 0))
        plain, _ = self.launch(case, qkv, do, entry="plain")
        full, _ = self.launch(case, qkv, do)
        torch.cuda.synchronize()
        rec = {"st0_vs_shift": equal_patch_rows(cut0, shf0, BT, N), "zero_vs_plain": equal_patch_rows(zero, plain, BT, N)}
        if case.shift[0]:          # the t cut is live: it moves the output against st = 0
            rec["t_cut_matters"] = not all(equal_patch_rows(full, cut0, BT, N).values())
        return rec


# what the *_shift entries refuse, one by one
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
    run = Runner(ops, torch.device("cuda"))
    res = {"cases": {}, "bits": {}}
    with torch.no_grad():
        res["refusals"] = run.refusals(REFUSAL_SHAPES)
        for case in cases():
            inp = make_inputs(case)
            res["cases"][case.name] = run.run_case(case, inp, expected_groups(case, inp))
            for k, r in res["cases"][case.name]["checks"].items():
                print(f"{case.name} {k}: {r:.3f}", flush=True)
        for case in cases():
            if case.family == "unit":
                res["bits"][case.name] = run.run_bit_identity(case, make_inputs(case))
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
