"""Cases and the child process of tests/test_attn_shift_gpu.py: the head-shifted attention kernels against the unshifted
ones on a rolled copy of K and V, bit for bit.

aim_attn_fwd_shift / aim_attn_bwd_shift change where an item's K and V are read (and dK, dV written), nothing else, so there
is no tolerance here: with `qkv_rolled` = qkv whose K and V column blocks of head h are rolled by shifts[h] along the frames of
every clip (torch.roll, out[t] = in[t - s]),
    fwd_shift(qkv)                == fwd(qkv_rolled)                        in out and lse
    bwd_shift(qkv, out, dO, lse)  == bwd(qkv_rolled, out, dO, lse)          in dQ; in dK, dV after rolling them back
on every route of the backward (attn_cases.ROUTES; one child process per route, the switches are read once per process).
The numerics of the unshifted kernels are held to float64 by tests/test_attn_routes_gpu.py.

A child runs one route: python attn_shift_cases.py <route> <result.json>."""
import json
import os
import sys
from dataclasses import dataclass
from typing import Tuple

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_cases import BF16, F32, ROUTE_ENV, ROUTE_VARS, ROUTES, _flat, bwd_plan  # noqa: E402,F401
from gemm_cases import _pad_intact  # noqa: E402

# B, T, N, H.  198 = ViT-B/16's 197 tokens + the temporal class token: pipelined backward with the extra tile (as 197);
# 180: pipelined without it; 258 and 5: two kernels.
SHAPES = ((2, 8, 198, 12), (1, 32, 198, 12), (2, 16, 258, 16), (2, 8, 197, 12), (3, 8, 5, 2), (2, 8, 180, 6), (3, 4, 198, 3))
# the backbone's table by frames per clip (vit_clip_zeroI2V.py, HeadShift); any other T: none
MODEL_SHIFTS = {8: (1, -1), 16: (1, -1, 2, -2), 32: (1, -1, 2, -2, 3)}


@dataclass(frozen=True)
class ShiftCase:
    name: str
    B: int
    T: int
    N: int
    H: int
    shifts: Tuple[int, ...]
    seed: int
    poison: bool = False          # B = 3: K / V of clip 1 are NaN, clips 0 and 2 must keep their bits


def tables(T: int, H: int):
    """name -> H shifts: none, the backbone's, and an arbitrary one that holds both extremes T - 1 and -(T - 1)"""
    model = MODEL_SHIFTS.get(T, ())[:H]
    arb = [((-1) ** h) * ((h * 5 + 3) % T) for h in range(H)]
    arb[0], arb[H - 1] = T - 1, -(T - 1)
    return {"zero": (0,) * H, "model": tuple(model) + (0,) * (H - len(model)), "arbitrary": tuple(arb)}


def cases():
    out, seed = [], 7000
    for B, T, N, H in SHAPES:
        for tname, tab in tables(T, H).items():
            out.append(ShiftCase(f"B{B}T{T}N{N}H{H}/{tname}", B, T, N, H, tab, seed))
            seed += 1
            if B == 3 and tname != "zero":
                out.append(ShiftCase(f"B{B}T{T}N{N}H{H}/{tname}/poison", B, T, N, H, tab, seed, poison=True))
                seed += 1
    return out


def make_inputs(case: ShiftCase):
    g = torch.Generator().manual_seed(case.seed)
    D, rows = case.H * 64, case.B * case.T * case.N
    qkv = torch.randn((rows, 3 * D), generator=g).to(BF16)
    do = torch.randn((rows, D), generator=g).to(BF16)
    return qkv, do


def roll_kv(x, case: ShiftCase, sign: int = 1):
    """[B T N, 3 D] rows with the K and V column blocks of every head rolled by sign * shifts[h] along the clip's frames"""
    B, T, N, H = case.B, case.T, case.N, case.H
    D = H * 64
    y = x.clone().view(B, T, N, 3 * D)
    for h, s in enumerate(case.shifts):
        if s % T == 0:
            continue
        for part in (1, 2):
            c = slice(part * D + h * 64, part * D + (h + 1) * 64)
            y[:, :, :, c] = torch.roll(y[:, :, :, c], shifts=sign * s, dims=1)
    return y.view(B * T * N, 3 * D)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b) -> bool:
    return bool(torch.equal(_bits(a), _bits(b)))


class Runner:
    def __init__(self, ops, route, dev):
        self.ops, self.route, self.dev = ops, route, dev

    def launch(self, case: ShiftCase, qkv, do, shifted: bool):
        """forward, then the backward on the forward's own out / lse -> views, (buffer, elements) per output"""
        ops, dev = self.ops, self.dev
        B, T, N, H = case.B, case.T, case.N, case.H
        BT, D = B * T, H * 64
        out, obuf = _flat(BT * N * D, BF16, dev)
        lse, lbuf = _flat(BT * H * N, F32, dev)
        dqkv, dbuf = _flat(BT * N * 3 * D, BF16, dev)
        delta, ebuf = _flat(BT * H * N, F32, dev)
        out, dqkv = out.view(BT * N, D), dqkv.view(BT * N, 3 * D)
        if shifted:
            ops.attn_fwd_shift(qkv, out, lse, B, T, N, H, case.shifts)
            ops.attn_bwd_shift(qkv, out, do, lse, delta, dqkv, B, T, N, H, case.shifts)
        else:
            ops.attn_fwd(qkv, out, lse, BT, N, H)
            ops.attn_bwd(qkv, out, do, lse, delta, dqkv, BT, N, H)
        torch.cuda.synchronize()
        got = {"out": out, "lse": lse, "dqkv": dqkv, "delta": delta}
        bufs = {"out": (obuf, BT * N * D), "lse": (lbuf, BT * H * N), "dqkv": (dbuf, BT * N * 3 * D), "delta": (ebuf, BT * H * N)}
        return got, bufs

    def run(self, case: ShiftCase):
        dev = self.dev
        qkv, do = (t.to(dev) for t in make_inputs(case))
        D = case.H * 64
        rec = {"plan": list(bwd_plan(case.N, self.route)), "shifts": list(case.shifts)}
        got, bufs = self.launch(case, qkv, do, True)
        rec["pad"] = {k: _pad_intact(b, 1, n) for k, (b, n) in bufs.items()}
        rec["finite"] = {k: bool(torch.isfinite(got[k]).all()) for k in ("out", "lse", "dqkv")}
        again, _ = self.launch(case, qkv, do, True)
        rec["repeat"] = {k: _same(got[k], again[k]) for k in got}
        if case.poison:
            # K and V of clip 1 -> NaN: every row of clips 0 and 2 keeps its bits (no item reads outside its clip)
            rows = case.T * case.N
            bad = qkv.clone()
            bad[rows:2 * rows, D:] = float("nan")
            pois, _ = self.launch(case, bad, do, True)
            keep = {}
            for k in ("out", "dqkv"):
                keep[k] = _same(got[k][:rows], pois[k][:rows]) and _same(got[k][2 * rows:], pois[k][2 * rows:])
            n = case.T * case.H * case.N
            keep["lse"] = _same(got["lse"][:n], pois["lse"][:n]) and _same(got["lse"][2 * n:], pois["lse"][2 * n:])
            rec["clips_kept"] = keep
            rec["poison_seen"] = not bool(torch.isfinite(pois["out"][rows:2 * rows]).any())
            return rec
        # the path the kernels replace: unshifted kernels on a rolled copy, dK / dV rolled back
        ref, _ = self.launch(case, roll_kv(qkv, case), do, False)
        want = roll_kv(ref["dqkv"], case, -1)
        rec["equal"] = {"out": _same(got["out"], ref["out"]), "lse": _same(got["lse"], ref["lse"]),
                        "dq": _same(got["dqkv"][:, :D], want[:, :D]), "dk": _same(got["dqkv"][:, D:2 * D], want[:, D:2 * D]),
                        "dv": _same(got["dqkv"][:, 2 * D:], want[:, 2 * D:]), "delta": _same(got["delta"], ref["delta"])}
        if not any(case.shifts):
            plain, _ = self.launch(case, qkv, do, False)
            rec["zero_is_unshifted"] = {k: _same(got[k], plain[k]) for k in got}
        else:
            # the case must be able to fail: without the shift the results differ
            plain, _ = self.launch(case, qkv, do, False)
            rec["shift_matters"] = not _same(got["out"], plain["out"]) and not _same(got["dqkv"], plain["dqkv"])
        return rec

    def refusals(self):
        out = {}
        q = torch.zeros((8 * 5, 3 * 128), dtype=BF16, device=self.dev)
        o = torch.zeros((8 * 5, 128), dtype=BF16, device=self.dev)
        l = torch.zeros((8 * 2 * 5,), dtype=F32, device=self.dev)
        for name, shifts in (("s=T", (8, 0)), ("s=-T", (0, -8))):
            for kind in ("fwd", "bwd"):
                try:
                    if kind == "fwd":
                        self.ops.attn_fwd_shift(q, o, l, 1, 8, 5, 2, shifts)
                    else:
                        self.ops.attn_bwd_shift(q, o, o, l, l.clone(), q.clone(), 1, 8, 5, 2, shifts)
                    out[f"{kind} {name}"] = None
                except RuntimeError as e:
                    out[f"{kind} {name}"] = str(e)
        return out


def main(argv):
    route, path = argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aim_amd import ops
    run = Runner(ops, route, torch.device("cuda"))
    res = {"route": route, "cases": {}}
    with torch.no_grad():
        res["refusals"] = run.refusals()
        for case in cases():
            res["cases"][case.name] = run.run(case)
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
