"""Stand-alone time of the cut 3-D window attention kernels (aim_win_attn_fwd_cut / aim_win_attn_bwd_cut) beside the shifted
(wrapping) and the unshifted ones at the same (B, T, G, H, window), for the window of the AIM recipes, (32,2,2) cut at (0,1,1),
and for (16,7,7) cut at (8,3,3), the t cut, at 32 clips x 32 frames x 197 tokens, 12 heads.

    python tools/bench_win_attn_cut.py [--clips 32] [--reps 9] [--other-lib PATH/libaim_hip.so] [--json OUT.json]

One process, INTERLEAVED: every repetition launches each call of a window once (HIP events around every launch), after two
warm-up rounds, the order rotated from repetition to repetition.  Reported per call: median, minimum and maximum over the
repetitions; per pair (forward + backward) the same of the per-repetition sums.  The spread (max - min) of a pair is the
yardstick for "equal": DESIGN.md 2g.  --other-lib: a second build of the library (an earlier commit's, say; any ABI that has
the unshifted and the *_shift entries) whose four entries are timed in the same rounds as `fwd@other` ... `bwd_shift@other`.
The work count (64-key tiles x 16-token wave chunks per box and head) is printed beside."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aim_amd import ops  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
WINDOWS = (((32, 2, 2), (0, 1, 1)), ((16, 7, 7), (8, 3, 3)))


def segments(G, w, s):
    cuts = ([0] if s else []) + list(range(s, G, w)) + [G]
    return [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def wave_tile_steps(T, G, window, shift, cut_t):
    """per clip and head: sum over the boxes of ceil(S / 64) key tiles x ceil(S / 16) wave chunks, and the sum of S^2"""
    steps = sq = 0
    for et in (segments(T, window[0], shift[0]) if cut_t else [window[0]] * (T // window[0])):
        for eh in segments(G, window[1], shift[1]):
            for ew in segments(G, window[2], shift[2]):
                S = et * eh * ew
                steps += -(-S // 64) * -(-S // 16)
                sq += S * S
    return steps, sq


def other_calls(path, qkv, out, do, lse, delta, dqkv, B, T, N, H, w, s):
    """the unshifted and the *_shift entries of a second build of the library, through ctypes, on the current stream"""
    lib = ctypes.CDLL(path)
    P, I = ctypes.c_void_p, ctypes.c_int
    sig = {"aim_win_attn_fwd": [P] * 3 + [I] * 8 + [P], "aim_win_attn_bwd": [P] * 6 + [I] * 8 + [P],
           "aim_win_attn_fwd_shift": [P] * 3 + [I] * 11 + [P], "aim_win_attn_bwd_shift": [P] * 6 + [I] * 11 + [P]}
    for name, args in sig.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, I
    stream = lambda: torch.cuda.current_stream().cuda_stream
    f3 = (qkv.data_ptr(), out.data_ptr(), lse.data_ptr())
    b6 = (qkv.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr())

    def call(name, ptrs, ints):
        def f():
            rc = getattr(lib, name)(*ptrs, *ints, stream())
            if rc:
                raise RuntimeError(f"{name} of {path} failed (rc={rc})")
        return f

    geom = (B, T, N, N, H) + tuple(w)
    return {"fwd@other": call("aim_win_attn_fwd", f3, geom), "bwd@other": call("aim_win_attn_bwd", b6, geom),
            "fwd_shift@other": call("aim_win_attn_fwd_shift", f3, geom + tuple(s)),
            "bwd_shift@other": call("aim_win_attn_bwd_shift", b6, geom + tuple(s))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, T, G, H = a.clips, 32, 14, 12
    N = G * G + 1
    D, BT = H * 64, B * T
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device=dev).to(BF16)
    qkv, do = rnd(BT * N, 3 * D), rnd(BT * N, D)
    out, dqkv = torch.zeros((BT * N, D), dtype=BF16, device=dev), torch.zeros((BT * N, 3 * D), dtype=BF16, device=dev)
    lse, delta = torch.zeros((BT, H, N), dtype=F32, device=dev), torch.zeros((BT, H, N), dtype=F32, device=dev)
    res = {"clips": B, "frames": T, "heads": H, "reps": a.reps, "other_lib": bool(a.other_lib), "windows": {}}
    for w, s in WINDOWS:
        calls = {"fwd": lambda: ops.win_attn_fwd(qkv, out, lse, B, T, N, H, w),
                 "bwd": lambda: ops.win_attn_bwd(qkv, out, do, lse, delta, dqkv, B, T, N, H, w),
                 "fwd_shift": lambda: ops.win_attn_fwd_shift(qkv, out, lse, B, T, N, H, w, s),
                 "bwd_shift": lambda: ops.win_attn_bwd_shift(qkv, out, do, lse, delta, dqkv, B, T, N, H, w, s),
                 "fwd_cut": lambda: ops.win_attn_fwd_cut(qkv, out, lse, B, T, N, H, w, s),
                 "bwd_cut": lambda: ops.win_attn_bwd_cut(qkv, out, do, lse, delta, dqkv, B, T, N, H, w, s)}
        if a.other_lib:
            calls.update(other_calls(a.other_lib, qkv, out, do, lse, delta, dqkv, B, T, N, H, w, s))
        # each backward right after its own forward, so that it reads the lse / out of its own grouping
        pairs = [("fwd" + x, "bwd" + x) for x in ("", "_shift", "_cut") + (("@other", "_shift@other") if a.other_lib else ())]
        times = {k: [] for k in calls}
        for rep in range(a.reps + 2):
            r = rep % len(pairs)
            for fk, bk in pairs[r:] + pairs[:r]:
                for k in (fk, bk):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    calls[k]()
                    e1.record()
                    e1.synchronize()
                    if rep >= 2:
                        times[k].append(e0.elapsed_time(e1))
        stat = lambda v: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)}
        rec = {k: stat(v) for k, v in times.items()}
        for fk, bk in pairs:
            rec["pair" + fk[3:]] = stat([f + b for f, b in zip(times[fk], times[bk])])
        rec["work_unshifted"] = wave_tile_steps(T, G, w, (0, 0, 0), False)
        rec["work_shift"], rec["work_cut"] = wave_tile_steps(T, G, w, s, False), wave_tile_steps(T, G, w, s, True)
        res["windows"]["x".join(map(str, w))] = rec
        for k in list(calls) + ["pair" + fk[3:] for fk, _ in pairs]:
            r = rec[k]
            print(f"{w} {k:18s} median {r['median_ms']:.3f} ms  (min {r['min_ms']:.3f}, max {r['max_ms']:.3f})", flush=True)
        print(f"{w} wave-tile steps per clip and head (sum S^2): cut {rec['work_cut']}, shifted {rec['work_shift']}, "
              f"unshifted {rec['work_unshifted']}", flush=True)
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
