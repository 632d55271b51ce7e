"""Stand-alone time of the shifted 3-D window attention kernels (aim_win_attn_fwd_shift / aim_win_attn_bwd_shift) beside the
unshifted ones at the same (B, T, G, H, window), for the two windows of the AIM_FLASH recipes at their videos_per_gpu
(32 clips x 32 frames x 197 tokens, 12 heads; diving48 runs (32,2,2) at 64 clips: --clips 64).

    python tools/bench_win_attn_shift.py [--clips 32] [--reps 9] [--json OUT.json]

One process, INTERLEAVED: every repetition launches each of the four calls of a window once (HIP events around every launch),
after two warm-up rounds.  Reported per call: median, minimum and maximum over the repetitions; per pair (forward +
backward) the same of the per-repetition sums, and the spread (max - min) of the unshifted pair, which is the yardstick for
"not slower": DESIGN.md 2f.  The work count (64-key tiles x 16-token wave chunks per box and head) is printed beside."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aim_amd import ops  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
WINDOWS = (((16, 7, 7), (8, 3, 3)), ((32, 2, 2), (0, 1, 1)))


def segments(G, w, s):
    cuts = ([0] if s else []) + list(range(s, G, w)) + [G]
    return [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def wave_tile_steps(T, G, window, shift):
    """per clip and head: sum over the boxes of ceil(S / 64) key tiles x ceil(S / 16) wave chunks, and the sum of S^2"""
    steps = sq = 0
    for _ in range(T // window[0]):
        for eh in segments(G, window[1], shift[1]):
            for ew in segments(G, window[2], shift[2]):
                S = window[0] * eh * ew
                steps += -(-S // 64) * -(-S // 16)
                sq += S * S
    return steps, sq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
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
    res = {"clips": B, "frames": T, "heads": H, "reps": a.reps, "windows": {}}
    for w, s in WINDOWS:
        calls = {"fwd": lambda: ops.win_attn_fwd(qkv, out, lse, B, T, N, H, w),
                 "fwd_shift": lambda: ops.win_attn_fwd_shift(qkv, out, lse, B, T, N, H, w, s),
                 "bwd": lambda: ops.win_attn_bwd(qkv, out, do, lse, delta, dqkv, B, T, N, H, w),
                 "bwd_shift": lambda: ops.win_attn_bwd_shift(qkv, out, do, lse, delta, dqkv, B, T, N, H, w, s)}
        # each backward right after its own forward, so that it reads the lse / out of its own grouping
        order = ("fwd", "bwd", "fwd_shift", "bwd_shift")
        times = {k: [] for k in calls}
        for rep in range(a.reps + 2):
            for k in (order if rep % 2 == 0 else order[2:] + order[:2]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[k]()
                e1.record()
                e1.synchronize()
                if rep >= 2:
                    times[k].append(e0.elapsed_time(e1))
        stat = lambda v: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)}
        rec = {k: stat(v) for k, v in times.items()}
        rec["pair"] = stat([f + b for f, b in zip(times["fwd"], times["bwd"])])
        rec["pair_shift"] = stat([f + b for f, b in zip(times["fwd_shift"], times["bwd_shift"])])
        rec["work_unshifted"], rec["work_shifted"] = wave_tile_steps(T, G, w, (0, 0, 0)), wave_tile_steps(T, G, w, s)
        res["windows"]["x".join(map(str, w))] = rec
        for k in ("fwd", "fwd_shift", "bwd", "bwd_shift", "pair", "pair_shift"):
            r = rec[k]
            print(f"{w} {k:10s} median {r['median_ms']:.3f} ms  (min {r['min_ms']:.3f}, max {r['max_ms']:.3f})", flush=True)
        print(f"{w} wave-tile steps per clip and head (sum S^2): shifted {rec['work_shifted']}, unshifted {rec['work_unshifted']}",
              flush=True)
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
