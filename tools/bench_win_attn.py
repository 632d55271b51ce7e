"""Stand-alone time of the 3-D window attention kernels at the hmdb51 recipe's per-GPU shape (16 clips x 32 frames x 197 tokens,
12 heads) for the two recipe windows, beside the spatial kernels (aim_attn_fwd / aim_attn_bwd at 512 frames x 198 tokens)
measured in the same process: the spatial kernels' rate is the yardstick for the streaming kernel.

    python tools/bench_win_attn.py [--reps 7] [--json OUT.json]

The kernels are timed INTERLEAVED (one launch of each per repetition, HIP events around every launch, median over the
repetitions after two warm-up rounds), so that clock and thermal drift hit all of them alike.  FLOP counts are the
algorithm's, 4 S^2 64 per (window, head) forward and 2.5 times that backward (the two-pass backward executes 7 products for
the algorithm's 5: its achieved rate is reported against the 5)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aim_amd import ops  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, T, N, H = 16, 32, 197, 12
    D, BT = H * 64, B * T
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device=dev).to(BF16)
    calls = {}
    # window attention on the N-token layout
    qkv, do = rnd(BT * N, 3 * D), rnd(BT * N, D)
    out, dqkv = torch.zeros((BT * N, D), dtype=BF16, device=dev), torch.zeros((BT * N, 3 * D), dtype=BF16, device=dev)
    lse, delta = torch.zeros((BT, H, N), dtype=F32, device=dev), torch.zeros((BT, H, N), dtype=F32, device=dev)
    for w in ((16, 7, 7), (32, 1, 1)):
        S = w[0] * w[1] * w[2]
        flops = 4.0 * S * S * 64 * (BT * (N - 1) // S) * H
        tag = "x".join(map(str, w))
        calls[f"win_attn_fwd {tag}"] = (lambda w=w: ops.win_attn_fwd(qkv, out, lse, B, T, N, H, w), flops)
        calls[f"win_attn_bwd {tag}"] = (lambda w=w: ops.win_attn_bwd(qkv, out, do, lse, delta, dqkv, B, T, N, H, w), 2.5 * flops)
    # the spatial kernels at the prompt's 198 tokens
    Ns = N + 1
    qkv2, do2 = rnd(BT * Ns, 3 * D), rnd(BT * Ns, D)
    out2, dqkv2 = torch.zeros((BT * Ns, D), dtype=BF16, device=dev), torch.zeros((BT * Ns, 3 * D), dtype=BF16, device=dev)
    lse2, delta2 = torch.zeros((BT, H, Ns), dtype=F32, device=dev), torch.zeros((BT, H, Ns), dtype=F32, device=dev)
    fs = 4.0 * Ns * Ns * 64 * BT * H
    calls["attn_fwd 198"] = (lambda: ops.attn_fwd(qkv2, out2, lse2, BT, Ns, H), fs)
    calls["attn_bwd 198"] = (lambda: ops.attn_bwd(qkv2, out2, do2, lse2, delta2, dqkv2, BT, Ns, H), 2.5 * fs)
    # forwards first, so that every backward reads the lse / out of its own forward
    order = sorted(calls, key=lambda k: "bwd" in k)
    times = {k: [] for k in calls}
    for rep in range(a.reps + 2):
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            calls[k][0]()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[k].append(e0.elapsed_time(e1))
    res = {}
    for k in calls:
        ts = sorted(times[k])
        ms = ts[len(ts) // 2]
        res[k] = dict(ms=ms, min_ms=ts[0], max_ms=ts[-1], tflops=calls[k][1] / ms / 1e9, gflop=calls[k][1] / 1e9)
        print(f"{k:24s} {ms:8.3f} ms  (min {ts[0]:.3f}, max {ts[-1]:.3f})  {res[k]['tflops']:7.1f} TFLOP/s  [{res[k]['gflop']:.0f} GFLOP]")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(shape=dict(B=B, T=T, N=N, H=H), reps=a.reps, results=res), f, indent=1)


if __name__ == "__main__":
    main()
