"""Head-shifted attention kernels against what they replace, at the sthv2 ZeroI2V recipe's per-GPU shape
(32 clips x 8 frames, 12 heads, 198 tokens: ViT-B/16's 197 + the temporal class token; shifts +1, -1 on heads 0, 1).

Part 1, the kernels: device time (HIP events around --iters calls) of, interleaved over --rounds rounds in one process,
  fwd_shift / bwd_shift   -- aim_attn_fwd_shift / aim_attn_bwd_shift on the fused qkv buffer
  fwd / bwd               -- (a) the unshifted entry points on the same buffers (what the shift costs)
  fwd_roll / bwd_roll     -- (b) the path the kernels replace: torch.roll of the shifted heads' K and V column blocks into a
                             copy of qkv, the unshifted kernel, and for the backward the roll back of dK / dV
with the bytes each form moves (computed from the shapes).  The shifted kernels must beat (b) in every round.
Part 2 (--steps > 0), for information: whole training steps (fwd + bwd + FlatAdamW) of ViT_CLIP_ZEROI2V next to ViT_CLIP at
the same shape in the same run, with peak memory.

    python tools/attn_shift_probe.py [--iters 20] [--rounds 5] [--steps 5] [--clips 32] [--out RESULT.json]

Prints one JSON line per part; --out also writes them to a file.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF16, F32 = torch.bfloat16, torch.float32


def kernel_part(dev, B, T, N, H, iters, rounds):
    from aim_amd import ops
    from aim_amd.zeroi2v import head_shifts
    shifts = head_shifts(T, H)
    BT, D = B * T, H * 64
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn((BT * N, 3 * D), generator=g).to(BF16).to(dev)
    do = torch.randn((BT * N, D), generator=g).to(BF16).to(dev)
    out, lse = torch.empty((BT * N, D), dtype=BF16, device=dev), torch.empty((BT, H, N), dtype=F32, device=dev)
    delta, dqkv = torch.empty((BT, H, N), dtype=F32, device=dev), torch.empty((BT * N, 3 * D), dtype=BF16, device=dev)
    qkv_r, dqkv_r = torch.empty_like(qkv), torch.empty_like(dqkv)
    cols = [(h, s) for h, s in enumerate(shifts) if s]

    def roll_into(dst, src, sign):
        """dst = src with the K and V column blocks of the shifted heads rolled along the clip's frames"""
        dst.copy_(src)
        d5, s5 = dst.view(B, T, N, 3 * D), src.view(B, T, N, 3 * D)
        for h, s in cols:
            for part in (1, 2):
                c = slice(part * D + h * 64, part * D + (h + 1) * 64)
                d5[:, :, :, c] = torch.roll(s5[:, :, :, c], shifts=sign * s, dims=1)

    def bwd_roll():
        ops.attn_bwd(qkv_r, out, do, lse, delta, dqkv_r, BT, N, H)
        roll_into(dqkv, dqkv_r, -1)

    def fwd_roll():
        roll_into(qkv_r, qkv, 1)
        ops.attn_fwd(qkv_r, out, lse, BT, N, H)

    cases = {
        "fwd_shift": lambda: ops.attn_fwd_shift(qkv, out, lse, B, T, N, H, shifts),
        "fwd": lambda: ops.attn_fwd(qkv, out, lse, BT, N, H),
        "fwd_roll": fwd_roll,
        "bwd_shift": lambda: ops.attn_bwd_shift(qkv, out, do, lse, delta, dqkv, B, T, N, H, shifts),
        "bwd": lambda: ops.attn_bwd(qkv, out, do, lse, delta, dqkv, BT, N, H),
        "bwd_roll": bwd_roll,
    }
    # bytes from the shapes: the kernels read q, k, v (+ O, dO in the backward) and write O (dq, dk, dv); the roll path
    # also copies the whole buffer once and re-reads / re-writes the shifted blocks
    e = 2
    fwd_b = BT * N * (3 * D + D) * e + BT * H * N * 4
    bwd_b = BT * N * (3 * D + 2 * D + 3 * D) * e + BT * H * N * 4
    roll_b = 2 * BT * N * 3 * D * e + 2 * 2 * len(cols) * BT * N * 64 * e
    res = {"shape": dict(B=B, T=T, N=N, H=H, shifts=list(shifts)),
           "MB": dict(fwd=fwd_b / 1e6, bwd=bwd_b / 1e6, roll_extra=roll_b / 1e6), "ms": {k: [] for k in cases}}
    fwd_roll()                       # qkv_r, out, lse hold consistent values for every backward form
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for r in range(rounds):
        order = list(cases) if r % 2 == 0 else list(reversed(cases))
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                cases[k]()
            e1.record()
            torch.cuda.synchronize()
            res["ms"][k].append(e0.elapsed_time(e1) / iters)
    ms = res["ms"]
    res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    res["shift_over_unshifted"] = {d: sorted(a / b for a, b in zip(ms[d + "_shift"], ms[d]))[rounds // 2] for d in ("fwd", "bwd")}
    res["beats_roll_in_every_round"] = {d: all(a < b for a, b in zip(ms[d + "_shift"], ms[d + "_roll"])) for d in ("fwd", "bwd")}
    # the two paths compute the same bits
    ops.attn_fwd_shift(qkv, out, lse, B, T, N, H, shifts)
    o1, l1 = out.clone(), lse.clone()
    ops.attn_bwd_shift(qkv, out, do, lse, delta, dqkv, B, T, N, H, shifts)
    d1 = dqkv.clone()
    fwd_roll()
    bwd_roll()
    torch.cuda.synchronize()
    res["bit_identical"] = bool(torch.equal(o1.view(torch.int16), out.view(torch.int16)) and torch.equal(l1, lse)
                                and torch.equal(d1.view(torch.int16), dqkv.view(torch.int16)))
    return res


def step_part(dev, clips, rounds, steps):
    import aim_amd
    from aim_amd.dist import build_optimizer
    arch = dict(patch_size=16, width=768, layers=12, heads=12)
    models = {}
    for name, bb in (("ViT_CLIP", dict(type='ViT_CLIP')), ("ViT_CLIP_ZEROI2V", dict(type='ViT_CLIP_ZEROI2V', with_t_cls_token=True))):
        cfg = dict(type='Recognizer3D',
                   backbone=dict(input_resolution=224, num_frames=8, drop_path_rate=0.2, adapter_scale=0.5, pretrained=None,
                                 **arch, **bb),
                   cls_head=dict(type='I3DHead', in_channels=768, num_classes=174, spatial_type='avg', dropout_ratio=0.5),
                   test_cfg=dict(average_clips='prob'),
                   train_cfg=dict(blending=dict(type='LabelSmoothing', num_classes=174, smoothing=0.1)))
        torch.manual_seed(0)
        m = aim_amd.build_model(cfg)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "D_fc2" in n:
                    p.normal_(0, 0.02)
        m = m.to(dev).train()
        models[name] = (m, build_optimizer(m, dict(type='AdamW', lr=3e-4, weight_decay=0.05)))
    g = torch.Generator().manual_seed(1234)
    imgs = torch.randn((clips, 1, 3, 8, 224, 224), generator=g).to(dev)
    label = torch.randint(0, 174, (clips, 1), generator=g).to(dev)

    def run(name, n):
        m, opt = models[name]
        for _ in range(n):
            opt.zero_grad()
            m(imgs, label, return_loss=True)["loss_cls"].backward()
            opt.step()

    for name in models:
        run(name, 2)
    torch.cuda.synchronize()
    times, peaks = {k: [] for k in models}, {}
    for r in range(rounds):
        for name in (list(models) if r % 2 == 0 else list(reversed(models))):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            run(name, steps)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
            peaks[name] = max(peaks.get(name, 0.0), torch.cuda.max_memory_allocated() / 1e9)
    return {"clips": clips, **{k: dict(ms_per_step=sorted(v), median=sorted(v)[len(v) // 2], peak_GB=peaks[k]) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5, help="training steps per round of part 2 (0: part 1 only)")
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_shift_probe.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"kernels": kernel_part(dev, args.clips, 8, 198, 12, args.iters, args.rounds)}
    print(json.dumps(res["kernels"]), flush=True)
    torch.cuda.empty_cache()
    if args.steps > 0:
        res["steps"] = step_part(dev, args.clips, args.rounds, args.steps)
        print(json.dumps(res["steps"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if not all(res["kernels"]["beats_roll_in_every_round"].values()) or not res["kernels"]["bit_identical"]:
        raise SystemExit("the shifted kernels did not beat the roll path in every round, or the bits differ")


if __name__ == "__main__":
    main()
