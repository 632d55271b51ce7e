"""Mixup / Cutmix fused into the patch gather vs the reference's materialised blend, at BASELINE configs[1]'s shape
(64 clips x 3 x 8 x 224^2 fp32, ViT-B/16).

Part 1, the gather alone: device time (HIP events, mean of --iters calls after a warm-up) and peak memory above the
resident inputs of
  patchify                 -- aim_patchify of the clip batch (what every training step runs)
  fused mixup / cutmix     -- aim_patchify_blend (no blended copy is written)
  eager mixup / cutmix     -- blending.apply's eager ops (the reference's) + aim_patchify of the blended copy
Part 2, whole training steps (bench.py's model, FlatAdamW), interleaved over --rounds rounds of --steps steps each:
  none / LabelSmoothing(400, 0.1) / Mixup fused / Mixup materialised (fuse_blending = False).

    python tools/blend_probe.py [--iters 20] [--rounds 4] [--steps 5] [--out RESULT.json]

Both parts print one JSON line each; --out also writes them to a file.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gather_part(dev, iters):
    from aim_amd import ops
    from aim_amd.blending import CutmixBlending, MixupBlending
    B, T, R, p = 64, 8, 224, 16
    g = torch.Generator().manual_seed(0)
    imgs6 = torch.randn((B, 1, 3, T, R, R), generator=g).to(dev)
    imgs = imgs6.view(B, 3, T, R, R)
    Kp = 3 * p * p
    A = torch.empty((B * T * (R // p) ** 2, Kp), dtype=torch.bfloat16, device=dev)
    torch.manual_seed(1)
    mix, cut = MixupBlending(400, alpha=0.8), CutmixBlending(400, alpha=1.0)
    pm, pc = mix.draw(imgs6.shape), cut.draw(imgs6.shape)
    fm, fc = mix.fused(pm, 1, dev), cut.fused(pc, 1, dev)

    def eager(bl, plan):
        x = bl.mix_imgs(imgs6, plan).view(B, 3, T, R, R)
        ops.patchify(x, A, B, T, R, R, p, Kp)

    cases = {
        "patchify": lambda: ops.patchify(imgs, A, B, T, R, R, p, Kp),
        "fused_mixup": lambda: ops.patchify(imgs, A, B, T, R, R, p, Kp, blend=fm),
        "fused_cutmix": lambda: ops.patchify(imgs, A, B, T, R, R, p, Kp, blend=fc),
        "eager_mixup": lambda: eager(mix, pm),
        "eager_cutmix": lambda: eager(cut, pc),
    }
    out = {"box": list(pc.box), "clip_batch_MB": imgs.numel() * 4 / 1e6}
    for name, fn in cases.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = dict(ms=e0.elapsed_time(e1) / iters, peak_extra_MB=(torch.cuda.max_memory_allocated() - base) / 1e6)
    # the fused gathers write what patchify of the eager blend writes
    ref = torch.empty_like(A)
    for bl, plan, fb in ((mix, pm, fm), (cut, pc, fc)):
        eager(bl, plan)
        ref.copy_(A)
        ops.patchify(imgs, A, B, T, R, R, p, Kp, blend=fb)
        out["bit_identical_" + type(bl).__name__] = bool(torch.equal(A.view(torch.int16), ref.view(torch.int16)))
    return out


def step_part(dev, rounds, steps):
    import bench
    from aim_amd.blending import LabelSmoothing, MixupBlending
    from aim_amd.dist import build_optimizer
    model = bench.build_model(8, dev)
    opt = build_optimizer(model, dict(type='AdamW', lr=3e-4, weight_decay=0.05))
    g = torch.Generator().manual_seed(1234)
    imgs = torch.randn((64, 1, 3, 8, 224, 224), generator=g).to(dev)
    label = torch.randint(0, 400, (64, 1), generator=g).to(dev)
    variants = {"none": (None, True), "label_smoothing": (LabelSmoothing(400, smoothing=0.1), True),
                "mixup_fused": (MixupBlending(400, alpha=0.8), True), "mixup_materialised": (MixupBlending(400, alpha=0.8), False)}

    def run(n):
        for _ in range(n):
            opt.zero_grad()
            loss = model(imgs, label, return_loss=True)["loss_cls"]
            loss.backward()
            opt.step()

    times = {k: [] for k in variants}
    peaks = {}
    for k, (bl, fuse) in variants.items():       # warm-up of every variant
        model.blending, model.fuse_blending = bl, fuse
        run(2)
    torch.cuda.synchronize()
    for r in range(rounds):
        order = list(variants) if r % 2 == 0 else list(reversed(variants))
        for k in order:
            bl, fuse = variants[k]
            model.blending, model.fuse_blending = bl, fuse
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            run(steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
            peaks[k] = max(peaks.get(k, 0.0), torch.cuda.max_memory_allocated() / 1e9)
    return {k: dict(ms_per_step=sorted(v), median=sorted(v)[len(v) // 2], peak_GB=peaks[k]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="part 1 only")
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blend_probe.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"gather": gather_part(dev, args.iters)}
    print(json.dumps(res["gather"]), flush=True)
    torch.cuda.empty_cache()
    if not args.no_steps:
        res["steps"] = step_part(dev, args.rounds, args.steps)
        print(json.dumps(res["steps"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
