"""Whole training steps (forward + backward + FlatAdamW) of the AIM recipes' model on one GPU, for DESIGN.md 2g.

    python tools/aim_win_step.py [--clips 8] [--frames 32] [--window 32,2,2] [--steps 4] [--warmup 2] [--rounds 3] [--stock] [--json OUT]

The model is the hmdb51 recipe's (AIM_base_hmdb51.py: ViT-B/16, 32 frames, drop_path_rate 0.2, adapter_scale 0.5, prompt,
wind_attn=True, window (32,2,2), not_shift=False, 51 classes) with pretrained=None and non-zero D_fc2; --stock builds stock AIM
(wind_attn=False: temporal attention over the frames of every token) at the same shape instead.  Under `rocprofv3
--kernel-trace --stats -- python tools/aim_win_step.py --rounds 1` the per-kernel table gives the window attention's share of
the step (tools/prof_summary.py)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--window", default="32,2,2")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stock", action="store_true", help="stock AIM (wind_attn=False) at the same shape")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import aim_amd
    from aim_amd.dist import build_optimizer
    dev = torch.device("cuda")
    window = tuple(int(v) for v in a.window.split(","))
    cfg = dict(type='Recognizer3D',
               backbone=dict(type='AIM', input_resolution=224, patch_size=16, width=768, layers=12, heads=12, num_frames=a.frames,
                             drop_path_rate=0.2, adapter_scale=0.5, pretrained=None, prompt=True, wind_attn=not a.stock,
                             window_size=window, not_shift=a.stock),
               cls_head=dict(type='I3DHead', in_channels=768, num_classes=51, spatial_type='avg', dropout_ratio=0.5),
               test_cfg=dict(average_clips='prob'))
    torch.manual_seed(0)
    m = aim_amd.build_model(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "D_fc2" in n:
                p.normal_(0, 0.02)
    m = m.to(dev).train()
    opt = build_optimizer(m, dict(type='AdamW', lr=3e-4, weight_decay=0.05))
    g = torch.Generator().manual_seed(1234)
    imgs = torch.randn((a.clips, 1, 3, a.frames, 224, 224), generator=g).to(dev)
    label = torch.randint(0, 51, (a.clips, 1), generator=g).to(dev)

    def run(n):
        loss = None
        for _ in range(n):
            opt.zero_grad()
            loss = m(imgs, label, return_loss=True)["loss_cls"]
            loss.backward()
            opt.step()
        return loss

    run(a.warmup)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.rounds):
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        loss = run(a.steps)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / a.steps)
    res = dict(backbone=type(m.backbone).__name__, wind_attn=bool(m.backbone.wind_attn), clips=a.clips, frames=a.frames, window=list(window), rows=a.clips * a.frames * 197, ms_per_step=sorted(times),
               median_ms=sorted(times)[len(times) // 2], peak_GB=torch.cuda.max_memory_allocated() / 1e9,
               last_loss=float(loss.detach()))
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
