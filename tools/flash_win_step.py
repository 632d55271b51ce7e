"""Whole training steps (forward + backward + FlatAdamW) of the AIM_FLASH_WIN recipes' model on one GPU, for DESIGN.md 2e.

    python tools/flash_win_step.py [--clips 16] [--frames 16] [--window 16,7,7] [--steps 4] [--warmup 2] [--rounds 3] [--shift] [--json OUT]

The model is the hmdb51 recipe's (ViT-B/16, drop_path_rate 0.2, adapter_scale 0.5, prompt, 51 classes; its 16 frames unless
--frames says otherwise) with pretrained=None and non-zero D_fc2; --shift builds the AIM_FLASH recipes' model instead.  Under `rocprofv3 --kernel-trace --stats -- python
tools/flash_win_step.py --rounds 1` the per-kernel table gives the window attention's share of the step
(tools/prof_summary.py)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--window", default="16,7,7")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shift", action="store_true", help="AIM_FLASH: every odd block on windows shifted by half a window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import aim_amd
    from aim_amd.dist import build_optimizer
    dev = torch.device("cuda")
    window = tuple(int(v) for v in a.window.split(","))
    cfg = dict(type='Recognizer3D',
               backbone=dict(type='AIM_FLASH' if a.shift else 'AIM_FLASH_WIN', input_resolution=224, patch_size=16, width=768, layers=12, heads=12,
                             num_frames=a.frames, drop_path_rate=0.2, adapter_scale=0.5, pretrained=None, use_flash_attn=True,
                             checkpoint=False, prompt=True, wind_attn=True, window_size=window, not_shift=not a.shift),
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
    res = dict(backbone=type(m.backbone).__name__, clips=a.clips, frames=a.frames, window=list(window), rows=a.clips * a.frames * 197, ms_per_step=sorted(times),
               median_ms=sorted(times)[len(times) // 2], peak_GB=torch.cuda.max_memory_allocated() / 1e9,
               last_loss=float(loss.detach()))
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
