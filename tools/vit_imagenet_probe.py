#!/usr/bin/env python3
"""Time the vit_imagenet_k400 per-GPU training step (8 clips x 8 frames, 224^2, update_interval=1: fwd + bwd + FlatAdamW) with
hipEvents, three ways: ViT_ImageNet training every parameter, ViT_ImageNet frozen by AIM's policy (adapters, temporal_embedding,
ln_post), and the stock AIM at the same shape.  One JSON line per mode.

    python tools/vit_imagenet_probe.py [--steps 10] [--warmup 3] [--modes full,frozen,aim]

Under ``rocprofv3 --kernel-trace --stats -- python tools/vit_imagenet_probe.py --modes full`` the kernel table gives the share
of the step spent in the weight-gradient kernels."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aim_amd  # noqa: E402
from aim_amd.dist import build_optimizer  # noqa: E402


def model_cfg(mode):
    if mode == "aim":
        bb = dict(type='AIM', input_resolution=224, patch_size=16, num_frames=8, width=768, layers=12, heads=12,
                  drop_path_rate=0.2, adapter_scale=0.5)
    else:
        bb = dict(type='ViT_ImageNet', img_size=224, patch_size=16, num_frames=8, embed_dim=768, depth=12, num_heads=12,
                  drop_path_rate=0.2, adapter_scale=0.5)
    return dict(type='Recognizer3D', backbone=bb,
                cls_head=dict(type='I3DHead', in_channels=768, num_classes=400, spatial_type='avg', dropout_ratio=0.5),
                test_cfg=dict(average_clips='prob'))


def run(mode, steps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = aim_amd.build_model(model_cfg(mode))
    if mode == "frozen":
        for n, p in model.backbone.named_parameters():
            if not ("temporal_embedding" in n or "ln_post" in n or "Adapter" in n):
                p.requires_grad = False
    model = model.to(dev).train()
    opt = build_optimizer(model, dict(type='AdamW', lr=3e-4, betas=(0.9, 0.999), weight_decay=0.05))
    imgs = torch.randn((8, 1, 3, 8, 224, 224), device=dev)
    label = torch.randint(0, 400, (8, 1), device=dev)

    def step():
        opt.zero_grad()
        model(imgs, label, return_loss=True)["loss_cls"].backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
    return dict(mode=mode, ms_per_step=round(ms, 3), clips_per_s=round(8 * 1000.0 / ms, 1), trainable_params=n_train,
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="full,frozen,aim")
    a = ap.parse_args()
    for mode in a.modes.split(","):
        print(json.dumps(run(mode, a.steps, a.warmup)), flush=True)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
