"""SwinTransformer3D at the k400 base recipe's per-GPU shape: whole training steps, for DESIGN.md section 2k.

    python tools/swin3d_step.py [--clips 8] [--frames 32] [--window 8 7 7] [--rounds 5] [--warmup 2] [--json OUT]

The model is the recipe's Swin-B (embed 128, depths 2 / 2 / 18 / 2, heads 4 / 8 / 16 / 32, window (8,7,7), patch_norm,
drop_path_rate 0.3 as in swin_base_patch244_window877_kinetics400_1k.py) with an I3DHead of 400 classes after ``init_weights()``.
A step is zero_grad, forward, loss, backward and one FlatAdamW step on random clips, between two hipEvents.  ``--clips 0`` takes
the largest of (8, 6, 4, 2, 1) whose step fits the GPU's memory.  The figure is the median over the rounds behind the warm-up,
with min and max, and the peak of torch's allocator.  Under ``rocprofv3 --kernel-trace --stats -- python tools/swin3d_step.py
--rounds 1 --warmup 1`` the kernel table is that of two steps."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--window", type=int, nargs=3, default=(8, 7, 7))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import aim_amd
    from aim_amd.dist import build_optimizer
    dev = torch.device("cuda")
    cfg = dict(type='Recognizer3D',
               backbone=dict(type='SwinTransformer3D', patch_size=(2, 4, 4), embed_dim=128, depths=[2, 2, 18, 2],
                             num_heads=[4, 8, 16, 32], window_size=tuple(a.window), patch_norm=True, drop_path_rate=0.3),
               cls_head=dict(type='I3DHead', in_channels=1024, num_classes=400, spatial_type='avg', dropout_ratio=0.5),
               test_cfg=dict(average_clips='prob'))
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg)
    model.backbone.init_weights()
    model = model.to(dev).train()
    opt = build_optimizer(model, dict(type='AdamW', lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05,
                                      paramwise_cfg=dict(custom_keys={'absolute_pos_embed': dict(decay_mult=0.),
                                                                      'relative_position_bias_table': dict(decay_mult=0.),
                                                                      'norm': dict(decay_mult=0.), 'backbone': dict(lr_mult=0.1)})))
    gen = torch.Generator().manual_seed(1234)

    def step(imgs, label):
        opt.zero_grad()
        loss = model(imgs, label, return_loss=True)["loss_cls"]
        loss.backward()
        opt.step()
        return loss

    B = None
    for cand in ([a.clips] if a.clips else [8, 6, 4, 2, 1]):
        try:
            imgs = torch.randn((cand, 1, 3, a.frames, 224, 224), generator=gen).to(dev)
            label = torch.randint(0, 400, (cand, 1), generator=gen).to(dev)
            step(imgs, label)
            torch.cuda.synchronize()
            B = cand
            break
        except torch.cuda.OutOfMemoryError:
            opt.zero_grad()
            imgs = label = None
            torch.cuda.empty_cache()
    assert B, "no batch size fits"
    torch.cuda.reset_peak_memory_stats()
    ms, losses = [], []
    for r in range(a.warmup + a.rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step(imgs, label)
        e1.record()
        torch.cuda.synchronize()
        losses.append(float(loss))
        if r >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    s = sorted(ms)
    res = dict(model="SwinTransformer3D Swin-B (k400 base recipe shape)", clips=B, frames=a.frames, window=list(a.window),
               rows_stage0=B * (a.frames // 2) * 3136, rounds=a.rounds, warmup=a.warmup, median_ms=round(s[len(s) // 2], 2),
               min_ms=round(s[0], 2), max_ms=round(s[-1], 2), clips_per_s=round(B * 1e3 / s[len(s) // 2], 2),
               peak_alloc_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
               losses_finite=all(l == l and abs(l) != float("inf") for l in losses), optimizer=type(opt).__name__,
               parameters=sum(p.numel() for p in model.parameters()))
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
