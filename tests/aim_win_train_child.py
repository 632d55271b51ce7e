"""Child process of tests/test_aim_win_gpu.py: three training steps of the hmdb51 AIM recipe (stored values, pretrained=None,
wind_attn=True, not_shift=False) at reduced width and depth (128 wide, 2 heads, 2 layers, so that block 1 is cut; the recipe's
32 frames, 224 x 224 and (32,2,2) windows cut at (0,1,1)) on uint8 clips through the GPUNormalize hook and build_optimizer;
writes the losses and a digest of every parameter before and after.  The stream switches (AIM_SIDE_STREAM, AIM_DETACH_WGRAD,
AIM_DETACH_BIG) are read when the package is imported, hence one process per setting:
python aim_win_train_child.py <result.json>"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from aim_flash_win_train_child import SMALL, STEPS, digest  # noqa: E402

RECIPE = "recognition/vit/AIM/AIM_base_hmdb51.py"


def main(path):
    import aim_amd
    from aim_amd.dist import build_optimizer
    from test_aim_win_cpu import write_config_tree
    root = path + ".cfg"
    write_config_tree(root)
    cfg = aim_amd.Config.fromfile(os.path.join(root, RECIPE))
    cfg.merge_from_dict(SMALL)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg.model)
    # D_fc2 starts at zero (init_weights): give it values so that every gradient path is live from the first step
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "D_fc2" in n:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    model = model.to(dev).train()
    aim_amd.register_module_hooks(model, [dict(h) for h in cfg.module_hooks])
    opt = build_optimizer(model, dict(cfg.optimizer))
    B, T = 2, cfg.model.backbone.num_frames
    imgs = torch.randint(0, 256, (B, 1, 3, T, 224, 224), generator=gen, dtype=torch.uint8).to(dev)
    label = torch.randint(0, cfg.model.cls_head.num_classes, (B, 1), generator=gen).to(dev)
    before = {n: digest(p) for n, p in model.named_parameters()}
    trainable = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    losses, finite = [], True
    for step in range(STEPS):
        opt.zero_grad()
        loss = model(imgs, label, return_loss=True)["loss_cls"]
        loss.backward()
        for n, p in model.named_parameters():
            if p.requires_grad:
                finite = finite and p.grad is not None and bool(torch.isfinite(p.grad).all())
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    after = {n: digest(p) for n, p in model.named_parameters()}
    bb = model.backbone
    res = dict(losses=losses, loss_bits=[digest(torch.tensor(v, dtype=torch.float64)) for v in losses], finite=finite,
               trainable=trainable, before=before, after=after, optimizer=type(opt).__name__, backbone=type(bb).__name__,
               in_place=bool(bb.grad_in_place), window=list(bb.window_size), frames=T, prompt=bool(bb.prompt), wind_attn=bool(bb.wind_attn),
               shifts=[bb._block_shift(i, T, 14) for i in range(bb.layers)])
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
