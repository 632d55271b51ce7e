"""Child process of tests/test_zeroi2v_linear_gpu.py: two training steps of the sthv2 ZeroI2V recipe with
``linear_adapter=True`` (stored recipe values, pretrained=None) on uint8 clips through the GPUNormalize hook, LabelSmoothing and
build_optimizer (FlatAdamW, in-place gradients); then a merged forward.  Writes the losses, a digest of every parameter before
and after, and a digest of the merged features:  python zeroi2v_linear_train_child.py <result.json>"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from zeroi2v_train_child import HOOKS_FROM, RECIPE, _value, digest  # noqa: E402


def main(path):
    import aim_amd
    from aim_amd.dist import build_optimizer
    with open(os.path.join(HERE, "golden", "reference_zeroi2v_configs.json")) as f:
        configs = json.load(f)
    root = path + ".cfg"
    for rel, d in configs.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {_value(v)!r}\n")
    cfg = aim_amd.Config.fromfile(os.path.join(root, RECIPE))
    cfg.merge_from_dict({"model.backbone.pretrained": None, "model.backbone.linear_adapter": True})
    hooks = cfg.get("module_hooks") or aim_amd.Config.fromfile(os.path.join(root, HOOKS_FROM)).module_hooks
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    # the D_fc2 that start at zero (init_weights): give them values so that every gradient path is live from the first step
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "D_fc2" in n:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    model = model.to(dev).train()
    aim_amd.register_module_hooks(model, [dict(h) for h in hooks])
    opt = build_optimizer(model, dict(cfg.optimizer))
    B, T = 2, cfg.model.backbone.num_frames
    imgs = torch.randint(0, 256, (B, 1, 3, T, 224, 224), generator=gen, dtype=torch.uint8).to(dev)
    label = torch.randint(0, cfg.model.cls_head.num_classes, (B, 1), generator=gen).to(dev)
    before = {n: digest(p) for n, p in model.named_parameters()}
    trainable = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    losses, finite = [], True
    for step in range(2):
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
    # the optimizer wrote the adapters through raw pointers: the fold must follow (weights_epoch)
    clip = imgs[:1, 0]                     # uint8 [1, 3, T, 224, 224]: the GPUNormalize hook is on the backbone
    with torch.no_grad():
        model.eval()
        y = bb(clip)
        ym = bb.merge_adapters()(clip)
    torch.cuda.synchronize()
    res = dict(losses=losses, loss_bits=[digest(torch.tensor(v, dtype=torch.float64)) for v in losses], finite=finite,
               trainable=trainable, before=before, after=after, optimizer=type(opt).__name__, backbone=type(bb).__name__,
               linear=bool(bb.linear_adapter), share=bool(bb.share_adapter), tcls=bool(bb.with_t_cls_token),
               in_place=bool(bb.grad_in_place), merged_bits=digest(ym),
               merged_rel=float((ym.double() - y.double()).norm() / y.double().norm()),
               merged_finite=bool(torch.isfinite(ym).all()))
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
