"""Child process of tests/test_zeroi2v_gpu.py: two training steps of the sthv2 ZeroI2V recipe (stored values, pretrained=None)
on uint8 clips through the GPUNormalize hook, LabelSmoothing and build_optimizer; writes the losses and a digest of every
parameter before and after.  The stream switches (AIM_SIDE_STREAM, AIM_DETACH_WGRAD, AIM_DETACH_BIG) are read when the
package is imported, hence one process per setting:  python zeroi2v_train_child.py <result.json>"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
RECIPE = "recognition/vit/zeroI2V/vitclip_zeroI2V_base_sthv2.py"
HOOKS_FROM = "recognition/vit/zeroI2V/vitclip_zeroI2V_base_diving48.py"      # (sthv2 normalises in its CPU pipeline)


def _value(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_value(v) for v in o["__tuple__"])
        return {k: _value(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_value(v) for v in o]
    return o


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


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
    cfg.merge_from_dict({"model.backbone.pretrained": None})
    hooks = cfg.get("module_hooks") or aim_amd.Config.fromfile(os.path.join(root, HOOKS_FROM)).module_hooks
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
    aim_amd.register_module_hooks(model, [dict(h) for h in hooks])
    opt = build_optimizer(model, dict(cfg.optimizer))
    B, T = 2, cfg.model.backbone.num_frames
    imgs = torch.randint(0, 256, (B, 1, 3, T, 224, 224), generator=gen, dtype=torch.uint8).to(dev)
    label = torch.randint(0, cfg.model.cls_head.num_classes, (B, 1), generator=gen).to(dev)
    before = {n: digest(p) for n, p in model.named_parameters()}
    trainable = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
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
    res = dict(losses=losses, loss_bits=[digest(torch.tensor(v, dtype=torch.float64)) for v in losses], finite=finite,
               trainable=trainable, before=before, after=after, optimizer=type(opt).__name__,
               backbone=type(model.backbone).__name__, blending=type(model.blending).__name__,
               in_place=bool(model.backbone.grad_in_place))
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
