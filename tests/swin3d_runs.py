"""The GPU runs of tests/test_swin3d_gpu.py, one child process each: `python swin3d_runs.py WHAT OUT.json` with
WHAT = fixture:<a|b|c|d> | bitwise | recipe.  A plain module (no fixtures); the test file starts the children one after the
other, each under its own timeout, stops at the first that fails and reads the records."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from swin2d_adapter_runs import against  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_swin3d", os.path.join(GOLDEN, "make_golden_swin3d.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)


def build(tag, dev, **override):
    import aim_amd
    kw, clip, train, seed = MG.CASES[tag]
    kw = dict(kw, **override)
    m = aim_amd.SwinTransformer3D(patch_size=MG.PATCH, **kw)
    m.init_weights()
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    m.load_state_dict(MG.synth_params(shapes, seed), strict=False)
    return m.to(dev).train(train), kw, clip, train, seed


def inject_masks(m, z, dev):
    """the reference's drawn factors, in its call order, as what ``_drop_factors`` returns"""
    masks = [torch.from_numpy(z[f"mask.{k}"]).to(dev) for k in range(sum(1 for key in z.files if key.startswith("mask.")))]
    out, it = [], iter(masks)
    for blk in m._blocks():
        if not blk.training or blk.drop_prob == 0.0:
            out.append((None, None))
        else:
            f1 = next(it)
            out.append((f1, next(it)))
    assert next(it, None) is None
    m._drop_factors = lambda B, dev_: out


def inputs(tag, z, dev):
    kw, (B, frames, side), train, seed = MG.CASES[tag]
    imgs = MG.randn((B, 3, frames, side, side), seed + 1).to(dev)
    g = MG.randn(tuple(int(v) for v in z["yshape"]), seed + 2).to(dev)
    return imgs, g


def run_fixture(tag, dev):
    z = np.load(os.path.join(GOLDEN, f"swin3d_tiny_{tag}.npz"))
    m, kw, clip, train, seed = build(tag, dev)
    inject_masks(m, z, dev)
    imgs, g = inputs(tag, z, dev)
    names = [n for n, _ in m.named_parameters()]
    assert names == [str(n) for n in z["names"]]
    trainable = [str(n) for n in z["trainable"]]
    assert [n for n, p in m.named_parameters() if p.requires_grad] == trainable
    y = m(imgs)
    assert tuple(y.shape) == tuple(int(v) for v in z["yshape"])
    y.backward(g)
    grads = {n: p.grad for n, p in m.named_parameters()}
    errs, zeros = {}, {}
    against(z, "y", y.detach(), seed * 1000 + 999, errs, zeros)
    for k, n in enumerate(names):
        if n in trainable:
            assert grads[n] is not None, n
            against(z, "grad." + n, grads[n], seed * 1000 + k, errs, zeros)
    rec = {"errs": errs, "zeros": zeros, "none": [n for n in names if grads[n] is None],
           "frozen": [n for n in names if n not in trainable], "finite": all(bool(torch.isfinite(v).all()) for v in grads.values() if v is not None)}
    if "frozen_stages" in kw:          # the same model with nothing frozen, in the same mode: the rest keep their bits
        full, _, _, _, _ = build(tag, dev, frozen_stages=-1)
        full.train(train)
        full(imgs).backward(g)
        fg = {n: p.grad for n, p in full.named_parameters()}
        rec["frozen_none_rest_same_bits"] = all((grads[n] is None) if n not in trainable else torch.equal(grads[n], fg[n]) for n in names)
        rec["full_has_all"] = all(v is not None for v in fg.values())
    return rec


def run_bitwise(dev):
    """case b (train mode, stored masks): the no-grad forward against the grad-mode forward, two backwards"""
    z = np.load(os.path.join(GOLDEN, "swin3d_tiny_b.npz"))
    m, kw, clip, train, seed = build("b", dev)
    inject_masks(m, z, dev)
    imgs, g = inputs("b", z, dev)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        y = m(imgs)
        y.backward(g)
        runs.append((y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    with torch.no_grad():
        y0 = m(imgs)
    return {"no_grad_forward_same_bits": bool(torch.equal(y0, runs[0][0])), "second_forward_same_bits": bool(torch.equal(runs[0][0], runs[1][0])),
            "second_backward_same_bits": all(bool(torch.equal(runs[0][1][n], runs[1][1][n])) for n in runs[0][1]),
            "tensors": len(runs[0][1])}


def write_config_tree(root):
    with open(os.path.join(GOLDEN, "reference_swin3d_configs.json")) as f:
        configs = json.load(f)

    def value(o):
        if isinstance(o, dict):
            if set(o) == {"__tuple__"}:
                return tuple(value(v) for v in o["__tuple__"])
            return {k: value(v) for k, v in o.items()}
        if isinstance(o, list):
            return [value(v) for v in o]
        return o

    for r, d in configs.items():
        path = os.path.join(root, r)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {value(v)!r}\n")
    return sorted(r for r in configs if r.startswith("recognition"))


K400_BASE = "recognition/swin/swin_base_patch244_window877_kinetics400_1k.py"


def run_recipe(dev, tmp):
    """three FlatAdamW steps of the k400 base recipe reduced to depths [2, 2, 2, 2], 1 clip of 8 frames of 224 x 224; twice"""
    import aim_amd
    from aim_amd.dist import build_optimizer
    write_config_tree(tmp)
    cfg = aim_amd.Config.fromfile(os.path.join(tmp, K400_BASE))
    cfg.merge_from_dict({"model.backbone.depths": [2, 2, 2, 2]})

    def train():
        torch.manual_seed(0)
        model = aim_amd.build_model(cfg.model)
        model.backbone.init_weights()
        model = model.to(dev).train()
        opt = build_optimizer(model, dict(cfg.optimizer))
        before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        gen = torch.Generator().manual_seed(9)
        imgs = torch.randn((1, 1, 3, 8, 224, 224), generator=gen).to(dev)
        label = torch.randint(0, 400, (1, 1), generator=gen).to(dev)
        torch.manual_seed(3); torch.cuda.manual_seed(3)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = model(imgs, label, return_loss=True)["loss_cls"]
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        after = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        want = {n for n, p in model.named_parameters() if p.requires_grad}
        return torch.stack(losses).cpu(), before, after, want, type(opt).__name__

    l1, b1, a1, want, opt_name = train()
    l2, _, a2, _, _ = train()
    changed = {n for n in a1 if not torch.equal(a1[n], b1[n])}
    return {"optimizer": opt_name, "losses": [float(v) for v in l1], "finite": bool(torch.isfinite(l1).all()),
            "params_finite": all(bool(torch.isfinite(v).all()) for v in a1.values()),
            "unchanged_trainable": sorted(want - changed), "changed_frozen": sorted(changed - want), "trainable": len(want),
            "same_bits": bool(torch.equal(l1, l2)) and all(bool(torch.equal(a1[n], a2[n])) for n in a1)}


def main(argv):
    what, path = argv
    dev = torch.device("cuda:0")
    if what.startswith("fixture:"):
        rec = run_fixture(what.split(":")[1], dev)
    elif what == "bitwise":
        rec = run_bitwise(dev)
    elif what == "recipe":
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            rec = run_recipe(dev, tmp)
    else:
        raise SystemExit(f"unknown run {what}")
    with open(path, "w") as f:
        json.dump(rec, f)


if __name__ == "__main__":
    main(sys.argv[1:])
