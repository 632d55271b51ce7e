#!/usr/bin/env python3
"""Generate tests/golden/blending_ref.npz from the REAL reference's mini-batch blendings and cross-entropy loss.

Needs a checkout of the reference (adapt-image-models), passed as the only argument.  Like ``make_golden.load_reference()`` it loads
``mmaction/datasets/blending_utils.py``, ``mmaction/models/losses/base.py`` and ``cross_entropy_loss.py`` by path behind
stand-in registries.  No reference source is copied: only inputs, the random draws the reference made (recorded through a
thin wrapper of its ``torch`` and ``Beta.sample`` calls) and its numeric outputs are stored.

    python tests/golden/make_golden_blending.py <reference checkout>

Contents (``<case>.<field>``):
  blend cases  -- ``seed`` (torch.manual_seed right before the call), ``shape`` (the clips: ``clip_input(shape, seed)``),
                  ``label``, ``num_classes``, ``alpha``,
                  ``smoothing``, ``kind`` (0 LabelSmoothing, 1 Mixup, 2 Cutmix), the draws ``order`` (1 randperm, 2 Beta
                  sample, 3 randint, in call order), ``lam`` (the Beta sample), ``perm``, ``box`` (x1, y1, x2, y2; Cutmix),
                  and the outputs ``out_label`` and (Mixup / Cutmix) ``out_imgs`` (clips of more than 20000 values: ``out_imgs_sha256``, the
                  digest of their little-endian f32 bytes).
  loss cases   -- ``score``, ``label`` (hard int64 or soft f32), ``weight`` (empty: none), ``loss`` and ``grad``
                  (torch.autograd of the reference's CrossEntropyLoss w.r.t. the score).
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "blending_ref.npz")


class _Reg:
    def register_module(self, *a, **k):
        return lambda c: c


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    src = os.path.join(ref_root, "mmaction")
    for pkg in ("mmaction", "mmaction.datasets", "mmaction.models", "mmaction.models.losses"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    b = types.ModuleType("mmaction.datasets.builder")
    b.BLENDINGS = _Reg()
    sys.modules[b.__name__] = b
    mb = types.ModuleType("mmaction.models.builder")
    mb.LOSSES = _Reg()
    sys.modules[mb.__name__] = mb
    blend = _load("mmaction.datasets.blending_utils", os.path.join(src, "datasets", "blending_utils.py"))
    _load("mmaction.models.losses.base", os.path.join(src, "models", "losses", "base.py"))
    ce = _load("mmaction.models.losses.cross_entropy_loss", os.path.join(src, "models", "losses", "cross_entropy_loss.py"))
    return blend, ce


class _Recorder:
    """Stands in for the ``torch`` module inside the reference's blending file: forwards everything, records the draws."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def randperm(self, *a, **k):
        r = torch.randperm(*a, **k)
        self.log.append(("randperm", r.clone()))
        return r

    def randint(self, *a, **k):
        r = torch.randint(*a, **k)
        self.log.append(("randint", r.clone()))
        return r

    def clamp(self, *a, **k):
        r = torch.clamp(*a, **k)
        self.log.append(("clamp", r.clone()))
        return r


def blend_case(mod, kind, shape, num_classes, alpha, smoothing, seed):
    imgs, g = clip_input(shape, seed)
    label = torch.randint(0, num_classes, (shape[0], 1), generator=g)
    cls = {0: mod.LabelSmoothing, 1: mod.MixupBlending, 2: mod.CutmixBlending}[kind]
    obj = cls(num_classes, smoothing=smoothing) if kind == 0 else cls(num_classes, alpha, smoothing=smoothing)
    rec = _Recorder()
    if kind:
        real = obj.beta.sample

        def sample(*a, **k):
            r = real(*a, **k)
            rec.log.append(("beta", r.clone()))
            return r
        obj.beta.sample = sample
    mod.torch = rec
    try:
        torch.manual_seed(seed)
        out_imgs, out_label = obj(imgs.clone(), label)
    finally:
        mod.torch = torch
    code = {"randperm": 1, "beta": 2, "randint": 3}
    order = [code[k] for k, _ in rec.log if k in code]
    get = lambda k: [v for n, v in rec.log if n == k]     # noqa: E731
    lam = get("beta")[0].numpy() if kind else np.zeros((), np.float32)
    perm = get("randperm")[0].numpy() if kind else np.zeros((0,), np.int64)
    box = np.array([int(v) for v in get("clamp")], np.int64)[[0, 1, 2, 3]] if kind == 2 else np.zeros((0,), np.int64)
    d = dict(seed=np.int64(seed), shape=np.array(shape, np.int64), label=label.numpy(), num_classes=np.int64(num_classes),
             alpha=np.float64(alpha), smoothing=np.float64(smoothing), kind=np.int64(kind), order=np.array(order, np.int64),
             lam=lam, perm=perm, box=box, out_label=out_label.numpy())
    assert torch.equal(imgs, clip_input(shape, seed)[0])
    if kind == 0:
        assert torch.equal(out_imgs, imgs)     # LabelSmoothing passes the clips through
    elif out_imgs.numel() <= 20000:
        d["out_imgs"] = out_imgs.numpy()
    else:               # the reference tests' full-size clips: the exact bytes, by digest (keeps the fixture small)
        d["out_imgs_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(out_imgs.numpy(), "<f4").tobytes()).hexdigest())
    return d


def clip_input(shape, seed):
    """The clips of a blend case, rebuilt from its seed (tests/test_blending_cpu.py does the same)."""
    g = torch.Generator().manual_seed(int(seed) + 1000)
    return torch.randn(tuple(int(v) for v in shape), generator=g), g


def loss_case(ce, score, label, weight):
    loss_fn = ce.CrossEntropyLoss(class_weight=None if weight is None else weight.numpy().tolist())
    s = score.clone().requires_grad_(True)
    loss = loss_fn(s, label)
    loss.backward()
    return dict(score=score.numpy(), label=label.numpy(), weight=np.zeros((0,), np.float32) if weight is None else weight.numpy(),
                loss=loss.detach().numpy(), grad=s.grad.numpy())


def main(ref_root):
    blend, ce = load_reference(ref_root)
    out = {}

    def put(name, d):
        for k, v in d.items():
            out[f"{name}.{k}"] = np.asarray(v)

    # the shapes of the reference's tests/test_data/test_blending.py (4-D per segment and 6-D), plus a non-square clip
    shapes = {"nchw": (4, 4, 3, 32, 32), "ncthw": (4, 4, 2, 3, 32, 32), "odd": (3, 2, 3, 2, 12, 20)}
    seed = 11
    for kind, kname in ((1, "mixup"), (2, "cutmix"), (0, "smooth")):
        for sname, shape in shapes.items():
            for smoothing in (0.0, 0.1):
                seed += 1
                put(f"blend_{kname}_{sname}_s{int(smoothing * 10)}", blend_case(blend, kind, shape, 10, 0.2, smoothing, seed))
    # alpha = 1 (a wide Beta: large boxes) and the sthv2 recipes' LabelSmoothing(num_classes=174, smoothing=0.1)
    put("blend_cutmix_alpha1", blend_case(blend, 2, (5, 1, 3, 2, 16, 24), 10, 1.0, 0.0, 101))
    put("blend_mixup_alpha1", blend_case(blend, 1, (5, 1, 3, 2, 16, 24), 10, 1.0, 0.0, 102))
    put("blend_smooth_sthv2", blend_case(blend, 0, (4, 1, 3, 2, 16, 16), 174, 0.2, 0.1, 103))

    g = torch.Generator().manual_seed(7)
    # tests/test_metrics/test_losses.py:82-116
    score = torch.rand((3, 4), generator=g)
    hard = torch.LongTensor([0, 1, 2])
    soft = torch.FloatTensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
    weight = torch.rand(4, generator=g)
    put("loss_soft", loss_case(ce, score, soft, None))
    put("loss_soft_w", loss_case(ce, score, soft, weight))
    put("loss_hard_w", loss_case(ce, score, hard, weight))
    # a 174-class batch through the sthv2 LabelSmoothing, with and without class weights
    score = torch.randn((8, 174), generator=g) * 3
    lab = torch.randint(0, 174, (8, 1), generator=g)
    ls = blend.LabelSmoothing(174, smoothing=0.1)
    _, sm = ls(torch.zeros((8, 1)), lab)
    w174 = torch.rand(174, generator=g) + 0.5
    put("loss_smooth174", loss_case(ce, score, sm, None))
    put("loss_smooth174_w", loss_case(ce, score, sm, w174))
    # mixed two-hot rows (Mixup-style) and hard labels with an ignored row (-100, F.cross_entropy's ignore_index)
    score = torch.randn((5, 10), generator=g)
    mix = torch.zeros((5, 10))
    mix[torch.arange(5), torch.tensor([1, 3, 5, 7, 9])] += 0.7
    mix[torch.arange(5), torch.tensor([2, 3, 0, 8, 4])] += 0.3
    put("loss_mix_w", loss_case(ce, score, mix, torch.rand(10, generator=g) + 0.1))
    score = torch.randn((6, 7), generator=g)
    put("loss_hard_w_ignore", loss_case(ce, score, torch.LongTensor([0, 6, -100, 3, 3, 1]), torch.rand(7, generator=g) + 0.1))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
