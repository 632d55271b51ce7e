#!/usr/bin/env python3
"""Generate the ViT_ImageNet golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (it is not needed by any test).  It loads
``mmaction/models/backbones/vit_imagenet.py`` by path with ``make_golden.load_reference()``'s stand-ins, plus an empty
``turtle`` module (the reference file's unused ``from turtle import forward`` needs tkinter).  No reference source is
copied: only the reference's numeric outputs are stored; the inputs and weights are rebuilt from seeds
(``synth_params`` / ``randn``, CPU generators, shared with the tests).

    python tests/golden/make_golden_imagenet.py

Writes vit_imagenet_tiny_{a,b,c}.npz and reference_vit_imagenet_configs.json.  Geometry: img 32, patch 16, D 128, H 2,
depth 3, B 2.  Gradients of more than ``WHOLE`` elements are stored as ``SAMPLE`` elements at seeded positions
(``sample_index``) plus their fp64 sum and sum of squares, to keep each file small; every parameter's shape is stored
(``shape.<name>``).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_ROOT = "/root/reference"
REF = os.path.join(REF_ROOT, "mmaction/models/backbones/vit_imagenet.py")

GEOM = dict(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2)
B = 2
WHOLE, SAMPLE = 2048, 1024
# name -> (T, train, constructor keywords beyond GEOM, seed)
CASES = {
    "a": (2, False, dict(num_tadapter=1), 3100),
    "b": (4, True, dict(num_tadapter=2, drop_path_rate=0.5, adapter_scale=0.5), 3200),
    "c": (2, False, dict(num_tadapter=1, qkv_bias=False, patch_embedding_bias=False), 3300),
}


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def synth_params(shapes, seed):
    """Name-ordered synthetic weights: LayerNorm weights 1 + 0.1 n, biases and embeddings 0.05 n / 0.1 n, matrices
    n / sqrt(fan_in) / 2 (every adapter's D_fc2 non-zero, so its gradient path is exercised)."""
    out = {}
    for k, (name, shape) in enumerate(shapes):
        n = randn(shape, seed * 1000 + k)
        if name.endswith(".weight") and len(shape) == 1:
            v = 1.0 + 0.1 * n
        elif name.endswith(".bias"):
            v = 0.05 * n
        elif name in ("cls_token", "pos_embed", "temporal_embedding"):
            v = 0.1 * n
        else:
            fan_in = int(np.prod(shape[1:]))
            v = n / (2.0 * fan_in ** 0.5)
        out[name] = v
    return out


def sample_index(numel, seed):
    return torch.randperm(numel, generator=torch.Generator().manual_seed(seed))[:SAMPLE]


def load_reference_imagenet():
    sys.path.insert(0, HERE)
    import make_golden
    make_golden.load_reference()              # timm / clip / mmaction stand-ins
    sys.modules.setdefault("turtle", types.ModuleType("turtle")).forward = None
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmaction.models.backbones.vit_imagenet", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def gen_case(mod, tag):
    import logging
    logging.getLogger("ref").setLevel(logging.ERROR)
    T, train, kw, seed = CASES[tag]
    m = mod.ViT_ImageNet(num_frames=T, **GEOM, **kw)
    m.init_weights()
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    assert all(p.requires_grad for p in m.parameters())
    msg = m.load_state_dict(synth_params(shapes, seed), strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    m.train() if train else m.eval()
    imgs = randn((B, 3, T, GEOM["img_size"], GEOM["img_size"]), seed + 1)
    g = randn((B, GEOM["embed_dim"], T, 1, 1), seed + 2)
    drawn = sys.modules["timm.models.layers"].DropPath.drawn
    del drawn[:]
    torch.manual_seed(seed + 9)
    y = m(imgs)
    masks = list(drawn)
    grads = torch.autograd.grad(y, [p for _, p in m.named_parameters()], g)
    out = dict(y=y.detach(), meta=np.array([GEOM["embed_dim"], GEOM["num_heads"], GEOM["depth"], B, T, seed]),
               names=np.array([n for n, _ in shapes]))
    out.update({"shape." + n: np.array(sh, dtype=np.int64) for n, sh in shapes})      # every parameter's shape
    if train:
        assert len(masks) == 4 and all(k.shape == (B * T,) for k in masks) and any((k == 0).any() for k in masks)
        out["masks"] = torch.stack(masks)
    for k, ((n, _), gr) in enumerate(zip(shapes, grads)):
        if gr.numel() <= WHOLE:
            out["grad." + n] = gr
        else:
            flat = gr.reshape(-1)
            out["grad." + n + ".val"] = flat[sample_index(flat.numel(), seed * 1000 + k)]
            out["grad." + n + ".sum"] = flat.double().sum()
            out["grad." + n + ".sq"] = (flat.double() ** 2).sum()
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, f"vit_imagenet_tiny_{tag}.npz"), **arrays)


def gen_configs():
    """reference_vit_imagenet_configs.json: the two vit_imagenet_*.py configs and their ``_base_`` files, in the format of
    reference_vit_configs.json (make_golden.gen_configs)."""
    import json
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from aim_amd.registry import _load_py
    from make_golden import CFG_KEYS, _cfg_data
    cfg_root = os.path.join(REF_ROOT, "configs")
    todo = [os.path.join(cfg_root, "recognition", "vit", f) for f in ("vit_imagenet_k400.py", "vit_imagenet_ssv2.py")]
    out = {}
    while todo:
        path = os.path.normpath(todo.pop(0))
        rel = os.path.relpath(path, cfg_root)
        if rel in out:
            continue
        d = {k: v for k, v in _load_py(path).items() if k in CFG_KEYS}
        out[rel] = _cfg_data(d)
        bases = d.get("_base_", [])
        todo += [os.path.join(os.path.dirname(path), b) for b in ([bases] if isinstance(bases, str) else bases)]
    with open(os.path.join(HERE, "reference_vit_imagenet_configs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    torch.set_num_threads(8)
    gen_configs()
    mod = load_reference_imagenet()
    for tag in CASES:
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
