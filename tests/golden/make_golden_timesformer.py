#!/usr/bin/env python3
"""Generate the TimeSformer golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (it is not needed by any test).  It loads
``mmaction/models/backbones/timesformer.py`` by path with ``make_golden.load_reference()``'s stand-ins.  No reference source is
copied: only the reference's numeric outputs are stored; the inputs and weights are rebuilt from seeds (``synth_params`` here,
``randn`` / ``sample_index`` of make_golden_imagenet.py, CPU generators, shared with the tests).

    python tests/golden/make_golden_timesformer.py

Writes timesformer_tiny_{a,b,c}.npz and reference_timesformer_configs.json.  Geometry: resolution 32, patch 16, width 128,
2 heads, 3 layers, B 2.  Case b trains with drop_path_rate 0.5: the six masks the reference's DropPath drew (layers 1 and 2,
three each, of shapes (T,), (N,), (N,)) are stored as ``mask.<k>`` (the factors: 0 or 1 / keep); the seed of the draws is
chosen so that every one of them keeps an entry and drops an entry.  Gradients of more than ``WHOLE`` elements are stored as
``SAMPLE`` elements at seeded positions plus their fp64 sum and sum of squares; every parameter's shape is stored
(``shape.<name>``).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden_imagenet import REF_ROOT, WHOLE, randn, sample_index      # noqa: E402

REF = os.path.join(REF_ROOT, "mmaction/models/backbones/timesformer.py")

GEOM = dict(input_resolution=32, patch_size=16, width=128, layers=3, heads=2)
B = 2
# name -> (T, train, constructor keywords beyond GEOM, seed)
CASES = {
    "a": (2, False, dict(drop_path_rate=0.0), 4100),
    "b": (4, True, dict(drop_path_rate=0.5), 4200),
    "c": (2, False, dict(drop_path_rate=0.0, attn_type='space'), 4300),
}
DRAW = 10        # torch's global seed for the DropPath draws is seed + DRAW: the first offset from 9 up at which case b's six masks
                 # each keep an entry and drop an entry (asserted in gen_case)
_EMBEDDINGS = ("class_embedding", "positional_embedding", "temporal_embedding")


def synth_params(shapes, seed):
    """Name-ordered synthetic weights: LayerNorm weights 1 + 0.1 n, biases 0.05 n, embeddings 0.1 n, matrices (the conv and
    ``T_Adapter`` included) n / sqrt(fan_in) / 2: nothing is zero, so every gradient path is exercised."""
    out = {}
    for k, (name, shape) in enumerate(shapes):
        n = randn(shape, seed * 1000 + k)
        if name in _EMBEDDINGS:
            v = 0.1 * n
        elif name.endswith("bias"):
            v = 0.05 * n
        elif len(shape) == 1:
            v = 1.0 + 0.1 * n
        else:
            v = n / (2.0 * int(np.prod(shape[1:])) ** 0.5)
        out[name] = v
    return out


def load_reference_timesformer():
    import make_golden
    make_golden.load_reference()              # timm / clip / mmaction stand-ins
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmaction.models.backbones.timesformer", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def gen_case(mod, tag):
    import logging
    logging.getLogger("ref").setLevel(logging.ERROR)
    T, train, kw, seed = CASES[tag]
    m = mod.TimeSformer(num_frames=T, **GEOM, **kw)
    m.init_weights()
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    L = GEOM["layers"]
    assert all(p.requires_grad for p in m.parameters())
    assert len(shapes) == 6 + 20 * L + 2 - (kw.get("attn_type", "tadapter") != "tadapter")
    msg = m.load_state_dict(synth_params(shapes, seed), strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    m.train() if train else m.eval()
    res = GEOM["input_resolution"]
    N = (res // GEOM["patch_size"]) ** 2 + 1
    imgs = randn((B, 3, T, res, res), seed + 1)
    g = randn((B, GEOM["width"], T, 1, 1), seed + 2)
    drawn = sys.modules["timm.models.layers"].DropPath.drawn
    del drawn[:]
    torch.manual_seed(seed + DRAW)
    y = m(imgs)
    masks = list(drawn)
    grads = torch.autograd.grad(y, [p for _, p in m.named_parameters()], g)
    assert all(gr is not None for gr in grads)
    out = dict(y=y.detach(), meta=np.array([GEOM["width"], GEOM["heads"], L, B, T, seed]), names=np.array([n for n, _ in shapes]))
    out.update({"shape." + n: np.array(sh, dtype=np.int64) for n, sh in shapes})      # every parameter's shape
    if train:
        assert [tuple(k.shape) for k in masks] == [(T,), (N,), (N,)] * (L - 1), [tuple(k.shape) for k in masks]
        assert all((k == 0).any() and (k != 0).any() for k in masks), "choose a seed whose masks all keep and drop an entry"
        for k, mk in enumerate(masks):
            out[f"mask.{k}"] = mk
    else:
        assert not masks
    for k, ((n, _), gr) in enumerate(zip(shapes, grads)):
        if gr.numel() <= WHOLE:
            out["grad." + n] = gr
        else:
            flat = gr.reshape(-1)
            out["grad." + n + ".val"] = flat[sample_index(flat.numel(), seed * 1000 + k)]
            out["grad." + n + ".sum"] = flat.double().sum()
            out["grad." + n + ".sq"] = (flat.double() ** 2).sum()
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, f"timesformer_tiny_{tag}.npz"), **arrays)


def gen_configs():
    """reference_timesformer_configs.json: timesformer_k400.py and its ``_base_`` files, in the format of
    reference_vit_configs.json (make_golden.gen_configs)."""
    import json
    sys.path.insert(0, ROOT)
    from aim_amd.registry import _load_py
    from make_golden import CFG_KEYS, _cfg_data
    cfg_root = os.path.join(REF_ROOT, "configs")
    todo = [os.path.join(cfg_root, "recognition", "vit", "timesformer_k400.py")]
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
    with open(os.path.join(HERE, "reference_timesformer_configs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    torch.set_num_threads(8)
    gen_configs()
    mod = load_reference_timesformer()
    for tag in CASES:
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
