#!/usr/bin/env python3
"""Generate the SwinTransformer3D golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (no test needs it).  It loads ``mmaction/models/backbones/swin_transformer.py`` by path
with ``make_golden.load_reference()``'s stand-ins plus stub modules ``mmcv`` and ``mmcv.runner`` (``einops`` is the installed
package).  No reference source is copied: only numeric outputs are stored; weights are ``synth_params`` of
make_golden_swin2d_adapter.py (name-seeded, LayerNorms around 1, bias tables at ``TABLE_STD`` = 1) and the inputs are rebuilt
from seeds by the tests.

    python tests/golden/make_golden_swin3d.py

Writes swin3d_tiny_{a,b,c,d}.npz, swin3d_inflate.npz and reference_swin3d_configs.json (the six recipes and the three base
model files: numbers and names only), in the storage scheme of make_golden_swin2d_adapter.py: whole small tensors, ``SAMPLE``
seeded elements plus fp64 sum and sum of squares for large ones, ``shape.<name>``, ``keys``, ``trainable`` and the DropPath
factors the reference drew as ``mask.<k>`` in call order (a block in training mode with a rate above 0 draws two of B entries:
the attention branch's, then the MLP's).  All cases are 3-channel clips with patch_size (2, 4, 4).

``effect.shift`` / ``effect.bias`` / ``effect.index`` are the rel-L2 changes of the output (same weights, input and masks) when
every block's shift is set to 0 / every bias table is zeroed / every ``relative_position_index`` is transposed: the generator
refuses a case where one of them is below 7.5e-2, three times the gradient bound of the GPU test.  ``bf16_floor`` is the
``_bf16_floor`` of make_golden_swin2d_adapter.py (``_BF16Linear``, same masks): the generator refuses a case whose floor is
above the GPU test's bound, 2.5e-2.  Seeds are chosen by the reference alone.

Measured (case: effects shift / bias / index; bf16 floor and the tensor it is on):
  a (eval, seed 7100):            0.312 / 0.265 / 0.362;  1.21e-2 on layers.0.blocks.0.norm2.bias
  b (train, rate 0.5, seed 7200): 0.177 / 0.194 / 0.271;  0.88e-2 on layers.0.blocks.1.attn.relative_position_bias_table
  c (train, rate 0.2, seed 7300): 0.350 / 0.326 / 0.461;  0.98e-2 on layers.0.blocks.0.norm2.weight
  d (eval, frozen_stages=1, seed 7400): 0.152 / 0.200 / 0.278;  0.88e-2 on layers.1.blocks.1.attn.relative_position_bias_table
Every case keeps its first seed.  In a, b and c stage 0's window is not clipped in t and is shifted in t; in a, b and d stage 1's
window spans the 7 x 7 grid, so its odd block shifts t only (in d the t window is clipped to the 4 frame tokens: no shift at all
there, and the table stride differs from the window).
"""
import importlib.util
import json
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_swin2d_adapter as MG2  # noqa: E402
from make_golden_swin2d_adapter import (BOUND, DRAW, MIN_EFFECT, REF_ROOT, _bf16_floor, _rel, _replay, _store, randn,  # noqa: E402,F401
                                        sample_index, synth_params)

REF = os.path.join(REF_ROOT, "mmaction/models/backbones/swin_transformer.py")
PATCH = (2, 4, 4)
# name -> (constructor keywords, (B, frames, side), train, seed)
CASES = {
    "a": (dict(embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=(2, 7, 7), patch_norm=True, drop_path_rate=0.0), (2, 8, 56), False, 7100),
    "b": (dict(embed_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=(4, 7, 7), patch_norm=True, drop_path_rate=0.5), (2, 16, 56), True, 7200),
    "c": (dict(embed_dim=32, depths=[1, 3], num_heads=[1, 2], window_size=(3, 4, 4), patch_norm=False, drop_path_rate=0.2), (2, 12, 64), True, 7300),
    "d": (dict(embed_dim=96, depths=[2, 2], num_heads=[3, 6], window_size=(8, 7, 7), patch_norm=True, drop_path_rate=0.0, frozen_stages=1),
          (1, 8, 56), False, 7400),
}
RECIPES = ("swin_tiny_patch244_window877_kinetics400_1k.py", "swin_small_patch244_window877_kinetics400_1k.py",
           "swin_base_patch244_window877_kinetics400_1k.py", "swin_base_patch244_window877_kinetics400_22k.py",
           "swin_base_patch244_window877_kinetics600_22k.py", "swin_base_patch244_window1677_sthv2.py")
INFLATE = dict(embed_dim=32, depths=[2], num_heads=[1], window_size=(2, 4, 4), patch_norm=True)      # the inflate fixture's model
INFLATE_SIDE_2D = 7                                                                               # its 2-D checkpoint's window


def load_reference_swin3d():
    import make_golden
    make_golden.load_reference()              # timm / clip / mmaction stand-ins
    for name in ("mmcv", "mmcv.runner"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["mmcv.runner"].load_checkpoint = lambda *a, **k: None
    spec = importlib.util.spec_from_file_location("mmaction.models.backbones.swin_transformer", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def gen_case(mod, tag):
    logging.getLogger("ref").setLevel(logging.ERROR)
    kw, (B, frames, side), train, seed = CASES[tag]
    m = mod.SwinTransformer3D(patch_size=PATCH, **kw)
    m.init_weights()
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    msg = m.load_state_dict(synth_params(shapes, seed), strict=False)
    assert not msg.unexpected_keys and all(k.endswith("relative_position_index") for k in msg.missing_keys)
    m.train(train)      # (the reference's train() returns None)
    imgs = randn((B, 3, frames, side, side), seed + 1)
    drawn = sys.modules["timm.models.layers"].DropPath.drawn
    del drawn[:]
    torch.manual_seed(seed + DRAW)
    y = m(imgs)
    masks = [k.clone() for k in drawn]
    g = randn(tuple(y.shape), seed + 2)
    named = [(n, p) for n, p in m.named_parameters()]
    trainable = [(n, p) for n, p in named if p.requires_grad]
    if "frozen_stages" not in kw:
        assert len(trainable) == len(named)
    grads = torch.autograd.grad(y, [p for _, p in trainable], g)
    assert all(gr is not None for gr in grads)
    last = side // PATCH[1] // 2 ** (len(kw["depths"]) - 1)
    assert tuple(y.shape) == (B, kw["embed_dim"] * 2 ** (len(kw["depths"]) - 1), frames // PATCH[0], last, last)
    sd = m.state_dict()
    out = dict(meta=np.array([B, frames, side, seed]), names=np.array([n for n, _ in named]), keys=np.array(list(sd)),
               trainable=np.array([n for n, _ in trainable]), yshape=np.array(y.shape))
    out.update({"shape." + k: np.array(tuple(v.shape), dtype=np.int64) for k, v in sd.items()})
    _store(out, "y", y.detach(), seed * 1000 + 999)
    blocks = [blk for layer in m.layers for blk in layer.blocks]
    want = [B] * (2 * sum(1 for blk in blocks if train and getattr(blk.drop_path, "drop_prob", 0.) > 0.))
    assert [k.numel() for k in masks] == want, ([k.numel() for k in masks], want)
    if train:
        assert any((k == 0).any() for k in masks) and any((k != 0).any() for k in masks), "choose a seed whose masks drop and keep"
    for k, mk in enumerate(masks):
        out[f"mask.{k}"] = mk
    index = {n: k for k, (n, _) in enumerate(named)}
    for (n, _), gr in zip(trainable, grads):
        _store(out, "grad." + n, gr, seed * 1000 + index[n])
    worst = _bf16_floor(m, imgs, g, masks, y, grads, trainable)
    out["bf16_floor"] = np.float64(worst[1])
    print(tag, "bf16 floor", worst)
    assert worst[1] <= BOUND, f"case {tag}: the bf16 floor {worst} is above {BOUND}; choose another seed"
    # the three effects (same weights, input and masks)
    y0 = _replay(m, imgs, masks)
    assert _rel(y0, y.detach()) < 1e-6
    saved = [blk.shift_size for blk in blocks]
    for blk in blocks:
        blk.shift_size = (0, 0, 0)
    out["effect.shift"] = np.float64(_rel(_replay(m, imgs, masks), y0))
    for blk, s in zip(blocks, saved):
        blk.shift_size = s
    for blk in blocks:
        blk.attn.relative_position_index = blk.attn.relative_position_index.t().contiguous()
    out["effect.index"] = np.float64(_rel(_replay(m, imgs, masks), y0))
    for blk in blocks:
        blk.attn.relative_position_index = blk.attn.relative_position_index.t().contiguous()
    assert _rel(_replay(m, imgs, masks), y0) < 1e-6
    with torch.no_grad():
        for n, p in named:
            if n.endswith("bias_table"):
                p.zero_()
    out["effect.bias"] = np.float64(_rel(_replay(m, imgs, masks), y0))
    effects = {k: float(out["effect." + k]) for k in ("shift", "bias", "index")}
    print(tag, "effects", effects, "masks", len(masks))
    assert min(effects.values()) >= MIN_EFFECT, f"case {tag}: an effect below {MIN_EFFECT}: {effects}; choose another seed"
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, f"swin3d_tiny_{tag}.npz"), **arrays)


def inflate_checkpoint(seed=7500):
    """the synthetic 2-D Swin checkpoint of the inflate fixture: the names of a two-block stage, its 2-D bias tables of side
    2 * INFLATE_SIDE_2D - 1 (another side than the model's: the bicubic branch runs), and the buffers inflate_weights drops"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen)
    C = INFLATE["embed_dim"]
    sd = {"patch_embed.proj.weight": r(C, 3, 4, 4), "patch_embed.proj.bias": r(C), "patch_embed.norm.weight": r(C), "patch_embed.norm.bias": r(C)}
    for j in range(2):
        p = f"layers.0.blocks.{j}."
        sd[p + "attn.relative_position_bias_table"] = r((2 * INFLATE_SIDE_2D - 1) ** 2, 1)
        sd[p + "attn.relative_position_index"] = torch.zeros((INFLATE_SIDE_2D ** 2,) * 2, dtype=torch.long)
        sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"] = r(3 * C, C), r(3 * C)
        sd[p + "mlp.fc1.weight"] = r(4 * C, C)
        if j:
            sd[p + "attn_mask"] = torch.zeros((4, INFLATE_SIDE_2D ** 2, INFLATE_SIDE_2D ** 2))
    sd["head.weight"] = r(5, C)
    return sd


def gen_inflate(mod):
    """swin3d_inflate.npz: what the reference's inflate_weights makes of ``inflate_checkpoint()``, and one buffer"""
    import tempfile
    m = mod.SwinTransformer3D(patch_size=PATCH, pretrained2d=True, **INFLATE)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "swin2d.pth")
        torch.save({"model": inflate_checkpoint()}, path)
        m.pretrained = path
        m.inflate_weights(logging.getLogger("ref"))
    out = {"sd." + k: v.detach().numpy() for k, v in m.state_dict().items() if not k.endswith("relative_position_index")}
    out["index.233"] = mod.WindowAttention3D(32, (2, 3, 3), 1).relative_position_index.numpy()
    np.savez_compressed(os.path.join(HERE, "swin3d_inflate.npz"), **out)


def gen_configs():
    """reference_swin3d_configs.json: the six recipes and their ``_base_`` files, in the format of reference_vit_configs.json"""
    from aim_amd.registry import _load_py
    from make_golden import CFG_KEYS, _cfg_data
    cfg_root = os.path.join(REF_ROOT, "configs")
    todo = [os.path.join(cfg_root, "recognition", "swin", r) for r in RECIPES]
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
    with open(os.path.join(HERE, "reference_swin3d_configs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    torch.set_num_threads(8)
    gen_configs()
    mod = load_reference_swin3d()
    gen_inflate(mod)
    for tag in (sys.argv[1:] or CASES):
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
