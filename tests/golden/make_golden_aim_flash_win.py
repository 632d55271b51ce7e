#!/usr/bin/env python3
"""Generate the AIM_FLASH_WIN golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (no test needs it).  It loads ``mmaction/models/backbones/vitclip_aim_flash_win.py``
by path with ``make_golden.load_reference()``'s stand-ins (``einops`` is the installed package) and two more, for the
``flash_attn`` package that is not installed: ``flash_attn.modules.mha.MHA`` (``Wqkv``, ``out_proj``,
softmax(Q K^T / sqrt(dh)) V with the q | k | v head-major split) and ``flash_attn.modules.mlp.Mlp`` (``fc1``, activation,
``fc2``).  THE ATTENTION AND MLP ARITHMETIC OF THESE FIXTURES IS THOSE FEW LINES BELOW (``_MHA.forward``, ``_Mlp.forward``),
not flash_attn's kernels; the block wiring, the window partition and its reverse, the class-token attention, the prompt
token, the three DropPath draws per block and the readout are the reference's own code.  No reference source is copied:
only numeric outputs are stored; weights are ``oracle.synth_state_dict`` of the parameter shapes (name-seeded: every
``D_fc2`` and the ``temporal_embedding`` are non-zero) and the inputs are rebuilt from seeds by the tests.

    python tests/golden/make_golden_aim_flash_win.py

Writes aim_flash_win_tiny_{a,b,c,d,e}.npz and reference_aim_flash_win_configs.json.  Geometry: img 64, patch 16 (G = 4,
N = 17), head width 64, B = 2.  Gradients of more than ``WHOLE`` elements are stored as ``SAMPLE`` elements at seeded
positions plus their fp64 sum and sum of squares (as make_golden_imagenet.py), every parameter's shape as ``shape.<name>``,
the DropPath factors the reference drew as ``mask.<k>`` in call order (three of B T entries per block with rate > 0).
``window_effect`` / ``prompt_effect`` are the rel-L2 changes of the output when the window partition is replaced by
per-frame windows (wt = 1) / the prompt token is removed: the generator refuses a case where either is below 7.5e-2 (five
times the bf16 output bound of the GPU test), so that a backbone that ignores either cannot pass.
"""
import importlib.util
import logging
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_ROOT = "/root/reference"
REF = os.path.join(REF_ROOT, "mmaction/models/backbones/vitclip_aim_flash_win.py")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_imagenet import SAMPLE, WHOLE, randn, sample_index  # noqa: E402

IMG, PATCH, B = 64, 16, 2
# name -> (T, window, width, heads, layers, train, prompt, seed)
CASES = {
    "a": (4, (2, 2, 2), 128, 2, 3, True, True, 5100),
    "b": (8, (8, 1, 1), 128, 2, 2, False, True, 5214),      # (5200, 5207: prompt effect 0.052 < MIN_EFFECT)
    "c": (4, (16, 7, 7), 192, 3, 2, False, True, 5300),
    "d": (6, (3, 2, 4), 128, 2, 2, False, True, 5400),
    "e": (4, (2, 2, 2), 128, 2, 3, False, False, 5100),
}
DROP_RATE = 0.5
MIN_EFFECT = 7.5e-2


class _MHA(nn.Module):
    """stand-in for flash_attn.modules.mha.MHA at the reference's call (self-attention, no dropout, no rotary)"""

    def __init__(self, embed_dim, num_heads, cross_attn=False, dropout=0., use_flash_attn=False, **kw):
        super().__init__()
        assert not cross_attn and dropout == 0.
        self.num_heads = num_heads
        self.Wqkv = nn.Linear(embed_dim, 3 * embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)

    def forward(self, x):
        Nb, S, D = x.shape
        H = self.num_heads
        qkv = self.Wqkv(x).view(Nb, S, 3, H, D // H).permute(2, 0, 3, 1, 4)
        p = (qkv[0] @ qkv[1].transpose(-2, -1) / (D // H) ** 0.5).softmax(dim=-1)
        return self.out_proj((p @ qkv[2]).permute(0, 2, 1, 3).reshape(Nb, S, D))


class _Mlp(nn.Module):
    """stand-in for flash_attn.modules.mlp.Mlp"""

    def __init__(self, in_features, hidden_features=None, out_features=None, activation=None, **kw):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.activation = activation
        self.fc2 = nn.Linear(hidden_features, out_features or in_features)

    def forward(self, x):
        return self.fc2(self.activation(self.fc1(x)))


def load_reference_flash_win():
    import make_golden
    make_golden.load_reference()              # timm / clip / mmaction stand-ins
    for name in ("flash_attn", "flash_attn.modules"):
        sys.modules[name] = types.ModuleType(name)
    mha, mlp = types.ModuleType("flash_attn.modules.mha"), types.ModuleType("flash_attn.modules.mlp")
    mha.MHA, mlp.Mlp = _MHA, _Mlp
    sys.modules[mha.__name__], sys.modules[mlp.__name__] = mha, mlp
    spec = importlib.util.spec_from_file_location("mmaction.models.backbones.vitclip_aim_flash_win", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def _build(mod, T, window, D, H, L, train, prompt, st):
    m = mod.AIM_FLASH_WIN(IMG, T, PATCH, D, L, H, drop_path_rate=DROP_RATE if train else 0.0, adapter_scale=0.5,
                          use_flash_attn=False, prompt=prompt, wind_attn=True, window_size=window, not_shift=True)
    m.init_weights()
    msg = m.load_state_dict(st, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    return m.train() if train else m.eval()


def gen_case(mod, tag):
    import aim_flash_win_ref as R
    from oracle import vit_clip_oracle as O
    logging.getLogger("ref").setLevel(logging.ERROR)
    T, window, D, H, L, train, prompt, seed = CASES[tag]
    st = O.synth_state_dict(R.backbone_param_shapes(IMG, T, PATCH, D, L), seed=seed)
    assert float(st["temporal_embedding"].abs().max()) > 0
    assert all(float(v.abs().max()) > 0 for k, v in st.items() if "D_fc2" in k)
    m = _build(mod, T, window, D, H, L, train, prompt, st)
    imgs = randn((B, 3, T, IMG, IMG), seed + 1)
    g = randn((B, D, T, 1, 1), seed + 2)
    drawn = sys.modules["timm.models.layers"].DropPath.drawn
    del drawn[:]
    torch.manual_seed(seed + 9)
    y = m(imgs)
    masks = [k.clone() for k in drawn]
    params = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(n for n, _ in params) == sorted(O.trainable_names(st)) and len(params) == 12 * L + 3
    grads = torch.autograd.grad(y, [p for _, p in params], g)

    def other(window_, prompt_):            # the same weights, inputs and (train mode) DropPath factors in another model
        m0 = _build(mod, T, window_, D, H, L, train, prompt_, st)
        with torch.no_grad():
            torch.manual_seed(seed + 9)
            y0 = m0(imgs)
        return float((y.detach() - y0).norm() / y.detach().norm())

    w_eff = other((1,) + tuple(window[1:]), prompt)
    p_eff = other(window, False) if prompt else float("nan")
    assert w_eff >= MIN_EFFECT, (tag, "window", w_eff)
    assert not prompt or p_eff >= MIN_EFFECT, (tag, "prompt", p_eff)
    names = [n for n, _ in m.named_parameters()]
    out = dict(y=y.detach(), meta=np.array([D, H, L, B, T, seed, int(train), int(prompt)] + list(window)),
               names=np.array(names), trainable=np.array([n for n, _ in params]), window_effect=np.float64(w_eff),
               prompt_effect=np.float64(p_eff))
    out.update({"shape." + n: np.array(tuple(p.shape), dtype=np.int64) for n, p in m.named_parameters()})
    if train:
        rates = [r.item() for r in torch.linspace(0, DROP_RATE, L)]
        want = [B * T for r in rates if r > 0 for _ in range(3)]
        assert [k.numel() for k in masks] == want and any((k == 0).any() for k in masks), [k.shape for k in masks]
        for k, mk in enumerate(masks):
            out[f"mask.{k}"] = mk
    else:
        assert not masks
    for k, ((n, _), gr) in enumerate(zip(params, grads)):
        if gr.numel() <= WHOLE:
            out["grad." + n] = gr
        else:
            flat = gr.reshape(-1)
            out["grad." + n + ".val"] = flat[sample_index(flat.numel(), seed * 1000 + k)]
            out["grad." + n + ".sum"] = flat.double().sum()
            out["grad." + n + ".sq"] = (flat.double() ** 2).sum()
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, f"aim_flash_win_tiny_{tag}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 400_000, os.path.getsize(path)
    print(f"{tag}: window effect {w_eff:.3f}, prompt effect {p_eff:.3f}, {os.path.getsize(path)} bytes")


def gen_configs():
    """reference_aim_flash_win_configs.json: the four AIM_flash_win recipes and their ``_base_`` files, in the format of
    reference_vit_configs.json (make_golden.gen_configs)."""
    import json
    from aim_amd.registry import _load_py
    from make_golden import CFG_KEYS, _cfg_data
    cfg_root = os.path.join(REF_ROOT, "configs")
    todo = [os.path.join(cfg_root, "recognition", "vit", "AIM", f"AIM_flash_win_base_{d}.py")
            for d in ("hmdb51", "diving48", "sthv2", "ucf101")]
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
    with open(os.path.join(HERE, "reference_aim_flash_win_configs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    torch.set_num_threads(8)
    gen_configs()
    mod = load_reference_flash_win()
    for tag in CASES:
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
