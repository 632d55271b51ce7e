#!/usr/bin/env python3
"""Generate the ViT_CLIP_ZEROI2V golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (no test needs it).  It loads ``mmaction/models/backbones/vit_clip_zeroI2V.py`` by
path with ``make_golden.load_reference()``'s stand-ins (``einops`` is the installed package).  No reference source is copied:
only the reference's numeric outputs are stored; weights are ``oracle.synth_state_dict`` of the backbone's parameter shapes
(name-seeded: every ``D_fc2`` is non-zero) and the inputs are rebuilt from seeds by the tests.

    python tests/golden/make_golden_zeroi2v.py

Writes zeroi2v_tiny_{a,b,c,d}.npz and reference_zeroi2v_configs.json.  Geometry: img 32, patch 16 (N = 5), head width 64,
B = 2.  Gradients of more than ``WHOLE`` elements are stored as ``SAMPLE`` elements at seeded positions plus their fp64 sum and
sum of squares (as make_golden_imagenet.py), every parameter's shape as ``shape.<name>``, the DropPath factors the reference
drew as ``mask.<k>`` in call order (N + 1 then N entries per block with rate > 0).  ``shift_effect`` is the rel-L2 change of
the output when ``HeadShift.shift`` is replaced by the identity: the generator refuses a case where it is below 7.5e-2 (five
times the bf16 output bound of the GPU test), so that a backbone that ignores the shift cannot pass.
"""
import importlib.util
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_ROOT = "/root/reference"
REF = os.path.join(REF_ROOT, "mmaction/models/backbones/vit_clip_zeroI2V.py")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_imagenet import SAMPLE, WHOLE, randn, sample_index  # noqa: E402

IMG, PATCH, B = 32, 16, 2
# name -> (T, width, heads, layers, train, with_t_cls_token, seed)
CASES = {
    "a": (8, 256, 4, 3, True, True, 4100),
    "b": (16, 256, 4, 2, False, True, 4200),
    "c": (32, 384, 6, 2, False, True, 4300),
    "d": (8, 128, 2, 2, False, False, 4400),
}
DROP_RATE = 0.5
MIN_SHIFT_EFFECT = 7.5e-2


def load_reference_zeroi2v():
    import make_golden
    make_golden.load_reference()              # timm / clip / mmaction stand-ins
    spec = importlib.util.spec_from_file_location("mmaction.models.backbones.vit_clip_zeroI2V", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def gen_case(mod, tag):
    import zeroi2v_ref as Z
    from oracle import vit_clip_oracle as O
    logging.getLogger("ref").setLevel(logging.ERROR)
    T, D, H, L, train, tcls, seed = CASES[tag]
    m = mod.ViT_CLIP_ZEROI2V(IMG, T, PATCH, D, L, H, drop_path_rate=DROP_RATE if train else 0.0, adapter_scale=0.5,
                             with_t_cls_token=tcls, linear_adapter=False)
    m.init_weights()
    st = O.synth_state_dict(Z.backbone_param_shapes(IMG, T, PATCH, D, L, tcls), seed=seed)
    msg = m.load_state_dict(st, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    m.train() if train else m.eval()
    imgs = randn((B, 3, T, IMG, IMG), seed + 1)
    g = randn((B, D, T, 1, 1), seed + 2)
    drawn = sys.modules["timm.models.layers"].DropPath.drawn
    del drawn[:]
    torch.manual_seed(seed + 9)
    y = m(imgs)
    masks = [k.clone() for k in drawn]
    params = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(n for n, _ in params) == sorted(O.trainable_names(st))
    assert len(params) == (12 if tcls else 8) * L + 3
    grads = torch.autograd.grad(y, [p for _, p in params], g)
    # the same forward with the head shift switched off: how much of the output the shift carries
    real = mod.HeadShift.shift
    mod.HeadShift.shift = staticmethod(lambda x, inv=False, num_frames=8: x)
    try:
        with torch.no_grad():
            torch.manual_seed(seed + 9)          # train mode: the same DropPath factors again, in the same order
            y0 = m(imgs)
    finally:
        mod.HeadShift.shift = staticmethod(real)
    effect = float((y.detach() - y0).norm() / y.detach().norm())
    assert effect >= MIN_SHIFT_EFFECT, (tag, effect)
    names = [n for n, _ in m.named_parameters()]
    out = dict(y=y.detach(), meta=np.array([D, H, L, B, T, seed, int(train), int(tcls)]), names=np.array(names),
               trainable=np.array([n for n, _ in params]), shift_effect=np.float64(effect))
    out.update({"shape." + n: np.array(tuple(p.shape), dtype=np.int64) for n, p in m.named_parameters()})
    if train:
        N = (IMG // PATCH) ** 2 + 1
        rates = [r.item() for r in torch.linspace(0, DROP_RATE, L)]
        want = [n for r in rates if r > 0 for n in (N + int(tcls), N)]
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
    path = os.path.join(HERE, f"zeroi2v_tiny_{tag}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 400_000, os.path.getsize(path)
    print(f"{tag}: shift effect {effect:.3f}, {os.path.getsize(path)} bytes")


def gen_configs():
    """reference_zeroi2v_configs.json: the three zeroI2V recipes and their ``_base_`` files, in the format of
    reference_vit_configs.json (make_golden.gen_configs).

    The recipes name their bases as ``../../_base_/...``, written for ``configs/recognition/vit/``; they sit one directory
    deeper, so the paths point at ``configs/recognition/_base_/``, which the reference tree does not have.  The two base files
    are therefore read from ``configs/_base_/`` (the only copies in the tree) and stored under the paths the recipes name, so
    that the recipes themselves load unchanged."""
    import json
    from aim_amd.registry import _load_py
    from make_golden import CFG_KEYS, _cfg_data
    cfg_root = os.path.join(REF_ROOT, "configs")
    todo = [os.path.join(cfg_root, "recognition", "vit", "zeroI2V", f"vitclip_zeroI2V_base_{d}.py")
            for d in ("sthv2", "diving48", "hmdb51")]
    out = {}
    while todo:
        path = os.path.normpath(todo.pop(0))
        rel = os.path.relpath(path, cfg_root)
        if rel in out:
            continue
        src = path
        if not os.path.isfile(src):       # a base the recipe looks for under configs/recognition/_base_/
            src = os.path.join(cfg_root, os.path.relpath(path, os.path.join(cfg_root, "recognition")))
            assert rel.startswith("recognition/_base_/") and os.path.isfile(src), path
        d = {k: v for k, v in _load_py(src).items() if k in CFG_KEYS}
        out[rel] = _cfg_data(d)
        bases = d.get("_base_", [])
        todo += [os.path.join(os.path.dirname(path), b) for b in ([bases] if isinstance(bases, str) else bases)]
    with open(os.path.join(HERE, "reference_zeroi2v_configs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    torch.set_num_threads(8)
    gen_configs()
    mod = load_reference_zeroi2v()
    for tag in CASES:
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
