#!/usr/bin/env python3
"""Generate the windowed-AIM golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (no test needs it).  It loads ``mmaction/models/backbones/vitclip_aim.py`` by path
through ``make_golden.load_reference`` / ``load_reference_aim`` (imported, not edited: timm / clip / mmaction stand-ins;
``einops`` is the installed package) and builds ``AIM(wind_attn=True, not_shift=False)``: the roll, the window partition, the
-100 mask, the class-token attention, the prompt token, the two DropPath draws per block and the readout are the reference's
own code.  No reference source is copied: only numeric outputs are stored; weights are ``oracle.synth_state_dict`` of the
parameter shapes.

    python tests/golden/make_golden_aim_win.py            # writes the fixtures
    python tests/golden/make_golden_aim_win.py search a   # prints the effects of a range of seeds (restatement only)

Writes aim_win_tiny_{a,b,c,d}.npz and reference_aim_win_configs.json.  Patch 16, head width 64, B = 2, 3 layers (block 1 is
the shifted one).  Stored per fixture: ``y``, ``g``, the gradients (more than ``WHOLE`` elements: ``SAMPLE`` elements at seeded
positions plus the fp64 sum and sum of squares, as make_golden_imagenet.py), every parameter's shape, the DropPath factors the
reference drew as ``mask.<k>`` in call order (two of N entries per block with rate > 0) and three recorded effects:
  shift_effect   rel-L2 by which y moves at not_shift=True (the reference itself); refused below MIN_EFFECT = 7.5e-2
  t_wrap_effect  rel-L2 by which y moves when t wraps as in AIM_FLASH instead of being cut (tests/aim_win_ref.py, t_wrap=True)
  cross_mass     the largest probability mass the reference's own softmax assigns across a -100 mask entry, over every masked
                 attention call of the forward (``attention`` is hooked); refused above 1e-20
The clip ``imgs`` is NOT stored (fixture d's alone would be 1.7 MiB): the tests rebuild it from the stored seed, as the
sibling families do.
"""
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)
from make_golden_aim_flash_win import B, DROP_RATE, MIN_EFFECT, PATCH, REF_ROOT  # noqa: E402  (and tests/ on sys.path)
from make_golden_imagenet import WHOLE, randn, sample_index  # noqa: E402

MAX_CROSS_MASS = 1e-20
# name -> (img, T, window, width, heads, layers, train, prompt, seed)
CASES = {
    "a": (64, 4, (2, 2, 2), 128, 2, 3, False, True, 7100),       # shift (1, 1, 1), eval
    "b": (64, 4, (32, 2, 2), 128, 2, 3, True, True, 7224),       # the recipes' form: clipped (4, 2, 2), shift (0, 1, 1); DropPath
    "c": (64, 4, (2, 2, 2), 64, 1, 3, True, False, 7436),        # train, no prompt, one head
    "d": (96, 8, (4, 3, 3), 128, 2, 3, False, True, 7649),       # G = 6, shift (2, 1, 1), eval
}
# (T, G, window): the geometries on which the mask is compared with the boxes
RULE = ((4, 4, (2, 2, 2)), (4, 4, (32, 2, 2)), (8, 6, (4, 3, 3)), (4, 4, (4, 1, 2)), (32, 14, (32, 2, 2)), (32, 14, (16, 7, 7)))


def load_reference_aim_win():
    MG.load_reference()
    return MG.load_reference_aim()


def assert_mask_is_the_boxes(mod):
    """compute_mask of the reference, rolled back into original coordinates, separates exactly the pairs of cells that
    aim_win_ref.cut_index puts into different boxes of the same rolled window"""
    import aim_win_ref as WR
    for T, G, window in RULE:
        ws, ss = mod.get_window_size((T, G, G), window, tuple(w // 2 for w in window))
        assert ss == WR.clip_shift(window, T, G) and ws == WR.clip_window(window, T, G)
        if not any(ss):
            continue
        mask = mod.compute_mask(T, G, G, ws, ss, torch.device("cpu"))                     # [nW, S, S]
        ids = torch.arange(T * G * G).view(1, T, G, G, 1).float()
        rolled = torch.roll(ids, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
        wins = mod.window_partition(rolled, ws).squeeze(-1).long()                       # [nW, S] original cell ids
        box = torch.empty(T * G * G, dtype=torch.long)
        k = 0
        for idx in WR.cut_index(1, T, G, window, ss):
            for seq in idx:
                box[seq] = k
                k += 1
        same_box = box[wins].unsqueeze(1) == box[wins].unsqueeze(2)
        assert torch.equal(mask == 0, same_box), (T, G, window)
        # and no box spans two rolled windows: every box lies in one row of `wins`
        owner = torch.empty(T * G * G, dtype=torch.long)
        owner[wins.reshape(-1)] = torch.arange(wins.shape[0]).repeat_interleave(wins.shape[1])
        assert all(len(set(owner[seq].tolist())) == 1 for idx in WR.cut_index(1, T, G, window, ss) for seq in idx)
        print(f"mask ok: T={T} G={G} window={window} shift={ss}: {k} boxes per clip")


class _MassHook:
    """around the reference block's ``attention``: for every call with a mask, the largest probability mass its own softmax
    puts on masked (-100) entries of a row"""

    def __init__(self, mod):
        self.mod, self.worst, self.calls = mod, 0.0, 0
        self.orig = mod.ResidualAttentionBlock.attention

    def __enter__(self):
        hook = self

        def attention(blk, x, mask=None):
            if mask is not None:
                with torch.no_grad():
                    D, H = blk.d_model, blk.attn.num_heads
                    L, N, _ = x.shape
                    qkv = torch.nn.functional.linear(x.double(), blk.attn.in_proj_weight.double(), blk.attn.in_proj_bias.double())
                    q, k = (t.view(L, N, H, D // H).permute(1, 2, 0, 3) for t in (qkv[..., :D], qkv[..., D:2 * D]))
                    aff = q @ k.transpose(-2, -1) / (D // H) ** 0.5
                    nW = mask.shape[0]
                    aff = aff.view(N // nW, nW, H, L, L) + mask.double().unsqueeze(1).unsqueeze(0)
                    p = aff.softmax(dim=-1)
                    cross = (p * (mask != 0).unsqueeze(1).unsqueeze(0)).sum(-1)
                    hook.worst = max(hook.worst, float(cross.max()))
                    hook.calls += 1
            return hook.orig(blk, x, mask)

        self.mod.ResidualAttentionBlock.attention = attention
        return self

    def __exit__(self, *a):
        self.mod.ResidualAttentionBlock.attention = self.orig


def _build(mod, img, T, window, D, H, L, train, prompt, st, not_shift=False):
    m = mod.AIM(img, T, PATCH, D, L, H, drop_path_rate=DROP_RATE if train else 0.0, adapter_scale=0.5, prompt=prompt,
                wind_attn=True, window_size=window, not_shift=not_shift)
    m.init_weights()
    msg = m.load_state_dict(st, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    return m.train() if train else m.eval()


def _draw_masks(L, N, seed):
    """masks for the seed search only (the fixtures store what the reference drew)"""
    gen = torch.Generator().manual_seed(seed)
    rates = [r.item() for r in torch.linspace(0, DROP_RATE, L)]
    return [None if r <= 0 else tuple((torch.rand(N, generator=gen) < 1 - r).float() / (1 - r) for _ in range(2)) for r in rates]


def effects(tag, seed, masks="draw"):
    """(shift effect, t-wrap effect) of a case at a seed, from the restatement alone"""
    import aim_win_ref as WR
    from oracle import vit_clip_oracle as O
    img, T, window, D, H, L, train, prompt, _ = CASES[tag]
    st = O.synth_state_dict(WR.backbone_param_shapes(img, T, PATCH, D, L), seed=seed)
    imgs = randn((B, 3, T, img, img), seed + 1)
    if masks == "draw":
        masks = _draw_masks(L, (img // PATCH) ** 2 + 1, seed) if train else None
    with torch.no_grad():
        y = WR.backbone(imgs, st, H, T, window, 0.5, prompt, masks)
        y0 = WR.backbone(imgs, st, H, T, window, 0.5, prompt, masks, not_shift=True)
        yw = WR.backbone(imgs, st, H, T, window, 0.5, prompt, masks, t_wrap=True)
    return float((y - y0).norm() / y.norm()), float((y - yw).norm() / y.norm())


def gen_case(mod, tag):
    import aim_win_ref as WR
    from oracle import vit_clip_oracle as O
    logging.getLogger("ref").setLevel(logging.ERROR)
    img, T, window, D, H, L, train, prompt, seed = CASES[tag]
    G = img // PATCH
    N = G * G + 1
    st = O.synth_state_dict(WR.backbone_param_shapes(img, T, PATCH, D, L), seed=seed)
    assert float(st["temporal_embedding"].abs().max()) > 0
    assert all(float(v.abs().max()) > 0 for k, v in st.items() if "D_fc2" in k)
    m = _build(mod, img, T, window, D, H, L, train, prompt, st)
    assert [tuple(b.shift_size) for b in m.transformer.resblocks] == [tuple(w // 2 for w in window) if i % 2 else (0, 0, 0)
                                                                      for i in range(L)]
    imgs = randn((B, 3, T, img, img), seed + 1)
    g = randn((B, D, T, 1, 1), seed + 2)
    drawn = sys.modules["timm.models.layers"].DropPath.drawn
    del drawn[:]
    torch.manual_seed(seed + 9)
    with _MassHook(mod) as hook:
        y = m(imgs)
    masks = [k.clone() for k in drawn]
    shift = WR.clip_shift(window, T, G)
    assert hook.calls == sum(1 for i in range(L) if i % 2 and any(shift)) and hook.calls > 0
    assert hook.worst <= MAX_CROSS_MASS, (tag, "cross-region mass", hook.worst)
    params = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(n for n, _ in params) == sorted(O.trainable_names(st)) and len(params) == 12 * L + 3
    grads = torch.autograd.grad(y, [p for _, p in params], g)
    m0 = _build(mod, img, T, window, D, H, L, train, prompt, st, not_shift=True)
    with torch.no_grad():
        torch.manual_seed(seed + 9)
        y0 = m0(imgs)
    s_eff = float((y.detach() - y0).norm() / y.detach().norm())
    assert s_eff >= MIN_EFFECT, (tag, "shift", s_eff)
    rates = [r.item() for r in torch.linspace(0, DROP_RATE, L)]
    per_layer = WR.masks_per_layer(masks, rates) if train else None
    with torch.no_grad():
        yr = WR.backbone(imgs, st, H, T, window, 0.5, prompt, per_layer)
        yw = WR.backbone(imgs, st, H, T, window, 0.5, prompt, per_layer, t_wrap=True)
    assert float((yr - y.detach()).norm() / y.detach().norm()) <= 2e-5
    w_eff = float((y.detach() - yw).norm() / y.detach().norm())
    names = [n for n, _ in m.named_parameters()]
    out = dict(y=y.detach(), g=g, meta=np.array([D, H, L, B, T, seed, int(train), int(prompt), img] + list(window) + list(shift)),
               names=np.array(names), trainable=np.array([n for n, _ in params]), shift_effect=np.float64(s_eff),
               t_wrap_effect=np.float64(w_eff), cross_mass=np.float64(hook.worst))
    out.update({"shape." + n: np.array(tuple(p.shape), dtype=np.int64) for n, p in m.named_parameters()})
    if train:
        want = [N for r in rates if r > 0 for _ in range(2)]
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
    path = os.path.join(HERE, f"aim_win_tiny_{tag}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 400_000, os.path.getsize(path)
    print(f"{tag}: shift {shift}, shift effect {s_eff:.4f}, t-wrap effect {w_eff:.4f}, cross-region mass {hook.worst:.2e}, "
          f"{os.path.getsize(path)} bytes")


def gen_configs():
    """reference_aim_win_configs.json: the two AIM recipes and their ``_base_`` files, in the format of
    reference_vit_configs.json (make_golden.gen_configs)."""
    import json
    from aim_amd.registry import _load_py
    from make_golden import CFG_KEYS, _cfg_data
    cfg_root = os.path.join(REF_ROOT, "configs")
    todo = [os.path.join(cfg_root, "recognition", "vit", "AIM", f"AIM_base_{d}.py") for d in ("hmdb51", "diving48")]
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
    with open(os.path.join(HERE, "reference_aim_win_configs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def search(tag, n=400):
    """seeds from the case's own upwards, by the smaller of the two effects (a, d) or by the shift effect (b, c)"""
    seed0 = CASES[tag][-1]
    best = []
    for seed in range(seed0, seed0 + n):
        s, w = effects(tag, seed)
        best.append((min(s, w) if tag in ("a", "d") else s, seed, s, w))
    for score, seed, s, w in sorted(best, reverse=True)[:8]:
        print(f"{tag}: seed {seed}: shift effect {s:.4f}, t-wrap effect {w:.4f}")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "search":
        torch.set_num_threads(1)
        return search(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 400)
    torch.set_num_threads(8)
    mod = load_reference_aim_win()
    assert_mask_is_the_boxes(mod)
    gen_configs()
    for tag in CASES:
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
