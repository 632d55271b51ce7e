#!/usr/bin/env python3
"""Generate the AIM_FLASH golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (no test needs it).  It loads ``mmaction/models/backbones/vitclip_aim_flash.py`` by
path with the stand-ins of make_golden_aim_flash_win.py (imported from it: timm / clip / mmaction, and the few lines of
``_MHA.forward`` / ``_Mlp.forward`` for the ``flash_attn`` package that is not installed, WHICH ARE THE ATTENTION AND MLP
ARITHMETIC OF THESE FIXTURES); the block wiring, the roll, the border strips, the nine cats, the class-token attention, the
prompt token, the three DropPath draws per block and the readout are the reference's own code.  No reference source is
copied: only numeric outputs are stored; weights are ``oracle.synth_state_dict`` of the parameter shapes and the inputs are
rebuilt from seeds by the tests.

    python tests/golden/make_golden_aim_flash.py

Before it writes anything it re-asserts, on the reference's own ``ResidualAttentionBlock``, what the kernels and the
restatement (tests/aim_flash_ref.py) take as the grouping rule of a shifted block -- every sequence the block hands to its
attention is recorded and compared, token order included, with ``aim_flash_ref.box_index`` -- and the two geometries the
reference itself cannot run (a shift beside a window as wide as the grid: ZeroDivisionError; beside an extent of 1:
EinopsError on an empty slice), which ``aim_amd.AIM_FLASH`` refuses.

Writes aim_flash_tiny_{a,b,c,d}.npz and reference_aim_flash_configs.json.  Geometry: img 64, patch 16 (G = 4, N = 17), head
width 64, B = 2; format and element sampling as make_golden_aim_flash_win.py.  ``shift_effect`` is the rel-L2 change of the
output against the same model with ``not_shift=True``: the generator refuses a case below 7.5e-2 (five times the bf16 output
bound of the GPU test), so that a backbone that ignores the shift cannot pass; tests/test_aim_flash_cpu.py asserts the same of
the stored figures.
"""
import importlib.util
import logging
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aim_flash_win as MW  # noqa: E402  (also puts the repository root and tests/ on sys.path)
from make_golden_aim_flash_win import B, DROP_RATE, IMG, MIN_EFFECT, PATCH, REF_ROOT  # noqa: E402
from make_golden_imagenet import WHOLE, randn, sample_index  # noqa: E402

REF = os.path.join(REF_ROOT, "mmaction/models/backbones/vitclip_aim_flash.py")
# name -> (T, window, width, heads, layers, train, prompt, seed)
CASES = {
    "a": (4, (2, 2, 2), 128, 2, 3, True, True, 6101),        # train mode with drawn DropPath; shift (1, 1, 1)  (6100: 0.059)
    "b": (8, (8, 2, 2), 64, 1, 2, False, True, 10613),       # the t shift clipped to 0: shift (0, 1, 1); one head
    "c": (12, (6, 2, 2), 128, 2, 2, False, True, 7229),      # wrapping t windows, two per clip: shift (3, 1, 1)
    "d": (4, (2, 2, 2), 128, 2, 3, False, False, 6101),      # as a, eval, prompt=False
}
# The seeds of b and c were searched for.  With two layers the only shifted block is the last one, and its patch tokens reach the
# read-out class token through one spatial attention alone: the shift effect is typically 0.03 .. 0.06 (b: at most 0.065 over
# 3 500 seeds at width 128; c: 2 of 250 seeds at width 128 reach 7.5e-2) with a long upper tail.  b is at width 64, where 6 of
# 4 800 seeds reach 7.5e-2 (10613: 0.091); c keeps width 128 (7229: 0.081).
# (T, G, window): the geometries on which the grouping rule is asserted
RULE = ((4, 4, (2, 2, 2)), (8, 14, (4, 7, 7)), (32, 14, (32, 2, 2)), (32, 14, (16, 7, 7)), (12, 8, (6, 4, 4)), (8, 6, (4, 3, 2)))


def load_reference_flash():
    MW.load_reference_flash_win()             # every stand-in, flash_attn's included
    spec = importlib.util.spec_from_file_location("mmaction.models.backbones.vitclip_aim_flash", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Recorder(nn.Module):
    """in place of a block's attention: keeps the token ids (channel 0) of every sequence it is handed, returns zeros"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x):
        self.seen += [tuple(int(v) for v in s) for s in x[..., 0].round().long().tolist()]
        return torch.zeros_like(x)


def _drive_block(mod, T, G, window, shift, nb=2):
    """the reference's block on a [nb T, G G + 1, 2] tensor whose channel 0 is the token's frame-major row number, its
    attention replaced by a recorder, ln_1 by the identity, the adapters' up-projections zero -> the recorded sequences"""
    N = G * G + 1
    blk = mod.ResidualAttentionBlock(2, 1, scale=0.5, num_frames=T, drop_path=0., use_flash_attn=False, prompt=True,
                                     wind_attn=True, window_size=window, shift_size=shift, win_prompt=False)
    blk.attn, blk.ln_1 = _Recorder(), nn.Identity()
    for a in (blk.T_Adapter, blk.S_Adapter, blk.MLP_Adapter):
        nn.init.zeros_(a.D_fc2.weight)
        nn.init.zeros_(a.D_fc2.bias)
    x = torch.zeros((nb * T, N, 2))
    x[..., 0] = torch.arange(nb * T * N).view(nb * T, N).float()
    with torch.no_grad():
        blk(x)
    return blk.attn.seen


def assert_grouping_rule(mod):
    import aim_flash_ref as FR
    for T, G, window in RULE:
        N, nb = G * G + 1, 2
        shift = tuple(w // 2 for w in window)                 # the reference's Transformer; get_window_size clips it
        seen = _drive_block(mod, T, G, window, shift, nb)
        patch_only = sorted(s for s in seen if all(r % N for r in s))
        want = []
        for idx in FR.box_index(nb, T, G, window, FR.clip_shift(window, T, G)):
            want += [tuple(int(v) + int(v) // (G * G) + 1 for v in seq) for seq in idx.tolist()]      # grid index -> row
        assert patch_only == sorted(want), (T, G, window)
        assert sum(len(s) for s in patch_only) == nb * T * G * G
        sizes = sorted({len(s) for s in patch_only})
        print(f"rule ok: T={T} G={G} window={window} shift={FR.clip_shift(window, T, G)}: {len(want) // nb} boxes per clip, S in "
              f"{sizes[0]} .. {sizes[-1]}")
    from einops import EinopsError
    for err, (T, G, window) in ((ZeroDivisionError, (8, 4, (4, 2, 4))), (ZeroDivisionError, (8, 4, (4, 4, 2))),
                                (EinopsError, (8, 4, (4, 2, 1))), (EinopsError, (8, 4, (4, 1, 2)))):
        shift = tuple(w // 2 for w in window)
        assert shift[0] > 0 and 0 in FR.clip_shift(window, T, G)[1:]
        try:
            _drive_block(mod, T, G, window, shift)
        except err as e:
            print(f"reference fails as recorded: window={window}: {type(e).__name__}")
        else:
            raise AssertionError(("the reference ran", T, G, window))


def _build(mod, T, window, D, H, L, train, prompt, st, not_shift=False):
    m = mod.AIM_FLASH(IMG, T, PATCH, D, L, H, drop_path_rate=DROP_RATE if train else 0.0, adapter_scale=0.5,
                      use_flash_attn=False, prompt=prompt, wind_attn=True, window_size=window, not_shift=not_shift,
                      win_prompt=False)
    m.init_weights()
    msg = m.load_state_dict(st, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    return m.train() if train else m.eval()


def gen_case(mod, tag):
    import aim_flash_ref as FR
    from oracle import vit_clip_oracle as O
    logging.getLogger("ref").setLevel(logging.ERROR)
    T, window, D, H, L, train, prompt, seed = CASES[tag]
    G = IMG // PATCH
    st = O.synth_state_dict(FR.backbone_param_shapes(IMG, T, PATCH, D, L), seed=seed)
    assert float(st["temporal_embedding"].abs().max()) > 0
    assert all(float(v.abs().max()) > 0 for k, v in st.items() if "D_fc2" in k)
    m = _build(mod, T, window, D, H, L, train, prompt, st)
    shifts = [tuple(b.shift_size) for b in m.transformer.resblocks]
    assert shifts == [tuple(w // 2 for w in window) if i % 2 else (0, 0, 0) for i in range(L)]
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
    m0 = _build(mod, T, window, D, H, L, train, prompt, st, not_shift=True)
    with torch.no_grad():
        torch.manual_seed(seed + 9)
        y0 = m0(imgs)
    s_eff = float((y.detach() - y0).norm() / y.detach().norm())
    assert s_eff >= MIN_EFFECT, (tag, "shift", s_eff)
    names = [n for n, _ in m.named_parameters()]
    shift = FR.clip_shift(window, T, G)
    out = dict(y=y.detach(), meta=np.array([D, H, L, B, T, seed, int(train), int(prompt)] + list(window) + list(shift)),
               names=np.array(names), trainable=np.array([n for n, _ in params]), shift_effect=np.float64(s_eff))
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
    path = os.path.join(HERE, f"aim_flash_tiny_{tag}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 400_000, os.path.getsize(path)
    print(f"{tag}: shift {shift}, shift effect {s_eff:.4f}, {os.path.getsize(path)} bytes")


def gen_configs():
    """reference_aim_flash_configs.json: the three AIM_flash recipes and their ``_base_`` files, in the format of
    reference_vit_configs.json (make_golden.gen_configs)."""
    import json
    from aim_amd.registry import _load_py
    from make_golden import CFG_KEYS, _cfg_data
    cfg_root = os.path.join(REF_ROOT, "configs")
    todo = [os.path.join(cfg_root, "recognition", "vit", "AIM", f"AIM_flash_base_{d}.py") for d in ("hmdb51", "diving48", "ucf101")]
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
    with open(os.path.join(HERE, "reference_aim_flash_configs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    torch.set_num_threads(8)
    mod = load_reference_flash()
    assert_grouping_rule(mod)
    gen_configs()
    for tag in CASES:
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
