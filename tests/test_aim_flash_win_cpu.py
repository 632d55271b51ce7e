"""AIM_FLASH_WIN's host surface (no GPU): the reference's four recipes through Config.fromfile -> build_model, its parameter
names / shapes / freeze policy, the refusals, the window kernels' address rule against the reference partition -- and the
plain-PyTorch restatement (tests/aim_flash_win_ref.py) that the GPU tests lean on, held to the REAL reference's stored
outputs and autograd gradients (tests/golden/aim_flash_win_tiny_*.npz)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, GOLDEN)
import aim_flash_win_ref as R  # noqa: E402
from make_golden_imagenet import randn, sample_index  # noqa: E402
from oracle import vit_clip_oracle as O  # noqa: E402

with open(os.path.join(GOLDEN, "reference_aim_flash_win_configs.json")) as _f:
    CONFIGS = json.load(_f)
RECIPES = sorted(p for p in CONFIGS if "AIM_flash_win" in p)
TAGS = ("a", "b", "c", "d", "e")
ORACLE_BOUND = 2e-5           # rel-L2 of an fp32 / fp64 restatement against the fp32 reference: the project's oracle bound
DROP_RATE = 0.5               # make_golden_aim_flash_win.py
IMG, PATCH = 64, 16
MIN_EFFECT = 7.5e-2


def _value(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_value(v) for v in o["__tuple__"])
        return {k: _value(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_value(v) for v in o]
    return o


def write_config_tree(root):
    for rel, d in CONFIGS.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {_value(v)!r}\n")


def load_case(tag):
    """-> dict(meta..., st fp32 state dict, imgs, g, masks per layer or None, z)"""
    z = np.load(os.path.join(GOLDEN, f"aim_flash_win_tiny_{tag}.npz"))
    D, H, L, B, T, seed, train, prompt, wt, wh, ww = (int(v) for v in z["meta"])
    st = O.synth_state_dict(R.backbone_param_shapes(IMG, T, PATCH, D, L), seed=seed)
    masks = None
    if train:
        stored = [torch.from_numpy(z[f"mask.{k}"]) for k in range(sum(1 for k in z.files if k.startswith("mask.")))]
        masks = R.masks_per_layer(stored, [r.item() for r in torch.linspace(0, DROP_RATE, L)])
    return dict(D=D, H=H, L=L, B=B, T=T, seed=seed, train=bool(train), prompt=bool(prompt), window=(wt, wh, ww), st=st,
                masks=masks, z=z, imgs=randn((B, 3, T, IMG, IMG), seed + 1), g=randn((B, D, T, 1, 1), seed + 2))


def stored_grad(z, name, k, seed, got):
    """(reference values, the same elements of `got`, reference sum, reference sum of squares or None)"""
    if "grad." + name in z.files:
        return torch.from_numpy(z["grad." + name]), got, None, None
    idx = sample_index(got.numel(), seed * 1000 + k)
    return (torch.from_numpy(z["grad." + name + ".val"]), got.reshape(-1)[idx], float(z["grad." + name + ".sum"]),
            float(z["grad." + name + ".sq"]))


def build(c, **kw):
    import aim_amd
    m = aim_amd.AIM_FLASH_WIN(IMG, c["T"], PATCH, c["D"], c["L"], c["H"], drop_path_rate=DROP_RATE if c["train"] else 0.0,
                              adapter_scale=0.5, prompt=c["prompt"], wind_attn=True, window_size=c["window"], **kw)
    m.init_weights()
    return m


def test_four_recipes_are_stored():
    assert [os.path.basename(p) for p in RECIPES] == [f"AIM_flash_win_base_{d}.py" for d in ("diving48", "hmdb51", "sthv2", "ucf101")]
    wins = {os.path.basename(p): _value(CONFIGS[p]["model"]["backbone"]["window_size"]) for p in RECIPES}
    assert wins["AIM_flash_win_base_ucf101.py"] == (32, 1, 1)
    assert all(w == (16, 7, 7) for n, w in wins.items() if "ucf101" not in n)


@pytest.mark.parametrize("rel", RECIPES, ids=[os.path.basename(p) for p in RECIPES])
def test_reference_recipe_builds_unchanged(rel, tmp_path):
    import aim_amd
    write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(os.path.join(str(tmp_path), rel))
    m = cfg.model
    assert m.type == "Recognizer3D" and m.backbone.type == "AIM_FLASH_WIN" and m.cls_head.type == "I3DHead"
    assert (m.backbone.width, m.backbone.layers, m.backbone.heads, m.backbone.patch_size) == (768, 12, 12, 16)
    assert m.backbone.pretrained == "openaiclip" and m.backbone.wind_attn is True and m.backbone.prompt is True
    with pytest.raises(RuntimeError, match="clip"):          # the OpenAI clip package and its weights are not here
        aim_amd.build_model(m)
    cfg.merge_from_dict({"model.backbone.pretrained": None})
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    assert isinstance(bb, aim_amd.AIM_FLASH_WIN) and isinstance(bb, aim_amd.ViT_CLIP)
    assert bb.num_frames == m.backbone.num_frames and bb.window_size == tuple(m.backbone.window_size) and bb.prompt
    assert bb.positional_embedding.shape == (197, 768) and bb.temporal_embedding.shape == (1, bb.num_frames, 768)
    assert abs(bb.transformer.resblocks[-1].drop_prob - m.backbone.drop_path_rate) < 1e-6
    assert all(float(b.scale) == m.backbone.adapter_scale for b in bb.transformer.resblocks)
    train = [n for n, p in model.named_parameters() if p.requires_grad]
    assert len(train) == 12 * 12 + 3 + 2
    assert all(any(k in n for k in ("Adapter", "ln_post", "temporal_embedding", "cls_head")) for n in train)
    assert all(float(p.detach().abs().max()) == 0 for n, p in model.named_parameters() if "D_fc2" in n)
    assert sorted(bb.state_dict()) == sorted(R.backbone_param_shapes(224, bb.num_frames, 16, 768, 12))
    assert sorted(id(p) for p in bb._trainable_list()) == sorted(id(p) for p in bb.parameters() if p.requires_grad)
    from aim_amd.dist import build_optimizer
    opt = build_optimizer(model, dict(cfg.optimizer))
    assert sum(len(g["params"]) for g in opt.param_groups) == len(train)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_matches_reference(tag):
    c = load_case(tag)
    z = c["z"]
    m = build(c)
    names = [str(n) for n in z["names"]]
    sd = m.state_dict()
    assert sorted(sd) == sorted(names)
    for n in names:
        assert tuple(int(v) for v in z["shape." + n]) == tuple(sd[n].shape), n
    train = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert train == sorted(str(n) for n in z["trainable"]) and len(train) == 12 * c["L"] + 3
    assert "transformer.resblocks.0.attn.Wqkv.weight" in sd and "transformer.resblocks.0.mlp.fc2.bias" in sd
    m.load_state_dict(c["st"], strict=True)
    assert float(z["window_effect"]) >= MIN_EFFECT
    assert (float(z["prompt_effect"]) >= MIN_EFFECT) if c["prompt"] else np.isnan(float(z["prompt_effect"]))


def test_refusals_and_modes():
    import aim_amd
    kw = dict(input_resolution=64, num_frames=4, patch_size=16, width=128, layers=1, heads=2, drop_path_rate=0.0)
    ok = dict(kw, wind_attn=True, window_size=(2, 2, 2))
    with pytest.raises(NotImplementedError, match="wind_attn"):
        aim_amd.AIM_FLASH_WIN(**kw)
    with pytest.raises(NotImplementedError, match="not_shift"):
        aim_amd.AIM_FLASH_WIN(**ok, not_shift=False)
    with pytest.raises(NotImplementedError, match="num_tadapter"):
        aim_amd.AIM_FLASH_WIN(**ok, num_tadapter=2)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        aim_amd.AIM_FLASH_WIN(**ok, checkpoint=True)
    with pytest.raises(ValueError, match="head_dim"):
        aim_amd.AIM_FLASH_WIN(**dict(ok, heads=4))
    for bad in ((3, 2, 2), (2, 3, 2), (2, 2, 3)):
        with pytest.raises(ValueError, match="divide"):
            aim_amd.AIM_FLASH_WIN(**dict(ok, window_size=bad))
    m = aim_amd.AIM_FLASH_WIN(**dict(ok, window_size=(16, 7, 7)))          # clipped to (4, 4, 4): one window per clip
    from aim_amd.aim_flash_win import clip_window
    assert clip_window(m.window_size, 4, 4) == (4, 4, 4) == R.clip_window((16, 7, 7), 4, 4)
    for flash in (True, False):
        for prompt in (True, False):
            assert aim_amd.AIM_FLASH_WIN(**ok, use_flash_attn=flash, prompt=prompt).prompt is prompt
    with pytest.raises(NotImplementedError, match="fp32"):
        m.set_precision('fp32')
    assert m.set_precision('bf16').precision == 'bf16'
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 4, 64, 64))
    with pytest.raises(TypeError, match="pretrained"):
        aim_amd.AIM_FLASH_WIN(**ok, pretrained=3).init_weights()
    assert aim_amd.BACKBONES.get("AIM_FLASH_WIN") is aim_amd.AIM_FLASH_WIN
    with pytest.raises(NotImplementedError):                                # existing behaviour: stock AIM still refuses
        aim_amd.AIM(**kw, wind_attn=True)


def test_drop_masks_are_per_frame_three_per_block():
    import aim_amd
    torch.manual_seed(3)
    m = aim_amd.AIM_FLASH_WIN(64, 4, 16, 128, 3, 2, drop_path_rate=0.5, adapter_scale=0.5, wind_attn=True, window_size=(2, 2, 2))
    assert [round(b.drop_prob, 6) for b in m.transformer.resblocks] == [0.0, 0.25, 0.5]
    f = m._drop_masks_w(8, True, torch.device("cpu"))
    assert f.shape == (3, 3, 8)
    assert bool((f[0, 0] == 1.0).all()) and bool((f[0, 1:] == 0.5).all())
    for i, keep in ((1, 0.75), (2, 0.5)):
        assert all(abs(v) < 1e-12 or abs(v - 1.0 / keep) < 1e-6 for v in f[i, 0].tolist())          # no adapter scale
        for t in (f[i, 1], f[i, 2]):
            assert all(abs(v) < 1e-12 or abs(v - 0.5 / keep) < 1e-6 for v in t.tolist())
    e = m._drop_masks_w(8, False, torch.device("cpu"))
    assert bool((e[:, 0] == 1.0).all()) and bool((e[:, 1:] == 0.5).all())


def _reference_partition(B, T, G, window):
    """the permutation of the reference's window_partition, computed on row NUMBERS: view / permute / view as Video Swin does"""
    wt, wh, ww = R.clip_window(window, T, G)
    N = G * G + 1
    rows = ((torch.arange(B * T).view(B * T, 1) * N) + 1 + torch.arange(G * G).view(1, G * G)).view(B, T, G, G, 1)
    x = rows.view(B, T // wt, wt, G // wh, wh, G // ww, ww, 1)
    return x.permute(0, 1, 3, 5, 2, 4, 6, 7).contiguous().view(-1, wt * wh * ww)


@pytest.mark.parametrize("tag", ("a", "b", "c", "d"))
def test_kernel_address_rule_is_the_reference_partition(tag):
    import win_attn_cases as W
    c = load_case(tag)
    want = _reference_partition(c["B"], c["T"], 4, c["window"])
    assert torch.equal(R.kernel_rows(c["B"], c["T"], 4, c["window"]), want)
    assert torch.equal(W.window_rows(c["B"], c["T"], 4, c["window"]), want)
    # the restatement's index into the patch grid is the same permutation
    idx = R.window_index(c["B"], c["T"], 4, c["window"])
    assert torch.equal(idx + idx // 16 + 1, want)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference(tag):
    """output and every trainable gradient of tests/aim_flash_win_ref.py against the real reference's, train mode with the
    masks it drew included"""
    c = load_case(tag)
    z = c["z"]
    st = {k: v.double().requires_grad_(True) for k, v in c["st"].items()}
    y = R.backbone(c["imgs"].double(), st, c["H"], c["T"], c["window"], 0.5, c["prompt"], c["masks"])
    yr = torch.from_numpy(z["y"]).double()
    e = float((y.detach() - yr).norm() / yr.norm())
    print(f"{tag}: output rel-L2 {e:.2e}")
    assert e <= ORACLE_BOUND
    names = [str(n) for n in z["trainable"]]
    grads = torch.autograd.grad(y, [st[n] for n in names], c["g"].double())
    worst = 0.0
    for k, (n, g) in enumerate(zip(names, grads)):
        ref, got, rsum, rsq = stored_grad(z, n, k, c["seed"], g)
        assert ref.shape == got.shape, n
        if float(ref.abs().max()) == 0:
            assert float(got.abs().max()) == 0, n
            continue
        err = float((got - ref.double()).norm() / ref.double().norm())
        worst = max(worst, err)
        assert err <= ORACLE_BOUND, (n, err)
        if rsq is not None:         # the elements that were not sampled: the whole tensor's sum of squares and sum
            assert abs(float((g ** 2).sum()) - rsq) <= 1e-4 * rsq, n
            assert abs(float(g.sum()) - rsum) <= 1e-4 * float(g.abs().sum()), n
    print(f"{tag}: worst gradient rel-L2 {worst:.2e}")
    # the window partition and the prompt are live in the restatement too: the stored changes of the reference's output
    with torch.no_grad():
        yw = R.backbone(c["imgs"].double(), st, c["H"], c["T"], (1,) + c["window"][1:], 0.5, c["prompt"], c["masks"])
        assert abs(float((y.detach() - yw).norm() / y.detach().norm()) - float(z["window_effect"])) <= 1e-4
        if c["prompt"]:
            yp = R.backbone(c["imgs"].double(), st, c["H"], c["T"], c["window"], 0.5, False, c["masks"])
            assert abs(float((y.detach() - yp).norm() / y.detach().norm()) - float(z["prompt_effect"])) <= 1e-4
