"""AIM_FLASH's host surface (no GPU): the reference's three recipes through Config.fromfile -> build_model, its parameter
names / shapes / freeze policy, the refusals, which blocks are shifted and by how much -- and the plain-PyTorch restatement
(tests/aim_flash_ref.py) that the GPU tests lean on, held to the REAL reference's stored outputs and autograd gradients
(tests/golden/aim_flash_tiny_*.npz) and to the kernels' address rule (tests/win_attn_shift_cases.box_rows)."""
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
import aim_flash_ref as R  # noqa: E402
from make_golden_imagenet import randn  # noqa: E402
from oracle import vit_clip_oracle as O  # noqa: E402
from test_aim_flash_win_cpu import _value, stored_grad  # noqa: E402

with open(os.path.join(GOLDEN, "reference_aim_flash_configs.json")) as _f:
    CONFIGS = json.load(_f)
RECIPES = sorted(p for p in CONFIGS if "AIM_flash_base" in p)
TAGS = ("a", "b", "c", "d")
ORACLE_BOUND = 2e-5           # rel-L2 of an fp32 / fp64 restatement against the fp32 reference: the project's oracle bound
DROP_RATE = 0.5               # make_golden_aim_flash_win.py
IMG, PATCH = 64, 16
MIN_EFFECT = 7.5e-2           # the family's threshold: five times the bf16 output bound of the GPU test
OUT_BOUND = 1.5e-2            # tests/test_aim_flash_gpu.py


def write_config_tree(root):
    for rel, d in CONFIGS.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {_value(v)!r}\n")


def load_case(tag):
    """-> dict(meta..., st fp32 state dict, imgs, g, masks per layer or None, z)"""
    z = np.load(os.path.join(GOLDEN, f"aim_flash_tiny_{tag}.npz"))
    D, H, L, B, T, seed, train, prompt, wt, wh, ww, st_, sh, sw = (int(v) for v in z["meta"])
    st = O.synth_state_dict(R.backbone_param_shapes(IMG, T, PATCH, D, L), seed=seed)
    masks = None
    if train:
        stored = [torch.from_numpy(z[f"mask.{k}"]) for k in range(sum(1 for k in z.files if k.startswith("mask.")))]
        masks = R.masks_per_layer(stored, [r.item() for r in torch.linspace(0, DROP_RATE, L)])
    return dict(D=D, H=H, L=L, B=B, T=T, seed=seed, train=bool(train), prompt=bool(prompt), window=(wt, wh, ww),
                shift=(st_, sh, sw), st=st, masks=masks, z=z, imgs=randn((B, 3, T, IMG, IMG), seed + 1),
                g=randn((B, D, T, 1, 1), seed + 2))


def build(c, **kw):
    import aim_amd
    kw.setdefault("not_shift", False)
    m = aim_amd.AIM_FLASH(IMG, c["T"], PATCH, c["D"], c["L"], c["H"], drop_path_rate=DROP_RATE if c["train"] else 0.0,
                          adapter_scale=0.5, prompt=c["prompt"], wind_attn=True, window_size=c["window"], **kw)
    m.init_weights()
    return m


def test_three_recipes_are_stored():
    assert [os.path.basename(p) for p in RECIPES] == [f"AIM_flash_base_{d}.py" for d in ("diving48", "hmdb51", "ucf101")]
    bbs = {os.path.basename(p): CONFIGS[p]["model"]["backbone"] for p in RECIPES}
    assert _value(bbs["AIM_flash_base_hmdb51.py"]["window_size"]) == (16, 7, 7)
    assert _value(bbs["AIM_flash_base_diving48.py"]["window_size"]) == _value(bbs["AIM_flash_base_ucf101.py"]["window_size"]) == (32, 2, 2)
    for bb in bbs.values():
        assert bb["type"] == "AIM_FLASH" and bb["wind_attn"] is True and bb["not_shift"] is False and bb["win_prompt"] is False


@pytest.mark.parametrize("rel", RECIPES, ids=[os.path.basename(p) for p in RECIPES])
def test_reference_recipe_builds_unchanged(rel, tmp_path):
    import aim_amd
    write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(os.path.join(str(tmp_path), rel))
    m = cfg.model
    assert m.type == "Recognizer3D" and m.backbone.type == "AIM_FLASH" and m.cls_head.type == "I3DHead"
    assert (m.backbone.width, m.backbone.layers, m.backbone.heads, m.backbone.patch_size) == (768, 12, 12, 16)
    assert m.backbone.pretrained == "openaiclip" and m.backbone.wind_attn is True and m.backbone.prompt is True
    with pytest.raises(RuntimeError, match="clip"):          # the OpenAI clip package and its weights are not here
        aim_amd.build_model(m)
    cfg.merge_from_dict({"model.backbone.pretrained": None})
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    assert type(bb) is aim_amd.AIM_FLASH and isinstance(bb, aim_amd.AIM_FLASH_WIN) and isinstance(bb, aim_amd.ViT_CLIP)
    assert bb.num_frames == m.backbone.num_frames and bb.window_size == tuple(m.backbone.window_size) and bb.prompt
    assert bb.not_shift is False and bb.win_prompt is False
    T = bb.num_frames
    want = {(16, 7, 7): (8, 3, 3), (32, 2, 2): (0, 1, 1)}[bb.window_size]
    assert [bb._block_shift(i, T, 14) for i in range(12)] == [want if i % 2 else None for i in range(12)]
    assert bb.positional_embedding.shape == (197, 768) and bb.temporal_embedding.shape == (1, T, 768)
    assert abs(bb.transformer.resblocks[-1].drop_prob - m.backbone.drop_path_rate) < 1e-6
    assert all(float(b.scale) == m.backbone.adapter_scale for b in bb.transformer.resblocks)
    train = [n for n, p in model.named_parameters() if p.requires_grad]
    assert len(train) == 12 * 12 + 3 + 2
    assert all(any(k in n for k in ("Adapter", "ln_post", "temporal_embedding", "cls_head")) for n in train)
    assert all(float(p.detach().abs().max()) == 0 for n, p in model.named_parameters() if "D_fc2" in n)
    assert sorted(bb.state_dict()) == sorted(R.backbone_param_shapes(224, T, 16, 768, 12))
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
    # which blocks are shifted, and by how much: the stored shift is the reference's after get_window_size
    assert [m._block_shift(i, c["T"], 4) for i in range(c["L"])] == [c["shift"] if i % 2 else None for i in range(c["L"])]
    assert c["shift"] == R.clip_shift(c["window"], c["T"], 4) and any(c["shift"])


def test_fixture_geometries_are_the_issues():
    got = {t: (load_case(t)["T"], load_case(t)["window"], load_case(t)["shift"], load_case(t)["L"], load_case(t)["train"],
               load_case(t)["prompt"]) for t in TAGS}
    assert got == {"a": (4, (2, 2, 2), (1, 1, 1), 3, True, True), "b": (8, (8, 2, 2), (0, 1, 1), 2, False, True),
                   "c": (12, (6, 2, 2), (3, 1, 1), 2, False, True), "d": (4, (2, 2, 2), (1, 1, 1), 3, False, False)}
    assert all(load_case(t)["B"] == 2 and load_case(t)["D"] == 64 * load_case(t)["H"] for t in TAGS)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_shift_effect_reaches_the_family_threshold(tag):
    """The reference's output moves by at least 7.5e-2 rel-L2 (five times the bf16 output bound) when the shift is removed:
    the generator's own refusal, asserted of the stored figures.  With two layers (b, c) the only shifted block is the last
    one and the effect is typically 0.03 .. 0.06; the generator records how the seeds that reach the threshold were found."""
    e = float(load_case(tag)["z"]["shift_effect"])
    print(f"{tag}: shift effect {e:.4f}")
    assert e >= MIN_EFFECT, (tag, e)


@pytest.mark.parametrize("tag", TAGS)
def test_a_backbone_that_ignores_the_shift_cannot_pass_the_gpu_bound(tag):
    """triangle inequality: if y0 is the reference without the shift and a backbone computes it within OUT_BOUND (relative to
    |y0|), its distance from the shifted reference y is at least |y - y0| - OUT_BOUND |y0| >= (e - OUT_BOUND (1 + e)) |y|,
    which exceeds OUT_BOUND |y| when e > 2 OUT_BOUND / (1 - OUT_BOUND)"""
    e = float(load_case(tag)["z"]["shift_effect"])
    assert e - OUT_BOUND * (1 + e) > OUT_BOUND, (tag, e)


def test_refusals_and_modes():
    import aim_amd
    kw = dict(input_resolution=64, num_frames=4, patch_size=16, width=128, layers=2, heads=2, drop_path_rate=0.0)
    ok = dict(kw, wind_attn=True, window_size=(2, 2, 2), not_shift=False)
    with pytest.raises(NotImplementedError, match="wind_attn"):
        aim_amd.AIM_FLASH(**kw)
    with pytest.raises(NotImplementedError, match="win_prompt"):
        aim_amd.AIM_FLASH(**ok, win_prompt=True)
    with pytest.raises(NotImplementedError, match="num_tadapter"):
        aim_amd.AIM_FLASH(**ok, num_tadapter=2)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        aim_amd.AIM_FLASH(**ok, checkpoint=True)
    with pytest.raises(ValueError, match="head_dim"):
        aim_amd.AIM_FLASH(**dict(ok, heads=4))
    for bad in ((3, 2, 2), (2, 3, 2), (2, 2, 3)):
        with pytest.raises(ValueError, match="divide"):
            aim_amd.AIM_FLASH(**dict(ok, window_size=bad))
    with pytest.raises(ValueError, match="at most"):
        aim_amd.AIM_FLASH(**dict(ok, input_resolution=1040, num_frames=32, window_size=(32, 65, 65)))      # S cap
    # a shifted geometry the reference cannot run: some shift non-zero while the h or the w shift is 0
    for bad in ((2, 2, 4), (2, 4, 2), (2, 2, 1), (2, 1, 2), (2, 4, 4)):
        with pytest.raises(ValueError, match="reference cannot run"):
            aim_amd.AIM_FLASH(**dict(ok, window_size=bad))
        assert aim_amd.AIM_FLASH(**dict(ok, window_size=bad, not_shift=True))._block_shift(1, 4, 4) is None
    # every shift clipped to 0: no block is shifted, nothing is refused
    m0 = aim_amd.AIM_FLASH(**dict(ok, window_size=(16, 7, 7)))
    assert [m0._block_shift(i, 4, 4) for i in range(2)] == [None, None]
    m = aim_amd.AIM_FLASH(**ok)
    assert [m._block_shift(i, 4, 4) for i in range(2)] == [None, (1, 1, 1)]
    assert [aim_amd.AIM_FLASH(**dict(ok, not_shift=True))._block_shift(i, 4, 4) for i in range(2)] == [None, None]
    assert aim_amd.AIM_FLASH(**dict(kw, wind_attn=True)).not_shift is True                  # the reference's default
    from aim_amd.aim_flash import clip_shift
    assert clip_shift((16, 7, 7), 32, 14) == (8, 3, 3) == R.clip_shift((16, 7, 7), 32, 14)
    assert clip_shift((32, 2, 2), 32, 14) == (0, 1, 1) == R.clip_shift((32, 2, 2), 32, 14)
    for flash in (True, False):
        for prompt in (True, False):
            assert aim_amd.AIM_FLASH(**ok, use_flash_attn=flash, prompt=prompt).prompt is prompt
    with pytest.raises(NotImplementedError, match="fp32"):
        m.set_precision('fp32')
    assert m.set_precision('bf16').precision == 'bf16'
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 4, 64, 64))
    with pytest.raises(TypeError, match="pretrained"):
        aim_amd.AIM_FLASH(**ok, pretrained=3).init_weights()
    assert aim_amd.BACKBONES.get("AIM_FLASH") is aim_amd.AIM_FLASH
    with pytest.raises(NotImplementedError, match="not_shift"):            # existing behaviour: the sibling still refuses
        aim_amd.AIM_FLASH_WIN(**dict(ok))


def test_drop_masks_are_per_frame_three_per_block():
    import aim_amd
    torch.manual_seed(3)
    m = aim_amd.AIM_FLASH(64, 4, 16, 128, 3, 2, drop_path_rate=0.5, adapter_scale=0.5, wind_attn=True, window_size=(2, 2, 2),
                          not_shift=False)
    w = aim_amd.AIM_FLASH_WIN(64, 4, 16, 128, 3, 2, drop_path_rate=0.5, adapter_scale=0.5, wind_attn=True, window_size=(2, 2, 2))
    assert [round(b.drop_prob, 6) for b in m.transformer.resblocks] == [0.0, 0.25, 0.5]
    torch.manual_seed(11)
    f = m._drop_masks_w(8, True, torch.device("cpu"))
    torch.manual_seed(11)
    assert f.shape == (3, 3, 8) and torch.equal(f, w._drop_masks_w(8, True, torch.device("cpu")))


@pytest.mark.parametrize("shape", range(6))
def test_restatement_labels_give_the_kernel_boxes(shape):
    """aim_flash_ref.box_index (labels per grid cell) and win_attn_shift_cases.box_rows (the kernels' address rule: segments
    and a wrapping frame) are the same sequences, token order included"""
    import win_attn_shift_cases as WS
    B, T, G, _, window, shift = WS.SHAPES[shape]
    assert shift == R.clip_shift(window, T, G)
    to_rows = lambda idx: idx + idx // (G * G) + 1
    a = sorted(tuple(s) for idx in R.box_index(B, T, G, window, shift) for s in to_rows(idx).tolist())
    b = sorted(tuple(s) for idx in WS.box_rows(B, T, G, window, shift) for s in idx.tolist())
    assert a == b


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference(tag):
    """output and every trainable gradient of tests/aim_flash_ref.py against the real reference's, train mode with the
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
    # the shift is live in the restatement too: the stored change of the reference's output
    with torch.no_grad():
        y0 = R.backbone(c["imgs"].double(), st, c["H"], c["T"], c["window"], 0.5, c["prompt"], c["masks"], not_shift=True)
        assert abs(float((y.detach() - y0).norm() / y.detach().norm()) - float(z["shift_effect"])) <= 1e-4
