"""SwinTransformer3D's host surface (no GPU): the reference's six recipes through Config.fromfile -> build_model, its state_dict
keys, shapes and buffers, the trainable set, inflate_weights, the refusals, the DropPath draw order and the optimizer groups."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import swin3d_attn_cases as W  # noqa: E402
import swin3d_runs as R  # noqa: E402

MG = R.MG
RECIPES = tuple(sorted("recognition/swin/" + r for r in MG.RECIPES))
# recipe -> (embed_dim, depths, heads, window, drop_path_rate)
SPEC = {"swin_tiny_patch244_window877_kinetics400_1k.py": (96, [2, 2, 6, 2], [3, 6, 12, 24], (8, 7, 7)),
        "swin_small_patch244_window877_kinetics400_1k.py": (96, [2, 2, 18, 2], [3, 6, 12, 24], (8, 7, 7)),
        "swin_base_patch244_window877_kinetics400_1k.py": (128, [2, 2, 18, 2], [4, 8, 16, 32], (8, 7, 7)),
        "swin_base_patch244_window877_kinetics400_22k.py": (128, [2, 2, 18, 2], [4, 8, 16, 32], (8, 7, 7)),
        "swin_base_patch244_window877_kinetics600_22k.py": (128, [2, 2, 18, 2], [4, 8, 16, 32], (8, 7, 7)),
        "swin_base_patch244_window1677_sthv2.py": (128, [2, 2, 18, 2], [4, 8, 16, 32], (16, 7, 7))}


def _tiny(**kw):
    import aim_amd
    args = dict(patch_size=(2, 4, 4), embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=(2, 7, 7), drop_path_rate=0.0)
    args.update(kw)
    return aim_amd.SwinTransformer3D(**args)


@pytest.mark.parametrize("recipe", RECIPES)
def test_reference_recipe_builds_unchanged(tmp_path, recipe):
    import aim_amd
    assert list(RECIPES) == R.write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(str(tmp_path / recipe))
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    assert isinstance(bb, aim_amd.SwinTransformer3D) and aim_amd.BACKBONES.get("SwinTransformer3D") is type(bb)
    dim, depths, heads, window = SPEC[os.path.basename(recipe)]
    assert (bb.embed_dim, bb.num_features, bb.patch_size, bb.window_size) == (dim, dim * 8, (2, 4, 4), window)
    assert [l.depth for l in bb.layers] == depths and [l.blocks[0].num_heads for l in bb.layers] == heads
    blocks = bb._blocks()
    half = tuple(w // 2 for w in window)
    assert [b.shift_size for b in blocks] == [(0, 0, 0), half] * (len(blocks) // 2)
    assert blocks[0].drop_prob == 0.0 and abs(blocks[-1].drop_prob - cfg.model.backbone.drop_path_rate) < 1e-6
    assert all(p.requires_grad for p in bb.parameters()) and bb.frozen_stages == -1 and bb.patch_norm
    assert model.cls_head.in_channels == bb.num_features
    # get_window_size's clipping at the recipe's clip: 32 frames of 224 x 224 -> (16, 56, 56) tokens
    geo = [bb._geo(l.blocks[1], 8, 16, 56 // 2 ** i) for i, l in enumerate(bb.layers)]
    assert [g[4] for g in geo] == [(min(window[0], 16), 7, 7)] * 4
    assert [g[5] for g in geo] == [(half[0] if window[0] < 16 else 0, 3, 3)] * 3 + [(half[0] if window[0] < 16 else 0, 0, 0)]
    assert all(g[6] == window for g in geo)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_names_shapes_buffers_and_trainable_set_match_reference(tag):
    import aim_amd
    z = np.load(os.path.join(GOLDEN, f"swin3d_tiny_{tag}.npz"))
    kw = MG.CASES[tag][0]
    m = aim_amd.SwinTransformer3D(patch_size=MG.PATCH, **kw)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]
    for k, v in sd.items():
        assert tuple(int(x) for x in z["shape." + k]) == tuple(v.shape), k
    assert [n for n, _ in m.named_parameters()] == [str(n) for n in z["names"]]
    assert [n for n, p in m.named_parameters() if p.requires_grad] == [str(n) for n in z["trainable"]]
    assert {n.rsplit(".", 1)[1] for n, _ in m.named_buffers()} == {"relative_position_index"}
    assert m.train() is m and m.eval() is m
    if "frozen_stages" not in kw:
        assert all(p.requires_grad for p in m.parameters())
    else:
        m.train()
        assert not m.patch_embed.training and not m.layers[0].training and m.layers[1].training
        assert not any(p.requires_grad for p in m.layers[0].parameters()) and all(p.requires_grad for p in m.layers[1].parameters())
        assert m._drop_factors(2, torch.device("cpu")) == [(None, None)] * 4


def test_relative_position_index_is_the_reference_buffer_and_the_arithmetic_formula():
    from aim_amd.swin3d import get_window_size, relative_position_index
    z = np.load(os.path.join(GOLDEN, "swin3d_inflate.npz"))
    assert torch.equal(relative_position_index((2, 3, 3)), torch.from_numpy(z["index.233"]))
    for full in ((2, 3, 3), (8, 3, 3), (3, 4, 4), (2, 7, 7)):
        assert torch.equal(relative_position_index(full), W.relative_position_index(full))
        assert torch.equal(relative_position_index(full), W.arithmetic_index(full, full))
    assert torch.equal(_tiny().layers[0].blocks[1].attn.relative_position_index, W.relative_position_index((2, 7, 7)))
    assert get_window_size((4, 56, 56), (8, 7, 7), (4, 3, 3)) == ((4, 7, 7), (0, 3, 3))
    assert get_window_size((16, 7, 7), (8, 7, 7), (4, 3, 3)) == ((8, 7, 7), (4, 0, 0))
    assert get_window_size((16, 7, 7), (8, 7, 7)) == (8, 7, 7)


def test_inflate_weights_reproduces_the_reference(tmp_path):
    import aim_amd
    z = np.load(os.path.join(GOLDEN, "swin3d_inflate.npz"))
    path = str(tmp_path / "swin2d.pth")
    torch.save({"model": MG.inflate_checkpoint()}, path)
    m = aim_amd.SwinTransformer3D(patch_size=MG.PATCH, pretrained=path, pretrained2d=True, **MG.INFLATE)
    m.init_weights()
    sd = m.state_dict()
    loaded = 0
    for k in z.files:
        if k.startswith("sd."):
            name = k[3:]
            if name in MG.inflate_checkpoint():
                assert torch.equal(sd[name], torch.from_numpy(z[k])), name      # inflated, interpolated, repeated: exactly
                loaded += 1
    assert loaded == 4 + 2 * 4
    table = sd["layers.0.blocks.0.attn.relative_position_bias_table"]
    assert tuple(table.shape) == (3 * 49, 1) and torch.equal(table[:49], table[49:98])
    assert m._last_load.unexpected_keys == ["head.weight"] and "norm.weight" in m._last_load.missing_keys
    # pretrained2d=False: a local Video Swin checkpoint, loaded directly
    path3 = str(tmp_path / "swin3d.pth")
    torch.save({"state_dict": {"backbone." + k: v for k, v in sd.items()}}, path3)
    m3 = aim_amd.SwinTransformer3D(patch_size=MG.PATCH, pretrained=path3, pretrained2d=False, **MG.INFLATE)
    m3.init_weights()
    assert all(torch.equal(v, m3.state_dict()[k]) for k, v in sd.items()) and not m3._last_load.missing_keys
    with pytest.raises(TypeError):
        m.init_weights(pretrained=3)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(num_heads=[2, 2]), ValueError, "head_dim 32"),
    (dict(embed_dim=64, num_heads=[2, 2]), ValueError, "head_dim 32"),
    (dict(window_size=(16, 9, 9)), ValueError, "1296 tokens per window"),
    (dict(window_size=(16, 8, 8)), ValueError, "6975 bias-table entries"),
    (dict(window_size=7), ValueError, "tuple is needed"),
    (dict(patch_size=4), ValueError, "tuple is needed"),
    (dict(use_checkpoint=True), NotImplementedError, "use_checkpoint"),
    (dict(qk_scale=0.2), NotImplementedError, "qk_scale"),
    (dict(drop_rate=0.1), NotImplementedError, "dropout"),
    (dict(attn_drop_rate=0.1), NotImplementedError, "dropout"),
    (dict(in_chans=1), NotImplementedError, "in_chans=1"),
    (dict(mlp_ratio=2.), NotImplementedError, "mlp_ratio=2.0"),
    (dict(norm_layer=torch.nn.BatchNorm1d), NotImplementedError, "only nn.LayerNorm"),
])
def test_constructor_refusals(kw, exc, match):
    with pytest.raises(exc, match=match):
        _tiny(**kw)


@pytest.mark.parametrize("shape,kw,match", [
    ((1, 3, 8, 56, 64), {}, "square clip"),
    ((1, 3, 7, 56, 56), {}, "not a multiple of the patch"),
    ((1, 3, 8, 58, 58), {}, "not a multiple of the patch"),
    ((1, 3, 8, 84, 84), {}, "grid side 21 is odd"),
    ((1, 3, 8, 112, 112), dict(window_size=(2, 8, 8)), "does not divide stage 0's token grid"),
    ((1, 3, 12, 56, 56), dict(window_size=(4, 7, 7)), "does not divide stage 0's token grid"),
    ((1, 3, 8, 24, 24), {}, "smaller than the window side"),
])
def test_clips_the_reference_would_pad_are_refused_at_forward(shape, kw, match):
    with pytest.raises(ValueError, match=match):
        _tiny(**kw)(torch.zeros(shape))


def test_precision_switches_and_cpu_forward_are_refused():
    m = _tiny()
    with pytest.raises(NotImplementedError, match="no fp32 mode"):
        m.set_precision('fp32')
    assert m.set_precision('bf16').precision == 'bf16'
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    with pytest.raises(RuntimeError, match="SwinTransformer3D runs on MI355X only"):
        m(torch.zeros(1, 3, 8, 56, 56))


@pytest.mark.parametrize("tag", ["b", "c"])
def test_drop_factors_are_the_reference_draws(tag):
    """from the generator's seed the model draws, block by block, the very masks the reference's DropPath drew"""
    import aim_amd
    z = np.load(os.path.join(GOLDEN, f"swin3d_tiny_{tag}.npz"))
    kw, (B, _, _), train, seed = MG.CASES[tag]
    m = aim_amd.SwinTransformer3D(patch_size=MG.PATCH, **kw).train()
    torch.manual_seed(seed + MG.DRAW)
    fac = m._drop_factors(B, torch.device("cpu"))
    assert fac[0] == (None, None)          # the first block's rate is 0: it draws nothing
    k = 0
    for f1, f2 in fac[1:]:
        assert tuple(f1.shape) == tuple(f2.shape) == (B,)
        assert torch.equal(f1, torch.from_numpy(z[f"mask.{k}"])) and torch.equal(f2, torch.from_numpy(z[f"mask.{k + 1}"]))
        k += 2
    assert k == 6 and f"mask.{k}" not in z.files
    assert m.eval()._drop_factors(B, torch.device("cpu")) == [(None, None)] * len(fac)


def test_optimizer_groups_of_the_recipe(tmp_path):
    import aim_amd
    from aim_amd.dist import build_optimizer
    R.write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(str(tmp_path / R.K400_BASE))
    cfg.merge_from_dict({"model.backbone.depths": [2, 2], "model.backbone.num_heads": [4, 8], "model.cls_head.in_channels": 256})
    model = aim_amd.build_model(cfg.model)
    opt = build_optimizer(model, dict(cfg.optimizer))
    names = {id(p): n for n, p in model.named_parameters()}
    lr, wd = cfg.optimizer["lr"], cfg.optimizer["weight_decay"]
    keys = cfg.optimizer["paramwise_cfg"]["custom_keys"]
    seen = 0
    for g in opt.param_groups:
        for p in g["params"]:
            n = names[id(p)]
            seen += 1
            # mmcv's DefaultOptimizerConstructor applies ONE custom key per parameter: the longest that occurs in its name
            hit = sorted((k for k in keys if k in n), key=lambda k: (-len(k), k))
            rule = keys[hit[0]] if hit else {}
            want = (lr * rule.get("lr_mult", 1.0), wd * rule.get("decay_mult", 1.0))
            assert abs(g["lr"] - want[0]) < 1e-12 and abs(g["weight_decay"] - want[1]) < 1e-12, (n, g["lr"], g["weight_decay"])
    assert seen == len(list(model.parameters()))
    assert any("relative_position_bias_table" in n for n in names.values()) and "relative_position_bias_table" in keys
