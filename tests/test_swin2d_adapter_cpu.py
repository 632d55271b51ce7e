"""SwinTransformer2D_Adapter's host surface (no GPU): the reference's two recipes through Config.fromfile -> build_model, its
state_dict keys, shapes and buffers, the trainable set, the init policy, the refusals, the DropPath factor layout and draw order,
the optimizer groups, and the box rule of the shifted windows against the reference's roll / partition / mask on row numbers."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import swin2d_adapter_runs as R  # noqa: E402
import swin_attn_cases as W  # noqa: E402

MG = R.MG
RECIPES = ("recognition/swin/swin2d_adapter_patch244_window7_kinetics400_1k.py",
           "recognition/swin/swin2d_adapter_patch244_window7_sthv2_1k.py")


def _tiny(**kw):
    import aim_amd
    args = dict(patch_size=(2, 4, 4), num_frames=4, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=7, drop_path_rate=0.0)
    args.update(kw)
    return aim_amd.SwinTransformer2D_Adapter(**args)


@pytest.mark.parametrize("recipe", RECIPES)
def test_reference_recipe_builds_unchanged(tmp_path, recipe):
    import aim_amd
    assert sorted(RECIPES) == R.write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(str(tmp_path / recipe))
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    assert isinstance(bb, aim_amd.SwinTransformer2D_Adapter) and aim_amd.BACKBONES.get("SwinTransformer2D_Adapter") is type(bb)
    assert (bb.embed_dim, bb.num_features, bb.num_frames, bb.num_Ttokens, bb.patch_size) == (128, 1024, 32, 16, (2, 4, 4))
    assert [l.depth for l in bb.layers] == [2, 2, 18, 2] and [l.res for l in bb.layers] == [56, 28, 14, 7]
    assert [l.blocks[0].num_heads for l in bb.layers] == [4, 8, 16, 32]
    blocks = bb._blocks()
    assert [b.t_attn for b in blocks] == [i % 2 == 0 for l in bb.layers for i in range(l.depth)]
    assert [b.shift_size for b in blocks[:22]] == [0, 3] * 11 and [b.shift_size for b in blocks[22:]] == [0, 0]
    assert [b.window_size for b in blocks] == [7] * 24
    rate = {RECIPES[0]: 0.2, RECIPES[1]: 0.4}[recipe]
    assert cfg.model.backbone.drop_path_rate == rate and blocks[0].drop_prob == 0.0 and abs(blocks[-1].drop_prob - rate) < 1e-6
    assert all(p.requires_grad for p in bb.parameters()) and bb.frozen_stages == -1
    assert model.cls_head.in_channels == bb.num_features


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_names_shapes_buffers_and_trainable_set_match_reference(tag):
    import aim_amd
    z = np.load(os.path.join(GOLDEN, f"swin2d_adapter_tiny_{tag}.npz"))
    kw = MG.CASES[tag][0]
    m = aim_amd.SwinTransformer2D_Adapter(patch_size=MG.PATCH, **kw)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]
    for k, v in sd.items():
        assert tuple(int(x) for x in z["shape." + k]) == tuple(v.shape), k
    assert [n for n, _ in m.named_parameters()] == [str(n) for n in z["names"]]
    assert [n for n, p in m.named_parameters() if p.requires_grad] == [str(n) for n in z["trainable"]]
    buffers = {n.rsplit(".", 1)[1] for n, _ in m.named_buffers()}
    assert buffers == {"relative_position_index", "attn_mask", "t_relative_coords"}
    if "frozen_stages" not in kw:
        assert all(p.requires_grad for p in m.parameters())
    else:
        m.train()
        assert not m.patch_embed.training and not m.layers[0].training and m.layers[1].training
        assert not any(p.requires_grad for p in m.layers[0].parameters()) and all(p.requires_grad for p in m.layers[1].parameters())


def test_buffers_are_the_reference_constructions():
    m = _tiny()
    blk = m.layers[0].blocks[1]
    assert (blk.window_size, blk.shift_size) == (7, 3) and tuple(blk.attn_mask.shape) == (64, 49, 49)
    _, allow = W.rolled_geometry(1, 56, 7, 3)
    assert torch.equal(blk.attn_mask == 0, allow) and set(blk.attn_mask.unique().tolist()) == {0.0, -100.0}
    assert torch.equal(blk.attn.relative_position_index.reshape(-1), W.relative_position_index(7))
    assert torch.equal(m.layers[0].blocks[0].attn.t_relative_coords, W.t_relative_coords(2))
    assert m.layers[0].blocks[0].attn_mask is None and not hasattr(blk.attn, "t_relative_coords")


def _table_ok(p):
    """trunc_normal_(std=.02): no entry is 0 or far out, and a table with enough entries has that spread"""
    p = p.detach()
    return bool((p != 0).all()) and float(p.abs().max()) < 0.12 and (p.numel() < 100 or 0.015 < float(p.std()) < 0.025)


def test_init_weights_policy(tmp_path):
    m = _tiny()
    for n, p in m.named_parameters():          # the constructor's tables: trunc_normal_(.02)
        if n.endswith("bias_table"):
            assert _table_ok(p), n
    m.init_weights()
    zeroed = 0
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".D_fc2." in n:                  # S_Adapter, S_Adapter2 ('S_Adapter' matches both) and T_Adapter
                assert float(p.abs().max()) == 0, n
                zeroed += 1
            elif n.endswith("bias_table"):
                assert _table_ok(p), n
            elif "patch_embed.proj" in n:
                pass                            # the Conv3d keeps torch's own init
            elif n.endswith("bias"):
                assert float(p.abs().max()) == 0, n
            elif "norm" in n:
                assert torch.equal(p, torch.ones_like(p)), n
            else:
                assert 0.015 < float(p.std()) < 0.025, n
    assert zeroed == 2 * (2 * 4 + 2)            # 4 blocks x (S_Adapter, S_Adapter2) + 2 even blocks x T_Adapter, weight and bias
    assert m.no_weight_decay() == {'absolute_pos_embed', 'temporal_embedding'}
    assert m.no_weight_decay_keywords() == {'relative_position_bias_table', 'temporal_position_bias_table'}
    with pytest.raises(TypeError):
        m.init_weights(pretrained=3)
    # a str `pretrained` is a local torch.load(path)['model'], its 2-D patch conv inflated over the temporal patch, strict=False
    gen = torch.Generator().manual_seed(1)
    w2d = torch.randn((32, 3, 4, 4), generator=gen)
    q = torch.randn((96, 32), generator=gen)
    path = str(tmp_path / "swin.pth")
    torch.save({"model": {"patch_embed.proj.weight": w2d, "layers.0.blocks.0.attn.qkv.weight": q, "head.weight": torch.zeros(3, 3)}}, path)
    m.init_weights(pretrained=path)
    assert torch.equal(m.patch_embed.proj.weight, w2d.unsqueeze(2).repeat(1, 1, 2, 1, 1) / 2)
    assert torch.equal(m.layers[0].blocks[0].attn.qkv.weight, q)
    assert m._last_load.unexpected_keys == ["head.weight"] and "norm.weight" in m._last_load.missing_keys
    assert float(m.layers[0].blocks[0].S_Adapter2.D_fc2.weight.abs().max()) == 0


@pytest.mark.parametrize("kw,exc,match", [
    (dict(num_heads=[2, 2]), ValueError, "head_dim 32"),
    (dict(embed_dim=64, num_heads=[2, 2]), ValueError, "head_dim 32"),
    (dict(window_size=9), ValueError, "81 tokens per window"),
    (dict(window_size=5), ValueError, "window 5 does not divide stage 0's resolution 56"),
    (dict(window_size=8), ValueError, "window 8 does not divide stage 1's resolution 28"),
    (dict(img_size=256), ValueError, "only 224 can run"),
    (dict(num_frames=5), ValueError, "not a multiple of the temporal patch size 2"),
    (dict(num_frames=66), ValueError, "33 frame tokens"),
    (dict(patch_size=4), ValueError, "tuple is needed"),
    (dict(ape=True), NotImplementedError, "absolute_pos_embed"),
    (dict(t_relative=False), NotImplementedError, "t_relative=False"),
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


def test_precision_switches_and_cpu_forward_are_refused():
    m = _tiny()
    with pytest.raises(NotImplementedError, match="no fp32 mode"):
        m.set_precision('fp32')
    assert m.set_precision('bf16').precision == 'bf16'
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    with pytest.raises(RuntimeError, match="SwinTransformer2D_Adapter runs on MI355X only"):
        m(torch.zeros(1, 3, 4, 224, 224))


@pytest.mark.parametrize("tag", ["b", "c"])
def test_drop_factors_layout_and_draw_order_are_the_reference_draws(tag):
    """from the generator's seed the model draws, block by block, the very masks the reference's DropPath drew"""
    import aim_amd
    z = np.load(os.path.join(GOLDEN, f"swin2d_adapter_tiny_{tag}.npz"))
    kw, B, train, seed = MG.CASES[tag]
    m = aim_amd.SwinTransformer2D_Adapter(patch_size=MG.PATCH, **kw).train()
    T = kw["num_frames"] // 2
    torch.manual_seed(seed + MG.DRAW)
    fac = m._drop_factors(B, T, torch.device("cpu"))
    blocks = m._blocks()
    assert len(fac) == len(blocks) and fac[0] == (None, None)          # the first block's rate is 0: it draws nothing
    k = 0
    for blk, (dp_t, dp_m) in zip(blocks[1:], fac[1:]):
        assert (dp_t is not None) == blk.t_attn and dp_m is not None
        if blk.t_attn:                                                   # one entry per (clip, position), drawn first
            assert tuple(dp_t.shape) == (B * blk.res ** 2,) and torch.equal(dp_t, torch.from_numpy(z[f"mask.{k}"]))
            k += 1
        assert tuple(dp_m.shape) == (B * T,) and torch.equal(dp_m, torch.from_numpy(z[f"mask.{k}"]))      # one per frame
        k += 1
    assert f"mask.{k}" not in z.files
    assert m.eval()._drop_factors(B, T, torch.device("cpu")) == [(None, None)] * len(blocks)


def test_optimizer_groups_of_the_recipe(tmp_path):
    import aim_amd
    from aim_amd.dist import build_optimizer
    R.write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(str(tmp_path / RECIPES[0]))
    cfg.merge_from_dict({"model.backbone.depths": [2, 2], "model.backbone.num_heads": [4, 8], "model.cls_head.in_channels": 256})
    model = aim_amd.build_model(cfg.model)
    opt = build_optimizer(model, dict(cfg.optimizer))
    names = {id(p): n for n, p in model.named_parameters()}
    lr, wd = cfg.optimizer["lr"], cfg.optimizer["weight_decay"]
    seen = 0
    for g in opt.param_groups:
        for p in g["params"]:
            n = names[id(p)]
            seen += 1
            # mmcv's DefaultOptimizerConstructor applies ONE custom key per parameter, the longest that occurs in its name:
            # the tables get decay_mult 0 at the full rate; every other backbone tensor, its norms included, gets lr_mult 0.1
            # at the full decay ('backbone' is longer than 'norm'); the head's tensors get neither
            if "relative_position_bias_table" in n:
                want = (lr, 0.0)
            elif n.startswith("backbone"):
                want = (0.1 * lr, wd)
            else:
                want = (lr, 0.0 if "norm" in n else wd)
            assert abs(g["lr"] - want[0]) < 1e-12 and g["weight_decay"] == want[1], (n, g["lr"], g["weight_decay"])
    assert seen == len(list(model.parameters()))
    tables = [n for n in names.values() if n.endswith("bias_table")]
    assert any("temporal" in n for n in tables) and any("relative" in n for n in tables)


def _axis_cuts(res, w, s):
    return sorted({0, res} | ({s + k * w for k in range(res // w)} if s else {k * w for k in range(res // w)}))


@pytest.mark.parametrize("res,w,s", [(56, 7, 3), (28, 7, 3), (14, 7, 3), (8, 4, 2), (16, 8, 4), (7, 7, 0), (12, 4, 1)])
def test_box_rule_in_original_coordinates_is_the_reference_roll_partition_and_mask(res, w, s):
    """Cut each axis at 0, s, s + w, ...: the boxes are exactly the groups of rows that attend to each other under the
    reference's roll / window_partition / attn_mask, and the bias of a pair is table[(dh + w - 1)(2w - 1) + dw + w - 1] of its
    ORIGINAL coordinate differences."""
    from aim_amd.swin2d_adapter import relative_position_index, shift_mask
    idx, allow = W.rolled_geometry(1, res, w, s)          # the reference's construction on row numbers
    if s:
        assert torch.equal(shift_mask(res, w, s) == 0, allow)
    groups = set()
    for rows, al in zip(idx, allow):
        for i in range(w * w):
            groups.add(frozenset(rows[al[i]].tolist()))
    cuts = _axis_cuts(res, w, s)
    boxes = {frozenset(y * res + x for y in range(y0, y1) for x in range(x0, x1))
             for y0, y1 in zip(cuts[:-1], cuts[1:]) for x0, x1 in zip(cuts[:-1], cuts[1:])}
    assert groups == boxes and sum(len(b) for b in boxes) == res * res
    rpi = relative_position_index(w)
    for rows, al in zip(idx, allow):
        y, x = rows // res, rows % res
        dh, dw = y[:, None] - y[None, :], x[:, None] - x[None, :]
        want = (dh + w - 1) * (2 * w - 1) + dw + w - 1
        assert torch.equal(rpi[al], want[al])             # pairs of one region keep their differences
