"""ViT_CLIP_ZEROI2V's host surface (no GPU): the reference's three recipes through Config.fromfile -> build_model, its
parameter names / shapes / freeze policy, the refusals -- and the plain-PyTorch restatement (tests/zeroi2v_ref.py) that the
GPU tests lean on, held to the REAL reference's stored outputs and autograd gradients (tests/golden/zeroi2v_tiny_*.npz)."""
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
import zeroi2v_ref as Z  # noqa: E402
from make_golden_imagenet import randn, sample_index  # noqa: E402
from oracle import vit_clip_oracle as O  # noqa: E402

with open(os.path.join(GOLDEN, "reference_zeroi2v_configs.json")) as _f:
    CONFIGS = json.load(_f)
RECIPES = sorted(p for p in CONFIGS if "zeroI2V" in p)
TAGS = ("a", "b", "c", "d")
ORACLE_BOUND = 2e-5           # rel-L2 of an fp32 / fp64 restatement against the fp32 reference: the project's oracle bound
DROP_RATE = 0.5               # make_golden_zeroi2v.py


def _value(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_value(v) for v in o["__tuple__"])
        return {k: _value(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_value(v) for v in o]
    return o


def _write_config_tree(root):
    for rel, d in CONFIGS.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {_value(v)!r}\n")


def load_case(tag):
    """-> dict(meta..., st fp32 state dict, imgs, g, masks per layer or None, z)"""
    z = np.load(os.path.join(GOLDEN, f"zeroi2v_tiny_{tag}.npz"))
    D, H, L, B, T, seed, train, tcls = (int(v) for v in z["meta"])
    st = O.synth_state_dict(Z.backbone_param_shapes(32, T, 16, D, L, bool(tcls)), seed=seed)
    masks = None
    if train:
        stored = [torch.from_numpy(z[f"mask.{k}"]) for k in range(sum(1 for k in z.files if k.startswith("mask.")))]
        masks = Z.masks_per_layer(stored, [r.item() for r in torch.linspace(0, DROP_RATE, L)])
    return dict(D=D, H=H, L=L, B=B, T=T, seed=seed, train=bool(train), tcls=bool(tcls), st=st, masks=masks, z=z,
                imgs=randn((B, 3, T, 32, 32), seed + 1), g=randn((B, D, T, 1, 1), seed + 2))


def stored_grad(z, name, k, seed, got):
    """(reference values, the same elements of `got`, reference sum, reference sum of squares or None)"""
    if "grad." + name in z.files:
        return torch.from_numpy(z["grad." + name]), got, None, None
    idx = sample_index(got.numel(), seed * 1000 + k)
    return (torch.from_numpy(z["grad." + name + ".val"]), got.reshape(-1)[idx], float(z["grad." + name + ".sum"]),
            float(z["grad." + name + ".sq"]))


def test_three_recipes_are_stored():
    assert [os.path.basename(p) for p in RECIPES] == [f"vitclip_zeroI2V_base_{d}.py" for d in ("diving48", "hmdb51", "sthv2")]


@pytest.mark.parametrize("rel", RECIPES, ids=[os.path.basename(p) for p in RECIPES])
def test_reference_recipe_builds_unchanged(rel, tmp_path):
    import aim_amd
    _write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(os.path.join(str(tmp_path), rel))
    m = cfg.model
    assert m.type == "Recognizer3D" and m.backbone.type == "ViT_CLIP_ZEROI2V" and m.cls_head.type == "I3DHead"
    assert (m.backbone.width, m.backbone.layers, m.backbone.heads, m.backbone.patch_size) == (768, 12, 12, 16)
    assert m.backbone.pretrained == "openaiclip" and m.backbone.linear_adapter is False
    with pytest.raises(RuntimeError, match="clip"):          # the OpenAI clip package and its weights are not here
        aim_amd.build_model(m)
    cfg.merge_from_dict({"model.backbone.pretrained": None})
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    assert isinstance(bb, aim_amd.ViT_CLIP_ZEROI2V) and isinstance(bb, aim_amd.ViT_CLIP)
    assert bb.num_frames == m.backbone.num_frames and bb.with_t_cls_token == bool(m.backbone.with_t_cls_token)
    assert bb.head_shifts == Z.head_shifts(bb.num_frames, 12)
    assert bb.positional_embedding.shape == (197, 768) and bb.temporal_embedding.shape == (1, bb.num_frames, 768)
    assert abs(bb.transformer.resblocks[-1].drop_prob - m.backbone.drop_path_rate) < 1e-6
    assert all(float(b.scale) == m.backbone.adapter_scale for b in bb.transformer.resblocks)
    assert model.cls_head.fc_cls.weight.shape == (m.cls_head.num_classes, 768)
    train = [n for n, p in model.named_parameters() if p.requires_grad]
    per = 12 if bb.with_t_cls_token else 8
    assert len(train) == per * 12 + 3 + 2
    assert all(any(k in n for k in ("Adapter", "ln_post", "temporal_embedding", "cls_head")) for n in train)
    assert all(float(p.abs().max()) == 0 for n, p in model.named_parameters() if "D_fc2" in n)
    assert sorted(bb.state_dict()) == sorted(Z.backbone_param_shapes(224, bb.num_frames, 16, 768, 12, bb.with_t_cls_token))
    assert [id(p) for p in bb._trainable_list()] == [id(p) for p in bb._trainable_list()] and \
        sorted(id(p) for p in bb._trainable_list()) == sorted(id(p) for p in bb.parameters() if p.requires_grad)
    if "blending" in (m.get("train_cfg") or {}):
        assert isinstance(model.blending, aim_amd.LabelSmoothing)
    from aim_amd.dist import build_optimizer
    opt = build_optimizer(model, dict(cfg.optimizer))
    assert sum(len(g["params"]) for g in opt.param_groups) == len(train)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_matches_reference(tag):
    import aim_amd
    c = load_case(tag)
    z = c["z"]
    m = aim_amd.ViT_CLIP_ZEROI2V(32, c["T"], 16, c["D"], c["L"], c["H"], drop_path_rate=DROP_RATE if c["train"] else 0.0,
                                 with_t_cls_token=c["tcls"])
    m.init_weights()
    names = [str(n) for n in z["names"]]
    sd = m.state_dict()
    assert sorted(sd) == sorted(names)
    for n in names:
        assert tuple(int(v) for v in z["shape." + n]) == tuple(sd[n].shape), n
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted(str(n) for n in z["trainable"])
    assert len(z["trainable"]) == (12 if c["tcls"] else 8) * c["L"] + 3
    assert ("transformer.resblocks.0.T_Adapter.D_fc1.weight" in sd) == c["tcls"]
    m.load_state_dict(c["st"], strict=True)
    assert float(z["shift_effect"]) >= 7.5e-2          # the reference's output moves by this much without the shift


def test_refusals_and_modes():
    import aim_amd
    kw = dict(input_resolution=32, num_frames=8, patch_size=16, width=128, layers=1, heads=2, drop_path_rate=0.0)
    with pytest.raises(NotImplementedError, match="linear_adapter"):
        aim_amd.ViT_CLIP_ZEROI2V(**kw, linear_adapter=True)
    with pytest.raises(TypeError, match="num_tadapter"):
        aim_amd.ViT_CLIP_ZEROI2V(**kw, num_tadapter=2, with_t_cls_token=True)
    with pytest.raises(ValueError, match="head_dim"):
        aim_amd.ViT_CLIP_ZEROI2V(**dict(kw, heads=4))
    with pytest.raises(ValueError, match="heads"):           # 16 frames shift four heads
        aim_amd.ViT_CLIP_ZEROI2V(**dict(kw, num_frames=16))
    m = aim_amd.ViT_CLIP_ZEROI2V(**kw, num_tadapter=2)       # without the class token the keyword is unused, as in the reference
    assert not m.with_t_cls_token and not hasattr(m.transformer.resblocks[0], "T_Adapter")
    with pytest.raises(NotImplementedError, match="fp32"):
        m.set_precision('fp32')
    assert m.set_precision('bf16').precision == 'bf16'
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 8, 32, 32))
    with pytest.raises(TypeError, match="pretrained"):
        aim_amd.ViT_CLIP_ZEROI2V(**kw, pretrained=3).init_weights()
    assert aim_amd.BACKBONES.get("ViT_CLIP_ZEROI2V") is aim_amd.ViT_CLIP_ZEROI2V
    assert aim_amd.ViT_CLIP_ZEROI2V(**dict(kw, num_frames=4)).head_shifts == (0, 0)
    from aim_amd.zeroi2v import HEAD_SHIFTS
    assert HEAD_SHIFTS == Z.HEAD_SHIFTS == {8: (1, -1), 16: (1, -1, 2, -2), 32: (1, -1, 2, -2, 3)}


def test_drop_masks_follow_the_reference_draws():
    """two masks per block, N + 1 then N entries, rates linspace(0, rate, L), factor scale / keep or 0"""
    import aim_amd
    torch.manual_seed(3)
    m = aim_amd.ViT_CLIP_ZEROI2V(32, 8, 16, 128, 3, 2, drop_path_rate=0.5, adapter_scale=0.5, with_t_cls_token=True)
    assert [round(b.drop_prob, 6) for b in m.transformer.resblocks] == [0.0, 0.25, 0.5]
    dp1, dp2 = m._drop_masks_z(6, 5, True, torch.device("cpu"))
    assert dp1.shape == (3, 6) and dp2.shape == (3, 5)
    assert bool((dp1[0] == 0.5).all()) and bool((dp2[0] == 0.5).all())
    for i, keep in ((1, 0.75), (2, 0.5)):
        for t in (dp1[i], dp2[i]):
            assert all(abs(v) < 1e-12 or abs(v - 0.5 / keep) < 1e-6 for v in t.tolist())
    e1, e2 = m._drop_masks_z(6, 5, False, torch.device("cpu"))
    assert bool((e1 == 0.5).all()) and bool((e2 == 0.5).all())


@pytest.mark.parametrize("T,H,shifts", [(8, 4, (1, -1, 0, 0)), (16, 4, (1, -1, 2, -2)), (32, 6, (1, -1, 2, -2, 3, 0)),
                                        (8, 3, (7, -7, 3)), (4, 2, (0, 0))])
def test_head_shift_is_torch_roll_inside_a_clip(T, H, shifts):
    B, L, C = 3, 2, 4
    x = torch.randn(B * T, H, L, C)
    got = Z.head_shift(x, T, shifts)
    y = x.view(B, T, H, L, C)
    want = torch.stack([torch.roll(y[:, :, h], shifts=s, dims=1) for h, s in enumerate(shifts)], dim=2).reshape(B * T, H, L, C)
    assert torch.equal(got, want)
    # out[t] = in[t - s]
    for h, s in enumerate(shifts):
        for t in range(T):
            assert torch.equal(got.view(B, T, H, L, C)[1, t, h], y[1, (t - s) % T, h])
    # a clip never sees another clip: poison clip 1, clips 0 and 2 keep their values
    xp = x.clone().view(B, T, H, L, C)
    xp[1] = float("nan")
    gp = Z.head_shift(xp.view(B * T, H, L, C), T, shifts).view(B, T, H, L, C)
    assert torch.equal(gp[0], got.view(B, T, H, L, C)[0]) and torch.equal(gp[2], got.view(B, T, H, L, C)[2])
    assert Z.head_shifts(T, H) == (tuple(Z.HEAD_SHIFTS.get(T, ())) + (0,) * H)[:H]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference(tag):
    """output and every trainable gradient of tests/zeroi2v_ref.py against the real reference's, train mode with the masks
    it drew included"""
    c = load_case(tag)
    z = c["z"]
    st = {k: v.double().requires_grad_(True) for k, v in c["st"].items()}
    y = Z.backbone(c["imgs"].double(), st, c["H"], c["T"], 0.5, c["tcls"], c["masks"])
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
        if float(ref.abs().max()) == 0:       # (case a: the last block's MLP_Adapter factor of the class token was drawn 0)
            assert float(got.abs().max()) == 0, n
            continue
        err = float((got - ref.double()).norm() / ref.double().norm())
        worst = max(worst, err)
        assert err <= ORACLE_BOUND, (n, err)
        if rsq is not None:         # the elements that were not sampled: the whole tensor's sum of squares and sum
            assert abs(float((g ** 2).sum()) - rsq) <= 1e-4 * rsq, n
            assert abs(float(g.sum()) - rsum) <= 1e-4 * float(g.abs().sum()), n
    print(f"{tag}: worst gradient rel-L2 {worst:.2e}")
    # frozen tensors get none
    frozen = [n for n in st if n not in names]
    assert frozen and all("Adapter" not in n for n in frozen)
    # and the shift is live in the restatement too: the stored change of the reference's output without it
    with torch.no_grad():
        y0 = Z.backbone(c["imgs"].double(), st, c["H"], c["T"], 0.5, c["tcls"], c["masks"], shift=False)
    eff = float((y.detach() - y0).norm() / y.detach().norm())
    assert abs(eff - float(z["shift_effect"])) <= 1e-4 and eff >= 7.5e-2
