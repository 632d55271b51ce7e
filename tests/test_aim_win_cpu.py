"""The windowed AIM's host surface (no GPU): the reference's two ``AIM`` recipes through Config.fromfile -> build_model, its
parameter names / shapes / freeze policy, the refusals and modes, which blocks are cut and at which shift, the DropPath
draws -- and the plain-PyTorch restatement in the box form (tests/aim_win_ref.py) that the GPU tests lean on, held to the REAL
reference's stored outputs and autograd gradients (tests/golden/aim_win_tiny_*.npz; the reference computes the same thing
with a roll and a -100 mask) and to the kernels' address rule (tests/win_attn_cut_cases.box_rows)."""
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
import aim_win_ref as R  # noqa: E402
from make_golden_imagenet import randn  # noqa: E402
from oracle import vit_clip_oracle as O  # noqa: E402
from test_aim_flash_win_cpu import _value, stored_grad  # noqa: E402

with open(os.path.join(GOLDEN, "reference_aim_win_configs.json")) as _f:
    CONFIGS = json.load(_f)
RECIPES = sorted(p for p in CONFIGS if "AIM_base_" in p)
TAGS = ("a", "b", "c", "d")
ORACLE_BOUND = 2e-5           # rel-L2 of an fp32 / fp64 restatement against the fp32 reference: the project's oracle bound
DROP_RATE = 0.5               # make_golden_aim_flash_win.py
PATCH = 16
MIN_EFFECT = 7.5e-2           # the family's threshold: five times the bf16 output bound of the GPU test
OUT_BOUND = 1.5e-2            # tests/test_aim_win_gpu.py
MAX_CROSS_MASS = 1e-20        # make_golden_aim_win.py


def write_config_tree(root):
    for rel, d in CONFIGS.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {_value(v)!r}\n")


def load_case(tag):
    """-> dict(meta..., st fp32 state dict, imgs, g, masks per layer or None, z)"""
    z = np.load(os.path.join(GOLDEN, f"aim_win_tiny_{tag}.npz"))
    D, H, L, B, T, seed, train, prompt, img, wt, wh, ww, st_, sh, sw = (int(v) for v in z["meta"])
    st = O.synth_state_dict(R.backbone_param_shapes(img, T, PATCH, D, L), seed=seed)
    masks = None
    if train:
        stored = [torch.from_numpy(z[f"mask.{k}"]) for k in range(sum(1 for k in z.files if k.startswith("mask.")))]
        masks = R.masks_per_layer(stored, [r.item() for r in torch.linspace(0, DROP_RATE, L)])
    return dict(D=D, H=H, L=L, B=B, T=T, seed=seed, train=bool(train), prompt=bool(prompt), img=img, G=img // PATCH,
                window=(wt, wh, ww), shift=(st_, sh, sw), st=st, masks=masks, z=z, imgs=randn((B, 3, T, img, img), seed + 1),
                g=torch.from_numpy(z["g"]))


def build(c, **kw):
    import aim_amd
    kw.setdefault("not_shift", False)
    m = aim_amd.AIM(c["img"], c["T"], PATCH, c["D"], c["L"], c["H"], drop_path_rate=DROP_RATE if c["train"] else 0.0,
                    adapter_scale=0.5, prompt=c["prompt"], wind_attn=True, window_size=c["window"], **kw)
    m.init_weights()
    return m


def test_two_recipes_are_stored():
    assert [os.path.basename(p) for p in RECIPES] == ["AIM_base_diving48.py", "AIM_base_hmdb51.py"]
    for p in RECIPES:
        bb = CONFIGS[p]["model"]["backbone"]
        assert bb["type"] == "AIM" and bb["wind_attn"] is True and bb["not_shift"] is False and bb["prompt"] is True
        assert _value(bb["window_size"]) == (32, 2, 2)


@pytest.mark.parametrize("rel", RECIPES, ids=[os.path.basename(p) for p in RECIPES])
def test_reference_recipe_builds_unchanged(rel, tmp_path):
    import aim_amd
    write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(os.path.join(str(tmp_path), rel))
    m = cfg.model
    assert m.type == "Recognizer3D" and m.backbone.type == "AIM" and m.cls_head.type == "I3DHead"
    assert (m.backbone.width, m.backbone.layers, m.backbone.heads, m.backbone.patch_size) == (768, 12, 12, 16)
    assert m.backbone.pretrained == "openaiclip" and m.backbone.wind_attn is True and m.backbone.prompt is True
    assert m.backbone.not_shift is False and tuple(m.backbone.window_size) == (32, 2, 2)
    with pytest.raises(RuntimeError, match="clip"):          # the OpenAI clip package and its weights are not here
        aim_amd.build_model(m)
    cfg.merge_from_dict({"model.backbone.pretrained": None})
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    assert type(bb) is aim_amd.AIM and isinstance(bb, aim_amd.ViT_CLIP)
    assert bb.num_frames == m.backbone.num_frames and bb.window_size == (32, 2, 2) and bb.prompt is True
    assert bb.wind_attn is True and bb.not_shift is False
    T = bb.num_frames
    want = R.clip_shift((32, 2, 2), T, 14)
    assert want == ((0, 1, 1) if T <= 32 else (16, 1, 1))
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
    import aim_amd
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
    # the state_dict keys of AIM do not depend on wind_attn
    stock = aim_amd.AIM(c["img"], c["T"], PATCH, c["D"], c["L"], c["H"], drop_path_rate=0.0)
    assert list(stock.state_dict()) == list(sd)
    m.load_state_dict(c["st"], strict=True)
    # which blocks are cut, and at which shift: the stored shift is the reference's after get_window_size
    assert [m._block_shift(i, c["T"], c["G"]) for i in range(c["L"])] == [c["shift"] if i % 2 else None for i in range(c["L"])]
    assert c["shift"] == R.clip_shift(c["window"], c["T"], c["G"]) and any(c["shift"])


def test_fixture_geometries_are_the_issues():
    got = {t: (load_case(t)["img"], load_case(t)["T"], load_case(t)["window"], load_case(t)["shift"], load_case(t)["prompt"],
               load_case(t)["train"], load_case(t)["H"]) for t in TAGS}
    assert got == {"a": (64, 4, (2, 2, 2), (1, 1, 1), True, False, 2), "b": (64, 4, (32, 2, 2), (0, 1, 1), True, True, 2),
                   "c": (64, 4, (2, 2, 2), (1, 1, 1), False, True, 1), "d": (96, 8, (4, 3, 3), (2, 1, 1), True, False, 2)}
    assert all(load_case(t)["B"] == 2 and load_case(t)["L"] == 3 and load_case(t)["D"] == 64 * load_case(t)["H"] for t in TAGS)
    assert R.clip_window((32, 2, 2), 4, 4) == (4, 2, 2)
    b = load_case("b")
    assert len(b["masks"]) == 3 and b["masks"][0] is None and all(len(mk) == 2 and mk[0].shape == (17,) for mk in b["masks"][1:])


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_effects_and_cross_region_mass(tag):
    """The reference's output moves by at least 7.5e-2 rel-L2 (five times the bf16 output bound) when the shift is removed, and
    the reference's own softmax leaves at most 1e-20 of probability mass across its -100 mask: the generator's refusals,
    asserted of the stored figures.  A backbone that ignores the shift cannot pass the GPU bound (triangle inequality, as
    tests/test_aim_flash_cpu.py).  Where t is cut (a, c, d) the output moves as far when t wraps as in AIM_FLASH instead, so a
    backbone that ran the wrapping kernels could not pass either; where st = 0 (b) the two are the same partition."""
    z = load_case(tag)["z"]
    e, w, mass = float(z["shift_effect"]), float(z["t_wrap_effect"]), float(z["cross_mass"])
    print(f"{tag}: shift effect {e:.4f}, t-wrap effect {w:.4f}, cross-region mass {mass:.2e}")
    assert e >= MIN_EFFECT, (tag, e)
    assert e - OUT_BOUND * (1 + e) > OUT_BOUND, (tag, e)
    assert 0 <= mass <= MAX_CROSS_MASS, (tag, mass)
    if load_case(tag)["shift"][0]:
        assert w >= MIN_EFFECT and w - OUT_BOUND * (1 + w) > OUT_BOUND, (tag, w)
    else:
        assert w <= ORACLE_BOUND          # st = 0: the same partition (the figure is the restatement's distance from the reference)


def test_refusals_and_modes():
    import aim_amd
    kw = dict(input_resolution=64, num_frames=4, patch_size=16, width=128, layers=2, heads=2, drop_path_rate=0.0)
    ok = dict(kw, wind_attn=True, window_size=(2, 2, 2), not_shift=False)
    with pytest.raises(NotImplementedError, match="wind_attn") as e:          # the constructor's default not_shift=True
        aim_amd.AIM(**kw, wind_attn=True)
    assert "not_shift=False" in str(e.value) and "unshifted" in str(e.value)
    with pytest.raises(NotImplementedError, match="wind_attn"):
        aim_amd.AIM(**dict(ok, not_shift=True))
    with pytest.raises(NotImplementedError, match="num_tadapter"):
        aim_amd.AIM(**ok, num_tadapter=2)
    with pytest.raises(NotImplementedError, match="num_tadapter"):
        aim_amd.AIM(**kw, num_tadapter=2)
    with pytest.raises(ValueError, match="head_dim"):
        aim_amd.AIM(**dict(ok, heads=4))
    for bad in ((3, 2, 2), (2, 3, 2), (2, 2, 3)):
        with pytest.raises(ValueError, match="divide"):
            aim_amd.AIM(**dict(ok, window_size=bad))
    with pytest.raises(ValueError, match="at most"):
        aim_amd.AIM(**dict(ok, input_resolution=1040, num_frames=32, window_size=(32, 65, 65)))      # S cap
    m = aim_amd.AIM(**ok)
    assert m.wind_attn is True and m.not_shift is False and m.window_size == (2, 2, 2)
    assert [m._block_shift(i, 4, 4) for i in range(2)] == [None, (1, 1, 1)]
    # a shift that is zero on h or w is fine here (the mask has no strips to lose); all three zero: no block is cut
    assert aim_amd.AIM(**dict(ok, window_size=(2, 2, 4)))._block_shift(1, 4, 4) == (1, 1, 0)
    assert aim_amd.AIM(**dict(ok, window_size=(16, 7, 7)))._block_shift(1, 4, 4) is None
    for prompt in (True, False):
        assert aim_amd.AIM(**ok, prompt=prompt).prompt is prompt
    with pytest.raises(NotImplementedError, match="fp32"):
        m.set_precision('fp32')
    assert m.set_precision('bf16').precision == 'bf16'
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 4, 64, 64))
    assert aim_amd.BACKBONES.get("AIM") is aim_amd.AIM
    # wind_attn=False is what it was: the stock block, with its fp32 mode
    s = aim_amd.AIM(**kw)
    assert s.wind_attn is False and s.variant == 'aim' and s.set_precision('fp32').precision == 'fp32'


def test_frame_and_token_limits_are_refused_in_forward(monkeypatch):
    """more than 288 tokens per frame or more than 32 frames: ValueError, like AIM_FLASH_WIN (checked before any launch; the
    device check is bypassed with a stand-in tensor class attribute)"""
    import aim_amd
    big = aim_amd.AIM(272, 4, 16, 64, 1, 1, drop_path_rate=0.0, wind_attn=True, window_size=(2, 1, 1), not_shift=False)   # 17 x 17 + 2
    long = aim_amd.AIM(64, 36, 16, 64, 1, 1, drop_path_rate=0.0, wind_attn=True, window_size=(2, 2, 2), not_shift=False)
    monkeypatch.setattr(aim_amd.ViT_CLIP, "_take_blend_check_clip", lambda self, x, name: None)
    with pytest.raises(ValueError, match="at most 288"):
        big(torch.zeros(1, 3, 4, 272, 272))
    with pytest.raises(ValueError, match="at most 32"):
        long(torch.zeros(1, 3, 36, 64, 64))


def test_block_shifts_of_the_recipe_geometries():
    import aim_amd
    from aim_amd.aim_flash import clip_shift
    for window, T, want in (((32, 2, 2), 32, (0, 1, 1)), ((32, 2, 2), 8, (0, 1, 1)), ((16, 7, 7), 32, (8, 3, 3))):
        assert clip_shift(window, T, 14) == want == R.clip_shift(window, T, 14)
        m = aim_amd.AIM(224, T, 16, 64, 4, 1, drop_path_rate=0.0, wind_attn=True, window_size=window, not_shift=False)
        assert [m._block_shift(i, T, 14) for i in range(4)] == [None, want, None, want]
        assert [R.block_shift(i, window, T, 14) for i in range(4)] == [None, want, None, want]


def test_drop_masks_are_per_token_position_two_per_block():
    """two draws per block, each over the N token positions, in the reference's order: the first (T_Adapter's, without the
    adapter scale once the block divides it out), then the MLP_Adapter's; the stock table, which the windowed path reads"""
    import aim_amd
    m = aim_amd.AIM(64, 4, 16, 128, 3, 2, drop_path_rate=0.5, adapter_scale=0.5, wind_attn=True, window_size=(2, 2, 2),
                    not_shift=False)
    s = aim_amd.AIM(64, 4, 16, 128, 3, 2, drop_path_rate=0.5, adapter_scale=0.5)
    assert [round(b.drop_prob, 6) for b in m.transformer.resblocks] == [0.0, 0.25, 0.5]
    torch.manual_seed(11)
    f = m._drop_masks(17, True, torch.device("cpu"))
    torch.manual_seed(11)
    assert f.shape == (3, 2, 17) and torch.equal(f, s._drop_masks(17, True, torch.device("cpu")))
    assert bool((f[0] == 0.5).all())
    for i, keep in ((1, 0.75), (2, 0.5)):
        assert all(abs(v) < 1e-12 or abs(v - 0.5 / keep) < 1e-6 for v in f[i].reshape(-1).tolist())
    assert bool((m._drop_masks(17, False, torch.device("cpu")) == 0.5).all())


@pytest.mark.parametrize("shape", range(4))
def test_restatement_labels_give_the_kernel_boxes(shape):
    """aim_win_ref.cut_index (labels per grid cell) and win_attn_cut_cases.box_rows (the kernels' address rule: segments on
    every axis) are the same sequences, token order included"""
    import win_attn_cut_cases as WC
    B, T, G, _, window, shift = WC.SHAPES[shape]
    assert shift == R.clip_shift(window, T, G)
    to_rows = lambda idx: idx + idx // (G * G) + 1
    a = sorted(tuple(s) for idx in R.cut_index(B, T, G, window, shift) for s in to_rows(idx).tolist())
    b = sorted(tuple(s) for idx in WC.box_rows(B, T, G, window, shift) for s in idx.tolist())
    assert a == b


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference(tag):
    """output and every trainable gradient of tests/aim_win_ref.py against the real reference's, train mode with the masks
    it drew included"""
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
    # the shift and the t cut are live in the restatement too: the stored changes of the reference's output
    with torch.no_grad():
        y0 = R.backbone(c["imgs"].double(), st, c["H"], c["T"], c["window"], 0.5, c["prompt"], c["masks"], not_shift=True)
        assert abs(float((y.detach() - y0).norm() / y.detach().norm()) - float(z["shift_effect"])) <= 1e-4
        yw = R.backbone(c["imgs"].double(), st, c["H"], c["T"], c["window"], 0.5, c["prompt"], c["masks"], t_wrap=True)
        assert abs(float((y.detach() - yw).norm() / y.detach().norm()) - float(z["t_wrap_effect"])) <= 1e-4
