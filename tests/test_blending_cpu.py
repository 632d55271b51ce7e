"""``train_cfg.blending`` on the host: the BLENDINGS registry, the recognizer building it from the reference's own
recipes, the three blendings' seeded draws and outputs, and the soft-label / class-weighted ``CrossEntropyLoss``, all held
to numbers the REAL reference produced (tests/golden/blending_ref.npz, tests/golden/make_golden_blending.py)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "blending_ref.npz"))
BLEND_CASES = sorted({k.split(".")[0] for k in Z.files if k.startswith("blend_")})
LOSS_CASES = sorted({k.split(".")[0] for k in Z.files if k.startswith("loss_")})
KINDS = {0: "LabelSmoothing", 1: "MixupBlending", 2: "CutmixBlending"}


def _value(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_value(v) for v in o["__tuple__"])
        return {k: _value(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_value(v) for v in o]
    return o


def _write_config_tree(root):
    """The stored reference configs as config files (as tests/test_reference_configs.py writes them)."""
    with open(os.path.join(HERE, "golden", "reference_vit_configs.json")) as f:
        configs = json.load(f)
    for rel, d in configs.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {_value(v)!r}\n")


def _case(name):
    return {k.split(".", 1)[1]: Z[k] for k in Z.files if k.split(".")[0] == name}


def _clips(c):
    g = torch.Generator().manual_seed(int(c["seed"]) + 1000)
    return torch.randn(tuple(int(v) for v in c["shape"]), generator=g)


def _tiny_cfg(**extra):
    return dict(type='Recognizer3D',
                backbone=dict(type='ViT_CLIP', input_resolution=32, num_frames=2, patch_size=16, width=128, layers=1, heads=2,
                              drop_path_rate=0.0, adapter_scale=0.5, pretrained=None),
                cls_head=dict(type='I3DHead', in_channels=128, num_classes=10, spatial_type='avg', dropout_ratio=0.0),
                test_cfg=dict(average_clips='prob'), **extra)


def test_sthv2_recipe_builds_its_label_smoothing(tmp_path):
    """vitclip_large_sthv2.py's train_cfg.blending reaches the recognizer (recognizers/base.py:104-107)."""
    import aim_amd
    _write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(os.path.join(str(tmp_path), "recognition/vit/vitclip_large_sthv2.py"))
    torch.manual_seed(0)
    model = aim_amd.build_model(cfg.model)
    bl = model.blending
    assert isinstance(bl, aim_amd.LabelSmoothing) and bl.num_classes == 174
    assert bl.off_value == 0.1 / 174 and bl.on_value == 0.9 + 0.1 / 174


def test_no_train_cfg_no_blending():
    import aim_amd
    assert aim_amd.build_model(_tiny_cfg()).blending is None
    assert aim_amd.build_model(_tiny_cfg(train_cfg=dict(aux_info=[]))).blending is None


def test_unknown_blending_raises_keyerror():
    import aim_amd
    with pytest.raises(KeyError, match="not in the blending registry"):
        aim_amd.build_model(_tiny_cfg(train_cfg=dict(blending=dict(type='NoSuchBlending', num_classes=10))))
    assert sorted(aim_amd.BLENDINGS.module_dict) == ["CutmixBlending", "LabelSmoothing", "MixupBlending"]


@pytest.mark.parametrize("name", BLEND_CASES)
def test_blending_matches_reference(name):
    """Seeded draws (the reference's call order) and the CPU outputs, bit for bit."""
    import aim_amd
    c = _case(name)
    kind = int(c["kind"])
    cls = aim_amd.BLENDINGS.get(KINDS[kind])
    bl = cls(int(c["num_classes"]), smoothing=float(c["smoothing"])) if kind == 0 else \
        cls(int(c["num_classes"]), float(c["alpha"]), smoothing=float(c["smoothing"]))
    imgs, label = _clips(c), torch.from_numpy(c["label"])
    before = imgs.clone()
    torch.manual_seed(int(c["seed"]))
    plan = bl.draw(imgs.shape)
    if kind == 0:
        assert plan is None
    else:
        assert plan.lam_drawn.dtype == torch.float32 and float(plan.lam_drawn) == float(c["lam"])
        assert torch.equal(plan.perm, torch.from_numpy(c["perm"]))
    if kind == 2:
        assert plan.box == tuple(int(v) for v in c["box"])
    out_imgs, out_label = bl.apply(imgs, label, plan)
    assert torch.equal(imgs, before)                 # the caller's clips are left intact
    assert out_label.shape == c["out_label"].shape and torch.equal(out_label, torch.from_numpy(c["out_label"]))
    assert out_imgs.shape == imgs.shape
    if kind == 0:
        assert out_imgs is imgs
    elif "out_imgs" in c:
        assert torch.equal(out_imgs, torch.from_numpy(c["out_imgs"]))
    else:
        digest = hashlib.sha256(np.ascontiguousarray(out_imgs.numpy(), "<f4").tobytes()).hexdigest()
        assert digest == str(c["out_imgs_sha256"])
    # __call__ = apply(draw()) under the same seed
    torch.manual_seed(int(c["seed"]))
    again_imgs, again_label = bl(imgs, label)
    assert torch.equal(again_imgs, out_imgs) and torch.equal(again_label, out_label)


@pytest.mark.parametrize("name", LOSS_CASES)
def test_cross_entropy_matches_reference(name):
    """cross_entropy_loss.py:52-80 on CPU tensors: soft, soft + class_weight, hard + class_weight (ignored rows too)."""
    import aim_amd
    c = _case(name)
    w = c["weight"].tolist() if c["weight"].size else None
    loss_fn = aim_amd.CrossEntropyLoss(class_weight=w)
    s = torch.from_numpy(c["score"]).clone().requires_grad_(True)
    loss = loss_fn(s, torch.from_numpy(c["label"]))
    loss.backward()
    ref = torch.from_numpy(c["loss"])
    assert abs(float(loss.detach()) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))
    assert (s.grad - torch.from_numpy(c["grad"])).abs().max() <= 1e-7


def test_soft_label_head_loss_has_only_loss_cls():
    """heads/base.py:87-95: no top-1 / top-5 for soft labels; a batch of one keeps working (the unsqueeze fix)."""
    import aim_amd
    head = aim_amd.I3DHead(10, 16, dropout_ratio=0.0)
    score = torch.randn(3, 10)
    soft = torch.softmax(torch.randn(3, 10), 1)
    out = head.loss(score, soft)
    assert list(out) == ["loss_cls"]
    ref = -(soft * torch.log_softmax(score, 1)).sum(1).mean()
    assert torch.allclose(out["loss_cls"], ref)
    one = head.loss(score[:1], soft[0])
    assert list(one) == ["loss_cls"] and torch.allclose(one["loss_cls"], -(soft[0] * torch.log_softmax(score[0], 0)).sum())
    hard = head.loss(score, torch.tensor([1, 2, 3]))
    assert set(hard) == {"top1_acc", "top5_acc", "loss_cls"}


def test_forward_applies_blending_before_forward_train(monkeypatch):
    """recognizers/base.py:254-255: forward(return_loss=True) hands forward_train the smoothed labels (CPU tensors take the
    materialised path; the fused one needs the GPU)."""
    import aim_amd
    model = aim_amd.build_model(_tiny_cfg(train_cfg=dict(blending=dict(type='LabelSmoothing', num_classes=10, smoothing=0.2))))
    seen = {}

    def fake(imgs, labels, **kw):
        seen["imgs"], seen["labels"] = imgs, labels
        return {}
    monkeypatch.setattr(model, "forward_train", fake)
    imgs = torch.zeros(2, 1, 3, 2, 32, 32)
    model(imgs, torch.tensor([[3], [7]]), return_loss=True)
    assert seen["imgs"] is imgs
    want = torch.full((2, 10), 0.02)
    want[0, 3] = want[1, 7] = 0.82
    assert torch.allclose(seen["labels"], want, atol=0, rtol=0)

