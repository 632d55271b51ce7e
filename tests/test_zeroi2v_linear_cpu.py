"""ViT_CLIP_ZEROI2V(linear_adapter=True) on the host (no GPU): parameter names / shapes / trainable sets against the real
reference's (tests/golden/zeroi2v_linear_tiny_*.npz), the init quirks, the refusals, merging's host surface -- and the
plain-PyTorch restatement and fold (tests/zeroi2v_linear_ref.py) that the GPU tests lean on, held to the reference's stored
outputs and autograd gradients."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, GOLDEN)
import zeroi2v_linear_ref as ZL  # noqa: E402
from make_golden_imagenet import randn  # noqa: E402
from make_golden_zeroi2v_linear import ADAPTER_SCALE, CASES, MIN_EFFECT, case_state  # noqa: E402
from test_zeroi2v_cpu import ORACLE_BOUND, stored_grad  # noqa: E402  (the restatement tolerance of test_zeroi2v_cpu.py)

TAGS = ("a", "b", "c", "d")
FOLD_BOUND = 1e-5             # folded against unfolded restatement, rel-L2 (2e-7 measured on two layers; the margin is for depth)
PER_BLOCK = {(False, True): 28, (False, False): 24, (True, True): 20, (True, False): 16}      # (share, tcls) -> trainable


def load_case(tag):
    z = np.load(os.path.join(GOLDEN, f"zeroi2v_linear_tiny_{tag}.npz"))
    D, H, L, B, T, seed, train, tcls, share, r = (int(v) for v in z["meta"])
    assert (T, D, H, L, r, bool(train), bool(tcls), bool(share), seed) == CASES[tag]
    return dict(D=D, H=H, L=L, B=B, T=T, seed=seed, train=bool(train), tcls=bool(tcls), share=bool(share), r=r, z=z,
                st=case_state(tag), imgs=randn((B, 3, T, 32, 32), seed + 1), g=randn((B, D, T, 1, 1), seed + 2))


def build(c, **kw):
    import aim_amd
    m = aim_amd.ViT_CLIP_ZEROI2V(32, c["T"], 16, c["D"], c["L"], c["H"], drop_path_rate=0.5 if c["train"] else 0.0,
                                 with_t_cls_token=c["tcls"], share_adapter=c["share"], bottleneck=c["r"], linear_adapter=True,
                                 **kw)
    m.init_weights()
    return m


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def null_sibling(name):
    """The gradient of Attn_Adapter_k's two BIASES is zero by the algebra: they add one constant vector to every key of a
    frame, and a softmax over keys ignores a constant.  The reference's autograd stores its own rounding noise there (1e-6
    beside 10 for the same tensor of Attn_Adapter_q), which no relative error can be held to.  For these tensors the error is
    measured against the norm of the Attn_Adapter_q tensor of the same name -- a sum of the same terms, without the
    cancellation.  Returns that name, or None for every other tensor."""
    if "Attn_Adapter_k." in name and name.endswith(".bias"):
        return name.replace("Attn_Adapter_k.", "Attn_Adapter_q.")
    return None


def test_the_four_fixtures_are_the_issues_cases():
    assert CASES == {"a": (8, 256, 4, 3, 64, True, True, False, 5100), "b": (16, 256, 4, 2, 64, False, True, True, 5200),
                     "c": (32, 384, 6, 2, 96, False, True, False, 5300), "d": (8, 128, 2, 2, 32, False, False, True, 5400)}
    assert MIN_EFFECT == 7.5e-2 and ADAPTER_SCALE == 0.5
    for tag in TAGS:
        z = np.load(os.path.join(GOLDEN, f"zeroi2v_linear_tiny_{tag}.npz"))
        assert os.path.getsize(os.path.join(GOLDEN, f"zeroi2v_linear_tiny_{tag}.npz")) < 400_000
        assert min(float(z[k]) for k in ("attn_effect", "mlp_effect", "skip_effect")) >= MIN_EFFECT


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
    assert train == sorted(str(n) for n in z["trainable"])
    assert len(train) == PER_BLOCK[(c["share"], c["tcls"])] * c["L"] + 3
    assert sorted(id(p) for p in m._trainable_list()) == sorted(id(p) for p in m.parameters() if p.requires_grad)
    assert sorted(sd) == sorted(ZL.backbone_param_shapes(32, c["T"], 16, c["D"], c["L"], c["tcls"], c["share"], c["r"]))
    m.load_state_dict(c["st"], strict=True)


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("tcls", [False, True])
def test_all_four_combinations_and_the_init_quirks(share, tcls):
    import aim_amd
    torch.manual_seed(1)
    m = aim_amd.ViT_CLIP_ZEROI2V(32, 8, 16, 128, 2, 2, drop_path_rate=0.1, with_t_cls_token=tcls, share_adapter=share,
                                 bottleneck=32, linear_adapter=True)
    m.init_weights()
    blk = m.transformer.resblocks[0]
    have = {n for n, _ in blk.named_children() if "Adapter" in n}
    assert have == set(ZL.adapter_names(share, tcls))
    assert not hasattr(blk, "S_Adapter") and not hasattr(blk, "MLP_Adapter")
    train = [n for n, p in m.named_parameters() if p.requires_grad]
    assert len(train) == PER_BLOCK[(share, tcls)] * 2 + 3
    for n, p in m.named_parameters():
        if "Adapter" not in n:
            continue
        if "D_fc2" in n and ("MLP_Adapter" in n or "T_Adapter" in n):
            assert float(p.detach().abs().max()) == 0, n                        # matched by the reference's zeroing loops
        elif n.endswith("weight"):            # trunc_normal_(std=.02), cut at +-2 absolute; Attn_Adapter_*.D_fc2 stays live
            assert 0.015 < float(p.detach().std()) < 0.025, n
        else:
            assert float(p.detach().abs().max()) == 0, n                        # every nn.Linear bias
    assert m.linear_adapter and m.share_adapter == share and m.bottleneck == 32 and not m.merged


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference(tag):
    c = load_case(tag)
    z = c["z"]
    st = {k: v.double().requires_grad_(True) for k, v in c["st"].items()}
    y = ZL.backbone(c["imgs"].double(), st, c["H"], c["T"], c["tcls"], c["share"])
    yr = torch.from_numpy(z["y"]).double()
    e = rel(y.detach(), yr)
    print(f"{tag}: output rel-L2 {e:.2e}")
    assert e <= ORACLE_BOUND
    names = [str(n) for n in z["trainable"]]
    grads = torch.autograd.grad(y, [st[n] for n in names], c["g"].double())
    worst = 0.0
    refs = {n: stored_grad(z, n, k, c["seed"], g)[0] for k, (n, g) in enumerate(zip(names, grads))}
    for k, (n, g) in enumerate(zip(names, grads)):
        ref, got, rsum, rsq = stored_grad(z, n, k, c["seed"], g)
        assert ref.shape == got.shape and float(ref.abs().max()) > 0, n       # every trainable tensor receives a gradient
        if null_sibling(n):
            scale = float(refs[null_sibling(n)].double().norm())
            assert float(ref.double().norm()) <= ORACLE_BOUND * scale, n      # zero by the algebra: the reference holds noise
            assert float((got - ref.double()).norm()) <= ORACLE_BOUND * scale, n
            continue
        err = rel(got, ref)
        worst = max(worst, err)
        assert err <= ORACLE_BOUND, (n, err)
        if rsq is not None:
            assert abs(float((g ** 2).sum()) - rsq) <= 1e-4 * rsq, n
            assert abs(float(g.sum()) - rsum) <= 1e-4 * float(g.abs().sum()), n
    print(f"{tag}: worst gradient rel-L2 {worst:.2e}")
    # the three stored effects: each adapter family and the doubled skip are live in the restatement as in the reference
    with torch.no_grad():
        for key, kw in (("attn_effect", dict(attn_identity=True)), ("mlp_effect", dict(mlp_identity=True)),
                        ("skip_effect", dict(single_skip=True))):
            y0 = ZL.backbone(c["imgs"].double(), st, c["H"], c["T"], c["tcls"], c["share"], **kw)
            eff = rel(y0, y.detach())
            assert abs(eff - float(z[key])) <= 1e-4 and eff >= MIN_EFFECT, (key, eff, float(z[key]))


@pytest.mark.parametrize("tag", TAGS)
def test_fold_reproduces_the_unfolded_model(tag):
    """fp64 restatement: folded against unfolded at most 1e-5; folding the class chain's attention weights in place must
    EXCEED that bound (the test can see the mistake); and in fp32 against the fixture"""
    c = load_case(tag)
    st = {k: v.double() for k, v in c["st"].items()}
    with torch.no_grad():
        y = ZL.backbone(c["imgs"].double(), st, c["H"], c["T"], c["tcls"], c["share"])
        fs = ZL.fold(st, c["L"], c["tcls"], c["share"])
        assert not any("Attn_Adapter" in k or "MLP_Adapter" in k for k in fs)
        yf = ZL.backbone(c["imgs"].double(), fs, c["H"], c["T"], c["tcls"], c["share"], folded=True)
        e = rel(yf, y)
        print(f"{tag}: folded against unfolded {e:.2e}")
        assert e <= FOLD_BOUND
        if c["tcls"]:
            bad = ZL.fold(st, c["L"], c["tcls"], c["share"], cls_in_place=True)
            eb = rel(ZL.backbone(c["imgs"].double(), bad, c["H"], c["T"], c["tcls"], c["share"], folded=True), y)
            print(f"{tag}: class chain folded in place {eb:.2e}")
            assert eb > FOLD_BOUND
        f32 = ZL.fold(c["st"], c["L"], c["tcls"], c["share"])
        y32 = ZL.backbone(c["imgs"], f32, c["H"], c["T"], c["tcls"], c["share"], folded=True)
        assert rel(y32, torch.from_numpy(c["z"]["y"])) <= FOLD_BOUND


@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_package_fold_is_the_restatements_fold(tag):
    """``zeroi2v_linear.fold_block`` (fp64 products, one rounding to bf16) against ``ZL.fold`` in fp64 rounded the same way:
    equal bits for every merged weight, biases to fp32 rounding"""
    from aim_amd.zeroi2v_linear import fold_block
    c = load_case(tag)
    m = build(c)
    m.load_state_dict(c["st"], strict=True)
    fs = ZL.fold({k: v.double() for k, v in c["st"].items()}, c["L"], c["tcls"], c["share"])
    for i, blk in enumerate(m.transformer.resblocks):
        mg = fold_block(blk, c["share"], c["tcls"])
        pre = f"transformer.resblocks.{i}."
        for attr, key in (("Wqkv", "attn.in_proj_weight"), ("Wo", "attn.out_proj.weight"), ("Wfc", "mlp.c_fc.weight"),
                          ("Wpr", "mlp.c_proj.weight")):
            got = getattr(mg, attr)
            assert got.dtype == torch.bfloat16 and torch.equal(got, fs[pre + key].float().to(torch.bfloat16)), (i, attr)
        for attr, key in (("bqkv", "attn.in_proj_bias"), ("bo", "attn.out_proj.bias"), ("bfc", "mlp.c_fc.bias"),
                          ("bpr", "mlp.c_proj.bias")):
            got = getattr(mg, attr)
            assert got.dtype == torch.float32 and torch.equal(got, fs[pre + key].float()), (i, attr)
        assert hasattr(mg, "tad") == c["tcls"]


def test_refusals():
    import aim_amd
    kw = dict(input_resolution=32, num_frames=8, patch_size=16, width=128, layers=1, heads=2, drop_path_rate=0.0,
              linear_adapter=True)
    for r in (192, 136, 100, 36, 4, 0):            # above the width; not a multiple of 8; below 8
        with pytest.raises(NotImplementedError, match="linear_adapter"):
            aim_amd.ViT_CLIP_ZEROI2V(**kw, bottleneck=r)
    with pytest.raises(NotImplementedError, match="linear_adapter"):      # within the width, above the kernels' 256
        aim_amd.ViT_CLIP_ZEROI2V(**dict(kw, width=512, heads=8), bottleneck=264)
    with pytest.raises(TypeError, match="num_tadapter"):
        aim_amd.ViT_CLIP_ZEROI2V(**kw, bottleneck=32, num_tadapter=2, with_t_cls_token=True)
    for D, H, r in ((768, 12, 192), (1024, 16, 256)):                     # every recipe-sized model is inside the limit
        m = aim_amd.ViT_CLIP_ZEROI2V(224, 8, 16, D, 1, H, 0.0, bottleneck=r, linear_adapter=True)
        assert m.transformer.resblocks[0].Attn_Adapter_q.D_fc1.weight.shape == (r, D)
    m = aim_amd.ViT_CLIP_ZEROI2V(**kw, bottleneck=32)
    with pytest.raises(NotImplementedError, match="fp32"):                # fp32 mode and fp8 stay as they are
        m.set_precision('fp32')
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 8, 32, 32))
    with pytest.raises(RuntimeError, match="linear_adapter"):             # nothing to fold without linear adapters
        aim_amd.ViT_CLIP_ZEROI2V(**dict(kw, linear_adapter=False)).merge_adapters()


def test_merged_with_gradients_raises():
    import aim_amd
    m = aim_amd.ViT_CLIP_ZEROI2V(32, 8, 16, 128, 1, 2, 0.0, with_t_cls_token=True, bottleneck=32, linear_adapter=True)
    m.init_weights()
    assert not m.merged
    assert m.merge_adapters() is m and m.merged
    x = torch.zeros(1, 3, 8, 32, 32)
    with pytest.raises(RuntimeError, match="merged"):
        m(x)
    with torch.no_grad():                                                 # allowed: fails later, at the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x)
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # nothing needs a gradient
        m(x)
    assert m.unmerge_adapters() is m and not m.merged
    # the fold follows the adapters: same operands while nothing changed, new ones after an in-place update
    m.merge_adapters()
    a = m._merged_operands()
    assert m._merged_operands() is a
    with torch.no_grad():
        m.transformer.resblocks[0].Attn_Adapter_out.D_fc2.weight.add_(0.01)
    b = m._merged_operands()
    assert b is not a and not torch.equal(a[0].Wo, b[0].Wo) and torch.equal(a[0].Wfc, b[0].Wfc)
    m.weights_epoch += 1                                                  # what dist.FlatAdamW.step() does
    assert m._merged_operands() is not b


def test_register_into_mmaction_registers_the_backbone(monkeypatch):
    import aim_amd
    from aim_amd.registry import register_into_mmaction

    class Reg:
        def __init__(self):
            self.mods = {}

        def register_module(self, name=None, force=False, module=None):
            assert force
            self.mods[name] = module

    reg = Reg()
    builder = types.ModuleType("mmaction.models.builder")
    builder.BACKBONES = reg
    for name in ("mmaction", "mmaction.models"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.setitem(sys.modules, "mmaction.models.builder", builder)
    assert register_into_mmaction() is True
    assert reg.mods["ViT_CLIP_ZEROI2V"] is aim_amd.ViT_CLIP_ZEROI2V and reg.mods["ViT_CLIP"] is aim_amd.ViT_CLIP
