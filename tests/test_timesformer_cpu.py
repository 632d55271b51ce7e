"""TimeSformer's host surface (no GPU): the reference's recipe through Config.fromfile -> build_model, its parameter names,
order and shapes, the init policy (nothing frozen, T_Adapter not zeroed), the refusals, the CLIP key mapping, and the plain-torch
restatement (tests/timesformer_ref.py) against the reference's own outputs and gradients (tests/golden/timesformer_tiny_*.npz)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
with open(os.path.join(GOLDEN, "reference_timesformer_configs.json")) as _f:
    CONFIGS = json.load(_f)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MG = _load("make_golden_timesformer", os.path.join(GOLDEN, "make_golden_timesformer.py"))
REF = _load("timesformer_ref", os.path.join(HERE, "timesformer_ref.py"))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _value(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_value(v) for v in o["__tuple__"])
        return {k: _value(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_value(v) for v in o]
    return o


def _write_config_tree(root):
    for r, d in CONFIGS.items():
        path = os.path.join(root, r)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for k, v in d.items():
                f.write(f"{k} = {_value(v)!r}\n")


def _build(tag):
    import aim_amd
    T, train, kw, seed = MG.CASES[tag]
    m = aim_amd.TimeSformer(num_frames=T, **MG.GEOM, **kw)
    m.init_weights()
    return m, T, train, seed


def fixture_factors(z, L):
    """the six stored masks as ``_drop_factors`` returns them: layer 0 draws none, layers 1.. draw (T,), (N,), (N,) each"""
    out = [(None, None, None)]
    for i in range(1, L):
        out.append(tuple(torch.from_numpy(z[f"mask.{3 * (i - 1) + j}"]) for j in range(3)))
    return out


def fixture_errors(z, names, y, grads, seed):
    """rel-L2 of the output and of every gradient against a fixture (whole tensors, or the stored sample, norm and sum)"""
    errs = {"y": rel(y, torch.from_numpy(z["y"]))}
    for k, (n, gr) in enumerate(zip(names, grads)):
        assert gr is not None, n
        if "grad." + n in z:
            errs[n] = rel(gr, torch.from_numpy(z["grad." + n]))
        else:
            flat = gr.reshape(-1).cpu()
            idx = MG.sample_index(flat.numel(), seed * 1000 + k)
            errs[n] = rel(flat[idx], torch.from_numpy(z["grad." + n + ".val"]))
            ref_norm = float(z["grad." + n + ".sq"]) ** 0.5
            errs[n + "|norm"] = abs(float(flat.double().norm()) - ref_norm) / ref_norm
            # the whole tensor's sum: |sum(err)| <= sqrt(numel) ||err||, so it is scaled by sqrt(numel) ||g_ref||
            errs[n + "|sum"] = abs(float(flat.double().sum()) - float(z["grad." + n + ".sum"])) / (ref_norm * flat.numel() ** 0.5)
    return errs


def test_reference_recipe_builds(tmp_path):
    import aim_amd
    from aim_amd.dist import build_optimizer
    _write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(str(tmp_path / "recognition" / "vit" / "timesformer_k400.py"))
    model = aim_amd.build_model(cfg.model)
    bb = model.backbone
    assert isinstance(bb, aim_amd.TimeSformer)
    assert (bb.width, bb.layers, bb.heads, bb.num_frames, bb.input_resolution, bb.patch_size) == (768, 12, 12, 8, 224, 16)
    assert bb.tadapter and tuple(bb.temporal_embedding.shape) == (1, 8, 768)
    rates = [blk.drop_prob for blk in bb.transformer.resblocks]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.1) < 1e-6
    assert len(list(bb.parameters())) == 6 + 20 * 12 + 2 and all(p.requires_grad for p in bb.parameters())
    assert model.cls_head.num_classes == 400
    opt = build_optimizer(model, dict(cfg.optimizer))
    names = {id(p): n for n, p in model.named_parameters()}
    keys = ("class_embedding", "positional_embedding", "ln_1", "ln_2", "ln_pre", "ln_post")
    n_params = 0
    for g in opt.param_groups:
        for p in g["params"]:
            n_params += 1
            n = names[id(p)]
            assert g["weight_decay"] == (0.0 if any(k in n for k in keys) else cfg.optimizer["weight_decay"]), n
    assert n_params == len(list(model.parameters()))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_parameter_names_order_and_shapes_match_reference(tag):
    z = np.load(os.path.join(GOLDEN, f"timesformer_tiny_{tag}.npz"))
    m, T, train, seed = _build(tag)
    assert [n for n, _ in m.named_parameters()] == [str(n) for n in z["names"]]
    assert list(m.state_dict()) == [str(n) for n in z["names"]]
    for n, p in m.named_parameters():
        assert tuple(int(v) for v in z["shape." + n]) == tuple(p.shape), n
    assert all(p.requires_grad for p in m.parameters())
    assert ("temporal_embedding" in dict(m.named_parameters())) == (tag != "c")
    assert len(list(m.parameters())) == 6 + 20 * MG.GEOM["layers"] + 2 - (tag == "c")


def test_init_weights_policy():
    m, _, _, _ = _build("a")
    norm = lambda n: ".ln_" in n or ".t_norm." in n or n.startswith(("ln_pre", "ln_post"))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("T_Adapter.weight"):          # trunc_normal_(std=.02), NOT zeroed: the zeroing loops look for D_fc2
                assert 0.015 < float(p.std()) < 0.025, n
            elif n.endswith("bias"):
                assert float(p.abs().max()) == 0, n
            elif norm(n):
                assert torch.equal(p, torch.ones_like(p)), n
    assert m.no_weight_decay() == {'absolute_pos_embed', 'temporal_embedding'}
    assert m.no_weight_decay_keywords() == {'relative_position_bias_table', 'temporal_position_bias_table'}
    with pytest.raises(TypeError):
        m.init_weights(pretrained=3)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(heads=4), ValueError, "head_dim 64"),
    (dict(input_resolution=16 * 17), ValueError, "290 tokens per frame"),
    (dict(num_frames=33), ValueError, "33 frames"),
])
def test_constructor_refusals(kw, exc, match):
    import aim_amd
    args = dict(MG.GEOM, num_frames=2, drop_path_rate=0.0)
    args.update(kw)
    with pytest.raises(exc, match=match):
        aim_amd.TimeSformer(**args)


def test_forward_and_pretrained_refusals():
    import aim_amd
    m = aim_amd.TimeSformer(num_frames=2, drop_path_rate=0.0, **MG.GEOM)
    with pytest.raises(RuntimeError, match="TimeSformer runs on MI355X only"):
        m(torch.zeros(1, 3, 2, 32, 32))
    try:
        import clip  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="needs the OpenAI `clip` package"):
            m.init_weights(pretrained="clip")
    assert m.set_precision('fp32').precision == 'fp32' and m.set_precision('bf16').precision == 'bf16'
    with pytest.raises(ValueError):
        m.set_precision('fp16')
    assert m.set_inference_precision('fp8').inference_precision == 'fp8'
    assert aim_amd.BACKBONES.get("TimeSformer") is aim_amd.TimeSformer


class _Meta:
    """stands in for a CUDA clip: the shape checks of ``forward`` come behind the device check"""
    is_cuda = True
    dtype = torch.float32

    def __init__(self, shape):
        self.shape = shape


@pytest.mark.parametrize("shape,match", [((1, 3, 4, 32, 32), "expected 2 frames"), ((1, 3, 2, 48, 48), "expected input")])
def test_wrong_clip_shape_is_refused(shape, match):
    import aim_amd
    m = aim_amd.TimeSformer(num_frames=2, drop_path_rate=0.0, **MG.GEOM)
    with pytest.raises(ValueError, match=match):
        m(_Meta(shape))


def test_clip_key_mapping_loads_strict():
    import aim_amd
    from aim_amd.timesformer import clip_state_dict
    clip_like = aim_amd.ViT_CLIP(num_frames=2, drop_path_rate=0.0, **MG.GEOM)
    gen = torch.Generator().manual_seed(5)
    visual = {k: torch.randn(v.shape, generator=gen) for k, v in clip_like.state_dict().items()
              if "Adapter" not in k and k != "temporal_embedding"}
    visual["proj"] = torch.randn(128, 64, generator=gen)
    m = aim_amd.TimeSformer(num_frames=2, drop_path_rate=0.0, **MG.GEOM)
    m.init_weights()
    tad = m.transformer.resblocks[1].T_Adapter.weight.detach().clone()
    mapped = clip_state_dict(visual, m)
    assert "proj" not in mapped
    msg = m.load_state_dict(mapped, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    for blk in m.transformer.resblocks:
        assert torch.equal(blk.t_attn.in_proj_weight, blk.attn.in_proj_weight)
        assert torch.equal(blk.t_attn.in_proj_bias, blk.attn.in_proj_bias)
        assert torch.equal(blk.t_attn.out_proj.weight, blk.attn.out_proj.weight)
        assert torch.equal(blk.t_attn.out_proj.bias, blk.attn.out_proj.bias)
        assert torch.equal(blk.t_norm.weight, blk.ln_1.weight) and torch.equal(blk.t_norm.bias, blk.ln_1.bias)
    assert torch.equal(m.conv1.weight, visual["conv1.weight"])
    assert torch.equal(m.transformer.resblocks[2].attn.in_proj_weight, visual["transformer.resblocks.2.attn.in_proj_weight"])
    assert torch.equal(m.transformer.resblocks[1].T_Adapter.weight, tad)
    # a source that already carries t_attn / t_norm keeps its own (timesformer.py:145-148)
    own = dict(visual)
    own["transformer.resblocks.0.t_norm.weight"] = torch.full((128,), 7.0)
    assert torch.equal(clip_state_dict(own, m)["transformer.resblocks.0.t_norm.weight"], torch.full((128,), 7.0))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_matches_reference_fixture(tag):
    """tests/timesformer_ref.py in fp32 on the CPU, with the stored masks: output and every gradient within 1e-5 rel-L2"""
    z = np.load(os.path.join(GOLDEN, f"timesformer_tiny_{tag}.npz"))
    T, train, kw, seed = MG.CASES[tag]
    names = [str(n) for n in z["names"]]
    shapes = [(n, tuple(int(v) for v in z["shape." + n])) for n in names]
    P = {n: v.clone().requires_grad_(True) for n, v in MG.synth_params(shapes, seed).items()}
    res = MG.GEOM["input_resolution"]
    imgs = MG.randn((MG.B, 3, T, res, res), seed + 1)
    g = MG.randn((MG.B, MG.GEOM["width"], T, 1, 1), seed + 2)
    factors = fixture_factors(z, MG.GEOM["layers"]) if train else None
    y = REF.forward(P, imgs, MG.GEOM["heads"], MG.GEOM["patch_size"], factors)
    grads = torch.autograd.grad(y, [P[n] for n in names], g)
    errs = fixture_errors(z, names, y, grads, seed)
    worst = max(errs.items(), key=lambda kv: kv[1])
    assert worst[1] <= 1e-5, (worst, sorted(errs.items(), key=lambda kv: -kv[1])[:8])


def test_drop_factors_shapes_and_eval_identity():
    m, T, _, _ = _build("b")
    N = 5
    m.train()
    torch.manual_seed(0)
    fac = m._drop_factors(T, N, True, torch.device("cpu"))
    assert len(fac) == 3 and fac[0] == (None, None, None)
    for i in (1, 2):
        keep = 1.0 - m.transformer.resblocks[i].drop_prob
        assert [tuple(v.shape) for v in fac[i]] == [(T,), (N,), (N,)]
        for v in fac[i]:
            assert set(v.tolist()) <= {0.0, float(torch.tensor(1.0 / keep, dtype=torch.float32))}
    assert m._drop_factors(T, N, False, torch.device("cpu")) == [(None, None, None)] * 3
    f1, f2, f3 = m._expand_factors(fac, 2)[1]
    assert torch.equal(f1, fac[1][0].repeat(2)) and torch.equal(f2, fac[1][1]) and torch.equal(f3, fac[1][2])
