"""ViT_CLIP_ZEROI2V(linear_adapter=True) on the MI355X: the whole backbone against the real reference's stored outputs and
autograd gradients (tests/golden/zeroi2v_linear_tiny_{a,b,c,d}.npz: separate and shared attention adapters, 8 / 16 / 32
frames, with and without the temporal class token), at ViT-B's real shape against the fp32 restatement
tests/zeroi2v_linear_ref.py (itself held to the fixtures by tests/test_zeroi2v_linear_cpu.py), the same at a small shape with
the bottlenecks 8, 72, 136, 200 and 248 that no fixture has, merging, the requires_grad
contract, and two FlatAdamW steps of the sthv2 recipe in a child process.

Bounds: 1.5e-2 rel-L2 on the bf16 output and 2.5e-2 on every trainable gradient -- the project's bounds for bf16 against an
fp32 reference fixture (tests/test_zeroi2v_gpu.py).  The two biases of Attn_Adapter_k have a gradient that is zero by the
algebra (test_zeroi2v_linear_cpu.null_sibling): their error is measured against the norm of Attn_Adapter_q's tensor of the
same name.  The fixtures' outputs move by at least 0.20 rel-L2 when the attention adapters or the MLP adapters are removed and
by 0.70 when the doubled skip is un-doubled, so a backbone that dropped one of them could not pass.

Measured on MI355X (worst over a fixture's tensors): see DESIGN.md section 2d."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_zeroi2v_linear_cpu as C  # noqa: E402  (load_case, build, null_sibling)
import zeroi2v_linear_ref as ZL  # noqa: E402
from test_zeroi2v_cpu import stored_grad  # noqa: E402

OUT_BOUND, GRAD_BOUND = 1.5e-2, 2.5e-2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build(c):
    m = C.build(c)
    m.load_state_dict(c["st"], strict=True)
    return m.to(DEV).train(c["train"])


def grad_errors(names, got, ref):
    """{name: rel-L2 error}; the analytically zero gradients against their sibling's norm"""
    errs = {}
    for n in names:
        sib = C.null_sibling(n)
        if sib is None:
            errs[n] = rel(got[n], ref[n])
        else:
            errs[n + "|vs " + sib.split(".")[-3]] = float((got[n].double().cpu() - ref[n].double().cpu()).norm()
                                                          / ref[sib].double().cpu().norm())
    return errs


@pytest.mark.parametrize("tag", C.TAGS)
def test_bf16_against_reference_fixture(tag):
    c = C.load_case(tag)
    z = c["z"]
    m = build(c)
    y = m(c["imgs"].to(DEV))
    names = [str(n) for n in z["trainable"]]
    byname = dict(m.named_parameters())
    grads = torch.autograd.grad(y, [byname[n] for n in names], c["g"].to(DEV))
    ey = rel(y, torch.from_numpy(z["y"]))
    got, ref, extra = {}, {}, {}
    for k, (n, g) in enumerate(zip(names, grads)):
        r_, g_, rsum, rsq = stored_grad(z, n, k, c["seed"], g.cpu())
        ref[n], got[n] = r_, g_
        if rsq is not None and C.null_sibling(n) is None:          # the elements that were not sampled
            extra[n + "|norm"] = abs(float(g.double().norm()) - rsq ** 0.5) / rsq ** 0.5
            extra[n + "|sum"] = abs(float(g.double().sum()) - rsum) / (rsq ** 0.5 * g.numel() ** 0.5)
    errs = dict(grad_errors(names, got, ref), **extra)
    worst_g = max(errs.items(), key=lambda kv: kv[1])
    print(f"zeroi2v linear fixture {tag}: output {ey:.3e}, worst gradient {worst_g[1]:.3e} ({worst_g[0]})")
    assert ey <= OUT_BOUND, ey
    assert worst_g[1] <= GRAD_BOUND, sorted(errs.items(), key=lambda kv: -kv[1])[:8]


def test_real_shape_against_the_restatement():
    """ViT-B width at 224 x 224 (198 tokens with the temporal class token), 2 layers, 8 frames, 2 clips, separate q / k / v
    adapters at the recipes' bottleneck 192; reference = tests/zeroi2v_linear_ref.py in fp32 on the CPU"""
    import aim_amd
    from oracle import vit_clip_oracle as O
    D, H, L, T, B, r = 768, 12, 2, 8, 2, 192
    st = O.synth_state_dict(ZL.backbone_param_shapes(224, T, 16, D, L, True, False, r), seed=78)
    for k in st:
        if ("Attn_Adapter" in k or "MLP_Adapter" in k) and k.endswith(".weight"):
            st[k] = st[k] * C.ADAPTER_SCALE
    m = aim_amd.ViT_CLIP_ZEROI2V(224, T, 16, D, L, H, drop_path_rate=0.0, with_t_cls_token=True, bottleneck=r,
                                 linear_adapter=True)
    m.init_weights()
    m.load_state_dict(st, strict=True)
    m = m.to(DEV).eval()
    gen = torch.Generator().manual_seed(9)
    imgs = torch.randn((B, 3, T, 224, 224), generator=gen)
    g = torch.randn((B, D, T, 1, 1), generator=gen)
    y = m(imgs.to(DEV))
    names = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert len(names) == 28 * L + 3
    byname = dict(m.named_parameters())
    grads = torch.autograd.grad(y, [byname[n] for n in names], g.to(DEV))
    sr = {k: v.clone().requires_grad_(k in names) for k, v in st.items()}
    torch.set_num_threads(16)
    yr = ZL.backbone(imgs, sr, H, T, True, False)
    gr = torch.autograd.grad(yr, [sr[n] for n in names], g)
    errs = grad_errors(names, dict(zip(names, grads)), dict(zip(names, gr)))
    ey = rel(y, yr.detach())
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"zeroi2v linear real shape: output {ey:.3e}, worst gradient {worst[1]:.3e} ({worst[0]})")
    assert ey <= OUT_BOUND, ey
    assert worst[1] <= GRAD_BOUND, sorted(errs.items(), key=lambda kv: -kv[1])[:8]


@pytest.mark.parametrize("bottleneck,share", [(8, False), (72, True), (136, False), (200, False), (248, False)])
def test_uncommon_bottlenecks_against_the_restatement(bottleneck, share):
    """The bottlenecks no fixture has: the smallest (8), and one with a partial last 64-chunk per rk = 2, 3, 4 (72, 136, 200,
    248; the last two take the 32-row backward of the q / k / v adapters).  Width 256, 4 heads, 2 layers, 8 frames of 32 x 32,
    2 clips, with the temporal class token; reference = tests/zeroi2v_linear_ref.py in fp32 on the CPU; every call twice."""
    import aim_amd
    from oracle import vit_clip_oracle as O
    D, H, L, T, B = 256, 4, 2, 8, 2
    st = O.synth_state_dict(ZL.backbone_param_shapes(32, T, 16, D, L, True, share, bottleneck), seed=79)
    for k in st:
        if ("Attn_Adapter" in k or "MLP_Adapter" in k) and k.endswith(".weight"):
            st[k] = st[k] * C.ADAPTER_SCALE
    m = aim_amd.ViT_CLIP_ZEROI2V(32, T, 16, D, L, H, drop_path_rate=0.0, with_t_cls_token=True, share_adapter=share,
                                 bottleneck=bottleneck, linear_adapter=True)
    m.init_weights()
    m.load_state_dict(st, strict=True)
    m = m.to(DEV).eval()
    gen = torch.Generator().manual_seed(10)
    imgs = torch.randn((B, 3, T, 32, 32), generator=gen)
    g = torch.randn((B, D, T, 1, 1), generator=gen)
    names = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert len(names) == (20 if share else 28) * L + 3
    byname = dict(m.named_parameters())
    y = m(imgs.to(DEV))
    grads = torch.autograd.grad(y, [byname[n] for n in names], g.to(DEV))
    y2 = m(imgs.to(DEV))
    grads2 = torch.autograd.grad(y2, [byname[n] for n in names], g.to(DEV))
    sr = {k: v.clone().requires_grad_(k in names) for k, v in st.items()}
    yr = ZL.backbone(imgs, sr, H, T, True, share)
    gr = torch.autograd.grad(yr, [sr[n] for n in names], g)
    errs = grad_errors(names, dict(zip(names, grads)), dict(zip(names, gr)))
    ey = rel(y, yr.detach())
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"zeroi2v linear bottleneck {bottleneck}{' shared' if share else ''}: output {ey:.3e}, "
          f"worst gradient {worst[1]:.3e} ({worst[0]})")
    assert ey <= OUT_BOUND, ey
    assert worst[1] <= GRAD_BOUND, sorted(errs.items(), key=lambda kv: -kv[1])[:8]
    assert torch.equal(y.detach(), y2.detach())
    for n, a, b in zip(names, grads, grads2):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("tag", C.TAGS)
def test_merged_forward(tag, monkeypatch):
    """merged: within the output bound of the fixture and of the unmerged forward, no call to the low-rank wrappers and no
    GEMM beyond the frozen model's; a forward that needs gradients raises; the fold follows an optimizer step"""
    from aim_amd import ops
    c = C.load_case(tag)
    z = c["z"]
    m = build(c).eval()
    imgs = c["imgs"].to(DEV)
    with torch.no_grad():
        y = m(imgs)
    calls = {"lowrank_fwd": 0, "lowrank_bwd": 0, "gemm": 0}
    for name in calls:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    with torch.no_grad():
        y2 = m(imgs)
    # an unmerged block's forward: the attention adapters in one call (G = 3 or 1), Attn_Adapter_out, MLP_Adapter_in, _out
    assert torch.equal(y, y2) and calls["lowrank_fwd"] == 4 * c["L"] and calls["lowrank_bwd"] == 0
    m.merge_adapters()
    assert m.merged
    calls.update(lowrank_fwd=0, lowrank_bwd=0, gemm=0)
    with torch.no_grad():
        ym = m(imgs)
    assert calls["lowrank_fwd"] == 0 and calls["lowrank_bwd"] == 0
    # patch embedding + per block QKV, out_proj, c_fc, c_proj (+ the class chain's QKV, out_proj and two T_Adapter GEMMs)
    assert calls["gemm"] == 1 + c["L"] * (4 + (4 if c["tcls"] else 0))
    e_fix, e_un = rel(ym, torch.from_numpy(z["y"])), rel(ym, y)
    print(f"zeroi2v linear merged {tag}: against the fixture {e_fix:.3e}, against the unmerged forward {e_un:.3e}")
    assert e_fix <= OUT_BOUND and e_un <= OUT_BOUND
    with pytest.raises(RuntimeError, match="merged"):
        m(imgs)
    # one optimizer step on the unmerged model, then merged again: the fold is redone from the new adapters
    m.unmerge_adapters()
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    m(imgs).backward(c["g"].to(DEV))
    opt.step()
    m.merge_adapters()
    with torch.no_grad():
        ym2 = m(imgs)
        y3 = m.unmerge_adapters()(imgs)
    assert not torch.equal(ym2, ym) and rel(y3, y) > 1e-4          # the step moved the model ...
    assert rel(ym2, y3) <= OUT_BOUND                               # ... and the merged operands followed it


def test_frozen_tensors_get_no_gradient_and_reruns_give_equal_bits():
    c = C.load_case("a")
    m = build(c)
    imgs = c["imgs"].to(DEV)
    y = m(imgs)
    y.backward(c["g"].to(DEV))
    train = {str(n) for n in c["z"]["trainable"]}
    for n, p in m.named_parameters():
        assert (p.grad is not None) == (n in train), n
        assert p.requires_grad == (n in train), n
    with torch.no_grad():
        y2 = m(imgs)
    assert torch.equal(y.detach(), y2) and not y2.requires_grad
    g1 = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    y3 = m(imgs)
    y3.backward(c["g"].to(DEV))
    assert torch.equal(y3.detach(), y.detach())
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g1[n]), n
    # the requires_grad contract: a tensor switched off gets no gradient, the others the same bits
    m.zero_grad(set_to_none=True)
    off = "transformer.resblocks.1.Attn_Adapter_v.D_fc1.weight"
    dict(m.named_parameters())[off].requires_grad_(False)
    m(imgs).backward(c["g"].to(DEV))
    for n, p in m.named_parameters():
        assert (p.grad is None) == (n not in train or n == off), n
        if p.grad is not None:
            assert torch.equal(p.grad, g1[n]), n


def test_fp8_request_warns_and_runs_bf16(caplog):
    c = C.load_case("d")
    m = build(c)
    imgs = c["imgs"].to(DEV)
    with torch.no_grad():
        y = m(imgs)
        m.set_inference_precision('fp8')
        with caplog.at_level("WARNING", logger="aim_amd"):
            y8 = m(imgs)
    assert torch.equal(y, y8)
    assert any("fp8" in r.getMessage() and "bf16" in r.getMessage() for r in caplog.records)


@pytest.fixture(scope="module")
def training_runs(tmp_path_factory):
    """the sthv2 recipe with linear adapters: two FlatAdamW steps and a merged forward, in two child processes"""
    out = {}
    for tag in ("run1", "run2"):
        path = str(tmp_path_factory.mktemp("zeroi2v_linear_train") / f"{tag}.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "zeroi2v_linear_train_child.py"), path], timeout=600,
                           capture_output=True, text=True)
        if p.returncode != 0:        # stop at the first failing child: nothing more is started on the GPU
            pytest.fail(f"{tag}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[tag] = json.load(f)
    return out


def test_recipe_training_is_finite_and_changes_exactly_the_trainable_set(training_runs):
    r = training_runs["run1"]
    assert r["backbone"] == "ViT_CLIP_ZEROI2V" and r["linear"] and not r["share"] and r["tcls"] and r["optimizer"] == "FlatAdamW"
    assert r["in_place"] and r["finite"] and all(v == v and abs(v) < 1e4 for v in r["losses"])
    assert len(r["trainable"]) == 28 * 12 + 3 + 2
    changed = sorted(n for n in r["before"] if r["before"][n] != r["after"][n])
    assert changed == r["trainable"]
    assert r["merged_finite"] and r["merged_rel"] <= OUT_BOUND, r["merged_rel"]     # the fold followed FlatAdamW's raw writes


def test_recipe_training_is_bitwise_reproducible(training_runs):
    a, b = training_runs["run1"], training_runs["run2"]
    assert a["loss_bits"] == b["loss_bits"] and a["after"] == b["after"] and a["merged_bits"] == b["merged_bits"]
