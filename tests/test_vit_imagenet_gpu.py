"""ViT_ImageNet on the MI355X: the new kernels against float64 torch, the whole backbone against the reference's own
outputs and gradients (tests/golden/vit_imagenet_tiny_{a,b,c}.npz), the requires_grad contract, optimizer steps that rewrite
the weights, and the k400 / ssv2 configs at their per-GPU shape."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location("make_golden_imagenet", os.path.join(HERE, "golden", "make_golden_imagenet.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_embed_nopre_fwd_bwd_vs_fp64():
    from aim_amd import ops
    g = torch.Generator().manual_seed(1)
    for (B, T, N, D) in ((2, 2, 5, 128), (2, 8, 197, 768)):
        BT = B * T
        tok, cls = torch.randn((BT * (N - 1), D), generator=g), torch.randn(D, generator=g)
        pos, tmp = torch.randn((N, D), generator=g), torch.randn((T, D), generator=g)
        x = torch.empty((BT * N, D), device=DEV)
        ops.embed_nopre_fwd(tok.to(DEV), cls.to(DEV), pos.to(DEV), tmp.to(DEV), x, B, T, N, D)
        ref = torch.cat([cls.double().expand(BT, 1, D), tok.double().view(BT, N - 1, D)], 1) + pos.double()
        ref = (ref.view(B, T, N, D) + tmp.double().view(1, T, 1, D)).reshape(BT * N, D)
        assert rel(x, ref) < 1e-7
        dx = torch.randn((BT * N, D), generator=g).to(torch.bfloat16)
        outs = []
        for _ in range(2):
            dcls, dpos = torch.ones(D, device=DEV), torch.ones((N, D), device=DEV)
            dtmp, db = torch.ones((T, D), device=DEV), torch.ones(D, device=DEV)
            dtok = torch.empty((BT * (N - 1), D), dtype=torch.bfloat16, device=DEV)
            ops.embed_nopre_bwd(dx.to(DEV), B, T, N, D, dtok=dtok, dcls=dcls, dpos=dpos, dtemporal=dtmp, dbias=db)
            outs.append([t.cpu() for t in (dcls, dpos, dtmp, db, dtok)])
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        d = dx.double().view(B, T, N, D)
        dcls, dpos, dtmp, db, dtok = outs[0]
        assert rel(dcls - 1, d[:, :, 0].sum((0, 1))) < 1e-6
        assert rel(dpos - 1, d.sum((0, 1))) < 1e-6
        assert rel(dtmp - 1, d.sum((0, 2))) < 1e-6
        assert rel(db - 1, d[:, :, 1:].sum((0, 1, 2))) < 1e-6
        assert torch.equal(dtok, dx.view(BT, N, D)[:, 1:].reshape(-1, D))


def test_layernorm_gamma_beta_grad_100k_rows():
    """M = 100 864 rows (64 clips x 8 frames x 197 tokens), bf16 dy: fp64 agreement and bitwise reproducibility."""
    from aim_amd import ops
    M, D = 100864, 768
    g = torch.Generator().manual_seed(2)
    x = (torch.randn((M, D), generator=g) * 2 + 0.3).to(DEV)
    dy = torch.randn((M, D), generator=g).to(torch.bfloat16).to(DEV)
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-6).rsqrt()
    res = []
    for _ in range(2):
        dg, dbt = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        ops.layernorm_gb_bwd(dy, x, mean.float(), rstd.float(), M, D, dg, dbt)
        res.append((dg.cpu(), dbt.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    xhat = (x.double() - mean[:, None]) * rstd[:, None]
    assert rel(res[0][0], (dy.double() * xhat).sum(0)) < 1e-5
    assert rel(res[0][1], dy.double().sum(0)) < 1e-5


def test_per_frame_row_factors_vs_fp64():
    """The per-frame DropPath form: ACT / DACT epilogues with ``af`` (index m / ntok), the F32 epilogue with a per-frame
    bias row ``vec`` (ldv = D), and the per-frame-weighted bias column sum; at N = 197 (256 x 256 kernel) and N = 5."""
    from aim_amd import ops
    g = torch.Generator().manual_seed(3)
    for BT, N, D, r in ((16, 197, 768, 192), (8, 5, 128, 32)):
        M = BT * N
        a = torch.randn((M, D), generator=g).to(torch.bfloat16)
        w1 = (torch.randn((r, D), generator=g) / D ** 0.5).to(torch.bfloat16)
        b1 = torch.randn(r, generator=g) * 0.1
        af = (torch.rand(BT, generator=g) < 0.6).float() * 1.7
        af_rows = af.repeat_interleave(N).double()
        x0 = torch.randn((M, D), generator=g)
        w2 = (torch.randn((D, r), generator=g) / r ** 0.5).to(torch.bfloat16)
        b2 = torch.randn(D, generator=g)
        res = []
        for _ in range(2):
            h, pre = torch.empty((M, r), dtype=torch.bfloat16, device=DEV), torch.empty((M, r), dtype=torch.bfloat16, device=DEV)
            ops.gemm(a.to(DEV), w1.to(DEV), ops.EPI_ACT, h, bias=b1.to(DEV), out2=pre, act=ops.ACT_GELU, af=af.to(DEV), ntok=N)
            y = torch.empty((M, D), device=DEV)
            ops.gemm(h, w2.to(DEV), ops.EPI_F32, y, resid=x0.to(DEV), vec=af.to(DEV)[:, None] * b2.to(DEV)[None, :], ntok=N)
            db = torch.zeros(D, device=DEV)
            ops.colsum(a.to(DEV), db, af=af.to(DEV), ntok=N)
            res.append([t.cpu() for t in (h, pre, y, db)])
        for u, v in zip(*res):
            assert torch.equal(u, v)
        h, pre, y, db = res[0]
        pre64 = a.double() @ w1.double().T + b1.double()
        assert rel(pre.float(), pre64) < 1e-2
        assert rel(h.float(), af_rows[:, None] * torch.nn.functional.gelu(pre64)) < 1e-2
        y64 = x0.double() + h.double() @ w2.double().T + af_rows[:, None] * b2.double()
        assert rel(y, y64) < 1e-5
        assert rel(db, (af_rows[:, None] * a.double()).sum(0)) < 1e-5
        # DACT with af: d(pre) = af[f] * GELU'(pre) * (dy W2)
        dy = torch.randn((M, D), generator=g).to(torch.bfloat16)
        dpre = torch.empty((M, r), dtype=torch.bfloat16, device=DEV)
        ops.gemm(dy.to(DEV), w2.T.contiguous().to(DEV), ops.EPI_DACT, dpre, aux=pre.to(DEV), act=ops.ACT_GELU, af=af.to(DEV),
                 ntok=N)
        p64 = pre.double().requires_grad_(True)
        gd, = torch.autograd.grad(torch.nn.functional.gelu(p64).sum(), p64)
        assert rel(dpre.cpu().float(), af_rows[:, None] * gd * (dy.double() @ w2.double())) < 1e-2


@pytest.mark.parametrize("Nw,Kw", [(2304, 768), (768, 768), (3072, 768), (768, 3072)])
def test_wgrad_frozen_sizes_vs_fp64(Nw, Kw):
    from aim_amd import ops
    M = 12608          # 8 clips x 8 frames x 197 tokens
    g = torch.Generator().manual_seed(Nw + Kw)
    G = torch.randn((M, Nw), generator=g).to(torch.bfloat16)
    A = torch.randn((M, Kw), generator=g).to(torch.bfloat16)
    res = []
    for _ in range(2):
        dw, db = torch.zeros((Nw, Kw), device=DEV), torch.zeros(Nw, device=DEV)
        ops.wgrad(G.to(DEV), A.to(DEV), dw, db)
        res.append((dw.cpu(), db.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert rel(res[0][0], G.double().T @ A.double()) < 1e-5
    assert rel(res[0][1], G.double().sum(0)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# whole backbone against the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------
def _build(tag, **extra):
    import aim_amd
    T, train, kw, seed = MG.CASES[tag]
    m = aim_amd.ViT_ImageNet(num_frames=T, **MG.GEOM, **kw, **extra)
    m.init_weights()
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    m.load_state_dict(MG.synth_params(shapes, seed), strict=True)
    m = m.to(DEV).train(train)
    return m, T, train, seed


def _inject_masks(m, masks, B, T):
    """The reference's drawn masks (layers 1 and 2, temporal then MLP) as the model's [L, 2, B*T] factors."""
    L = len(m.blocks)
    fac = torch.empty((L, 2, B * T))
    for i, blk in enumerate(m.blocks):
        fac[i, 0], fac[i, 1] = 1.0, float(blk.scale)
    for k in range(masks.shape[0]):
        i, j = 1 + k // 2, k % 2
        fac[i, j] = masks[k] * (float(m.blocks[i].scale) if j == 1 else 1.0)
    fac = fac.to(DEV)
    m._drop_masks = lambda BT, training, dev: fac


def _run(tag, bound, precision="bf16"):
    z = np.load(os.path.join(HERE, "golden", f"vit_imagenet_tiny_{tag}.npz"))
    m, T, train, seed = _build(tag)
    m.set_precision(precision)
    B = MG.B
    if train:
        _inject_masks(m, torch.from_numpy(z["masks"]), B, T)
    imgs = MG.randn((B, 3, T, 32, 32), seed + 1).to(DEV)
    g = MG.randn((B, MG.GEOM["embed_dim"], T, 1, 1), seed + 2).to(DEV)
    names = [str(n) for n in z["names"]]
    assert names == [n for n, _ in m.named_parameters()]
    params = [p for _, p in m.named_parameters()]
    y = m(imgs)
    grads = torch.autograd.grad(y, params, g)
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
    worst = max(errs.items(), key=lambda kv: kv[1])
    assert worst[1] <= bound, (worst, sorted(errs.items(), key=lambda kv: -kv[1])[:8])
    return m, errs


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_bf16_against_reference_fixture(tag):
    _run(tag, 2.5e-2)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fp32_against_reference_fixture(tag):
    """set_precision('fp32'): output and every gradient (about 300 tensors over the three fixtures) at 1e-5 of the reference's
    own fp32 autograd -- tight enough to see LayerNorm eps 1e-5 vs 1e-6 or QuickGELU vs erf GELU on the frozen MLP."""
    _run(tag, 1e-5, precision="fp32")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_fp32_no_grad_forward_matches_grad_forward(precision):
    m, T, train, seed = _build("a")
    m.set_precision(precision)
    imgs = MG.randn((MG.B, 3, T, 32, 32), seed + 1).to(DEV)
    y1 = m(imgs).detach()
    with torch.no_grad():
        y2 = m(imgs)
    assert torch.equal(y1, y2)


def test_fused_mlp_erf_gelu_form_vs_fp64():
    """The fused MLP call form of this model at the k400 per-GPU M (persistent 256 x 256 route): [fc1 ; D_fc1] with erf GELU on
    BOTH column ranges (act = act2 = GELU, n_split = 4D), the per-frame factor `af` on the adapter columns, the derivative
    stored in fragment order (aux_grad / aux_frag), and its DACT partner."""
    from aim_amd import ops
    from aim_amd.backbone import _AUX_FRAG, _AUX_GRAD
    BT, N, D, r = 64, 197, 768, 192
    M, H4 = BT * N, 4 * D
    g = torch.Generator().manual_seed(11)
    xn = torch.randn((M, D), generator=g).to(torch.bfloat16)
    W = (torch.randn((H4 + r, D), generator=g) / D ** 0.5).to(torch.bfloat16)
    b = torch.randn(H4 + r, generator=g) * 0.1
    af = (torch.rand(BT, generator=g) < 0.7).float() * 0.8
    dy = torch.randn((M, D), generator=g).to(torch.bfloat16)
    W2 = (torch.randn((D, H4 + r), generator=g) / H4 ** 0.5).to(torch.bfloat16)
    frag = _AUX_FRAG
    res = []
    for _ in range(2):
        hcat = torch.empty((M, H4 + r), dtype=torch.bfloat16, device=DEV)
        aux = ops.frag_buffer(M, H4 + r, DEV) if frag else torch.empty((M, H4 + r), dtype=torch.bfloat16, device=DEV)
        ops.gemm(xn.to(DEV), W.to(DEV), ops.EPI_ACT, hcat, bias=b.to(DEV), out2=aux, act=ops.ACT_GELU, n_split=H4,
                 act2=ops.ACT_GELU, af=af.to(DEV), ntok=N, aux_grad=_AUX_GRAD, aux_frag=frag)
        dcat = torch.empty((M, H4 + r), dtype=torch.bfloat16, device=DEV)
        ops.gemm(dy.to(DEV), W2.T.contiguous().to(DEV), ops.EPI_DACT, dcat, aux=aux, act=ops.ACT_GELU, n_split=H4,
                 act2=ops.ACT_GELU, af=af.to(DEV), ntok=N, aux_grad=_AUX_GRAD, aux_frag=frag)
        res.append((hcat.cpu(), dcat.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    hcat, dcat = res[0]
    fac = torch.ones(M, H4 + r, dtype=torch.float64)
    fac[:, H4:] = af.double().repeat_interleave(N)[:, None]
    pre = (xn.double() @ W.double().T + b.double()).requires_grad_(True)
    y = torch.nn.functional.gelu(pre)
    up = dy.double() @ W2.double()
    gd, = torch.autograd.grad(y, pre, up)
    for sl in (slice(0, H4), slice(H4, H4 + r)):
        assert rel(hcat[:, sl].float(), (fac * y.detach())[:, sl]) < 1e-2
        assert rel(dcat[:, sl].float(), (fac * gd)[:, sl]) < 1e-2


def test_frozen_aim_style_gets_none_and_same_adapter_grads():
    """Freezing by AIM's policy (only adapters, temporal_embedding, ln_post train): the frozen tensors get None and the
    trainable ones the same bits as in the full-parameter run."""
    z = np.load(os.path.join(HERE, "golden", "vit_imagenet_tiny_b.npz"))
    out = []
    for frozen in (False, True):
        m, T, train, seed = _build("b")
        _inject_masks(m, torch.from_numpy(z["masks"]), MG.B, T)
        if frozen:
            for n, p in m.named_parameters():
                if not ("temporal_embedding" in n or "ln_post" in n or "Adapter" in n):
                    p.requires_grad = False
        imgs = MG.randn((MG.B, 3, T, 32, 32), seed + 1).to(DEV)
        g = MG.randn((MG.B, MG.GEOM["embed_dim"], T, 1, 1), seed + 2).to(DEV)
        m(imgs).backward(g)
        out.append({n: (None if p.grad is None else p.grad.cpu().clone()) for n, p in m.named_parameters()})
    full, part = out
    for n in full:
        if "temporal_embedding" in n or "ln_post" in n or "Adapter" in n:
            assert part[n] is not None and torch.equal(part[n], full[n]), n
        else:
            assert part[n] is None and full[n] is not None, n


def test_two_flat_adamw_steps_then_forward_matches_fresh_model():
    import aim_amd
    from aim_amd.dist import build_optimizer
    m, T, train, seed = _build("a")
    opt = build_optimizer(m, dict(type='AdamW', lr=1e-3, weight_decay=0.05))
    assert type(opt).__name__ == "FlatAdamW"
    imgs = MG.randn((MG.B, 3, T, 32, 32), seed + 1).to(DEV)
    g = MG.randn((MG.B, MG.GEOM["embed_dim"], T, 1, 1), seed + 2).to(DEV)
    y0 = m(imgs).detach().clone()
    for _ in range(2):
        opt.zero_grad()
        m(imgs).backward(g)
        opt.step()
    y1 = m(imgs).detach()
    fresh = aim_amd.ViT_ImageNet(num_frames=T, **MG.GEOM, **MG.CASES["a"][2])
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    fresh = fresh.to(DEV).eval()
    y2 = fresh(imgs).detach()
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, y2)


def test_flat_adamw_built_directly_refreshes_operands():
    """A FlatAdamW constructed by hand (no build_optimizer, nothing registered) still invalidates the bf16 operand cache."""
    import aim_amd
    m, T, train, seed = _build("a")
    opt = aim_amd.FlatAdamW([{"params": list(m.parameters())}], lr=1e-3, weight_decay=0.05)
    imgs = MG.randn((MG.B, 3, T, 32, 32), seed + 1).to(DEV)
    g = MG.randn((MG.B, MG.GEOM["embed_dim"], T, 1, 1), seed + 2).to(DEV)
    opt.zero_grad()
    m(imgs).backward(g)
    opt.step()
    y1 = m(imgs).detach()
    fresh = aim_amd.ViT_ImageNet(num_frames=T, **MG.GEOM, **MG.CASES["a"][2])
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    assert torch.equal(y1, fresh.to(DEV).eval()(imgs).detach())


# ---------------------------------------------------------------------------------------------------------------------
# the reference configs at their per-GPU shape
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(ssv2):
    bb = dict(type='ViT_ImageNet', img_size=224, patch_size=16, num_frames=8, embed_dim=768, depth=12, num_heads=12,
              drop_path_rate=0.2, adapter_scale=1 if ssv2 else 0.5, num_tadapter=2 if ssv2 else 1)
    cfg = dict(type='Recognizer3D', backbone=bb,
               cls_head=dict(type='I3DHead', in_channels=768, num_classes=174 if ssv2 else 400, spatial_type='avg',
                             dropout_ratio=0.5),
               test_cfg=dict(average_clips='prob'))
    if ssv2:
        cfg["train_cfg"] = dict(blending=dict(type='LabelSmoothing', num_classes=174, smoothing=0.1))
    return cfg


@pytest.mark.parametrize("ssv2", [False, True], ids=["k400", "ssv2"])
def test_real_shape_two_steps_finite_and_reproducible(ssv2):
    import aim_amd
    from aim_amd.dist import build_optimizer
    C = 174 if ssv2 else 400

    def train():
        torch.manual_seed(0)
        model = aim_amd.build_model(_cfg(ssv2)).to(DEV).train()
        opt = build_optimizer(model, dict(type='AdamW', lr=3e-4, betas=(0.9, 0.999), weight_decay=0.05))
        gen = torch.Generator().manual_seed(9)
        imgs = torch.randn((8, 1, 3, 8, 224, 224), generator=gen).to(DEV)
        label = torch.randint(0, C, (8, 1), generator=gen).to(DEV)
        torch.manual_seed(3); torch.cuda.manual_seed(3)
        losses = []
        for step in range(2):
            opt.zero_grad()
            loss = model(imgs, label, return_loss=True)["loss_cls"]
            loss.backward()
            if step == 0:
                for n, p in model.named_parameters():
                    assert p.grad is not None and torch.isfinite(p.grad).all(), n
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), {n: p.detach().cpu().clone() for n, p in model.named_parameters()}

    l1, p1 = train()
    l2, p2 = train()
    assert torch.isfinite(l1).all() and torch.equal(l1, l2)
    for n in p1:
        assert torch.equal(p1[n], p2[n]), n
