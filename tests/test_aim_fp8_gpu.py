"""fp8 inference of stock AIM (``AIM(wind_attn=False)``) on a real MI355X: the inference forms of the temporal attention
kernel (``aim_tattn_fwd_infer``), the block against the rounding-point emulation of tests/aim_fp8_emu.py, the fp8 operand
cache, the one remaining warning, and multi-view inference through ``Recognizer3D``.  Every measured number is appended to
the suite's parity record (``test_fp8_gpu._record``).

Measured on MI355X, fp8_vs_emu8 / emu8_vs_emu16 (bound: ratio < 0.75) / fp8_vs_bf16 / bf16_vs_emu16:
  B16_L2  3.05e-2 / 5.59e-2 (ratio 0.55) / 5.55e-2 / 3.2e-3
  L14_L2  2.95e-2 / 5.20e-2 (ratio 0.57) / 5.42e-2 / 2.9e-3
fp8 form of the kernel against float64: all 37 056 bytes of the four shapes equal, under either LDS staging (every T from
1 to 32 under both stagings: test_attn_lengths_gpu.py).
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import vit_clip_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aim_fp8_emu as E  # noqa: E402
from attn_cases import e4m3_code as _code, tattn_ref64 as _ref64  # noqa: E402  (shared with the sweep over every T)
from test_fp8_gpu import _record  # noqa: E402  (the parity record that the ViT_CLIP fp8 tests append to)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 1), (2, 5, 3, 3), (1, 32, 5, 2), (3, 8, 7, 1)]      # (B, T, N, H); (2, 5, 3, 3): a partial last workgroup
GUARD = 64                                                              # canary rows behind every output


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _qkv(B, T, N, H, v_scale=1.0):
    D = H * 64
    g = torch.Generator().manual_seed(1000 * B + 100 * T + 10 * N + H)
    qkv = torch.randn((B * T * N, 3 * D), generator=g) * 0.8
    qkv[:, 2 * D:] *= v_scale
    return qkv.to(torch.bfloat16)


def _guarded(M, D, dtype):
    """an [M, D] output filled with canary bytes, GUARD more rows of them behind it"""
    buf = torch.full(((M + GUARD) * D * dtype.itemsize,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[:M * D * dtype.itemsize].view(dtype).view(M, D)


def _guard_intact(buf, M, D, dtype):
    return bool((buf[M * D * dtype.itemsize:] == 0xA5).all())


@pytest.mark.parametrize("B,T,N,H", SHAPES)
def test_tattn_infer_bf16_form_has_the_training_kernels_bits(B, T, N, H):
    from aim_amd import ops
    D, M = H * 64, B * T * N
    qkv = _qkv(B, T, N, H).to(DEV)
    want = torch.empty((M, D), dtype=torch.bfloat16, device=DEV)
    probs = torch.empty((B * N, H, T, T), dtype=torch.float32, device=DEV)
    ops.tattn_fwd(qkv, want, probs, B, T, N, H)
    buf, out = _guarded(M, D, torch.bfloat16)
    ops.tattn_fwd_infer(qkv, out, B, T, N, H)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert _guard_intact(buf, M, D, torch.bfloat16)


@pytest.mark.parametrize("B,T,N,H", SHAPES)
def test_tattn_infer_fp8_form(B, T, N, H):
    """every byte is the e4m3 cast of the float64 result or its neighbour on the grid; at most 1e-3 of them are neighbours:
    an fp32 sum over T <= 32 terms errs by ~2e-6 relative and e4m3's rounding boundaries lie 2^-4 .. 2^-3 apart, so ~6e-5
    of the values may flip; the cap is 15 times that"""
    from aim_amd import ops
    D, M = H * 64, B * T * N
    qkv = _qkv(B, T, N, H)
    buf, out = _guarded(M, D, torch.uint8)
    ops.tattn_fwd_infer(qkv.to(DEV), out, B, T, N, H)
    torch.cuda.synchronize()
    want = O.q8(_ref64(qkv, B, T, N, H).float()).to(torch.float8_e4m3fn).view(torch.uint8)
    got = out.cpu()
    step = (_code(got) - _code(want)).abs()
    print("TATTN8", (B, T, N, H), "bytes", got.numel(), "neighbours", int((step == 1).sum()), "farther", int((step > 1).sum()))
    assert int(step.max()) <= 1
    assert (got != want).float().mean().item() <= 1e-3
    assert _guard_intact(buf, M, D, torch.uint8)
    # the float8 view of the same buffer is accepted as well
    out8 = torch.empty((M, D), dtype=torch.float8_e4m3fn, device=DEV)
    ops.tattn_fwd_infer(qkv.to(DEV), out8, B, T, N, H)
    assert torch.equal(out8.view(torch.uint8), out)


def test_tattn_infer_fp8_saturates():
    """|out| > 448 is stored as +-448 (0x7E / 0xFE), never as the NaN codes 0x7F / 0xFF"""
    from aim_amd import ops
    B, T, N, H = 2, 5, 3, 3
    D, M = H * 64, B * T * N
    qkv = _qkv(B, T, N, H).float()
    sign = torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0)
    qkv[:, 2 * D:] = 600.0 * sign               # every frame's v: the attention's average is +-600 whatever the weights
    qkv = qkv.to(torch.bfloat16)
    buf, out = _guarded(M, D, torch.uint8)
    ops.tattn_fwd_infer(qkv.to(DEV), out, B, T, N, H)
    torch.cuda.synchronize()
    got = out.cpu()
    want = torch.where(sign < 0, 0xFE, 0x7E).to(torch.uint8).expand(M, D)
    assert torch.equal(got, want)
    assert _guard_intact(buf, M, D, torch.uint8)


def test_tattn_infer_refuses_no_or_two_outputs():
    import aim_amd
    from aim_amd import ops
    B, T, N, H = 2, 5, 3, 3
    D, M = H * 64, B * T * N
    lib = aim_amd.load_library()
    qkv = _qkv(B, T, N, H).to(DEV)
    b16, o16 = _guarded(M, D, torch.bfloat16)
    b8, o8 = _guarded(M, D, torch.uint8)
    assert lib.aim_tattn_fwd_infer(qkv.data_ptr(), None, None, B, T, N, H, ops._stream()) != 0
    assert b"exactly one" in lib.aim_last_error()
    assert lib.aim_tattn_fwd_infer(qkv.data_ptr(), o16.data_ptr(), o8.data_ptr(), B, T, N, H, ops._stream()) != 0
    assert b"exactly one" in lib.aim_last_error()
    with pytest.raises(RuntimeError):
        ops.tattn_fwd_infer(qkv, o16, B, 33, N, H)               # the shape checks of aim_tattn_fwd
    with pytest.raises(TypeError):
        ops.tattn_fwd_infer(qkv, torch.empty((M, D), device=DEV), B, T, N, H)
    torch.cuda.synchronize()
    assert bool((b16 == 0xA5).all()) and bool((b8 == 0xA5).all())      # nothing was written


def _model(arch, st=None):
    import aim_amd
    res, T, patch, D, H, B = E.CASES[arch]
    m = aim_amd.AIM(res, T, patch, D, E.LAYERS, H, 0.0)
    m.init_weights()
    if st is not None:
        m.load_state_dict(st, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("arch", list(E.CASES))
def test_aim_fp8_forward_matches_rounding_point_emulation(arch):
    st, imgs = E.case_inputs(arch)
    H = E.CASES[arch][4]
    m = _model(arch, st)
    with torch.no_grad():
        y16 = m(imgs.to(DEV))
        m.set_inference_precision('fp8')
        y8 = m(imgs.to(DEV))
        e8 = E.emu_aim_backbone_f8(imgs, st, H)
        e16 = E.emu_aim_backbone_f8(imgs, st, H, f8=False)
    vals = dict(fp8_vs_emu8=_rel(y8, e8), fp8_vs_bf16=_rel(y8, y16), emu8_vs_emu16=_rel(e8, e16), bf16_vs_emu16=_rel(y16, e16))
    _record("aim_fp8_forward_" + arch, **vals)
    assert not torch.equal(y8, y16)                      # the fp8 kernels really ran
    # the bound and the argument of test_fp8_gpu.py::test_fp8_forward_matches_rounding_point_oracle: two implementations of one
    # chain of rounded stages drift apart by a fraction of the rounding's own effect; it guards the wiring (the mutants of
    # tests/test_aim_fp8_cpu.py all lie outside it), the kernels' arithmetic is pinned at kernel level
    assert vals["fp8_vs_emu8"] < 0.75 * vals["emu8_vs_emu16"], vals
    # a grad-enabled forward never takes the fp8 path, and the no-grad bf16 forward (no stored probabilities) has its bits
    y_tr = m(imgs.to(DEV))
    assert y_tr.requires_grad and torch.equal(y_tr.detach(), y16)


def test_fp8_operands_follow_weight_changes():
    """an in-place change of a quantised weight, and an optimizer step through raw pointers (``FlatAdamW`` via
    ``attach_backbone``: no tensor version moves), both reach the next fp8 forward: it equals a freshly built model's"""
    import aim_amd
    from aim_amd.dist import build_optimizer
    arch = "B16_L2"
    res, T, patch, D, H, B = E.CASES[arch]
    st, imgs = E.case_inputs(arch)
    imgs = imgs.to(DEV)

    def fresh8(state):
        f = _model(arch, {k: v.detach().clone() for k, v in state.items()}).set_inference_precision('fp8')
        with torch.no_grad():
            return f(imgs)

    m = _model(arch, st).set_inference_precision('fp8')
    with torch.no_grad():
        y_a = m(imgs)
        w = m.transformer.resblocks[0].MLP_Adapter.D_fc2.weight
        w.add_(0.05 * torch.randn(w.shape, generator=torch.Generator().manual_seed(7)).to(DEV))
        y_b = m(imgs)
    assert not torch.equal(y_a, y_b)
    assert torch.equal(y_b, fresh8(m.state_dict()))
    # FlatAdamW
    cfg = dict(type='Recognizer3D',
               backbone=dict(type='AIM', input_resolution=res, patch_size=patch, num_frames=T, width=D, layers=E.LAYERS, heads=H,
                             drop_path_rate=0.0, adapter_scale=0.5, pretrained=None),
               cls_head=dict(type='I3DHead', in_channels=D, num_classes=9, dropout_ratio=0.0),
               test_cfg=dict(average_clips='prob'))
    torch.manual_seed(3)
    model = aim_amd.build_model(cfg).to(DEV)
    opt = build_optimizer(model, dict(type='AdamW', lr=5e-2, weight_decay=0.0))
    bb = model.backbone.set_inference_precision('fp8')
    assert bb.grad_ready_hook is not None               # attach_backbone ran
    label = torch.randint(0, 9, (B, 1), generator=torch.Generator().manual_seed(4)).to(DEV)

    def eval8():
        model.eval()
        with torch.no_grad():
            y = bb(imgs)
        model.train()
        return y

    y0 = eval8()
    epoch = bb.weights_epoch
    for _ in range(2):                                  # (D_fc2 starts at zero: the second step moves D_fc1 as well)
        opt.zero_grad()
        model(imgs.unsqueeze(1), label, return_loss=True)["loss_cls"].backward()
        opt.step()
    assert bb.weights_epoch > epoch
    y1 = eval8()
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, fresh8(bb.state_dict()))


def test_fp8_warning_only_under_1024_rows(caplog):
    import aim_amd
    m = aim_amd.AIM(32, 2, 16, 128, 2, 2, 0.0)
    m.init_weights()
    m = m.to(DEV).eval()
    imgs = torch.randn((1, 3, 2, 32, 32), generator=torch.Generator().manual_seed(1)).to(DEV)       # M = 10 rows
    with torch.no_grad():
        y = m(imgs)
        m.set_inference_precision('fp8')
        with caplog.at_level("WARNING", logger="aim_amd"):
            y8 = m(imgs)
    assert torch.equal(y, y8)
    assert any("fp8" in r.getMessage() and "bf16" in r.getMessage() and "1024" in r.getMessage() for r in caplog.records)
    caplog.clear()
    big = _model("B16_L2").set_inference_precision('fp8')
    with torch.no_grad(), caplog.at_level("WARNING", logger="aim_amd"):
        big(E.case_inputs("B16_L2")[1].to(DEV))
    assert not [r for r in caplog.records if "fp8" in r.getMessage()]


def test_aim_fp8_multiview_inference_agrees_with_bf16():
    """``Recognizer3D._do_test`` on stock AIM at ViT-L width: 3 views per sample in chunks of ``max_testing_views=2`` (4 112 and
    2 056 token rows), clip averaging.  The pairwise-ranking criterion of
    test_fp8_gpu.py::test_fp8_multiview_inference_agrees_with_bf16, with its definition of ``tol``."""
    import aim_amd
    T, L, C, S = 8, 2, 400, 8
    cfg = dict(type='Recognizer3D',
               backbone=dict(type='AIM', input_resolution=224, patch_size=14, num_frames=T, width=1024, layers=L,
                             heads=16, drop_path_rate=0.0, adapter_scale=0.5, pretrained=None),
               cls_head=dict(type='I3DHead', in_channels=1024, num_classes=C, spatial_type='avg', dropout_ratio=0.5, init_std=0.05),
               test_cfg=dict(average_clips='score', max_testing_views=2))
    torch.manual_seed(5)
    model = aim_amd.build_model(cfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "D_fc2" in n:
                p.normal_(0, 0.02)
    model = model.to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    samples = [torch.randn((1, 3, 3, T, 224, 224), generator=gen) for _ in range(S)]       # [1, V=3, 3, T, H, W]
    with torch.no_grad():
        s16 = np.concatenate([model(s.to(DEV), return_loss=False) for s in samples])
        model.backbone.set_inference_precision('fp8')
        s8 = np.concatenate([model(s.to(DEV), return_loss=False) for s in samples])
        model.test_cfg['average_clips'] = 'prob'
        p8 = model(samples[0].to(DEV), return_loss=False)
    assert s16.shape == (S, C) and p8.shape == (1, C) and abs(p8.sum() - 1) < 1e-4
    assert not np.array_equal(s8, s16)
    noise = float(np.sqrt(np.mean((s8 - s16) ** 2)))
    tol = 5.0 * np.sqrt(2.0) * noise
    d16 = s16[:, :, None] - s16[:, None, :]
    d8 = s8[:, :, None] - s8[:, None, :]
    sep = d16 > tol
    top2 = np.sort(s16, axis=1)[:, -2:]
    margin_ok = (top2[:, 1] - top2[:, 0]) > tol
    _record("aim_fp8_multiview_ranking", logit_rms_noise=noise, logit_std=float(s16.std()), tol=tol,
            pairs_separated=float(sep.mean() * 2), pairs_misranked=int((d8[sep] <= 0).sum()),
            top1_agree_all=float((s8.argmax(1) == s16.argmax(1)).mean()), top1_margin_ok=int(margin_ok.sum()), n_samples=S,
            rel=_rel(torch.from_numpy(s8), torch.from_numpy(s16)))
    assert sep.mean() * 2 > 0.5                     # the criterion covers most class pairs
    assert (d8[sep] > 0).all()
    assert (s8.argmax(1)[margin_ok] == s16.argmax(1)[margin_ok]).all()
