"""The gradient bookkeeping that the CLIP-family backbones share (backbone.py: ``_GradBufs``, ``_embed_backward``), pinned
directly on every class that uses it: with ``grad_in_place`` the kernels accumulate straight into existing fp32 ``.grad``
tensors and autograd gets None for them, a parameter without such a tensor still gets its gradient through autograd, frozen
parameters get nothing, and ``grad_ready_hook`` fires once per layer from the top down.

Every comparison is ``torch.equal``: the two modes run the same kernels on the same inputs and only the address the sums land
in differs (zero-filled either way), so there is no rounding to allow for.  Shapes: the tiny fixtures' (32 x 32 clips, patch 16:
5 tokens per frame; 8 frames, where ViT_CLIP_ZEROI2V shifts heads; width 128, 2 heads, 3 layers, 2 clips), eval mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, D, L, H, B = 8, 128, 3, 2, 2
CASES = {
    # tag: (constructor, adapters per block)
    "ViT_CLIP": (lambda A: A.ViT_CLIP(32, T, 16, D, L, H, 0.0), 3),
    "AIM": (lambda A: A.AIM(32, T, 16, D, L, H, 0.0), 3),
    "ViT_CLIP_ZEROI2V": (lambda A: A.ViT_CLIP_ZEROI2V(32, T, 16, D, L, H, drop_path_rate=0.0), 2),
    "ViT_CLIP_ZEROI2V-tcls": (lambda A: A.ViT_CLIP_ZEROI2V(32, T, 16, D, L, H, drop_path_rate=0.0, with_t_cls_token=True), 3),
    "AIM_FLASH_WIN-prompt": (lambda A: A.AIM_FLASH_WIN(32, T, 16, D, L, H, drop_path_rate=0.0, wind_attn=True, prompt=True,
                                                       window_size=(2, 2, 2)), 3),
}


def _build(tag):
    import aim_amd
    torch.manual_seed(11)
    m = CASES[tag][0](aim_amd)
    m.init_weights()
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():       # init_weights leaves D_fc2 and temporal_embedding at zero: make every gradient path live
        for n, p in m.named_parameters():
            if "D_fc2" in n or n == "temporal_embedding":
                p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    imgs = torch.randn((B, 3, T, 32, 32), generator=gen).to(DEV)
    g = torch.randn((B, D, T, 1, 1), generator=gen).to(DEV)
    return m.to(DEV).eval(), imgs, g


def _run(m, imgs, g, in_place, without=None):
    """one forward / backward -> (output, {name: gradient or None}, the hook's (layer, in_place) calls); ``in_place``: zero-filled
    fp32 ``.grad`` tensors beforehand (all trainable parameters but ``without``), ``grad_in_place`` and a recording hook"""
    calls = []
    for n, p in m.named_parameters():
        p.grad = torch.zeros_like(p, dtype=torch.float32) if in_place and p.requires_grad and n != without else None
    m.grad_in_place = in_place
    m.grad_ready_hook = (lambda i, ip, streams: calls.append((i, ip))) if in_place else None
    y = m(imgs)
    y.backward(g)
    torch.cuda.synchronize()
    return y.detach(), {n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()}, calls


@pytest.mark.parametrize("tag", list(CASES))
def test_in_place_buffers_and_hook_match_plain_autograd(tag):
    m, imgs, g = _build(tag)
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert len(trainable) == 3 + 4 * CASES[tag][1] * L and frozen
    ya, ga, calls_a = _run(m, imgs, g, False)
    assert calls_a == [] and all(ga[n] is not None and float(ga[n].abs().max()) > 0 for n in trainable)
    yb, gb, calls_b = _run(m, imgs, g, True)
    assert torch.equal(ya, yb)
    for n in trainable:
        assert gb[n].dtype == torch.float32 and torch.equal(ga[n].float(), gb[n]), n
    assert all(ga[n] is None and gb[n] is None for n in frozen)
    assert calls_b == [(i, True) for i in reversed(range(L))]
    # one adapter tensor without a .grad: its layer is reported as not in place, and autograd delivers that gradient
    without = "transformer.resblocks.1.S_Adapter.D_fc1.weight"
    assert without in trainable
    yc, gc, calls_c = _run(m, imgs, g, True, without=without)
    assert torch.equal(ya, yc)
    for n in trainable:
        assert torch.equal(ga[n].float(), gc[n]), n
    assert all(gc[n] is None for n in frozen)
    assert calls_c == [(i, i != 1) for i in reversed(range(L))]
