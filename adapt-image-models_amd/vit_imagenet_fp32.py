"""Reference-precision mode of ``ViT_ImageNet`` (``set_precision('fp32')``): the model on fp32 operands and the fp32 kernels
(csrc/fp32.hip: f32 MFMA GEMMs, exact erf; the fp32 forms of ``aim_embed_nopre_fwd/bwd`` and ``aim_layernorm_gb_bwd``), forward
and the same hand-written backward, every parameter's gradient included.  It is held to the reference's own fp32 outputs and
autograd gradients at 1e-5 (tests/test_vit_imagenet_gpu.py), which is what pins the model's numerics (LayerNorm eps 1e-6, erf
GELU on the frozen MLP, per-frame DropPath, T_Adapter_in) below bf16 noise.

The block is ``fp32_path.aim_block_forward_f32`` / ``aim_block_backward_f32``, the one fp32 AIM-style block, which stock ``AIM``
runs too: it reads this model's blocks through ``vit_imagenet._frozen_view`` and takes eps, the erf GELU, ``T_Adapter_in``, the
per-frame DropPath form and the wanted gradients as data.  This file keeps what is the model's own: the stem without ``ln_pre``,
``ln_post``, the embedding backward and the autograd node.

One stream, operands built from the current parameters on every call (nothing cached), plain autograd outputs: a verification
mode, not a fast path (the f32 MFMA runs at 1/16 of the bf16 rate).
"""
import torch

from . import ops
from .backbone import _ln_post_forward
from .fp32_path import _Block32, _Drop, _e, _f, aim_block_backward_f32, aim_block_forward_f32
from .full_param import GradBufs, conv_wgrad_f32, ln_post_backward, node_forward_f32
from .vit_imagenet import _frozen_view

F32 = torch.float32


def forward_f32(model, imgs, P, wants):
    """imgs [B, 3, T, H, W] -> [B, D, T] f32 (vit_imagenet.py:238-266); ``P`` = parameters by name.  ``wants``: the names of the
    parameters whose gradient the backward will be asked for; empty = forward only, nothing is saved."""
    save = bool(wants)
    B, C, T, Hh, Ww = imgs.shape
    D, p, H, L = model.embed_dim, model.patch_size, model.num_heads, model.depth
    G = Hh // p
    N = G * G + 1
    BT, M = B * T, B * T * N
    dev = imgs.device
    K = 3 * p * p
    if imgs.dtype != F32:
        imgs = imgs.float().contiguous()
    A = _e((BT * G * G, K), dev)
    ops.patchify(imgs, A, B, T, Hh, Ww, p, K)
    tok = _e((BT * G * G, D), dev)
    cb = P.get("patch_embed.proj.bias")
    ops.gemm_f32(A, _f(P["patch_embed.proj.weight"]).reshape(D, K), ops.EPI_BF16, tok, bias=None if cb is None else _f(cb))
    del A
    x = _e((M, D), dev)
    ops.embed_nopre_fwd(tok, _f(P["cls_token"]).view(D), _f(P["pos_embed"]).view(N, D), _f(P["temporal_embedding"]).view(T, D), x,
                        B, T, N, D)
    del tok
    masks = model._drop_masks(BT, model.training, dev)
    ctxs, blocks = [], []
    for i, blk in enumerate(model.blocks):
        w = _Block32(_frozen_view(blk), act=ops.ACT_GELU)
        # a GEMM's input is kept only when its weight trains (a bias gradient is a column sum of d(out) alone)
        keep = [k for k in ("qkv", "proj") if f"blocks.{i}.attn.{k}.weight" in wants]
        out = aim_block_forward_f32(x, w, B, T, N, H, _Drop(masks[i, 0], True), _Drop(masks[i, 1], True), keep, save=save)
        x, c = out if save else (out, None)
        ctxs.append(c)
        blocks.append(w if save else None)
    y, gw, meanp, rstdp = _ln_post_forward(x, P["ln_post.weight"], P["ln_post.bias"], BT, N, eps=model.eps)
    y = y.reshape(B, T, D).permute(0, 2, 1)
    saved = dict(ctxs=ctxs, blocks=blocks, xL=x, gw=gw, meanp=meanp, rstdp=rstdp, imgs=imgs,
                 dims=(B, T, N, H, D, L, G)) if save else None
    return y, saved


class _ViTImageNetFn32(torch.autograd.Function):
    """imgs -> [B, D, T] in fp32 with the hand-written fp32 backward.  Differentiable inputs: every parameter, in
    ``named_parameters()`` order; a parameter that does not require grad gets None and no launch."""

    @staticmethod
    def forward(ctx, model, imgs, *params):
        return node_forward_f32(ctx, forward_f32, model, imgs, params)

    @staticmethod
    def backward(ctx, dout):
        model, s = ctx.model, ctx.saved
        B, T, N, H, D, L, G = s["dims"]
        BT = B * T
        dev = dout.device
        GR = GradBufs(model._param_names(), ctx.params, ctx.need, dev, False)      # (this mode never accumulates in place)
        dx = ln_post_backward(dout, s, GR["ln_post.weight"], GR["ln_post.bias"], BT, N, F32)
        for i in reversed(range(L)):
            dx = aim_block_backward_f32(dx, s["ctxs"][i], s["blocks"][i], GR.block(f"blocks.{i}."), B, T, N, H)
            s["ctxs"][i] = s["blocks"][i] = None
        gconv = GR["patch_embed.proj.weight"]
        dtok = _e((BT * (N - 1), D), dev) if gconv is not None else None
        gtmp, gcls, gpos = GR["temporal_embedding"], GR["cls_token"], GR["pos_embed"]
        ops.embed_nopre_bwd(dx, B, T, N, D, dtok=dtok, dcls=None if gcls is None else gcls.view(D),
                            dpos=None if gpos is None else gpos.view(N, D), dtemporal=None if gtmp is None else gtmp.view(T, D),
                            dbias=GR.get("patch_embed.proj.bias"))
        del dx
        if gconv is not None:
            conv_wgrad_f32(s["imgs"], dtok, gconv, model.patch_size)
        ctx.saved = None
        return GR.result(2)
