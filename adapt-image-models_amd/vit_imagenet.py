"""``ViT_ImageNet`` backbone (AIM adapters on an ImageNet-21k ViT-B/16, the paper's ImageNet baseline) on the HIP kernels.

Drop-in for ``mmaction/models/backbones/vit_imagenet.py`` of the reference: same registry name, constructor keywords, timm-style
parameter names and shapes, ``init_weights`` policy (nothing is frozen) and ``forward(x[B,3,T,H,W]) -> [B,D,T,1,1]``.  The block
(``:86-126``) is the stock-AIM block of ``aim_variant.py`` with these differences:

- no ``ln_pre``: the first block reads conv(+bias) tokens, ``cls_token``, ``+ pos_embed``, ``+ temporal_embedding``
  (``aim_embed_nopre_fwd``);
- LayerNorm eps 1e-6 (``norm_layer``), exact-erf GELU on the frozen MLP columns of the fused ``[fc1 ; D_fc1]`` GEMM;
- ``num_tadapter=2``: ``T_Adapter_in`` (with skip) between ``norm1`` and the temporal attention;
- DropPath per FRAME (the reference's x is ``[BT, N, D]``): the factors ride the epilogues' per-frame ``af`` slot, the
  adapter biases as a per-frame ``vec`` (``ldv = D``), and the D_fc2 bias gradients are per-frame-weighted column sums;
- every parameter trains: the backward also produces the weight and bias gradients of ``qkv`` / ``proj`` (each used twice),
  ``fc1`` / ``fc2``, ``norm1`` (twice) / ``norm2`` / ``ln_post`` (``aim_layernorm_gb_bwd``: ordered, no atomics), the patch conv
  (the patch matrix is gathered again in the backward) and the embeddings (``aim_embed_nopre_bwd``).  A parameter whose
  ``requires_grad`` is False gets ``None`` and costs no launch.

Every GEMM weight gradient uses the split-M, fixed-order ``aim_wgrad_bias_bf16``; the step is bitwise reproducible.

The block's bf16 operands are ``backbone._Frozen``'s, which reads the timm-named block through ``_frozen_view``; the fp32 mode
(vit_imagenet_fp32.py) reads it through the same view and runs the one fp32 AIM-style block of fp32_path.py.
"""
import functools
import logging
from typing import Dict, List, Optional

import torch
from torch import nn

from . import ops
from .backbone import (BF16, F32, _AUX_FRAG, _AUX_GRAD, _SMALL_ADAPTERS as _SMALL, _AdapterW, _Frozen, _clip_names, _conv_operand,
                       _empty, _ln_post_forward)
from .full_param import FullParamBackbone, GradBufs, conv_wgrad, ln_post_backward
from .registry import BACKBONES

_LOG = logging.getLogger("aim_amd")

CHECKPOINT = "checkpoints/jx_vit_base_p16_224-80ecf9dd.pth"     # what the reference loads for any string `pretrained` (:192)


# ----------------------------------------------------------------------------------------------
# parameter containers (timm names, so the reference's state_dicts and the jx ViT-B/16 checkpoint load)
# ----------------------------------------------------------------------------------------------
class Adapter(nn.Module):
    """Bottleneck adapter parameters (reference ``Adapter``, vit_imagenet.py:16-34; erf GELU)."""

    def __init__(self, D_features: int, mlp_ratio: float = 0.25, skip_connect: bool = True):
        super().__init__()
        self.skip_connect = skip_connect
        hidden = int(D_features * mlp_ratio)
        self.D_fc1 = nn.Linear(D_features, hidden)
        self.D_fc2 = nn.Linear(hidden, D_features)


class Mlp(nn.Module):
    def __init__(self, in_features: int, hidden_features: int):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim: int, num_heads: int, qkv_bias: bool):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    """Parameters of one block (reference vit_imagenet.py:86-126); compute lives in ``_block_forward`` / ``_block_backward``."""

    def __init__(self, dim, num_frames, num_heads, eps, scale=0.5, num_tadapter=1, qkv_bias=True, drop_path=0.1):
        super().__init__()
        self.num_frames, self.num_tadapter = num_frames, num_tadapter
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, num_heads, qkv_bias)
        self.MLP_Adapter = Adapter(dim, skip_connect=False)
        self.S_Adapter = Adapter(dim)
        self.scale = scale
        self.T_Adapter = Adapter(dim, skip_connect=False)
        if num_tadapter == 2:
            self.T_Adapter_in = Adapter(dim)
        self.drop_prob = float(drop_path)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, 4 * dim)


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim, bias):
        super().__init__()
        self.img_size, self.patch_size = (img_size, img_size), (patch_size, patch_size)
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=bias)


_ADAPTERS = ("MLP_Adapter",) + _SMALL


def _frozen_view(blk: Block):
    """the block's tensors under the names ``_Frozen`` and ``fp32_path._Block32`` read (as ``aim_flash_win._frozen_view``)"""
    return _clip_names(blk, blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2, blk.norm1, blk.norm2)


# ----------------------------------------------------------------------------------------------
# one block: forward / backward on raw buffers (frame-major rows m = (b*T + t)*N + n)
# ----------------------------------------------------------------------------------------------
def _adapter_skip_fwd(xin, ad: _AdapterW, M, r, D):
    """Adapter with skip on bf16 rows: xin + D_fc2(GELU(D_fc1(xin))) as bf16 (the operand of the next GEMM)."""
    dev = xin.device
    pre, h = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(xin, ad.W1, ops.EPI_ACT, h, bias=ad.b1, out2=pre, act=ops.ACT_GELU)
    y = _empty((M, D), F32, dev)
    ops.gemm(h, ad.W2, ops.EPI_F32, y, bias=ad.b2)
    ops.acc_bf16(y, xin)
    yb = _empty((M, D), BF16, dev)
    ops.cast_bf16(y, yb)
    return yb, pre, h


def _block_forward(x, fz: _Frozen, adp: Dict[str, _AdapterW], B, T, N, H, dp1, dms2, save: bool, keep: Dict[str, bool]):
    """x: [B*T*N, D] f32 -> x3.  ``dp1`` [B*T]: the temporal branch's per-frame DropPath factor (:121); ``dms2`` [B*T]: the
    MLP_Adapter's, times ``scale`` (:125).  ``keep``: which frozen-size weights need gradients (their operands are saved)."""
    dev = x.device
    M, D = x.shape
    BT, r, H4, eps = B * T, fz.r, fz.H4, fz.eps
    tad, sad, tin_ad = adp["T_Adapter"], adp["S_Adapter"], adp.get("T_Adapter_in")
    # ---- temporal adaptation: norm1 -> [T_Adapter_in] -> qkv -> attention over frames -> proj -> T_Adapter -> + drop_path
    xl = _empty((M, D), BF16, dev)
    mean1, rstd1 = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x, fz.g1, fz.b1, M, D, D, y_bf16=xl, mean=mean1, rstd=rstd1, eps=eps)
    tin = tin_pre = tin_h = None
    if tin_ad is not None:
        tin, tin_pre, tin_h = _adapter_skip_fwd(xl, tin_ad, M, r, D)
    qin = tin if tin is not None else xl
    qkv_t = _empty((M, 3 * D), BF16, dev)
    ops.gemm(qin, fz.Wqkv, ops.EPI_BF16, qkv_t, bias=fz.bqkv)
    ot = _empty((M, D), BF16, dev)
    probs = _empty((B * N, H, T, T), F32, dev)
    ops.tattn_fwd(qkv_t, ot, probs, B, T, N, H)
    ta = _empty((M, D), BF16, dev)
    ops.gemm(ot, fz.Wo, ops.EPI_BF16, ta, bias=fz.bo)
    t_pre, t_hs = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(ta, tad.W1, ops.EPI_ACT, t_hs, bias=tad.b1, out2=t_pre, act=ops.ACT_GELU, af=dp1, ntok=N)
    x1 = _empty((M, D), F32, dev)
    ops.gemm(t_hs, tad.W2, ops.EPI_F32, x1, resid=x, vec=dp1[:, None] * tad.b2[None, :], ntok=N)
    # ---- spatial adaptation: norm1 -> qkv -> attention over tokens -> proj -> S_Adapter (with skip)
    xl2 = _empty((M, D), BF16, dev)
    mean1b, rstd1b = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x1, fz.g1, fz.b1, M, D, D, y_bf16=xl2, mean=mean1b, rstd=rstd1b, eps=eps)
    qkv_s = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl2, fz.Wqkv, ops.EPI_BF16, qkv_s, bias=fz.bqkv)
    ao = _empty((M, D), BF16, dev)
    lse = _empty((BT, H, N), F32, dev)
    ops.attn_fwd(qkv_s, ao, lse, BT, N, H)
    sa = _empty((M, D), BF16, dev)
    ops.gemm(ao, fz.Wo, ops.EPI_BF16, sa, bias=fz.bo)
    s_pre, s_h = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(sa, sad.W1, ops.EPI_ACT, s_h, bias=sad.b1, out2=s_pre, act=ops.ACT_GELU)
    x2 = _empty((M, D), F32, dev)
    ops.gemm(s_h, sad.W2, ops.EPI_F32, x2, bias=sad.b2, resid=x1)
    ops.acc_bf16(x2, sa)
    # ---- joint adaptation: x3 = x2 + fc2(GELU(fc1(xn))) + drop_path(scale * MLP_Adapter(xn)), one GEMM pair
    xn = _empty((M, D), BF16, dev)
    mean2, rstd2 = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x2, fz.g2, fz.b2, M, D, D, y_bf16=xn, mean=mean2, rstd=rstd2, eps=eps)
    frag = _AUX_FRAG and M >= 1024
    if frag:
        hcat_pre = ops.frag_buffer(M, H4 + r, dev) if save else None
    else:
        hcat_pre = _empty((M, H4 + r), BF16, dev) if (save or M < 1024) else None
    hcat = _empty((M, H4 + r), BF16, dev)
    ops.gemm(xn, fz.Wcat1, ops.EPI_ACT, hcat, bias=fz.bcat1, out2=hcat_pre, act=ops.ACT_GELU, n_split=H4, act2=ops.ACT_GELU,
             af=dms2, ntok=N, aux_grad=_AUX_GRAD, aux_frag=frag and hcat_pre is not None)
    x3 = _empty((M, D), F32, dev)
    ops.gemm(hcat, fz.Wcat2, ops.EPI_F32, x3, bias=fz.bpr, resid=x2, vec=dms2[:, None] * fz.b2row, ntok=N)
    if not save:
        return x3, None
    ctx = dict(x=x, mean1=mean1, rstd1=rstd1, xl=xl, tin=tin, tin_pre=tin_pre, tin_h=tin_h, qkv_t=qkv_t, probs=probs,
               ot=ot if keep["proj"] else None, ta=ta, t_pre=t_pre, t_hs=t_hs, x1=x1, mean1b=mean1b, rstd1b=rstd1b,
               xl2=xl2 if keep["qkv"] else None, qkv_s=qkv_s, ao=ao, lse=lse, sa=sa, s_pre=s_pre, s_h=s_h, x2=x2,
               mean2=mean2, rstd2=rstd2, xn=xn, hcat_pre=hcat_pre, hcat=hcat, dp1=dp1, dms2=dms2, frag=frag)
    if not keep["qkv"] and tin is None:
        ctx["xl"] = None
    return x3, ctx


def _block_backward(dyb, c, fz: _Frozen, adp: Dict[str, _AdapterW], gr: Dict[str, Optional[torch.Tensor]], B, T, N, H):
    """dyb = d(loss)/d(x3) [M, D] bf16 -> d(loss)/d(x) bf16.  ``gr``: this block's fp32 gradient buffers by parameter name
    under ``blocks.{i}.`` (missing = not wanted); every kernel ACCUMULATES into them."""
    dev = dyb.device
    M, D = dyb.shape
    BT, r, H4 = B * T, fz.r, fz.H4
    tad, sad, tin_ad = adp["T_Adapter"], adp["S_Adapter"], adp.get("T_Adapter_in")
    g = lambda n: gr.get(n)

    def wgrad(gm, a, wname, bname):
        dw, db = g(wname), g(bname)
        if dw is not None:
            ops.wgrad(gm, a, dw, db)
        elif db is not None:
            ops.colsum(gm, db)

    def adapter_d_fc2(gm, h, name, af):
        """D_fc2 of an adapter whose output rows carry the per-frame factor ``af`` (folded into h by the forward)."""
        dw, db = g(name + ".D_fc2.weight"), g(name + ".D_fc2.bias")
        if dw is not None:
            ops.wgrad(gm, h, dw)
        if db is not None:
            ops.colsum(gm, db, af=af, ntok=N)

    # ---- x3 = x2 + [h | a] [fc2 | D_fc2]^T + fc2.bias + dms2[f] * D_fc2.bias,  [h | a] = [GELU | dms2[f] GELU]([fc1 ; D_fc1] xn)
    hcat, dms2 = c["hcat"], c["dms2"]
    wgrad(dyb, hcat[:, :H4], "mlp.fc2.weight", "mlp.fc2.bias")
    adapter_d_fc2(dyb, hcat[:, H4:], "MLP_Adapter", dms2)
    dcat = _empty((M, H4 + r), BF16, dev)
    ops.gemm(dyb, fz.WcatT2, ops.EPI_DACT, dcat, aux=c["hcat_pre"], act=ops.ACT_GELU, n_split=H4, act2=ops.ACT_GELU,
             af=dms2, ntok=N, aux_grad=_AUX_GRAD, aux_frag=c["frag"])
    xn = c["xn"]
    wgrad(dcat[:, :H4], xn, "mlp.fc1.weight", "mlp.fc1.bias")
    wgrad(dcat[:, H4:], xn, "MLP_Adapter.D_fc1.weight", "MLP_Adapter.D_fc1.bias")
    dxn = _empty((M, D), BF16, dev)
    ops.gemm(dcat, fz.WcatT1, ops.EPI_BF16, dxn)
    del dcat
    dx2b = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxn, c["x2"], fz.g2, c["mean2"], c["rstd2"], M, D, lddy=D, ldx=D, lddx=D, dres=dyb, dx_bf16=dx2b)
    if g("norm2.weight") is not None or g("norm2.bias") is not None:
        ops.layernorm_gb_bwd(dxn, c["x2"], c["mean2"], c["rstd2"], M, D, g("norm2.weight"), g("norm2.bias"))
    del dxn
    # ---- x2 = x1 + sa + (s_h W2^T + b2),  s_h = GELU(sa W1^T + b1),  sa = ao proj^T + proj.bias
    wgrad(dx2b, c["s_h"], "S_Adapter.D_fc2.weight", "S_Adapter.D_fc2.bias")
    dsh_pre = _empty((M, r), BF16, dev)
    ops.gemm(dx2b, sad.W2T, ops.EPI_DACT, dsh_pre, aux=c["s_pre"], act=ops.ACT_GELU)
    wgrad(dsh_pre, c["sa"], "S_Adapter.D_fc1.weight", "S_Adapter.D_fc1.bias")
    dsa = _empty((M, D), BF16, dev)
    ops.gemm(dsh_pre, sad.W1T, ops.EPI_BF16, dsa)
    ops.add_bf16(dsa, dx2b, dsa)
    wgrad(dsa, c["ao"], "attn.proj.weight", "attn.proj.bias")
    dao = _empty((M, D), BF16, dev)
    ops.gemm(dsa, fz.WoT, ops.EPI_BF16, dao)
    del dsa
    dqkv = _empty((M, 3 * D), BF16, dev)
    delta = _empty((BT, H, N), F32, dev)
    ops.attn_bwd(c["qkv_s"], c["ao"], dao, c["lse"], delta, dqkv, BT, N, H)
    del dao
    wgrad(dqkv, c["xl2"], "attn.qkv.weight", "attn.qkv.bias")
    dxl2 = _empty((M, D), BF16, dev)
    ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dxl2)
    dx1b = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl2, c["x1"], fz.g1, c["mean1b"], c["rstd1b"], M, D, lddy=D, ldx=D, lddx=D, dres=dx2b, dx_bf16=dx1b)
    if g("norm1.weight") is not None or g("norm1.bias") is not None:
        ops.layernorm_gb_bwd(dxl2, c["x1"], c["mean1b"], c["rstd1b"], M, D, g("norm1.weight"), g("norm1.bias"))
    del dxl2, dx2b
    # ---- x1 = x + t_hs W2^T + dp1[f] b2,  t_hs = dp1[f] GELU(ta W1^T + b1),  ta = attention_T(qkv(qin)) proj^T + proj.bias
    dp1 = c["dp1"]
    adapter_d_fc2(dx1b, c["t_hs"], "T_Adapter", dp1)
    dth_pre = _empty((M, r), BF16, dev)
    ops.gemm(dx1b, tad.W2T, ops.EPI_DACT, dth_pre, aux=c["t_pre"], act=ops.ACT_GELU, af=dp1, ntok=N)
    wgrad(dth_pre, c["ta"], "T_Adapter.D_fc1.weight", "T_Adapter.D_fc1.bias")
    dta = _empty((M, D), BF16, dev)
    ops.gemm(dth_pre, tad.W1T, ops.EPI_BF16, dta)
    del dth_pre
    wgrad(dta, c["ot"], "attn.proj.weight", "attn.proj.bias")
    dot = _empty((M, D), BF16, dev)
    ops.gemm(dta, fz.WoT, ops.EPI_BF16, dot)
    del dta
    ops.tattn_bwd(c["qkv_t"], c["probs"], dot, dqkv, B, T, N, H)      # (overwrites the spatial branch's d(qkv))
    del dot
    xl, tin = c["xl"], c["tin"]
    wgrad(dqkv, tin if tin is not None else xl, "attn.qkv.weight", "attn.qkv.bias")
    dqin = _empty((M, D), BF16, dev)
    ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dqin)
    del dqkv
    if tin_ad is not None:       # qin = xl + D_fc2(GELU(D_fc1(xl)))
        wgrad(dqin, c["tin_h"], "T_Adapter_in.D_fc2.weight", "T_Adapter_in.D_fc2.bias")
        dpre = _empty((M, r), BF16, dev)
        ops.gemm(dqin, tin_ad.W2T, ops.EPI_DACT, dpre, aux=c["tin_pre"], act=ops.ACT_GELU)
        wgrad(dpre, xl, "T_Adapter_in.D_fc1.weight", "T_Adapter_in.D_fc1.bias")
        dxl = _empty((M, D), BF16, dev)
        ops.gemm(dpre, tin_ad.W1T, ops.EPI_BF16, dxl)
        ops.add_bf16(dxl, dqin, dxl)
        del dpre, dqin
    else:
        dxl = dqin
    dxb = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl, c["x"], fz.g1, c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dx1b, dx_bf16=dxb)
    if g("norm1.weight") is not None or g("norm1.bias") is not None:
        ops.layernorm_gb_bwd(dxl, c["x"], c["mean1"], c["rstd1"], M, D, g("norm1.weight"), g("norm1.bias"))
    return dxb


# ----------------------------------------------------------------------------------------------
# whole backbone as one autograd node
# ----------------------------------------------------------------------------------------------
class _ViTImageNetFn(torch.autograd.Function):
    """imgs -> [B, D, T] features.  Differentiable inputs: every parameter, in ``named_parameters()`` order."""

    @staticmethod
    def forward(ctx, model: "ViT_ImageNet", grad_enabled: bool, imgs: torch.Tensor, *params: torch.Tensor):
        L, H = model.depth, model.num_heads
        B, C, T, Hh, Ww = imgs.shape
        D, p = model.embed_dim, model.patch_size
        G = Hh // p
        N = G * G + 1
        BT, M = B * T, B * T * N
        dev = imgs.device
        need = [grad_enabled and bool(ctx.needs_input_grad[3 + k]) for k in range(len(params))]
        need_grad = any(need)
        names = model._param_names()
        P = dict(zip(names, params))
        ops_ = model._frozen_operands()
        adp = model._stage_adapters(ops_, P)
        # patch embedding: the conv as a GEMM over the patch matrix, bias in the fp32 epilogue
        Kp = ops_["conv"].shape[1]
        A = _empty((BT * G * G, Kp), BF16, dev)
        ops.patchify(imgs, A, B, T, Hh, Ww, p, Kp)
        tok = _empty((BT * G * G, D), F32, dev)
        ops.gemm(A, ops_["conv"], ops.EPI_F32, tok, bias=ops_["conv_b"])
        del A
        x = _empty((M, D), F32, dev)
        tmp = P["temporal_embedding"].detach().reshape(T, D).float().contiguous()
        ops.embed_nopre_fwd(tok, ops_["cls"], ops_["pos"], tmp, x, B, T, N, D)
        del tok
        masks = model._drop_masks(BT, model.training, dev)          # [L, 2, B*T]
        ctxs: List[Optional[dict]] = []
        wants = dict(zip(names, need))
        for i in range(L):
            pre = f"blocks.{i}."
            # the forward keeps a GEMM's input only when its weight trains (a bias gradient is a column sum of d(out) alone)
            keep = dict(qkv=wants[pre + "attn.qkv.weight"], proj=wants[pre + "attn.proj.weight"])
            x, c = _block_forward(x, ops_["blocks"][i], adp[i], B, T, N, H, masks[i, 0], masks[i, 1], need_grad, keep)
            ctxs.append(c)
        y, gw, meanp, rstdp = _ln_post_forward(x, P["ln_post.weight"], P["ln_post.bias"], BT, N, eps=model.eps)
        if need_grad:
            ctx.model, ctx.dims, ctx.need = model, (B, T, N, H, D, L, G), need
            ctx.saved = dict(ctxs=ctxs, adp=adp, ops=ops_, xL=x, gw=gw, meanp=meanp, rstdp=rstdp, imgs=imgs, params=params)
        return y.reshape(B, T, D).permute(0, 2, 1)

    @staticmethod
    def backward(ctx, dout):
        model = ctx.model
        B, T, N, H, D, L, G = ctx.dims
        s, need = ctx.saved, ctx.need
        BT = B * T
        dev = dout.device
        # every kernel ACCUMULATES into these; with `grad_in_place` they are the `param.grad` views of the flat gradient buffer
        G_ = GradBufs(model._param_names(), s["params"], need, dev, model.grad_in_place)
        dxb = ln_post_backward(dout, s, G_["ln_post.weight"], G_["ln_post.bias"], BT, N, BF16)
        s["xL"] = None
        for i in reversed(range(L)):
            dxb = _block_backward(dxb, s["ctxs"][i], s["ops"]["blocks"][i], s["adp"][i], G_.block(f"blocks.{i}."), B, T, N, H)
            s["ctxs"][i] = None
        # embedding: cls_token / pos_embed / temporal_embedding / conv bias, and the token rows of d(x) for the conv weight
        gconv = G_["patch_embed.proj.weight"]
        dtok = _empty((BT * (N - 1), D), BF16, dev) if gconv is not None else None
        gtmp = G_["temporal_embedding"]
        ops.embed_nopre_bwd(dxb, B, T, N, D, dtok=dtok,
                            dcls=None if G_["cls_token"] is None else G_["cls_token"].view(D),
                            dpos=None if G_["pos_embed"] is None else G_["pos_embed"].view(N, D),
                            dtemporal=None if gtmp is None else gtmp.view(T, D),
                            dbias=G_.get("patch_embed.proj.bias"))
        del dxb
        if gconv is not None:
            conv_wgrad(s["imgs"], dtok, gconv, model.patch_size, s["ops"]["conv"].shape[1])
        ctx.saved = None
        return G_.result(3)


def _layernorm_eps(norm_layer) -> float:
    """eps of a LayerNorm ``norm_layer`` (class or functools.partial); anything else is not built."""
    if norm_layer is nn.LayerNorm:
        return 1e-5
    if isinstance(norm_layer, functools.partial) and norm_layer.func is nn.LayerNorm and not norm_layer.args \
            and set(norm_layer.keywords) <= {"eps"}:
        return float(norm_layer.keywords.get("eps", 1e-5))
    raise NotImplementedError(f"ViT_ImageNet(norm_layer={norm_layer!r}): only nn.LayerNorm (any eps) is built")


@BACKBONES.register_module()
class ViT_ImageNet(FullParamBackbone):
    """AIM on an ImageNet-21k ViT (reference vit_imagenet.py:129-266); constructor keywords and defaults of the reference."""

    def __init__(self, img_size=224, num_frames=8, patch_size=16, in_chans=3, embed_dim=768, depth=12, adapter_scale=0.5,
                 num_tadapter=1, num_heads=12, mlp_ratio=4., patch_embedding_bias=True, qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=functools.partial(nn.LayerNorm, eps=1e-6),
                 pretrained=None):
        super().__init__()
        if qk_scale is not None:
            raise NotImplementedError("ViT_ImageNet(qk_scale=...) is not built: the attention kernels scale by head_dim ** -0.5")
        if drop_rate != 0 or attn_drop_rate != 0:
            raise NotImplementedError("ViT_ImageNet(drop_rate / attn_drop_rate > 0): dropout is not built")
        if in_chans != 3:
            raise NotImplementedError(f"ViT_ImageNet(in_chans={in_chans}): only 3-channel clips are built")
        if mlp_ratio != 4:
            raise NotImplementedError(f"ViT_ImageNet(mlp_ratio={mlp_ratio}): only mlp_ratio=4 is built")
        eps = _layernorm_eps(norm_layer)
        if embed_dim % num_heads != 0 or embed_dim // num_heads != 64:
            raise ValueError("the HIP attention kernels are built for head_dim 64 (ViT-B/16, ViT-L/14)")
        self.num_tadapter = num_tadapter
        self.pretrained = pretrained
        self.depth = depth
        self.num_frames = num_frames
        self.num_features = self.embed_dim = embed_dim
        self.num_heads, self.patch_size, self.img_size = num_heads, patch_size, img_size
        self.qkv_bias, self.eps = bool(qkv_bias), eps
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim, patch_embedding_bias)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.pos_drop = nn.Dropout(p=drop_rate)          # built, never used (as in the reference)
        self.temporal_embedding = nn.Parameter(torch.zeros(1, num_frames, embed_dim))
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([Block(embed_dim, num_frames, num_heads, eps, scale=adapter_scale, num_tadapter=num_tadapter,
                                           qkv_bias=qkv_bias, drop_path=dpr[i]) for i in range(depth)])
        self.ln_post = nn.LayerNorm(embed_dim, eps=eps)
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self._cast_table = None

    # ---- reference API ------------------------------------------------------------------------
    def init_weights(self, pretrained=None):
        """Reference ``init_weights`` (:180-236): init, optional load of the local jx ViT-B/16 checkpoint, zero every adapter's
        D_fc2.  Nothing is frozen."""
        if self._init_then_wants_load(pretrained):
            _LOG.info('load model from: %s', self.pretrained)
            state_dict = torch.load(CHECKPOINT, map_location="cpu")
            state_dict['ln_post.weight'] = state_dict['norm.weight']
            state_dict['ln_post.bias'] = state_dict['norm.bias']
            msg = self.load_state_dict(state_dict, strict=False)
            _LOG.info('Missing keys: %s', msg.missing_keys)
            _LOG.info('Unexpected keys: %s', msg.unexpected_keys)
            self._last_load = msg
        for n, m in self.blocks.named_modules():
            if any(a in n for a in ("S_Adapter", "T_Adapter", "MLP_Adapter")) and n.endswith("D_fc2"):
                nn.init.constant_(m.weight, 0)
                nn.init.constant_(m.bias, 0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'temporal_embedding'}

    # ---- operand staging ------------------------------------------------------------------------
    def _operand_params(self):
        """The parameters cached as bf16 operands across forwards (everything but the adapters, temporal_embedding, ln_post)."""
        return [p for n, p in self.named_parameters()
                if "Adapter" not in n and n not in ("temporal_embedding", "ln_post.weight", "ln_post.bias")]

    def _frozen_operands(self):
        """bf16 copies of the large weights, cached across forwards (``_cached_operands``)"""
        return self._cached_operands(self._operand_params(), self._build_operands)

    def _build_operands(self):
        D = self.embed_dim
        w, b = self.patch_embed.proj.weight, self.patch_embed.proj.bias
        f = lambda t: t.detach().float().contiguous()
        self._cast_table = None          # (its entries point into the operands being replaced)
        return dict(conv=_conv_operand(w), conv_b=f(b) if b is not None else torch.zeros(D, dtype=F32, device=w.device),
                    cls=f(self.cls_token).view(D), pos=f(self.pos_embed).view(-1, D),
                    blocks=[_Frozen(_frozen_view(blk)) for blk in self.blocks])

    def _stage_adapters(self, ops_, P):
        """Every adapter's weights -> its bf16 operand buffers (one ``aim_cast_multi`` launch); returns per-block _AdapterW."""
        srcs, entries = [], []
        for i, fz in enumerate(ops_["blocks"]):
            for a in _ADAPTERS:
                pre = f"blocks.{i}.{a}."
                if pre + "D_fc1.weight" not in P:
                    continue
                w1, b1, w2 = P[pre + "D_fc1.weight"].detach(), P[pre + "D_fc1.bias"].detach(), P[pre + "D_fc2.weight"].detach()
                srcs += [w1, w2, b1] if a == "MLP_Adapter" else [w1, w2]
                entries += fz.cast_entries(a, w1, w2, b1 if a == "MLP_Adapter" else None)
        ok = all(t.dtype == F32 and t.is_contiguous() for t in srcs)
        if ok:
            key = tuple(t.data_ptr() for t in srcs) + (id(ops_),)
            if self._cast_table is None or self._cast_table[0] != key:
                self._cast_table = (key, ops.CastTable(entries, srcs[0].device))
            self._cast_table[1].run()
        else:
            for src, dst, tr in entries:
                if tr == 2:
                    dst.copy_(src.float())
                else:
                    ops.cast_bf16(src.float().contiguous(), dst, transpose=tr)
        adp = []
        for i, fz in enumerate(ops_["blocks"]):
            pre = f"blocks.{i}."
            fz.stage_mlp_bias(P[pre + "MLP_Adapter.D_fc1.bias"], P[pre + "MLP_Adapter.D_fc2.bias"], copy_b1=not ok)
            d = {}
            for a in _SMALL:
                if pre + a + ".D_fc1.weight" in P:
                    d[a] = _AdapterW(P[pre + a + ".D_fc1.weight"], P[pre + a + ".D_fc1.bias"], P[pre + a + ".D_fc2.weight"],
                                     P[pre + a + ".D_fc2.bias"], bufs=fz.small[a])
            adp.append(d)
        return adp

    def _drop_masks(self, BT, training, dev):
        """Both DropPath factors of every block, ``[L, 2, B*T]``, per FRAME (timm draws ``[x.shape[0]]`` and x is [BT, N, D]):
        [:, 0] the temporal branch's (no adapter scale, :121), [:, 1] the MLP_Adapter's times ``scale`` (:125)."""
        L = len(self.blocks)
        rates = torch.tensor([b.drop_prob for b in self.blocks], dtype=F32)
        scale = torch.tensor([float(b.scale) for b in self.blocks], dtype=F32)
        out = torch.empty((L, 2, BT), dtype=F32)
        out[:, 0] = 1.0
        out[:, 1] = scale[:, None]
        out = out.to(dev)
        if training and float(rates.max()) > 0:
            keep = (1.0 - rates).to(dev).view(L, 1, 1)
            u = torch.rand((L, 2, BT), dtype=F32, device=dev)
            fac = torch.where(keep > 0, 1.0 / keep.clamp_min(1e-12), torch.zeros_like(keep))
            out = out * (u < keep).to(F32) * fac
        return out

    # ---- forward --------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        x = self._check_clip(x, self.img_size)
        from .vit_imagenet_fp32 import _ViTImageNetFn32, forward_f32
        return self._dispatch(x, _ViTImageNetFn, _ViTImageNetFn32, forward_f32)
