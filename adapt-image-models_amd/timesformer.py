"""``TimeSformer`` backbone (the AIM paper's full fine-tuning baseline: a CLIP ViT with a second, separately weighted temporal
attention per block) on the HIP kernels.

Drop-in for ``mmaction/models/backbones/timesformer.py`` of the reference: same registry name, constructor keywords and
defaults, parameter names and shapes (``ViT_CLIP``'s stem and ``attn`` / ``ln_1`` / ``mlp`` / ``ln_2`` per block, plus
``t_attn`` / ``t_norm`` and ``T_Adapter``, a plain ``nn.Linear(D, D)``), ``init_weights`` policy (nothing is frozen, nothing is
zeroed) and ``forward(x[B,3,T,H,W]) -> [B,width,T,1,1]``.  The block (``:57-71``), on frame-major rows m = (b*T + t)*N + n:

    x1 = x  + T_Adapter(f1[t] * t_attn(t_norm(x)))       attention over the T frames of every token position, class token included
    x2 = x1 + f2[n] * attn(ln_1(x1))                     attention over the N tokens of every frame
    x3 = x2 + f3[n] * c_proj(QuickGELU(c_fc(ln_2(x2))))

``f1`` is DropPath's factor per FRAME INDEX (the reference's mask sees [T, B N, D]) and sits between ``t_attn.out_proj`` and
``T_Adapter``, whose bias therefore survives a drop; ``f2`` / ``f3`` are per TOKEN INDEX (the mask sees [N, BT, D]).  Where each
factor rides: ``f1``, expanded to one entry per frame, is ``af`` of the temporal ``out_proj`` launch and,
in the backward, of ``T_Adapter``'s dgrad launch; ``f2`` is ``at`` of the spatial ``out_proj`` launch; ``f3`` is ``at`` of the
``c_fc`` (folded into the activation, as the adapters' factors are) and ``c_proj`` (on the bias alone) launches.

Every parameter trains: the backward produces the seven weight-and-bias gradients of a block on the split-M, fixed-order
``aim_wgrad_bias_bf16``, the LayerNorm gradients on ``aim_layernorm_gb_bwd``, the stem's six (class / positional / temporal
embedding, ``ln_pre``, and the token rows behind ``conv1``) on ``aim_embed_ln_bwd``, and ``conv1``'s from the patch matrix,
gathered again.  A parameter whose ``requires_grad`` is False gets ``None`` and costs no launch.  The step is bitwise
reproducible.  ``set_precision('fp32')`` runs the same forward and backward on the fp32 kernels (timesformer_fp32.py), reading a
block through the same ``_block_view``.
"""
from collections import OrderedDict
from typing import Dict, List, Optional

import torch
from torch import nn

from . import ops
from .backbone import BF16, F32, _AUX_GRAD, LayerNorm, QuickGELU, _cast, _conv_operand, _empty, _ln_post_forward
from .full_param import FullParamBackbone, GradBufs, conv_wgrad, ln_post_backward
from .registry import BACKBONES

# the seven Linear layers of a block, in the order the backward meets them last to first
_LINEARS = ("t_qkv", "t_out", "t_ad", "qkv", "out", "fc", "pr")
_NORMS = ("t_norm", "ln_1", "ln_2")


class ResidualAttentionBlock(nn.Module):
    """Parameters of one block (reference timesformer.py:27-47, in its registration order); compute lives in
    ``_block_forward`` / ``_block_backward``."""

    def __init__(self, d_model: int, n_head: int, scale: float = 1., num_frames: int = 8, drop_path: float = 0.):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)       # parameter container only
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([
            ("c_fc", nn.Linear(d_model, d_model * 4)),
            ("gelu", QuickGELU()),
            ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = LayerNorm(d_model)
        self.n_head = n_head
        self.t_attn = nn.MultiheadAttention(d_model, n_head)
        self.t_norm = LayerNorm(d_model)
        self.T_Adapter = nn.Linear(d_model, d_model)
        self.num_frames = num_frames
        self.scale = scale                                        # accepted and unused, as in the reference
        self.drop_prob = float(drop_path)


class Transformer(nn.Module):
    def __init__(self, num_frames, width, layers, heads, scale=1., drop_path=0.1):
        super().__init__()
        self.width, self.layers = width, layers
        dpr = [x.item() for x in torch.linspace(0, drop_path, layers)]      # timesformer.py:79
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, scale, num_frames, dpr[i]) for i in range(layers)])


def _block_view(blk: ResidualAttentionBlock):
    """The block's tensors as both precisions read them: ``linear`` = ``{name: (weight, bias)}`` for ``_LINEARS``, ``norm`` =
    ``{name: (weight, bias)}`` for ``_NORMS``, and the LayerNorms' ``eps``."""
    lin = dict(t_qkv=(blk.t_attn.in_proj_weight, blk.t_attn.in_proj_bias), t_out=(blk.t_attn.out_proj.weight, blk.t_attn.out_proj.bias),
               t_ad=(blk.T_Adapter.weight, blk.T_Adapter.bias), qkv=(blk.attn.in_proj_weight, blk.attn.in_proj_bias),
               out=(blk.attn.out_proj.weight, blk.attn.out_proj.bias), fc=(blk.mlp.c_fc.weight, blk.mlp.c_fc.bias),
               pr=(blk.mlp.c_proj.weight, blk.mlp.c_proj.bias))
    norms = {n: (getattr(blk, n).weight, getattr(blk, n).bias) for n in _NORMS}
    return dict(linear=lin, norm=norms, eps=float(blk.ln_1.eps))


# parameter names under ``transformer.resblocks.{i}.`` of each linear's (weight, bias) and each norm's
_NAMES = dict(t_qkv=("t_attn.in_proj_weight", "t_attn.in_proj_bias"), t_out=("t_attn.out_proj.weight", "t_attn.out_proj.bias"),
              t_ad=("T_Adapter.weight", "T_Adapter.bias"), qkv=("attn.in_proj_weight", "attn.in_proj_bias"),
              out=("attn.out_proj.weight", "attn.out_proj.bias"), fc=("mlp.c_fc.weight", "mlp.c_fc.bias"),
              pr=("mlp.c_proj.weight", "mlp.c_proj.bias"), t_norm=("t_norm.weight", "t_norm.bias"),
              ln_1=("ln_1.weight", "ln_1.bias"), ln_2=("ln_2.weight", "ln_2.bias"))


class _BlockW:
    """bf16 operands of one block: every Linear's weight as the forward GEMM reads it (``W``) and transposed for its dgrad
    (``WT``), biases and LayerNorm tensors in fp32.  Rebuilt when a weight changed (``TimeSformer._operands``)."""

    def __init__(self, view):
        f = lambda p: p.detach().float().contiguous()
        self.eps = view["eps"]
        self.W = {n: _cast(w) for n, (w, _) in view["linear"].items()}
        self.WT = {n: _cast(w, True) for n, (w, _) in view["linear"].items()}
        self.b = {n: f(b) for n, (_, b) in view["linear"].items()}
        self.g = {n: f(w) for n, (w, _) in view["norm"].items()}
        self.beta = {n: f(b) for n, (_, b) in view["norm"].items()}


# ----------------------------------------------------------------------------------------------
# one block: forward / backward on raw buffers (frame-major rows m = (b*T + t)*N + n)
# ----------------------------------------------------------------------------------------------
def _block_forward(x, w: _BlockW, B, T, N, H, f1, f2, f3, save: bool):
    """x: [B*T*N, D] f32 -> x3.  ``f1`` [B*T] | None: the temporal branch's factor per frame (the [T] vector repeated per clip);
    ``f2`` / ``f3`` [N] | None: the spatial branch's and the MLP's factor per token index.  None = 1."""
    dev = x.device
    M, D = x.shape
    BT, eps = B * T, w.eps
    stat = lambda: (_empty((M,), F32, dev), _empty((M,), F32, dev))
    # ---- x1 = x + T_Adapter(f1 * t_attn(t_norm(x)))
    xt = _empty((M, D), BF16, dev)
    mean_t, rstd_t = stat()
    ops.layernorm_fwd(x, w.g["t_norm"], w.beta["t_norm"], M, D, D, y_bf16=xt, mean=mean_t, rstd=rstd_t, eps=eps)
    qkv_t = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xt, w.W["t_qkv"], ops.EPI_BF16, qkv_t, bias=w.b["t_qkv"])
    ot = _empty((M, D), BF16, dev)
    probs = _empty((B * N, H, T, T), F32, dev)
    ops.tattn_fwd(qkv_t, ot, probs, B, T, N, H)
    ta = _empty((M, D), BF16, dev)
    ops.gemm(ot, w.W["t_out"], ops.EPI_BF16, ta, bias=w.b["t_out"], af=f1, ntok=N)
    x1 = _empty((M, D), F32, dev)
    ops.gemm(ta, w.W["t_ad"], ops.EPI_F32, x1, bias=w.b["t_ad"], resid=x)
    # ---- x2 = x1 + f2 * attn(ln_1(x1))
    xl = _empty((M, D), BF16, dev)
    mean1, rstd1 = stat()
    ops.layernorm_fwd(x1, w.g["ln_1"], w.beta["ln_1"], M, D, D, y_bf16=xl, mean=mean1, rstd=rstd1, eps=eps)
    qkv_s = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl, w.W["qkv"], ops.EPI_BF16, qkv_s, bias=w.b["qkv"])
    ao = _empty((M, D), BF16, dev)
    lse = _empty((BT, H, N), F32, dev)
    ops.attn_fwd(qkv_s, ao, lse, BT, N, H)
    x2 = _empty((M, D), F32, dev)
    ops.gemm(ao, w.W["out"], ops.EPI_F32, x2, bias=w.b["out"], resid=x1, at=f2, ntok=N)
    # ---- x3 = x2 + f3 * c_proj(QuickGELU(c_fc(ln_2(x2)))): f3 is folded into the activation, so c_proj applies it to its bias alone
    xn = _empty((M, D), BF16, dev)
    mean2, rstd2 = stat()
    ops.layernorm_fwd(x2, w.g["ln_2"], w.beta["ln_2"], M, D, D, y_bf16=xn, mean=mean2, rstd=rstd2, eps=eps)
    h = _empty((M, 4 * D), BF16, dev)
    h_pre = _empty((M, 4 * D), BF16, dev) if (save or M < 1024) else None
    ops.gemm(xn, w.W["fc"], ops.EPI_ACT, h, bias=w.b["fc"], out2=h_pre, act=ops.ACT_QGELU, at=f3, ntok=N, aux_grad=_AUX_GRAD)
    x3 = _empty((M, D), F32, dev)
    ops.gemm(h, w.W["pr"], ops.EPI_F32, x3, bias=w.b["pr"], resid=x2, at=f3, ntok=N, rs_bias_only=True)
    if not save:
        return x3, None
    return x3, dict(x=x, mean_t=mean_t, rstd_t=rstd_t, xt=xt, qkv_t=qkv_t, probs=probs, ot=ot, ta=ta, x1=x1, mean1=mean1,
                    rstd1=rstd1, xl=xl, qkv_s=qkv_s, ao=ao, lse=lse, x2=x2, mean2=mean2, rstd2=rstd2, xn=xn, h=h, h_pre=h_pre,
                    f1=f1, f2=f2, f3=f3)


def _block_backward(dyb, c, w: _BlockW, gr: Dict[str, Optional[torch.Tensor]], eye, B, T, N, H):
    """dyb = d(loss)/d(x3) [M, D] bf16 -> d(loss)/d(x) bf16.  ``gr``: this block's fp32 gradient buffers by parameter name under
    ``transformer.resblocks.{i}.`` (missing = not wanted); every kernel ACCUMULATES into them.  ``eye``: the bf16 [D, D] identity."""
    dev = dyb.device
    M, D = dyb.shape
    BT = B * T
    f1, f2, f3 = c["f1"], c["f2"], c["f3"]

    def wgrad(gm, a, lin, at=None):
        """dW += gm^T a, db += sum_m at[m % N] gm[m] in one launch.  A bias that trains beside a frozen weight still comes out of
        that launch (its weight half goes to a scratch buffer): a column-sum kernel adds in another order, and a gradient's bits
        must not depend on what else trains."""
        dw, db = gr.get(_NAMES[lin][0]), gr.get(_NAMES[lin][1])
        if dw is None and db is not None:
            dw = torch.zeros((gm.shape[1], a.shape[1]), dtype=F32, device=dev)
        if dw is not None:
            ops.wgrad(gm, a, dw, db, at=at, ntok=N if at is not None else 0)

    def ln_gb(dxl, xin, mean, rstd, norm):
        dg, db = gr.get(_NAMES[norm][0]), gr.get(_NAMES[norm][1])
        if dg is not None or db is not None:
            ops.layernorm_gb_bwd(dxl, xin, mean, rstd, M, D, dg, db)

    # ---- x3 = x2 + h' W_pr^T + f3 b_pr,  h' = f3 QuickGELU(xn W_fc^T + b_fc)
    wgrad(dyb, c["h"], "pr", at=f3)
    dpre = _empty((M, 4 * D), BF16, dev)
    ops.gemm(dyb, w.WT["pr"], ops.EPI_DACT, dpre, aux=c["h_pre"], act=ops.ACT_QGELU, at=f3, ntok=N, aux_grad=_AUX_GRAD)
    wgrad(dpre, c["xn"], "fc")
    dxn = _empty((M, D), BF16, dev)
    ops.gemm(dpre, w.WT["fc"], ops.EPI_BF16, dxn)
    del dpre
    dx2b = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxn, c["x2"], w.g["ln_2"], c["mean2"], c["rstd2"], M, D, lddy=D, ldx=D, lddx=D, dres=dyb, dx_bf16=dx2b)
    ln_gb(dxn, c["x2"], c["mean2"], c["rstd2"], "ln_2")
    del dxn
    # ---- x2 = x1 + f2 (ao W_o^T + b_o): the gradient of the bracket is f2 * d(x2).  d(x2) comes from a LayerNorm backward, not
    # from a GEMM whose epilogue could carry f2, and the weight gradient needs the product as a bf16 operand: one D x D identity
    # GEMM with f2 in its epilogue (exact products; 1 / 51 of the block's GEMM work; not launched where f2 is 1)
    g2 = dx2b
    if f2 is not None:
        g2 = _empty((M, D), BF16, dev)
        ops.gemm(dx2b, eye, ops.EPI_BF16, g2, at=f2, ntok=N)
    wgrad(g2, c["ao"], "out")
    dao = _empty((M, D), BF16, dev)
    ops.gemm(g2, w.WT["out"], ops.EPI_BF16, dao)
    del g2
    dqkv = _empty((M, 3 * D), BF16, dev)
    delta = _empty((BT, H, N), F32, dev)
    ops.attn_bwd(c["qkv_s"], c["ao"], dao, c["lse"], delta, dqkv, BT, N, H)
    del dao
    wgrad(dqkv, c["xl"], "qkv")
    dxl = _empty((M, D), BF16, dev)
    ops.gemm(dqkv, w.WT["qkv"], ops.EPI_BF16, dxl)
    dx1b = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl, c["x1"], w.g["ln_1"], c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dx2b, dx_bf16=dx1b)
    ln_gb(dxl, c["x1"], c["mean1"], c["rstd1"], "ln_1")
    del dxl, dx2b
    # ---- x1 = x + ta W_ad^T + b_ad,  ta = f1 (ot W_to^T + b_to): f1 rides the dgrad of T_Adapter
    wgrad(dx1b, c["ta"], "t_ad")
    gt = _empty((M, D), BF16, dev)
    ops.gemm(dx1b, w.WT["t_ad"], ops.EPI_BF16, gt, af=f1, ntok=N)
    wgrad(gt, c["ot"], "t_out")
    dot = _empty((M, D), BF16, dev)
    ops.gemm(gt, w.WT["t_out"], ops.EPI_BF16, dot)
    del gt
    ops.tattn_bwd(c["qkv_t"], c["probs"], dot, dqkv, B, T, N, H)      # (overwrites the spatial branch's d(qkv))
    del dot
    wgrad(dqkv, c["xt"], "t_qkv")
    dxt = _empty((M, D), BF16, dev)
    ops.gemm(dqkv, w.WT["t_qkv"], ops.EPI_BF16, dxt)
    del dqkv
    dxb = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxt, c["x"], w.g["t_norm"], c["mean_t"], c["rstd_t"], M, D, lddy=D, ldx=D, lddx=D, dres=dx1b, dx_bf16=dxb)
    ln_gb(dxt, c["x"], c["mean_t"], c["rstd_t"], "t_norm")
    return dxb


# ----------------------------------------------------------------------------------------------
# whole backbone as one autograd node
# ----------------------------------------------------------------------------------------------
_STEM = ("class_embedding", "positional_embedding", "temporal_embedding", "ln_pre.weight", "ln_pre.bias")


class _TimeSformerFn(torch.autograd.Function):
    """imgs -> [B, D, T] features.  Differentiable inputs: every parameter, in ``named_parameters()`` order."""

    @staticmethod
    def forward(ctx, model: "TimeSformer", grad_enabled: bool, imgs: torch.Tensor, *params: torch.Tensor):
        L, H = model.layers, model.heads
        B, C, T, Hh, Ww = imgs.shape
        D, p = model.width, model.patch_size
        G = Hh // p
        N = G * G + 1
        BT, M = B * T, B * T * N
        dev = imgs.device
        need = [grad_enabled and bool(ctx.needs_input_grad[3 + k]) for k in range(len(params))]
        need_grad = any(need)
        names = model._param_names()
        P = dict(zip(names, params))
        ops_ = model._operands()
        # patch embedding: the conv as a GEMM over the patch matrix (no bias), then [cls ; tok] + pos + temporal -> ln_pre
        Kp = ops_["conv"].shape[1]
        A = _empty((BT * G * G, Kp), BF16, dev)
        ops.patchify(imgs, A, B, T, Hh, Ww, p, Kp)
        tok = _empty((BT * G * G, D), BF16, dev)
        ops.gemm(A, ops_["conv"], ops.EPI_BF16, tok)
        del A
        x = _empty((M, D), F32, dev)
        mean0, rstd0 = _empty((M,), F32, dev), _empty((M,), F32, dev)
        tmp = model._temporal_rows(P, T, D, dev)
        gpre, bpre = (P[n].detach().float().contiguous() for n in ("ln_pre.weight", "ln_pre.bias"))
        ops.embed_ln(tok, ops_["cls"], ops_["pos"], tmp, gpre, bpre, x, mean0, rstd0, B, T, N, D)
        factors = model._expand_factors(model._drop_factors(T, N, model.training, dev), B)
        ctxs: List[Optional[dict]] = []
        for i in range(L):
            x, c = _block_forward(x, ops_["blocks"][i], B, T, N, H, *factors[i], need_grad)
            ctxs.append(c)
        y, gw, meanp, rstdp = _ln_post_forward(x, P["ln_post.weight"], P["ln_post.bias"], BT, N)
        if need_grad:
            ctx.model, ctx.dims, ctx.need = model, (B, T, N, H, D, L, G), need
            ctx.saved = dict(ctxs=ctxs, ops=ops_, xL=x, gw=gw, meanp=meanp, rstdp=rstdp, imgs=imgs, params=params, tok=tok,
                             tmp=tmp, gpre=gpre, mean0=mean0, rstd0=rstd0)
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
        eye = model._identity(dev)
        for i in reversed(range(L)):
            gr = G_.block(f"transformer.resblocks.{i}.")
            dxb = _block_backward(dxb, s["ctxs"][i], s["ops"]["blocks"][i], gr, eye, B, T, N, H)
            s["ctxs"][i] = None
        # the stem: ln_pre, the three embeddings, and the token rows of d(ln_pre's input) for the conv weight
        gconv = G_["conv1.weight"]
        dtok = _empty((BT * (N - 1), D), BF16, dev) if gconv is not None else None
        stem = [G_.get(n) for n in _STEM]
        if dtok is not None or any(t is not None for t in stem):
            gcls, gpos, gtmp, ggam, gbet = stem
            ops.embed_ln_bwd(dxb, s["tok"], s["ops"]["cls"], s["ops"]["pos"], s["tmp"], s["gpre"], s["mean0"], s["rstd0"], B, T, N, D,
                             dtok=dtok, dcls=gcls, dpos=gpos, dtemporal=None if gtmp is None else gtmp.view(T, D), dgamma=ggam,
                             dbeta=gbet)
        del dxb
        if gconv is not None:
            conv_wgrad(s["imgs"], dtok, gconv, model.patch_size, s["ops"]["conv"].shape[1])
        ctx.saved = None
        return G_.result(3)


def clip_state_dict(visual_sd: Dict[str, torch.Tensor], model: "TimeSformer") -> "OrderedDict[str, torch.Tensor]":
    """A CLIP visual ``state_dict`` -> ``model``'s, as the reference's ``init_weights`` maps it (timesformer.py:140-155): ``proj``
    is dropped, every block's ``attn.*`` is copied to ``t_attn.*`` and its ``ln_1.*`` to ``t_norm.*`` unless the source already
    has them.  The tensors CLIP does not have (``temporal_embedding``, ``T_Adapter``), which the reference's ``strict=False`` load
    leaves as they are, come from ``model``: the result loads with ``strict=True``."""
    sd = OrderedDict((k, v) for k, v in visual_sd.items() if k != 'proj')
    out = OrderedDict(sd)
    for key, v in sd.items():
        if 'transformer' not in key:
            continue
        for src, dst in (('attn', 't_attn'), ('ln_1', 't_norm')):
            if src in key:
                new_key = key.replace(src, dst)
                if new_key not in sd:
                    out[new_key] = v
    for k, v in model.state_dict().items():
        if k not in out and (k == 'temporal_embedding' or '.T_Adapter.' in k):
            out[k] = v
    return out


@BACKBONES.register_module()
class TimeSformer(FullParamBackbone):
    """Full fine-tuning on the CLIP-layout ViT (reference timesformer.py:86-225); constructor keywords and defaults of the
    reference."""

    def __init__(self, input_resolution: int, num_frames: int, patch_size: int, width: int, layers: int, heads: int,
                 drop_path_rate, adapter_scale=0.5, attn_type='tadapter', pretrained=None):
        super().__init__()
        if width % heads != 0 or width // heads != 64:
            raise ValueError("the HIP attention kernels are built for head_dim 64 (ViT-B/16, ViT-L/14)")
        N = (input_resolution // patch_size) ** 2 + 1
        if N > 288:
            raise ValueError(f"{N} tokens per frame: the spatial attention kernels take at most 288")
        if num_frames > 32:
            raise ValueError(f"{num_frames} frames: the temporal attention kernels take at most 32")
        self.input_resolution = input_resolution
        self.pretrained = pretrained
        self.patch_size = patch_size
        self.width, self.layers, self.heads = width, layers, heads
        self.conv1 = nn.Conv2d(in_channels=3, out_channels=width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(N, width))
        self.ln_pre = LayerNorm(width)
        self.tadapter = attn_type == 'tadapter'
        self.num_frames = num_frames
        if self.tadapter:
            self.temporal_embedding = nn.Parameter(torch.zeros(1, num_frames, width))
        self.transformer = Transformer(num_frames, width, layers, heads, scale=adapter_scale, drop_path=drop_path_rate)
        self.ln_post = LayerNorm(width)
        self._eye = None
        self.grad_ready_hook = None                 # set by dist.FlatAdamW and never called: gradients are reduced after the backward

    # ---- reference API ------------------------------------------------------------------------
    def init_weights(self, pretrained=None):
        """Reference ``init_weights`` (:117-182): trunc_normal_(.02) Linear weights, zero biases, LayerNorms 1 / 0, optional
        CLIP load.  Nothing is frozen, and nothing is zeroed: the reference's zeroing loops look for a ``D_fc2`` child, which
        the plain-Linear ``T_Adapter`` does not have."""
        if self._init_then_wants_load(pretrained):
            try:
                import clip  # noqa: F401
            except ImportError as e:
                raise RuntimeError(
                    "pretrained=%r needs the OpenAI `clip` package and its downloaded weights "
                    "(reference timesformer.py:134-138); load a CLIP visual state_dict through "
                    "timesformer.clip_state_dict() instead" % (self.pretrained,)) from e
            name = "ViT-B/16" if self.layers == 12 else "ViT-L/14"
            clip_model, _ = clip.load(name, device="cpu")
            sd = clip_model.visual.state_dict()
            del clip_model
            self.load_state_dict(clip_state_dict(sd, self), strict=True)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'absolute_pos_embed', 'temporal_embedding'}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {'relative_position_bias_table', 'temporal_position_bias_table'}

    # ---- operand staging ------------------------------------------------------------------------
    def _operands(self):
        """bf16 copies of the GEMM weights (and fp32 copies of the small tensors the kernels read), cached across forwards
        (``_cached_operands``)"""
        ps = [p for n, p in self.named_parameters() if n not in ("temporal_embedding", "ln_pre.weight", "ln_pre.bias",
                                                                  "ln_post.weight", "ln_post.bias")]
        return self._cached_operands(ps, self._build_operands)

    def _build_operands(self):
        f = lambda t: t.detach().float().contiguous()
        return dict(conv=_conv_operand(self.conv1.weight), cls=f(self.class_embedding), pos=f(self.positional_embedding),
                    blocks=[_BlockW(_block_view(blk)) for blk in self.transformer.resblocks])

    def _identity(self, dev):
        """the bf16 [D, D] identity behind the one row-scaling GEMM of a block's backward (``_block_backward``)"""
        if self._eye is None or self._eye.device != dev:
            self._eye = torch.eye(self.width, dtype=BF16, device=dev)
        return self._eye

    def _temporal_rows(self, P, T, D, dev):
        """temporal_embedding as the stem kernels read it, [T, D] f32; zeros for a model without one (``attn_type``)"""
        if "temporal_embedding" in P:
            return P["temporal_embedding"].detach().reshape(T, D).float().contiguous()
        return torch.zeros((T, D), dtype=F32, device=dev)

    def _drop_factors(self, T, N, training, dev):
        """The DropPath factors of every layer: ``L`` triples ``(f1 [T], f2 [N], f3 [N])`` of fp32 vectors holding 0 or
        1 / keep, or None for a factor that is 1 everywhere (eval, and layer 0, whose DropPath is an Identity).  ``f1`` drops a
        FRAME INDEX across all clips and tokens (timm draws ``x.shape[0]`` entries and the temporal branch's x is
        [T, B N, D], timesformer.py:61-63); ``f2`` / ``f3`` drop a TOKEN INDEX (x is [N, BT, D], :67,70).  Tests override this
        to inject drawn masks."""
        out = []
        for blk in self.transformer.resblocks:
            rate = blk.drop_prob
            if not training or rate <= 0.:
                out.append((None, None, None))
                continue
            keep = 1.0 - rate
            u = torch.rand((T + 2 * N,), dtype=F32, device=dev)
            fac = (u < keep).to(F32) * (1.0 / keep if keep > 0 else 0.0)
            out.append((fac[:T].contiguous(), fac[T:T + N].contiguous(), fac[T + N:].contiguous()))
        return out

    @staticmethod
    def _expand_factors(factors, B):
        """``_drop_factors``' triples as the kernels take them: f1 [T] repeated per clip to one entry per frame [B*T]"""
        f = lambda v: None if v is None else v.detach().float().contiguous()
        return [(None if f1 is None else f(f1).repeat(B), f(f2), f(f3)) for f1, f2, f3 in factors]

    # ---- forward --------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        x = self._check_clip(x, self.input_resolution)
        from .timesformer_fp32 import _TimeSformerFn32, forward_f32
        return self._dispatch(x, _TimeSformerFn, _TimeSformerFn32, forward_f32)
