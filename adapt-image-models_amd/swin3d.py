"""``SwinTransformer3D`` backbone (Video Swin) on the HIP kernels.

Drop-in for ``mmaction/models/backbones/swin_transformer.py`` of the reference: same registry name, constructor keywords,
``state_dict`` keys, shapes and buffers (``relative_position_index``), ``init_weights`` / ``inflate_weights`` policy and
``forward(x[B,3,T,S,S]) -> [B, C_last, D', H', W']`` after the final ``norm``.  Every parameter trains; ``frozen_stages`` is
honoured through ``requires_grad`` plus ``eval()`` in ``train()``, and a parameter whose ``requires_grad`` is False gets
``None`` and costs no launch.

Rows are frame-major, m = ((b D' + d) G + y) G + x, fp32 residual stream.  One block (:254-275):

- x += dp1 * proj(attention(qkv(norm1(x)))): ``aim_swin3d_attn_*`` reads the rolled, partitioned and masked 3-D windows by
  address as the boxes of the cut partition and the relative-position bias straight from its table,
  so nothing is rolled, copied into window order or gathered into a dense bias; the table's gradient comes back folded.
  Even blocks have shift (0, 0, 0), odd ones ``window // 2``, both after ``get_window_size``'s clipping to the token grid;
- x += dp2 * mlp(norm2(x)).

``dp1`` / ``dp2`` are the DropPath factors, one per clip (the reference's ``x.shape[0]`` is B): they ride the GEMM epilogues as
``af`` with ``ntok`` = the rows of a clip.  The stem, 2 x 2 patch merging, LayerNorm and gradient helpers are those of
``swin2d_adapter.py``.  Every GEMM weight gradient uses the split-M, fixed-order ``aim_wgrad_bias_bf16`` and the table
gradient is a fixed-order sum: the step is bitwise reproducible.
"""
import logging
from types import SimpleNamespace
from typing import Dict, List

import torch
from torch import nn

from . import ops
from .backbone import BF16, F32, _cast, _empty
from .full_param import FullParamBackbone, GradBufs
from .registry import BACKBONES
from .swin2d_adapter import HEAD_DIM, Mlp, _f32, _linear_ops, _ln, _merge_backward, _merge_forward

_LOG = logging.getLogger("aim_amd")

MAX_WINDOW_TOKENS = 1024      # the 3-D Swin attention kernels' capacity (include/aim_kernels.h)
MAX_TABLE_ENTRIES = 5248


def get_window_size(x_size, window_size, shift_size=None):
    """the reference's clipping (:71-84): an axis no longer than its window takes the axis as window and is not shifted"""
    use_w, use_s = list(window_size), list(shift_size) if shift_size is not None else None
    for i in range(len(x_size)):
        if x_size[i] <= window_size[i]:
            use_w[i] = x_size[i]
            if use_s is not None:
                use_s[i] = 0
    return tuple(use_w) if use_s is None else (tuple(use_w), tuple(use_s))


def relative_position_index(window) -> torch.Tensor:
    """[N, N] index into the (2Wt-1)(2Wh-1)(2Ww-1) table (:113-127): f(q) - f(k) + f(Wt-1, Wh-1, Ww-1) with
    f(t, h, w) = (t (2Wh-1) + h)(2Ww-1) + w"""
    wt, wh, ww = window
    fh, fw = 2 * wh - 1, 2 * ww - 1
    t, h, w = (c.reshape(-1) for c in torch.meshgrid(torch.arange(wt), torch.arange(wh), torch.arange(ww), indexing="ij"))
    f = (t * fh + h) * fw + w
    return f[:, None] - f[None, :] + ((wt - 1) * fh + wh - 1) * fw + ww - 1


# ----------------------------------------------------------------------------------------------
# parameter containers (the reference's names, so its state_dicts and the Video Swin checkpoints load)
# ----------------------------------------------------------------------------------------------
class WindowAttention3D(nn.Module):
    def __init__(self, dim, window_size, num_heads, qkv_bias):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        wt, wh, ww = window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wt - 1) * (2 * wh - 1) * (2 * ww - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(window_size))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)


class SwinTransformerBlock3D(nn.Module):
    """Parameters and geometry of one block (:172-275); compute lives in ``_block_forward`` / ``_block_backward``."""

    def __init__(self, dim, num_heads, window_size, shift_size, qkv_bias, drop_path):
        super().__init__()
        self.dim, self.num_heads, self.window_size, self.shift_size = dim, num_heads, window_size, shift_size
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention3D(dim, window_size, num_heads, qkv_bias)
        self.drop_prob = float(drop_path)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, 4 * dim)


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size, qkv_bias, drop_path, downsample):
        super().__init__()
        self.dim, self.depth, self.window_size = dim, depth, window_size
        self.shift_size = tuple(i // 2 for i in window_size)
        self.blocks = nn.ModuleList([
            SwinTransformerBlock3D(dim, num_heads, window_size, (0, 0, 0) if i % 2 == 0 else self.shift_size, qkv_bias, drop_path[i])
            for i in range(depth)])
        self.downsample = PatchMerging(dim) if downsample else None


class PatchEmbed3D(nn.Module):
    def __init__(self, patch_size, in_chans, embed_dim, norm: bool):
        super().__init__()
        self.patch_size, self.in_chans, self.embed_dim = patch_size, in_chans, embed_dim
        self.proj = nn.Conv3d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.LayerNorm(embed_dim) if norm else None


def _block_ops(blk: SwinTransformerBlock3D):
    a = blk.attn
    return SimpleNamespace(qkv=_linear_ops(a.qkv), proj=_linear_ops(a.proj), fc1=_linear_ops(blk.mlp.fc1), fc2=_linear_ops(blk.mlp.fc2),
                           g1=_f32(blk.norm1.weight), b1=_f32(blk.norm1.bias), g2=_f32(blk.norm2.weight), b2=_f32(blk.norm2.bias),
                           eps=float(blk.norm1.eps), table=_f32(a.relative_position_bias_table),
                           eye=torch.eye(blk.dim, dtype=BF16, device=a.qkv.weight.device))


# ----------------------------------------------------------------------------------------------
# one block: forward / backward on raw buffers
# ----------------------------------------------------------------------------------------------
def _block_forward(x, o, geo, f1, f2, save: bool):
    """x [M, C] f32 -> the block's output.  ``geo`` = (B, D, G, heads, window, shift, full window); ``f1`` / ``f2`` [B] or None:
    the DropPath factor of every clip on the attention and on the MLP branch (None = 1)."""
    B, D, G, H, win, shift, full = geo
    dev = x.device
    M, C = x.shape
    R = D * G * G      # rows of a clip
    r1 = dict(af=f1, ntok=R) if f1 is not None else {}
    r2 = dict(af=f2, ntok=R) if f2 is not None else {}
    xl, mean1, rstd1 = _ln(x, o.g1, o.b1, M, C, o.eps)
    qkv = _empty((M, 3 * C), BF16, dev)
    ops.gemm(xl, o.qkv.W, ops.EPI_BF16, qkv, bias=o.qkv.b)
    ao, lse = _empty((M, C), BF16, dev), _empty((M, H), F32, dev)
    ops.swin3d_attn_fwd(qkv, o.table, ao, lse, B, D, G, H, win, shift, full)
    x1 = _empty((M, C), F32, dev)
    ops.gemm(ao, o.proj.W, ops.EPI_F32, x1, bias=o.proj.b, resid=x, **r1)      # x1 = x + f1 (ao proj^T + b)
    xn, mean2, rstd2 = _ln(x1, o.g2, o.b2, M, C, o.eps)
    h_pre, h = _empty((M, 4 * C), BF16, dev), _empty((M, 4 * C), BF16, dev)
    ops.gemm(xn, o.fc1.W, ops.EPI_ACT, h, bias=o.fc1.b, out2=h_pre, act=ops.ACT_GELU, **r2)      # h = f2 GELU(pre)
    x2 = _empty((M, C), F32, dev)
    ops.gemm(h, o.fc2.W, ops.EPI_F32, x2, bias=o.fc2.b, resid=x1, rs_bias_only=f2 is not None, **r2)
    if not save:
        return x2, None
    return x2, dict(x=x, f1=f1, f2=f2, xl=xl, mean1=mean1, rstd1=rstd1, qkv=qkv, ao=ao, lse=lse, x1=x1, xn=xn, mean2=mean2,
                    rstd2=rstd2, h_pre=h_pre, h=h)


def _block_backward(dyb, c, o, gr: Dict[str, torch.Tensor], geo):
    """dyb = d(loss)/d(output) [M, C] bf16 -> d(loss)/d(x) bf16.  ``gr``: this block's fp32 gradient buffers by parameter name
    under the block's prefix (missing = not wanted); every kernel ACCUMULATES into them."""
    B, D, G, H, win, shift, full = geo
    dev = dyb.device
    M, C = dyb.shape
    R = D * G * G
    g = gr.get
    f1, f2 = c["f1"], c["f2"]
    r1 = dict(af=f1, ntok=R) if f1 is not None else {}
    r2 = dict(af=f2, ntok=R) if f2 is not None else {}

    def wgrad(gm, a, wname, bname):
        dw, db = g(wname), g(bname)
        if dw is not None:
            ops.wgrad(gm, a, dw, db)
        elif db is not None:
            ops.colsum(gm, db)

    def norm_gb(dy, x, mean, rstd, name):
        if g(name + ".weight") is not None or g(name + ".bias") is not None:
            ops.layernorm_gb_bwd(dy, x, mean, rstd, M, C, g(name + ".weight"), g(name + ".bias"))

    # ---- x2 = x1 + h fc2^T + f2 fc2.b,  h = f2 GELU(xn fc1^T + fc1.b)
    if f2 is None:
        wgrad(dyb, c["h"], "mlp.fc2.weight", "mlp.fc2.bias")
    else:
        if g("mlp.fc2.weight") is not None:
            ops.wgrad(dyb, c["h"], g("mlp.fc2.weight"))
        if g("mlp.fc2.bias") is not None:
            ops.colsum(dyb, g("mlp.fc2.bias"), **r2)
    dh = _empty((M, 4 * C), BF16, dev)
    ops.gemm(dyb, o.fc2.WT, ops.EPI_DACT, dh, aux=c["h_pre"], act=ops.ACT_GELU, **r2)
    wgrad(dh, c["xn"], "mlp.fc1.weight", "mlp.fc1.bias")
    dxn = _empty((M, C), BF16, dev)
    ops.gemm(dh, o.fc1.WT, ops.EPI_BF16, dxn)
    del dh
    dx1b = _empty((M, C), BF16, dev)
    ops.layernorm_bwd(dxn, c["x1"], o.g2, c["mean2"], c["rstd2"], M, C, lddy=C, ldx=C, lddx=C, dres=dyb, dx_bf16=dx1b)
    norm_gb(dxn, c["x1"], c["mean2"], c["rstd2"], "norm2")
    del dxn
    # ---- x1 = x + f1 (ao proj^T + proj.b): the gradient of the bracket is f1 * d(x1), needed as a bf16 operand of the weight
    # gradient: one C x C identity GEMM with f1 in its epilogue (exact products; not launched where f1 is 1), as in timesformer.py
    g1 = dx1b
    if f1 is not None:
        g1 = _empty((M, C), BF16, dev)
        ops.gemm(dx1b, o.eye, ops.EPI_BF16, g1, **r1)
    wgrad(g1, c["ao"], "attn.proj.weight", "attn.proj.bias")
    dao = _empty((M, C), BF16, dev)
    ops.gemm(g1, o.proj.WT, ops.EPI_BF16, dao)
    del g1
    dqkv, delta = _empty((M, 3 * C), BF16, dev), _empty((M, H), F32, dev)
    ops.swin3d_attn_bwd(c["qkv"], o.table, dao, c["lse"], delta, dqkv, g("attn.relative_position_bias_table"), B, D, G, H, win,
                        shift, full)
    del dao, delta
    wgrad(dqkv, c["xl"], "attn.qkv.weight", "attn.qkv.bias")
    dxl = _empty((M, C), BF16, dev)
    ops.gemm(dqkv, o.qkv.WT, ops.EPI_BF16, dxl)
    del dqkv
    dxb = _empty((M, C), BF16, dev)
    ops.layernorm_bwd(dxl, c["x"], o.g1, c["mean1"], c["rstd1"], M, C, lddy=C, ldx=C, lddx=C, dres=dx1b, dx_bf16=dxb)
    norm_gb(dxl, c["x"], c["mean1"], c["rstd1"], "norm1")
    return dxb


# ----------------------------------------------------------------------------------------------
# whole backbone as one autograd node
# ----------------------------------------------------------------------------------------------
class _Swin3DFn(torch.autograd.Function):
    """imgs -> [B, C_last, D', H', W'].  Differentiable inputs: every parameter, in ``named_parameters()`` order."""

    @staticmethod
    def forward(ctx, model: "SwinTransformer3D", grad_enabled: bool, imgs: torch.Tensor, *params: torch.Tensor):
        B, _, Tin, Hh, Ww = imgs.shape
        pt, p = model.patch_size[0], model.patch_size[1]
        D, G0, C0 = Tin // pt, Hh // p, model.embed_dim
        F, dev = B * D, imgs.device
        need = [grad_enabled and bool(ctx.needs_input_grad[3 + k]) for k in range(len(params))]
        need_grad = any(need)
        o = model._operands()
        # stem: Conv3d as one GEMM over the patch matrix [(frame, position), (offset, c, py, px)]; bias in the fp32 epilogue
        K = 3 * p * p
        A = _empty((B * Tin * G0 * G0, K), BF16, dev)
        ops.patchify(imgs, A, B, Tin, Hh, Ww, p, K)
        A = A.view(F, pt, G0 * G0, K).permute(0, 2, 1, 3).reshape(F * G0 * G0, pt * K)
        tok = _empty((F * G0 * G0, C0), F32, dev)
        ops.gemm(A, o.conv, ops.EPI_F32, tok, bias=o.conv_b)
        stem = dict(A=A, tok=tok)
        if o.pnorm is not None:
            x, stem["mean"], stem["rstd"] = _ln(tok, o.pnorm.g, o.pnorm.b, F * G0 * G0, C0, o.pnorm.eps, f32_out=True)
        else:
            x = tok
        factors = model._drop_factors(B, dev)
        ctxs, merges, grids = [], [], []
        k, G = 0, G0
        for li, layer in enumerate(model.layers):
            C = layer.dim
            grids.append(G)
            for blk in layer.blocks:
                x, c = _block_forward(x, o.blocks[k], model._geo(blk, B, D, G), *factors[k], need_grad)
                ctxs.append(c)
                k += 1
            if layer.downsample is not None:
                x, c = _merge_forward(x, o.merges[li], F, G, C)
                merges.append(c if need_grad else None)
                G //= 2
        C = model.num_features
        y, mean, rstd = _ln(x, o.norm.g, o.norm.b, F * G * G, C, o.norm.eps, f32_out=True)
        if need_grad:
            ctx.model, ctx.dims, ctx.need = model, (B, D, grids), need
            ctx.saved = dict(ctxs=ctxs, merges=merges, ops=o, stem=stem, xL=x, mean=mean, rstd=rstd, params=params)
        return y.view(B, D, G, G, C).permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, dout):
        model = ctx.model
        B, D, grids = ctx.dims
        s, need, o = ctx.saved, ctx.need, ctx.saved["ops"]
        F, dev = B * D, dout.device
        # every kernel ACCUMULATES into these; with `grad_in_place` they are the `param.grad` views of the flat gradient buffer
        G_ = GradBufs(model._param_names(), s["params"], need, dev, model.grad_in_place)
        C = model.num_features
        G = grids[-1] // 2 if model.layers[-1].downsample is not None else grids[-1]
        M = F * G * G
        dy = dout.permute(0, 2, 3, 4, 1).reshape(M, C).contiguous().float()
        dxb = _empty((M, C), BF16, dev)
        ops.layernorm_bwd(dy, s["xL"], o.norm.g, s["mean"], s["rstd"], M, C, lddy=C, ldx=C, lddx=C, dx_bf16=dxb)
        if G_["norm.weight"] is not None or G_["norm.bias"] is not None:
            ops.layernorm_gb_bwd(dy, s["xL"], s["mean"], s["rstd"], M, C, G_["norm.weight"], G_["norm.bias"])
        s["xL"] = None
        k = len(s["ctxs"])
        for li in reversed(range(len(model.layers))):
            layer, G = model.layers[li], grids[li]
            if layer.downsample is not None:
                dxb = _merge_backward(dxb, s["merges"][li], o.merges[li], G_.block(f"layers.{li}.downsample."), F, G, layer.dim)
                s["merges"][li] = None
            for bi in reversed(range(layer.depth)):
                k -= 1
                dxb = _block_backward(dxb, s["ctxs"][k], o.blocks[k], G_.block(f"layers.{li}.blocks.{bi}."),
                                      model._geo(layer.blocks[bi], B, D, G))
                s["ctxs"][k] = None
        # stem: patch_embed.norm, then the conv's weight and bias from the saved patch matrix
        stem, gw, gb = s["stem"], G_["patch_embed.proj.weight"], G_["patch_embed.proj.bias"]
        M0, C0 = dxb.shape
        if o.pnorm is not None:
            gnw, gnb = G_["patch_embed.norm.weight"], G_["patch_embed.norm.bias"]
            if gnw is not None or gnb is not None:
                ops.layernorm_gb_bwd(dxb, stem["tok"], stem["mean"], stem["rstd"], M0, C0, gnw, gnb)
            if gw is not None or gb is not None:
                dtok = _empty((M0, C0), BF16, dev)
                ops.layernorm_bwd(dxb, stem["tok"], o.pnorm.g, stem["mean"], stem["rstd"], M0, C0, lddy=C0, ldx=C0, lddx=C0, dx_bf16=dtok)
                dxb = dtok
        if gw is not None:
            pt, K = model.patch_size[0], stem["A"].shape[1] // model.patch_size[0]
            dwc = torch.zeros((C0, pt * K), dtype=F32, device=dev)
            ops.wgrad(dxb, stem["A"], dwc, gb)
            gw.add_(dwc.view(C0, pt, 3, K // 3).permute(0, 2, 1, 3).reshape(gw.shape))
        elif gb is not None:
            ops.colsum(dxb, gb)
        ctx.saved = None
        return G_.result(3)


@BACKBONES.register_module()
class SwinTransformer3D(FullParamBackbone):
    """Video Swin (reference swin_transformer.py:456-668); constructor keywords and defaults of the reference."""

    def __init__(self, pretrained=None, pretrained2d=True, patch_size=(4, 4, 4), in_chans=3, embed_dim=96, depths=[2, 2, 6, 2],
                 num_heads=[3, 6, 12, 24], window_size=(2, 7, 7), mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0.2, norm_layer=nn.LayerNorm, patch_norm=False, frozen_stages=-1,
                 use_checkpoint=False):
        super().__init__()
        name = "SwinTransformer3D"
        if qk_scale is not None:
            raise NotImplementedError(f"{name}(qk_scale=...) is not built: the attention kernels scale by head_dim ** -0.5")
        if drop_rate != 0 or attn_drop_rate != 0:
            raise NotImplementedError(f"{name}(drop_rate / attn_drop_rate > 0): dropout is not built")
        if in_chans != 3:
            raise NotImplementedError(f"{name}(in_chans={in_chans}): only 3-channel clips are built")
        if mlp_ratio != 4:
            raise NotImplementedError(f"{name}(mlp_ratio={mlp_ratio}): only mlp_ratio=4 is built")
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError(f"{name}(norm_layer={norm_layer!r}): only nn.LayerNorm is built")
        if use_checkpoint:
            raise NotImplementedError(f"{name}(use_checkpoint=True): activation recompute is not built")
        if isinstance(patch_size, int) or len(patch_size) != 3 or patch_size[1] != patch_size[2]:
            raise ValueError(f"{name}(patch_size={patch_size!r}): a (pt, p, p) tuple is needed")
        patch_size = tuple(int(v) for v in patch_size)
        if (3 * patch_size[1] ** 2) % 8 != 0:
            raise ValueError(f"{name}(patch_size={patch_size!r}): the patch side must give a patch row of a multiple of 8 values")
        if isinstance(window_size, int) or len(window_size) != 3:
            raise ValueError(f"{name}(window_size={window_size!r}): a (wt, wh, ww) tuple is needed")
        window_size = tuple(int(v) for v in window_size)
        ntab = (2 * window_size[0] - 1) * (2 * window_size[1] - 1) * (2 * window_size[2] - 1)
        if window_size[0] * window_size[1] * window_size[2] > MAX_WINDOW_TOKENS or ntab > MAX_TABLE_ENTRIES:
            raise ValueError(f"{name}(window_size={window_size}): {window_size[0] * window_size[1] * window_size[2]} tokens per window and "
                             f"{ntab} bias-table entries; the attention kernels take at most {MAX_WINDOW_TOKENS} and {MAX_TABLE_ENTRIES}")
        if len(depths) != len(num_heads):
            raise ValueError(f"{name}: depths {depths} and num_heads {num_heads} differ in length")
        for i, h in enumerate(num_heads):
            dim = embed_dim * 2 ** i
            if dim % h != 0 or dim // h != HEAD_DIM:
                raise ValueError(f"{name}: stage {i} has dim {dim} / {h} heads; the HIP attention kernels are built for head_dim {HEAD_DIM}")
        self.pretrained, self.pretrained2d = pretrained, pretrained2d
        self.num_layers, self.embed_dim, self.patch_norm = len(depths), embed_dim, patch_norm
        self.frozen_stages, self.window_size, self.patch_size = frozen_stages, window_size, patch_size
        self.patch_embed = PatchEmbed3D(patch_size, in_chans, embed_dim, patch_norm)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList([
            BasicLayer(int(embed_dim * 2 ** i), depths[i], num_heads[i], window_size, qkv_bias,
                       dpr[sum(depths[:i]):sum(depths[:i + 1])], i < self.num_layers - 1) for i in range(self.num_layers)])
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.norm = nn.LayerNorm(self.num_features)
        self._freeze_stages()

    # ---- reference API ------------------------------------------------------------------------
    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 1:
            self.pos_drop.eval()
            for i in range(0, self.frozen_stages):
                self.layers[i].eval()
                for p in self.layers[i].parameters():
                    p.requires_grad = False

    def inflate_weights(self, state_dict=None):
        """The reference's ``inflate_weights`` (:538-594) on the 2-D Swin checkpoint ``self.pretrained`` (or its ``'model'``
        dict given directly): drop the ``relative_position_index`` and ``attn_mask`` buffers, inflate the patch conv over
        ``patch_size[0]`` and divide by it, bicubic-interpolate a bias table whose side differs from this window's, repeat it
        over the 2 wt - 1 temporal offsets, load with ``strict=False``."""
        if state_dict is None:
            state_dict = torch.load(self.pretrained, map_location='cpu')['model']
        state_dict = dict(state_dict)
        for k in [k for k in state_dict if "relative_position_index" in k or "attn_mask" in k]:
            del state_dict[k]
        pt = self.patch_size[0]
        state_dict['patch_embed.proj.weight'] = state_dict['patch_embed.proj.weight'].unsqueeze(2).repeat(1, 1, pt, 1, 1) / pt
        own = self.state_dict()
        wd = self.window_size[0]
        for k in [k for k in state_dict if "relative_position_bias_table" in k]:
            pre, cur = state_dict[k], own[k]
            L1, nH1 = pre.size()
            L2, nH2 = cur.size()
            L2 = (2 * self.window_size[1] - 1) * (2 * self.window_size[2] - 1)
            if nH1 != nH2:
                _LOG.warning("Error in loading %s, passing", k)
            elif L1 != L2:
                S1 = int(L1 ** 0.5)
                pre = torch.nn.functional.interpolate(pre.permute(1, 0).view(1, nH1, S1, S1),
                                                      size=(2 * self.window_size[1] - 1, 2 * self.window_size[2] - 1), mode='bicubic')
                pre = pre.view(nH2, L2).permute(1, 0)
            state_dict[k] = pre.repeat(2 * wd - 1, 1)
        msg = self.load_state_dict(state_dict, strict=False)
        _LOG.info('%s', msg)
        _LOG.info("=> loaded successfully '%s'", self.pretrained)
        self._last_load = msg
        self._operand_cache = None
        return msg

    def init_weights(self, pretrained=None):
        """Reference ``init_weights`` (:596-623): ``_init_weights``, then a local checkpoint -- a 2-D Swin one through
        ``inflate_weights`` where ``pretrained2d``, else a Video Swin one loaded directly (``strict=False``)."""
        if self._init_then_wants_load(pretrained):
            _LOG.info('load model from: %s', self.pretrained)
            if self.pretrained2d:
                self.inflate_weights()
            else:
                ck = torch.load(self.pretrained, map_location='cpu')
                sd = ck.get('state_dict', ck.get('model', ck))
                sd = {(k[len('backbone.'):] if k.startswith('backbone.') else k): v for k, v in sd.items()}
                self._last_load = self.load_state_dict(sd, strict=False)
                self._operand_cache = None

    def train(self, mode=True):
        """Convert the model into training mode while keep layers freezed."""
        super().train(mode)
        self._freeze_stages()
        return self

    def set_precision(self, precision: str):
        if precision == 'fp32':
            raise NotImplementedError("SwinTransformer3D has no fp32 mode")
        return super().set_precision(precision)

    # ---- operand staging, geometry, DropPath --------------------------------------------------
    def _blocks(self) -> List[SwinTransformerBlock3D]:
        return [blk for layer in self.layers for blk in layer.blocks]

    def _operands(self):
        """bf16 copies (both orientations) of every GEMM weight, the fp32 vectors and bias tables, cached until a parameter
        changes (``_cached_operands``)"""
        return self._cached_operands([p for p in self.parameters()], self._build_operands)

    def _build_operands(self):
        pe = self.patch_embed
        w = pe.proj.weight                                            # [C, 3, pt, p, p] -> [C, (pt, 3, p, p)]
        ln = lambda m: SimpleNamespace(g=_f32(m.weight), b=_f32(m.bias), eps=float(m.eps))
        merges = []
        for layer in self.layers:
            d = layer.downsample
            merges.append(None if d is None else SimpleNamespace(W=_cast(d.reduction.weight), WT=_cast(d.reduction.weight, True),
                                                                 g=_f32(d.norm.weight), b=_f32(d.norm.bias), eps=float(d.norm.eps)))
        return SimpleNamespace(conv=_cast(w.detach().permute(0, 2, 1, 3, 4).reshape(w.shape[0], -1)), conv_b=_f32(pe.proj.bias),
                               pnorm=None if pe.norm is None else ln(pe.norm), blocks=[_block_ops(b) for b in self._blocks()],
                               merges=merges, norm=ln(self.norm))

    def _geo(self, blk: SwinTransformerBlock3D, B: int, D: int, G: int):
        win, shift = get_window_size((D, G, G), blk.window_size, blk.shift_size)
        return B, D, G, blk.num_heads, win, shift, blk.window_size

    def _drop_factors(self, B, dev):
        """Per block (f1, f2), each None or the DropPath factors (0 or 1 / keep) the reference would draw, in its order: one
        entry per clip for the attention branch, then one per clip for the MLP branch; a block whose rate is 0, or that is in
        eval mode (the whole model, or a frozen stage), draws nothing."""
        out = []
        for blk in self._blocks():
            rate = blk.drop_prob
            if not blk.training or rate == 0.0:
                out.append((None, None))
                continue
            keep = 1.0 - rate
            draw = lambda: torch.empty((B,), dtype=F32, device=dev).bernoulli_(keep).div_(keep)
            f1 = draw()
            out.append((f1, draw()))
        return out

    def _check_grid(self, x):
        """the clip checks that need its size: what the reference pads (and then attends over) is refused"""
        name = "SwinTransformer3D"
        B, C, T, Hh, Ww = x.shape
        pt, p = self.patch_size[0], self.patch_size[1]
        if Hh != Ww:
            raise ValueError(f"{name}: a square clip is needed, got {Hh} x {Ww}")
        if T % pt or Hh % p:
            raise ValueError(f"{name}: clip {T} x {Hh} x {Ww} is not a multiple of the patch {self.patch_size} "
                             "(the reference zero-pads it; that is not built)")
        D, G = T // pt, Hh // p
        for i, layer in enumerate(self.layers):
            win, _ = get_window_size((D, G, G), layer.window_size, layer.shift_size)
            if G < layer.window_size[1] or G < layer.window_size[2]:
                raise ValueError(f"{name}: stage {i}'s grid side {G} is smaller than the window side {layer.window_size[1:]}: the "
                                 "reference's relative_position_index[:N, :N] slice then pairs tokens with the wrong table rows")
            if D % win[0] or G % win[1] or G % win[2]:
                raise ValueError(f"{name}: window {win} does not divide stage {i}'s token grid ({D}, {G}, {G}) "
                                 "(the reference zero-pads there and the padded tokens take part in attention; that is not built)")
            if layer.downsample is not None:
                if G % 2:
                    raise ValueError(f"{name}: stage {i}'s grid side {G} is odd and cannot be merged 2 x 2 (the reference pads it)")
                G //= 2

    # ---- forward --------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        if x.dim() != 5:
            raise ValueError(f"SwinTransformer3D takes clips [B, 3, T, S, S], got {tuple(x.shape)}")
        self._check_grid(x)
        self.num_frames = x.shape[2]      # (any frame count the grid checks accept)
        x = self._check_clip(x, x.shape[3])
        if self.inference_precision == 'fp8' and not self._fp8_warned:
            self._fp8_warned = True
            _LOG.warning("fp8 inference was requested but SwinTransformer3D has no fp8 path: this forward runs bf16")
        return _Swin3DFn.apply(self, torch.is_grad_enabled(), x, *[p for _, p in self.named_parameters()])
