"""``SwinTransformer2D_Adapter`` backbone (AIM on a Swin image backbone, the other half of the AIM paper) on the HIP kernels.

Drop-in for ``mmaction/models/backbones/swin2d_adapter.py`` of the reference: same registry name, constructor keywords,
``state_dict`` keys, shapes and buffers (``relative_position_index``, ``attn_mask``, ``t_relative_coords``), ``init_weights``
policy and ``forward(x[B,3,T,224,224]) -> [B, C_last, T', H_last, W_last]``.  Every parameter trains (``frozen_stages=-1``);
``frozen_stages >= 0`` is honoured through ``requires_grad`` plus ``eval()`` in ``train()``, and a parameter whose
``requires_grad`` is False gets ``None`` and costs no launch.

Rows are frame-major, m = (b T' + t') L + h G + w, fp32 residual stream.  One block (:356-403), with ``attn.qkv``, ``attn.proj``
and ``norm1`` used by BOTH attentions of an even block (their gradients add):

- even blocks first: x += dp_t * T_Adapter(proj(temporal attention(qkv(norm1(x))))) over the T' tokens of every (clip,
  position) under the temporal relative bias (``aim_swin_tattn_*``).  ``dp_t`` has one entry per (clip, position): it rides the
  epilogues as a per-ROW factor (``at`` with ``ntok`` = all rows);
- x += S_Adapter2(proj(window attention(qkv(norm1(x))))) (skip inside the adapter, no DropPath): ``aim_swin_win_attn_*`` reads
  the rolled, partitioned and masked windows by address, so nothing is rolled or copied into window order;
- xn = norm2(x); x += mlp(xn) + dp_m * 0.5 * S_Adapter(xn), ``dp_m`` per frame (the epilogues' ``af``).

The dense biases [heads, S, S] are gathered from the tables once per operand build; their gradients come back dense from
the attention backward (two-stage fixed-order sums) and are folded into the tables by ``aim_swin_bias_scatter``.  Every GEMM
weight gradient uses the split-M, fixed-order ``aim_wgrad_bias_bf16``: the step is bitwise reproducible.

Torch glue in this file (not kernels): the patch matrix's (frame, offset) -> K reordering of the stem, the 2 x 2 gather of
PatchMerging and its scatter back, and the output's layout change.
"""
import logging
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch
from torch import nn

from . import ops
from .backbone import BF16, F32, _cast, _empty
from .full_param import FullParamBackbone, GradBufs
from .registry import BACKBONES

_LOG = logging.getLogger("aim_amd")

HEAD_DIM = 32          # the Swin attention kernels' head width
MAX_WINDOW_TOKENS = 64
MAX_T = 32


# ----------------------------------------------------------------------------------------------
# parameter containers (the reference's names, so its state_dicts and the Swin checkpoints load)
# ----------------------------------------------------------------------------------------------
class Adapter(nn.Module):
    """Bottleneck adapter parameters (``Adapter`` / ``SAdapter2`` / ``T_Adapter``, :11-60; erf GELU; the skip is the block's)."""

    def __init__(self, D_features: int, mlp_ratio: float = 0.25):
        super().__init__()
        hidden = int(D_features * mlp_ratio)
        self.D_fc1 = nn.Linear(D_features, hidden)
        self.D_fc2 = nn.Linear(hidden, D_features)


class Mlp(nn.Module):
    def __init__(self, in_features: int, hidden_features: int):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)


def relative_position_index(w: int) -> torch.Tensor:
    """[S, S] index into the (2w-1)^2 table (:187-196)"""
    coords = torch.stack(torch.meshgrid([torch.arange(w), torch.arange(w)], indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += w - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * w - 1
    return rel.sum(-1)


def shift_mask(res: int, w: int, s: int) -> torch.Tensor:
    """[nW, S, S] additive mask of a shifted block, 0 / -100 (:331-350).  The kernels do not read it: they give the masked
    pairs the weight exactly 0."""
    img = torch.zeros((1, res, res, 1))
    cnt = 0
    for hs in (slice(0, -w), slice(-w, -s), slice(-s, None)):
        for ws in (slice(0, -w), slice(-w, -s), slice(-s, None)):
            img[:, hs, ws, :] = cnt
            cnt += 1
    mw = img.view(1, res // w, w, res // w, w, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, float(-100.0)).masked_fill(m == 0, float(0.0))


class WindowAttention(nn.Module):
    def __init__(self, dim, num_ttokens, window, num_heads, use_temporal, qkv_bias):
        super().__init__()
        self.dim, self.window, self.num_heads = dim, window, num_heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, num_heads))
        self.register_buffer("relative_position_index", relative_position_index(window))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        if use_temporal:
            self.num_ttokens = num_ttokens
            self.temporal_position_bias_table = nn.Parameter(torch.zeros(2 * num_ttokens - 1, num_heads))
            nn.init.trunc_normal_(self.temporal_position_bias_table, std=.02)
            t = torch.arange(num_ttokens)
            self.register_buffer("t_relative_coords", (t[:, None] - t[None, :] + num_ttokens - 1).view(-1))


class SwinTransformerBlock(nn.Module):
    """Parameters and geometry of one block (:276-354); compute lives in ``_block_forward`` / ``_block_backward``."""

    def __init__(self, dim, res, num_frames, num_heads, window_size, shift_size, t_attn, qkv_bias, drop_path):
        super().__init__()
        self.dim, self.res, self.num_frames, self.num_heads = dim, res, num_frames, num_heads
        self.window_size, self.shift_size = window_size, shift_size
        if res <= window_size:           # the window becomes the resolution and nothing is shifted (:306-309)
            self.shift_size, self.window_size = 0, res
        self.t_attn = t_attn
        if t_attn:
            self.T_Adapter = Adapter(dim)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, num_frames, self.window_size, num_heads, t_attn, qkv_bias)
        self.drop_prob = float(drop_path)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, 4 * dim)
        self.S_Adapter = Adapter(dim)
        self.S_Adapter2 = Adapter(dim)
        self.register_buffer("attn_mask", shift_mask(res, self.window_size, self.shift_size) if self.shift_size > 0 else None)


class PatchMerging(nn.Module):
    def __init__(self, res, dim):
        super().__init__()
        self.res, self.dim = res, dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)


class BasicLayer(nn.Module):
    def __init__(self, dim, res, num_frames, depth, num_heads, window_size, qkv_bias, drop_path, downsample):
        super().__init__()
        self.dim, self.res, self.depth = dim, res, depth
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim, res, num_frames, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, i % 2 == 0,
                                 qkv_bias, drop_path[i]) for i in range(depth)])
        self.downsample = PatchMerging(res, dim) if downsample else None


class PatchEmbed3D(nn.Module):
    def __init__(self, patch_size, in_chans, embed_dim, norm: bool):
        super().__init__()
        self.patch_size, self.in_chans, self.embed_dim = patch_size, in_chans, embed_dim
        self.patches_resolution = [224 // patch_size[1], 224 // patch_size[2]]      # built without img_size (:649): 56 x 56
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.proj = nn.Conv3d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.LayerNorm(embed_dim) if norm else None


# ----------------------------------------------------------------------------------------------
# bf16 operands of this step (every weight trains: rebuilt when a weight changed)
# ----------------------------------------------------------------------------------------------
def _f32(t):
    return t.detach().float().contiguous()


def _dense_bias(table, index, S):
    """table [entries, heads] gathered along index [S*S] -> [heads, S, S] fp32 with dense strides"""
    out = torch.empty((table.shape[1], S, S), dtype=F32, device=table.device)
    out.copy_(_f32(table)[index.reshape(-1)].view(S, S, -1).permute(2, 0, 1))
    return out


def _linear_ops(lin: nn.Linear):
    """W [out, in] and W^T as bf16, the bias as fp32 (zeros where the layer has none: the epilogues always add one)"""
    w = lin.weight
    b = _f32(lin.bias) if lin.bias is not None else torch.zeros(w.shape[0], dtype=F32, device=w.device)
    return SimpleNamespace(W=_cast(w), WT=_cast(w, True), b=b)


def _block_ops(blk: SwinTransformerBlock):
    a, S = blk.attn, blk.window_size ** 2
    o = SimpleNamespace(qkv=_linear_ops(a.qkv), proj=_linear_ops(a.proj), fc1=_linear_ops(blk.mlp.fc1), fc2=_linear_ops(blk.mlp.fc2),
                        S1=_linear_ops(blk.S_Adapter.D_fc1), S2=_linear_ops(blk.S_Adapter.D_fc2),
                        A1=_linear_ops(blk.S_Adapter2.D_fc1), A2=_linear_ops(blk.S_Adapter2.D_fc2),
                        g1=_f32(blk.norm1.weight), b1=_f32(blk.norm1.bias), g2=_f32(blk.norm2.weight), b2=_f32(blk.norm2.bias),
                        eps=float(blk.norm1.eps))
    idx = a.relative_position_index.reshape(-1)
    o.sidx = idx.to(torch.int32).contiguous()
    o.sbias = _dense_bias(a.relative_position_bias_table, idx, S)
    if blk.t_attn:
        T = a.num_ttokens
        o.T1, o.T2 = _linear_ops(blk.T_Adapter.D_fc1), _linear_ops(blk.T_Adapter.D_fc2)
        o.tidx = a.t_relative_coords.to(torch.int32).contiguous()
        o.tbias = _dense_bias(a.temporal_position_bias_table, a.t_relative_coords, T)
    return o


# ----------------------------------------------------------------------------------------------
# one block: forward / backward on raw buffers
# ----------------------------------------------------------------------------------------------
def _ln(x, g, b, M, C, eps, f32_out=False):
    dev = x.device
    y = _empty((M, C), F32 if f32_out else BF16, dev)
    mean, rstd = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x, g, b, M, C, C, mean=mean, rstd=rstd, eps=eps, **({"y_f32": y} if f32_out else {"y_bf16": y}))
    return y, mean, rstd


def _block_forward(x, o, geo, st, dm, save: bool):
    """x [M, C] f32 -> the block's output.  ``geo`` = (B, T', G, heads, window, shift, t_attn); ``st`` [M] or None: the
    temporal branch's DropPath factor of every row; ``dm`` [B*T']: the S_Adapter's per-frame factor (0.5 x its DropPath)."""
    B, T, G, H, w, s, t_attn = geo
    dev = x.device
    M, C = x.shape
    L, F, r, S = G * G, B * T, o.S1.W.shape[0], w * w
    c = dict(x=x, st=st, dm=dm)
    if t_attn:
        rs = dict(at=st, ntok=M) if st is not None else {}
        xl, c["mean1"], c["rstd1"] = _ln(x, o.g1, o.b1, M, C, o.eps)
        qkv_t = _empty((M, 3 * C), BF16, dev)
        ops.gemm(xl, o.qkv.W, ops.EPI_BF16, qkv_t, bias=o.qkv.b)
        ot, lse_t = _empty((M, C), BF16, dev), _empty((B * L, H, ops.swin_attn_cap(T)), F32, dev)
        ops.swin_tattn_fwd(qkv_t, o.tbias, ot, lse_t, B, T, L, H)
        ta = _empty((M, C), BF16, dev)
        ops.gemm(ot, o.proj.W, ops.EPI_BF16, ta, bias=o.proj.b)
        t_pre, t_hs = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
        ops.gemm(ta, o.T1.W, ops.EPI_ACT, t_hs, bias=o.T1.b, out2=t_pre, act=ops.ACT_GELU, **rs)      # t_hs = st * GELU(pre)
        x1 = _empty((M, C), F32, dev)
        ops.gemm(t_hs, o.T2.W, ops.EPI_F32, x1, bias=o.T2.b, resid=x, rs_bias_only=st is not None, **rs)
        c.update(xl=xl, qkv_t=qkv_t, ot=ot, lse_t=lse_t, ta=ta, t_pre=t_pre, t_hs=t_hs)
    else:
        x1 = x
    # ---- spatial: norm1 -> qkv -> shifted-window attention -> proj -> S_Adapter2 (skip inside)
    xl2, c["mean1b"], c["rstd1b"] = _ln(x1, o.g1, o.b1, M, C, o.eps)
    qkv_s = _empty((M, 3 * C), BF16, dev)
    ops.gemm(xl2, o.qkv.W, ops.EPI_BF16, qkv_s, bias=o.qkv.b)
    ao, lse_s = _empty((M, C), BF16, dev), _empty((F * (G // w) ** 2, H, ops.swin_attn_cap(S)), F32, dev)
    ops.swin_win_attn_fwd(qkv_s, o.sbias, ao, lse_s, F, G, H, w, s)
    sa = _empty((M, C), BF16, dev)
    ops.gemm(ao, o.proj.W, ops.EPI_BF16, sa, bias=o.proj.b)
    s_pre, s_h = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(sa, o.A1.W, ops.EPI_ACT, s_h, bias=o.A1.b, out2=s_pre, act=ops.ACT_GELU)
    x2 = _empty((M, C), F32, dev)
    ops.gemm(s_h, o.A2.W, ops.EPI_F32, x2, bias=o.A2.b, resid=x1)
    ops.acc_bf16(x2, sa)
    # ---- x3 = x2 + fc2(GELU(fc1(xn))) + dm[frame] * S_Adapter(xn)
    xn, c["mean2"], c["rstd2"] = _ln(x2, o.g2, o.b2, M, C, o.eps)
    h_pre, h = _empty((M, 4 * C), BF16, dev), _empty((M, 4 * C), BF16, dev)
    ops.gemm(xn, o.fc1.W, ops.EPI_ACT, h, bias=o.fc1.b, out2=h_pre, act=ops.ACT_GELU)
    xm = _empty((M, C), F32, dev)
    ops.gemm(h, o.fc2.W, ops.EPI_F32, xm, bias=o.fc2.b, resid=x2)
    a_pre, a_s = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(xn, o.S1.W, ops.EPI_ACT, a_s, bias=o.S1.b, out2=a_pre, act=ops.ACT_GELU, af=dm, ntok=L)       # a_s = dm * GELU(pre)
    x3 = _empty((M, C), F32, dev)
    ops.gemm(a_s, o.S2.W, ops.EPI_F32, x3, bias=o.S2.b, resid=xm, af=dm, ntok=L, rs_bias_only=True)
    if not save:
        return x3, None
    c.update(x1=x1, xl2=xl2, qkv_s=qkv_s, ao=ao, lse_s=lse_s, sa=sa, s_pre=s_pre, s_h=s_h, x2=x2, xn=xn, h_pre=h_pre, h=h,
             a_pre=a_pre, a_s=a_s)
    return x3, c


def _block_backward(dyb, c, o, gr: Dict[str, torch.Tensor], geo):
    """dyb = d(loss)/d(output) [M, C] bf16 -> d(loss)/d(x) bf16.  ``gr``: this block's fp32 gradient buffers by parameter name
    under the block's prefix (missing = not wanted); every kernel ACCUMULATES into them."""
    B, T, G, H, w, s, t_attn = geo
    dev = dyb.device
    M, C = dyb.shape
    L, F, r, S = G * G, B * T, o.S1.W.shape[0], w * w
    g = gr.get
    st, dm = c["st"], c["dm"]

    def wgrad(gm, a, wname, bname):
        dw, db = g(wname), g(bname)
        if dw is not None:
            ops.wgrad(gm, a, dw, db)
        elif db is not None:
            ops.colsum(gm, db)

    def norm_gb(dy, x, mean, rstd, name):
        if g(name + ".weight") is not None or g(name + ".bias") is not None:
            ops.layernorm_gb_bwd(dy, x, mean, rstd, M, C, g(name + ".weight"), g(name + ".bias"))

    def table_grad(dense, index, name):
        if dense is not None:
            ops.swin_bias_scatter(dense, index, g(name))

    # ---- x3 = xm + a_s S2^T + dm[f] S2.b,  a_s = dm[f] GELU(xn S1^T + S1.b);  xm = x2 + GELU(xn fc1^T + b) fc2^T + b
    if g("S_Adapter.D_fc2.weight") is not None:
        ops.wgrad(dyb, c["a_s"], g("S_Adapter.D_fc2.weight"))
    if g("S_Adapter.D_fc2.bias") is not None:
        ops.colsum(dyb, g("S_Adapter.D_fc2.bias"), af=dm, ntok=L)
    da = _empty((M, r), BF16, dev)
    ops.gemm(dyb, o.S2.WT, ops.EPI_DACT, da, aux=c["a_pre"], act=ops.ACT_GELU, af=dm, ntok=L)
    wgrad(da, c["xn"], "S_Adapter.D_fc1.weight", "S_Adapter.D_fc1.bias")
    wgrad(dyb, c["h"], "mlp.fc2.weight", "mlp.fc2.bias")
    dh = _empty((M, 4 * C), BF16, dev)
    ops.gemm(dyb, o.fc2.WT, ops.EPI_DACT, dh, aux=c["h_pre"], act=ops.ACT_GELU)
    wgrad(dh, c["xn"], "mlp.fc1.weight", "mlp.fc1.bias")
    dxn_a = _empty((M, C), F32, dev)
    ops.gemm(da, o.S1.WT, ops.EPI_F32, dxn_a)
    dxn = _empty((M, C), F32, dev)
    ops.gemm(dh, o.fc1.WT, ops.EPI_F32, dxn, resid=dxn_a)
    del dh, da, dxn_a
    dx2b = _empty((M, C), BF16, dev)
    ops.layernorm_bwd(dxn, c["x2"], o.g2, c["mean2"], c["rstd2"], M, C, lddy=C, ldx=C, lddx=C, dres=dyb, dx_bf16=dx2b)
    norm_gb(dxn, c["x2"], c["mean2"], c["rstd2"], "norm2")
    del dxn
    # ---- x2 = x1 + sa + s_h A2^T + A2.b,  s_h = GELU(sa A1^T + A1.b),  sa = ao proj^T + proj.b
    wgrad(dx2b, c["s_h"], "S_Adapter2.D_fc2.weight", "S_Adapter2.D_fc2.bias")
    dsh = _empty((M, r), BF16, dev)
    ops.gemm(dx2b, o.A2.WT, ops.EPI_DACT, dsh, aux=c["s_pre"], act=ops.ACT_GELU)
    wgrad(dsh, c["sa"], "S_Adapter2.D_fc1.weight", "S_Adapter2.D_fc1.bias")
    dsa = _empty((M, C), BF16, dev)
    ops.gemm(dsh, o.A1.WT, ops.EPI_BF16, dsa)
    ops.add_bf16(dsa, dx2b, dsa)
    wgrad(dsa, c["ao"], "attn.proj.weight", "attn.proj.bias")
    dao = _empty((M, C), BF16, dev)
    ops.gemm(dsa, o.proj.WT, ops.EPI_BF16, dao)
    del dsa, dsh
    dqkv = _empty((M, 3 * C), BF16, dev)
    dsb = _empty((H, S, S), F32, dev) if g("attn.relative_position_bias_table") is not None else None
    ops.swin_win_attn_bwd(c["qkv_s"], o.sbias, dao, c["lse_s"], dqkv, dsb, F, G, H, w, s)
    table_grad(dsb, o.sidx, "attn.relative_position_bias_table")
    del dao
    wgrad(dqkv, c["xl2"], "attn.qkv.weight", "attn.qkv.bias")
    dxl2 = _empty((M, C), BF16, dev)
    ops.gemm(dqkv, o.qkv.WT, ops.EPI_BF16, dxl2)
    dx1b = _empty((M, C), BF16, dev)
    ops.layernorm_bwd(dxl2, c["x1"], o.g1, c["mean1b"], c["rstd1b"], M, C, lddy=C, ldx=C, lddx=C, dres=dx2b, dx_bf16=dx1b)
    norm_gb(dxl2, c["x1"], c["mean1b"], c["rstd1b"], "norm1")
    del dxl2, dx2b
    if not t_attn:
        return dx1b
    # ---- x1 = x + t_hs T2^T + st[m] T2.b,  t_hs = st[m] GELU(ta T1^T + T1.b),  ta = temporal attention(qkv(norm1(x))) proj^T + proj.b
    rs = dict(at=st, ntok=M) if st is not None else {}
    if g("T_Adapter.D_fc2.weight") is not None:
        ops.wgrad(dx1b, c["t_hs"], g("T_Adapter.D_fc2.weight"))
    if g("T_Adapter.D_fc2.bias") is not None:
        ops.colsum(dx1b, g("T_Adapter.D_fc2.bias"), **rs)
    dth = _empty((M, r), BF16, dev)
    ops.gemm(dx1b, o.T2.WT, ops.EPI_DACT, dth, aux=c["t_pre"], act=ops.ACT_GELU, **rs)
    wgrad(dth, c["ta"], "T_Adapter.D_fc1.weight", "T_Adapter.D_fc1.bias")
    dta = _empty((M, C), BF16, dev)
    ops.gemm(dth, o.T1.WT, ops.EPI_BF16, dta)
    del dth
    wgrad(dta, c["ot"], "attn.proj.weight", "attn.proj.bias")
    dot = _empty((M, C), BF16, dev)
    ops.gemm(dta, o.proj.WT, ops.EPI_BF16, dot)
    del dta
    dtb = _empty((H, T, T), F32, dev) if g("attn.temporal_position_bias_table") is not None else None
    ops.swin_tattn_bwd(c["qkv_t"], o.tbias, dot, c["lse_t"], dqkv, dtb, B, T, L, H)      # (overwrites the spatial branch's d(qkv))
    table_grad(dtb, o.tidx, "attn.temporal_position_bias_table")
    del dot
    wgrad(dqkv, c["xl"], "attn.qkv.weight", "attn.qkv.bias")
    dxl = _empty((M, C), BF16, dev)
    ops.gemm(dqkv, o.qkv.WT, ops.EPI_BF16, dxl)
    del dqkv
    dxb = _empty((M, C), BF16, dev)
    ops.layernorm_bwd(dxl, c["x"], o.g1, c["mean1"], c["rstd1"], M, C, lddy=C, ldx=C, lddx=C, dres=dx1b, dx_bf16=dxb)
    norm_gb(dxl, c["x"], c["mean1"], c["rstd1"], "norm1")
    return dxb


# ----------------------------------------------------------------------------------------------
# PatchMerging (:428-465): 2 x 2 gather (torch), LayerNorm over 4C, bias-free reduction to 2C
# ----------------------------------------------------------------------------------------------
def _merge_gather(x, F, G, C):
    """[F G G, C] -> [F (G/2)^2, 4C] in the order [h even w even | h odd w even | h even w odd | h odd w odd]"""
    v = x.view(F, G, G, C)
    return torch.cat([v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)


def _merge_scatter(d, F, G, C):
    """the inverse of ``_merge_gather`` on a gradient [F (G/2)^2, 4C] -> [F G G, C]"""
    v = d.view(F, G // 2, G // 2, 4, C)
    out = torch.empty((F, G, G, C), dtype=d.dtype, device=d.device)
    out[:, 0::2, 0::2], out[:, 1::2, 0::2], out[:, 0::2, 1::2], out[:, 1::2, 1::2] = v[..., 0, :], v[..., 1, :], v[..., 2, :], v[..., 3, :]
    return out.view(F * G * G, C)


def _merge_forward(x, o, F, G, C):
    xc = _merge_gather(x, F, G, C)
    M4 = xc.shape[0]
    xn, mean, rstd = _ln(xc, o.g, o.b, M4, 4 * C, o.eps)
    y = _empty((M4, 2 * C), F32, x.device)
    ops.gemm(xn, o.W, ops.EPI_F32, y)
    return y, dict(xc=xc, xn=xn, mean=mean, rstd=rstd)


def _merge_backward(dyb, c, o, gr, F, G, C):
    M4 = dyb.shape[0]
    if gr.get("reduction.weight") is not None:
        ops.wgrad(dyb, c["xn"], gr["reduction.weight"])
    dxn = _empty((M4, 4 * C), BF16, dyb.device)
    ops.gemm(dyb, o.WT, ops.EPI_BF16, dxn)
    dxc = _empty((M4, 4 * C), BF16, dyb.device)
    ops.layernorm_bwd(dxn, c["xc"], o.g, c["mean"], c["rstd"], M4, 4 * C, lddy=4 * C, ldx=4 * C, lddx=4 * C, dx_bf16=dxc)
    if gr.get("norm.weight") is not None or gr.get("norm.bias") is not None:
        ops.layernorm_gb_bwd(dxn, c["xc"], c["mean"], c["rstd"], M4, 4 * C, gr.get("norm.weight"), gr.get("norm.bias"))
    return _merge_scatter(dxc, F, G, C)


# ----------------------------------------------------------------------------------------------
# whole backbone as one autograd node
# ----------------------------------------------------------------------------------------------
class _Swin2DAdapterFn(torch.autograd.Function):
    """imgs -> [B, C_last, T', H_last, W_last].  Differentiable inputs: every parameter, in ``named_parameters()`` order."""

    @staticmethod
    def forward(ctx, model: "SwinTransformer2D_Adapter", grad_enabled: bool, imgs: torch.Tensor, *params: torch.Tensor):
        B, _, Tin, Hh, Ww = imgs.shape
        pt, p = model.patch_size[0], model.patch_size[1]
        T, G0, C0 = Tin // pt, Hh // p, model.embed_dim
        F, dev = B * T, imgs.device
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
        factors = model._drop_factors(B, T, dev)
        ctxs, merges = [], []
        k = 0
        for li, layer in enumerate(model.layers):
            G, C = layer.res, layer.dim
            for blk in layer.blocks:
                dp_t, dp_m = factors[k]
                st = None if dp_t is None else dp_t.view(B, 1, G * G).expand(B, T, G * G).reshape(-1).contiguous()
                dm = torch.full((F,), 0.5, dtype=F32, device=dev) if dp_m is None else (0.5 * dp_m).contiguous()
                x, c = _block_forward(x, o.blocks[k], model._geo(blk, B, T), st, dm, need_grad)
                ctxs.append(c)
                k += 1
            if layer.downsample is not None:
                x, c = _merge_forward(x, o.merges[li], F, G, C)
                merges.append(c if need_grad else None)
        G, C = model.layers[-1].res, model.num_features
        y, mean, rstd = _ln(x, o.norm.g, o.norm.b, F * G * G, C, o.norm.eps, f32_out=True)
        if need_grad:
            ctx.model, ctx.dims, ctx.need = model, (B, T), need
            ctx.saved = dict(ctxs=ctxs, merges=merges, ops=o, stem=stem, xL=x, mean=mean, rstd=rstd, params=params)
        return y.view(B, T, G, G, C).permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, dout):
        model = ctx.model
        B, T = ctx.dims
        s, need, o = ctx.saved, ctx.need, ctx.saved["ops"]
        F, dev = B * T, dout.device
        # every kernel ACCUMULATES into these; with `grad_in_place` they are the `param.grad` views of the flat gradient buffer
        G_ = GradBufs(model._param_names(), s["params"], need, dev, model.grad_in_place)
        G, C = model.layers[-1].res, model.num_features
        M = F * G * G
        dy = dout.permute(0, 2, 3, 4, 1).reshape(M, C).contiguous().float()
        dxb = _empty((M, C), BF16, dev)
        ops.layernorm_bwd(dy, s["xL"], o.norm.g, s["mean"], s["rstd"], M, C, lddy=C, ldx=C, lddx=C, dx_bf16=dxb)
        if G_["norm.weight"] is not None or G_["norm.bias"] is not None:
            ops.layernorm_gb_bwd(dy, s["xL"], s["mean"], s["rstd"], M, C, G_["norm.weight"], G_["norm.bias"])
        s["xL"] = None
        k = len(s["ctxs"])
        for li in reversed(range(len(model.layers))):
            layer = model.layers[li]
            if layer.downsample is not None:
                dxb = _merge_backward(dxb, s["merges"][li], o.merges[li], G_.block(f"layers.{li}.downsample."), F, layer.res, layer.dim)
                s["merges"][li] = None
            for bi in reversed(range(layer.depth)):
                k -= 1
                dxb = _block_backward(dxb, s["ctxs"][k], o.blocks[k], G_.block(f"layers.{li}.blocks.{bi}."),
                                      model._geo(layer.blocks[bi], B, T))
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
class SwinTransformer2D_Adapter(FullParamBackbone):
    """AIM on Swin (reference swin2d_adapter.py:600-834); constructor keywords and defaults of the reference."""

    def __init__(self, pretrained=None, img_size=224, patch_size=4, num_frames=32, in_chans=3, num_classes=1000, embed_dim=96,
                 depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4., frozen_stages=-1, qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False,
                 patch_norm=True, t_relative=True, use_checkpoint=False, **kwargs):
        super().__init__()
        name = "SwinTransformer2D_Adapter"
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
        if ape:
            raise NotImplementedError(f"{name}(ape=True): the reference never creates absolute_pos_embed, its forward fails")
        if not t_relative:
            raise NotImplementedError(f"{name}(t_relative=False): the absolute temporal embedding is not built")
        if use_checkpoint:
            raise NotImplementedError(f"{name}(use_checkpoint=True): activation recompute is not built")
        if img_size != 224:
            raise ValueError(f"{name}(img_size={img_size}): the reference builds its patch grid for 224 x 224 clips whatever "
                             "img_size says; only 224 can run")
        if isinstance(patch_size, int) or len(patch_size) != 3 or patch_size[1] != patch_size[2]:
            raise ValueError(f"{name}(patch_size={patch_size!r}): a (pt, p, p) tuple is needed (the reference indexes patch_size[0])")
        patch_size = tuple(int(v) for v in patch_size)
        if 224 % patch_size[1] != 0 or (3 * patch_size[1] ** 2) % 8 != 0:
            raise ValueError(f"{name}(patch_size={patch_size!r}): the patch side must divide 224 and give a patch row of a multiple of 8 values")
        if num_frames % patch_size[0] != 0:
            raise ValueError(f"{name}: num_frames={num_frames} is not a multiple of the temporal patch size {patch_size[0]} "
                             "(the reference pads the clip and then fails in its temporal rearrange)")
        T = num_frames // patch_size[0]
        if T > MAX_T:
            raise ValueError(f"{name}: {T} frame tokens per position, the temporal attention kernel takes at most {MAX_T}")
        if window_size ** 2 > MAX_WINDOW_TOKENS:
            raise ValueError(f"{name}(window_size={window_size}): {window_size ** 2} tokens per window, the window attention "
                             f"kernel takes at most {MAX_WINDOW_TOKENS}")
        if len(depths) != len(num_heads):
            raise ValueError(f"{name}: depths {depths} and num_heads {num_heads} differ in length")
        res0 = 224 // patch_size[1]
        for i, h in enumerate(num_heads):
            dim, res = embed_dim * 2 ** i, res0 // 2 ** i
            if dim % h != 0 or dim // h != HEAD_DIM:
                raise ValueError(f"{name}: stage {i} has dim {dim} / {h} heads; the HIP attention kernels are built for head_dim {HEAD_DIM}")
            if res * 2 ** i != res0 or (i < len(depths) - 1 and res % 2):
                raise ValueError(f"{name}: stage {i}'s resolution {res0} / {2 ** i} cannot be merged 2 x 2")
            if res > window_size and res % window_size != 0:
                raise ValueError(f"{name}: window {window_size} does not divide stage {i}'s resolution {res} "
                                 "(the reference fails in window_partition's view there too)")
        self.num_classes, self.num_layers, self.embed_dim = num_classes, len(depths), embed_dim
        self.ape, self.patch_norm, self.t_relative = ape, patch_norm, t_relative
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.mlp_ratio, self.pretrained, self.num_frames = mlp_ratio, pretrained, num_frames
        self.frozen_stages, self.patch_size, self.img_size = frozen_stages, patch_size, img_size
        self.patch_embed = PatchEmbed3D(patch_size, in_chans, embed_dim, patch_norm)
        self.patches_resolution = self.patch_embed.patches_resolution
        self.num_Ttokens = T
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList([
            BasicLayer(int(embed_dim * 2 ** i), res0 // 2 ** i, T, depths[i], num_heads[i], window_size, qkv_bias,
                       dpr[sum(depths[:i]):sum(depths[:i + 1])], i < self.num_layers - 1) for i in range(self.num_layers)])
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

    def init_weights(self, pretrained=None):
        """Reference ``init_weights`` (:714-775): init, optional load of a local Swin checkpoint with the patch conv inflated
        over the temporal patch, then zero the D_fc2 of every S_Adapter, S_Adapter2 ('S_Adapter' matches both) and T_Adapter."""
        if self._init_then_wants_load(pretrained):
            _LOG.info('load model from: %s', self.pretrained)
            state_dict = torch.load(self.pretrained, map_location='cpu')['model']
            pt = self.patch_size[0]
            state_dict['patch_embed.proj.weight'] = state_dict['patch_embed.proj.weight'].unsqueeze(2).repeat(1, 1, pt, 1, 1) / pt
            msg = self.load_state_dict(state_dict, strict=False)
            _LOG.info('Missing keys: %s', msg.missing_keys)
            _LOG.info('Unexpected keys: %s', msg.unexpected_keys)
            self._last_load = msg
        for n, m in self.layers.named_modules():
            if ('S_Adapter' in n or 'T_Adapter' in n) and n.endswith('D_fc2'):
                nn.init.constant_(m.weight, 0)
                nn.init.constant_(m.bias, 0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'absolute_pos_embed', 'temporal_embedding'}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {'relative_position_bias_table', 'temporal_position_bias_table'}

    def train(self, mode=True):
        """Convert the model into training mode while keep layers freezed."""
        super().train(mode)
        self._freeze_stages()
        return self

    def set_precision(self, precision: str):
        if precision == 'fp32':
            raise NotImplementedError("SwinTransformer2D_Adapter has no fp32 mode")
        return super().set_precision(precision)

    # ---- operand staging, geometry, DropPath --------------------------------------------------
    def _blocks(self) -> List[SwinTransformerBlock]:
        return [blk for layer in self.layers for blk in layer.blocks]

    def _operands(self):
        """bf16 copies (both orientations) of every GEMM weight, the fp32 vectors and the dense attention biases, cached until a
        parameter changes (``_cached_operands``)"""
        return self._cached_operands([p for p in self.parameters()], self._build_operands)

    def _build_operands(self):
        pe, pt = self.patch_embed, self.patch_size[0]
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

    def _geo(self, blk: SwinTransformerBlock, B: int, T: int):
        return B, T, blk.res, blk.num_heads, blk.window_size, blk.shift_size, blk.t_attn

    def _drop_factors(self, B, T, dev):
        """Per block (dp_t, dp_m), each None or the DropPath factors (0 or 1 / keep) the reference would draw, in its order: an
        even block draws dp_t [B * L] (x is ``(b n) t c`` there: one entry per clip and position) and then dp_m [B * T']
        (``(b t) n c``: one per frame); an odd block draws dp_m only; a block whose rate is 0, or that is in eval mode (the whole
        model, or a frozen stage), draws nothing."""
        out = []
        for blk in self._blocks():
            rate = blk.drop_prob
            if not blk.training or rate == 0.0:
                out.append((None, None))
                continue
            keep = 1.0 - rate
            draw = lambda n: torch.empty((n,), dtype=F32, device=dev).bernoulli_(keep).div_(keep)
            dp_t = draw(B * blk.res * blk.res) if blk.t_attn else None
            out.append((dp_t, draw(B * T)))
        return out

    # ---- forward --------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        x = self._check_clip(x, self.img_size)
        if self.inference_precision == 'fp8' and not self._fp8_warned:
            self._fp8_warned = True
            _LOG.warning("fp8 inference was requested but SwinTransformer2D_Adapter has no fp8 path: this forward runs bf16")
        return _Swin2DAdapterFn.apply(self, torch.is_grad_enabled(), x, *[p for _, p in self.named_parameters()])
