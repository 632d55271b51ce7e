"""``ViT_CLIP_ZEROI2V(linear_adapter=True)``: the block with ZeroI2V's purely linear adapters on the fused low-rank kernels,
and the fold of those adapters into the frozen weights (reference vit_clip_zeroI2V.py:15-38, :153-206, :244-311).

LA(x) = x + D_fc2(D_fc1(x)), no activation, ``bottleneck`` hidden units.  Per block, on the P-row slot layout of zeroi2v.py:

  1. (with_t_cls_token) the temporal class token, exactly as without linear adapters: the UN-ADAPTED in_proj / out_proj and the
     GELU T_Adapter; xt lands in row 1 of every frame.
  2. xln = ln_1(x'); Y_q, Y_k, Y_v = LA_{q,k,v}(xln) in ONE ``aim_lowrank_fwd`` (G = 3) that writes three column slabs; the three
     D x D projections read the slabs and write the column slabs of the fused qkv buffer.  share_adapter: one LA_in (G = 1) and
     the fused QKV GEMM.  Head-shifted attention.  x'1 = x' + out_proj(LA_out(attn)): a G = 1 call and the out_proj GEMM with
     the residual epilogue.  No S_Adapter, no DropPath, no adapter scale.
  3. xn = ln_2(x1); m = mlp(xn + LA_in(xn)): ``aim_lowrank_fwd`` with alpha = 2 (the reference adds the adapter's input to an
     adapter that already carries its skip), c_fc with QuickGELU, c_proj to bf16.
  4. x2 = x1 + m + LA_out(m) = x1 + 2 m + ...: ``aim_lowrank_fwd`` with alpha = 2 in its fp32 form, the residual added in fp32.

Rounding points beyond those of the other blocks: every adapter's H (bf16, read rounded by its second product), the adapters'
outputs Y (bf16 operands of the projection behind them), and m (bf16: it is the input of MLP_Adapter_out).

Backward, per adapter: ``aim_lowrank_bwd`` turns the gradient(s) of Y into dH and the input gradient; dW2 += dY^T H with
db2 += sum dY, and dW1 += dH^T X with db1 += sum dH, go through ``ops.wgrad`` on the detached stream.  The q, k, v dgrads read
column slabs of dqkv and slabs of W_qkv^T.  Row 1 of every frame is the dead slot of zeroi2v.py: its gradient row is zero, so
every sum over rows gets exactly zero from it.
"""
from types import SimpleNamespace
from typing import Dict, Optional

import torch
from torch import nn

from . import ops
from .backbone import _AUX_GRAD, _DP_RESERVE, BF16, F32, _AdapterW, _cast, _empty, _Fork, _wgrads_beside

MAX_BOTTLENECK = 256          # aim_lowrank_fwd / _bwd: r a multiple of 8, at most 256


class Linear_Adapter(nn.Module):
    """Parameters of one linear adapter (reference ``Linear_Adapter``, :15-38; its own ``init_weights`` is never called)."""

    def __init__(self, D_features: int, bottleneck: int = 196):
        super().__init__()
        self.D_fc1 = nn.Linear(D_features, bottleneck)
        self.D_fc2 = nn.Linear(bottleneck, D_features)


def adapter_names(share_adapter: bool, with_t_cls_token: bool):
    """a block's adapters in the reference's construction order (:109-136)"""
    attn = ("Attn_Adapter_in",) if share_adapter else ("Attn_Adapter_q", "Attn_Adapter_k", "Attn_Adapter_v")
    return (("T_Adapter",) if with_t_cls_token else ()) + attn + ("Attn_Adapter_out", "MLP_Adapter_in", "MLP_Adapter_out")


class _FrozenLin:
    """bf16 copies (and transposes, for dgrad) of one block's frozen weights, each on its own -- the linear adapters sit in
    front of and behind the projections, nothing is concatenated -- and the persistent bf16 operand buffers of its adapters
    (``_Frozen``'s interface towards ``ViT_CLIP._stage_adapters``)."""

    def __init__(self, blk, names):
        a = blk.attn
        D = blk.ln_1.normalized_shape[0]
        dev = a.in_proj_weight.device
        self.eps, self.D = float(blk.ln_1.eps), D
        self.Wqkv, self.WqkvT = _cast(a.in_proj_weight), _cast(a.in_proj_weight, True)
        self.Wo, self.WoT = _cast(a.out_proj.weight), _cast(a.out_proj.weight, True)
        self.Wfc, self.WfcT = _cast(blk.mlp.c_fc.weight), _cast(blk.mlp.c_fc.weight, True)          # [4D, D], [D, 4D]
        self.Wpr, self.WprT = _cast(blk.mlp.c_proj.weight), _cast(blk.mlp.c_proj.weight, True)      # [D, 4D], [4D, D]
        f = lambda p: p.detach().float().contiguous()
        self.bqkv, self.bo = f(a.in_proj_bias), f(a.out_proj.bias)
        self.bfc, self.bpr = f(blk.mlp.c_fc.bias), f(blk.mlp.c_proj.bias)
        self.g1, self.b1 = f(blk.ln_1.weight), f(blk.ln_1.bias)
        self.g2, self.b2 = f(blk.ln_2.weight), f(blk.ln_2.bias)
        self.small = {}
        for n in names:
            r = getattr(blk, n).D_fc1.weight.shape[0]
            self.small[n] = dict(W1=_empty((r, D), BF16, dev), W1T=_empty((D, r), BF16, dev),
                                 W2=_empty((D, r), BF16, dev), W2T=_empty((r, D), BF16, dev))

    def cast_entries(self, name, w1, w2, b1=None):
        b = self.small[name]
        return [(w1, b["W1"], False), (w1, b["W1T"], True), (w2, b["W2"], False), (w2, b["W2T"], True)]


def _la_forward(x, ad: _AdapterW, save: bool, alpha: float = 1.0, y32=None, resid=None):
    """one linear adapter on x [M, D] bf16 -> (Y bf16, or None in the fp32 form; H, or None when nothing will read it)"""
    M, D = x.shape
    h = _empty((M, ad.W1.shape[0]), BF16, x.device) if save else None
    y = _empty((M, D), BF16, x.device) if y32 is None else None
    ops.lowrank_fwd(x, [ad.W1], [ad.b1], [ad.W2], [ad.b2], h=[h], y=[y], alpha=alpha, y32=y32, resid=resid)
    return y, h


def _la_backward(dy, ad: _AdapterW, h, x, g, later: list, alpha: float = 1.0):
    """backward of one linear adapter: returns d(x) bf16; queues dW2 += dy^T h, db2 += sum dy, dW1 += dh^T x, db1 += sum dh"""
    M, D = dy.shape
    dh = _empty((M, ad.W1.shape[0]), BF16, dy.device)
    dx = _empty((M, D), BF16, dy.device)
    ops.lowrank_bwd([dy], [ad.W2T], [ad.W1T], [dh], dx, alpha=alpha)
    later.append(lambda: ops.wgrad(dy, h, g["D_fc2.weight"], g["D_fc2.bias"]))
    later.append(lambda: ops.wgrad(dh, x, g["D_fc1.weight"], g["D_fc1.bias"]))
    return dx


def block_forward(x, fz: _FrozenLin, adp: Dict[str, _AdapterW], B, T, P, H, tcls: bool, share: bool, shifts, save: bool,
                  cls_forward):
    """x [B*T*P, D] f32 (row 1 of every frame: the slot of the temporal class token) -> x2, ctx"""
    dev = x.device
    M, D = x.shape
    BT = B * T
    c: dict = {}
    if tcls:
        c.update(cls_forward(x, fz, adp["T_Adapter"], B, T, P, H))
    xl = _empty((M, D), BF16, dev)
    mean1, rstd1 = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x, fz.g1, fz.b1, M, D, D, y_bf16=xl, mean=mean1, rstd=rstd1)
    qkv = _empty((M, 3 * D), BF16, dev)
    if share:
        y_in, h_in = _la_forward(xl, adp["Attn_Adapter_in"], save)
        ops.gemm(y_in, fz.Wqkv, ops.EPI_BF16, qkv, bias=fz.bqkv)
        del y_in
    else:
        ads = [adp["Attn_Adapter_" + n] for n in "qkv"]
        r = ads[0].W1.shape[0]
        ycat = _empty((M, 3 * D), BF16, dev)
        h_in = _empty((M, 3 * r), BF16, dev) if save else None
        ops.lowrank_fwd(xl, [a.W1 for a in ads], [a.b1 for a in ads], [a.W2 for a in ads], [a.b2 for a in ads],
                        h=[h_in[:, g * r:(g + 1) * r] for g in range(3)] if save else None,
                        y=[ycat[:, g * D:(g + 1) * D] for g in range(3)])
        for g in range(3):
            s = slice(g * D, (g + 1) * D)
            ops.gemm(ycat[:, s], fz.Wqkv[s], ops.EPI_BF16, qkv[:, s], bias=fz.bqkv[s])
        del ycat
    ao = _empty((M, D), BF16, dev)
    lse = _empty((BT, H, P), F32, dev)
    ops.attn_fwd_shift(qkv, ao, lse, B, T, P, H, shifts)
    y_o, h_o = _la_forward(ao, adp["Attn_Adapter_out"], save)
    x1 = _empty((M, D), F32, dev)
    ops.gemm(y_o, fz.Wo, ops.EPI_F32, x1, bias=fz.bo, resid=x)
    del y_o
    xn = _empty((M, D), BF16, dev)
    mean2, rstd2 = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x1, fz.g2, fz.b2, M, D, D, y_bf16=xn, mean=mean2, rstd=rstd2)
    y_mi, h_mi = _la_forward(xn, adp["MLP_Adapter_in"], save, alpha=2.0)
    hid = _empty((M, 4 * D), BF16, dev)
    pre = _empty((M, 4 * D), BF16, dev) if (save or M < 1024) else None          # (the small-M kernels always store it)
    ops.gemm(y_mi, fz.Wfc, ops.EPI_ACT, hid, bias=fz.bfc, out2=pre, act=ops.ACT_QGELU, aux_grad=_AUX_GRAD)
    del y_mi
    mm = _empty((M, D), BF16, dev)
    ops.gemm(hid, fz.Wpr, ops.EPI_BF16, mm, bias=fz.bpr)
    del hid
    x2 = _empty((M, D), F32, dev)
    _, h_mo = _la_forward(mm, adp["MLP_Adapter_out"], save, alpha=2.0, y32=x2, resid=x1)
    if not save:
        return x2, None
    c.update(x=x, xl=xl, mean1=mean1, rstd1=rstd1, qkv=qkv, ao=ao, lse=lse, h_in=h_in, h_o=h_o, x1=x1, mean2=mean2,
             rstd2=rstd2, xn=xn, h_mi=h_mi, pre=pre, mm=mm, h_mo=h_mo)
    return x2, c


def block_backward(dyb, c, fz: _FrozenLin, adp: Dict[str, _AdapterW], grads, B, T, P, H, tcls: bool, share: bool, shifts,
                   keep: Optional[list], cls_backward):
    """dyb = d(loss)/d(x2) [M, D] bf16 with a zero row 1 in every frame (tcls) -> d(loss)/d(x) with the same property; the
    adapters' gradients are accumulated into ``grads``."""
    dev = dyb.device
    M, D = dyb.shape
    BT = B * T
    fork = _Fork(dev, "bwd")
    later: list = []
    # ---- x2 = x1 + 2 m + ...;  m = c_proj(QuickGELU(c_fc(2 xn + ...)))
    dm = _la_backward(dyb, adp["MLP_Adapter_out"], c["h_mo"], c["mm"], grads["MLP_Adapter_out"], later, alpha=2.0)
    dpre = _empty((M, 4 * D), BF16, dev)
    ops.gemm(dm, fz.WprT, ops.EPI_DACT, dpre, aux=c["pre"], act=ops.ACT_QGELU, aux_grad=_AUX_GRAD, reserve_cus=_DP_RESERVE)
    del dm
    dy_mi = _empty((M, D), BF16, dev)
    ops.gemm(dpre, fz.WfcT, ops.EPI_BF16, dy_mi, reserve_cus=_DP_RESERVE)
    del dpre
    dxn = _la_backward(dy_mi, adp["MLP_Adapter_in"], c["h_mi"], c["xn"], grads["MLP_Adapter_in"], later, alpha=2.0)
    dx1b = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxn, c["x1"], fz.g2, c["mean2"], c["rstd2"], M, D, lddy=D, ldx=D, lddx=D, dres=dyb, dx_bf16=dx1b)
    del dxn
    # ---- x'1 = x' + out_proj(LA_out(attn))
    dy_o = _empty((M, D), BF16, dev)
    ops.gemm(dx1b, fz.WoT, ops.EPI_BF16, dy_o, reserve_cus=_DP_RESERVE)
    dao = _la_backward(dy_o, adp["Attn_Adapter_out"], c["h_o"], c["ao"], grads["Attn_Adapter_out"], later)
    dqkv = _empty((M, 3 * D), BF16, dev)
    delta = _empty((BT, H, P), F32, dev)
    ops.attn_bwd_shift(c["qkv"], c["ao"], dao, c["lse"], delta, dqkv, B, T, P, H, shifts)
    del dao
    # ---- q, k, v = in_proj slabs of LA_{q,k,v}(xln)
    xl, h_in = c["xl"], c["h_in"]
    if share:
        dy_in = _empty((M, D), BF16, dev)
        ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dy_in, reserve_cus=_DP_RESERVE)
        dxl = _la_backward(dy_in, adp["Attn_Adapter_in"], h_in, xl, grads["Attn_Adapter_in"], later)
    else:
        ads = [adp["Attn_Adapter_" + n] for n in "qkv"]
        r = ads[0].W1.shape[0]
        dycat = _empty((M, 3 * D), BF16, dev)
        for g in range(3):
            s = slice(g * D, (g + 1) * D)
            ops.gemm(dqkv[:, s], fz.WqkvT[:, s], ops.EPI_BF16, dycat[:, s], reserve_cus=_DP_RESERVE)
        dhcat = _empty((M, 3 * r), BF16, dev)
        dxl = _empty((M, D), BF16, dev)
        ops.lowrank_bwd([dycat[:, g * D:(g + 1) * D] for g in range(3)], [a.W2T for a in ads], [a.W1T for a in ads],
                        [dhcat[:, g * r:(g + 1) * r] for g in range(3)], dxl)
        for g, n in enumerate("qkv"):
            gg = grads["Attn_Adapter_" + n]
            dy_g, h_g, dh_g = dycat[:, g * D:(g + 1) * D], h_in[:, g * r:(g + 1) * r], dhcat[:, g * r:(g + 1) * r]
            later.append(lambda dy_g=dy_g, h_g=h_g, gg=gg: ops.wgrad(dy_g, h_g, gg["D_fc2.weight"], gg["D_fc2.bias"]))
            later.append(lambda dh_g=dh_g, gg=gg: ops.wgrad(dh_g, xl, gg["D_fc1.weight"], gg["D_fc1.bias"]))
    del dqkv
    if tcls:
        cls_backward(dxl, c, fz, adp["T_Adapter"], grads["T_Adapter"], later, B, T, P, H)
    dxb = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl, c["x"], fz.g1, c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dx1b, dx_bf16=dxb)
    if tcls:
        dxb.view(BT, P, D)[:, 1].zero_()             # the slot belongs to this block: nothing flows further down through it
    _wgrads_beside(fork, later, keep)
    return dxb


# ----------------------------------------------------------------------------------------------
# merging: the adapters folded into the frozen weights
# ----------------------------------------------------------------------------------------------
def fold_block(blk, share: bool, tcls: bool) -> SimpleNamespace:
    """The merged operands of one block, from the fp32 parameters: with A = c I + W2 W1 and d = W2 b1 + b2 (c = 1 for the
    attention adapters, 2 for the two MLP adapters)  W_{q,k,v}' = W A, b' = b + W d;  W_o' = W_o A, b_o' = b_o + W_o d;
    W_fc' = W_fc A, b_fc' = b_fc + W_fc d;  W_proj' = A W_proj, b_proj' = A b_proj + d.  Products in fp64, then one rounding
    of every weight to bf16 (biases stay fp32).  Plain torch: 6 small products per block, once per change of an adapter."""
    d = lambda t: t.detach().double()

    def pair(ad, c):
        W1, b1, W2, b2 = d(ad.D_fc1.weight), d(ad.D_fc1.bias), d(ad.D_fc2.weight), d(ad.D_fc2.bias)
        return c * torch.eye(W2.shape[0], dtype=torch.float64, device=W2.device) + W2 @ W1, W2 @ b1 + b2

    w16 = lambda t: t.float().to(BF16).contiguous()
    f32 = lambda t: t.float().contiguous()
    W, b = d(blk.attn.in_proj_weight), d(blk.attn.in_proj_bias)
    D = W.shape[1]
    Ws, bs = [], []
    for j, n in enumerate("qkv"):
        A, dd = pair(getattr(blk, "Attn_Adapter_in" if share else "Attn_Adapter_" + n), 1.0)
        Wj, bj = W[j * D:(j + 1) * D], b[j * D:(j + 1) * D]
        Ws.append(Wj @ A)
        bs.append(bj + Wj @ dd)
    out = SimpleNamespace(Wqkv=w16(torch.cat(Ws)), bqkv=f32(torch.cat(bs)))
    A, dd = pair(blk.Attn_Adapter_out, 1.0)
    Wo, bo = d(blk.attn.out_proj.weight), d(blk.attn.out_proj.bias)
    out.Wo, out.bo = w16(Wo @ A), f32(bo + Wo @ dd)
    A, dd = pair(blk.MLP_Adapter_in, 2.0)
    Wf, bf = d(blk.mlp.c_fc.weight), d(blk.mlp.c_fc.bias)
    out.Wfc, out.bfc = w16(Wf @ A), f32(bf + Wf @ dd)
    A, dd = pair(blk.MLP_Adapter_out, 2.0)
    Wp, bp = d(blk.mlp.c_proj.weight), d(blk.mlp.c_proj.bias)
    out.Wpr, out.bpr = w16(A @ Wp), f32(A @ bp + dd)
    if tcls:            # the T_Adapter is not folded (GELU): its operands, staged here so that a merged forward casts nothing
        t = blk.T_Adapter
        out.tad = SimpleNamespace(W1=w16(d(t.D_fc1.weight)), b1=f32(t.D_fc1.bias.detach()), W2=w16(d(t.D_fc2.weight)),
                                  b2=f32(t.D_fc2.bias.detach()))
    return out


def merged_block_forward(x, fz: _FrozenLin, mg: SimpleNamespace, B, T, P, H, tcls: bool, shifts, cls_forward):
    """the block on the folded weights: no adapter work at all.  The class chain keeps the ORIGINAL in_proj / out_proj."""
    dev = x.device
    M, D = x.shape
    BT = B * T
    if tcls:
        cls_forward(x, fz, mg.tad, B, T, P, H)
    xl = _empty((M, D), BF16, dev)
    ops.layernorm_fwd(x, fz.g1, fz.b1, M, D, D, y_bf16=xl)
    qkv = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl, mg.Wqkv, ops.EPI_BF16, qkv, bias=mg.bqkv)
    ao = _empty((M, D), BF16, dev)
    ops.attn_fwd_shift(qkv, ao, _empty((BT, H, P), F32, dev), B, T, P, H, shifts)
    x1 = _empty((M, D), F32, dev)
    ops.gemm(ao, mg.Wo, ops.EPI_F32, x1, bias=mg.bo, resid=x)
    xn = _empty((M, D), BF16, dev)
    ops.layernorm_fwd(x1, fz.g2, fz.b2, M, D, D, y_bf16=xn)
    hid = _empty((M, 4 * D), BF16, dev)
    pre = _empty((M, 4 * D), BF16, dev) if M < 1024 else None                  # (the small-M kernels always store it)
    ops.gemm(xn, mg.Wfc, ops.EPI_ACT, hid, bias=mg.bfc, out2=pre, act=ops.ACT_QGELU, aux_grad=_AUX_GRAD)
    x2 = _empty((M, D), F32, dev)
    ops.gemm(hid, mg.Wpr, ops.EPI_F32, x2, bias=mg.bpr, resid=x1)
    return x2
