"""Stock-AIM backbone (``AIM``) on the HIP kernels: the published AIM model (README accuracy table), SURVEY section 8f-4.

Drop-in for ``mmaction/models/backbones/vitclip_aim.py:353-493`` (class ``AIM``) with ``wind_attn=False`` and
``num_tadapter=1`` -- the block at ``:195-211``:

    xt = T_Adapter(attention(ln_1('n (b t) d -> t (b n) d' x)))     temporal attention over the T frames of EVERY token
    x  = x + drop_path(xt)                                           (batch B*N; T_Adapter skip_connect=False)
    x  = x + S_Adapter(attention(ln_1(x)))                           S_Adapter skip_connect=True: y + fc2(gelu(fc1(y)))
    x  = x + mlp(ln_2(x)) + drop_path(scale * MLP_Adapter(ln_2(x)))  (same joint adaptation as vit_clip.py:285-286)

Same parameter names / shapes, same ``init_weights`` policy, same embedding and class-token readout as ``ViT_CLIP``
(``vitclip_aim.py:468-493`` restates ``vit_clip.py:433-458``), so it subclasses it; only the block's forward and its
hand-written backward differ.  Every GEMM here has M = B*T*N rows (persistent 256x256 kernel); the temporal attention is
``aim_tattn_fwd/bwd`` (csrc/tattn.hip), which reads the frame-major fused qkv buffer in place instead of rearranging the
activations twice as the reference does.  A no-grad forward uses ``aim_tattn_fwd_infer`` (no stored probabilities, same bits),
and with ``set_inference_precision('fp8')`` and at least 1024 token rows the block's six large GEMMs run on fp8 e4m3 operands
(``_aim_block_forward_f8``).

The window-attention branch (``wind_attn=True``, ``:212-287``, what the reference's two ``AIM`` recipes set together with
``not_shift=False``) is the second half of this file: per block, N = G G + 1 tokens per frame, d1 d2 the block's DropPath
draws over the N token positions,

  1. xl = ln_1(x), qkv = xl Wqkv^T + b over ALL rows (ln_1 and the projection are token-wise: one pass serves 2 and 3)
  2. patch tokens: attention inside 3-D windows of the [T, G, G] grid.  Even blocks: the (wt, wh, ww) windows,
     ``aim_win_attn_fwd``.  Odd blocks: the reference rolls the grid by minus the shift, attends inside whole windows of the
     rolled grid under an additive -100 mask between the regions ``compute_mask`` numbers (:62-75, :180-187) and rolls back.
     In the ORIGINAL coordinates that is plain attention inside boxes: every axis, t included, cut at 0, s, s + w, s + 2 w, ...
     with nothing wrapping -- ``aim_win_attn_fwd_cut`` (AIM_FLASH's strips keep whole t windows that wrap, aim_flash.py).
     A masked pair gets a weight of exactly 0 here and at most (S - 1) e^(spread - 100) in the reference.
  3. class tokens: attention over the T class tokens of each clip -- ``aim_cls_attn_fwd`` on the same buffer
  4. ta = [3 | 2] Wo^T + bo;  x1 = x + d1[token] T_Adapter(ta)      (no adapter scale, as in the stock block)
  5. (prompt) ta's class row becomes one more token of its frame; x2 = x' + S_Adapter(attention(ln_1 x')) with S_Adapter's
     skip connection and no DropPath, exactly the stock block's spatial step at N + 1 tokens; the prompt token is dropped
  6. x3 = x2 + mlp(ln_2 x2) + d2[token] scale MLP_Adapter(ln_2 x2)      (``_mlp_adapter_forward``)

The prompt lives as in aim_flash_win.py: the residual stream keeps P = N + 1 rows per frame, the extra row is a slot BEHIND
the frame's tokens, filled in step 5, dead after step 6, and its gradient row returns through the class rows of ``ta``.

Steps 1-3, the out-projection of 4 and the slot layout are win_block.py's, shared with aim_flash_win.py; T_Adapter under the
first DropPath and the spatial step are ``_t_adapter_*`` and ``_spatial_*`` below, shared by the stock and the windowed block.
"""
import logging
from typing import Dict, List, Optional

import torch

from . import ops
from .backbone import (BF16, F32, ViT_CLIP, _AdapterW, _embed_backward, _embed_forward, _empty, _Fork, _Frozen, _Frozen8, _GradBufs,
                       _ln_post_backward, _ln_post_forward, _mlp_adapter_backward, _mlp_adapter_forward,
                       _mlp_adapter_forward_f8, _wgrads_beside)
from .registry import BACKBONES
from .win_block import (check_win_clip, check_window, clip_shift, clip_window, from_slot_layout, to_slot_layout, win_prompt_grad,
                        win_temporal_backward, win_temporal_forward)

_LOG = logging.getLogger("aim_amd")


def _t_adapter_forward(ta, x, tad: _AdapterW, dp1, ntok, r):
    """x1 = x + dp1[token] T_Adapter(ta) (no adapter scale, no skip) -> t_pre, t_hs, x1.  The DropPath factor is folded into
    the stored activation (t_hs = dp1 * GELU(pre)), so the D_fc2 weight gradient is a plain product and the bias rides along
    token-scaled as `vec`."""
    M, D = x.shape
    t_pre, t_hs = _empty((M, r), BF16, x.device), _empty((M, r), BF16, x.device)
    ops.gemm(ta, tad.W1, ops.EPI_ACT, t_hs, bias=tad.b1, out2=t_pre, act=ops.ACT_GELU, at=dp1, ntok=ntok)
    x1 = _empty((M, D), F32, x.device)
    ops.gemm(t_hs, tad.W2, ops.EPI_F32, x1, resid=x, vec=tad.b2.reshape(1, -1), ldv=0, bt=dp1, ntok=ntok)
    return t_pre, t_hs, x1


def _t_adapter_backward(dx1b, c, tad: _AdapterW, gT, later, ntok, r):
    """x1 = x + t_hs W2^T + dp1[tok] b2,  t_hs = dp1[tok] GELU(ta W1^T + b1):  d(loss)/d(x1) -> d(loss)/d(ta)"""
    M, D = dx1b.shape
    t_hs, t_pre, ta, dp1 = c["t_hs"], c["t_pre"], c["ta"], c["dp1"]
    later.append(lambda: ops.wgrad(dx1b, t_hs, gT["D_fc2.weight"], gT["D_fc2.bias"], at=dp1, ntok=ntok))
    dth_pre = _empty((M, r), BF16, dx1b.device)
    ops.gemm(dx1b, tad.W2T, ops.EPI_DACT, dth_pre, aux=t_pre, act=ops.ACT_GELU, at=dp1, ntok=ntok)
    later.append(lambda: ops.wgrad(dth_pre, ta, gT["D_fc1.weight"], gT["D_fc1.bias"]))
    dta = _empty((M, D), BF16, dx1b.device)
    ops.gemm(dth_pre, tad.W1T, ops.EPI_BF16, dta)
    return dta


def _spatial_forward(x1, fz: _Frozen, sad: _AdapterW, BT, n, H, r):
    """spatial adaptation over the n token rows of a frame: ln_1 -> QKV -> attention over tokens -> out_proj -> S_Adapter
    (with skip) -> x2, and what the backward reads"""
    dev = x1.device
    M, D = x1.shape
    xl2 = _empty((M, D), BF16, dev)
    mean1b, rstd1b = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x1, fz.g1, fz.b1, M, D, D, y_bf16=xl2, mean=mean1b, rstd=rstd1b)
    qkv2 = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl2, fz.Wqkv, ops.EPI_BF16, qkv2, bias=fz.bqkv)
    del xl2
    ao = _empty((M, D), BF16, dev)
    lse = _empty((BT, H, n), F32, dev)
    ops.attn_fwd(qkv2, ao, lse, BT, n, H)
    sa = _empty((M, D), BF16, dev)
    ops.gemm(ao, fz.Wo, ops.EPI_BF16, sa, bias=fz.bo)
    s_pre, s_h = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(sa, sad.W1, ops.EPI_ACT, s_h, bias=sad.b1, out2=s_pre, act=ops.ACT_GELU)
    x2 = _empty((M, D), F32, dev)
    ops.gemm(s_h, sad.W2, ops.EPI_F32, x2, bias=sad.b2, resid=x1)      # x1 + D_fc2(GELU(D_fc1(sa)))
    ops.acc_bf16(x2, sa)                                                # + sa: the adapter's skip connection
    return x2, dict(x1=x1, mean1b=mean1b, rstd1b=rstd1b, qkv2=qkv2, ao=ao, lse=lse, sa=sa, s_pre=s_pre, s_h=s_h)


def _spatial_backward(dx2b, c, fz: _Frozen, sad: _AdapterW, gS, later, BT, n, H, r):
    """x2 = x1 + sa + (s_h W2^T + b2),  s_h = GELU(sa W1^T + b1),  sa = ao Wo^T + bo:  d(loss)/d(x2) -> d(loss)/d(x1), and the
    d(qkv), delta and dxl buffers for the temporal step to overwrite"""
    dev = dx2b.device
    M, D = dx2b.shape
    s_h, s_pre, sa = c["s_h"], c["s_pre"], c["sa"]
    later.append(lambda: ops.wgrad(dx2b, s_h, gS["D_fc2.weight"], gS["D_fc2.bias"]))
    dsh_pre = _empty((M, r), BF16, dev)
    ops.gemm(dx2b, sad.W2T, ops.EPI_DACT, dsh_pre, aux=s_pre, act=ops.ACT_GELU)
    later.append(lambda: ops.wgrad(dsh_pre, sa, gS["D_fc1.weight"], gS["D_fc1.bias"]))
    dsa = _empty((M, D), BF16, dev)
    ops.gemm(dsh_pre, sad.W1T, ops.EPI_BF16, dsa)
    ops.add_bf16(dsa, dx2b, dsa)                     # + the skip connection's share
    dao = _empty((M, D), BF16, dev)
    ops.gemm(dsa, fz.WoT, ops.EPI_BF16, dao)
    del dsa
    dqkv = _empty((M, 3 * D), BF16, dev)
    delta = _empty((BT, H, n), F32, dev)
    ops.attn_bwd(c["qkv2"], c["ao"], dao, c["lse"], delta, dqkv, BT, n, H)
    del dao
    dxl = _empty((M, D), BF16, dev)
    ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dxl)
    dx1b = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl, c["x1"], fz.g1, c["mean1b"], c["rstd1b"], M, D, lddy=D, ldx=D, lddx=D, dres=dx2b, dx_bf16=dx1b)
    return dx1b, dqkv, delta, dxl


def _aim_block_forward_f8(x, fz: _Frozen, f8: _Frozen8, adp: Dict[str, _AdapterW], B, T, N, H, dp1, dms2):
    """The stock block's forward on fp8 e4m3 operands (inference, M >= 1024): the QKV projection (twice), both out_proj GEMMs
    and the MLP pair run ``aim_gemm_fp8``; their A operands are written as fp8 by the producing kernel -- ln_1 / ln_2, the
    temporal attention (``tattn_fwd_infer``), the spatial attention, the [c_fc ; D_fc1] epilogue.  ``qkv``, ``ta`` and ``sa``
    are bf16, T_Adapter and S_Adapter stay on the bf16 GEMMs, the residual stream stays fp32.  No context is kept."""
    dev = x.device
    M, D = x.shape
    BT, r = B * T, fz.r
    tad, sad = adp["T_Adapter"], adp["S_Adapter"]
    # a forward without a backward has no reader for the adapters' pre-activations: the large-tile GEMM drops the stores of
    # an absent `out2`; an adapter too narrow for that kernel writes into a scratch buffer
    pre = None if (r >= 64 and r % 8 == 0) else _empty((M, r), BF16, dev)
    # ---- temporal adaptation
    xl = _empty((M, D), ops.FP8, dev)
    ops.layernorm_fwd_fp8(x, fz.g1, fz.b1, M, D, D, xl)
    qkv = _empty((M, 3 * D), BF16, dev)
    ops.gemm_fp8(xl, f8.Wqkv, f8.sqkv, ops.EPI_BF16, qkv, bias=fz.bqkv)
    ot = _empty((M, D), ops.FP8, dev)
    ops.tattn_fwd_infer(qkv, ot, B, T, N, H)
    ta = _empty((M, D), BF16, dev)
    ops.gemm_fp8(ot, f8.Wo, f8.so, ops.EPI_BF16, ta, bias=fz.bo)
    del ot
    t_hs = _empty((M, r), BF16, dev)
    ops.gemm(ta, tad.W1, ops.EPI_ACT, t_hs, bias=tad.b1, out2=pre, act=ops.ACT_GELU, at=dp1, ntok=N)
    x1 = _empty((M, D), F32, dev)
    ops.gemm(t_hs, tad.W2, ops.EPI_F32, x1, resid=x, vec=tad.b2.reshape(1, -1), ldv=0, bt=dp1, ntok=N)
    del ta
    # ---- spatial adaptation (the ln_1 and QKV buffers serve again)
    ops.layernorm_fwd_fp8(x1, fz.g1, fz.b1, M, D, D, xl)
    ops.gemm_fp8(xl, f8.Wqkv, f8.sqkv, ops.EPI_BF16, qkv, bias=fz.bqkv)
    ao = _empty((M, D), ops.FP8, dev)
    ops.attn_fwd_fp8(qkv, ao, BT, N, H)
    sa = _empty((M, D), BF16, dev)
    ops.gemm_fp8(ao, f8.Wo, f8.so, ops.EPI_BF16, sa, bias=fz.bo)
    del ao, xl, qkv
    ops.gemm(sa, sad.W1, ops.EPI_ACT, t_hs, bias=sad.b1, out2=pre, act=ops.ACT_GELU)
    x2 = _empty((M, D), F32, dev)
    ops.gemm(t_hs, sad.W2, ops.EPI_F32, x2, bias=sad.b2, resid=x1)      # x1 + D_fc2(GELU(D_fc1(sa)))
    ops.acc_bf16(x2, sa)                                                # + sa: the adapter's skip connection
    # ---- joint adaptation (shared with the vit_clip block)
    return _mlp_adapter_forward_f8(x2, fz, f8, dms2, N)


def aim_block_forward(x, fz: _Frozen, adp: Dict[str, _AdapterW], B, T, N, H, dp1, dms2, save: bool,
                      f8: Optional[_Frozen8] = None, infer: bool = False):
    """x: [B*T*N, D] f32 frame-major -> x3.  ``dp1``: the first DropPath factor per token (no adapter scale,
    vitclip_aim.py:205); ``dms2``: the second one times ``scale`` (:210).  ``infer`` (a no-grad forward; ``save`` must be
    False): the temporal attention stores no probabilities -- same bits.  ``f8`` (with ``infer``): the block's fp8 operands,
    and the large GEMMs run on them (``_aim_block_forward_f8``)."""
    assert not (save and (infer or f8 is not None))
    if f8 is not None:
        return _aim_block_forward_f8(x, fz, f8, adp, B, T, N, H, dp1, dms2), None
    dev = x.device
    M, D = x.shape
    BT, r = B * T, fz.r
    # ---- temporal adaptation: ln_1 -> QKV -> attention over frames -> out_proj -> T_Adapter -> + drop_path
    xl = _empty((M, D), BF16, dev)
    mean1, rstd1 = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x, fz.g1, fz.b1, M, D, D, y_bf16=xl, mean=mean1, rstd=rstd1)
    qkv_t = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl, fz.Wqkv, ops.EPI_BF16, qkv_t, bias=fz.bqkv)
    ot = _empty((M, D), BF16, dev)
    if infer:                           # no backward will read the probabilities: the form that does not store them
        probs = None
        ops.tattn_fwd_infer(qkv_t, ot, B, T, N, H)
    else:
        probs = _empty((B * N, H, T, T), F32, dev)
        ops.tattn_fwd(qkv_t, ot, probs, B, T, N, H)
    ta = _empty((M, D), BF16, dev)
    ops.gemm(ot, fz.Wo, ops.EPI_BF16, ta, bias=fz.bo)
    del ot, xl
    t_pre, t_hs, x1 = _t_adapter_forward(ta, x, adp["T_Adapter"], dp1, N, r)
    # ---- spatial adaptation
    x2, c = _spatial_forward(x1, fz, adp["S_Adapter"], BT, N, H, r)
    # ---- joint adaptation (shared with the vit_clip block)
    x3, xn, mean2, rstd2, hcat_pre, a_s = _mlp_adapter_forward(x2, fz, dms2, N, save)
    if not save:
        return x3, None
    c.update(x=x, mean1=mean1, rstd1=rstd1, qkv_t=qkv_t, probs=probs, ta=ta, t_pre=t_pre, t_hs=t_hs, x2=x2, mean2=mean2,
             rstd2=rstd2, xn=xn, hcat_pre=hcat_pre, a_s=a_s, dp1=dp1, dms2=dms2)
    return x3, c


def aim_block_backward(dyb, c, fz: _Frozen, adp: Dict[str, _AdapterW], grads, B, T, N, H, keep: Optional[list] = None):
    """dyb = d(loss)/d(x3) [M, D] bf16 -> d(loss)/d(x) bf16; the 12 adapter gradients are accumulated into ``grads``
    (their kernels run on the detached stream, joined at the end of the backward)."""
    dev = dyb.device
    M, D = dyb.shape
    BT, r = B * T, fz.r
    dx2b, later = _mlp_adapter_backward(dyb, c["x2"], c["mean2"], c["rstd2"], c["xn"], c["hcat_pre"], c["a_s"], c["dms2"],
                                        fz, grads["MLP_Adapter"], N)
    dx1b, dqkv = _spatial_backward(dx2b, c, fz, adp["S_Adapter"], grads["S_Adapter"], later, BT, N, H, r)[:2]
    # ---- ta = attention_T(ln_1(x)) Wo^T + bo
    dta = _t_adapter_backward(dx1b, c, adp["T_Adapter"], grads["T_Adapter"], later, N, r)
    dot = _empty((M, D), BF16, dev)
    ops.gemm(dta, fz.WoT, ops.EPI_BF16, dot)
    del dta
    ops.tattn_bwd(c["qkv_t"], c["probs"], dot, dqkv, B, T, N, H)      # (re-uses the spatial branch's d(qkv) buffer)
    del dot
    dxl = _empty((M, D), BF16, dev)     # not the spatial step's: held across the stretch above it would add to the step's peak
    ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dxl)
    del dqkv
    dxb = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl, c["x"], fz.g1, c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dx1b, dx_bf16=dxb)
    # the six weight gradients + bias column sums: off the gradient path, on the detached stream behind the main stream's
    # work so far (``keep`` None, stand-alone use: inline, complete when this function returns)
    _wgrads_beside(_Fork(dev, "aim-bwd"), later, keep)
    return dxb


def aim_win_block_forward(x, fz: _Frozen, adp: Dict[str, _AdapterW], B, T, N, P, H, window, shift, dp1, dms2, save: bool):
    """x [B*T*P, D] f32 (P = N + 1 with the prompt: row N of every frame is its slot) -> x3, ctx.  ``dp1``, ``dms2`` [P]: the
    two DropPath factors per token position (``dms2`` times the adapter scale; 0 at the slot).  ``shift``: None (plain windows)
    or the (st, sh, sw) at which every axis of this block's windows is cut."""
    BT, r = B * T, fz.r
    # ---- 1, 2, 3 and out_proj (win_block.py)
    ta, c = win_temporal_forward(x, fz, B, T, N, P, H, window, shift, True)
    # ---- 4: T_Adapter under the first DropPath
    t_pre, t_hs, x1 = _t_adapter_forward(ta, x, adp["T_Adapter"], dp1, P, r)
    # ---- 5: the prompt token, then the stock block's spatial step over the P tokens of a frame
    if P != N:
        x1.view(BT, P, -1)[:, N] = ta.view(BT, P, -1)[:, 0]
    x2, cs = _spatial_forward(x1, fz, adp["S_Adapter"], BT, P, H, r)
    # ---- 6: joint adaptation
    x3, xn, mean2, rstd2, hcat_pre, a_s = _mlp_adapter_forward(x2, fz, dms2, P, save)
    if not save:
        return x3, None
    c.update(cs, x=x, ta=ta, t_pre=t_pre, t_hs=t_hs, x2=x2, mean2=mean2, rstd2=rstd2, xn=xn, hcat_pre=hcat_pre, a_s=a_s,
             dp1=dp1, dms2=dms2)
    return x3, c


def aim_win_block_backward(dyb, c, fz: _Frozen, adp: Dict[str, _AdapterW], grads, B, T, N, P, H, window, shift,
                           keep: Optional[list]):
    """dyb = d(loss)/d(x3) [M, D] bf16 with a zero slot row in every frame -> d(loss)/d(x) with the same property; the 12
    adapter gradients are accumulated into ``grads``.  ``shift``: what the block's forward was given."""
    BT, r = B * T, fz.r
    fork = _Fork(dyb.device, "bwd")
    dx2b, later = _mlp_adapter_backward(dyb, c["x2"], c["mean2"], c["rstd2"], c["xn"], c["hcat_pre"], c["a_s"], c["dms2"],
                                        fz, grads["MLP_Adapter"], P)
    # ---- 5 (the slot's rows of dx2b are zero)
    dx1b, dqkv, delta, dxl = _spatial_backward(dx2b, c, fz, adp["S_Adapter"], grads["S_Adapter"], later, BT, P, H, r)
    dprompt = win_prompt_grad(dx1b, BT, N, P)
    # ---- 4
    dta = _t_adapter_backward(dx1b, c, adp["T_Adapter"], grads["T_Adapter"], later, P, r)
    # ---- out_proj, 3, 2, 1 (win_block.py), on the spatial step's d(qkv), delta and dxl buffers
    dxb = win_temporal_backward(dta, dx1b, c, fz, dqkv, delta, dxl, B, T, N, P, H, window, shift, True, dprompt)
    _wgrads_beside(fork, later, keep)
    return dxb


class _AimWinFn(torch.autograd.Function):
    """imgs -> [B, D, T] features of the windowed AIM.  Differentiable inputs: ``AIM._trainable_list()``."""

    @staticmethod
    def forward(ctx, model: "AIM", grad_enabled: bool, imgs: torch.Tensor, *params: torch.Tensor):
        L, H = model.layers, model.heads
        B, C, T, Hh, Ww = imgs.shape
        D, p = model.width, model.patch_size
        G = Hh // p
        N = G * G + 1
        P = N + int(model.prompt)
        BT = B * T
        dev = imgs.device
        temporal, lnp_w, lnp_b = params[0], params[1], params[2]
        need_grad = grad_enabled and any(ctx.needs_input_grad)
        frozen = model._frozen_operands()
        adp = model._stage_adapters(frozen, params)
        tok, x0, mean0, rstd0, tmp = _embed_forward(model, frozen, imgs, temporal)
        x = to_slot_layout(x0, BT, N, P)
        del x0
        if model.inference_precision == 'fp8' and not need_grad and not getattr(model, "_fp8_warned", False):
            model._fp8_warned = True
            _LOG.warning("fp8 inference was requested but this forward runs bf16: the windowed AIM variant has no fp8 path")
        masks = model._drop_masks(N, model.training, dev)            # [L, 2, N], both times the adapter scale
        if P != N:
            masks = torch.cat([masks, masks.new_zeros((L, 2, 1))], dim=2)
        window = clip_window(model.window_size, T, G)
        shifts = [model._block_shift(i, T, G) for i in range(L)]
        ctxs: List[Optional[dict]] = []
        for i in range(L):
            # the first DropPath acts on the un-scaled temporal branch (vitclip_aim.py:267)
            dp1 = (masks[i, 0] * (1.0 / float(model.transformer.resblocks[i].scale))).contiguous()
            x, c = aim_win_block_forward(x, frozen["blocks"][i], adp[i], B, T, N, P, H, window, shifts[i], dp1,
                                         masks[i, 1].contiguous(), need_grad)
            ctxs.append(c)
        y, gw, meanp, rstdp = _ln_post_forward(x, lnp_w, lnp_b, BT, P)
        if need_grad:
            ctx.model, ctx.dims = model, (B, T, N, P, H, D, L)
            ctx.saved = dict(ctxs=ctxs, adp=adp, tok=tok, mean0=mean0, rstd0=rstd0, tmp=tmp, xL=x, gw=gw, meanp=meanp,
                             rstdp=rstdp, params=params, window=window, shifts=shifts)
        return y.reshape(B, T, D).permute(0, 2, 1)      # '(b t) d -> b d t'

    @staticmethod
    def backward(ctx, dout):
        model = ctx.model
        B, T, N, P, H, D, L = ctx.dims
        s = ctx.saved
        BT = B * T
        dev = dout.device
        frozen = model._frozen_operands()
        gbufs = _GradBufs(model, s["params"], dev)
        layer_grads = gbufs.layers(L, model._adapter_names)
        dgw, dgb = gbufs.buf(1), gbufs.buf(2)
        dy = dout.permute(0, 2, 1).reshape(BT, D).contiguous().float()
        dxb = _ln_post_backward(dy, s, dgw, dgb, BT, P)
        keep: list = []
        for i in reversed(range(L)):
            dxb = aim_win_block_backward(dxb, s["ctxs"][i], frozen["blocks"][i], s["adp"][i], layer_grads[i], B, T, N, P, H,
                                         s["window"], s["shifts"][i], keep)
            s["ctxs"][i] = None
            gbufs.layer_ready(i)
        dxb = from_slot_layout(dxb, BT, N, P)
        grads = _embed_backward(gbufs, frozen, s, dxb, keep, B, T, N, D)
        ctx.saved = None
        return grads


@BACKBONES.register_module()
class AIM(ViT_CLIP):
    """Stock AIM (reference ``vitclip_aim.py:353-493``); constructor keywords of the reference class."""

    def __init__(self, input_resolution: int, num_frames: int, patch_size: int, width: int, layers: int, heads: int,
                 drop_path_rate, num_tadapter=1, adapter_scale=0.5, pretrained=None, prompt=True, wind_attn=False,
                 window_size=(32, 2, 2), not_shift=True):
        if wind_attn and not_shift:
            raise NotImplementedError("AIM(wind_attn=True, not_shift=True): the window-attention block (vitclip_aim.py:212-287) "
                                      "is built with not_shift=False, what the reference's AIM recipes set; its unshifted "
                                      "form is not built")
        if num_tadapter != 1:
            raise NotImplementedError("AIM(num_tadapter=2) (T_Adapter_in, vitclip_aim.py:201-202) is not built")
        if wind_attn:
            check_window(window_size, num_frames, input_resolution // patch_size,
                         " (the reference zero-pads such a grid; no recipe does that and it is not built)")
        super().__init__(input_resolution, num_frames, patch_size, width, layers, heads, drop_path_rate,
                         adapter_scale=adapter_scale, pretrained=pretrained)
        self.variant = 'aim'
        self.num_tadapter, self.prompt, self.wind_attn = num_tadapter, prompt, wind_attn
        if wind_attn:
            self.prompt, self.not_shift = bool(prompt), bool(not_shift)
            self.window_size = tuple(int(w) for w in window_size)
            self.variant = 'aim_win'

    def set_precision(self, precision: str):
        if self.wind_attn and precision == 'fp32':
            raise NotImplementedError("AIM(wind_attn=True) has no fp32 verification mode")
        return super().set_precision(precision)

    def _block_shift(self, i: int, T: int, G: int):
        """the (st, sh, sw) at which block i's windows are cut on a T x G x G grid, or None for plain windows: odd blocks, half
        a window, 0 where the grid does not exceed the window (the reference's ``get_window_size``, :47-60 and :304, :317)"""
        if i % 2 == 0:
            return None
        shift = clip_shift(self.window_size, T, G)
        return shift if any(shift) else None

    def forward(self, x: torch.Tensor):
        if not self.wind_attn:
            return super().forward(x)
        blend = self._take_blend_check_clip(x, "AIM")
        T, N = x.shape[2], (x.shape[3] // self.patch_size) ** 2 + 1
        check_win_clip(T, N, self.prompt)
        x = self._arm_clip(x, blend)
        y = _AimWinFn.apply(self, torch.is_grad_enabled(), x, *self._trainable_list())     # [B, D, T]
        return y.unsqueeze(-1).unsqueeze(-1)
