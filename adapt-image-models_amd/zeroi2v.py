"""``ViT_CLIP_ZEROI2V`` backbone (ZeroI2V: CLIP ViT + adapters + head-shifted spatial attention) on the HIP kernels.

Drop-in for ``mmaction/models/backbones/vit_clip_zeroI2V.py:361-509`` of the reference.  This file: the class, and the block at
``linear_adapter=False`` (what its three recipes use); the block with the linear adapters, and their fold into the frozen
weights, are in zeroi2v_linear.py.  Same registry name, constructor keywords, ``init_weights`` policy and parameter names / shapes as
``ViT_CLIP`` (``T_Adapter`` exists only with ``with_t_cls_token=True``), same ``forward(x[B,3,T,H,W]) -> [B,width,T,1,1]``.

Per block (reference ``:244-311``), frame-major rows, P = N + 1 tokens per frame with the temporal class token, else N:

  1. (with_t_cls_token) xt = T_Adapter(attention over the T class tokens of a clip(ln_1(cls))): ViT_CLIP's class-token chain
     (class-row ln_1 + QKV, ``aim_cls_attn_fwd``, out_proj, adapter).  xt becomes token 1: x' = [cls, xt, patches].
  2. xln = ln_1(x'), one QKV projection over all B T P rows.
  3. attention in which head h of frame (b, t) reads the K and V of frame (b, (t - s_h) mod T): ``aim_attn_fwd_shift`` on the
     fused qkv buffer -- the shift is the base address of the K / V staging, the reference's four clone + roll passes are gone.
  4. x'1 = x' + out_proj(attn) + dp1[n'] scale S_Adapter(x')      (S_Adapter on the residual stream itself, no skip)
  5. token 1 is dropped
  6. x2 = x1 + mlp(ln_2 x1) + dp2[n] scale MLP_Adapter(ln_2 x1)   (``_mlp_adapter_forward``, shared with ViT_CLIP)

Layout: the residual stream keeps P tokens per frame through the WHOLE stack.  Row 1 of every frame is a slot: a block's
T_Adapter GEMM writes xt straight into it (row stride P D), steps 2-4 run on all P rows, and step 6 runs on them too -- row 1
of its result is a dead value (0.5 % more rows at P = 198) that the next block overwrites.  "Dropping token 1" is then no
copy: dp2 gets a zero at position 1, and in the backward the gradient row 1 that a block hands down is zeroed once ln_1's
backward has produced it (it IS d(xt), the T_Adapter chain's input).  With a zero gradient row every weight-gradient sum,
LayerNorm backward and dgrad of the dead row contributes exactly zero.  Only the embedding (N tokens) is copied into the
P-token layout once per forward, and its gradient back once per backward.
"""
import logging
from typing import Dict, List, Optional

import torch
from torch import nn

from . import ops
from . import zeroi2v_linear as lin
from .backbone import (_AUX_GRAD, _DP_RESERVE, BF16, F32, ViT_CLIP, _AdapterW, _Arena, _embed_backward, _embed_forward, _empty,
                       _Fork, _Frozen, _GradBufs, _ln_post_backward, _ln_post_forward, _mlp_adapter_backward,
                       _mlp_adapter_forward, _wgrads_beside)
from .registry import BACKBONES

_LOG = logging.getLogger("aim_amd")

# HeadShift (reference :553-605): shift of the first heads along the clip's frames, by frames per clip; every other head, and
# every other T, is unshifted.  out[t] = in[t - s] (torch.roll).
HEAD_SHIFTS = {8: (1, -1), 16: (1, -1, 2, -2), 32: (1, -1, 2, -2, 3)}


def head_shifts(T: int, H: int):
    tab = HEAD_SHIFTS.get(T, ())
    if len(tab) > H:
        raise ValueError(f"num_frames={T} shifts heads 0..{len(tab) - 1}; the model has {H} heads")
    return tuple(tab) + (0,) * (H - len(tab))


def _cls_chain_forward(x, fz, ad, B, T, P, H):
    """The temporal class token (both adapter modes): ln_1 + QKV of the class rows, attention over the T frames of each clip,
    out_proj (the block's frozen, un-adapted ``fz.Wqkv`` / ``fz.Wo``), then the T_Adapter ``ad``, whose up-projection writes xt
    into row 1 of every frame of x.  Returns what ``_cls_chain_backward`` reads."""
    dev = x.device
    D = x.shape[1]
    BT, r = B * T, ad.W1.shape[0]
    ar = _Arena(dev, 24 * BT * D + 4 * B * H * T * T + (1 << 16))
    xl_cls = ar.take((BT, D), BF16)
    ops.layernorm_fwd(x, fz.g1, fz.b1, BT, D, P * D, y_bf16=xl_cls, mean=ar.take((BT,), F32), rstd=ar.take((BT,), F32))
    qkv_cls = ar.take((BT, 3 * D), BF16)
    ops.gemm(xl_cls, fz.Wqkv, ops.EPI_BF16, qkv_cls, bias=fz.bqkv)
    ot, probs = ar.take((BT, D), BF16), ar.take((B, H, T, T), F32)
    ops.cls_attn_fwd(qkv_cls, ot, probs, B, T, 1, H)            # "N = 1": the rows ARE the class tokens
    ta = ar.take((BT, D), BF16)
    ops.gemm(ot, fz.Wo, ops.EPI_BF16, ta, bias=fz.bo)
    t_pre, t_h = ar.take((BT, r), BF16), ar.take((BT, r), BF16)
    ops.gemm(ta, ad.W1, ops.EPI_ACT, t_h, bias=ad.b1, out2=t_pre, act=ops.ACT_GELU, aux_grad=_AUX_GRAD)
    ops.gemm(t_h, ad.W2, ops.EPI_F32, x.view(BT, P * D)[:, D:2 * D], bias=ad.b2)
    return dict(qkv_cls=qkv_cls, probs=probs, ta=ta, t_pre=t_pre, t_h=t_h)


def _cls_chain_backward(dxl, c, fz, ad, gt, later: list, B, T, P, H):
    """d(xt) = row 1 of ln_1's backward (nothing else reaches it: row 1 of d(x'1) is zero); through the T_Adapter chain it
    becomes one more gradient of the class rows' ln_1 output, added to ``dxl`` before the full-row ln_1 backward.  The
    T_Adapter's weight-gradient closures are appended to ``later``."""
    dev = dxl.device
    D = dxl.shape[1]
    BT, r = B * T, ad.W1.shape[0]
    ar = _Arena(dev, 24 * BT * D + (1 << 16))
    mean1s, rstd1s = c["mean1"].view(BT, P)[:, 1].contiguous(), c["rstd1"].view(BT, P)[:, 1].contiguous()
    dxt = ar.take((BT, D), BF16)
    ops.layernorm_bwd(dxl[1:], c["x"][1:], fz.g1, mean1s, rstd1s, BT, D, lddy=P * D, ldx=P * D, lddx=D, dx_bf16=dxt)
    t_h, ta = c["t_h"], c["ta"]
    later.append(lambda: ops.wgrad(dxt, t_h, gt["D_fc2.weight"], gt["D_fc2.bias"]))
    dtp = ar.take((BT, r), BF16)
    ops.gemm(dxt, ad.W2T, ops.EPI_DACT, dtp, aux=c["t_pre"], act=ops.ACT_GELU, aux_grad=_AUX_GRAD)
    later.append(lambda: ops.wgrad(dtp, ta, gt["D_fc1.weight"], gt["D_fc1.bias"]))
    dta = ar.take((BT, D), BF16)
    ops.gemm(dtp, ad.W1T, ops.EPI_BF16, dta)
    dot = ar.take((BT, D), BF16)
    ops.gemm(dta, fz.WoT, ops.EPI_BF16, dot)
    dqkv_cls = ar.take((BT, 3 * D), BF16)
    ops.cls_attn_bwd(c["qkv_cls"], c["probs"], dot, dqkv_cls, B, T, 1, H, compact=True)
    dxl_cls = ar.take((BT, D), F32)
    ops.gemm(dqkv_cls, fz.WqkvT, ops.EPI_F32, dxl_cls)
    ops.add_rows(dxl, P * D, dxl_cls)            # class rows: row 0 of every frame


def _block_forward(x, fz: _Frozen, adp: Dict[str, _AdapterW], B, T, P, H, tcls: bool, shifts, dms1, dms2, save: bool):
    """x [B*T*P, D] f32 (row 1 of every frame: the slot of the temporal class token) -> x2, ctx.  dms1 / dms2: [P] DropPath
    factor times adapter scale per token (dms2[1] = 0 with the slot)."""
    dev = x.device
    M, D = x.shape
    BT, r = B * T, fz.r
    c: dict = {}
    if tcls:
        c.update(_cls_chain_forward(x, fz, adp["T_Adapter"], B, T, P, H))
    # ln_1 and the QKV projection over every row
    xl = _empty((M, D), BF16, dev)
    mean1, rstd1 = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x, fz.g1, fz.b1, M, D, D, y_bf16=xl, mean=mean1, rstd=rstd1)
    qkv = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl, fz.Wqkv, ops.EPI_BF16, qkv, bias=fz.bqkv)
    del xl
    # head-shifted spatial attention: K / V of head h from frame (t - s_h) mod T of the same clip
    ao = _empty((M, D), BF16, dev)
    lse = _empty((BT, H, P), F32, dev)
    ops.attn_fwd_shift(qkv, ao, lse, B, T, P, H, shifts)
    # S_Adapter on the residual stream: s_h = dms1[tok] * GELU(x' W1^T + b1)
    sa = adp["S_Adapter"]
    xb = _empty((M, D), BF16, dev)
    ops.cast_bf16(x, xb)
    s_pre = _empty((M, r), BF16, dev) if (save or M < 1024) else None       # (the small-M kernels always store it)
    s_h = _empty((M, r), BF16, dev)
    ops.gemm(xb, sa.W1, ops.EPI_ACT, s_h, bias=sa.b1, out2=s_pre, act=ops.ACT_GELU, at=dms1, ntok=P, aux_grad=_AUX_GRAD)
    # x'1 = x' + ao Wo^T + bo + s_h W2^T + dms1[tok] * b2
    xa = _empty((M, D), F32, dev)
    ops.gemm(ao, fz.Wo, ops.EPI_F32, xa, bias=fz.bo, resid=x)
    x1 = _empty((M, D), F32, dev)
    ops.gemm(s_h, sa.W2, ops.EPI_F32, x1, resid=xa, vec=sa.b2.reshape(1, -1), ldv=0, bt=dms1, ntok=P)
    del xa
    x2, xn, mean2, rstd2, hcat_pre, a_s = _mlp_adapter_forward(x1, fz, dms2, P, save)
    if not save:
        return x2, None
    c.update(x=x, xb=xb, mean1=mean1, rstd1=rstd1, qkv=qkv, ao=ao, lse=lse, s_pre=s_pre, s_h=s_h, x1=x1, mean2=mean2,
             rstd2=rstd2, xn=xn, hcat_pre=hcat_pre, a_s=a_s, dms1=dms1, dms2=dms2)
    return x2, c


def _block_backward(dyb, c, fz: _Frozen, adp: Dict[str, _AdapterW], grads, B, T, P, H, tcls: bool, shifts, keep: Optional[list]):
    """dyb = d(loss)/d(x2) [M, D] bf16 with a zero row 1 in every frame (tcls) -> d(loss)/d(x) with the same property;
    the adapters' gradients are accumulated into ``grads``."""
    dev = dyb.device
    M, D = dyb.shape
    BT, r = B * T, fz.r
    fork = _Fork(dev, "bwd")
    dx1b, later = _mlp_adapter_backward(dyb, c["x1"], c["mean2"], c["rstd2"], c["xn"], c["hcat_pre"], c["a_s"], c["dms2"], fz,
                                        grads["MLP_Adapter"], P)
    # ---- x'1 = x' + ao Wo^T + bo + s_h W2^T + dms1 b2,  s_h = dms1 GELU(xb W1^T + b1)
    sa, gs = adp["S_Adapter"], grads["S_Adapter"]
    dms1, s_h, xb = c["dms1"], c["s_h"], c["xb"]
    later.append(lambda: ops.wgrad(dx1b, s_h, gs["D_fc2.weight"], gs["D_fc2.bias"], at=dms1, ntok=P))
    dpre = _empty((M, r), BF16, dev)
    ops.gemm(dx1b, sa.W2T, ops.EPI_DACT, dpre, aux=c["s_pre"], act=ops.ACT_GELU, at=dms1, ntok=P, aux_grad=_AUX_GRAD)
    later.append(lambda: ops.wgrad(dpre, xb, gs["D_fc1.weight"], gs["D_fc1.bias"]))
    dxs = _empty((M, D), BF16, dev)
    ops.gemm(dpre, sa.W1T, ops.EPI_BF16, dxs)
    dres = _empty((M, D), BF16, dev)                 # what reaches x' beside ln_1: the residual and the S_Adapter's input
    ops.add_bf16(dx1b, dxs, dres)
    del dxs
    # ---- attention: out_proj dgrad, head-shifted backward (dK / dV land in the frames the keys came from), QKV dgrad
    dao = _empty((M, D), BF16, dev)
    ops.gemm(dx1b, fz.WoT, ops.EPI_BF16, dao, reserve_cus=_DP_RESERVE)
    dqkv = _empty((M, 3 * D), BF16, dev)
    delta = _empty((BT, H, P), F32, dev)
    ops.attn_bwd_shift(c["qkv"], c["ao"], dao, c["lse"], delta, dqkv, B, T, P, H, shifts)
    del dao
    dxl = _empty((M, D), BF16, dev)
    ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dxl, reserve_cus=_DP_RESERVE)
    del dqkv
    if tcls:
        _cls_chain_backward(dxl, c, fz, adp["T_Adapter"], grads["T_Adapter"], later, B, T, P, H)
    dxb = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl, c["x"], fz.g1, c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dres, dx_bf16=dxb)
    if tcls:
        dxb.view(BT, P, D)[:, 1].zero_()             # the slot belongs to this block: nothing flows further down through it
    _wgrads_beside(fork, later, keep)
    return dxb


class _ZeroI2VFn(torch.autograd.Function):
    """imgs -> [B, D, T] features.  Differentiable inputs: ``ViT_CLIP_ZEROI2V._trainable_list()``."""

    @staticmethod
    def forward(ctx, model: "ViT_CLIP_ZEROI2V", grad_enabled: bool, imgs: torch.Tensor, *params: torch.Tensor):
        L, H = model.layers, model.heads
        B, C, T, Hh, Ww = imgs.shape
        D, p = model.width, model.patch_size
        G = Hh // p
        N = G * G + 1
        tcls = model.with_t_cls_token
        P = N + int(tcls)
        BT = B * T
        dev = imgs.device
        temporal, lnp_w, lnp_b = params[0], params[1], params[2]
        need_grad = grad_enabled and any(ctx.needs_input_grad)
        frozen = model._frozen_operands()
        linear, share = model.linear_adapter, model.share_adapter
        merged = model._merged_operands() if (linear and model.merged) else None     # (forward() refused merged + gradients)
        adp = model._stage_adapters(frozen, params) if merged is None else None
        # patch embedding, class token, positional / temporal embeddings, ln_pre: ViT_CLIP's kernels, N tokens per frame
        tok, x0, mean0, rstd0, tmp = _embed_forward(model, frozen, imgs, temporal)
        if tcls:        # once per forward: into the P-token layout (row 1 = the temporal class token's slot)
            x = _empty((BT * P, D), F32, dev)
            xv, x0v = x.view(BT, P, D), x0.view(BT, N, D)
            xv[:, 0] = x0v[:, 0]
            xv[:, 2:] = x0v[:, 1:]
        else:
            x = x0
        del x0
        if model.inference_precision == 'fp8' and not need_grad and not model._fp8_warned:
            model._fp8_warned = True
            _LOG.warning("fp8 inference was requested but ViT_CLIP_ZEROI2V has no fp8 path: this forward runs bf16")
        if not linear:      # (the linear mode has no DropPath and no adapter scale)
            dp1, dp2 = model._drop_masks_z(P, N, model.training, dev)          # [L, P], [L, N]
            if tcls:
                dp2 = torch.cat([dp2[:, :1], torch.zeros_like(dp2[:, :1]), dp2[:, 1:]], dim=1).contiguous()
        shifts = model.head_shifts
        ctxs: List[Optional[dict]] = []
        for i in range(L):
            fz = frozen["blocks"][i]
            if merged is not None:
                x, c = lin.merged_block_forward(x, fz, merged[i], B, T, P, H, tcls, shifts, _cls_chain_forward), None
            elif linear:
                x, c = lin.block_forward(x, fz, adp[i], B, T, P, H, tcls, share, shifts, need_grad, _cls_chain_forward)
            else:
                x, c = _block_forward(x, fz, adp[i], B, T, P, H, tcls, shifts, dp1[i], dp2[i], need_grad)
            ctxs.append(c)
        y, gw, meanp, rstdp = _ln_post_forward(x, lnp_w, lnp_b, BT, P)
        if need_grad:
            ctx.model, ctx.dims = model, (B, T, N, P, H, D, L)
            ctx.saved = dict(ctxs=ctxs, adp=adp, tok=tok, mean0=mean0, rstd0=rstd0, tmp=tmp, xL=x, gw=gw, meanp=meanp,
                             rstdp=rstdp, params=params, shifts=shifts)
        return y.reshape(B, T, D).permute(0, 2, 1)      # '(b t) d -> b d t'

    @staticmethod
    def backward(ctx, dout):
        model = ctx.model
        B, T, N, P, H, D, L = ctx.dims
        s = ctx.saved
        tcls = P != N
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
            if model.linear_adapter:
                dxb = lin.block_backward(dxb, s["ctxs"][i], frozen["blocks"][i], s["adp"][i], layer_grads[i], B, T, P, H, tcls,
                                         model.share_adapter, s["shifts"], keep, _cls_chain_backward)
            else:
                dxb = _block_backward(dxb, s["ctxs"][i], frozen["blocks"][i], s["adp"][i], layer_grads[i], B, T, P, H, tcls,
                                      s["shifts"], keep)
            s["ctxs"][i] = None
            gbufs.layer_ready(i)
        if tcls:        # once per backward: back to the embedding's N tokens per frame (the slot's row is zero)
            d0 = _empty((BT, N, D), BF16, dev)
            dv = dxb.view(BT, P, D)
            d0[:, 0] = dv[:, 0]
            d0[:, 1:] = dv[:, 2:]
            dxb = d0.view(BT * N, D)
        grads = _embed_backward(gbufs, frozen, s, dxb, keep, B, T, N, D)
        ctx.saved = None
        return grads


@BACKBONES.register_module()
class ViT_CLIP_ZEROI2V(ViT_CLIP):
    """CLIP ViT + ZeroI2V adapters with head-shifted spatial attention (reference vit_clip_zeroI2V.py:361-509)."""

    def __init__(self, input_resolution: int, num_frames: int, patch_size: int, width: int, layers: int, heads: int,
                 drop_path_rate, num_tadapter=1, adapter_scale=0.5, with_t_cls_token=False, share_adapter=False,
                 bottleneck=192, linear_adapter=False, pretrained=None):
        if linear_adapter and (bottleneck % 8 != 0 or not 8 <= bottleneck <= min(width, lin.MAX_BOTTLENECK)):
            raise NotImplementedError(f"ViT_CLIP_ZEROI2V(linear_adapter=True, bottleneck={bottleneck}, width={width}): the fused "
                                      f"low-rank kernels of the linear adapters take a bottleneck that is a multiple of 8, at "
                                      f"most the width and at most {lin.MAX_BOTTLENECK}")
        if num_tadapter == 2 and with_t_cls_token:
            # reference :253 calls attention() with one argument: TypeError at the first forward
            raise TypeError("ViT_CLIP_ZEROI2V(num_tadapter=2, with_t_cls_token=True): the reference's block fails with "
                            "TypeError at its first forward (attention() misses an argument); num_tadapter must be 1")
        super().__init__(input_resolution, num_frames, patch_size, width, layers, heads, drop_path_rate,
                         adapter_scale=adapter_scale, pretrained=pretrained)
        self.num_tadapter = num_tadapter
        self.with_t_cls_token = bool(with_t_cls_token)
        self.share_adapter, self.bottleneck, self.linear_adapter = bool(share_adapter), bottleneck, bool(linear_adapter)
        for blk in self.transformer.resblocks:
            if not self.with_t_cls_token:   # reference :109-110: the T_Adapter exists only with the temporal class token
                del blk.T_Adapter
            if self.linear_adapter:         # reference :125-136: the linear adapters replace S_Adapter and MLP_Adapter
                del blk.S_Adapter, blk.MLP_Adapter
                for a in lin.adapter_names(self.share_adapter, False):
                    setattr(blk, a, lin.Linear_Adapter(width, bottleneck))
        self.head_shifts = head_shifts(num_frames, heads)
        self.variant = 'zeroi2v'
        if self.linear_adapter:
            self._adapter_names = lin.adapter_names(self.share_adapter, self.with_t_cls_token)
        else:
            self._adapter_names = ("MLP_Adapter", "S_Adapter") + (("T_Adapter",) if self.with_t_cls_token else ())
        self._fp8_warned = False
        self._merged, self._merge_cache = False, None

    def init_weights(self, pretrained=None):
        """ViT_CLIP's policy, with the reference's quirks in the linear mode (:397-458): ``Linear_Adapter.init_weights`` is
        never called, every nn.Linear gets trunc_normal_(.02), and the zeroing loops match ``MLP_Adapter_in / _out.D_fc2`` (and
        ``T_Adapter``) by name but not ``Attn_Adapter_*``, whose D_fc2 therefore starts non-zero.  With that and the doubled
        skip of the MLP adapters, an untrained linear model is NOT the frozen CLIP model."""
        super().init_weights(pretrained)
        if self.linear_adapter:
            for blk in self.transformer.resblocks:
                for a in ("MLP_Adapter_in", "MLP_Adapter_out"):
                    nn.init.constant_(getattr(blk, a).D_fc2.weight, 0)
                    nn.init.constant_(getattr(blk, a).D_fc2.bias, 0)

    def _frozen_block(self, blk):
        return lin._FrozenLin(blk, self._adapter_names) if self.linear_adapter else super()._frozen_block(blk)

    # ---- merging (linear mode): the adapters folded into the frozen weights --------------------------------------------
    @property
    def merged(self) -> bool:
        return self._merged

    def merge_adapters(self):
        """Fold every linear adapter into the frozen weight beside it (``zeroi2v_linear.fold_block``) and stage the result as
        a second set of frozen operands: from now on a no-grad forward runs every block without any adapter work, and a
        forward that needs gradients raises.  The fold is redone when an adapter (or frozen) tensor has changed."""
        if not self.linear_adapter:
            raise RuntimeError("ViT_CLIP_ZEROI2V.merge_adapters(): only the linear adapters (linear_adapter=True) fold into "
                               "the frozen weights")
        self._merged = True
        self._merged_operands()
        return self

    def unmerge_adapters(self):
        self._merged, self._merge_cache = False, None
        return self

    def _merged_operands(self):
        """per-block merged operands; rebuilt only when a block's tensor changed or moved"""
        # (FlatAdamW updates the adapters through raw pointers -- no tensor version changes -- and bumps `weights_epoch`)
        key = tuple((p.data_ptr(), p._version) for p in self._param_slots(self.transformer, "blocks")) + (self.weights_epoch,)
        if self._merge_cache is None or self._merge_cache[0] != key:
            with torch.no_grad():
                self._merge_cache = (key, [lin.fold_block(b, self.share_adapter, self.with_t_cls_token)
                                           for b in self.transformer.resblocks])
        return self._merge_cache[1]

    def set_precision(self, precision: str):
        if precision == 'fp32':
            raise NotImplementedError("ViT_CLIP_ZEROI2V has no fp32 verification mode")
        return super().set_precision(precision)

    def _drop_masks_z(self, P, N, training, dev):
        """DropPath factor times adapter scale per TOKEN index (timm's mask has shape (x.shape[0], 1, 1) and the reference's
        x is [tokens, BT, D]): per block the S_Adapter's over the P tokens, then the MLP_Adapter's over the N that remain --
        the reference's draw order and shapes (:297, :311) -> ([L, P], [L, N])."""
        blocks = self.transformer.resblocks
        L = len(blocks)
        # the per-layer constants live on the device (building them on the host every step costs pageable copies that stall it)
        key = (str(dev), tuple(float(b.drop_prob) for b in blocks), tuple(float(b.scale) for b in blocks))
        cached = getattr(self, "_drop_consts_z", None)
        if cached is None or cached[0] != key:
            rates, scale = torch.tensor(key[1], dtype=F32).view(L, 1), torch.tensor(key[2], dtype=F32).view(L, 1)
            keep = 1.0 - rates
            fac = torch.where(keep > 0, scale / keep.clamp_min(1e-12), torch.zeros_like(keep))
            cached = (key, float(rates.max()), scale.to(dev), keep.to(dev), fac.to(dev))
            self._drop_consts_z = cached
        _, max_rate, scale_d, keep_d, fac_d = cached
        if not training or max_rate <= 0.:
            return scale_d.expand(L, P).contiguous(), scale_d.expand(L, N).contiguous()
        u = torch.rand((L, P + N), dtype=F32, device=dev)
        m = (u < keep_d).to(F32) * fac_d
        return m[:, :P].contiguous(), m[:, P:].contiguous()

    def forward(self, x: torch.Tensor):
        if self._merged and torch.is_grad_enabled() and any(p.requires_grad for p in self._trainable_list()):
            raise RuntimeError("ViT_CLIP_ZEROI2V: the adapters are merged into the frozen weights, which has no backward; call "
                               "unmerge_adapters() before a forward that needs gradients")
        blend = self._take_blend_check_clip(x, "ViT_CLIP_ZEROI2V")
        N = (x.shape[3] // self.patch_size) ** 2 + 1
        if N + int(self.with_t_cls_token) > 288:
            raise ValueError(f"{N + int(self.with_t_cls_token)} tokens per frame: the attention kernels take at most 288")
        x = self._arm_clip(x, blend)
        y = _ZeroI2VFn.apply(self, torch.is_grad_enabled(), x, *self._trainable_list())     # [B, D, T]
        return y.unsqueeze(-1).unsqueeze(-1)
