"""``AIM_FLASH_WIN`` backbone (AIM with a 3-D window temporal attention and a temporal class-token prompt) on the HIP kernels.

Drop-in for ``mmaction/models/backbones/vitclip_aim_flash_win.py:276-433`` of the reference at ``wind_attn=True`` (what its four
recipes, ``configs/recognition/vit/AIM/AIM_flash_win_base_*.py``, use): same registry name, constructor keywords, ``init_weights``
policy, parameter names and shapes (``attn.Wqkv``, ``attn.out_proj``, ``mlp.fc1``, ``mlp.fc2`` of the reference's FlashMHA /
FlashMlp containers: the usual q | k | v head-major layout, softmax(Q K^T / sqrt(dh)) V and fc1 -> QuickGELU -> fc2, whatever
``use_flash_attn`` says), same ``forward(x[B,3,T,H,W]) -> [B,width,T,1,1]``.

Per block (reference ``:146-225``), frame-major rows, N = G G + 1 tokens per frame, f1 f2 f3 the block's three DropPath draws:

  1. xl = ln_1(x), qkv = xl Wqkv^T + b over ALL rows: ln_1 and the projection are token-wise, so one pass serves 2 and 3.
  2. patch tokens: attention inside the (wt, wh, ww) windows of the [T, G, G] grid -- ``aim_win_attn_fwd`` on the fused qkv
     buffer; window_partition / window_reverse are addresses inside the kernel, nothing is ever copied into window order.
  3. class tokens: attention over the T class tokens of each clip -- ``aim_cls_attn_fwd`` on the same buffer.
  4. ta = [3 | 2] Wo^T + bo (the reference's [cls_attn, windows_attn]);  x1 = x + f1[frame] T_Adapter(ta)   (no adapter scale)
  5. (prompt) ta's class row becomes one more token of its frame: x' = [x1, prompt];
     x2 = x' + attn(ln_1 x') + f2[frame] scale S_Adapter(x');  the prompt token is dropped.  This is zeroi2v.py's spatial step
     without head shifts (``aim_attn_fwd`` at 198 tokens).  The prompt's own output is discarded but it is a key and a value
     of every other token, so its gradient flows back into 3 through ta.
  6. x3 = x2 + mlp(ln_2 x2) + f3[frame] scale MLP_Adapter(ln_2 x2)      (``_mlp_adapter_forward``)

DropPath: x is [BT, n, d] when timm's DropPath sees it, so a draw has shape (BT, 1, 1) and drops FRAMES (``af`` of the GEMM
epilogues; ViT_CLIP drops token positions).  Three draws per block with rate > 0, in the order 4, 5, 6.

Layout: as in zeroi2v.py the residual stream keeps P = N + 1 token rows per frame through the whole stack when there is a
prompt.  The extra row is a slot BEHIND the frame's tokens (row N; attention does not see an order among keys, and every
other op is row-wise, so the reference's position 1 and this position N compute the same numbers): step 4's result is copied
into it (B T rows), steps 5 and 6 run on all P rows, and the slot's value after step 6 is dead -- the next block overwrites
it.  Its gradient row is extracted and zeroed once ln_1's backward of step 5 has produced it.  The window kernel takes the
row stride P beside N, so the slot costs no copy of the other rows; only the embedding is copied into the P layout once.

Steps 1-3, the out-projection of 4, their backward and the slot layout are plain functions in win_block.py, shared with the
windowed ``AIM`` (aim_variant.py); steps 4-6 are this file's.

The reference's shifted branch (``not_shift=False``) rolls the windows back and then DISCARDS the result (``:188`` assigns
``windows_attn``, ``:192`` rearranges ``shifted_win``): its output is mis-aligned by the shift.  It is not built.
"""
import logging
from typing import Dict, List, Optional

import torch
from torch import nn

from . import ops
from .backbone import (_AUX_GRAD, _DP_RESERVE, BF16, F32, Adapter, LayerNorm, QuickGELU, ViT_CLIP, _AdapterW, _embed_backward,
                       _clip_names, _embed_forward, _empty, _Fork, _Frozen, _GradBufs, _ln_post_backward, _ln_post_forward,
                       _mlp_adapter_backward, _mlp_adapter_forward, _wgrads_beside)
from .registry import BACKBONES
from .win_block import (check_win_clip, check_window, clip_window, from_slot_layout, to_slot_layout, win_prompt_grad,
                        win_temporal_backward, win_temporal_forward)

_LOG = logging.getLogger("aim_amd")


class _MHA(nn.Module):
    """Parameter container with the names of flash_attn's ``MHA`` (``Wqkv``, ``out_proj``)."""

    def __init__(self, d_model: int):
        super().__init__()
        self.Wqkv = nn.Linear(d_model, 3 * d_model)
        self.out_proj = nn.Linear(d_model, d_model)


class _Mlp(nn.Module):
    """Parameter container with the names of flash_attn's ``Mlp`` (``fc1``, ``fc2``)."""

    def __init__(self, d_model: int):
        super().__init__()
        self.fc1 = nn.Linear(d_model, 4 * d_model)
        self.activation = QuickGELU()
        self.fc2 = nn.Linear(4 * d_model, d_model)


class WinResidualAttentionBlock(nn.Module):
    """Parameters of one block (reference :100-139); compute lives in ``_FlashWinFn``."""

    def __init__(self, d_model: int, n_head: int, scale: float, num_frames: int, drop_path: float):
        super().__init__()
        self.attn = _MHA(d_model)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = _Mlp(d_model)
        self.ln_2 = LayerNorm(d_model)
        self.n_head, self.d_model = n_head, d_model
        self.MLP_Adapter = Adapter(d_model, skip_connect=False)
        self.S_Adapter = Adapter(d_model, skip_connect=False)
        self.scale = scale
        self.T_Adapter = Adapter(d_model, skip_connect=False)
        self.num_frames = num_frames
        self.drop_prob = float(drop_path)


class WinTransformer(nn.Module):
    def __init__(self, num_frames, width, layers, heads, scale, drop_path):
        super().__init__()
        self.width, self.layers = width, layers
        dpr = [x.item() for x in torch.linspace(0, drop_path, layers)]      # reference :235
        self.resblocks = nn.Sequential(*[WinResidualAttentionBlock(width, heads, scale, num_frames, dpr[i]) for i in range(layers)])


def _frozen_view(blk: WinResidualAttentionBlock):
    """the block's frozen tensors under the names ``_Frozen`` reads (CLIP's nn.MultiheadAttention / c_fc / c_proj)"""
    return _clip_names(blk, blk.attn.Wqkv, blk.attn.out_proj, blk.mlp.fc1, blk.mlp.fc2, blk.ln_1, blk.ln_2)


def _block_forward(x, fz: _Frozen, adp: Dict[str, _AdapterW], B, T, N, P, H, window, f1, f2, f3, tokm, save: bool, shift=None):
    """x [B*T*P, D] f32 (P = N + 1 with the prompt: row N of every frame is its slot) -> x3, ctx.  f1, f2, f3 [B*T]: the
    DropPath factors per frame (f2, f3 times the adapter scale); tokm [P]: 1 per token, 0 at the slot.  shift: None or the
    (st, sh, sw) by which this block's windows are shifted (aim_flash.py)."""
    dev = x.device
    M, D = x.shape
    BT, r = B * T, fz.r
    prompt = P != N
    xv = lambda t: t.view(BT, P, -1)
    # ---- 1, 2, 3 and out_proj (win_block.py)
    ta, c = win_temporal_forward(x, fz, B, T, N, P, H, window, shift, False)
    # ---- 4: T_Adapter, x1 = x + f1 (GELU(ta W1^T + b1) W2^T + b2)
    tad = adp["T_Adapter"]
    t_pre, t_hs = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(ta, tad.W1, ops.EPI_ACT, t_hs, bias=tad.b1, out2=t_pre, act=ops.ACT_GELU, af=f1, ntok=P, aux_grad=_AUX_GRAD)
    x1 = _empty((M, D), F32, dev)
    ops.gemm(t_hs, tad.W2, ops.EPI_F32, x1, resid=x, vec=f1.reshape(-1, 1) * tad.b2.reshape(1, -1), ldv=D, ntok=P)
    # ---- 5: the prompt token, spatial attention over the P tokens of a frame, S_Adapter on the residual stream itself
    if prompt:
        xv(x1)[:, N] = xv(ta)[:, 0]
    xl2 = _empty((M, D), BF16, dev)
    mean1b, rstd1b = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x1, fz.g1, fz.b1, M, D, D, y_bf16=xl2, mean=mean1b, rstd=rstd1b)
    qkv2 = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl2, fz.Wqkv, ops.EPI_BF16, qkv2, bias=fz.bqkv)
    del xl2
    ao = _empty((M, D), BF16, dev)
    lse = _empty((BT, H, P), F32, dev)
    ops.attn_fwd(qkv2, ao, lse, BT, P, H)
    sa = adp["S_Adapter"]
    xb = _empty((M, D), BF16, dev)
    ops.cast_bf16(x1, xb)
    s_pre, s_h = _empty((M, r), BF16, dev), _empty((M, r), BF16, dev)
    ops.gemm(xb, sa.W1, ops.EPI_ACT, s_h, bias=sa.b1, out2=s_pre, act=ops.ACT_GELU, af=f2, ntok=P, aux_grad=_AUX_GRAD)
    xa = _empty((M, D), F32, dev)
    ops.gemm(ao, fz.Wo, ops.EPI_F32, xa, bias=fz.bo, resid=x1)
    x2 = _empty((M, D), F32, dev)
    ops.gemm(s_h, sa.W2, ops.EPI_F32, x2, resid=xa, vec=f2.reshape(-1, 1) * sa.b2.reshape(1, -1), ldv=D, ntok=P)
    del xa
    # ---- 6: joint adaptation
    x3, xn, mean2, rstd2, hcat_pre, a_s = _mlp_adapter_forward(x2, fz, tokm, P, save, af=f3)
    if not save:
        return x3, None
    c.update(x=x, ta=ta, t_pre=t_pre, t_hs=t_hs, x1=x1, mean1b=mean1b, rstd1b=rstd1b, qkv2=qkv2, ao=ao, lse=lse, xb=xb,
             s_pre=s_pre, s_h=s_h, x2=x2, mean2=mean2, rstd2=rstd2, xn=xn, hcat_pre=hcat_pre, a_s=a_s, f1=f1, f2=f2, f3=f3,
             tokm=tokm)
    return x3, c


def _block_backward(dyb, c, fz: _Frozen, adp: Dict[str, _AdapterW], grads, B, T, N, P, H, window, keep: Optional[list],
                    shift=None):
    """dyb = d(loss)/d(x3) [M, D] bf16 with a zero slot row in every frame -> d(loss)/d(x) with the same property; the
    adapters' gradients are accumulated into ``grads``.  shift: what the block's forward was given."""
    dev = dyb.device
    M, D = dyb.shape
    BT, r = B * T, fz.r
    fork = _Fork(dev, "bwd")
    f1, f2, f3 = c["f1"], c["f2"], c["f3"]
    dx2b, later = _mlp_adapter_backward(dyb, c["x2"], c["mean2"], c["rstd2"], c["xn"], c["hcat_pre"], c["a_s"], c["tokm"], fz,
                                        grads["MLP_Adapter"], P, af=f3)
    # ---- 5: x2 = x' + ao Wo^T + bo + s_h W2^T + f2 b2,  s_h = f2 GELU(xb W1^T + b1)
    sa, gs = adp["S_Adapter"], grads["S_Adapter"]
    s_h, xb = c["s_h"], c["xb"]
    later.append(lambda: (ops.wgrad(dx2b, s_h, gs["D_fc2.weight"]), ops.colsum(dx2b, gs["D_fc2.bias"], af=f2, ntok=P)))
    dpre = _empty((M, r), BF16, dev)
    ops.gemm(dx2b, sa.W2T, ops.EPI_DACT, dpre, aux=c["s_pre"], act=ops.ACT_GELU, af=f2, ntok=P, aux_grad=_AUX_GRAD)
    later.append(lambda: ops.wgrad(dpre, xb, gs["D_fc1.weight"], gs["D_fc1.bias"]))
    dxs = _empty((M, D), BF16, dev)
    ops.gemm(dpre, sa.W1T, ops.EPI_BF16, dxs)
    dres = _empty((M, D), BF16, dev)
    ops.add_bf16(dx2b, dxs, dres)
    del dxs
    dao = _empty((M, D), BF16, dev)
    ops.gemm(dx2b, fz.WoT, ops.EPI_BF16, dao, reserve_cus=_DP_RESERVE)
    dqkv = _empty((M, 3 * D), BF16, dev)
    delta = _empty((BT, H, P), F32, dev)
    ops.attn_bwd(c["qkv2"], c["ao"], dao, c["lse"], delta, dqkv, BT, P, H)
    del dao
    dxl = _empty((M, D), BF16, dev)
    ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dxl, reserve_cus=_DP_RESERVE)
    dx1b = _empty((M, D), BF16, dev)
    ops.layernorm_bwd(dxl, c["x1"], fz.g1, c["mean1b"], c["rstd1b"], M, D, lddy=D, ldx=D, lddx=D, dres=dres, dx_bf16=dx1b)
    del dres
    dprompt = win_prompt_grad(dx1b, BT, N, P)
    # ---- 4: x1 = x + t_hs W2^T + f1 b2,  t_hs = f1 GELU(ta W1^T + b1),  ta = [cls_attn | windows_attn] Wo^T + bo
    tad, gt = adp["T_Adapter"], grads["T_Adapter"]
    t_hs, ta = c["t_hs"], c["ta"]
    later.append(lambda: (ops.wgrad(dx1b, t_hs, gt["D_fc2.weight"]), ops.colsum(dx1b, gt["D_fc2.bias"], af=f1, ntok=P)))
    dtp = _empty((M, r), BF16, dev)
    ops.gemm(dx1b, tad.W2T, ops.EPI_DACT, dtp, aux=c["t_pre"], act=ops.ACT_GELU, af=f1, ntok=P, aux_grad=_AUX_GRAD)
    dta = _empty((M, D), BF16, dev)
    ops.gemm(dtp, tad.W1T, ops.EPI_BF16, dta)
    later.append(lambda: ops.wgrad(dtp, ta, gt["D_fc1.weight"], gt["D_fc1.bias"]))
    # ---- out_proj, 3, 2, 1 (win_block.py), on the spatial step's d(qkv), delta and dxl buffers
    dxb = win_temporal_backward(dta, dx1b, c, fz, dqkv, delta, dxl, B, T, N, P, H, window, shift, False, dprompt)
    _wgrads_beside(fork, later, keep)
    return dxb


class _FlashWinFn(torch.autograd.Function):
    """imgs -> [B, D, T] features.  Differentiable inputs: ``AIM_FLASH_WIN._trainable_list()``."""

    @staticmethod
    def forward(ctx, model: "AIM_FLASH_WIN", grad_enabled: bool, imgs: torch.Tensor, *params: torch.Tensor):
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
        if model.inference_precision == 'fp8' and not need_grad and not model._fp8_warned:
            model._fp8_warned = True
            _LOG.warning("fp8 inference was requested but AIM_FLASH_WIN has no fp8 path: this forward runs bf16")
        fac = model._drop_masks_w(BT, model.training, dev)            # [L, 3, BT]
        tokm = torch.ones(P, dtype=F32, device=dev)
        if P != N:
            tokm[N] = 0
        window = clip_window(model.window_size, T, G)
        shifts = [model._block_shift(i, T, G) for i in range(L)]
        ctxs: List[Optional[dict]] = []
        for i in range(L):
            x, c = _block_forward(x, frozen["blocks"][i], adp[i], B, T, N, P, H, window, fac[i, 0], fac[i, 1], fac[i, 2], tokm,
                                  need_grad, shifts[i])
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
            dxb = _block_backward(dxb, s["ctxs"][i], frozen["blocks"][i], s["adp"][i], layer_grads[i], B, T, N, P, H,
                                  s["window"], keep, s["shifts"][i])
            s["ctxs"][i] = None
            gbufs.layer_ready(i)
        dxb = from_slot_layout(dxb, BT, N, P)
        grads = _embed_backward(gbufs, frozen, s, dxb, keep, B, T, N, D)
        ctx.saved = None
        return grads


@BACKBONES.register_module()
class AIM_FLASH_WIN(ViT_CLIP):
    """AIM with 3-D window temporal attention and a temporal class-token prompt (reference vitclip_aim_flash_win.py:276-433)."""

    def __init__(self, input_resolution: int, num_frames: int, patch_size: int, width: int, layers: int, heads: int,
                 drop_path_rate, num_tadapter=1, adapter_scale=0.5, pretrained=None, checkpoint=False, use_flash_attn=True,
                 prompt=True, wind_attn=False, window_size=(32, 2, 2), not_shift=True):
        if not wind_attn:
            raise NotImplementedError("AIM_FLASH_WIN(wind_attn=False) (vitclip_aim_flash_win.py:147-156: temporal attention "
                                      "over the frames of every token) is the stock AIM block: build type='AIM' for it")
        if not not_shift:
            raise NotImplementedError("AIM_FLASH_WIN(not_shift=False): the reference's shifted branch rolls the windows back and "
                                      "then discards the result (vitclip_aim_flash_win.py:188 against :192), so its output is "
                                      "mis-aligned by the shift; it is not built")
        if num_tadapter != 1:
            raise NotImplementedError("AIM_FLASH_WIN(num_tadapter=2) (T_Adapter_in) is not built")
        if checkpoint:
            raise NotImplementedError("AIM_FLASH_WIN(checkpoint=True) (activation recompute per block) is not built")
        check_window(window_size, num_frames, input_resolution // patch_size)
        super().__init__(input_resolution, num_frames, patch_size, width, 0, heads, drop_path_rate,
                         adapter_scale=adapter_scale, pretrained=pretrained)
        self.layers = layers
        self.transformer = WinTransformer(num_frames, width, layers, heads, adapter_scale, drop_path_rate)
        self.num_tadapter, self.use_flash_attn, self.prompt = num_tadapter, use_flash_attn, bool(prompt)
        self.wind_attn, self.window_size, self.not_shift = wind_attn, tuple(int(w) for w in window_size), not_shift
        self.variant = 'aim_flash_win'
        self._fp8_warned = False

    def set_precision(self, precision: str):
        if precision == 'fp32':
            raise NotImplementedError("AIM_FLASH_WIN has no fp32 verification mode")
        return super().set_precision(precision)

    def init_weights(self, pretrained=None):
        """Reference ``init_weights`` (:300-398): CLIP's ``in_proj_*`` / ``c_fc`` / ``c_proj`` go into ``Wqkv`` / ``fc1`` / ``fc2``."""
        if pretrained:
            self.pretrained = pretrained
        if isinstance(self.pretrained, str):
            try:
                import clip  # noqa: F401
            except ImportError as e:
                raise RuntimeError("pretrained=%r needs the OpenAI `clip` package and its downloaded weights; load a state_dict "
                                   "with this class's names instead" % (self.pretrained,)) from e
            name, self.pretrained = self.pretrained, None
            super().init_weights()
            self.pretrained = name
            clip_model, _ = clip.load("ViT-B/16" if self.layers == 12 else "ViT-L/14", device="cpu")
            sd = clip_model.visual.state_dict()
            del clip_model
            del sd['proj']
            swaps = (('attn.in_proj_weight', 'attn.Wqkv.weight'), ('attn.in_proj_bias', 'attn.Wqkv.bias'),
                     ('mlp.c_fc.', 'mlp.fc1.'), ('mlp.c_proj.', 'mlp.fc2.'))
            out = {}
            for k, v in sd.items():
                for a, b in swaps:
                    k = k.replace(a, b)
                out[k] = v
            msg = self.load_state_dict(out, strict=False)
            _LOG.info('Missing keys: %s', msg.missing_keys)
            _LOG.info('Unexpected keys: %s', msg.unexpected_keys)
            self._frozen_cache = None
        else:
            super().init_weights()

    def _frozen_block(self, blk):
        return _Frozen(_frozen_view(blk))

    def _block_shift(self, i: int, T: int, G: int):
        """the (st, sh, sw) of block i's windows on a T x G x G grid, or None: this class shifts none (aim_flash.py does)"""
        return None

    def _drop_masks_w(self, BT, training, dev):
        """The three DropPath factors of every block per FRAME, ``[L, 3, BT]``, in the reference's draw order (:200, :215,
        :224); the second and third carry the adapter scale, the first does not."""
        blocks = self.transformer.resblocks
        L = len(blocks)
        key = (str(dev), tuple(float(b.drop_prob) for b in blocks), tuple(float(b.scale) for b in blocks))
        cached = getattr(self, "_drop_consts_w", None)
        if cached is None or cached[0] != key:
            rates, scale = torch.tensor(key[1], dtype=F32).view(L, 1, 1), torch.tensor(key[2], dtype=F32).view(L, 1, 1)
            scale3 = torch.cat([torch.ones_like(scale), scale, scale], dim=1)            # [L, 3, 1]
            keep = 1.0 - rates
            fac = torch.where(keep > 0, scale3 / keep.clamp_min(1e-12), torch.zeros_like(scale3))
            cached = (key, float(rates.max()), scale3.to(dev), keep.to(dev), fac.to(dev))
            self._drop_consts_w = cached
        _, max_rate, scale_d, keep_d, fac_d = cached
        if not training or max_rate <= 0.:
            return scale_d.expand(L, 3, BT).contiguous()
        u = torch.rand((L, 3, BT), dtype=F32, device=dev)
        return ((u < keep_d).to(F32) * fac_d).contiguous()

    def forward(self, x: torch.Tensor):
        blend = self._take_blend_check_clip(x, "AIM_FLASH_WIN")
        T, N = x.shape[2], (x.shape[3] // self.patch_size) ** 2 + 1
        check_win_clip(T, N, self.prompt)
        x = self._arm_clip(x, blend)
        y = _FlashWinFn.apply(self, torch.is_grad_enabled(), x, *self._trainable_list())     # [B, D, T]
        return y.unsqueeze(-1).unsqueeze(-1)
