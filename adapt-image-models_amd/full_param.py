"""What the two full-parameter backbones (``ViT_ImageNet``, ``TimeSformer``) share, in both precisions: the gradient buffers of
a backward, ``ln_post``'s backward on the class rows, the patch conv's weight gradient, the fp32 autograd node's ``forward``,
and the module-level plumbing (precision switches, the operand cache's key, the clip checks, the dispatch).

Plain functions called in place and one small base class; each model keeps its own ``autograd.Function`` (DESIGN.md section 1:
no base ``Function``, no skeleton with callbacks).  Not here, because the two models differ in them: the block functions, the
``wgrad`` closures of the block backwards, the stems and their backwards, the DropPath factor producers, ``_stage_adapters``.
"""
import logging

import torch
from torch import nn

from . import ops
from .backbone import BF16, F32, _empty

_LOG = logging.getLogger("aim_amd")


class GradBufs:
    """Gradient buffers of one backward, by parameter name (fp32; every kernel ACCUMULATES into them).  A parameter that is not
    wanted has None and costs no launch.  With ``in_place`` (``model.grad_in_place``, set by dist.build_optimizer for the
    flat-buffer optimizer) a wanted parameter's buffer is its existing ``param.grad`` view of the flat gradient buffer and
    autograd gets None for it: no zero-filled temporary and no second pass to add it into the buffer."""

    def __init__(self, names, params, need, dev, in_place: bool):
        self.params = params
        self.in_place = [bool(need[k] and in_place and p_.grad is not None and p_.grad.dtype == F32
                              and p_.grad.is_contiguous() and p_.grad.device == dev) for k, p_ in enumerate(params)]
        self.grads = [p_.grad if self.in_place[k] else (torch.zeros(p_.shape, dtype=F32, device=dev) if need[k] else None)
                      for k, p_ in enumerate(params)]
        self.by_name = dict(zip(names, self.grads))

    def __getitem__(self, name):
        return self.by_name[name]

    def get(self, name):
        """as ``[name]``, and None for a parameter the model does not have"""
        return self.by_name.get(name)

    def block(self, pre):
        """the wanted buffers under the prefix ``pre``, by the rest of their name"""
        return {n[len(pre):]: t for n, t in self.by_name.items() if n.startswith(pre) and t is not None}

    def result(self, lead):
        """what autograd gets: ``lead`` Nones for the non-tensor inputs, then per parameter None (not wanted, or accumulated in
        place) or the buffer in the parameter's dtype"""
        out = []
        for k, p_ in enumerate(self.params):
            gk = None if self.in_place[k] else self.grads[k]
            out.append(gk if gk is None or gk.dtype == p_.dtype else gk.to(p_.dtype))
        return (None,) * lead + tuple(out)


def ln_post_backward(dout, s, dgw, dgb, BT, N, dtype):
    """ln_post's backward from d(loss)/d(output) [B, D, T] into a zero-filled [BT*N, D] gradient of ``dtype`` (it touches the
    class rows only), and its affine pair on ``aim_layernorm_gb_bwd`` (ordered, no atomics) when either is wanted."""
    D = dout.shape[1]
    dy = dout.permute(0, 2, 1).reshape(BT, D).contiguous().float()
    dx = torch.zeros((BT * N, D), dtype=dtype, device=dout.device)
    out = dict(dx_bf16=dx) if dtype == BF16 else dict(dx=dx)
    ops.layernorm_bwd(dy, s["xL"], s["gw"], s["meanp"], s["rstdp"], BT, D, lddy=D, ldx=N * D, lddx=N * D, **out)
    if dgw is not None or dgb is not None:
        ops.layernorm_gb_bwd(dy, s["xL"], s["meanp"], s["rstdp"], BT, D, dgw, dgb, ldx=N * D)
    return dx


def conv_wgrad(imgs, dtok, gconv, p, Kp):
    """gconv [D, 3, p, p] += dtok^T A on the bf16 path.  The patch matrix A was freed after the forward's GEMM: it is gathered
    again, at the conv operand's padded width ``Kp``; where Kp != K = 3 p p the product goes to a scratch buffer first."""
    B, _, T, Hh, Ww = imgs.shape
    D, K, dev = gconv.shape[0], 3 * p * p, dtok.device
    A = _empty((dtok.shape[0], Kp), BF16, dev)
    ops.patchify(imgs, A, B, T, Hh, Ww, p, Kp)
    dwc = torch.zeros((D, Kp), dtype=F32, device=dev) if Kp != K else gconv.view(D, K)
    ops.wgrad(dtok, A, dwc)
    if Kp != K:
        gconv.view(D, K).add_(dwc[:, :K])


def conv_wgrad_f32(imgs, dtok, gconv, p):
    """gconv [D, 3, p, p] += dtok^T A on the fp32 path: the f32 patch matrix, gathered again at K = 3 p p"""
    B, _, T, Hh, Ww = imgs.shape
    D, K = gconv.shape[0], 3 * p * p
    A = _empty((dtok.shape[0], K), F32, dtok.device)
    ops.patchify(imgs, A, B, T, Hh, Ww, p, K)
    ops.wgrad_f32(dtok, A, gconv.view(D, K))


def node_forward_f32(ctx, forward_f32, model, imgs, params):
    """``forward`` of an fp32 autograd node whose inputs are (model, imgs, *params): runs the model's ``forward_f32`` with the
    names of the parameters that want a gradient, and leaves ``need`` / ``model`` / ``saved`` / ``params`` on ``ctx``."""
    names = model._param_names()
    ctx.need = [bool(ctx.needs_input_grad[2 + k]) for k in range(len(params))]
    y, saved = forward_f32(model, imgs, dict(zip(names, params)), {n for n, nd in zip(names, ctx.need) if nd})
    ctx.model, ctx.saved, ctx.params = model, saved, params
    return y


def init_linear_layernorm(m):
    """the reference's ``_init_weights``: trunc_normal_(.02) Linear weights, zero biases, LayerNorms 1 / 0"""
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


class FullParamBackbone(nn.Module):
    """The runtime state and plumbing of a backbone in which every parameter trains; no parameters or buffers of its own."""

    def __init__(self):
        super().__init__()
        self._operand_cache = None
        self._names_cache = None
        self.weights_epoch = 0                      # bumped by an attached dist.FlatAdamW's step(): weights changed in place
        self.grad_in_place = False                  # accumulate straight into param.grad (set by dist.build_optimizer)
        self.inference_precision = 'bf16'
        self.precision = 'bf16'
        self._fp8_warned = False

    def _init_then_wants_load(self, pretrained) -> bool:
        """The head of the reference's ``init_weights``: take ``pretrained``, refuse what is neither a str nor None, apply
        ``init_linear_layernorm``, drop the cached operands.  True when a checkpoint is to be loaded over the result."""
        if pretrained:
            self.pretrained = pretrained
        if not (isinstance(self.pretrained, str) or self.pretrained is None):
            raise TypeError('pretrained must be a str or None')
        self.apply(init_linear_layernorm)
        self._operand_cache = None
        return isinstance(self.pretrained, str)

    def set_precision(self, precision: str):
        """'bf16' (default) | 'fp32': the reference-precision verification mode (the model's ``*_fp32.py``: f32-MFMA kernels, the
        same hand-written backward in fp32, plain autograd outputs)."""
        if precision not in ('bf16', 'fp32'):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        self.precision = precision
        return self

    def set_inference_precision(self, precision: str):
        """'bf16' | 'fp8'; these backbones have no fp8 path: 'fp8' warns once and runs bf16."""
        if precision not in ('bf16', 'fp8'):
            raise ValueError("inference precision must be 'bf16' or 'fp8'")
        self.inference_precision = precision
        return self

    def _param_names(self):
        if self._names_cache is None:
            self._names_cache = [n for n, _ in self.named_parameters()]
        return self._names_cache

    def _cached_operands(self, ps, build):
        """``build()``'s operands of the parameters ``ps``, rebuilt when one of them changed: moved, changed version, or -- when
        any of them trains -- an optimizer step that wrote them through raw pointers (``FlatAdamW.generation``,
        ``weights_epoch``)."""
        from .dist import FlatAdamW
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if any(p.requires_grad for p in ps):     # (a FlatAdamW step writes through raw pointers: no version changes)
            key += (self.weights_epoch, FlatAdamW.generation)
        if self._operand_cache is None or self._operand_cache[0] != key:
            self._operand_cache = (key, build())
        return self._operand_cache[1]

    def _check_clip(self, x: torch.Tensor, res: int) -> torch.Tensor:
        """the clip ``forward`` takes, [B, 3, num_frames, res, res] on the GPU, as the kernels read it (float32 / bfloat16,
        contiguous)"""
        name = type(self).__name__
        if not x.is_cuda:
            raise RuntimeError(f"aim_amd.{name} runs on MI355X only (HIP kernels); there is no CPU fallback")
        B, C, T, H, W = x.shape
        if T != self.num_frames:
            raise ValueError(f"expected {self.num_frames} frames, got {T}")
        if C != 3 or H != res or W != res:
            raise ValueError(f"expected input [B,3,{T},{res},{res}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"{name} takes float clips, got {x.dtype}")
        if x.dtype == torch.float16:
            x = x.float()
        return x.contiguous()

    def _dispatch(self, x, fn, fn32, forward_f32):
        """x -> [B, D, T, 1, 1] through the bf16 node ``fn``, or in fp32 mode through the node ``fn32`` when a gradient can be
        asked for and through plain ``forward_f32`` otherwise."""
        if self.inference_precision == 'fp8' and not self._fp8_warned:
            self._fp8_warned = True
            _LOG.warning(f"fp8 inference was requested but {type(self).__name__} has no fp8 path: this forward runs bf16")
        params = [p for _, p in self.named_parameters()]
        if self.precision == 'fp32':
            if torch.is_grad_enabled() and any(p.requires_grad for p in params):
                y = fn32.apply(self, x, *params)
            else:
                with torch.no_grad():
                    y = forward_f32(self, x, dict(zip(self._param_names(), params)), ())[0]
            return y.unsqueeze(-1).unsqueeze(-1)
        y = fn.apply(self, torch.is_grad_enabled(), x, *params)      # [B, D, T]
        return y.unsqueeze(-1).unsqueeze(-1)
