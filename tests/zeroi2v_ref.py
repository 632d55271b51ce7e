"""Plain PyTorch restatement of the ViT_CLIP_ZEROI2V block and backbone (reference vit_clip_zeroI2V.py, ``linear_adapter=False``):
test infrastructure, as oracle/ is for ViT_CLIP.  Written from the algebra, frame-major ([BT, tokens, D]), any float dtype;
autograd gives the gradients.  tests/test_zeroi2v_cpu.py holds it to the real reference's stored outputs and gradients
(tests/golden/zeroi2v_*.npz) at the oracle bound of 2e-5 rel-L2; tests/test_zeroi2v_gpu.py compares the HIP backbone to it
at shapes the fixtures do not cover.

Per block, x [BT, N, D] (token 0 = class):
  1. with_t_cls_token: xt = T_Adapter(attention over the T class tokens of a clip (ln_1(cls))); x' = [cls, xt, patches]
  2. xln = ln_1(x'); q, k, v = in_proj(xln)
  3. head h of frame (b, t) sees the K and V of frame (b, (t - s_h) mod T)  (HeadShift: torch.roll along t, Q stays)
  4. x'1 = x' + out_proj(attn) + dp1[n'] * scale * S_Adapter(x')            (S_Adapter on the residual stream, no skip)
  5. token 1 is dropped
  6. x2 = x1 + mlp(ln_2 x1) + dp2[n] * scale * MLP_Adapter(ln_2 x1)
"""
import os
import sys
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vit_clip_oracle as O  # noqa: E402

# shift of the first heads by frames per clip; every other head, and every other T, is unshifted
HEAD_SHIFTS = {8: (1, -1), 16: (1, -1, 2, -2), 32: (1, -1, 2, -2, 3)}


def head_shifts(T: int, H: int):
    tab = HEAD_SHIFTS.get(T, ())
    if len(tab) > H:
        raise ValueError(f"{T} frames shift {len(tab)} heads, the model has {H}")
    return tuple(tab) + (0,) * (H - len(tab))


def head_shift(x: torch.Tensor, T: int, shifts: Sequence[int]) -> torch.Tensor:
    """x [BT, H, L, C] -> out[b T + t, h] = x[b T + (t - shifts[h]) mod T, h]: a gather, no roll"""
    BT, H, L, C = x.shape
    t = torch.arange(T).view(T, 1)
    src = (t - torch.tensor(list(shifts)).view(1, H)) % T                 # [T, H] source frame inside the clip
    y = x.reshape(BT // T, T, H, L, C)
    return y[:, src, torch.arange(H).view(1, H)].reshape(BT, H, L, C)


def backbone_param_shapes(res, T, patch, width, layers, with_t_cls_token=True):
    s = O.backbone_param_shapes(res, T, patch, width, layers)
    return s if with_t_cls_token else {k: v for k, v in s.items() if "T_Adapter" not in k}


def _attention(xq, st, pre, H, T=None, shifts=None):
    """xq [Nb, S, D] -> out_proj(softmax(q k^T / sqrt(dh)) v); `shifts`: K and V of head h come from a neighbouring frame"""
    W, b = st[pre + "attn.in_proj_weight"], st[pre + "attn.in_proj_bias"]
    Nb, S, D = xq.shape
    qkv = F.linear(xq, W, b).view(Nb, S, 3, H, D // H).permute(2, 0, 3, 1, 4)      # [3, Nb, H, S, dh]
    q, k, v = qkv[0], qkv[1], qkv[2]
    if shifts is not None and any(shifts):
        k, v = head_shift(k, T, shifts), head_shift(v, T, shifts)
    p = (q @ k.transpose(-2, -1) / (D // H) ** 0.5).softmax(dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(Nb, S, D)
    return F.linear(o, st[pre + "attn.out_proj.weight"], st[pre + "attn.out_proj.bias"])


def block(x, st: Dict[str, torch.Tensor], i: int, H: int, T: int, scale: float, with_t_cls_token: bool,
          masks=None, shift: bool = True):
    """x [BT, N, D] -> [BT, N, D].  masks: None or (dp1 [N + 1 or N], dp2 [N]) DropPath factors (bernoulli / keep)."""
    pre = f"transformer.resblocks.{i}."
    BT, N, D = x.shape
    ln1 = lambda t: F.layer_norm(t, (D,), st[pre + "ln_1.weight"], st[pre + "ln_1.bias"], 1e-5)
    if with_t_cls_token:
        cls = ln1(x[:, 0]).view(BT // T, T, D)                                       # a clip's T class tokens: one sequence
        xt = O.ref_adapter(_attention(cls, st, pre, H), st, pre + "T_Adapter").reshape(BT, 1, D)
        x = torch.cat([x[:, :1], xt, x[:, 1:]], dim=1)
    shifts = head_shifts(T, H) if shift else None
    sa = scale * O.ref_adapter(x, st, pre + "S_Adapter")
    if masks is not None:
        sa = sa * masks[0].to(x.dtype).view(1, -1, 1)
    x = x + _attention(ln1(x), st, pre, H, T, shifts) + sa
    if with_t_cls_token:
        x = torch.cat([x[:, :1], x[:, 2:]], dim=1)
    xn = F.layer_norm(x, (D,), st[pre + "ln_2.weight"], st[pre + "ln_2.bias"], 1e-5)
    h = F.linear(xn, st[pre + "mlp.c_fc.weight"], st[pre + "mlp.c_fc.bias"])
    h = F.linear(h * torch.sigmoid(1.702 * h), st[pre + "mlp.c_proj.weight"], st[pre + "mlp.c_proj.bias"])
    ma = scale * O.ref_adapter(xn, st, pre + "MLP_Adapter")
    if masks is not None:
        ma = ma * masks[1].to(x.dtype).view(1, -1, 1)
    return x + h + ma


def embed(imgs, st, T: int):
    """patch embedding + class token + positional / temporal embeddings + ln_pre (ViT_CLIP's) -> [BT, N, D]"""
    B, C, _, Hh, Ww = imgs.shape
    W = st["conv1.weight"]
    D, p = W.shape[0], W.shape[-1]
    x = F.conv2d(imgs.permute(0, 2, 1, 3, 4).reshape(B * T, C, Hh, Ww), W, None, stride=p).flatten(2).transpose(1, 2)
    x = torch.cat([st["class_embedding"].expand(B * T, 1, D), x], dim=1) + st["positional_embedding"]
    x = (x.view(B, T, -1, D) + st["temporal_embedding"].view(1, T, 1, D)).view(B * T, -1, D)
    return F.layer_norm(x, (D,), st["ln_pre.weight"], st["ln_pre.bias"], 1e-5)


def backbone(imgs, st, H: int, T: int, scale: float = 0.5, with_t_cls_token: bool = True, drop_masks=None,
             layers: Optional[int] = None, shift: bool = True):
    """[B, 3, T, h, w] -> [B, D, T, 1, 1].  drop_masks: None or, per layer, None or the (dp1, dp2) pair that layer drew."""
    B = imgs.shape[0]
    if layers is None:
        layers = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("transformer.resblocks."))
    x = embed(imgs, st, T)
    for i in range(layers):
        x = block(x, st, i, H, T, scale, with_t_cls_token, None if drop_masks is None else drop_masks[i], shift)
    D = x.shape[-1]
    y = F.layer_norm(x[:, 0], (D,), st["ln_post.weight"], st["ln_post.bias"], 1e-5)
    return y.view(B, T, D).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)


def masks_per_layer(stored, rates):
    """the reference's drawn masks in call order (two per block whose rate is > 0) -> one (dp1, dp2) pair or None per layer"""
    out, k = [], 0
    for r in rates:
        if r > 0:
            out.append((stored[k], stored[k + 1]))
            k += 2
        else:
            out.append(None)
    assert k == len(stored)
    return out
