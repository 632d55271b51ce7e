"""Plain PyTorch restatement of the AIM_FLASH_WIN block and backbone (reference vitclip_aim_flash_win.py, ``wind_attn=True``,
unshifted): test infrastructure, as tests/zeroi2v_ref.py is for ViT_CLIP_ZEROI2V.  Written from the algebra, frame-major
([BT, tokens, D]), any float dtype, windows taken by INDEX (no view / permute of the grid); autograd gives the gradients.
tests/test_aim_flash_win_cpu.py holds it to the real reference's stored outputs and gradients
(tests/golden/aim_flash_win_tiny_*.npz) at the oracle bound of 2e-5 rel-L2; tests/test_aim_flash_win_gpu.py compares the
HIP backbone to it at the real window geometry, which the fixtures do not cover.

Per block, x [BT, N, D] (token 0 = class, G = sqrt(N - 1)), f1 f2 f3 the DropPath factors per FRAME (or None):
  1. xl = ln_1(x)
  2. patch tokens: attn(xl) inside each (wt, wh, ww) window of the [T, G, G] grid (extents clipped to the grid's)
  3. class tokens: attn(xl) over the T class tokens of each clip                                          -> cls_attn
  4. x = x + f1 T_Adapter([cls_attn, windows_attn])                                  (no adapter scale on this term)
  5. prompt: x' = [cls, cls_attn, patches];  x' = x' + attn(ln_1 x') + f2 scale S_Adapter(x');  token 1 is dropped
  6. x = x + mlp(ln_2 x) + f3 scale MLP_Adapter(ln_2 x)
attn = out_proj(softmax(q k^T / sqrt(dh)) v) with Wqkv (q | k | v, head-major); mlp = fc2(QuickGELU(fc1)).
"""
import os
import sys
from typing import Dict, Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vit_clip_oracle as O  # noqa: E402

RENAME = (("attn.in_proj_weight", "attn.Wqkv.weight"), ("attn.in_proj_bias", "attn.Wqkv.bias"), ("mlp.c_fc.", "mlp.fc1."),
          ("mlp.c_proj.", "mlp.fc2."))


def backbone_param_shapes(res, T, patch, width, layers):
    """ViT_CLIP's tensors under the names of the reference's FlashMHA / FlashMlp containers"""
    out = {}
    for k, v in O.backbone_param_shapes(res, T, patch, width, layers).items():
        for a, b in RENAME:
            k = k.replace(a, b)
        out[k] = v
    return out


def clip_window(window, T, G):
    return min(window[0], T), min(window[1], G), min(window[2], G)


def window_index(B, T, G, window):
    """[B nW, S] indices into the flattened [B, T, G, G] patch grid, windows in (b, it, ih, iw) order, tokens (dt, dh, dw)"""
    wt, wh, ww = clip_window(window, T, G)
    if T % wt or G % wh or G % ww:
        raise ValueError(f"window {(wt, wh, ww)} does not divide the grid {(T, G, G)}")
    b, it, ih, iw, dt, dh, dw = torch.meshgrid(torch.arange(B), torch.arange(T // wt), torch.arange(G // wh), torch.arange(G // ww),
                                               torch.arange(wt), torch.arange(wh), torch.arange(ww), indexing="ij")
    idx = ((b * T + it * wt + dt) * G + ih * wh + dh) * G + iw * ww + dw
    return idx.reshape(-1, wt * wh * ww)


def _attention(xq, st, pre, H):
    """xq [Nb, S, D] -> out_proj(softmax(q k^T / sqrt(dh)) v)"""
    Nb, S, D = xq.shape
    qkv = F.linear(xq, st[pre + "attn.Wqkv.weight"], st[pre + "attn.Wqkv.bias"]).view(Nb, S, 3, H, D // H).permute(2, 0, 3, 1, 4)
    p = (qkv[0] @ qkv[1].transpose(-2, -1) / (D // H) ** 0.5).softmax(dim=-1)
    o = (p @ qkv[2]).permute(0, 2, 1, 3).reshape(Nb, S, D)
    return F.linear(o, st[pre + "attn.out_proj.weight"], st[pre + "attn.out_proj.bias"])


def block(x, st: Dict[str, torch.Tensor], i: int, H: int, T: int, scale: float, window, prompt: bool = True, masks=None):
    """x [BT, N, D] -> [BT, N, D].  masks: None or the block's three DropPath factors per frame, each [BT]."""
    pre = f"transformer.resblocks.{i}."
    BT, N, D = x.shape
    B, G = BT // T, int(round((N - 1) ** 0.5))
    ln1 = lambda t: F.layer_norm(t, (D,), st[pre + "ln_1.weight"], st[pre + "ln_1.bias"], 1e-5)
    f = (lambda k: 1.0) if masks is None else (lambda k: masks[k].to(x.dtype).view(BT, 1, 1))
    xl = ln1(x)
    idx = window_index(B, T, G, window)
    patches = xl[:, 1:].reshape(BT * G * G, D)
    wo = _attention(patches[idx.reshape(-1)].view(idx.shape[0], idx.shape[1], D), st, pre, H)
    win = torch.zeros_like(patches).index_add(0, idx.reshape(-1), wo.reshape(-1, D)).view(BT, G * G, D)     # (a permutation)
    cls_attn = _attention(xl[:, 0].view(B, T, D), st, pre, H).reshape(BT, 1, D)
    x = x + f(0) * O.ref_adapter(torch.cat([cls_attn, win], dim=1), st, pre + "T_Adapter")
    if prompt:
        x = torch.cat([x[:, :1], cls_attn, x[:, 1:]], dim=1)
    x = x + _attention(ln1(x), st, pre, H) + f(1) * scale * O.ref_adapter(x, st, pre + "S_Adapter")
    if prompt:
        x = torch.cat([x[:, :1], x[:, 2:]], dim=1)
    xn = F.layer_norm(x, (D,), st[pre + "ln_2.weight"], st[pre + "ln_2.bias"], 1e-5)
    h = F.linear(xn, st[pre + "mlp.fc1.weight"], st[pre + "mlp.fc1.bias"])
    h = F.linear(h * torch.sigmoid(1.702 * h), st[pre + "mlp.fc2.weight"], st[pre + "mlp.fc2.bias"])
    return x + h + f(2) * scale * O.ref_adapter(xn, st, pre + "MLP_Adapter")


def embed(imgs, st, T: int):
    """patch embedding + class token + positional / temporal embeddings + ln_pre -> [BT, N, D]"""
    B, C, _, Hh, Ww = imgs.shape
    W = st["conv1.weight"]
    D, p = W.shape[0], W.shape[-1]
    x = F.conv2d(imgs.permute(0, 2, 1, 3, 4).reshape(B * T, C, Hh, Ww), W, None, stride=p).flatten(2).transpose(1, 2)
    x = torch.cat([st["class_embedding"].expand(B * T, 1, D), x], dim=1) + st["positional_embedding"]
    x = (x.view(B, T, -1, D) + st["temporal_embedding"].view(1, T, 1, D)).view(B * T, -1, D)
    return F.layer_norm(x, (D,), st["ln_pre.weight"], st["ln_pre.bias"], 1e-5)


def backbone(imgs, st, H: int, T: int, window, scale: float = 0.5, prompt: bool = True, drop_masks=None,
             layers: Optional[int] = None):
    """[B, 3, T, h, w] -> [B, D, T, 1, 1].  drop_masks: None or, per layer, None or the (f1, f2, f3) that layer drew."""
    B = imgs.shape[0]
    if layers is None:
        layers = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("transformer.resblocks."))
    x = embed(imgs, st, T)
    for i in range(layers):
        x = block(x, st, i, H, T, scale, window, prompt, None if drop_masks is None else drop_masks[i])
    D = x.shape[-1]
    y = F.layer_norm(x[:, 0], (D,), st["ln_post.weight"], st["ln_post.bias"], 1e-5)
    return y.view(B, T, D).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)


def masks_per_layer(stored, rates):
    """the reference's drawn masks in call order (three per block whose rate is > 0) -> one (f1, f2, f3) or None per layer"""
    out, k = [], 0
    for r in rates:
        if r > 0:
            out.append((stored[k], stored[k + 1], stored[k + 2]))
            k += 3
        else:
            out.append(None)
    assert k == len(stored)
    return out


def kernel_rows(B, T, G, window):
    """the window kernels' row-address rule (csrc/win_attn.hip, P = N) restated: [B nW, S] frame-major rows"""
    wt, wh, ww = clip_window(window, T, G)
    N = G * G + 1
    rows = []
    for b in range(B):
        for it in range(T // wt):
            for ih in range(G // wh):
                for iw in range(G // ww):
                    rows.append([(b * T + it * wt + i // (wh * ww)) * N + 1 + (ih * wh + (i % (wh * ww)) // ww) * G + iw * ww + i % ww
                                 for i in range(wt * wh * ww)])
    return torch.tensor(rows)
