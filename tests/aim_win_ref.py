"""Plain PyTorch restatement of the windowed AIM block and backbone (reference vitclip_aim.py:212-287, ``wind_attn=True``) in
the BOX form: test infrastructure, as tests/aim_flash_ref.py is for AIM_FLASH.  Written from the algebra, frame-major
([BT, tokens, D]), any float dtype, sequences taken by INDEX (no roll, no window view, no mask); autograd gives the gradients.

The reference rolls the [T, G, G] grid by minus the shift, attends inside whole windows of the rolled grid under an additive
-100 mask between the regions ``compute_mask`` numbers, and rolls back.  Here the grouping is a LABEL per grid cell in original
coordinates, every axis on its own, with (wt, wh, ww) the clipped window and (st, sh, sw) the shift:
    s = 0: x // w;     s > 0: 0 if x < s else 1 + (x - s) // w             (cut at 0, s, s + w, s + 2 w, ...; nothing wraps)
Cells with the same (clip, t label, h label, w label) attend to one another with plain softmax: a masked pair gets a weight of
exactly 0 where the reference leaves at most (S - 1) e^(spread - 100) (spread: the largest logit difference inside a window; the
fixtures record that mass, at most 1e-20).  ``t_wrap=True`` groups t as AIM_FLASH does instead (whole windows that start at st
and wrap round the clip's end, aim_flash_ref.box_index): the fixtures' ``t_wrap_effect``.
tests/test_aim_win_cpu.py holds this to the real reference's stored outputs and gradients (tests/golden/aim_win_tiny_*.npz) at
the oracle bound of 2e-5 rel-L2 and shows that the labels give the boxes of tests/win_attn_cut_cases.box_rows (the kernels'
address rule); tests/test_aim_win_gpu.py compares the HIP backbone to it at the recipes' real geometry.

Per block, x [BT, N, D] (token 0 = class, G = sqrt(N - 1)), d1 d2 the DropPath factors per TOKEN POSITION (or None):
  1. xl = ln_1(x)
  2. patch tokens: attn(xl) inside each window (even blocks) or box (odd blocks, by ``block_shift``)       -> windows_attn
  3. class tokens: attn(xl) over the T class tokens of each clip                                             -> cls_attn
  4. x = x + d1 T_Adapter([cls_attn, windows_attn])                                    (no adapter scale on this term)
  5. prompt: x' = [cls, cls_attn, patches];  x' = x' + sa + S_Adapter(sa), sa = attn(ln_1 x');  token 1 is dropped
  6. x = x + mlp(ln_2 x) + d2 scale MLP_Adapter(ln_2 x)
attn = out_proj(softmax(q k^T / sqrt(dh)) v) with in_proj (q | k | v, head-major); mlp = c_proj(QuickGELU(c_fc)).
"""
import os
import sys
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aim_flash_ref as FR  # noqa: E402
from aim_flash_ref import O, clip_shift, clip_window  # noqa: E402,F401

backbone_param_shapes = O.backbone_param_shapes          # AIM keeps ViT_CLIP's parameter names


def block_shift(i: int, window, T: int, G: int):
    """the shift of block i, or None for a block with plain windows"""
    s = clip_shift(window, T, G)
    return s if (i % 2 == 1 and any(s)) else None


def _axis_label(x, w, s):
    return torch.where(x < s, torch.zeros_like(x), 1 + (x - s) // w) if s else x // w


def cut_index(B, T, G, window, shift) -> List[torch.Tensor]:
    """the sequences of a block whose windows are cut at `shift` as indices into the flattened [B, T, G, G] patch grid: a list
    of [n, S] tensors, one per sequence length, tokens in (t, h, w) order"""
    wt, wh, ww = clip_window(window, T, G)
    st, sh, sw = shift
    if T % wt or G % wh or G % ww:
        raise ValueError(f"window {(wt, wh, ww)} does not divide the grid {(T, G, G)}")
    b, t, h, w = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(G), torch.arange(G), indexing="ij")
    nt, nh, nw = T // wt + 1, G // wh + 1, G // ww + 1
    label = (((b * nt + _axis_label(t, wt, st)) * nh + _axis_label(h, wh, sh)) * nw + _axis_label(w, ww, sw)).reshape(-1)
    inside = ((t * G + h) * G + w).reshape(-1)
    order = torch.argsort(label * (T * G * G) + inside)              # by sequence, then by (t, h, w) inside it
    counts = torch.bincount(label)
    counts = counts[counts > 0]
    by_S: Dict[int, list] = {}
    for seq in torch.split(order, counts.tolist()):
        by_S.setdefault(seq.numel(), []).append(seq)
    return [torch.stack(by_S[S]) for S in sorted(by_S)]


def _attention(xq, st, pre, H):
    """xq [Nb, S, D] -> out_proj(softmax(q k^T / sqrt(dh)) v)"""
    Nb, S, D = xq.shape
    qkv = F.linear(xq, st[pre + "attn.in_proj_weight"], st[pre + "attn.in_proj_bias"]).view(Nb, S, 3, H, D // H).permute(2, 0, 3, 1, 4)
    p = (qkv[0] @ qkv[1].transpose(-2, -1) / (D // H) ** 0.5).softmax(dim=-1)
    o = (p @ qkv[2]).permute(0, 2, 1, 3).reshape(Nb, S, D)
    return F.linear(o, st[pre + "attn.out_proj.weight"], st[pre + "attn.out_proj.bias"])


def block(x, st: Dict[str, torch.Tensor], i: int, H: int, T: int, scale: float, window, shift, prompt: bool = True, masks=None,
          t_wrap: bool = False):
    """x [BT, N, D] -> [BT, N, D].  shift: None or the block's (st, sh, sw); masks: None or the block's two DropPath factors per
    token position, each [N]."""
    pre = f"transformer.resblocks.{i}."
    BT, N, D = x.shape
    B, G = BT // T, int(round((N - 1) ** 0.5))
    ln1 = lambda t: F.layer_norm(t, (D,), st[pre + "ln_1.weight"], st[pre + "ln_1.bias"], 1e-5)
    f = (lambda k: 1.0) if masks is None else (lambda k: masks[k].to(x.dtype).view(1, N, 1))
    xl = ln1(x)
    patches = xl[:, 1:].reshape(BT * G * G, D)
    if shift is None:
        groups = [FR.R.window_index(B, T, G, window)]
    else:
        groups = FR.box_index(B, T, G, window, shift) if t_wrap else cut_index(B, T, G, window, shift)
    win = torch.zeros_like(patches)
    for idx in groups:
        wo = _attention(patches[idx.reshape(-1)].view(idx.shape[0], idx.shape[1], D), st, pre, H)
        win = win.index_add(0, idx.reshape(-1), wo.reshape(-1, D))                          # (a permutation)
    win = win.view(BT, G * G, D)
    cls_attn = _attention(xl[:, 0].view(B, T, D), st, pre, H).reshape(BT, 1, D)
    x = x + f(0) * O.ref_adapter(torch.cat([cls_attn, win], dim=1), st, pre + "T_Adapter")
    if prompt:
        x = torch.cat([x[:, :1], cls_attn, x[:, 1:]], dim=1)
    sa = _attention(ln1(x), st, pre, H)
    x = x + sa + O.ref_adapter(sa, st, pre + "S_Adapter")                                   # S_Adapter has its skip connection
    if prompt:
        x = torch.cat([x[:, :1], x[:, 2:]], dim=1)
    xn = F.layer_norm(x, (D,), st[pre + "ln_2.weight"], st[pre + "ln_2.bias"], 1e-5)
    h = F.linear(xn, st[pre + "mlp.c_fc.weight"], st[pre + "mlp.c_fc.bias"])
    h = F.linear(h * torch.sigmoid(1.702 * h), st[pre + "mlp.c_proj.weight"], st[pre + "mlp.c_proj.bias"])
    return x + h + f(1) * scale * O.ref_adapter(xn, st, pre + "MLP_Adapter")


def backbone(imgs, st, H: int, T: int, window, scale: float = 0.5, prompt: bool = True, drop_masks=None,
             layers: Optional[int] = None, not_shift: bool = False, t_wrap: bool = False):
    """[B, 3, T, h, w] -> [B, D, T, 1, 1].  drop_masks: None or, per layer, None or the (d1, d2) that layer drew."""
    B = imgs.shape[0]
    if layers is None:
        layers = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("transformer.resblocks."))
    x = FR.R.embed(imgs, st, T)
    G = int(round((x.shape[1] - 1) ** 0.5))
    for i in range(layers):
        x = block(x, st, i, H, T, scale, window, None if not_shift else block_shift(i, window, T, G), prompt,
                  None if drop_masks is None else drop_masks[i], t_wrap)
    D = x.shape[-1]
    y = F.layer_norm(x[:, 0], (D,), st["ln_post.weight"], st["ln_post.bias"], 1e-5)
    return y.view(B, T, D).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)


def masks_per_layer(stored, rates):
    """the reference's drawn masks in call order (two per block whose rate is > 0) -> one (d1, d2) or None per layer"""
    out, k = [], 0
    for r in rates:
        if r > 0:
            out.append((stored[k], stored[k + 1]))
            k += 2
        else:
            out.append(None)
    assert k == len(stored)
    return out
