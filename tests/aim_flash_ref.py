"""Plain PyTorch restatement of the AIM_FLASH block and backbone (reference vitclip_aim_flash.py, ``wind_attn=True``,
``win_prompt=False``): test infrastructure that builds on tests/aim_flash_win_ref.py (same embedding, attention, adapters,
prompt step and readout) and differs in ONE thing: the sequences of the patch-token attention of a shifted block.

The reference rolls the [T, G, G] grid by minus the shift, cuts strips off the rolled grid's border, attends inside every
piece, stitches and rolls back.  Here the same grouping is a LABEL per grid cell in original coordinates (no roll, no slice,
no cat), each axis on its own, with (wt, wh, ww) the clipped window and (st, sh, sw) the shift:
    t:  window ((t - st) mod T) // wt, position ((t - st) mod T) % wt inside it          (whole windows, the last one wraps)
    h:  sh = 0: h // wh;   sh > 0: 0 if h < sh else 1 + (h - sh) // wh                  (cut at 0, sh, sh + wh, ...; no wrap)
    w:  as h
Cells with the same (clip, t label, h label, w label) attend to one another; inside a sequence they are ordered by (position
in the t window, h, w).  tests/test_aim_flash_cpu.py holds this to the real reference's stored outputs and gradients
(tests/golden/aim_flash_tiny_*.npz) at the oracle bound of 2e-5 rel-L2 and shows that the labels give the boxes of
tests/win_attn_shift_cases.box_rows (the kernels' address rule); tests/test_aim_flash_gpu.py compares the HIP backbone to it
at the recipes' real geometry.

Block i is shifted when ``i % 2 == 1 and not not_shift`` by ``window_size[k] // 2``, zeroed on every axis where the grid does
not exceed the window; an unshifted block is aim_flash_win_ref.block.
"""
import os
import sys
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aim_flash_win_ref as R  # noqa: E402
from aim_flash_win_ref import O, backbone_param_shapes, clip_window, masks_per_layer  # noqa: E402,F401


def clip_shift(window, T, G):
    """half a window, 0 on every axis where the grid does not exceed the window (the reference's get_window_size)"""
    return tuple(0 if x <= w else w // 2 for w, x in zip(window, (T, G, G)))


def block_shift(i: int, window, T: int, G: int, not_shift: bool = False):
    """the shift of block i, or None for an unshifted block"""
    s = clip_shift(window, T, G)
    return s if (i % 2 == 1 and not not_shift and any(s)) else None


def box_index(B, T, G, window, shift) -> List[torch.Tensor]:
    """the sequences of a shifted block as indices into the flattened [B, T, G, G] patch grid: a list of [n, S] tensors, one
    per sequence length, from the labels of the module docstring"""
    wt, wh, ww = clip_window(window, T, G)
    st, sh, sw = shift
    if T % wt or G % wh or G % ww:
        raise ValueError(f"window {(wt, wh, ww)} does not divide the grid {(T, G, G)}")
    b, t, h, w = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(G), torch.arange(G), indexing="ij")
    tr = (t - st) % T
    lab_h = torch.where(h < sh, torch.zeros_like(h), 1 + (h - sh) // wh) if sh else h // wh
    lab_w = torch.where(w < sw, torch.zeros_like(w), 1 + (w - sw) // ww) if sw else w // ww
    nh, nw = G // wh + 1, G // ww + 1
    label = (((b * (T // wt) + tr // wt) * nh + lab_h) * nw + lab_w).reshape(-1)
    inside = (((tr % wt) * G + h) * G + w).reshape(-1)
    order = torch.argsort(label * (wt * G * G) + inside)             # by sequence, then by (dt, h, w) inside it
    counts = torch.bincount(label)
    counts = counts[counts > 0]
    by_S: Dict[int, list] = {}
    for seq in torch.split(order, counts.tolist()):
        by_S.setdefault(seq.numel(), []).append(seq)
    return [torch.stack(by_S[S]) for S in sorted(by_S)]


def block(x, st: Dict[str, torch.Tensor], i: int, H: int, T: int, scale: float, window, shift, prompt: bool = True, masks=None):
    """aim_flash_win_ref.block with the patch-token attention inside the sequences of `box_index` (shift not None)"""
    if shift is None:
        return R.block(x, st, i, H, T, scale, window, prompt, masks)
    pre = f"transformer.resblocks.{i}."
    BT, N, D = x.shape
    B, G = BT // T, int(round((N - 1) ** 0.5))
    ln1 = lambda t: F.layer_norm(t, (D,), st[pre + "ln_1.weight"], st[pre + "ln_1.bias"], 1e-5)
    f = (lambda k: 1.0) if masks is None else (lambda k: masks[k].to(x.dtype).view(BT, 1, 1))
    xl = ln1(x)
    patches = xl[:, 1:].reshape(BT * G * G, D)
    win = torch.zeros_like(patches)
    for idx in box_index(B, T, G, window, shift):
        wo = R._attention(patches[idx.reshape(-1)].view(idx.shape[0], idx.shape[1], D), st, pre, H)
        win = win.index_add(0, idx.reshape(-1), wo.reshape(-1, D))
    win = win.view(BT, G * G, D)
    cls_attn = R._attention(xl[:, 0].view(B, T, D), st, pre, H).reshape(BT, 1, D)
    x = x + f(0) * O.ref_adapter(torch.cat([cls_attn, win], dim=1), st, pre + "T_Adapter")
    if prompt:
        x = torch.cat([x[:, :1], cls_attn, x[:, 1:]], dim=1)
    x = x + R._attention(ln1(x), st, pre, H) + f(1) * scale * O.ref_adapter(x, st, pre + "S_Adapter")
    if prompt:
        x = torch.cat([x[:, :1], x[:, 2:]], dim=1)
    xn = F.layer_norm(x, (D,), st[pre + "ln_2.weight"], st[pre + "ln_2.bias"], 1e-5)
    h = F.linear(xn, st[pre + "mlp.fc1.weight"], st[pre + "mlp.fc1.bias"])
    h = F.linear(h * torch.sigmoid(1.702 * h), st[pre + "mlp.fc2.weight"], st[pre + "mlp.fc2.bias"])
    return x + h + f(2) * scale * O.ref_adapter(xn, st, pre + "MLP_Adapter")


def backbone(imgs, st, H: int, T: int, window, scale: float = 0.5, prompt: bool = True, drop_masks=None,
             layers: Optional[int] = None, not_shift: bool = False):
    """[B, 3, T, h, w] -> [B, D, T, 1, 1].  drop_masks: None or, per layer, None or the (f1, f2, f3) that layer drew."""
    B = imgs.shape[0]
    if layers is None:
        layers = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("transformer.resblocks."))
    x = R.embed(imgs, st, T)
    G = int(round((x.shape[1] - 1) ** 0.5))
    for i in range(layers):
        x = block(x, st, i, H, T, scale, window, block_shift(i, window, T, G, not_shift), prompt,
                  None if drop_masks is None else drop_masks[i])
    D = x.shape[-1]
    y = F.layer_norm(x[:, 0], (D,), st["ln_post.weight"], st["ln_post.bias"], 1e-5)
    return y.view(B, T, D).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)
