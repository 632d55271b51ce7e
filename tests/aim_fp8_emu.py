"""CPU emulation of stock AIM's fp8 inference forward (aim_variant._aim_block_forward_f8) at its rounding points, built from
the oracle's public pieces (``q8``, ``q8_rows``, ``BF16``, ``emu_embed``, ``emu_adapter``).

Rounding points of the fp8 block ("fp8 inference of the stock block"):
  * the A operand of every fp8 GEMM is the saturating e4m3 cast of the producing kernel's fp32 result -- ln_1 (twice), the
    temporal attention, the spatial attention, ln_2, the [c_fc ; D_fc1] activations -- never of a bf16 intermediate;
  * weights are quantised per output channel (one scale per row of W; [c_fc ; D_fc1] and [c_proj | D_fc2] concatenated);
  * ``qkv`` (both), ``ta`` and ``sa`` are stored as bf16; T_Adapter and S_Adapter are the bf16 GEMMs of the bf16 block;
  * the residual stream is fp32 (no rounding of x1, x2, x3).
With ``f8=False`` every step is the one of ``oracle.vit_clip_oracle.emu_aim_block(rnd=BF16)``, in its order.

``mutant`` rewires one step (tests/test_aim_fp8_cpu.py shows that each of them moves the output past the GPU test's bound).
"""
import math
from typing import Optional

import torch
import torch.nn.functional as F

from oracle import vit_clip_oracle as O

R = O.BF16

# the model cases of tests/test_aim_fp8_gpu.py: (res, T, patch, D, H, B), two layers, and the seeds of weights and clips
CASES = {"B16_L2": (224, 4, 16, 768, 12, 2), "L14_L2": (224, 4, 14, 1024, 16, 1)}
LAYERS, SEED_W, SEED_X = 2, 81, 82
MUTANTS = ("no_s_skip", "no_temporal", "per_tensor_scale", "ot_unquantised", "ln1_of_x")


def case_inputs(arch):
    """(state dict, clips [B, 3, T, res, res]) of a model case"""
    res, T, patch, D, H, B = CASES[arch]
    st = O.synth_state_dict(O.backbone_param_shapes(res, T, patch, D, LAYERS), seed=SEED_W)
    imgs = torch.randn((B, 3, T, res, res), generator=torch.Generator().manual_seed(SEED_X))
    return st, imgs


def _lin(a, w, b):
    """bf16-operand / fp32-accumulate GEMM"""
    return F.linear(R(a), R(w), b)


def _quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def emu_aim_block_f8(x, st, i: int, heads: int, T: int, scale: float = 0.5, f8: bool = True, mutant: Optional[str] = None):
    """x [BT, N, D] fp32 -> the block's output (eval mode: no DropPath)"""
    assert mutant is None or (f8 and mutant in MUTANTS)
    pre = f"transformer.resblocks.{i}."
    BT, N, D = x.shape
    B = BT // T
    dh = D // heads
    W, bqkv = st[pre + "attn.in_proj_weight"], st[pre + "attn.in_proj_bias"]
    Wo, bo = st[pre + "attn.out_proj.weight"], st[pre + "attn.out_proj.bias"]

    def rows8(w):
        if mutant == "per_tensor_scale":
            sc = (w.abs().amax().clamp_min(1e-12) / 448.0).expand(w.shape[0])
            return O.q8(w / sc[:, None]), sc
        return O.q8_rows(w)

    def lin(a_f32, w, b):
        """a large GEMM of the block: fp8 operands cast from fp32 (f8), or bf16 operands"""
        if not f8:
            return _lin(R(a_f32), w, b)
        w8, sc = rows8(w)
        return F.linear(O.q8(a_f32), w8) * sc + (0 if b is None else b)

    ln1 = lambda t: F.layer_norm(t, (D,), st[pre + "ln_1.weight"], st[pre + "ln_1.bias"], 1e-5)

    def attn(q, k, v):          # [..., S, heads*dh] over the second-to-last axis
        sh = q.shape[:-1]
        qh, kh, vh = (t.reshape(*sh, heads, dh).transpose(-2, -3) for t in (q, k, v))
        p = ((qh @ kh.transpose(-1, -2)) / math.sqrt(dh)).softmax(-1)
        return (p @ vh).transpose(-2, -3).reshape(*sh, heads * dh)

    # temporal: sequence = frames, batch = (clip, token)
    qkv = R(lin(ln1(x), W, bqkv)).reshape(B, T, N, 3 * D).permute(0, 2, 1, 3)      # [B, N, T, 3D]
    ot_f = attn(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:])                 # [B, N, T, D] fp32
    ot_f = ot_f.permute(0, 2, 1, 3).reshape(BT, N, D)
    if mutant == "ot_unquantised":
        ta = R(_lin(R(ot_f), Wo, bo))
    else:
        ta = R(lin(ot_f, Wo, bo))
    tp = pre + "T_Adapter"
    t_pre = R(_lin(ta, st[tp + ".D_fc1.weight"], st[tp + ".D_fc1.bias"]))
    t_hs = R(1.0 * F.gelu(t_pre))
    x1 = x + _lin(t_hs, st[tp + ".D_fc2.weight"], None) + 1.0 * st[tp + ".D_fc2.bias"]
    if mutant == "no_temporal":
        x1 = x
    # spatial, S_Adapter with skip
    qkv2 = R(lin(ln1(x if mutant == "ln1_of_x" else x1), W, bqkv))
    q, k, v = qkv2[..., :D], qkv2[..., D:2 * D], qkv2[..., 2 * D:]
    qh = q.reshape(BT, N, heads, dh).permute(0, 2, 1, 3)
    kh = k.reshape(BT, N, heads, dh).permute(0, 2, 1, 3)
    vh = v.reshape(BT, N, heads, dh).permute(0, 2, 1, 3)
    sc = (qh @ kh.transpose(-1, -2)) / math.sqrt(dh)
    pu = torch.exp(sc - sc.amax(dim=-1, keepdim=True))          # un-normalised, max 1 (what the kernel rounds)
    ao_f = ((R(pu) @ vh) / pu.sum(dim=-1, keepdim=True)).permute(0, 2, 1, 3).reshape(BT, N, D)
    sa = R(lin(ao_f, Wo, bo))
    x2 = x1 + sa + O.emu_adapter(sa, st, pre + "S_Adapter", R)
    if mutant == "no_s_skip":
        x2 = x2 - sa
    # MLP + MLP_Adapter
    xn_f = F.layer_norm(x2, (D,), st[pre + "ln_2.weight"], st[pre + "ln_2.bias"], 1e-5)
    mp = pre + "MLP_Adapter"
    if f8:
        # as emu_block's f8 branch, without the rounding of the stream: concatenated operands, one scale per output channel
        h = _quick_gelu(lin(xn_f, st[pre + "mlp.c_fc.weight"], st[pre + "mlp.c_fc.bias"]))
        a = scale * F.gelu(lin(xn_f, st[mp + ".D_fc1.weight"], st[mp + ".D_fc1.bias"]))
        wcat2 = torch.cat([st[pre + "mlp.c_proj.weight"], st[mp + ".D_fc2.weight"]], dim=1)
        return x2 + lin(torch.cat([h, a], dim=-1), wcat2, None) + st[pre + "mlp.c_proj.bias"] + scale * st[mp + ".D_fc2.bias"]
    xn = R(xn_f)
    hpre = R(_lin(xn, st[pre + "mlp.c_fc.weight"], st[pre + "mlp.c_fc.bias"]))
    h = R(_quick_gelu(hpre))
    mlp = _lin(h, st[pre + "mlp.c_proj.weight"], st[pre + "mlp.c_proj.bias"])
    a_pre = R(_lin(xn, st[mp + ".D_fc1.weight"], st[mp + ".D_fc1.bias"]))
    a_s = R(1.0 * scale * F.gelu(a_pre))
    return x2 + mlp + _lin(a_s, st[mp + ".D_fc2.weight"], None) + 1.0 * scale * st[mp + ".D_fc2.bias"]


def emu_aim_backbone_f8(imgs, st, heads: int, scale: float = 0.5, f8: bool = True, mutant: Optional[str] = None,
                        layers: Optional[int] = None):
    """[B, 3, T, H, W] -> [B, D, T, 1, 1], as ``oracle.vit_clip_oracle.emu_aim_backbone`` (eval mode)"""
    B, _, T = imgs.shape[:3]
    if layers is None:
        layers = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("transformer.resblocks."))
    x = O.emu_embed(imgs, st, R)
    for i in range(layers):
        x = emu_aim_block_f8(x, st, i, heads, T, scale, f8=f8, mutant=mutant)
    c = F.layer_norm(x[:, 0], (x.shape[-1],), st["ln_post.weight"], st["ln_post.bias"], 1e-5)
    return c.reshape(B, T, -1).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)
