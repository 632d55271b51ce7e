"""Plain PyTorch restatement of ViT_CLIP_ZEROI2V at ``linear_adapter=True`` (reference vit_clip_zeroI2V.py:15-38, :153-206,
:244-311) and of the fold of its adapters into the frozen weights: test infrastructure, beside zeroi2v_ref.py (which it leaves
alone and imports the shared pieces from).  Frame-major ([BT, tokens, D]), any float dtype; autograd gives the gradients.
tests/test_zeroi2v_linear_cpu.py holds it to the real reference's stored outputs and gradients
(tests/golden/zeroi2v_linear_tiny_*.npz); tests/test_zeroi2v_linear_gpu.py compares the HIP backbone to it.

LA(x) = x + D_fc2(D_fc1(x)), no activation.  Per block, x [BT, N, D] (token 0 = class):
  1. with_t_cls_token: xt = T_Adapter(attention over the T class tokens of a clip (ln_1(cls))) with the UN-ADAPTED in_proj /
     out_proj and the GELU T_Adapter; x' = [cls, xt, patches]
  2. xln = ln_1(x'); q, k, v = Wq LA_q(xln) + bq, Wk LA_k(xln) + bk, Wv LA_v(xln) + bv  (share_adapter: one LA_in for the three);
     head-shifted attention; x'1 = x' + out_proj(LA_out(attn)).  No S_Adapter, no DropPath, no adapter scale.
  3. token 1 is dropped; xn = ln_2(x1)
  4. m = mlp(xn + LA_in(xn)); x2 = x1 + m + LA_out(m): both MLP adapters' skip is DOUBLED, as the reference writes it.

Fold, with A = c I + W2 W1 and d = W2 b1 + b2 (c = 1 for the attention adapters, 2 for the two MLP adapters):
  W_{q,k,v}' = W A, b' = b + W d;  W_o' = W_o A, b_o' = b_o + W_o d;  W_fc' = W_fc A, b_fc' = b_fc + W_fc d;
  W_proj' = A W_proj, b_proj' = A b_proj + d.
The class chain of step 1 keeps the original attention weights: ``fold`` stores them beside the folded ones.
"""
import os
import sys
from typing import Dict, Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zeroi2v_ref as Z  # noqa: E402
from oracle import vit_clip_oracle as O  # noqa: E402


def adapter_names(share_adapter: bool, with_t_cls_token: bool):
    """a block's adapters in the reference's construction order (:109-136)"""
    attn = ("Attn_Adapter_in",) if share_adapter else ("Attn_Adapter_q", "Attn_Adapter_k", "Attn_Adapter_v")
    return (("T_Adapter",) if with_t_cls_token else ()) + attn + ("Attn_Adapter_out", "MLP_Adapter_in", "MLP_Adapter_out")


def backbone_param_shapes(res, T, patch, width, layers, with_t_cls_token=True, share_adapter=False, bottleneck=192):
    s = {k: v for k, v in O.backbone_param_shapes(res, T, patch, width, layers).items() if "Adapter" not in k}
    D = width
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        for a in adapter_names(share_adapter, with_t_cls_token):
            r = int(D * 0.25) if a == "T_Adapter" else bottleneck
            s[p + a + ".D_fc1.weight"], s[p + a + ".D_fc1.bias"] = (r, D), (r,)
            s[p + a + ".D_fc2.weight"], s[p + a + ".D_fc2.bias"] = (D, r), (D,)
    return s


def la(x, st, pre, skip: float = 1.0):
    """Linear_Adapter.forward (:33-38); skip = 0: only the low-rank term"""
    h = F.linear(x, st[pre + ".D_fc1.weight"], st[pre + ".D_fc1.bias"])
    return skip * x + F.linear(h, st[pre + ".D_fc2.weight"], st[pre + ".D_fc2.bias"])


def _ths_attention(xs, W, b, Wo, bo, H, T, shifts, out_adapter):
    """xs = (xq, xk, xv) [Nb, S, D] -> out_proj(out_adapter(softmax(q k^T / sqrt(dh)) v)) (:153-206)"""
    Nb, S, D = xs[0].shape
    q, k, v = (F.linear(x, W[j * D:(j + 1) * D], b[j * D:(j + 1) * D]).view(Nb, S, H, D // H).permute(0, 2, 1, 3)
               for j, x in enumerate(xs))
    if shifts is not None and any(shifts):
        k, v = Z.head_shift(k, T, shifts), Z.head_shift(v, T, shifts)
    p = (q @ k.transpose(-2, -1) / (D // H) ** 0.5).softmax(dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(Nb, S, D)
    return F.linear(out_adapter(o), Wo, bo)


def block(x, st: Dict[str, torch.Tensor], i: int, H: int, T: int, with_t_cls_token: bool, share_adapter: bool,
          shift: bool = True, attn_identity: bool = False, mlp_identity: bool = False, single_skip: bool = False,
          folded: bool = False):
    """x [BT, N, D] -> [BT, N, D].  attn_identity / mlp_identity: those adapters replaced by the identity; single_skip: the two
    MLP adapters contribute only their low-rank term (the skip is counted once).  folded: `st` is ``fold``'s result -- no
    adapter is evaluated, the class chain reads the weights kept under ``attn_cls.``."""
    pre = f"transformer.resblocks.{i}."
    BT, N, D = x.shape
    ln1 = lambda t: F.layer_norm(t, (D,), st[pre + "ln_1.weight"], st[pre + "ln_1.bias"], 1e-5)
    W, b = st[pre + "attn.in_proj_weight"], st[pre + "attn.in_proj_bias"]
    Wo, bo = st[pre + "attn.out_proj.weight"], st[pre + "attn.out_proj.bias"]
    ident = lambda t: t
    if with_t_cls_token:
        c = "attn_cls." if folded else "attn."
        cls = ln1(x[:, 0]).view(BT // T, T, D)
        a = _ths_attention((cls, cls, cls), st[pre + c + "in_proj_weight"], st[pre + c + "in_proj_bias"],
                           st[pre + c + "out_proj.weight"], st[pre + c + "out_proj.bias"], H, T, None, ident)
        xt = O.ref_adapter(a, st, pre + "T_Adapter").reshape(BT, 1, D)
        x = torch.cat([x[:, :1], xt, x[:, 1:]], dim=1)
    xln = ln1(x)
    plain = folded or attn_identity
    if plain:
        xs = (xln, xln, xln)
    elif share_adapter:
        xs = (la(xln, st, pre + "Attn_Adapter_in"),) * 3
    else:
        xs = tuple(la(xln, st, pre + "Attn_Adapter_" + n) for n in "qkv")
    shifts = Z.head_shifts(T, H) if shift else None
    x = x + _ths_attention(xs, W, b, Wo, bo, H, T, shifts, ident if plain else (lambda o: la(o, st, pre + "Attn_Adapter_out")))
    if with_t_cls_token:
        x = torch.cat([x[:, :1], x[:, 2:]], dim=1)
    xn = F.layer_norm(x, (D,), st[pre + "ln_2.weight"], st[pre + "ln_2.bias"], 1e-5)
    mlp = lambda t: F.linear(O.ref_quick_gelu(F.linear(t, st[pre + "mlp.c_fc.weight"], st[pre + "mlp.c_fc.bias"])),
                             st[pre + "mlp.c_proj.weight"], st[pre + "mlp.c_proj.bias"])
    if folded:
        return x + mlp(xn)
    skip = 0.0 if single_skip else 1.0
    ain = (lambda t: t) if mlp_identity else (lambda t: la(t, st, pre + "MLP_Adapter_in", skip))
    aout = (lambda t: t) if mlp_identity else (lambda t: la(t, st, pre + "MLP_Adapter_out", skip))
    m = mlp(xn + ain(xn))
    return x + m + aout(m)


def backbone(imgs, st, H: int, T: int, with_t_cls_token: bool = True, share_adapter: bool = False,
             layers: Optional[int] = None, **block_kw):
    """[B, 3, T, h, w] -> [B, D, T, 1, 1]"""
    B = imgs.shape[0]
    if layers is None:
        layers = 1 + max(int(k.split(".")[2]) for k in st if k.startswith("transformer.resblocks."))
    x = Z.embed(imgs, st, T)
    for i in range(layers):
        x = block(x, st, i, H, T, with_t_cls_token, share_adapter, **block_kw)
    D = x.shape[-1]
    y = F.layer_norm(x[:, 0], (D,), st["ln_post.weight"], st["ln_post.bias"], 1e-5)
    return y.view(B, T, D).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)


def fold_pair(st, pre, c: float):
    """(A, d) of one adapter: LA-with-skip-c (x) = A x + d"""
    W1, b1 = st[pre + ".D_fc1.weight"], st[pre + ".D_fc1.bias"]
    W2, b2 = st[pre + ".D_fc2.weight"], st[pre + ".D_fc2.bias"]
    D = W2.shape[0]
    return c * torch.eye(D, dtype=W1.dtype) + W2 @ W1, W2 @ b1 + b2


def fold(st, layers: int, with_t_cls_token: bool, share_adapter: bool, cls_in_place: bool = False):
    """The state dict of the merged model: every linear adapter folded into the frozen weight beside it and removed.  The
    class chain's original attention weights are kept under ``attn_cls.`` -- or, with ``cls_in_place`` (the mistake the tests
    must be able to see), replaced by the folded ones."""
    out = {k: v for k, v in st.items() if "Attn_Adapter" not in k and "MLP_Adapter" not in k}
    for i in range(layers):
        pre = f"transformer.resblocks.{i}."
        W, b = st[pre + "attn.in_proj_weight"], st[pre + "attn.in_proj_bias"]
        D = W.shape[1]
        Ws, bs = [], []
        for j, n in enumerate("qkv"):
            A, d = fold_pair(st, pre + "Attn_Adapter_" + ("in" if share_adapter else n), 1.0)
            Wj, bj = W[j * D:(j + 1) * D], b[j * D:(j + 1) * D]
            Ws.append(Wj @ A)
            bs.append(bj + Wj @ d)
        out[pre + "attn.in_proj_weight"], out[pre + "attn.in_proj_bias"] = torch.cat(Ws), torch.cat(bs)
        A, d = fold_pair(st, pre + "Attn_Adapter_out", 1.0)
        Wo, bo = st[pre + "attn.out_proj.weight"], st[pre + "attn.out_proj.bias"]
        out[pre + "attn.out_proj.weight"], out[pre + "attn.out_proj.bias"] = Wo @ A, bo + Wo @ d
        A, d = fold_pair(st, pre + "MLP_Adapter_in", 2.0)
        Wf, bf = st[pre + "mlp.c_fc.weight"], st[pre + "mlp.c_fc.bias"]
        out[pre + "mlp.c_fc.weight"], out[pre + "mlp.c_fc.bias"] = Wf @ A, bf + Wf @ d
        A, d = fold_pair(st, pre + "MLP_Adapter_out", 2.0)
        Wp, bp = st[pre + "mlp.c_proj.weight"], st[pre + "mlp.c_proj.bias"]
        out[pre + "mlp.c_proj.weight"], out[pre + "mlp.c_proj.bias"] = A @ Wp, A @ bp + d
        if with_t_cls_token:
            for leaf in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
                out[pre + "attn_cls." + leaf] = (out if cls_in_place else st)[pre + "attn." + leaf]
    return out
