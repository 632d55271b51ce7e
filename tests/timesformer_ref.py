"""Plain-torch restatement of the reference's TimeSformer backbone (mmaction/models/backbones/timesformer.py:57-71,192-225),
written from its algebra, in whatever dtype and on whatever device the parameters are; differentiable through torch autograd.
DropPath does not draw here: the factors come in as explicit vectors (0 or 1 / keep), so a test can replay the masks a
reference run drew (tests/golden/timesformer_tiny_b.npz) or draw its own.

Rows stay in the reference's layouts -- [N, BT, D] through the blocks, [T, B N, D] inside the temporal branch -- so that a
frame-index factor and a token-index factor are each a plain broadcast over dimension 0, as timm's DropPath applies them.
"""
import torch
import torch.nn.functional as F


def mha(x, w_in, b_in, w_out, b_out, heads):
    """nn.MultiheadAttention(x, x, x) on [S, batch, D] without mask or dropout"""
    S, Bn, D = x.shape
    hd = D // heads
    q, k, v = F.linear(x, w_in, b_in).chunk(3, dim=-1)
    sh = lambda t: t.reshape(S, Bn * heads, hd).transpose(0, 1)             # [batch * heads, S, hd]
    att = torch.softmax(sh(q) @ sh(k).transpose(1, 2) * hd ** -0.5, dim=-1)
    o = (att @ sh(v)).transpose(0, 1).reshape(S, Bn, D)
    return F.linear(o, w_out, b_out)


def block(x, P, pre, heads, T, f1=None, f2=None, f3=None):
    """x [N, BT, D] -> [N, BT, D].  f1 [T]: the factor per frame index, between t_attn.out_proj and T_Adapter; f2 / f3 [N]: per
    token index, on the spatial attention and on the MLP.  None = 1."""
    g = lambda n: P[pre + n]
    N, BT, D = x.shape
    B = BT // T
    ln = lambda t, n: F.layer_norm(t, (D,), g(n + ".weight"), g(n + ".bias"), 1e-5)
    xt = x.reshape(N, B, T, D).permute(2, 1, 0, 3).reshape(T, B * N, D)                    # 'n (b t) d -> t (b n) d'
    xt = mha(ln(xt, "t_norm"), g("t_attn.in_proj_weight"), g("t_attn.in_proj_bias"), g("t_attn.out_proj.weight"),
             g("t_attn.out_proj.bias"), heads)
    if f1 is not None:
        xt = xt * f1.to(xt.dtype).view(T, 1, 1)
    xt = F.linear(xt, g("T_Adapter.weight"), g("T_Adapter.bias"))
    x = x + xt.reshape(T, B, N, D).permute(2, 1, 0, 3).reshape(N, BT, D)                  # 't (b n) d -> n (b t) d'
    a = mha(ln(x, "ln_1"), g("attn.in_proj_weight"), g("attn.in_proj_bias"), g("attn.out_proj.weight"), g("attn.out_proj.bias"),
            heads)
    x = x + (a if f2 is None else a * f2.to(a.dtype).view(N, 1, 1))
    h = F.linear(ln(x, "ln_2"), g("mlp.c_fc.weight"), g("mlp.c_fc.bias"))
    m = F.linear(h * torch.sigmoid(1.702 * h), g("mlp.c_proj.weight"), g("mlp.c_proj.bias"))
    return x + (m if f3 is None else m * f3.to(m.dtype).view(N, 1, 1))


def forward(P, imgs, heads, patch, factors=None):
    """imgs [B, 3, T, H, W] -> [B, D, T, 1, 1].  ``P``: tensors by parameter name (a model without ``temporal_embedding`` adds
    none).  ``factors``: one ``(f1 [T], f2 [N], f3 [N])`` per layer, entries or the whole argument None = 1."""
    B, C, T, Hh, Ww = imgs.shape
    D = P["conv1.weight"].shape[0]
    L = 1 + max(int(k.split(".")[2]) for k in P if k.startswith("transformer.resblocks."))
    x = F.conv2d(imgs.permute(0, 2, 1, 3, 4).reshape(B * T, C, Hh, Ww).to(P["conv1.weight"].dtype), P["conv1.weight"], stride=patch)
    x = x.reshape(B * T, D, -1).permute(0, 2, 1)
    x = torch.cat([P["class_embedding"].expand(B * T, 1, D), x], dim=1) + P["positional_embedding"]
    N = x.shape[1]
    if "temporal_embedding" in P:
        x = (x.reshape(B, T, N, D) + P["temporal_embedding"].reshape(1, T, 1, D)).reshape(B * T, N, D)
    x = F.layer_norm(x, (D,), P["ln_pre.weight"], P["ln_pre.bias"], 1e-5).permute(1, 0, 2)
    for i in range(L):
        f = (None, None, None) if factors is None else factors[i]
        x = block(x, P, f"transformer.resblocks.{i}.", heads, T, *f)
    x = F.layer_norm(x.permute(1, 0, 2)[:, 0], (D,), P["ln_post.weight"], P["ln_post.bias"], 1e-5)
    return x.reshape(B, T, D).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)
