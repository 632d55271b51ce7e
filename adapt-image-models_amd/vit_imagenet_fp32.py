"""Reference-precision mode of ``ViT_ImageNet`` (``set_precision('fp32')``): the block algebra of ``vit_imagenet.py`` on fp32
operands and the fp32 kernels (csrc/fp32.hip: f32 MFMA GEMMs, exact erf; the fp32 forms of ``aim_embed_nopre_fwd/bwd`` and
``aim_layernorm_gb_bwd``), forward and the same hand-written backward, every parameter's gradient included.  It is held to the
reference's own fp32 outputs and autograd gradients at 1e-5 (tests/test_vit_imagenet_gpu.py), which is what pins the model's
numerics (LayerNorm eps 1e-6, erf GELU on the frozen MLP, per-frame DropPath, T_Adapter_in) below bf16 noise.

One stream, operands built from the current parameters on every call (nothing cached), plain autograd outputs: a verification
mode, not a fast path (the f32 MFMA runs at 1/16 of the bf16 rate).  Same structure as ``fp32_path.aim_block_forward_f32``.
"""
import torch

from . import ops
from .fp32_path import _e, _f

F32 = torch.float32


class _Block32:
    """fp32 operands of one ViT_ImageNet block; transposes (dgrad operands) on first use."""

    def __init__(self, blk):
        a, ma = blk.attn, blk.MLP_Adapter
        D = blk.norm1.normalized_shape[0]
        dev = a.qkv.weight.device
        self.eps = float(blk.norm1.eps)
        self.Wqkv = _f(a.qkv.weight)
        self.bqkv = _f(a.qkv.bias) if a.qkv.bias is not None else torch.zeros(3 * D, dtype=F32, device=dev)
        self.Wo, self.bo = _f(a.proj.weight), _f(a.proj.bias)
        self.g1, self.b1, self.g2, self.b2 = _f(blk.norm1.weight), _f(blk.norm1.bias), _f(blk.norm2.weight), _f(blk.norm2.bias)
        self.Wcat1 = torch.cat([_f(blk.mlp.fc1.weight), _f(ma.D_fc1.weight)], 0).contiguous()
        self.bcat1 = torch.cat([_f(blk.mlp.fc1.bias), _f(ma.D_fc1.bias)], 0).contiguous()
        self.Wcat2 = torch.cat([_f(blk.mlp.fc2.weight), _f(ma.D_fc2.weight)], 1).contiguous()
        self.bpr, self.b2row = _f(blk.mlp.fc2.bias), _f(ma.D_fc2.bias).reshape(1, -1)
        self.ad = {n: tuple(_f(t) for t in (getattr(blk, n).D_fc1.weight, getattr(blk, n).D_fc1.bias,
                                            getattr(blk, n).D_fc2.weight, getattr(blk, n).D_fc2.bias))
                   for n in ("S_Adapter", "T_Adapter", "T_Adapter_in") if hasattr(blk, n)}
        self.r = ma.D_fc1.weight.shape[0]
        self._t = {}

    def t(self, name):
        if name not in self._t:
            self._t[name] = getattr(self, name).t().contiguous()
        return self._t[name]


def _colsum(g, db, w=None, ntok=0):
    """db += sum_m g[m] (w: per-frame weights w[m // ntok]) with the ordered fp32 frame sums (no atomics)."""
    M, C = g.shape
    if w is None:
        s = _e((1, C), g.device)
        ops.frame_sum(g.contiguous(), None, s, 1, M, C)
    else:
        frames = M // ntok
        per = _e((frames, C), g.device)
        ops.frame_sum(g.contiguous(), None, per, frames, ntok, C)
        s = _e((1, C), g.device)
        ops.frame_sum(per, w, s, 1, frames, C)
    db.add_(s.view(-1))


def _wgrad(g, a, G, wname, bname):
    dw, db = G.get(wname), G.get(bname)
    if dw is not None:
        ops.wgrad_f32(g, a, dw, db)
    elif db is not None:
        _colsum(g, db)


def block_forward_f32(x, w: _Block32, B, T, N, H, dp1, dms2, save: bool):
    """x [B*T*N, D] f32 -> x3; the steps of ``vit_imagenet._block_forward`` in fp32."""
    dev = x.device
    M, D = x.shape
    BT, r, eps = B * T, w.r, w.eps
    tw1, tb1, tw2, tb2 = w.ad["T_Adapter"]
    sw1, sb1, sw2, sb2 = w.ad["S_Adapter"]
    st = (lambda: _e((M,), dev)) if save else (lambda: None)
    # temporal adaptation: norm1 -> [T_Adapter_in, with skip] -> qkv -> attention over frames -> proj -> T_Adapter -> drop_path
    xl, mean1, rstd1 = _e((M, D), dev), st(), st()
    ops.layernorm_fwd(x, w.g1, w.b1, M, D, D, y_f32=xl, mean=mean1, rstd=rstd1, eps=eps)
    tin = tin_pre = tin_h = None
    if "T_Adapter_in" in w.ad:
        iw1, ib1, iw2, ib2 = w.ad["T_Adapter_in"]
        tin_h, tin_pre = _e((M, r), dev), _e((M, r), dev)
        ops.gemm_f32(xl, iw1, ops.EPI_ACT, tin_h, bias=ib1, act=ops.ACT_GELU, out2=tin_pre)
        tin = _e((M, D), dev)
        ops.gemm_f32(tin_h, iw2, ops.EPI_F32, tin, bias=ib2, resid=xl)
    qin = tin if tin is not None else xl
    qkv_t = _e((M, 3 * D), dev)
    ops.gemm_f32(qin, w.Wqkv, ops.EPI_BF16, qkv_t, bias=w.bqkv)
    ot = _e((M, D), dev)
    ops.tattn_fwd_f32(qkv_t, ot, B, T, N, H)
    ta = _e((M, D), dev)
    ops.gemm_f32(ot, w.Wo, ops.EPI_BF16, ta, bias=w.bo)
    t_hs, t_pre = _e((M, r), dev), _e((M, r), dev)          # dp1[f] * GELU(ta W1^T + b1)
    ops.gemm_f32(ta, tw1, ops.EPI_ACT, t_hs, bias=tb1, act=ops.ACT_GELU, af=dp1, ntok=N, out2=t_pre)
    x1 = _e((M, D), dev)
    ops.gemm_f32(t_hs, tw2, ops.EPI_F32, x1, resid=x, vec=dp1[:, None] * tb2[None, :], ntok=N)
    # spatial adaptation: norm1 -> qkv -> attention over tokens -> proj -> S_Adapter WITH its skip
    xl2, mean1b, rstd1b = _e((M, D), dev), st(), st()
    ops.layernorm_fwd(x1, w.g1, w.b1, M, D, D, y_f32=xl2, mean=mean1b, rstd=rstd1b, eps=eps)
    qkv_s = _e((M, 3 * D), dev)
    ops.gemm_f32(xl2, w.Wqkv, ops.EPI_BF16, qkv_s, bias=w.bqkv)
    ao = _e((M, D), dev)
    ops.attn_fwd_f32(qkv_s, ao, BT, N, H)
    sa, x1sa = _e((M, D), dev), _e((M, D), dev)
    ops.gemm_f32(ao, w.Wo, ops.EPI_BF16, sa, bias=w.bo)
    ops.gemm_f32(ao, w.Wo, ops.EPI_F32, x1sa, bias=w.bo, resid=x1)        # x1 + sa (the skip), by the same kernel
    s_h, s_pre = _e((M, r), dev), _e((M, r), dev)
    ops.gemm_f32(sa, sw1, ops.EPI_ACT, s_h, bias=sb1, act=ops.ACT_GELU, out2=s_pre)
    x2 = _e((M, D), dev)
    ops.gemm_f32(s_h, sw2, ops.EPI_F32, x2, bias=sb2, resid=x1sa)
    del x1sa
    # joint adaptation: [GELU(fc1) | dms2[f] GELU(D_fc1)] then [fc2 | D_fc2] + fc2.bias + dms2[f] D_fc2.bias
    xn, mean2, rstd2 = _e((M, D), dev), st(), st()
    ops.layernorm_fwd(x2, w.g2, w.b2, M, D, D, y_f32=xn, mean=mean2, rstd=rstd2, eps=eps)
    hcat, hcat_pre = _e((M, 4 * D + r), dev), _e((M, 4 * D + r), dev)
    ops.gemm_f32(xn, w.Wcat1, ops.EPI_ACT, hcat, bias=w.bcat1, act=ops.ACT_GELU, n_split=4 * D, act2=ops.ACT_GELU, af=dms2, ntok=N,
                 out2=hcat_pre)
    x3 = _e((M, D), dev)
    ops.gemm_f32(hcat, w.Wcat2, ops.EPI_F32, x3, bias=w.bpr, resid=x2, vec=dms2[:, None] * w.b2row, ntok=N)
    if not save:
        return x3, None
    return x3, dict(x=x, mean1=mean1, rstd1=rstd1, xl=xl, tin=tin, tin_pre=tin_pre, tin_h=tin_h, qkv_t=qkv_t, ot=ot, ta=ta,
                    t_pre=t_pre, t_hs=t_hs, x1=x1, mean1b=mean1b, rstd1b=rstd1b, xl2=xl2, qkv_s=qkv_s, ao=ao, sa=sa, s_pre=s_pre,
                    s_h=s_h, x2=x2, mean2=mean2, rstd2=rstd2, xn=xn, hcat=hcat, hcat_pre=hcat_pre, dp1=dp1, dms2=dms2)


def block_backward_f32(dy, c, w: _Block32, G, B, T, N, H):
    """d(loss)/d(x3) -> d(loss)/d(x); the steps of ``vit_imagenet._block_backward`` in fp32.  ``G``: this block's fp32 gradient
    buffers by name under ``blocks.{i}.`` (missing = not wanted), ADDED into."""
    dev = dy.device
    M, D = dy.shape
    BT, r, H4 = B * T, w.r, 4 * D
    tw1, _, tw2, _ = w.ad["T_Adapter"]
    sw1, _, sw2, _ = w.ad["S_Adapter"]

    def d_fc2(g, h, name, fac):       # an adapter output scaled per frame by `fac` (folded into h by the forward)
        if G.get(name + ".D_fc2.weight") is not None:
            ops.wgrad_f32(g, h, G[name + ".D_fc2.weight"])
        if G.get(name + ".D_fc2.bias") is not None:
            _colsum(g, G[name + ".D_fc2.bias"], fac, N)

    def ln_gb(dxl, xin, mean, rstd, name):
        if G.get(name + ".weight") is not None or G.get(name + ".bias") is not None:
            ops.layernorm_gb_bwd(dxl, xin, mean, rstd, M, D, G.get(name + ".weight"), G.get(name + ".bias"))

    # ---- joint adaptation
    hcat, dms2 = c["hcat"], c["dms2"]
    _wgrad(dy, hcat[:, :H4], G, "mlp.fc2.weight", "mlp.fc2.bias")
    d_fc2(dy, hcat[:, H4:], "MLP_Adapter", dms2)
    dcat = _e((M, H4 + r), dev)
    ops.gemm_f32(dy, w.t("Wcat2"), ops.EPI_DACT, dcat, aux=c["hcat_pre"], act=ops.ACT_GELU, n_split=H4, act2=ops.ACT_GELU,
                 af=dms2, ntok=N)
    _wgrad(dcat[:, :H4], c["xn"], G, "mlp.fc1.weight", "mlp.fc1.bias")
    _wgrad(dcat[:, H4:], c["xn"], G, "MLP_Adapter.D_fc1.weight", "MLP_Adapter.D_fc1.bias")
    dxn = _e((M, D), dev)
    ops.gemm_f32(dcat, w.t("Wcat1"), ops.EPI_BF16, dxn)
    del dcat
    dx2 = _e((M, D), dev)
    ops.layernorm_bwd(dxn, c["x2"], w.g2, c["mean2"], c["rstd2"], M, D, lddy=D, ldx=D, lddx=D, dres=dy, dx=dx2)
    ln_gb(dxn, c["x2"], c["mean2"], c["rstd2"], "norm2")
    del dxn
    # ---- spatial adaptation: x2 = x1 + sa + (s_h W2^T + b2),  s_h = GELU(sa W1^T + b1),  sa = ao proj^T + proj.bias
    _wgrad(dx2, c["s_h"], G, "S_Adapter.D_fc2.weight", "S_Adapter.D_fc2.bias")
    dsh_pre = _e((M, r), dev)
    ops.gemm_f32(dx2, sw2.t().contiguous(), ops.EPI_DACT, dsh_pre, aux=c["s_pre"], act=ops.ACT_GELU)
    _wgrad(dsh_pre, c["sa"], G, "S_Adapter.D_fc1.weight", "S_Adapter.D_fc1.bias")
    dsa = _e((M, D), dev)
    ops.gemm_f32(dsh_pre, sw1.t().contiguous(), ops.EPI_F32, dsa, resid=dx2)      # + the skip connection's share
    _wgrad(dsa, c["ao"], G, "attn.proj.weight", "attn.proj.bias")
    dao = _e((M, D), dev)
    ops.gemm_f32(dsa, w.t("Wo"), ops.EPI_BF16, dao)
    del dsa
    dqkv = _e((M, 3 * D), dev)
    ops.attn_bwd_f32(c["qkv_s"], dao, dqkv, BT, N, H)
    del dao
    _wgrad(dqkv, c["xl2"], G, "attn.qkv.weight", "attn.qkv.bias")
    dxl2 = _e((M, D), dev)
    ops.gemm_f32(dqkv, w.t("Wqkv"), ops.EPI_BF16, dxl2)
    dx1 = _e((M, D), dev)
    ops.layernorm_bwd(dxl2, c["x1"], w.g1, c["mean1b"], c["rstd1b"], M, D, lddy=D, ldx=D, lddx=D, dres=dx2, dx=dx1)
    ln_gb(dxl2, c["x1"], c["mean1b"], c["rstd1b"], "norm1")
    del dxl2, dx2
    # ---- temporal adaptation: x1 = x + t_hs W2^T + dp1[f] b2,  t_hs = dp1[f] GELU(ta W1^T + b1)
    dp1 = c["dp1"]
    d_fc2(dx1, c["t_hs"], "T_Adapter", dp1)
    dth_pre = _e((M, r), dev)
    ops.gemm_f32(dx1, tw2.t().contiguous(), ops.EPI_DACT, dth_pre, aux=c["t_pre"], act=ops.ACT_GELU, af=dp1, ntok=N)
    _wgrad(dth_pre, c["ta"], G, "T_Adapter.D_fc1.weight", "T_Adapter.D_fc1.bias")
    dta = _e((M, D), dev)
    ops.gemm_f32(dth_pre, tw1.t().contiguous(), ops.EPI_BF16, dta)
    del dth_pre
    _wgrad(dta, c["ot"], G, "attn.proj.weight", "attn.proj.bias")
    dot = _e((M, D), dev)
    ops.gemm_f32(dta, w.t("Wo"), ops.EPI_BF16, dot)
    del dta
    dqkv.zero_()
    ops.tattn_bwd_f32(c["qkv_t"], dot, dqkv, B, T, N, H)
    del dot
    tin = c["tin"]
    _wgrad(dqkv, tin if tin is not None else c["xl"], G, "attn.qkv.weight", "attn.qkv.bias")
    dqin = _e((M, D), dev)
    ops.gemm_f32(dqkv, w.t("Wqkv"), ops.EPI_BF16, dqin)
    del dqkv
    if tin is not None:      # qin = xl + D_fc2(GELU(D_fc1(xl)))
        iw1, _, iw2, _ = w.ad["T_Adapter_in"]
        _wgrad(dqin, c["tin_h"], G, "T_Adapter_in.D_fc2.weight", "T_Adapter_in.D_fc2.bias")
        dpre = _e((M, r), dev)
        ops.gemm_f32(dqin, iw2.t().contiguous(), ops.EPI_DACT, dpre, aux=c["tin_pre"], act=ops.ACT_GELU)
        _wgrad(dpre, c["xl"], G, "T_Adapter_in.D_fc1.weight", "T_Adapter_in.D_fc1.bias")
        dxl = _e((M, D), dev)
        ops.gemm_f32(dpre, iw1.t().contiguous(), ops.EPI_F32, dxl, resid=dqin)   # + the skip connection's share
        del dpre, dqin
    else:
        dxl = dqin
    dx = _e((M, D), dev)
    ops.layernorm_bwd(dxl, c["x"], w.g1, c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dx1, dx=dx)
    ln_gb(dxl, c["x"], c["mean1"], c["rstd1"], "norm1")
    return dx


def forward_f32(model, imgs, P, save: bool):
    """imgs [B, 3, T, H, W] -> [B, D, T] f32 (vit_imagenet.py:238-266); ``P`` = parameters by name."""
    B, C, T, Hh, Ww = imgs.shape
    D, p, H, L = model.embed_dim, model.patch_size, model.num_heads, model.depth
    G = Hh // p
    N = G * G + 1
    BT, M = B * T, B * T * N
    dev = imgs.device
    K = 3 * p * p
    if imgs.dtype != F32:
        imgs = imgs.float().contiguous()
    A = _e((BT * G * G, K), dev)
    ops.patchify_f32(imgs, A, B, T, Hh, Ww, p, K)
    tok = _e((BT * G * G, D), dev)
    cb = P.get("patch_embed.proj.bias")
    ops.gemm_f32(A, _f(P["patch_embed.proj.weight"]).reshape(D, K), ops.EPI_BF16, tok, bias=None if cb is None else _f(cb))
    del A
    x = _e((M, D), dev)
    ops.embed_nopre_fwd(tok, _f(P["cls_token"]).view(D), _f(P["pos_embed"]).view(N, D), _f(P["temporal_embedding"]).view(T, D), x,
                        B, T, N, D)
    del tok
    masks = model._drop_masks(BT, model.training, dev)
    ctxs, blocks = [], []
    for i, blk in enumerate(model.blocks):
        w = _Block32(blk)
        x, c = block_forward_f32(x, w, B, T, N, H, masks[i, 0], masks[i, 1], save)
        ctxs.append(c)
        blocks.append(w if save else None)
    gw = _f(P["ln_post.weight"])
    y = _e((BT, D), dev)
    meanp, rstdp = _e((BT,), dev), _e((BT,), dev)
    ops.layernorm_fwd(x, gw, _f(P["ln_post.bias"]), BT, D, N * D, y_f32=y, mean=meanp, rstd=rstdp, eps=model.eps)
    y = y.reshape(B, T, D).permute(0, 2, 1)
    saved = dict(ctxs=ctxs, blocks=blocks, xL=x, gw=gw, meanp=meanp, rstdp=rstdp, imgs=imgs,
                 dims=(B, T, N, H, D, L, G)) if save else None
    return y, saved


class _ViTImageNetFn32(torch.autograd.Function):
    """imgs -> [B, D, T] in fp32 with the hand-written fp32 backward.  Differentiable inputs: every parameter, in
    ``named_parameters()`` order; a parameter that does not require grad gets None and no launch."""

    @staticmethod
    def forward(ctx, model, imgs, *params):
        names = model._param_names()
        ctx.need = [bool(ctx.needs_input_grad[2 + k]) for k in range(len(params))]
        y, saved = forward_f32(model, imgs, dict(zip(names, params)), save=True)
        ctx.model, ctx.saved, ctx.params = model, saved, params
        return y

    @staticmethod
    def backward(ctx, dout):
        model, s, params, need = ctx.model, ctx.saved, ctx.params, ctx.need
        B, T, N, H, D, L, G = s["dims"]
        BT, M = B * T, B * T * N
        dev = dout.device
        names = model._param_names()
        grads = [torch.zeros(p_.shape, dtype=F32, device=dev) if nd else None for p_, nd in zip(params, need)]
        GR = dict(zip(names, grads))
        dy = dout.permute(0, 2, 1).reshape(BT, D).contiguous().float()
        dx = torch.zeros((M, D), dtype=F32, device=dev)
        ops.layernorm_bwd(dy, s["xL"], s["gw"], s["meanp"], s["rstdp"], BT, D, lddy=D, ldx=N * D, lddx=N * D, dx=dx)
        if GR["ln_post.weight"] is not None or GR["ln_post.bias"] is not None:
            ops.layernorm_gb_bwd(dy, s["xL"], s["meanp"], s["rstdp"], BT, D, GR["ln_post.weight"], GR["ln_post.bias"], ldx=N * D)
        for i in reversed(range(L)):
            pre = f"blocks.{i}."
            gi = {n[len(pre):]: t for n, t in GR.items() if n.startswith(pre) and t is not None}
            dx = block_backward_f32(dx, s["ctxs"][i], s["blocks"][i], gi, B, T, N, H)
            s["ctxs"][i] = s["blocks"][i] = None
        gconv = GR["patch_embed.proj.weight"]
        dtok = _e((BT * (N - 1), D), dev) if gconv is not None else None
        gtmp, gcls, gpos = GR["temporal_embedding"], GR["cls_token"], GR["pos_embed"]
        ops.embed_nopre_bwd(dx, B, T, N, D, dtok=dtok, dcls=None if gcls is None else gcls.view(D),
                            dpos=None if gpos is None else gpos.view(N, D), dtemporal=None if gtmp is None else gtmp.view(T, D),
                            dbias=GR.get("patch_embed.proj.bias"))
        del dx
        if gconv is not None:
            p, imgs = model.patch_size, s["imgs"]
            K = 3 * p * p
            A = _e((BT * (N - 1), K), dev)
            ops.patchify_f32(imgs, A, B, T, imgs.shape[3], imgs.shape[4], p, K)
            ops.wgrad_f32(dtok, A, gconv.view(D, K))
        ctx.saved = None
        out = [None if g_ is None else (g_ if g_.dtype == p_.dtype else g_.to(p_.dtype)) for g_, p_ in zip(grads, params)]
        return (None, None) + tuple(out)
