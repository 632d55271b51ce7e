"""Reference-precision mode of ``TimeSformer`` (``set_precision('fp32')``): the model on fp32 operands and the fp32 kernels
(csrc/fp32.hip: f32 MFMA GEMMs, exact exp; ``aim_tattn_*_f32``, ``aim_attn_*_f32``, ``aim_wgrad_f32``, ``aim_embed_ln_bwd`` with
f32 ``dx`` / ``dtok``), forward and the same hand-written backward, every parameter's gradient included.  It is held to the
reference's own fp32 outputs and autograd gradients at 1e-5 (tests/test_timesformer_gpu.py), which is what pins the block's
algebra (which LayerNorm feeds which attention, the DropPath factor between ``t_attn.out_proj`` and ``T_Adapter``) below bf16
noise.

The block is this file's own (``block_forward_f32`` / ``block_backward_f32``): it has two attentions with weights of their
own, a plain-Linear ``T_Adapter`` and no bottleneck adapters, so it shares no stretch with ``fp32_path.aim_block_forward_f32``.
It reads a block through ``timesformer._block_view``, as the bf16 path does.  A DropPath factor multiplies the gradient rows
with ``aim_scale_rows`` here (the bf16 path lets it ride GEMM epilogues).

One stream, operands built from the current parameters on every call (nothing cached), plain autograd outputs: a verification
mode, not a fast path (the f32 MFMA runs at 1/16 of the bf16 rate).
"""
import torch

from . import ops
from .backbone import _ln_post_forward
from .fp32_path import _e, _f
from .full_param import GradBufs, conv_wgrad_f32, ln_post_backward, node_forward_f32
from .timesformer import _NAMES, _STEM, _block_view

F32 = torch.float32


class _BlockW32:
    """fp32 operands of one block, read through ``_block_view``; the dgrad operands (the transposes) are made on first use"""

    def __init__(self, view):
        self.eps = view["eps"]
        self.W = {n: _f(w) for n, (w, _) in view["linear"].items()}
        self.b = {n: _f(b) for n, (_, b) in view["linear"].items()}
        self.g = {n: _f(w) for n, (w, _) in view["norm"].items()}
        self.beta = {n: _f(b) for n, (_, b) in view["norm"].items()}
        self._t = {}

    def WT(self, name):
        if name not in self._t:
            self._t[name] = self.W[name].t().contiguous()
        return self._t[name]


def _rows(f, BT):
    """a per-token factor f [N] as one entry per row m = (b*T + t)*N + n"""
    return None if f is None else f.repeat(BT).contiguous()


def _scaled(g, rows):
    """rows[m] * g[m] (``aim_scale_rows``); g itself where the factor is 1"""
    if rows is None:
        return g
    out = _e(g.shape, g.device)
    ops.scale_rows(g, rows, y_f32=out)
    return out


def block_forward_f32(x, w: _BlockW32, B, T, N, H, f1, f2, f3, save: bool):
    """The steps of ``timesformer._block_forward`` in fp32 (timesformer.py:57-71).  ``f1`` [B*T] per frame, ``f2`` / ``f3`` [N]
    per token index, None = 1."""
    dev = x.device
    M, D = x.shape
    BT, eps = B * T, w.eps
    stat = lambda: (_e((M,), dev), _e((M,), dev)) if save else (None, None)
    xt = _e((M, D), dev)
    mean_t, rstd_t = stat()
    ops.layernorm_fwd(x, w.g["t_norm"], w.beta["t_norm"], M, D, D, y_f32=xt, mean=mean_t, rstd=rstd_t, eps=eps)
    qkv_t = _e((M, 3 * D), dev)
    ops.gemm_f32(xt, w.W["t_qkv"], ops.EPI_BF16, qkv_t, bias=w.b["t_qkv"])
    ot = _e((M, D), dev)
    ops.tattn_fwd_f32(qkv_t, ot, B, T, N, H)
    ta = _e((M, D), dev)
    ops.gemm_f32(ot, w.W["t_out"], ops.EPI_BF16, ta, bias=w.b["t_out"], af=f1, ntok=N)
    x1 = _e((M, D), dev)
    ops.gemm_f32(ta, w.W["t_ad"], ops.EPI_F32, x1, bias=w.b["t_ad"], resid=x)
    xl = _e((M, D), dev)
    mean1, rstd1 = stat()
    ops.layernorm_fwd(x1, w.g["ln_1"], w.beta["ln_1"], M, D, D, y_f32=xl, mean=mean1, rstd=rstd1, eps=eps)
    qkv_s = _e((M, 3 * D), dev)
    ops.gemm_f32(xl, w.W["qkv"], ops.EPI_BF16, qkv_s, bias=w.b["qkv"])
    ao = _e((M, D), dev)
    ops.attn_fwd_f32(qkv_s, ao, BT, N, H)
    x2 = _e((M, D), dev)
    ops.gemm_f32(ao, w.W["out"], ops.EPI_F32, x2, bias=w.b["out"], resid=x1, at=f2, ntok=N)
    xn = _e((M, D), dev)
    mean2, rstd2 = stat()
    ops.layernorm_fwd(x2, w.g["ln_2"], w.beta["ln_2"], M, D, D, y_f32=xn, mean=mean2, rstd=rstd2, eps=eps)
    h = _e((M, 4 * D), dev)
    h_pre = _e((M, 4 * D), dev) if save else None
    ops.gemm_f32(xn, w.W["fc"], ops.EPI_ACT, h, bias=w.b["fc"], act=ops.ACT_QGELU, out2=h_pre)
    x3 = _e((M, D), dev)
    ops.gemm_f32(h, w.W["pr"], ops.EPI_F32, x3, bias=w.b["pr"], resid=x2, at=f3, ntok=N)
    if not save:
        return x3, None
    return x3, dict(x=x, mean_t=mean_t, rstd_t=rstd_t, xt=xt, qkv_t=qkv_t, ot=ot, ta=ta, x1=x1, mean1=mean1, rstd1=rstd1, xl=xl,
                    qkv_s=qkv_s, ao=ao, x2=x2, mean2=mean2, rstd2=rstd2, xn=xn, h=h, h_pre=h_pre, f1=f1, f2=f2, f3=f3)


def block_backward_f32(dy, c, w: _BlockW32, gr, B, T, N, H):
    """d(loss)/d(x3) [M, D] -> d(loss)/d(x); the steps of ``timesformer._block_backward`` in fp32.  ``gr``: fp32 gradient buffers
    by parameter name under ``transformer.resblocks.{i}.`` (missing = not wanted, no launch), ADDED into."""
    dev = dy.device
    M, D = dy.shape
    BT = B * T

    def wgrad(gm, a, lin):
        dw, db = gr.get(_NAMES[lin][0]), gr.get(_NAMES[lin][1])
        if dw is None and db is not None:                   # (as the bf16 path: the bias keeps the fused launch's bits)
            dw = torch.zeros((gm.shape[1], a.shape[1]), dtype=F32, device=dev)
        if dw is not None:
            ops.wgrad_f32(gm, a, dw, db)

    def ln_gb(dxl, xin, mean, rstd, norm):
        dg, db = gr.get(_NAMES[norm][0]), gr.get(_NAMES[norm][1])
        if dg is not None or db is not None:
            ops.layernorm_gb_bwd(dxl, xin, mean, rstd, M, D, dg, db)

    # ---- x3 = x2 + f3 (h W_pr^T + b_pr),  h = QuickGELU(xn W_fc^T + b_fc)
    g3 = _scaled(dy, _rows(c["f3"], BT))
    wgrad(g3, c["h"], "pr")
    dpre = _e((M, 4 * D), dev)
    ops.gemm_f32(g3, w.WT("pr"), ops.EPI_DACT, dpre, aux=c["h_pre"], act=ops.ACT_QGELU)
    wgrad(dpre, c["xn"], "fc")
    dxn = _e((M, D), dev)
    ops.gemm_f32(dpre, w.WT("fc"), ops.EPI_BF16, dxn)
    del dpre, g3
    dx2 = _e((M, D), dev)
    ops.layernorm_bwd(dxn, c["x2"], w.g["ln_2"], c["mean2"], c["rstd2"], M, D, lddy=D, ldx=D, lddx=D, dres=dy, dx=dx2)
    ln_gb(dxn, c["x2"], c["mean2"], c["rstd2"], "ln_2")
    del dxn
    # ---- x2 = x1 + f2 (ao W_o^T + b_o)
    g2 = _scaled(dx2, _rows(c["f2"], BT))
    wgrad(g2, c["ao"], "out")
    dao = _e((M, D), dev)
    ops.gemm_f32(g2, w.WT("out"), ops.EPI_BF16, dao)
    del g2
    dqkv = _e((M, 3 * D), dev)
    ops.attn_bwd_f32(c["qkv_s"], dao, dqkv, BT, N, H)
    del dao
    wgrad(dqkv, c["xl"], "qkv")
    dxl = _e((M, D), dev)
    ops.gemm_f32(dqkv, w.WT("qkv"), ops.EPI_BF16, dxl)
    dx1 = _e((M, D), dev)
    ops.layernorm_bwd(dxl, c["x1"], w.g["ln_1"], c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dx2, dx=dx1)
    ln_gb(dxl, c["x1"], c["mean1"], c["rstd1"], "ln_1")
    del dxl, dx2
    # ---- x1 = x + ta W_ad^T + b_ad,  ta = f1 (ot W_to^T + b_to)
    wgrad(dx1, c["ta"], "t_ad")
    gt = _e((M, D), dev)
    ops.gemm_f32(dx1, w.WT("t_ad"), ops.EPI_BF16, gt, af=c["f1"], ntok=N)
    wgrad(gt, c["ot"], "t_out")
    dot = _e((M, D), dev)
    ops.gemm_f32(gt, w.WT("t_out"), ops.EPI_BF16, dot)
    del gt
    dqkv.zero_()                                            # (aim_tattn_bwd_f32 ADDS)
    ops.tattn_bwd_f32(c["qkv_t"], dot, dqkv, B, T, N, H)
    del dot
    wgrad(dqkv, c["xt"], "t_qkv")
    dxt = _e((M, D), dev)
    ops.gemm_f32(dqkv, w.WT("t_qkv"), ops.EPI_BF16, dxt)
    del dqkv
    dx = _e((M, D), dev)
    ops.layernorm_bwd(dxt, c["x"], w.g["t_norm"], c["mean_t"], c["rstd_t"], M, D, lddy=D, ldx=D, lddx=D, dres=dx1, dx=dx)
    ln_gb(dxt, c["x"], c["mean_t"], c["rstd_t"], "t_norm")
    return dx


def forward_f32(model, imgs, P, wants):
    """imgs [B, 3, T, H, W] -> [B, D, T] f32 (timesformer.py:192-225); ``P`` = parameters by name.  ``wants``: the names of the
    parameters whose gradient the backward will be asked for; empty = forward only, nothing is saved."""
    save = bool(wants)
    B, C, T, Hh, Ww = imgs.shape
    D, p, H, L = model.width, model.patch_size, model.heads, model.layers
    G = Hh // p
    N = G * G + 1
    BT, M = B * T, B * T * N
    dev = imgs.device
    K = 3 * p * p
    if imgs.dtype != F32:
        imgs = imgs.float().contiguous()
    A = _e((BT * G * G, K), dev)
    ops.patchify(imgs, A, B, T, Hh, Ww, p, K)
    tok = _e((BT * G * G, D), dev)
    ops.gemm_f32(A, _f(P["conv1.weight"]).reshape(D, K), ops.EPI_BF16, tok)
    del A
    x = _e((M, D), dev)
    mean0, rstd0 = _e((M,), dev), _e((M,), dev)
    cls, pos, tmp, gpre = _f(P["class_embedding"]), _f(P["positional_embedding"]), model._temporal_rows(P, T, D, dev), _f(P["ln_pre.weight"])
    pre = _e((M, D), dev)           # (aim_embed_ln_f32 writes ln_pre's input rows beside the statistics; the backward rebuilds them)
    ops.embed_ln_f32(tok, cls, pos, tmp, gpre, _f(P["ln_pre.bias"]), x, B, T, N, D, pre=pre, mean=mean0, rstd=rstd0)
    del pre
    factors = model._expand_factors(model._drop_factors(T, N, model.training, dev), B)
    ctxs, blocks = [], []
    for i, blk in enumerate(model.transformer.resblocks):
        w = _BlockW32(_block_view(blk))
        x, c = block_forward_f32(x, w, B, T, N, H, *factors[i], save)
        ctxs.append(c)
        blocks.append(w if save else None)
    y, gw, meanp, rstdp = _ln_post_forward(x, P["ln_post.weight"], P["ln_post.bias"], BT, N)
    y = y.reshape(B, T, D).permute(0, 2, 1)
    saved = dict(ctxs=ctxs, blocks=blocks, xL=x, gw=gw, meanp=meanp, rstdp=rstdp, imgs=imgs, tok=tok, cls=cls, pos=pos, tmp=tmp,
                 gpre=gpre, mean0=mean0, rstd0=rstd0, dims=(B, T, N, H, D, L, G)) if save else None
    return y, saved


class _TimeSformerFn32(torch.autograd.Function):
    """imgs -> [B, D, T] in fp32 with the hand-written fp32 backward.  Differentiable inputs: every parameter, in
    ``named_parameters()`` order; a parameter that does not require grad gets None and no launch."""

    @staticmethod
    def forward(ctx, model, imgs, *params):
        return node_forward_f32(ctx, forward_f32, model, imgs, params)

    @staticmethod
    def backward(ctx, dout):
        model, s = ctx.model, ctx.saved
        B, T, N, H, D, L, G = s["dims"]
        BT = B * T
        dev = dout.device
        GR = GradBufs(model._param_names(), ctx.params, ctx.need, dev, False)      # (this mode never accumulates in place)
        dx = ln_post_backward(dout, s, GR["ln_post.weight"], GR["ln_post.bias"], BT, N, F32)
        for i in reversed(range(L)):
            dx = block_backward_f32(dx, s["ctxs"][i], s["blocks"][i], GR.block(f"transformer.resblocks.{i}."), B, T, N, H)
            s["ctxs"][i] = s["blocks"][i] = None
        gconv = GR["conv1.weight"]
        dtok = _e((BT * (N - 1), D), dev) if gconv is not None else None
        stem = [GR.get(n) for n in _STEM]
        if dtok is not None or any(t is not None for t in stem):
            gcls, gpos, gtmp, ggam, gbet = stem
            ops.embed_ln_bwd(dx, s["tok"], s["cls"], s["pos"], s["tmp"], s["gpre"], s["mean0"], s["rstd0"], B, T, N, D, dtok=dtok,
                             dcls=gcls, dpos=gpos, dtemporal=None if gtmp is None else gtmp.view(T, D), dgamma=ggam, dbeta=gbet)
        del dx
        if gconv is not None:
            conv_wgrad_f32(s["imgs"], dtok, gconv, model.patch_size)
        ctx.saved = None
        return GR.result(2)
