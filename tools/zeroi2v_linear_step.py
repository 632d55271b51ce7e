"""ViT_CLIP_ZEROI2V with linear adapters: whole training steps and inference, fused low-rank kernels beside a composition of
existing calls, for DESIGN.md sections 2d / 4 and profiles/zeroi2v_linear.json.

    python tools/zeroi2v_linear_step.py [--clips B] [--layers 12] [--rounds 7] [--warmup 2] [--only fused] [--json OUT]

The model is the sthv2 recipe's: ViT-B/16, 8 frames, 224 x 224, temporal class token, bottleneck 192, pretrained=None with
non-zero D_fc2.  ``--clips 0`` (default) takes the largest batch of (64, 48, 32, 24, 16, 8) whose linear-mode training step fits.
A round runs, interleaved in one process and each between two hipEvents,
  train    one forward + backward of the backbone (a random output gradient; no head, no optimizer) for
           ``base``      linear_adapter=False, for scale
           ``fused``     linear mode on aim_lowrank_fwd / aim_lowrank_bwd
           ``composed``  linear mode with ``ops.lowrank_fwd / _bwd`` replaced, inside this script only, by chains of
                         ``ops.gemm`` / ``ops.add_bf16`` / ``ops.acc_bf16`` calls that compute the same sums
  infer    one no-grad forward for ``unmerged``, ``merged`` (merge_adapters()) and ``base``.
The figure is the median over the rounds behind the warm-up, with min and max.  ``--only NAME`` runs one training variant alone
(for a kernel table under ``rocprofv3 --kernel-trace --stats``)."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def _stats(ms):
    s = sorted(ms)
    return dict(median_ms=round(s[len(s) // 2], 3), min_ms=round(s[0], 3), max_ms=round(s[-1], 3))


def composed(ops):
    """(lowrank_fwd, lowrank_bwd) with the wrappers' signatures, from existing calls: two GEMMs per adapter and bf16 adds"""
    BF16 = torch.bfloat16

    def fwd(x, w1, b1, w2, b2, *, h=None, y=None, alpha=1.0, y32=None, resid=None):
        M, D = x.shape
        for g in range(len(w1)):
            hg = h[g] if h is not None and h[g] is not None else torch.empty((M, w1[g].shape[0]), dtype=BF16, device=x.device)
            ops.gemm(x, w1[g], ops.EPI_BF16, hg, bias=b1[g])
            if y32 is not None:                         # resid + H W2^T + b2 in fp32, then alpha times x
                ops.gemm(hg, w2[g], ops.EPI_F32, y32, bias=b2[g], resid=resid)
                for _ in range(int(alpha)):
                    ops.acc_bf16(y32, x)
            else:
                ops.gemm(hg, w2[g], ops.EPI_BF16, y[g], bias=b2[g])
                for _ in range(int(alpha)):
                    ops.add_bf16(y[g], x, y[g])

    def bwd(dy, w2t, w1t, dh, dx, *, alpha=1.0):
        M, D = dy[0].shape
        t = torch.empty((M, D), dtype=BF16, device=dx.device)
        for g in range(len(w2t)):
            ops.gemm(dy[g], w2t[g], ops.EPI_BF16, dh[g])
            ops.gemm(dh[g], w1t[g], ops.EPI_BF16, dx if g == 0 else t)
            if g:
                ops.add_bf16(dx, t, dx)
            for _ in range(int(alpha)):
                ops.add_bf16(dx, dy[g], dx)

    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=0)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, choices=("base", "fused", "composed"))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import aim_amd
    from aim_amd import ops
    dev = torch.device("cuda")
    T, D, H = 8, 768, 12

    def model(linear):
        torch.manual_seed(0)
        m = aim_amd.ViT_CLIP_ZEROI2V(224, T, 16, D, a.layers, H, 0.2, adapter_scale=0.5, with_t_cls_token=True, bottleneck=192,
                                     linear_adapter=linear, pretrained=None)
        m.init_weights()
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "D_fc2" in n:
                    p.normal_(0, 0.02)
        return m.to(dev)

    base, lin = model(False), model(True)
    real = (ops.lowrank_fwd, ops.lowrank_bwd)
    comp = composed(ops)

    def use(pair):
        ops.lowrank_fwd, ops.lowrank_bwd = pair

    def train_step(m, imgs, g):
        m.train()
        m.zero_grad(set_to_none=True)
        m(imgs).backward(g)

    def infer(m, imgs):
        m.eval()
        with torch.no_grad():
            return m(imgs)

    gen = torch.Generator().manual_seed(1234)
    B = a.clips
    for cand in ([B] if B else [64, 48, 32, 24, 16, 8]):
        try:
            imgs = torch.randn((cand, 3, T, 224, 224), generator=gen).to(dev)
            g = torch.randn((cand, D, T, 1, 1), generator=gen).to(dev)
            use(comp)                                    # (the composition keeps a few more temporaries alive)
            train_step(lin, imgs, g)
            torch.cuda.synchronize()
            B = cand
            break
        except torch.cuda.OutOfMemoryError:
            lin.zero_grad(set_to_none=True)
            imgs = g = None
            torch.cuda.empty_cache()
    use(real)
    assert B, "no batch size fits"
    # the composition computes the same sums (other rounding points): its features stay within bf16 noise of the fused ones
    yf = infer(lin, imgs)
    use(comp)
    yc = infer(lin, imgs)
    use(real)
    check = float((yc.double() - yf.double()).norm() / yf.double().norm())

    # name -> (what is set up outside the timed span, the timed call); the fold of merge_adapters() is not part of a forward
    train = {"base": (lambda: None, lambda: train_step(base, imgs, g)),
             "fused": (lambda: use(real), lambda: train_step(lin, imgs, g)),
             "composed": (lambda: use(comp), lambda: train_step(lin, imgs, g))}
    if a.only:
        train = {a.only: train[a.only]}
    inf = {} if a.only else {"unmerged": (lambda: lin.unmerge_adapters(), lambda: infer(lin, imgs)),
                             "merged": (lambda: lin.merge_adapters(), lambda: infer(lin, imgs)),
                             "base": (lambda: None, lambda: infer(base, imgs))}
    times = {("train", k): [] for k in train}
    times.update({("infer", k): [] for k in inf})
    for r in range(a.warmup + a.rounds):
        for kind, table in (("train", train), ("infer", inf)):
            for k, (prep, fn) in table.items():
                prep()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[(kind, k)].append(e0.elapsed_time(e1))
                use(real)
        lin.unmerge_adapters()
    res = dict(model="ViT_CLIP_ZEROI2V ViT-B/16 (sthv2 recipe shape)", layers=a.layers, frames=T, clips=B, bottleneck=192,
               rows=B * T * 198, rounds=a.rounds, warmup=a.warmup, composed_vs_fused_rel=check, train={}, infer={})
    for (kind, k), ms in times.items():
        st = _stats(ms)
        st["clips_per_s" if kind == "train" else "views_per_s"] = round(B * 1e3 / st["median_ms"], 1)
        res[kind][k] = st
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
