"""Per-launch times of the wave-per-row LayerNorm family at the workload's shapes: 512 frames x 197 tokens x 768 (B = 64, T = 8).

usage: tools/bench_ln.py [NAME ...]      (no name: every figure; a name: that figure alone, for a process per figure)

Each figure is the median of 20 timed launches (HIP events around each launch) after 5 warm-ups, in microseconds.
AIM_HIP_LIB selects another build of the library.  A figure times the call of the Python wrapper as the model makes it:
embed_bwd and embed_ln_bwd include the wrapper's torch.empty of the workspace and their finish launches, the fsum figures
the assignment of ops.LN_FSUM_GROUPS; the same for every build, so two builds compare like for like.  Every tensor is built
(and embed_ln run once for the stem's x, mean and rstd) whichever figure is asked for.
"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aim_amd import ops
B, T, ntok, D = 64, 8, 197, 768
frames = B * T
M = frames * ntok
dev = "cuda"
x = torch.randn((M, D), device=dev); g = torch.ones(D, device=dev); beta = torch.zeros(D, device=dev)
dy = torch.randn((M, D), device=dev).to(torch.bfloat16); dres = torch.randn((M, D), device=dev).to(torch.bfloat16)
mean = x.mean(1).contiguous(); rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
out = torch.empty((M, D), dtype=torch.bfloat16, device=dev); w = torch.rand(ntok, device=dev)
# the stem: bf16 patch tokens, class / positional / temporal embeddings; embed_ln writes the x, mean and rstd its backwards read
tok = torch.randn((frames * (ntok - 1), D), device=dev).to(torch.bfloat16)
cls, pos, tmp = torch.randn(D, device=dev), torch.randn((ntok, D), device=dev), torch.randn((T, D), device=dev)
xe, me, re = torch.empty((M, D), device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev)
ops.embed_ln(tok, cls, pos, tmp, g, beta, xe, me, re, B, T, ntok, D)
dtok = torch.empty_like(tok)
dcls, dpos, dtmp, dg, db = (torch.zeros(s, device=dev) for s in ((D,), (ntok, D), (T, D), (D,), (D,)))

def t(fn, n=20, warm=5):
    for _ in range(warm): fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[n // 2]

def fsum(G):
    part = torch.empty((frames, G, D), device=dev)
    def fn():
        ops.LN_FSUM_GROUPS = G
        ops.layernorm_bwd_fsum(dy, x, g, mean, rstd, dres, out, w, part, frames, ntok, D)
    return fn

FIGURES = {
    "ln_fwd": lambda: ops.layernorm_fwd(x, g, beta, M, D, D, y_bf16=out, mean=me, rstd=re),
    "ln_bwd": lambda: ops.layernorm_bwd(dy, x, g, mean, rstd, M, D, lddy=D, ldx=D, lddx=D, dres=dres, dx_bf16=out),
    **{"ln_bwd_fsum_G%d" % G: fsum(G) for G in sorted({13, 25, 33, 50, ops.LN_FSUM_GROUPS})},
    "embed_ln": lambda: ops.embed_ln(tok, cls, pos, tmp, g, beta, xe, me, re, B, T, ntok, D),
    "embed_bwd": lambda: ops.embed_bwd(dy, tok, cls, pos, tmp, g, me, re, dtmp, B, T, ntok, D),
    "embed_ln_bwd": lambda: ops.embed_ln_bwd(dy, tok, cls, pos, tmp, g, me, re, B, T, ntok, D, dtok=dtok, dcls=dcls, dpos=dpos,
                                            dtemporal=dtmp, dgamma=dg, dbeta=db),
}
for name in sys.argv[1:] or FIGURES:
    print("%-16s %.1f us" % (name, t(FIGURES[name])), flush=True)
