"""The last block on the class rows only (backbone.py: AIM_TOP_CLS_ONLY).

The head reads the class row of every frame and nothing else, so the last block runs its spatial attention for the class
query alone (aim_attn_fwd_cls), out_proj / ln_2 / MLP + MLP_Adapter on B*T rows, and its backward starts from a compact
gradient (aim_attn_bwd_cls writes all of d(qkv) from one dO row per (frame, head)).

Kernel level: both kernels against the float64 references and the derived bounds of attn_cases.py, restricted to what
they compute: query row 0 of `out` and `lse`, and -- with dO zero outside the class rows, which is the situation they are
built for -- dK, dV of every key and dQ[0]; every other dQ row must be exactly zero.  The forward reuses the full kernel's
first query tile, so its results are also held to row 0 of aim_attn_fwd bit for bit.  A second run with NaN in the q part of
every non-class row of qkv must give the same bits: those values are never part of the class query's result (this pins
"no 0 x garbage product").

Model level: the same seed and clips with AIM_TOP_CLS_ONLY=0 and =1 in child processes (the switch is read at import).  The two
forms differ by GEMM route (the B*T-row launches run on the 64 x 64 kernel, the full ones on the 256 x 256 kernel) and by the fp32
summation order of the MLP_Adapter weight gradients: rounding noise.  Tiny config and ViT-B/16 at 2 clips x 4 frames with and
without checkpoint=True, and ViT-B/16 at the benchmark's 64 clips x 8 frames (B*T = 512).
Per tensor the relative L2 distance between the two forms must stay within ONE TENTH of the bound test_backbone_gpu.py asserts for that tensor against the reference: 2.5e-3 for every trainable gradient (a tenth
of 2.5e-2), 1.5e-3 for the returned features (a tenth of 1.5e-2).  The loss is a smooth function of the features alone
(mean over frames, a fixed linear head, cross-entropy), so it is held to the features' figure, relative.
Measured: loss and features bit-identical, gradients at most 4.0e-9 (tiny) and 5.7e-8 (ViT-B/16, the top
block's MLP_Adapter sums over B*T rows instead of all rows) with every gradient below the top block bit-identical; at
64 clips x 8 frames loss and features bit-identical, worst gradient tensor 6.7e-4.
"""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as AC  # noqa: E402
from gemm_cases import _pad_intact, _padded, ratio  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32

SHAPES = ((16, 197, 12), (8, 257, 16), (4, 5, 2))          # BT, N, H


def _flat(n, dtype):
    v, buf = _padded(1, n, dtype, DEV)
    return v[0], buf


def _run_kernels(ops, qkv, do_cls, out_a, lse_a, BT, N, H):
    """forward, backward of form a (rounded float64 out / lse handed in) and of form b (the forward's own) -> views, buffers"""
    D = H * 64
    got, bufs = {}, {}

    def new(name, n, dtype, shape):
        v, buf = _flat(n, dtype)
        got[name], bufs[name] = v.view(shape), (buf, n)
        return got[name]

    out = new("out", BT * D, BF16, (BT, D))
    lse = new("lse", BT * H, F32, (BT, H))
    ops.attn_fwd_cls(qkv, out, lse, BT, N, H)
    for form, o, l in (("a", out_a, lse_a), ("b", out, lse)):
        dqkv = new(f"dqkv@{form}", BT * N * 3 * D, BF16, (BT * N, 3 * D))
        ops.attn_bwd_cls(qkv, o, do_cls, l, dqkv, BT, N, H)
    return got, bufs


@pytest.mark.parametrize("BT,N,H", SHAPES)
def test_class_query_kernels_against_float64(BT, N, H):
    from aim_amd import ops
    D = H * 64
    case = AC.Case(f"top/{N}x{H}/BT{BT}", "spatial", BT, N, H, "unit", 4242 + N)
    inp = AC.make_inputs(case)
    inp["do"].view(BT, N, D)[:, 1:] = 0            # the gradient of the attention output is zero outside the class rows
    q, k, v = AC.split(inp["qkv"], BT, N, H, 3)
    do64 = AC.split(inp["do"], BT, N, H)
    fw = AC.forward_ref(q, k, v)
    o_a, l_a, eo, el = AC.handed_in(fw)
    bw = {"a": AC.backward_ref(q, k, v, do64, fw, eo, el), "b": AC.backward_ref(q, k, v, do64, fw, fw["out"][1], fw["lse"][1])}

    qkv = AC._guarded(inp["qkv"], DEV)
    do_cls = AC._guarded(inp["do"].view(BT, N, D)[:, 0].contiguous(), DEV)
    out_a = AC._guarded(o_a[:, :, 0].reshape(BT, D).contiguous(), DEV)
    lse_a = AC._guarded(l_a[:, :, 0].contiguous(), DEV)
    with torch.no_grad():
        got, bufs = _run_kernels(ops, qkv, do_cls, out_a, lse_a, BT, N, H)
        again, _ = _run_kernels(ops, qkv, do_cls, out_a, lse_a, BT, N, H)
        # the full forward kernel on the same input: row 0 of its results
        full_out = torch.empty((BT * N, D), dtype=BF16, device=DEV)
        full_lse = torch.empty((BT, H, N), dtype=F32, device=DEV)
        ops.attn_fwd(qkv, full_out, full_lse.view(-1), BT, N, H)
        # NaN in the q part of every non-class row: nothing the class query's result depends on
        poisoned = inp["qkv"].clone()
        poisoned.view(BT, N, 3 * D)[:, 1:, :D] = float("nan")
        pois, _ = _run_kernels(ops, AC._guarded(poisoned, DEV), do_cls, out_a, lse_a, BT, N, H)
        torch.cuda.synchronize()

    bits = lambda t: t.view(torch.int16 if t.dtype == BF16 else torch.int32)
    for name in got:
        assert _pad_intact(bufs[name][0], 1, bufs[name][1]), f"{name}: wrote outside its buffer"
        assert torch.isfinite(got[name].float()).all(), f"{name}: not finite"
        assert torch.equal(bits(got[name]), bits(again[name])), f"{name}: differs run to run"
        assert torch.equal(bits(got[name]), bits(pois[name])), f"{name}: depends on the q rows of other tokens"
    assert torch.equal(bits(got["out"]), bits(full_out.view(BT, N, D)[:, 0])), "out: not row 0 of aim_attn_fwd"
    assert torch.equal(bits(got["lse"]), bits(full_lse[:, :, 0])), "lse: not row 0 of aim_attn_fwd"

    host = {n_: t.cpu() for n_, t in got.items()}
    checks = {}
    checks["out"] = ratio(host["out"].view(BT, H, 64), fw["out"][0][:, :, 0], fw["out"][1][:, :, 0])
    checks["lse"] = ratio(host["lse"], fw["lse"][0][:, :, 0], fw["lse"][1][:, :, 0])
    for form in "ab":
        dq, dk, dv = AC.split(host[f"dqkv@{form}"], BT, N, H, 3)
        checks[f"dq0@{form}"] = ratio(dq[:, :, 0], bw[form]["dq"][0][:, :, 0], bw[form]["dq"][1][:, :, 0])
        checks[f"dk@{form}"] = ratio(dk, *bw[form]["dk"])
        checks[f"dv@{form}"] = ratio(dv, *bw[form]["dv"])
        assert (dq[:, :, 1:] == 0).all(), f"dq@{form}: a non-class row is not zero"
    print(f"top-block kernels BT={BT} N={N} H={H}: worst error / bound " + ", ".join(f"{k_}={v_:.3f}" for k_, v_ in checks.items()))
    for name, r in checks.items():
        assert r <= 1.0, (name, r)


# ------------------------------------------------------------------------------------------------ model level
CHILD = r'''
import sys, torch
sys.path.insert(0, %r)
import aim_amd
from aim_amd import backbone as bb
from oracle import vit_clip_oracle as O
assert bb._TOP_CLS_ONLY == (sys.argv[2] == "1")
out = {}
#        tag            res  T  patch D    L   H   B   drop checkpoint
CFGS = (("tiny",        32,  2, 16,   128, 2,  2,  2,  0.0, (False, True)),
        ("vitb16",      224, 4, 16,   768, 12, 12, 2,  0.1, (False, True)),
        ("vitb16_b64",  224, 8, 16,   768, 12, 12, 64, 0.1, (False,)))       # the benchmark's shape: B*T = 512 class rows
for tag, res, T, patch, D, L, H, B, drop, ckpts in CFGS:
    for ckpt in ckpts:
        m = aim_amd.ViT_CLIP(res, T, patch, D, L, H, drop, checkpoint=ckpt)
        m.init_weights()
        m.load_state_dict(O.synth_state_dict(O.backbone_param_shapes(res, T, patch, D, L), seed=11), strict=True)
        m = m.to("cuda").train()
        g = torch.Generator().manual_seed(5)
        clips = torch.randn((B, 3, T, res, res), generator=g).to("cuda")
        head = (torch.randn((D, 16), generator=g) * D ** -0.5).to("cuda")
        labels = torch.randint(0, 16, (B,), generator=g).to("cuda")
        torch.manual_seed(7)                  # the DropPath draws
        y = m(clips)                          # [B, D, T, 1, 1]
        loss = torch.nn.functional.cross_entropy(y.flatten(2).mean(-1) @ head, labels)
        loss.backward()
        torch.cuda.synchronize()
        key = tag + (".ckpt" if ckpt else "")
        out[key + ".loss"] = loss.detach().cpu()
        out[key + ".features"] = y.detach().cpu()
        for n, p in m.named_parameters():
            if p.requires_grad:
                assert p.grad is not None, n
                out[key + ".grad." + n] = p.grad.detach().float().cpu()
        del m, y, loss, clips
        torch.cuda.empty_cache()
torch.save(out, sys.argv[1])
''' % ROOT


def _run_model(top: str, path: str):
    env = dict(os.environ, AIM_TOP_CLS_ONLY=top)
    subprocess.run([sys.executable, "-c", CHILD, path, top], check=True, env=env, timeout=900)
    return torch.load(path, weights_only=True)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def test_class_rows_form_equals_full_row_form(tmp_path):
    full = _run_model("0", str(tmp_path / "full.pt"))
    top = _run_model("1", str(tmp_path / "top.pt"))
    assert set(full) == set(top)
    worst = {}
    for k in sorted(full):
        assert torch.isfinite(top[k]).all() and torch.isfinite(full[k]).all(), k
        cfg, kind = (k.split(".grad.")[0], "grad") if ".grad." in k else k.rsplit(".", 1)
        e = _rel(top[k], full[k])
        worst[(cfg, kind)] = max(worst.get((cfg, kind), 0.0), e)
    for (cfg, kind), e in sorted(worst.items()):
        print(f"top block, class rows against all rows: {cfg} {kind}: worst relative L2 {e:.3e}")
    n_grads = 0
    for k in sorted(full):
        e = _rel(top[k], full[k])
        if ".grad." in k:
            n_grads += 1
            assert full[k].norm() > 0, (k, "the full-row gradient is zero: the comparison says nothing")
            assert e <= 2.5e-3, (k, e)
        elif k.endswith(".features"):
            assert e <= 1.5e-3, (k, e)
        else:
            assert k.endswith(".loss") and e <= 1.5e-3, (k, e)
    # every trainable tensor of both models, with and without checkpointing: temporal_embedding, ln_post.{weight,bias}, 12 per layer
    assert n_grads == 2 * (3 + 12 * 2) + 3 * (3 + 12 * 12)
