"""TimeSformer on the MI355X: the stem's full backward (``aim_embed_ln_bwd``) against float64 autograd, the whole backbone
against the reference's own outputs and gradients (tests/golden/timesformer_tiny_{a,b,c}.npz) with its drawn DropPath masks
injected, one real-geometry case against the plain-torch restatement, the requires_grad / no-grad / optimizer contracts, and the
k400 recipe at its per-GPU shape."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_timesformer_cpu as C  # noqa: E402  (MG, REF, rel, fixture_factors, fixture_errors)

MG, REF, rel = C.MG, C.REF, C.rel
F32_BOUND = 1e-5        # tests/test_vit_imagenet_gpu.py holds its fp32 mode to this at the same geometry
BF16_BOUND = 2.5e-2     # ... and its bf16 mode to this, at the same geometry and rounding points


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
STEM_SHAPES = [(2, 2, 5, 128), (1, 3, 197, 768), (1, 2, 257, 1024), (8, 8, 197, 768)]
_OUTS = ("dtok", "dcls", "dpos", "dtemporal", "dgamma", "dbeta")


@functools.lru_cache(maxsize=None)
def _stem_case(B, T, N, D):
    """Inputs (tok and dx hold bf16-representable values, so ONE float64 reference serves the bf16 and the f32 call form) and
    the float64 autograd gradients of sum(dx * LN([cls ; tok] + pos + temporal))."""
    g = torch.Generator().manual_seed(B * 1000 + T * 100 + N + D)
    BT = B * T
    r = lambda *s: torch.randn(s, generator=g)
    tok, dx = r(BT * (N - 1), D).bfloat16().float(), r(BT * N, D).bfloat16().float()
    cls, pos, tmp, gamma, beta = r(D), r(N, D), r(T, D) * 0.5, 1.0 + 0.2 * r(D), 0.1 * r(D)
    leaves = [t.double().requires_grad_(True) for t in (tok, cls, pos, tmp, gamma, beta)]
    tk, c, p, tm, ga, be = leaves
    u = torch.cat([c.expand(BT, 1, D), tk.view(BT, N - 1, D)], 1) + p
    u = (u.view(B, T, N, D) + tm.view(1, T, 1, D)).reshape(BT * N, D)
    y = torch.nn.functional.layer_norm(u, (D,), ga, be, 1e-5)
    ref = dict(zip(_OUTS, torch.autograd.grad(y, leaves, dx.double())))
    return dict(tok=tok, dx=dx, cls=cls, pos=pos, tmp=tmp, gamma=gamma, beta=beta), ref


def _stem_forward(inp, B, T, N, D, bf16):
    """the saved tensors of the fused forward: tok in the path's dtype, ln_pre's statistics from the forward kernel itself"""
    from aim_amd import ops
    d = {k: v.to(DEV) for k, v in inp.items()}
    M = B * T * N
    x, mean, rstd = (torch.empty(s, device=DEV) for s in ((M, D), (M,), (M,)))
    if bf16:
        d["tok"] = d["tok"].bfloat16()
        d["dx"] = d["dx"].bfloat16()
        ops.embed_ln(d["tok"], d["cls"], d["pos"], d["tmp"], d["gamma"], d["beta"], x, mean, rstd, B, T, N, D)
    else:
        ops.embed_ln_f32(d["tok"], d["cls"], d["pos"], d["tmp"], d["gamma"], d["beta"], x, B, T, N, D,
                         pre=torch.empty((M, D), device=DEV), mean=mean, rstd=rstd)
    d.update(mean=mean, rstd=rstd)
    return d


def _stem_backward(d, B, T, N, D, want=_OUTS):
    """one call; the five fp32 outputs start from ones (the kernel ADDS), dtok from NaN (the kernel WRITES)"""
    from aim_amd import ops
    shapes = dict(dtok=(B * T * (N - 1), D), dcls=(D,), dpos=(N, D), dtemporal=(T, D), dgamma=(D,), dbeta=(D,))
    out = {k: (torch.full(shapes[k], float("nan"), dtype=d["dx"].dtype, device=DEV) if k == "dtok"
               else torch.ones(shapes[k], device=DEV)) for k in want}
    ops.embed_ln_bwd(d["dx"], d["tok"], d["cls"], d["pos"], d["tmp"], d["gamma"], d["mean"], d["rstd"], B, T, N, D, **out)
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_embed_ln_bwd_vs_fp64(shape, bf16):
    B, T, N, D = shape
    inp, ref = _stem_case(*shape)
    d = _stem_forward(inp, B, T, N, D, bf16)
    a = _stem_backward(d, B, T, N, D)
    b = _stem_backward(d, B, T, N, D)
    for k in _OUTS:                                          # equal bits on every run
        assert torch.equal(a[k], b[k]), k
    errs = {k: rel(a[k] - 1, ref[k]) for k in _OUTS[1:]}     # the buffers started from ones: the kernel accumulates
    errs["dtok"] = rel(a["dtok"].float(), ref["dtok"])
    print(shape, "bf16" if bf16 else "f32", {k: f"{v:.2e}" for k, v in errs.items()})
    for k in _OUTS[1:]:
        assert errs[k] < 1e-5, (k, errs)
    # one bf16 rounding is at most 2^-9 per element; the factor 2 covers the fp32 arithmetic before it
    assert errs["dtok"] < (2.0 ** -8 if bf16 else 1e-5), errs
    # bit for bit: both are 1 + s with the same s, the (token 0, frame-time t) partial rows added in the same order
    assert torch.equal(a["dcls"], a["dpos"][0])


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_embed_ln_bwd_optional_outputs(bf16):
    """A subset of the outputs gives the bits of the full call for what it asks for (the others are NULL to the kernel)."""
    B, T, N, D = STEM_SHAPES[0]
    inp, _ = _stem_case(B, T, N, D)
    d = _stem_forward(inp, B, T, N, D, bf16)
    full = _stem_backward(d, B, T, N, D)
    for want in (("dtok",), ("dcls",), ("dpos",), ("dtemporal", "dbeta"), ("dgamma",), ("dtok", "dcls", "dgamma")):
        part = _stem_backward(d, B, T, N, D, want)
        assert set(part) == set(want)
        for k in want:
            assert torch.equal(part[k], full[k]), (want, k)


def test_embed_ln_bwd_refuses_before_launching():
    from aim_amd import ops
    B, T, N, D = STEM_SHAPES[0]
    inp, _ = _stem_case(B, T, N, D)
    d = _stem_forward(inp, B, T, N, D, True)
    dpos = torch.ones((N, D), device=DEV)
    args = lambda **kw: [kw.get(k, d[k]) for k in ("dx", "tok", "cls", "pos", "tmp", "gamma", "mean", "rstd")]

    def shifted(t, by):        # the same values starting `by` elements into a larger buffer: misaligned
        buf = torch.empty(t.numel() + by, dtype=t.dtype, device=DEV)
        buf[by:].copy_(t.reshape(-1))
        return buf[by:].view(t.shape)

    with pytest.raises(RuntimeError, match="misaligned"):
        ops.embed_ln_bwd(*args(dx=shifted(d["dx"], 1)), B, T, N, D, dpos=dpos)
    with pytest.raises(RuntimeError, match="misaligned"):
        ops.embed_ln_bwd(*args(pos=shifted(d["pos"], 1)), B, T, N, D, dpos=dpos)
    with pytest.raises(RuntimeError, match="no output"):
        ops.embed_ln_bwd(*args(), B, T, N, D)
    with pytest.raises(ValueError, match="dpos must be contiguous"):
        ops.embed_ln_bwd(*args(), B, T, N, D, dpos=torch.ones((N - 1, D), device=DEV))
    # D above the 2 048 columns a wave holds, and a D that is no multiple of 4 (buffers sized to match: only the shape is wrong)
    for Dbad in (2052, 126):
        z = lambda *s: torch.zeros(s, device=DEV)
        out = torch.ones((2, Dbad), device=DEV)
        with pytest.raises(RuntimeError, match="bad shape"):
            ops.embed_ln_bwd(z(2, Dbad), z(1, Dbad), z(Dbad), z(2, Dbad), z(1, Dbad), z(Dbad), z(2), z(2), 1, 1, 2, Dbad, dpos=out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.ones(2, Dbad))
    torch.cuda.synchronize()
    assert torch.equal(dpos.cpu(), torch.ones(N, D))         # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# whole backbone against the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------
def _build(tag):
    m, T, train, seed = C._build(tag)
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    m.load_state_dict(MG.synth_params(shapes, seed), strict=True)
    return m.to(DEV).train(train), T, train, seed


def _inject(m, factors):
    fac = [tuple(None if v is None else v.to(DEV) for v in f) for f in factors]
    m._drop_factors = lambda T, N, training, dev: fac


def _clip_and_seed(T, seed):
    res = MG.GEOM["input_resolution"]
    return MG.randn((MG.B, 3, T, res, res), seed + 1).to(DEV), MG.randn((MG.B, MG.GEOM["width"], T, 1, 1), seed + 2).to(DEV)


def _run(tag, bound, precision):
    z = np.load(os.path.join(C.GOLDEN, f"timesformer_tiny_{tag}.npz"))
    m, T, train, seed = _build(tag)
    m.set_precision(precision)
    if train:
        _inject(m, C.fixture_factors(z, MG.GEOM["layers"]))
    imgs, g = _clip_and_seed(T, seed)
    names = [str(n) for n in z["names"]]
    assert names == [n for n, _ in m.named_parameters()]
    y = m(imgs)
    grads = torch.autograd.grad(y, [p for _, p in m.named_parameters()], g)
    errs = C.fixture_errors(z, names, y.detach(), grads, seed)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])
    print(tag, precision, "worst:", [(k, f"{v:.2e}") for k, v in worst[:4]])
    assert worst[0][1] <= bound, worst[:8]


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fp32_against_reference_fixture(tag):
    """set_precision('fp32'): output and every gradient at 1e-5 of the reference's own fp32 autograd -- tight enough to see a
    DropPath factor on the wrong side of T_Adapter, or ln_1's weights used for t_norm."""
    _run(tag, F32_BOUND, "fp32")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_bf16_against_reference_fixture(tag):
    _run(tag, BF16_BOUND, "bf16")


# ---------------------------------------------------------------------------------------------------------------------
# real geometry against the restatement
# ---------------------------------------------------------------------------------------------------------------------
REAL = dict(input_resolution=224, patch_size=16, width=128, layers=2, heads=2)
# ViT-L/14's patch at the tiny fixtures' size: K = 3 * 14 * 14 = 588 is no multiple of 64, so the bf16 conv operand is padded to
# Kp = 640 and the conv weight gradient goes through its scratch buffer (patch 16 has K = 768 = Kp)
PAD_K = dict(input_resolution=28, patch_size=14, width=128, layers=2, heads=2)
GEOMS = dict(real=(REAL, 8, 1, 4400), padk=(PAD_K, 2, 2, 4502))       # name -> (geometry, frames, clips, seed)


@functools.lru_cache(maxsize=None)
def _real_case(geom, masked):
    """224 / 16 (N = 197), T = 8, one clip, or 28 / 14 (N = 5), T = 2, two clips: the restatement in float64 on the CPU, with
    drawn factors or without."""
    import aim_amd
    kw, T, B, seed = GEOMS[geom]
    res = kw["input_resolution"]
    N = (res // kw["patch_size"]) ** 2 + 1
    m = aim_amd.TimeSformer(num_frames=T, drop_path_rate=0.5, **kw)
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    sd = MG.synth_params(shapes, seed)
    imgs, g = MG.randn((B, 3, T, res, res), seed + 1), MG.randn((B, kw["width"], T, 1, 1), seed + 2)
    factors = None
    if masked:          # layer 1 of 2 has rate 0.5: factors 0 or 2, drawn here; every vector keeps and drops an entry
        gen = torch.Generator().manual_seed(seed + 3)
        draw = lambda n: (torch.rand(n, generator=gen) < 0.5).float() * 2.0
        factors = [(None, None, None), (draw(T), draw(N), draw(N))]
        assert all(0 < int((v == 0).sum()) < v.numel() for v in factors[1])
    P = {n: v.double().requires_grad_(True) for n, v in sd.items()}
    y = REF.forward(P, imgs.double(), kw["heads"], kw["patch_size"], factors)
    grads = torch.autograd.grad(y, [P[n] for n, _ in shapes], g.double())
    return sd, imgs, g, factors, y.detach(), dict(zip([n for n, _ in shapes], grads))


@pytest.mark.parametrize("geom, masked, precision", [
    ("real", False, "bf16"), ("real", True, "bf16"), ("padk", False, "bf16"), ("padk", True, "bf16"),
    ("padk", False, "fp32"), ("padk", True, "fp32")],
    ids=["eval", "masks", "padk-eval", "padk-masks", "padk-fp32-eval", "padk-fp32-masks"])
def test_real_geometry_against_restatement(geom, masked, precision):
    import aim_amd
    sd, imgs, g, factors, y_ref, g_ref = _real_case(geom, masked)
    kw, T, _, _ = GEOMS[geom]
    m = aim_amd.TimeSformer(num_frames=T, drop_path_rate=0.5, **kw)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train(masked).set_precision(precision)
    if masked:
        _inject(m, factors)
    y = m(imgs.to(DEV))
    grads = torch.autograd.grad(y, [p for _, p in m.named_parameters()], g.to(DEV))
    errs = {"y": rel(y.detach(), y_ref)}
    errs.update({n: rel(gr, g_ref[n]) for (n, _), gr in zip(m.named_parameters(), grads)})
    worst = sorted(errs.items(), key=lambda kv: -kv[1])
    print(geom, precision, "masks" if masked else "eval", "worst:", [(k, f"{v:.2e}") for k, v in worst[:4]])
    assert worst[0][1] <= (BF16_BOUND if precision == "bf16" else F32_BOUND), worst[:8]


# ---------------------------------------------------------------------------------------------------------------------
# contracts
# ---------------------------------------------------------------------------------------------------------------------
def test_frozen_subset_gets_none_and_same_bits_for_the_rest():
    """Frozen: the whole stem, every t_attn / t_norm, one block's MLP weights (not their biases): None for those, and the bits of
    the full run for everything else."""
    z = np.load(os.path.join(C.GOLDEN, "timesformer_tiny_b.npz"))
    frozen_name = lambda n: (not n.startswith(("transformer", "ln_post")) or ".t_attn." in n or ".t_norm." in n
                             or n in ("transformer.resblocks.1.mlp.c_fc.weight", "transformer.resblocks.1.mlp.c_proj.weight"))
    out = []
    for frozen in (False, True):
        m, T, train, seed = _build("b")
        _inject(m, C.fixture_factors(z, MG.GEOM["layers"]))
        if frozen:
            for n, p in m.named_parameters():
                p.requires_grad = not frozen_name(n)
        imgs, g = _clip_and_seed(T, seed)
        m(imgs).backward(g)
        out.append({n: (None if p.grad is None else p.grad.cpu().clone()) for n, p in m.named_parameters()})
    full, part = out
    assert sum(frozen_name(n) for n in full) == 6 + 3 * 6 + 2
    for n in full:
        if frozen_name(n):
            assert part[n] is None and full[n] is not None, n
        else:
            assert part[n] is not None and torch.equal(part[n], full[n]), n


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_no_grad_forward_matches_grad_forward(precision):
    m, T, train, seed = _build("a")
    m.set_precision(precision)
    imgs, _ = _clip_and_seed(T, seed)
    y1 = m(imgs).detach()
    with torch.no_grad():
        y2 = m(imgs)
    assert torch.equal(y1, y2)


def test_two_flat_adamw_steps_then_forward_matches_fresh_model():
    import aim_amd
    from aim_amd.dist import build_optimizer
    m, T, train, seed = _build("a")
    opt = build_optimizer(m, dict(type='AdamW', lr=1e-3, weight_decay=0.05))
    assert type(opt).__name__ == "FlatAdamW" and m.grad_in_place
    imgs, g = _clip_and_seed(T, seed)
    y0 = m(imgs).detach().clone()
    for _ in range(2):
        opt.zero_grad()
        m(imgs).backward(g)
        opt.step()
    y1 = m(imgs).detach()
    fresh = aim_amd.TimeSformer(num_frames=T, **MG.GEOM, **MG.CASES["a"][2])
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    y2 = fresh.to(DEV).eval()(imgs).detach()
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, y2)


def test_fp8_inference_request_warns_and_runs_bf16(caplog):
    m, T, train, seed = _build("a")
    imgs, _ = _clip_and_seed(T, seed)
    with torch.no_grad():
        y16 = m(imgs)
        m.set_inference_precision('fp8')
        with caplog.at_level("WARNING", logger="aim_amd"):
            y8 = m(imgs)
    assert any("no fp8 path" in r.getMessage() for r in caplog.records)
    assert torch.equal(y16, y8)


# ---------------------------------------------------------------------------------------------------------------------
# the reference recipe at its per-GPU shape
# ---------------------------------------------------------------------------------------------------------------------
def test_recipe_two_steps_finite_and_reproducible(tmp_path):
    import aim_amd
    from aim_amd.dist import build_optimizer
    C._write_config_tree(str(tmp_path))
    cfg = aim_amd.Config.fromfile(str(tmp_path / "recognition" / "vit" / "timesformer_k400.py"))

    def train():
        torch.manual_seed(0)
        model = aim_amd.build_model(cfg.model).to(DEV).train()
        opt = build_optimizer(model, dict(cfg.optimizer))
        gen = torch.Generator().manual_seed(9)
        imgs = torch.randn((8, 1, 3, 8, 224, 224), generator=gen).to(DEV)
        label = torch.randint(0, 400, (8, 1), generator=gen).to(DEV)
        torch.manual_seed(3); torch.cuda.manual_seed(3)
        losses = []
        for step in range(2):
            opt.zero_grad()
            loss = model(imgs, label, return_loss=True)["loss_cls"]
            loss.backward()
            if step == 0:
                for n, p in model.named_parameters():
                    assert p.grad is not None and torch.isfinite(p.grad).all(), n
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), {n: p.detach().cpu().clone() for n, p in model.named_parameters()}

    l1, p1 = train()
    l2, p2 = train()
    assert torch.isfinite(l1).all() and torch.equal(l1, l2)
    for n in p1:
        assert torch.equal(p1[n], p2[n]), n
