"""CPU self-check of tests/rowwise_cases.py: the bounds that test_rowwise_gpu.py holds the LayerNorm, embedding, reduction,
row-add and cast kernels to accept an fp32 emulation of each kernel's arithmetic in its summation order, and reject the same
emulation with one plausible kernel bug (a mutant).  Nothing is tuned in between: the bounds are the derivations in the
module docstring of rowwise_cases.py.  The worst emulation error / bound per entry point and output, and the smallest
mutant error / bound over the cases that must see the mutant, are printed.

Which cases must see a mutant is stated by MUST_SEE with the reason; on the other cases the mutant changes nothing, or
changes less than the output format resolves (a bf16 or e4m3 output cannot show a relative change of 1e-5).

The mutant "layernorm_bwd_fsum sums the unrounded dx": the reference of `partial` is stated on the kernel's own stored
bf16 dx, so a sum of fp32 values differs by about 2^-9 |dx| per term against a bound of a few 2^-24: the bound separates
it (smallest factor printed), and it stays in the list.

Also: every branch of every restated host-side rule has a case, every NC template of every NC-templated entry point has a
case, all four (dy, dres) type pairs occur, and every loop seam has a case on each side."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowwise_cases as rc  # noqa: E402

CASES = rc.cases()
KINDS = sorted(rc.KINDS)


@pytest.fixture(scope="module")
def inputs():
    return {c.name: rc.build_inputs(c) for c in CASES}


@pytest.mark.parametrize("kind", KINDS)
def test_bounds_accept_the_emulation(kind, inputs):
    worst, n = {}, 0
    for c in CASES:
        if c.kind != kind:
            continue
        n += 1
        inp = inputs[c.name]
        got = rc.emulate(c, inp)
        for k, r in rc.compare(c, inp, got).items():
            key = k.rstrip("0123456789")
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, (c.name, k, r)
        for k, v in got.items():
            assert torch.isfinite(v.float()).all(), (c.name, k)
    print(f"{kind}: {n} cases, worst emulation error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert n > 0


def _f32_out(c):
    return c.kind == "embed_ln" or c.p.get("variant") == "f32"


# (kind, mutant) -> the cases that must be outside the bound, with the reason for leaving the others out
MUST_SEE = {
    # eps outside the root changes rstd by eps / sqrt(var) against eps / (2 var): visible in an fp32 y where var is far from
    # 1 (scaled rows, constant rows); at var = 1 the two differ by eps / 2, a few fp32 ulps
    ("ln_fwd", "eps_outside"): lambda c: _f32_out(c) and c.family in ("scaled", "const"),
    ("embed_ln", "eps_outside"): lambda c: c.family == "const",
    # D / (D - 1) is 1 + 1 / D: visible in fp32 at every D (constant rows: var = 0 either way)
    ("ln_fwd", "unbiased"): lambda c: _f32_out(c) and c.family != "const",
    ("embed_ln", "unbiased"): lambda c: c.family != "const",
    # E[x^2] - mean^2 in fp32 cancels at |mean| = 300 sigma
    ("ln_fwd", "one_pass"): lambda c: _f32_out(c) and c.family == "offset",
    # the padded count differs from D unless D = 256 NC
    ("ln_fwd", "mean_padded"): lambda c: _f32_out(c) and c.p["D"] != 256 * rc.ln_nc(c.p["D"]) and c.family != "scaled",
    ("embed_ln", "mean_padded"): lambda c: c.p["D"] != 256 * rc.ln_nc(c.p["D"]),
    # (one clip: bt = bt % T; const: every temporal row is equal)
    ("embed_ln", "temporal_bt"): lambda c: c.family != "const" and c.p["B"] > 1,
    ("nopre_fwd", "temporal_bt"): lambda c: c.p["B"] > 1,
    ("embed_bwd", "temporal_bt"): lambda c: c.family not in ("zero_dy", "const") and c.p["B"] > 1,
    # the two means vanish with dy; on constant rows xhat = 0 and m2 multiplies nothing
    ("ln_bwd", "no_m1"): lambda c: c.family != "zero_dy",
    ("ln_bwd", "no_m2"): lambda c: c.family not in ("zero_dy", "const"),
    ("ln_fsum", "no_m2"): lambda c: c.family != "zero_dy",
    ("embed_bwd", "no_m1"): lambda c: c.family != "zero_dy",
    ("ln_bwd", "dres_before_scale"): lambda c: bool(c.p.get("dres")),
    ("ln_bwd", "dres_at_lddx"): lambda c: c.p["form"] == "classrow",
    ("ln_bwd", "assign"): lambda c: bool(c.p.get("dparam")),
    ("ln_gb", "assign"): lambda c: True,
    ("embed_bwd", "assign"): lambda c: True,
    ("colsum", "assign"): lambda c: True,
    ("nopre_bwd", "assign"): lambda c: set(c.p["outs"]) != {"dtok"},
    ("elem", "assign"): lambda c: c.p["op"] in ("add_rows", "add_bf16", "acc_bf16"),
    ("colsum", "at_div"): lambda c: bool(c.p.get("at")) and c.p["M"] > 1,
    ("colsum", "af_mod"): lambda c: bool(c.p.get("af")) and c.p["M"] > 1,
    ("ln_fsum", "group_off_by_one"): lambda c: True,
    ("ln_fsum", "w_next"): lambda c: c.p["w"] != "none" and c.p["ntok"] > 1,
    ("ln_fsum", "fsum_unrounded"): lambda c: c.family != "zero_dy",                # (dy = 0: dx = dres, already bf16)
    ("frame_sum", "w_next"): lambda c: c.p["w"] and c.p["ntok"] > 1,
    ("nopre_bwd", "dbias_with_cls"): lambda c: "dbias" in c.p["outs"],
    ("nopre_bwd", "dtok_shift"): lambda c: "dtok" in c.p["outs"],
    ("cast", "no_transpose"): lambda c: c.p["mode"].startswith("transpose") and c.p["R"] == c.p["C"],
    ("cast", "truncate"): lambda c: True,
    ("cast_multi", "no_transpose"): lambda c: True,
    ("cast_multi", "truncate"): lambda c: True,
    ("elem", "truncate"): lambda c: c.p["op"] != "acc_bf16",                       # (acc_bf16 writes fp32)
    ("elem", "s_next"): lambda c: c.p["op"] == "scale_rows" and c.p["R"] > 1,
}


def test_every_mutant_of_every_kind_is_listed():
    assert set(MUST_SEE) == {(k, m) for k in rc.KINDS for m in rc.KINDS[k][4]}


@pytest.mark.parametrize("kind,mut", sorted(MUST_SEE))
def test_bounds_reject_the_mutant(kind, mut, inputs):
    seen, least = 0, None
    for c in CASES:
        if c.kind != kind or not MUST_SEE[(kind, mut)](c):
            continue
        inp = inputs[c.name]
        r = max(rc.compare(c, inp, rc.emulate(c, inp, mut)).values())
        assert r > 1.0, (c.name, mut, r)
        seen += 1
        least = r if least is None else min(least, r)
    assert seen > 0, (kind, mut)
    print(f"{kind} {mut}: outside the bound on {seen} cases, by a factor of {least:.3g} at least")


def test_zero_dy_is_exact_in_the_emulation(inputs):
    n = 0
    for c in CASES:
        if c.family != "zero_dy" or c.kind not in ("ln_bwd", "ln_fsum"):
            continue
        inp = inputs[c.name]
        got = rc.emulate(c, inp)
        for k in ("dx", "dxb"):
            if k in got and c.p.get("form") != "classrow":
                want = inp["dres"].float() if "dres" in inp else torch.zeros_like(got[k].float())
                assert torch.equal(got[k].float(), want.to(got[k].dtype).float()), (c.name, k)
                n += 1
        for k in ("dgamma", "dbeta"):
            if k in got:
                assert torch.equal(got[k], inp[k + "0"]), (c.name, k)
    assert n >= 6


def _by(kind):
    return [c for c in CASES if c.kind == kind]


def test_catalogue_covers_every_branch_and_seam():
    # NC templates of every NC-templated entry point (ln_fwd: each of its three entry points)
    for kind in rc.NC_KINDS:
        groups = {"": _by(kind)} if kind != "ln_fwd" else {v: [c for c in _by(kind) if c.p["variant"] == v] for v in ("f32", "x16", "fp8")}
        for tag, cs in groups.items():
            assert {rc.ln_nc(c.p["D"]) for c in cs} == {1, 2, 3, 4, 8}, (kind, tag)
    ds = {c.p["D"] for c in _by("ln_fwd")}
    assert {4, 252, 256, 260, 512, 768, 1024, 1028, 1280, 2048} <= ds                # one live lane; partly filled last chunks
    assert {c.p["rows"] for c in _by("ln_fwd")} >= {1, 3, 4, 5, 394}
    assert {c.eps for c in CASES} == {1e-5, 1e-6} and {c.family for c in CASES} == set(rc.FAMILIES)
    # layernorm_bwd: type pairs, output sets, forms, statistics forms, both dparam routes at their threshold
    bw = _by("ln_bwd")
    for D in rc.LN_D_CORE:
        at = [c for c in bw if c.p["D"] == D]
        assert {(c.p["dy"], c.p.get("dres")) for c in at} >= {(a, b) for a in ("f32", "bf16") for b in ("f32", "bf16", None)}, D
        assert {c.p["outs"] for c in at} == {"dx", "dxb", "both"} and {c.p["form"] for c in at} == {"strided", "dense", "classrow", "zshift"}
    assert {c.p.get("stats", "a") for c in bw} == {"a", "b"}
    dp = [c for c in bw if c.p.get("dparam")]
    assert {c.p["rows"] for c in dp} >= set(rc.DPARAM_ROWS) and {c.p["dy"] for c in dp} == {"f32", "bf16"}
    assert {rc.ln_dparam_route(c.p["rows"], True) for c in dp} == {"ordered", "atomic"}
    assert rc.ln_dparam_route(8192, True) == "ordered" and rc.ln_dparam_route(8193, True) == "atomic" and rc.ln_dparam_route(5, False) is None
    # ln_dparam_kernel's unrolled loop (r + 12 < rows, step 16): group 0 enters it from 13 rows on, twice from 29
    assert {12, 13, 16, 17, 29} <= {c.p["rows"] for c in dp}
    # layernorm_gb_bwd: one slab | two | three; 16-row slabs up to 16384 rows, ceil(rows / 1024) beyond; two column blocks
    gb = _by("ln_gb")
    assert {rc.gb_slabs(c.p["rows"]) for c in gb} >= {(16, 1), (16, 2), (16, 3), (17, 964)}
    assert rc.gb_slabs(16384) == (16, 1024) and rc.gb_slabs(16385) == (17, 964)
    assert any(c.p["D"] > 1024 for c in gb) and any(c.p.get("strided") for c in gb) and {c.p["which"] for c in gb} == {"both", "dgamma", "dbeta"}
    # layernorm_bwd_fsum: empty token groups (ntok < groups), one token per group, uneven last group, w NULL / with zeros
    fs = _by("ln_fsum")
    assert {c.p["ntok"] for c in fs} >= set(rc.FSUM_NTOK) and {c.p["groups"] for c in fs} == {1, 4, 13}
    assert {c.p["frames"] for c in fs} == {1, 3} and {c.p["w"] for c in fs} == {"none", "zeros"}
    assert any(c.p["ntok"] < c.p["groups"] for c in fs) and any(c.p["ntok"] % c.p["groups"] for c in fs)
    # frame_sum: both sides of t + 28 < ntok for group 0 (28 | 29) and of the second round (60 | 61); frames = 1; D = 4, 6144
    fr = _by("frame_sum")
    assert {c.p["ntok"] for c in fr} >= set(rc.FRAME_NTOK) and {c.p["x"] for c in fr} == {"f32", "bf16"} and {c.p["w"] for c in fr} == {True, False}
    assert any(c.p["frames"] == 1 and c.p["ntok"] > 1000 for c in fr) and {4, 6144} <= {c.p["D"] for c in fr}
    # colsum: every route, both sides of 64 | 65 and 2048 | 2049 rows, workspace one float short, every shape that forces the scalar kernel
    cs = _by("colsum")
    plans = {(rc.colsum_plan(c.p)[0], c.p["ws"]) for c in cs}
    assert plans >= {("two_stage", "exact"), ("one_block", "exact"), ("one_block", "none"), ("one_block", "short"),
                     ("atomic8", "none"), ("atomic8", "short"), ("scalar", "exact")}, plans
    assert {c.p["M"] for c in cs} >= set(rc.COLSUM_M) and {c.p["C"] for c in cs} >= set(rc.COLSUM_C)
    sc = [c for c in cs if rc.colsum_plan(c.p)[0] == "scalar"]
    assert {(c.p["C"] % 8 != 0, c.p["C"] > 2048, (c.p.get("ldx") or c.p["C"]) % 8 != 0) for c in sc} >= \
        {(True, False, True), (False, True, False), (False, False, True)}
    # colsum8: row slots that do not fill the block (C / 8 = 3: 85 slots, thread 255 idle) and one slot per row (C = 2048)
    assert {256 % (c.p["C"] // 8) != 0 for c in cs if rc.colsum_plan(c.p)[0] != "scalar"} == {True, False}
    assert any(c.p.get("af") and c.p.get("at") and 64 % c.p["ntok"] for c in cs)
    # embed_bwd: chunks below, at and above ceil(2048 / T); the finish loop's seam (28 | 29) and 1, 32, 33 chunks; both routes
    eb = _by("embed_bwd")
    ch = {(rc.embed_bwd_chunks(c.p["B"], c.p["T"], c.p["N"]), (c.p["B"] * c.p["N"] + 3) // 4, (2048 + c.p["T"] - 1) // c.p["T"]) for c in eb}
    assert any(a == raw < want for a, raw, want in ch) and any(a == raw == want for a, raw, want in ch) and any(a == want < raw for a, raw, want in ch)
    assert {a for a, _, _ in ch} >= {1, 28, 29, 32, 33}
    assert {(c.p["dx"], c.p["ws"]) for c in eb} >= {("f32", True), ("bf16", False), ("bf16", True), ("f32", False)}
    # embed_nopre_bwd: every subset the issue names, both dx types
    nb = _by("nopre_bwd")
    assert {tuple(c.p["outs"]) for c in nb} == {rc.NOPRE_OUTS} | {(k,) for k in rc.NOPRE_OUTS} and {c.p["dx"] for c in nb} == {"f32", "bf16"}
    # casts: every kernel of aim_cast_bf16 at every shape; every path of cast_multi
    ca = _by("cast")
    assert {(c.p["R"], c.p["C"], c.p["mode"]) for c in ca} == {(R, C, m) for R, C in rc.CAST_SHAPES for m in rc.CAST_MODES}
    assert {rc.cast_route(c.p["mode"].startswith("transpose"), {"dense": 0, "strided": c.p["C"] + 8}.get(c.p["mode"], 1), c.p["C"])
            for c in ca} == {"dense", "strided", "transpose"}
    assert {rc.cast_multi_route(rc.cast_multi_desc(*e)) for e in rc.cast_multi_entries()} == {"wide4", "tile32", "scalar", "copy32"}
    assert any(e[3] for e in rc.cast_multi_entries())
    assert {c.p["op"] for c in _by("elem")} == {"scale_rows", "add_rows", "add_bf16", "acc_bf16"}


def test_families_are_what_they_are_named_for():
    g = torch.Generator().manual_seed(1)
    x = rc._family_x("offset", 5, 768, g)
    assert (x.mean(1) > 299).all() and (x.std(1) < 1.2).all()
    x = rc._family_x("scaled", 5, 768, g)
    v = x.var(1)
    assert v[0] < 2e-6 and v[-1] > 5e5
    x = rc._family_x("const", 5, 768, g)
    assert (x.var(1) == 0).all() and (x[2] == 0).all() and (x[0] != 0).all()


def test_references_agree_with_float64_autograd():
    """the closed forms of rowwise_cases.py against torch's own float64 layer_norm and its autograd gradients"""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(9)
    rows, D, eps = 7, 260, 1e-5
    x = torch.randn((rows, D), generator=g, dtype=torch.float64, requires_grad=True)
    G = torch.randn(D, generator=g, dtype=torch.float64, requires_grad=True)
    B = torch.randn(D, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((rows, D), generator=g, dtype=torch.float64)
    dres = torch.randn((rows, D), generator=g, dtype=torch.float64)
    y = F.layer_norm(x, (D,), G, B, eps)
    (y * dy).sum().backward()
    e = rc.ln_fwd_expected(x.detach(), G.detach(), B.detach(), eps, rc.ln_nc(D))
    assert torch.allclose(e["y"][0], y.detach(), rtol=1e-12, atol=1e-12)
    mu, rs = e["mean"][0][:, None], e["rstd"][0][:, None]
    dx, _ = rc.ln_bwd_expected(dy, x.detach(), G.detach(), mu, rs, dres, rc.ln_nc(D))
    assert torch.allclose(dx, x.grad + dres, rtol=1e-10, atol=1e-12)
    case = rc.Case("x", "ln_gb", dict(rows=rows, D=D, dy="f32", which="both"))
    inp = {"x": x.detach(), "dy": dy, "mean": mu[:, 0], "rstd": rs[:, 0], "dgamma0": torch.zeros(D), "dbeta0": torch.zeros(D)}
    exp = rc.ln_gb_expected(case, inp)
    assert torch.allclose(exp["dgamma"][0], G.grad, rtol=1e-10, atol=1e-12) and torch.allclose(exp["dbeta"][0], B.grad, rtol=1e-10, atol=1e-12)
    # embed_bwd: d temporal through ln_pre, on the embedding the kernels add up in fp32
    c = next(c for c in CASES if c.kind == "embed_bwd" and c.p["D"] == 260 and c.family == "unit" and c.p.get("stats") != "b")
    inp = rc.build_inputs(c)
    p = c.p
    tmp = inp["temporal"].double().requires_grad_(True)
    a = torch.cat([inp["cls"].double().expand(p["B"] * p["T"], 1, p["D"]), inp["tok"].double().view(p["B"] * p["T"], p["N"] - 1, p["D"])], 1)
    t = torch.arange(p["B"] * p["T"]) % p["T"]
    v = a + inp["pos"].double()[None] + tmp[t][:, None, :]
    yy = F.layer_norm(v, (p["D"],), inp["gamma"].double(), None, c.eps)
    (yy.view(-1, p["D"]) * inp["dx"].double()).sum().backward()
    ref = rc.embed_bwd_expected(c, inp)["dtemporal"][0] - inp["dtemporal0"].double()
    assert torch.allclose(ref, tmp.grad, rtol=1e-4, atol=1e-5)      # (the statistics handed in are fp32 roundings)
