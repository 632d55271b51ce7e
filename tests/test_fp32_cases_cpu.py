"""CPU self-check of tests/fp32_cases.py: the bounds that test_fp32_cases_gpu.py holds the reference-precision kernels to accept
an fp32 evaluation of each kernel's arithmetic (`emulate`), and reject the same evaluation with one plausible kernel bug (a
mutant).  Nothing is tuned in between: the bounds are the derivations in the module docstring of fp32_cases.py.  The worst
emulation error / bound per kind and output, and the smallest mutant error / bound over the cases that must see the mutant,
are printed.

Which cases must see a mutant is stated by fp32_cases.MUST_SEE with the reason (`mutants(case)` reads it per case); on the
other cases the mutant changes nothing.

Also: every branch of every restated host-side rule has a case, every fp32 entry point of include/aim_kernels.h has a case
kind, the refusal table matches the AIM_CHECK_ARG lines of fp32.hip, case names are unique, the families are what they are named for, and the closed forms agree with float64 autograd."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_cases as fc  # noqa: E402

CASES = fc.cases()
KINDS = sorted(fc.KINDS)


def _inputs(c):
    return fc.build_inputs(c)


@pytest.mark.parametrize("kind", KINDS)
def test_bounds_accept_the_emulation(kind):
    worst, n = {}, 0
    for c in CASES:
        if c.kind != kind:
            continue
        n += 1
        inp = _inputs(c)
        got = fc.emulate(c, inp)
        for k, r in fc.compare(c, inp, got).items():
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (c.name, k, r)
        for k, v in got.items():
            assert torch.isfinite(v.float()).all(), (c.name, k)
    print(f"{kind}: {n} cases, worst emulation error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert n > 0


def _p(c, k, default=None):
    return c.p.get(k, default)


PAIRS = sorted((k, m) for k in fc.KINDS for m in fc.KINDS[k][4])


def test_every_mutant_of_every_kind_is_listed():
    """fp32_cases.MUST_SEE states, per mutant, the cases that must see it (with the reason for leaving the others out), and
    mutants(case) is that listing read per case"""
    assert set(fc.MUST_SEE) == {m for _, m in PAIRS}
    assert all(fc.KINDS[k][4] for k in fc.KINDS)                      # no kind without a mutant
    for c in CASES:
        assert set(fc.mutants(c)) == {m for m in fc.KINDS[c.kind][4] if fc.MUST_SEE[m](c)}


@pytest.mark.parametrize("kind,mut", PAIRS)
def test_bounds_reject_the_mutant(kind, mut):
    seen, least = 0, None
    for c in CASES:
        if c.kind != kind or mut not in fc.mutants(c):
            continue
        inp = _inputs(c)
        r = max(fc.compare(c, inp, fc.emulate(c, inp, mut)).values())
        assert r > 1.0, (c.name, mut, r)
        seen += 1
        least = r if least is None else min(least, r)
    assert seen > 0, (kind, mut)
    print(f"{kind} {mut}: outside the bound on {seen} cases, by a factor of {least:.3g} at least")


def test_zero_do_is_exact_in_the_emulation():
    n = 0
    for c in CASES:
        if c.kind == "attn_bwd" and c.family == "zero_do":
            got = fc.emulate(c, _inputs(c))
            assert all(bool((v == 0).all()) for v in got.values()), c.name
            n += 1
    assert n >= 40


def _by(kind):
    return [c for c in CASES if c.kind == kind]


def test_catalogue_covers_every_entry_point_branch_and_seam():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert set(fc.ENTRY) == set(fc.KINDS) == {c.kind for c in CASES}
    assert {s for v in fc.ENTRY.values() for s in v} == fc.header_symbols()
    # gemm_f32
    gm = _by("gemm")
    plain = [c for c in gm if _p(c, "batch", 1) == 1]
    for v in fc.GEMM_MN:
        assert {c.p["N"] for c in plain if c.p["M"] == v} >= {20, 129} and {c.p["M"] for c in plain if c.p["N"] == v} >= {20, 129}, v
    assert {c.p["K"] for c in gm} >= set(fc.GEMM_K) and {c.family for c in gm} == set(fc.GEMM_FAMILIES)
    assert {c.p["epi"] for c in gm} == set(fc.EPI)
    assert any(_p(c, "a_off") for c in gm) and any(_p(c, "w_off") for c in gm) and any(_p(c, "a_pad") for c in gm) and any(_p(c, "w_pad") for c in gm)
    lin = [c for c in gm if c.p["epi"] == "lin" and _p(c, "ntok")]
    assert {(c.p["ntok"], bool(_p(c, "bias")), bool(_p(c, "af")), bool(_p(c, "at"))) for c in lin} >= \
        {(n, b, af, at) for n in fc.NTOKS for b in (False, True) for af, at in ((True, False), (False, True), (True, True))}
    f32 = [c for c in gm if c.p["epi"] == "f32"]
    assert {(bool(_p(c, "resid")), _p(c, "vec") or "", bool(_p(c, "rbo"))) for c in f32} >= \
        {(r, v, o) for r in (False, True) for v in ("", "frame", "row0") for o in (False, True)}
    assert {bool(_p(c, "bt")) for c in f32 if _p(c, "vec")} == {False, True}              # ldv: 0 and not 0, with and without bt
    act = [c for c in gm if c.p["epi"] == "act"]
    assert {fc.split_branch(_p(c, "n_split", 0), c.p["N"]) for c in act} == {"none", "inside", "all_first"}
    assert {(_p(c, "act"), _p(c, "n_split"), bool(_p(c, "out2"))) for c in act} >= \
        {(a, ns, o) for a in (0, 1) for ns in (0, 4, 36, 64, 68) for o in (False, True)}
    dact = [c for c in gm if c.p["epi"] == "dact"]
    assert {fc.split_branch(_p(c, "n_split", 0), c.p["N"]) for c in dact} == {"none", "inside", "all_first"}
    assert {(_p(c, "act"), bool(_p(c, "af")), bool(_p(c, "at"))) for c in dact} >= {(a, f, t) for a in (0, 1) for f, t in ((1, 0), (0, 1), (1, 1))}
    assert {(c.p["M"], c.p["batch"]) for c in gm if _p(c, "batch", 1) > 1} == {(5, 3), (197, 3)}
    assert {i for c in gm for i in _p(c, "ident", ())} == {"repeat", "strided_eq_dense", "row_alone", "out2_split"}
    # attention: every N, in rising order; every family on every 7th; both sides of each acceptance limit
    for kind, top, fams in (("attn_fwd", fc.ATTN_FWD_MAX, fc.ATTN_FAMILIES[:-1]), ("attn_bwd", fc.ATTN_BWD_MAX, fc.ATTN_FAMILIES)):
        sweep = [c.p["N"] for c in _by(kind) if c.family == "unit" and c.p["BT"] == 2 and c.p["H"] == 2]
        assert sweep == list(range(1, top + 1)), kind
        for N in range(7, top + 1, 7):
            assert {c.family for c in _by(kind) if c.p["N"] == N} >= set(fams), (kind, N)
        assert {(c.p["N"], c.p["H"], c.p["BT"]) for c in _by(kind)} >= {(197, 12, 1), (197, 12, 2), (257, 16, 1), (257, 16, 2)}
        assert any("nan_neighbours" in _p(c, "ident", ()) and c.p["BT"] == 3 for c in _by(kind))
    assert fc.attn_fwd_accepts(fc.ATTN_FWD_MAX) and not fc.attn_fwd_accepts(fc.ATTN_FWD_MAX + 1)
    assert fc.attn_bwd_accepts(fc.ATTN_BWD_MAX) and not fc.attn_bwd_accepts(fc.ATTN_BWD_MAX + 1)
    # sequences
    for kind in ("cls_fwd", "cls_bwd"):
        cs = _by(kind)
        assert {c.p["T"] for c in cs} == set(range(1, 33))
        assert {(c.p["B"], c.p["H"], c.p["N"]) for c in cs} == {(B, H, N) for B in (1, 3) for H in (1, 12) for N in (2, 5, 197)}
        assert {c.family for c in cs} == set(fc.SEQ_FAMILIES)
    for kind in ("tattn_fwd", "tattn_bwd"):
        assert {(c.p["B"], c.p["T"], c.p["N"], c.p["H"]) for c in _by(kind)} == set(fc.TATTN_SHAPES)
        assert {c.family for c in _by(kind)} == set(fc.SEQ_FAMILIES)
    # lamda
    lm = _by("lambda")
    assert {c.p["N"] for c in lm} >= set(fc.LAMBDA_N) and {c.p["D"] for c in lm} == set(fc.LAMBDA_D)
    assert {c.family for c in lm} == set(fc.LAMBDA_FAMILIES) and {c.p["BT"] for c in lm} >= {1, 24}
    assert {c.p["lds"] - c.p["N"] for c in lm} == {0, 3} and {c.p["ldkx"] // c.p["D"] for c in lm} == {1, 2}
    assert {bool(c.p["one_minus"]) for c in lm} == {False, True}
    # wgrad: the chunk cap hit or not, a last chunk with no rows under the cap, every M, every Nw and Kw
    wg = _by("wgrad")
    assert {c.p["M"] for c in wg} == set(fc.WGRAD_M)
    assert {c.p["Nw"] for c in wg} >= set(fc.WGRAD_NK) and {c.p["Kw"] for c in wg} >= set(fc.WGRAD_NK)
    assert {(c.p["M"] + 511) // 512 > 64 for c in wg} == {False, True}
    assert {fc.wgrad_f32_chunks(c.p["M"]) for c in wg} >= {1, 2, 3, 64}
    empty = [c for c in wg if (fc.wgrad_f32_chunks(c.p["M"]) - 1) * fc.wgrad_f32_chunk(c.p["M"]) >= c.p["M"]]
    assert {c.p["M"] for c in empty} == {32769, 40000} and all(fc.wgrad_f32_chunks(c.p["M"]) == 64 for c in empty)
    assert (fc.wgrad_f32_chunks(1), fc.wgrad_f32_chunk(1)) == (1, 16) and (fc.wgrad_f32_chunks(513), fc.wgrad_f32_chunk(513)) == (2, 272)
    assert fc.wgrad_f32_workspace_bytes(40000, 8, 8) == 64 * 72 * 4
    assert {(bool(c.p["db"]), c.p["ntok"]) for c in wg} == {(False, 0), (True, 0), (True, 5), (True, 197)}
    assert any(c.p["ntok"] and c.p["M"] % c.p["ntok"] for c in wg)
    # embed_ln, patchify
    em = _by("embed_ln")
    assert {(c.p["B"], c.p["T"], c.p["N"], c.p["D"]) for c in em} == set(fc.EMBED_SHAPES)
    assert {c.family for c in em} == set(fc.EMBED_FAMILIES) and {c.p["eps"] for c in em} == {1e-5, 1e-6} and {c.p["stats"] for c in em} == {False, True}
    pt = _by("patchify")
    assert {(c.p["p"], c.p["H"], c.p["W"]) for c in pt} == set(fc.PATCH_SHAPES)
    assert {(c.p["Kp"] > 3 * c.p["p"] ** 2, c.p["dtype"], c.p["norm"]) for c in pt} == {(k, d, n) for k in (False, True) for d in ("f32", "u8")
                                                                                        for n in (False, True)}
    bl = _by("patchify_blend")
    assert {(c.p["mode"], tuple(c.p["partner"]) == (0, 1, 2)) for c in bl} == {(1, True), (1, False), (2, True), (2, False)}
    assert {c.p["lam"] for c in bl if c.p["mode"] == 1} == {0.0, 1.0, 0.3}
    assert all(any(t in c.name for c in bl) for t in ("empty", "full", "offgrid"))
    assert set(fc.REFUSAL_TEXT) >= {"gemm_f32/lda<K", "gemm_f32/ldr<N", "gemm_f32/ldv<N", "patchify_blend_f32/Kp%4"}


def test_families_are_what_they_are_named_for():
    g = torch.Generator().manual_seed(3)
    q, k, v = fc._attn_family("big", 1, 65, 1, g)
    s = (q[0, :, 0].double() @ k[0, :, 0].double().t()) / 8
    assert s.abs().max() > 200                                            # exp overflows in fp32 without the shift
    q, k, v = fc._attn_family("neg100", 1, 8, 1, g)
    s = (q[0, :, 0].double() @ k[0, :, 0].double().t()) / 8
    assert (s[:, 1::2] < -90).all() and (s[:, 0::2].abs() < 10).all()
    q, k, v = fc._attn_family("cls_sink", 1, 30, 1, g)
    assert ((q[0, :, 0].double() @ k[0, :, 0].double().t()).argmax(1) == 0).float().mean() > 0.8
    for fam, lo, hi in (("cw_dominant", 1 - 1e-6, 1.0), ("ow_dominant", 1e-8, 1e-4), ("unit", 0.01, 0.6)):
        c = fc.Case("x", "lambda", dict(BT=2, N=5, D=64, lds=5, ldkx=64, one_minus=True), fam, 1)
        lam = fc._lambda_core(fc.build_inputs(c), torch.float64)["lam"]
        assert ((lam >= lo) & (lam <= hi)).all(), (fam, lam)
    c = fc.Case("x", "lambda", dict(BT=2, N=5, D=64, lds=5, ldkx=64, one_minus=True), "huge", 1)
    core = fc._lambda_core(fc.build_inputs(c), torch.float64)
    assert core["a"].abs().max() > 150 and core["ss"].abs().max() > 100
    c = next(c for c in CASES if c.kind == "gemm" and c.family == "cancel" and c.p["K"] >= 64 and c.p["epi"] == "lin")
    inp = fc.build_inputs(c)
    acc = inp["A"].double() @ inp["W"].double().t()
    S = inp["A"].double().abs() @ inp["W"].double().abs().t()
    assert (acc.abs() / S).median() < 0.05
    for t in (inp["A"], inp["W"]):                                        # full fp32 values, not bf16-representable
        assert (t.bfloat16().float() != t).float().mean() > 0.9


def test_references_agree_with_float64_autograd():
    """the closed forms of fp32_cases.py against torch's own float64 autograd"""
    F = torch.nn.functional
    c = next(c for c in CASES if c.kind == "attn_bwd" and c.p["N"] == 14 and c.family == "unit")
    inp = fc.build_inputs(c)
    q, k, v = (fc._heads(inp[n]).double().requires_grad_(True) for n in ("q", "k", "v"))
    out = F.scaled_dot_product_attention(q, k, v)
    (out * fc._heads(inp["dO"]).double()).sum().backward()
    exp = fc.attn_expected(c, inp)
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        assert torch.allclose(fc._heads(exp[n][0]), t.grad, rtol=1e-10, atol=1e-12), n
    cf = next(x for x in CASES if x.kind == "attn_fwd" and x.p["N"] == 14 and x.family == "unit")
    inpf = fc.build_inputs(cf)
    ref = F.scaled_dot_product_attention(*(fc._heads(inpf[n]).double() for n in ("q", "k", "v")))
    assert torch.allclose(fc._heads(fc.attn_expected(cf, inpf)["out"][0]), ref, rtol=1e-10, atol=1e-12)
    # activations and their derivatives
    x = torch.linspace(-6, 6, 101, dtype=torch.float64, requires_grad=True)
    for act, f in ((fc.GELU, lambda t: F.gelu(t)), (fc.QGELU, lambda t: t * torch.sigmoid(fc.C1702 * t))):
        y = f(x)
        assert torch.allclose(fc._act64(x.detach(), act), y.detach(), rtol=1e-12, atol=1e-14)
        (gr,) = torch.autograd.grad(y.sum(), x)
        assert torch.allclose(fc._dact64(x.detach(), act), gr, rtol=1e-10, atol=1e-12)
    # embed_ln against layer_norm
    c = next(c for c in CASES if c.kind == "embed_ln" and c.p["D"] == 100 and c.family == "unit" and c.p["stats"])
    inp = fc.build_inputs(c)
    v = fc._embed_value(c.p, inp).double().reshape(-1, 100)
    y = F.layer_norm(v, (100,), inp["gamma"].double(), inp["beta"].double(), c.p["eps"])
    assert torch.allclose(fc.embed_expected(c, inp)["x"][0], y, rtol=1e-10, atol=1e-12)
    # wgrad against autograd of G = X W^T
    c = next(c for c in CASES if c.kind == "wgrad" and c.p["M"] == 17 and c.p["db"] and not c.p["ntok"])
    inp = fc.build_inputs(c)
    Wt = torch.zeros((c.p["Nw"], c.p["Kw"]), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c.p["Nw"], dtype=torch.float64, requires_grad=True)
    ((inp["A"].double() @ Wt.t() + b) * inp["G"].double()).sum().backward()
    exp = fc.wgrad_expected(c, inp)
    assert torch.allclose(exp["dW"][0] - inp["dW0"].double(), Wt.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(exp["db"][0] - inp["db0"].double(), b.grad, rtol=1e-10, atol=1e-12)
    # patchify against unfold of the frames
    c = next(c for c in CASES if c.kind == "patchify" and c.p["p"] == 14 and c.p["dtype"] == "f32" and not c.p["norm"] and c.p["Kp"] == 588)
    inp = fc.build_inputs(c)
    p = c.p
    fr = inp["img"].permute(0, 2, 1, 3, 4).reshape(p["B"] * p["T"], 3, p["H"], p["W"])
    ref = F.unfold(fr, p["p"], stride=p["p"]).transpose(1, 2).reshape(-1, 588)
    assert torch.equal(fc.patchify_expected(c, inp)["A"][0].float(), ref)


def test_refusal_table_covers_every_check_of_the_file():
    """every AIM_CHECK_ARG message of csrc/fp32.hip is matched by a REFUSAL_TEXT entry of its entry point, and every entry's
    text occurs in a message of its entry point (the calls themselves run on the GPU: test_fp32_cases_gpu.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "adapt-image-models_amd", "csrc", "fp32.hip")).read()
    msgs = re.findall(r'AIM_CHECK_ARG\([^"]*"([^"]*)"', src) + re.findall(r'aim_set_error\("([^"]*)"', src)
    assert len(msgs) >= 30
    by_fn = {}
    for name, text in fc.REFUSAL_TEXT.items():
        by_fn.setdefault(name.split("/")[0], []).append(text)
    for m in msgs:
        fn = m.split(":")[0]
        assert any(t in m for t in by_fn.get(fn, ())), f"no refusal case for: {m}"
    for fn, texts in by_fn.items():
        for t in texts:
            assert any(m.startswith(fn + ":") and t in m for m in msgs), (fn, t)
