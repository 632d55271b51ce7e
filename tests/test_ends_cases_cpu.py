"""CPU self-check of tests/ends_cases.py: the bounds that test_ends_cases_gpu.py holds the head, loss, lamda, patch-gather and
AdamW kernels to accept an fp32 emulation of each kernel's arithmetic in its summation order, and reject the same emulation
with one plausible kernel bug (a mutant).  Nothing is tuned in between: the bounds are the derivations in the module
docstring of ends_cases.py.  The worst emulation error / bound per entry point and output, and the smallest mutant error /
bound over the cases that must see the mutant, are printed.

Which cases must see a mutant is stated by MUST_SEE with the reason; on the other cases the mutant changes nothing.  One
listed mutant can be seen on no case at all -- aim_ce_topk with k2 not clamped to C, see EQUIVALENT -- and is held to the
unmutated bits instead.

Also: every shape, flag and family the catalogue is meant to cover has a case, the refusal table matches the AIM_CHECK_ARG
texts of the sources, and torch's own cross-entropy returns NaN on the CPU where the float64 references do."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ends_cases as ec  # noqa: E402

CASES = ec.cases()
KINDS = sorted(ec.KINDS)


@pytest.fixture(scope="module")
def inputs():
    return {c.name: ec.build_inputs(c) for c in CASES}


@pytest.mark.parametrize("kind", KINDS)
def test_bounds_accept_the_emulation(kind, inputs):
    worst, n = {}, 0
    for c in CASES:
        if c.kind != kind:
            continue
        n += 1
        inp = inputs[c.name]
        got = ec.emulate(c, inp)
        for k, r in ec.compare(c, inp, got).items():
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (c.name, k, r)
        assert all(ec.finite_where_expected(c, inp, got).values()), c.name
    print(f"{kind}: {n} cases, worst emulation error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert n > 0


def _some_valid(c):
    return c.p["labels"] == "valid" or (c.p["labels"] == "mix" and c.p["B"] > 1)


# (kind, mutant) -> the cases that must be outside the bound, with the reason for leaving the others out
MUST_SEE = {
    # equal frames have the same mean over T - 1 of them; one frame has none to leave out
    ("head_fwd", "mean_Tm1"): lambda c: c.p["T"] > 1 and c.family != "equal",
    ("head_fwd", "bias_next"): lambda c: c.p["bias"] and c.p["C"] > 1,
    ("head_fwd", "pooled_nodrop"): lambda c: c.p["drop"],
    ("head_fwd", "last_class_unwritten"): lambda c: c.p["C"] == 33,
    ("head_bwd", "assign"): lambda c: "dW" in c.p["outs"],
    ("head_bwd", "no_invT"): lambda c: "dfeat" in c.p["outs"] and c.p["T"] > 1,
    ("head_bwd", "drop_next"): lambda c: "dfeat" in c.p["outs"] and c.p["drop"],
    ("head_bwd", "db_Bm1"): lambda c: "db" in c.p["outs"],
    # the two means differ when some, not all, labels are ignored
    # (one class: every loss term is 0)
    ("ce_topk", "mean_over_B"): lambda c: c.p["labels"] == "mix" and c.p["B"] > 2 and c.p["C"] > 1,
    # rows with ties the two rules rank differently: the constructed tie rows need 16 classes and 8 samples to all occur
    ("ce_topk", "tie_lt"): lambda c: c.family == "ties" and c.p["C"] >= 16 and c.p["B"] >= 64 and c.p["labels"] != "ignored",
    # unshifted, e^100 overflows.  (At +-80 it does not: C e^80 <= 5.5e37, and the rounding of 80 log2e, about 1e-6 in the
    # result, is below the one rounding of lse = 80 that a correct kernel is allowed: no derived bound separates the two.)
    ("ce_topk", "no_max_shift"): lambda c: c.family == "pm100" and _some_valid(c),
    ("ce_topk", "onehot_next"): lambda c: c.p["dscore"] and c.p["C"] > 1 and _some_valid(c),
    # (one class: the loss and the dscore numerators are 0)
    ("ce_soft", "den_B_weighted"): lambda c: c.p["weighted"] and c.p["C"] > 1 and not ec.expects_nan(c, ec.build_inputs(c)),
    # sum w y = 1 on unweighted rows that are not zero: nothing to miss there
    ("ce_soft", "no_wy"): lambda c: c.p["dscore"] and (c.p["weighted"] or c.p["labels"] in ("somezero", "allzero"))
    and not ec.expects_nan(c, ec.build_inputs(c)),
    ("ce_soft", "w_next"): lambda c: c.p["weighted"] and c.p["C"] > 1 and c.p["labels"] != "uniform"
    and not ec.expects_nan(c, ec.build_inputs(c)),
    ("qk_cross", "no_scale"): lambda c: True,
    ("qk_cross", "kx_next"): lambda c: c.p["BT"] > 1,
    ("qk_border", "no_scale"): lambda c: True,
    ("qk_border", "kx_next"): lambda c: c.p["BT"] > 1,
    ("qk_border", "corner_both"): lambda c: True,
    ("qk_border", "corner_neither"): lambda c: True,
    ("qk_border", "slot_swapped"): lambda c: True,
    ("lambda", "diff_max"): lambda c: True,
    ("lambda", "neginf_nan"): lambda c: c.p["ntiles"] >= 3,
    # one tile of 257 is 0.4 % of ow: visible where lam (1 - lam) is not itself below the bound
    ("lambda", "ntiles_256"): lambda c: c.p["ntiles"] == 257 and c.family in ("unit", "near200"),
    ("lambda", "swap"): lambda c: True,
    ("lam_part", "diff_max"): lambda c: True,
    ("lam_part", "neginf_nan"): lambda c: True,
    ("lam_part", "swap"): lambda c: True,
    ("patchify", "swap_c_py"): lambda c: True,
    ("patchify", "h_stride"): lambda c: c.p["H"] != c.p["W"],
    ("patchify", "u8_signed"): lambda c: c.p["in_dtype"] == 1,
    # a bf16 input is its own rounding, a byte has 8 bits
    ("patchify", "truncate"): lambda c: c.p["in_dtype"] == 0 or c.p["norm"],
    ("patchify", "pad_unwritten"): lambda c: c.p["Kp"] > 3 * c.p["p"] ** 2,
    # sqrt(v + eps) and sqrt(v) + eps differ by less than an fp32 rounding unless v is far below eps^2 ... eps
    ("adamw", "eps_inside"): lambda c: c.family == "g0v0",
    # beta^(step - 1) and beta^step are both 0 in fp32 from a few hundred steps on; with v = inf the update is 0 whatever the
    # corrections are
    ("adamw", "bc_step_m1"): lambda c: c.p["step"] <= 2 and c.family != "g1e20",
    ("adamw", "l2_decay"): lambda c: c.p["wd"] != 0,
    # (g = 0 has no square; 1e-25 squared underflows and 1e20 squared overflows with or without the factor)
    ("adamw", "gs_not_squared"): lambda c: c.p["gs"] != 1.0 and c.family == "unit",
    ("adamw", "tail_skipped"): lambda c: c.p["n"] % 4 != 0,
}
# ahead <= C - 1 for a valid label, so (ahead < min(k2, C)) == (ahead < k2) whenever k2 >= C, and k2 < C is not clamped
EQUIVALENT = {("ce_topk", "k2_unclamped")}


def test_every_mutant_of_every_kind_is_listed():
    assert set(MUST_SEE) | EQUIVALENT == {(k, m) for k in ec.KINDS for m in ec.mutants(k)}
    assert not set(MUST_SEE) & EQUIVALENT


@pytest.mark.parametrize("kind,mut", sorted(MUST_SEE))
def test_bounds_reject_the_mutant(kind, mut, inputs):
    seen, least = 0, None
    for c in CASES:
        if c.kind != kind or not MUST_SEE[(kind, mut)](c):
            continue
        inp = inputs[c.name]
        r = max(ec.compare(c, inp, ec.emulate(c, inp, mut)).values())
        assert r > 1.0, (c.name, mut, r)
        seen += 1
        least = r if least is None else min(least, r)
    assert seen > 0, (kind, mut)
    print(f"{kind} {mut}: outside the bound on {seen} cases, by a factor of {least:.3g} at least")


@pytest.mark.parametrize("kind,mut", sorted(EQUIVALENT))
def test_the_unobservable_mutant_changes_no_bit(kind, mut, inputs):
    n = 0
    for c in CASES:
        if c.kind != kind:
            continue
        a, b = ec.emulate(c, inputs[c.name]), ec.emulate(c, inputs[c.name], mut)
        assert all(ec._bits_eq(a[k], b[k]) for k in a), c.name
        n += 1
    assert n > 0 and any(c.p["k2"] == "C+3" for c in CASES if c.kind == kind)


def _by(kind):
    return [c for c in CASES if c.kind == kind]


def _vals(kind, key):
    return {c.p[key] for c in _by(kind) if key in c.p}


def test_catalogue_covers_every_branch_and_seam():
    assert {c.kind for c in CASES} == set(ec.KINDS) and len({c.name for c in CASES}) == len(CASES)
    hf = _by("head_fwd")
    assert _vals("head_fwd", "B") == {1, 3} and _vals("head_fwd", "T") == {1, 2, 8}
    assert _vals("head_fwd", "D") == set(ec.HEAD_D) | {16384} and _vals("head_fwd", "C") == set(ec.HEAD_FWD_C)
    assert {(c.p["drop"], c.p["bias"]) for c in hf} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c.family for c in hf} == set(ec.HEAD_FAMILIES) and any(c.p["D"] == 16384 and c.p["C"] == 5 for c in hf)
    hb = _by("head_bwd")
    assert _vals("head_bwd", "D") == set(ec.HEAD_D) | {8} and _vals("head_bwd", "C") == set(ec.HEAD_BWD_C) | {16128}
    assert {c.p["outs"] for c in hb} == set(ec.HEAD_BWD_SUBSETS) and ("db",) in ec.HEAD_BWD_SUBSETS
    assert _vals("head_bwd", "drop") == {False, True} and _vals("head_bwd", "T") == {1, 2, 8}
    ct = _by("ce_topk")
    assert _vals("ce_topk", "B") == set(ec.CE_B) and _vals("ce_topk", "C") == set(ec.CE_C) and _vals("ce_topk", "k2") == set(ec.CE_K2)
    assert _vals("ce_topk", "dscore") == {False, True} and _vals("ce_topk", "labels") == set(ec.CE_LABELS)
    assert {c.family for c in ct} == set(ec.CE_FAMILIES)
    tie = ec.build_inputs(next(c for c in ct if c.family == "ties" and c.p["B"] >= 64 and c.p["C"] >= 16 and c.p["labels"] == "valid"))
    n_tied = [(int((tie["score"][b] == tie["score"][b, tie["label"][b]]).sum()) - 1, bool(tie["label"][b] < tie["score"].shape[1] // 2))
              for b in range(ec.TIE_VARIANTS)]
    assert set(n_tied[:6]) == {(n, side) for n in (4, 5, 6) for side in (True, False)}      # k - 1, k, k + 1 ties on either side of the label
    assert n_tied[6][0] == tie["score"].shape[1] - 1 and n_tied[7][0] == 2
    mix = ec.build_inputs(next(c for c in ct if c.p["labels"] == "mix" and c.p["B"] >= 64))["label"]
    assert {-100, -1, 2 ** 40} <= set(mix.tolist()) and any(0 <= v for v in mix.tolist())
    cs = _by("ce_soft")
    assert _vals("ce_soft", "B") == set(ec.CE_B) and _vals("ce_soft", "C") == set(ec.CE_C) and _vals("ce_soft", "labels") == set(ec.SOFT_LABELS)
    assert {(c.p["weighted"], c.p["dscore"]) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
    assert sum(ec.expects_nan(c, ec.build_inputs(c)) for c in cs) >= 2 and sum(ec.expects_nan(c, ec.build_inputs(c)) for c in ct) >= 2
    assert _vals("qk_cross", "BT") == {1, 3} and _vals("qk_cross", "N") == set(ec.QKC_N) and _vals("qk_cross", "D") == set(ec.QKC_D)
    assert {c.p["ldkx"] - c.p["D"] for c in _by("qk_cross")} == {0, 8}
    lm = _by("lambda")
    assert _vals("lambda", "form") == {"ss", "qk"} and _vals("lambda", "N") == set(ec.LAM_N) and _vals("lambda", "D") == set(ec.LAM_D)
    assert _vals("lambda", "ntiles") == set(ec.LAM_NT) and _vals("lambda", "oml") == {False, True}
    assert {(c.p["form"], c.family) for c in lm} == {(f, fam) for f in ("ss", "qk") for fam in ec.LAM_FAMILIES}
    assert {c.p["ldkx"] - c.p["D"] for c in lm if c.p["form"] == "qk"} == {0, 4}
    for c in lm:                    # the families are what they are named for
        inp = ec.build_inputs(c)
        ss = inp["ss"] if c.p["form"] == "ss" else ec._cross64(inp, c.p["D"], 0)[0]
        p0 = inp["partials"][..., 0]
        assert bool(torch.isneginf(p0).any()) == (c.p["ntiles"] >= 3)
        if c.family == "ow_dom":
            assert float((p0.max(1).values - ss.max(1).values).min()) > 104
        if c.family == "near200":
            assert float(ss.min()) > 150 and float(p0.max(1).values.min()) > 150
    qb = _by("qk_border")
    assert _vals("qk_border", "D") == {512, 1024} and _vals("qk_border", "N") == set(ec.BORDER_N)
    assert {(c.p["slot0"], c.p["nslots"]) for c in qb} == {(0, 2), (8, 10)} and _vals("qk_border", "BT") == {1, 3}
    assert _vals("lam_part", "BT") == set(ec.PART_BT) and {c.family for c in _by("lam_part")} == set(ec.LAM_FAMILIES)
    pt = _by("patchify")
    assert {(c.p["p"], c.p["Kp"]) for c in pt} >= {(8, 192), (8, 200), (16, 768), (16, 832), (14, 592), (14, 640), (12, 432), (4, 48)}
    assert {(c.p["in_dtype"], c.p["norm"]) for c in pt} == {(d, n) for d in (0, 1, 2) for n in (False, True)}
    assert any(c.p["H"] != c.p["W"] for c in pt) and {ec.patchify_fast_path(c.p) for c in pt} == {True, False}
    assert any(ec.patchify_fast_path(c.p) and c.p["Kp"] > 3 * c.p["p"] ** 2 for c in pt)          # a thread with k0 + 8 > K beside the fast ones
    assert any((3 * c.p["p"] ** 2) % 8 for c in pt)                                             # K inside a thread's 8 columns
    x = ec.build_inputs(next(c for c in pt if c.p["in_dtype"] == 1))["x"]
    assert int(x.min()) == 0 and int(x.max()) == 255
    ad = _by("adamw")
    assert _vals("adamw", "n") == set(ec.ADAM_N) and _vals("adamw", "step") == set(ec.ADAM_STEP) and _vals("adamw", "wd") == {0.0, 0.05}
    assert _vals("adamw", "gs") == {1.0, 0.125} and _vals("adamw", "betas") == set(ec.ADAM_BETAS) and {c.family for c in ad} == set(ec.ADAM_FAMILIES)


def test_refusal_table_matches_the_sources():
    csrc = os.path.join(os.path.dirname(HERE), "adapt-image-models_amd", "csrc")
    texts = {}
    for f in set(ec.REFUSAL_SOURCE.values()):
        src = open(os.path.join(csrc, f)).read()
        texts[f] = [lit for m in re.finditer(r"(?:AIM_CHECK_ARG|aim_set_error)\((.*?)\);", src, re.S) for lit in re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))]
    for name, text in ec.REFUSAL_TEXT.items():
        f = ec.REFUSAL_SOURCE[name.split("/")[0]]
        assert any(text in lit for lit in texts[f]), (name, text)
        assert "%" not in text


def test_torch_agrees_on_the_nan_cases():
    """torch on the CPU returns NaN where the float64 references do: F.cross_entropy with every label ignored, with and without
    class weights (aim_ce_soft takes such labels as all-zero one-hot rows), and the reference's weighted soft-label formula
    sum(-w y log_softmax) / sum(w y) on all-zero labels"""
    F = torch.nn.functional
    s = torch.randn(4, 5)
    assert torch.isnan(F.cross_entropy(s, torch.full((4,), -100)))
    w, y = torch.rand(5) + 0.5, torch.zeros(4, 5)
    assert torch.isnan(F.cross_entropy(s, torch.full((4,), -100), weight=w))      # the hard labels aim_ce_soft takes as zero one-hot rows
    assert torch.isnan(-(w * y * F.log_softmax(s, 1)).sum() / (w * y).sum())       # the reference's soft branch, in torch
    c = next(c for c in CASES if c.kind == "ce_topk" and c.p["labels"] == "ignored")
    assert torch.isnan(ec.ce_topk_expected(c, ec.build_inputs(c))["loss"][0]).all()
    c = next(c for c in CASES if c.kind == "ce_soft" and c.p["labels"] == "allzero" and c.p["weighted"])
    assert torch.isnan(ec.ce_soft_expected(c, ec.build_inputs(c))["out"][0]).all()


def test_references_agree_with_torch_float64():
    """the closed forms of ends_cases.py against torch's own float64 cross-entropy, autograd and AdamW"""
    F = torch.nn.functional
    c = next(c for c in CASES if c.kind == "ce_topk" and c.p["labels"] == "mix" and c.p["dscore"] and c.p["B"] == 64 and c.family == "unit")
    inp = ec.build_inputs(c)
    s = inp["score"].double().requires_grad_(True)
    lab = torch.where((inp["label"] >= 0) & (inp["label"] < c.p["C"]), inp["label"], torch.full_like(inp["label"], -100))
    loss = F.cross_entropy(s, lab)
    loss.backward()
    exp = ec.ce_topk_expected(c, inp)
    assert torch.allclose(exp["loss"][0], loss.detach().reshape(1), rtol=1e-12) and torch.allclose(exp["dscore"][0], s.grad, rtol=1e-10, atol=1e-14)
    c = next(c for c in CASES if c.kind == "ce_soft" and c.p["weighted"] and c.p["dscore"] and c.p["labels"] == "twohot")
    inp = ec.build_inputs(c)
    s = inp["score"].double().requires_grad_(True)
    w, y = inp["w"].double(), inp["label"].double()
    loss = -(w * y * F.log_softmax(s, 1)).sum() / (w * y).sum()
    loss.backward()
    exp = ec.ce_soft_expected(c, inp)
    assert torch.allclose(exp["out"][0], loss.detach().reshape(1), rtol=1e-12) and torch.allclose(exp["dscore"][0], s.grad, rtol=1e-10, atol=1e-14)
    c = next(c for c in CASES if c.kind == "adamw" and c.family == "unit" and c.p["wd"] and c.p["step"] == 2 and c.p["gs"] == 1.0)
    inp, h = ec.build_inputs(c), ec._hyp(c.p)
    p = inp["p"].double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    opt.state[p] = {"step": torch.tensor(float(c.p["step"] - 1)), "exp_avg": inp["m"].double().clone(), "exp_avg_sq": inp["v"].double().clone()}
    p.grad = inp["g"].double().clone()
    opt.step()
    exp = ec.adamw_expected(c, inp)
    want = p.detach() - inp["p"].double() * (1.0 - h["lr"] * h["wd"])
    assert torch.allclose(exp["update"][0], want, rtol=1e-9, atol=1e-15) and torch.allclose(exp["m"][0], opt.state[p]["exp_avg"], rtol=1e-12)
