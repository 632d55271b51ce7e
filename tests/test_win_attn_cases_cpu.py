"""CPU proof of tests/win_attn_cases.py: its bounds accept a float64 emulation of the window attention kernels' arithmetic
(rounding points inserted) on every case, in both backward forms, and reject each defect of MUTANTS on the cases where that
defect changes anything."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cases as W  # noqa: E402

CASES = W.cases()
_INPUTS = {}


def _inp(case):
    if case.name not in _INPUTS:
        _INPUTS[case.name] = W.make_inputs(case)
    return _INPUTS[case.name]


def _worst(case, mut=None):
    inp = _inp(case)
    got = W.emulate(case, inp, mut, own=True)
    return W.compare(case, inp, got, "b")


def test_case_list_covers_the_issue():
    shapes = {(c.B, c.T, c.G, c.H, c.window) for c in CASES}
    assert shapes == set(W.SHAPES)
    assert {c.family for c in CASES} == set(W.FAMILIES)
    S = {s[4][0] * s[4][1] * s[4][2] for s in W.SHAPES}
    assert S == {784, 32, 8, 128, 18}
    assert 784 % 64 == 16 and 784 % 128 == 16          # the tail past 12 x 64 and 6 x 128


def test_address_rule_is_a_partition():
    """every patch row lies in exactly one window, no class row in any"""
    for B, T, G, H, w in W.SHAPES:
        N = G * G + 1
        idx = W.window_rows(B, T, G, w)
        flat = idx.reshape(-1)
        assert flat.numel() == B * T * G * G and flat.unique().numel() == flat.numel()
        assert (flat % N != 0).all() and flat.max() < B * T * N


def test_late_max_sits_in_the_last_tile():
    for case in CASES:
        if case.family != "late_max":
            continue
        fw, _, _ = W.expected(case, _inp(case))
        S = fw["_z"].shape[-1]
        assert (fw["_z"].argmax(dim=-1) == S - 1).all(), case.name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bounds_accept_the_emulation(case):
    inp = _inp(case)
    for own, form in ((False, "a"), (True, "b")):
        got = W.emulate(case, inp, None, own=own)
        res = W.compare(case, inp, got, form)
        assert set(res) == {"out", "lse", "dq", "dk", "dv"}
        for name, r in res.items():
            assert r <= 1.0, (case.name, form, name, r)
        # the emulation leaves the class rows alone, as the kernels must
        assert (W.class_rows(got["out"], case.B * case.T, case.N) == 0).all()


def _by(shape_S, family):
    for c in CASES:
        w = W.clip_window(c.window, c.T, c.G)
        if w[0] * w[1] * w[2] == shape_S and c.family == family:
            return c
    raise KeyError((shape_S, family))


# defect -> the cases on which it must be caught: (tokens per window, family)
CATCH = {
    "swap_hw": [(18, "unit"), (18, "peaked")],                                     # needs wh != ww
    "wt1": [(784, "unit"), (32, "unit"), (8, "unit"), (18, "unit"), (128, "peaked")],
    "tail_unmasked": [(784, "unit"), (784, "neg100"), (8, "unit"), (18, "neg100"), (32, "unit")],
    "no_sum_rescale": [(784, "late_max"), (128, "late_max"), (784, "peaked")],     # needs more than one tile
    "lse_last_tile": [(784, "unit"), (128, "unit"), (784, "neg100"), (128, "late_max")],
}


@pytest.mark.parametrize("mut", W.MUTANTS)
def test_bounds_reject_the_defect(mut):
    assert mut in CATCH
    for S, fam in CATCH[mut]:
        case = _by(S, fam)
        res = _worst(case, mut)
        assert max(res.values()) > 1.0, (mut, case.name, res)
    if mut in ("swap_hw", "wt1", "tail_unmasked"):       # these change the forward output itself
        case = _by(*CATCH[mut][0])
        assert _worst(case, mut)["out"] > 1.0
    if mut == "lse_last_tile":
        assert _worst(_by(784, "unit"), mut)["lse"] > 1.0


def test_rescale_term_vanishes_for_one_tile():
    """S <= 64: the bounds are the spatial kernels' (attn_cases.forward_ref) with N -> S"""
    import attn_cases as A
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn((2, 18, 64), generator=g).to(torch.bfloat16).double() for _ in range(3))
    a, w = A.forward_ref(q, k, v), W.forward_ref(q, k, v)
    assert torch.equal(a["out"][1], w["out"][1]) and torch.equal(a["lse"][1], w["lse"][1])


def test_cap_on_window_tokens_is_the_header_value():
    """ops.WIN_ATTN_MAX_S (the constructor's check) and win_attn_cases.MAX_S restate AIM_WIN_ATTN_MAX_S of the C header"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "aim_kernels.h")).read()
    (cap,) = re.findall(r"^#define\s+AIM_WIN_ATTN_MAX_S\s+(\d+)\s*$", text, flags=re.M)
    from aim_amd import ops
    assert int(cap) == ops.WIN_ATTN_MAX_S == W.MAX_S and int(cap) >= 1024
    # the refused shape of the GPU run is over it, the largest recipe window under it
    assert 17 * 16 * 16 > int(cap) >= 16 * 7 * 7
