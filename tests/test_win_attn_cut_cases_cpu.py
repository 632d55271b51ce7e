"""CPU proof of tests/win_attn_cut_cases.py: its address rule is a partition in which no frame index wraps, its bounds
(win_attn_cases.py's, with S and nT of each box) accept a float64 emulation of the kernels' arithmetic on the boxes in both
backward forms, and they reject each addressing defect of MUTANTS on the cases where that defect changes anything."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cases as W  # noqa: E402
import win_attn_cut_cases as WC  # noqa: E402
import win_attn_shift_cases as WS  # noqa: E402

CASES = WC.cases()
_INPUTS, _GROUPS = {}, {}


def _inp(case):
    if case.name not in _INPUTS:
        _INPUTS[case.name] = WC.make_inputs(case)
        _GROUPS[case.name] = WC.expected_groups(case, _INPUTS[case.name])
    return _INPUTS[case.name]


def _worst(case, mut=None):
    inp = _inp(case)
    return WC.compare(case, inp, WC.emulate(case, inp, mut, own=True), "b", _GROUPS[case.name])


def _by(shape, family):
    (case,) = [c for c in CASES if (c.B, c.T, c.G, c.H, c.window, c.shift) == WC.SHAPES[shape] and c.family == family]
    return case


def test_case_list_covers_the_issue():
    assert {(c.B, c.T, c.G, c.H, c.window, c.shift) for c in CASES} == set(WC.SHAPES)
    assert {c.family for c in CASES} == set(W.FAMILIES) and len(CASES) == 4 * 4
    assert all(c.B == 2 and c.H == 2 for c in CASES)
    assert WC.SHAPES[:3] == ((2, 4, 4, 2, (2, 2, 2), (1, 1, 1)), (2, 8, 6, 2, (4, 3, 3), (2, 1, 1)), (2, 16, 6, 2, (8, 6, 6), (4, 0, 0)))
    sizes = [sorted({idx.shape[1] for idx in WC.box_rows(B, T, G, w, s)}) for B, T, G, H, w, s in WC.SHAPES]
    assert sizes[0] == [1, 2, 4, 8] and sizes[1][0] == 2 and sizes[1][-1] == 36 and sizes[2] == [144, 288]
    assert 288 % 64 == 32 and 144 % 64 == 16 and 288 > 8 * 16              # tails of 32 and 16; more than one chunk of own tokens
    per_clip = [sum(idx.shape[0] for idx in WC.box_rows(1, T, G, w, s)) for _, T, G, _, w, s in WC.SHAPES]
    assert per_clip == [(T // w[0] + (s[0] > 0)) * (G // w[1] + (s[1] > 0)) * (G // w[2] + (s[2] > 0)) for _, T, G, _, w, s in WC.SHAPES]
    assert per_clip == [27, 27, 3, 45]


def test_the_shift_module_keeps_its_own_boxes():
    """the rule is an argument: calls into the cut table leave what the shift table returns as it was"""
    case = min(WS.cases(), key=lambda c: c.B * c.T * c.N)          # the smallest shifted case
    geom = (case.B, case.T, case.G, case.window, case.shift)
    inp = WS.make_inputs(case)
    rows, got = WS.box_rows(*geom), WS.emulate(case, inp, None, own=True)
    cut = _by(0, "unit")
    assert len(WC.box_rows(*geom)) != len(rows)                     # the cut rule groups this geometry otherwise
    WC.boxes(*geom)
    WC.compare(cut, _inp(cut), WC.emulate(cut, _inp(cut), "t_wraps", own=True), "b", _GROUPS[cut.name])
    rows2, got2 = WS.box_rows(*geom), WS.emulate(case, inp, None, own=True)
    assert len(rows) == len(rows2) and all(torch.equal(a, b) for a, b in zip(rows, rows2))
    assert set(got) == set(got2) and all(torch.equal(got[k], got2[k]) for k in got)
    assert sorted(idx.shape[1] for idx in WS.box_rows(1, 4, 4, (2, 2, 2), (1, 1, 1))) == [2, 4, 8]


@pytest.mark.parametrize("mut", (None,) + WC.MUTANTS)
def test_address_rule_is_a_partition(mut):
    """every patch row lies in exactly one box, no class row in any; the defects are partitions too (they regroup)"""
    for B, T, G, H, w, s in WC.SHAPES:
        N = G * G + 1
        flat = torch.cat([idx.reshape(-1) for idx in WC.box_rows(B, T, G, w, s, mut)])
        assert flat.numel() == B * T * G * G and flat.unique().numel() == flat.numel(), (mut, w, s)
        assert (flat % N != 0).all() and flat.min() >= 0 and flat.max() < B * T * N


def test_boxes_are_contiguous_in_t_and_stay_inside_their_clip():
    """no frame index is taken modulo T: the frames of a box are consecutive and ascending; each axis is cut at 0, s, s + w, ..."""
    for B, T, G, H, w, s in WC.SHAPES:
        N = G * G + 1
        wt = min(w[0], T)
        starts = set()
        for (b, jt, _, _), rows in WC.boxes(B, T, G, w, s):
            assert ((rows // (T * N)) == b).all()
            frames = torch.unique_consecutive((rows // N) % T)
            assert torch.equal(frames, torch.arange(int(frames[0]), int(frames[0]) + frames.numel()))
            starts.add(int(frames[0]))
        assert starts == ({0} | set(range(s[0], T, wt)) if s[0] else set(range(0, T, wt)))


def test_zero_t_shift_is_the_shift_modules_rule_and_zero_shift_the_window_rule():
    for B, T, G, H, w, s in WC.SHAPES:
        s0 = (0,) + tuple(s[1:])
        a, b = WC.box_rows(B, T, G, w, s0), WS.box_rows(B, T, G, w, s0)
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
        (idx,) = WC.box_rows(B, T, G, w, (0, 0, 0))
        assert torch.equal(idx, W.window_rows(B, T, G, w))


def test_the_cut_rule_is_the_shift_modules_t_cut_mutant():
    """what win_attn_shift_cases lists as the defect `t_cut_into_strips` of the wrapping kernels is this module's rule"""
    for B, T, G, H, w, s in WC.SHAPES:
        a, b = WC.box_rows(B, T, G, w, s), WS.box_rows(B, T, G, w, s, "t_cut_into_strips")
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_late_max_sits_in_the_last_tile_of_every_box():
    for case in CASES:
        if case.family != "late_max":
            continue
        _inp(case)
        for idx, fw, _, _ in _GROUPS[case.name]:
            if idx.shape[1] > 1:
                assert (fw["_z"].argmax(dim=-1) == idx.shape[1] - 1).all(), case.name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bounds_accept_the_emulation(case):
    inp = _inp(case)
    for own, form in ((False, "a"), (True, "b")):
        got = WC.emulate(case, inp, None, own=own)
        res = WC.compare(case, inp, got, form, _GROUPS[case.name])
        assert set(res) == {"out", "lse", "dq", "dk", "dv"}
        for name, r in res.items():
            assert r <= 1.0, (case.name, form, name, r)
        assert (W.class_rows(got["out"], case.B * case.T, case.N) == 0).all()


# defect -> the cases on which it must be caught: (index into SHAPES, family)
CATCH = {
    "shift_ignored": [(0, "unit"), (1, "unit"), (2, "unit"), (3, "peaked")],
    "t_wraps": [(0, "unit"), (1, "unit"), (2, "unit"), (2, "neg100"), (3, "unit")],
    "t_not_cut": [(0, "unit"), (1, "peaked"), (2, "unit"), (3, "unit")],
    "cut_at_s_plus_1": [(0, "unit"), (1, "unit"), (2, "unit"), (3, "unit")],
    "cut_at_s_minus_1": [(0, "unit"), (1, "unit"), (2, "unit"), (3, "unit")],
    "hw_shifts_swapped": [(3, "unit"), (3, "peaked")],                # needs sh != sw
}


@pytest.mark.parametrize("mut", WC.MUTANTS)
def test_bounds_reject_the_defect(mut):
    assert mut in CATCH
    for shape, fam in CATCH[mut]:
        case = _by(shape, fam)
        res = _worst(case, mut)
        assert max(res.values()) > 1.0, (mut, case.name, res)
    assert _worst(_by(*CATCH[mut][0]), mut)["out"] > 1.0           # every one of them changes the forward output itself
