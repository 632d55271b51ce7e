"""CPU proof of tests/win_attn_shift_cases.py: its address rule is a partition, its bounds (win_attn_cases.py's, with S and
nT of each box) accept a float64 emulation of the kernels' arithmetic on the boxes in both backward forms, and they reject
each addressing defect of MUTANTS on the cases where that defect changes anything."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cases as W  # noqa: E402
import win_attn_shift_cases as WS  # noqa: E402

CASES = WS.cases()
_INPUTS, _GROUPS = {}, {}


def _inp(case):
    if case.name not in _INPUTS:
        _INPUTS[case.name] = WS.make_inputs(case)
        _GROUPS[case.name] = WS.expected_groups(case, _INPUTS[case.name])
    return _INPUTS[case.name]


def _worst(case, mut=None):
    inp = _inp(case)
    return WS.compare(case, inp, WS.emulate(case, inp, mut, own=True), "b", _GROUPS[case.name])


def _by(shape, family):
    (case,) = [c for c in CASES if (c.B, c.T, c.G, c.H, c.window, c.shift) == WS.SHAPES[shape] and c.family == family]
    return case


def test_case_list_covers_the_issue():
    assert {(c.B, c.T, c.G, c.H, c.window, c.shift) for c in CASES} == set(WS.SHAPES)
    assert {c.family for c in CASES} == set(W.FAMILIES) and len(CASES) == 6 * 4
    sizes = [sorted({idx.shape[1] for idx in WS.box_rows(B, T, G, w, s)}) for B, T, G, H, w, s in WS.SHAPES]
    assert sizes[0] == [144, 192, 256, 336, 448, 784]           # tails 16 (144, 336, 784) and 0 (192, 256, 448) mod 64
    assert sizes[1] == [32, 64, 128] and sizes[2] == [2, 4, 8] and sizes[3] == [24, 48, 96]
    assert sizes[4][0] == 4 and sizes[4][-1] == 24
    per_clip = [sum(idx.shape[0] for idx in WS.box_rows(1, T, G, w, s)) for _, T, G, _, w, s in WS.SHAPES]
    assert per_clip == [18, 64, 18, 18, 24, 6]


@pytest.mark.parametrize("mut", (None,) + WS.MUTANTS)
def test_address_rule_is_a_partition(mut):
    """every patch row lies in exactly one box, no class row in any; the defects are partitions too (they regroup)"""
    for B, T, G, H, w, s in WS.SHAPES:
        N = G * G + 1
        flat = torch.cat([idx.reshape(-1) for idx in WS.box_rows(B, T, G, w, s, mut)])
        assert flat.numel() == B * T * G * G and flat.unique().numel() == flat.numel(), (mut, w, s)
        assert (flat % N != 0).all() and flat.min() >= 0 and flat.max() < B * T * N


def test_boxes_stay_inside_their_clip_and_zero_shift_is_the_window_rule():
    for B, T, G, H, w, s in WS.SHAPES:
        N = G * G + 1
        for (b, _, _, _), rows in WS.boxes(B, T, G, w, s):
            assert ((rows // (T * N)) == b).all()
        (idx,) = WS.box_rows(B, T, G, w, (0, 0, 0))
        assert torch.equal(idx, W.window_rows(B, T, G, w))


def test_t_only_shift_is_the_window_rule_on_rolled_frames():
    for B, T, G, H, w, s in WS.SHAPES:
        if not s[0]:
            continue
        N = G * G + 1
        (idx,) = WS.box_rows(B, T, G, w, (s[0], 0, 0))
        base = W.window_rows(B, T, G, w)
        b, f, n = base // (T * N), (base // N) % T, base % N
        assert torch.equal(idx, (b * T + (f + s[0]) % T) * N + n)


def test_late_max_sits_in_the_last_tile_of_every_box():
    for case in CASES:
        if case.family != "late_max":
            continue
        _inp(case)
        for idx, fw, _, _ in _GROUPS[case.name]:
            assert (fw["_z"].argmax(dim=-1) == idx.shape[1] - 1).all(), case.name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bounds_accept_the_emulation(case):
    inp = _inp(case)
    for own, form in ((False, "a"), (True, "b")):
        got = WS.emulate(case, inp, None, own=own)
        res = WS.compare(case, inp, got, form, _GROUPS[case.name])
        assert set(res) == {"out", "lse", "dq", "dk", "dv"}
        for name, r in res.items():
            assert r <= 1.0, (case.name, form, name, r)
        assert (W.class_rows(got["out"], case.B * case.T, case.N) == 0).all()


# defect -> the cases on which it must be caught: (index into SHAPES, family)
CATCH = {
    "shift_ignored": [(0, "unit"), (1, "unit"), (2, "unit"), (3, "peaked"), (4, "unit"), (5, "unit")],
    "wrong_sign": [(0, "unit"), (4, "unit"), (4, "peaked")],          # needs an odd extent: w - s != s
    "strips_not_cut": [(0, "unit"), (1, "unit"), (2, "unit"), (3, "unit"), (4, "neg100"), (5, "unit")],
    "t_cut_into_strips": [(0, "unit"), (2, "unit"), (3, "unit"), (4, "peaked"), (5, "unit")],     # needs st > 0
    "wrap_mod_BT": [(3, "unit"), (3, "peaked")],                      # needs two clips
}


@pytest.mark.parametrize("mut", WS.MUTANTS)
def test_bounds_reject_the_defect(mut):
    assert mut in CATCH
    for shape, fam in CATCH[mut]:
        case = _by(shape, fam)
        res = _worst(case, mut)
        assert max(res.values()) > 1.0, (mut, case.name, res)
    assert _worst(_by(*CATCH[mut][0]), mut)["out"] > 1.0           # every one of them changes the forward output itself
