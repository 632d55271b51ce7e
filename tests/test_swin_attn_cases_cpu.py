"""tests/swin_attn_cases.py judged on the CPU: its address rule is the reference's roll / partition / mask, its bounds accept an
emulation of the kernels' arithmetic and reject the defects they are meant to catch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_attn_cases as W  # noqa: E402

CASES = {c.name: c for c in W.cases()}
# the case each defect is planted in: a shifted window case for the mask and the shift, the temporal case with the most
# frame tokens for the temporal index
PLANTED = {"bias_T": ("win/f2r14w7s3h1/unit", "t/B1T16L64h4/unit"), "no_mask": ("win/f2r14w7s3h1/unit", "win/f3r8w4s2h3/peaked"),
           "shift_sign": ("win/f2r14w7s3h1/unit", "win/f1r16w8s4h2/unit"), "swap_hw": ("win/f1r7w7s0h2/unit", "win/f1r56w7s3h4/unit"),
           "t_neg": ("t/B1T3L10h1/unit", "t/B1T32L8h1/peaked")}


def test_the_case_list_is_the_one_the_kernels_were_asked_to_pass():
    assert tuple(c.dims for c in W.cases() if c.kind == "win" and c.family == "unit") == W.WIN_SHAPES
    assert tuple(c.dims for c in W.cases() if c.kind == "t" and c.family == "unit") == W.T_SHAPES
    assert W.WIN_SHAPES == ((2, 14, 7, 3, 1), (1, 7, 7, 0, 2), (1, 16, 8, 4, 2), (3, 8, 4, 2, 3), (1, 56, 7, 3, 4))
    assert W.T_SHAPES == ((1, 1, 5, 1), (2, 2, 49, 2), (1, 3, 10, 1), (1, 16, 64, 4), (1, 32, 8, 1))
    assert {c.family for c in W.cases()} == {"unit", "peaked"} and len(CASES) == 20


@pytest.mark.parametrize("dims", W.WIN_SHAPES + ((1, 12, 4, 1, 1), (2, 8, 8, 0, 1)))
def test_address_and_mask_rule_is_the_reference_roll_partition_and_mask(dims):
    frames, res, w, s, H = dims
    idx, allow = W.geometry(W.Case("g", "win", dims))
    ridx, rallow = W.rolled_geometry(frames, res, w, s)
    assert torch.equal(idx, ridx) and torch.equal(allow, rallow)
    assert sorted(idx.reshape(-1).tolist()) == list(range(frames * res * res))          # every row has one writer
    if dims == (2, 14, 7, 3, 1):           # 1, 2, 2 and 4 regions in the four windows of a frame
        assert [len({tuple(r.tolist()) for r in a}) for a in allow[:4]] == [1, 2, 2, 4]


def test_peaked_logits_are_peaked():
    for name in ("win/f1r16w8s4h2", "t/B1T32L8h1"):
        tops = {}
        for fam in W.FAMILIES:
            c = CASES[f"{name}/{fam}"]
            inp = W.make_inputs(c)
            idx, _ = W.geometry(c)
            q, k, _ = W.gather(inp["qkv"], idx, c.H, 3)
            tops[fam] = float((q @ k.transpose(-1, -2) * W.SCALE).abs().amax())
        assert tops["peaked"] > 3 * tops["unit"] and tops["peaked"] > 15


@pytest.mark.parametrize("name", sorted(CASES))
def test_bounds_accept_the_emulated_kernels(name):
    c = CASES[name]
    inp = W.make_inputs(c)
    res = W.compare(c, inp, W.emulate(c, inp))
    assert set(res) == {"out", "lse", "dq", "dk", "dv", "dbias", "dtable"}
    assert all(r <= 1.0 for r in res.values()), res


def test_one_key_sequences_have_zero_score_gradients():
    c = CASES["t/B1T1L5h1/peaked"]
    inp = W.make_inputs(c)
    got = W.emulate(c, inp)
    C = c.H * W.HD
    assert not got["dqkv"][:, :2 * C].any() and not got["dbias"].any() and not got["dtable"].any()
    assert got["dqkv"][:, 2 * C:].any()


@pytest.mark.parametrize("mut", W.MUTANTS)
def test_bounds_reject_the_planted_defect(mut):
    assert set(PLANTED) == set(W.MUTANTS)
    for name in PLANTED[mut]:
        c = CASES[name]
        inp = W.make_inputs(c)
        res = W.compare(c, inp, W.emulate(c, inp, mut))
        assert max(res.values()) > 1.0, (mut, name, res)
        if mut in ("bias_T", "t_neg"):      # a defect of the bias alone shows in the bias gradient's fold too
            assert res["out"] > 1.0 and res["dtable"] > 1.0, (mut, name, res)
