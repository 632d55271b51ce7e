"""tests/swin3d_attn_cases.py on the CPU: its bounds accept an emulation of the kernels' arithmetic and reject the defects they
are meant to catch, its geometry is the reference's, and its case list covers what it says."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin3d_attn_cases as W  # noqa: E402

BY_NAME = {c.name: c for c in W.cases()}
# the shapes small enough for the CPU: S 18 (two clips, boxes of one token), S 98 (two tiles), the clipped t window, the
# t-only shift under a window that spans the grid, the walk shape and the hot cross-region scores
SMALL = [c for c in W.cases() if c.S <= 147 and c.family in ("unit", "bias_big", "cross_hot")]
# mutant -> the case that must reject it
REJECTS = {"bias_T": "c2D4G6w233s111h1/unit", "no_bias": "c2D4G6w233s111h1/unit", "swap_hw_f": "c1D4G14w277s133h3/unit",
           "clipped_const": "c2D4G6w433s011h2W833/unit", "cross_box": "c2D4G6w233s111h1/unit", "t_wrap": "c2D6G7w377s100h2/unit",
           "shift_sign": "c2D4G6w233s111h1/unit", "penalty_mask": "c2D4G6w233s111h1/cross_hot",
           "dtable_restart": "c2D4G6w233s111h1/unit", "dtable_scaled": "c2D4G6w233s111h1/unit"}


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            case = BY_NAME[name]
            inp = W.make_inputs(case)
            cache[name] = (case, inp, W.expected(case, inp))
        return cache[name]
    return get


def _ratios(case, inp, exp, mut=None):
    got = W.emulate(case, inp, mut)
    got["lse"] = got["lse"].double()      # emulate's lse is the natural logarithm already
    return W.compare(case, inp, got, exp)


@pytest.mark.parametrize("name", [c.name for c in SMALL])
def test_bounds_accept_the_emulated_kernels(refs, name):
    res = _ratios(*refs(name))
    assert set(res) == {"out", "lse", "dq", "dk", "dv", "dtable"}
    assert all(r <= 1.0 for r in res.values()), res


@pytest.mark.parametrize("mut", W.MUTANTS)
def test_bounds_reject_every_mutant(refs, mut):
    assert set(REJECTS) == set(W.MUTANTS)
    res = _ratios(*refs(REJECTS[mut]), mut)
    worst = max(res.values())
    assert not worst <= 1.0, (mut, res)
    if mut.startswith("dtable_"):      # a defect of the table gradient alone leaves everything else inside
        assert all(r <= 1.0 for k, r in res.items() if k != "dtable"), res


def test_every_shape_of_the_list_is_there_shifted_and_unshifted():
    names = set(BY_NAME)
    for d in W.SHAPES:
        for fam in W.FAMILIES:
            assert f"{W._tag(d)}/{fam}" in names
        assert f"{W._tag(d[:4] + ((0, 0, 0),) + d[5:])}/unit" in names
    assert len({c.seed for c in W.cases()}) == len(names)
    sizes = {c.S for c in W.cases()}
    assert {18, 98, 147, 196, 256, 36, 392, 784} <= sizes
    for c in W.cases():
        assert c.S <= W.MAX_S and c.ntable <= W.TAB_CAP


def test_the_walk_case_has_three_or_more_boxes_per_workgroup_and_a_short_last_walk():
    case = BY_NAME[f"walk/{W._tag(W.WALK_SHAPE)}/unit"]
    nw, per = W.walks(case.nboxes, case.H)
    assert case.nboxes == 243 and per >= 3 and nw >= 2
    assert 0 < case.nboxes - (nw - 1) * per < per
    for c in W.cases():
        if not c.name.startswith("walk/"):
            assert W.walks(c.nboxes, c.H)[1] <= 2, c.name


@pytest.mark.parametrize("dims", W.SHAPES + (W.WALK_SHAPE,))
def test_the_arithmetic_index_is_the_reference_buffer(dims):
    case = W.Case("i", dims)
    S = case.S
    ref = W.relative_position_index(case.full)
    assert ref.shape == (W.math.prod(case.full),) * 2 and int(ref.max()) == case.ntable - 1 and int(ref.min()) == 0
    assert torch.equal(W.arithmetic_index(case.window, case.full), ref[:S, :S])


@pytest.mark.parametrize("dims", W.SHAPES)
def test_the_mask_pieces_are_the_boxes_of_the_cut_partition(dims):
    """in original coordinates the allowed pairs of the reference's rolled, masked windows are the pairs of one box of the
    partition that cuts each axis at 0, s, s + w, ...; the number of boxes is the kernels' `nboxes`"""
    case = W.Case("g", dims)
    idx, allow = W.rolled_geometry(case)
    box = torch.zeros(case.rows, dtype=torch.long)
    r = torch.arange(case.rows)
    coords = ((r // (case.G * case.G)) % case.D, (r // case.G) % case.G, r % case.G)
    for c, ext, w, s in zip(coords, (case.D, case.G, case.G), case.window, case.shift):
        cut = (c - s + w) // w if s else c // w
        box = box * (ext // w + 1) + cut
    box = box + (r // (case.D * case.G * case.G)) * 10 ** 6
    b = box[idx]
    assert torch.equal(allow, b[:, :, None] == b[:, None, :])
    assert box.unique().numel() == case.nboxes
    if dims is W.SHAPES[0]:
        assert W.lone_rows(case).numel() == 2 * 2      # boxes (1, 1, 1): t in {0, 3}, y = x = 0, in each clip
