"""The CPU emulation of stock AIM's fp8 forward (tests/aim_fp8_emu.py): with fp8 off it IS the oracle's bf16 emulation, and
the bound the GPU test puts on the product (tests/test_aim_fp8_gpu.py: ``fp8_vs_emu8 < 0.75 * emu8_vs_emu16``) is one that a
mis-wired block misses -- every wiring mutant of the emulation lies farther from the emulation than that, at the GPU test's
own shapes and seeds."""
import os
import sys

import pytest
import torch

from oracle import vit_clip_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aim_fp8_emu as E  # noqa: E402


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


_CACHE = {}


def _case(arch):
    """(inputs, emu8, emu16) of a model case, computed once"""
    if arch not in _CACHE:
        st, imgs = E.case_inputs(arch)
        H = E.CASES[arch][4]
        with torch.no_grad():
            _CACHE[arch] = (st, imgs, E.emu_aim_backbone_f8(imgs, st, H), E.emu_aim_backbone_f8(imgs, st, H, f8=False))
    return _CACHE[arch]


@pytest.mark.parametrize("arch", list(E.CASES))
def test_emulation_without_fp8_is_the_oracle(arch):
    st, imgs, e8, e16 = _case(arch)
    with torch.no_grad():
        want = O.emu_aim_backbone(imgs, st, E.CASES[arch][4], rnd=O.BF16)
    assert torch.equal(e16, want)
    assert not torch.equal(e8, e16) and torch.isfinite(e8).all()


@pytest.mark.parametrize("mutant", E.MUTANTS)
@pytest.mark.parametrize("arch", list(E.CASES))
def test_wiring_mutant_misses_the_gpu_bound(arch, mutant):
    st, imgs, e8, e16 = _case(arch)
    with torch.no_grad():
        em = E.emu_aim_backbone_f8(imgs, st, E.CASES[arch][4], mutant=mutant)
    bound = 0.75 * _rel(e8, e16)
    d = _rel(em, e8)
    print("MUTANT", arch, mutant, f"rel(mutant, emu8) = {d:.3e}  bound = {bound:.3e}")
    assert d > bound, (d, bound)
