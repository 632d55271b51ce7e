"""CPU self-check of the float64 restatement in lowrank_cases.py: the comparison accepts the exact reference rounded once to
each output's dtype, and rejects each mutant -- the same result with one plausible kernel bug (alpha 1 for 2 or 2 for 1, a
dropped b1, a dropped b2, the adapters permuted among the G outputs, a second product that read the unrounded H, a dX without
its skip term, a dX whose skip term took one of the three dY), also rounded.  So the bounds the GPU test holds the kernels to
are tight enough to see those bugs.  The refusals of both entry points are argument checks on the host: they are exercised
here too, where a call that was NOT refused would fail at its launch with another return code."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowrank_cases as lc  # noqa: E402

SELF_CHECK = [c for c in lc.cases() if c.M in (127, 129) and (c.D, c.r) in ((128, 32), (256, 8), (768, 192))]


def test_case_table_covers_the_issue():
    cs = lc.cases()
    assert len(cs) == len({c.name for c in cs}) == 64
    assert {c.M for c in cs} == {1, 127, 129, 1029}
    assert {(c.D, c.r) for c in cs} == {(128, 32), (256, 8), (768, 192), (1024, 256)}
    assert {c.G for c in cs} == {1, 3} and {c.alpha for c in cs} == {1.0, 2.0}


@pytest.mark.parametrize("case", SELF_CHECK, ids=lambda c: c.name)
def test_reference_accepts_rounded_and_rejects_mutants(case):
    inp = lc.make_inputs(case)
    good = lc.compare(case, inp, lc.simulate(case, inp))
    want = {f"{k}{i}" for k in ("H", "dH", "Y") for i in range(case.G)} | {"dX"} | ({"Y32"} if case.G == 1 else set())
    assert set(good) == want and max(good.values()) <= 1.0, good
    muts = lc.mutants(case)
    assert set(muts) >= {"alpha_other", "no_b1", "no_b2", "h_unrounded", "dx_no_skip"}
    assert case.G == 1 or {"permuted", "dx_one_dy"} <= set(muts)
    for mut in muts:
        bad = lc.compare(case, inp, lc.simulate(case, inp, mut))
        assert max(bad.values()) > 1.0, (mut, bad)


def test_refusals_are_argument_checks():
    import aim_amd
    lib = aim_amd.load_library()
    res = lc.refused(lib)
    assert len(res) >= 27
    for what, rc, msg in res:
        assert rc == 1 and msg and b"aim_lowrank_" in msg, (what, rc, msg)
