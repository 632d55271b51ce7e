"""CPU self-check of the float64 restatement in lowrank_cases.py: the comparison accepts the exact reference rounded once to
each output's dtype, and rejects each mutant -- the same result with one plausible kernel bug (alpha 1 for 2 or 2 for 1, a
dropped b1, a dropped b2, the adapters permuted among the G outputs, a second product that read the unrounded H, a dX without
its skip term, a dX whose skip term took one of the three dY, a second product without the hidden units of r's last partial
64-chunk, a first product without the last 64 columns of D, a bias added where none was passed), also rounded.  So the bounds
the GPU test holds the kernels to are tight enough to see those bugs.  The refusals of both entry points are argument checks
on the host: they are exercised here too, where a call that was NOT refused would fail at its launch with another return
code."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowrank_cases as lc  # noqa: E402

SELF_CHECK = [c for c in lc.cases() if c.M in (127, 129) and (c.D, c.r) in ((128, 32), (256, 8), (768, 192))]

# of the sweep: one r per rk with a partial last chunk and r = 256, at both G and both D, and every call form
SWEEP_SELF_CHECK = [c for g, cs in lc.sweep_groups().items() for c in cs
                    if (g.startswith("r/") and c.r in (8, 72, 136, 200, 256)) or g == "forms"]


def test_case_table_covers_the_issue():
    cs = lc.cases()
    assert len(cs) == len({c.name for c in cs}) == 64
    assert {c.M for c in cs} == {1, 127, 129, 1029}
    assert {(c.D, c.r) for c in cs} == {(128, 32), (256, 8), (768, 192), (1024, 256)}
    assert {c.G for c in cs} == {1, 3} and {c.alpha for c in cs} == {1.0, 2.0}


def test_sweep_table_covers_the_issue():
    groups = lc.sweep_groups()
    cs = lc.sweep_cases()
    assert len(cs) == len({c.name for c in cs}) == 128 + 2 * 130 + 2 + 8
    assert not {c.name for c in cs} & {c.name for c in lc.cases()}
    assert sorted(groups) == sorted(["r/G1/D64", "r/G1/D192", "r/G3/D64", "r/G3/D192", "rows/D64/r8/G1", "rows/D64/r200/G3",
                                     "wide", "forms"])
    plain = lambda c: c.bias == "both" and c.form == "std"
    # every r, at both G and both D, M = 161, and both alphas at every (r, G)
    every_r = [c for g, v in groups.items() if g.startswith("r/") for c in v]
    assert {(c.r, c.G, c.D) for c in every_r} == {(r, G, D) for r in range(8, 257, 8) for G in (1, 3) for D in (64, 192)}
    assert len(every_r) == 128 and all(c.M == 161 and plain(c) for c in every_r)
    for r in range(8, 257, 8):
        for G in (1, 3):
            assert {c.alpha for c in every_r if (c.r, c.G) == (r, G)} == {1.0, 2.0}, (r, G)
    # every row count of 1 .. 130 at both row-sweep configurations
    for group, (D, r, G) in (("rows/D64/r8/G1", (64, 8, 1)), ("rows/D64/r200/G3", (64, 200, 3))):
        v = groups[group]
        assert sorted(c.M for c in v) == list(range(1, 131)), group
        assert all((c.D, c.r, c.G, c.alpha) == (D, r, G, 1.0) and plain(c) for c in v), group
    # the widest D
    assert {(c.M, c.D, c.r, c.G, c.alpha) for c in groups["wide"]} == {(129, 8192, 256, 3, 1.0), (129, 8192, 136, 1, 2.0)}
    assert all(plain(c) for c in groups["wide"])
    # the call forms
    forms = groups["forms"]
    assert all((c.M, c.D, c.r) == (161, 192, 72) for c in forms)
    assert sorted((c.G, c.bias, c.form) for c in forms) == sorted(
        [(G, b, "std") for G in (1, 3) for b in ("b1", "b2", "none")] + [(1, "both", "y_y32"), (3, "both", "h1")])
    assert {c.seed for c in cs}.isdisjoint({c.seed for c in lc.cases()}) and len({c.seed for c in cs}) == len(cs)


def test_sweep_self_check_subset():
    assert len(SWEEP_SELF_CHECK) == 5 * 2 * 2 + 8
    assert {(c.r, c.G, c.D) for c in SWEEP_SELF_CHECK if c.form == "std" and c.bias == "both"} == {
        (r, G, D) for r in (8, 72, 136, 200, 256) for G in (1, 3) for D in (64, 192)}
    assert {(c.r + 63) // 64 for c in SWEEP_SELF_CHECK if c.r % 64} == {1, 2, 3, 4}
    for mut in ("r_tail", "d_last_step", "bias_ignored_null"):
        assert any(mut in lc.mutants(c) for c in SWEEP_SELF_CHECK), mut


@pytest.mark.parametrize("case", SELF_CHECK + SWEEP_SELF_CHECK, ids=lambda c: c.name)
def test_reference_accepts_rounded_and_rejects_mutants(case):
    inp = lc.make_inputs(case)
    good = lc.compare(case, inp, lc.simulate(case, inp))
    want = {f"{k}{i}" for k in ("H", "dH", "Y") for i in range(case.G)} | {"dX"} | ({"Y32"} if case.G == 1 else set())
    assert set(good) == want and max(good.values()) <= 1.0, good
    muts = lc.mutants(case)
    assert set(muts) >= {"alpha_other", "h_unrounded", "dx_no_skip", "d_last_step"}
    assert ("no_b1" in muts) == (case.bias in ("both", "b1")) and ("no_b2" in muts) == (case.bias in ("both", "b2"))
    assert ("r_tail" in muts) == (case.r % 64 != 0) and ("bias_ignored_null" in muts) == (case.bias != "both")
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
