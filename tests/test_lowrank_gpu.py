"""The fused low-rank adapter kernels (aim_lowrank_fwd / aim_lowrank_bwd) against float64, every case of lowrank_cases.py:
M in {1, 127, 129, 1029} x (D, r) in {(128, 32), (256, 8), (768, 192), (1024, 256)} x G in {1, 3} x alpha in {1, 2}, with a
row-strided X, slab-strided Y_g and dY_g, the fp32 form with its residual, H stored and not, and every call run twice.

Then lowrank_cases.sweep_groups(), held to the same assertions: every r of 8 .. 256 at G in {1, 3} and D in {64, 192} (rk =
1 .. 4 with and without a partial last chunk, nk = 1 and 3; the 32-row backward at r = 200 .. 256); every row count of
1 .. 130 on the forward, the 64-row and the 32-row backward; D = 8192; and the call forms with a NULL b1 and / or b2, y[0]
beside y32, and H asked of one adapter of three.  Each group prints its worst ratio per output."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowrank_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


def hold(case, rec):
    want = {f"{k}{i}" for k in ("H", "dH", "Y") for i in range(case.G)} | {"dX"} | ({"Y32"} if case.G == 1 else set())
    assert set(rec["checks"]) == want, case.name
    assert all(rec["finite"].values()), (case.name, rec["finite"])
    assert all(rec["pad"].values()), (case.name, rec["pad"])      # nothing written beside the [M, D] / [M, r] views
    assert all(rec["same"].values()), (case.name, rec["same"])    # reruns, the H = NULL form and c.form give equal bits
    assert max(rec["checks"].values()) <= 1.0, (case.name, rec["checks"])


@pytest.mark.parametrize("case", lc.cases(), ids=lambda c: c.name)
def test_lowrank_against_float64(case):
    from aim_amd import ops
    rec = lc.run_case(ops, case, torch.device("cuda"))
    print(case.name, {k: round(v, 3) for k, v in rec["checks"].items()})
    hold(case, rec)


SWEEP = lc.sweep_groups()


@pytest.mark.parametrize("group", list(SWEEP))
def test_lowrank_sweep_against_float64(group):
    """one group of lowrank_cases.sweep_groups() per test; the first case that misses an assertion fails the group"""
    from aim_amd import ops
    worst = {}
    try:
        for case in SWEEP[group]:
            rec = lc.run_case(ops, case, torch.device("cuda"))
            for k, v in rec["checks"].items():
                if v > worst.get(k, (-1.0, None))[0]:
                    worst[k] = (v, case.name)
            hold(case, rec)
    finally:
        print(f"lowrank sweep {group}: {len(SWEEP[group])} cases, worst ratio per output",
              {k: f"{v:.3f} ({n})" for k, (v, n) in sorted(worst.items())})


def test_refused_shapes_launch_nothing():
    """every argument block is full of fake addresses: a refusal that came late would be a fault, not a return code"""
    import aim_amd
    for what, rc, msg in lc.refused(aim_amd.load_library()):
        assert rc == 1 and msg and b"aim_lowrank_" in msg, (what, rc, msg)
    torch.cuda.synchronize()


def test_wrappers_refuse_cpu_tensors():
    from aim_amd import ops
    x = torch.zeros((8, 64), dtype=torch.bfloat16)
    w1, w2 = torch.zeros((8, 64), dtype=torch.bfloat16), torch.zeros((64, 8), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lowrank_fwd(x, [w1], [None], [w2], [None], y=[x.clone()])
