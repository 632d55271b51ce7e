"""The fused low-rank adapter kernels (aim_lowrank_fwd / aim_lowrank_bwd) against float64, every case of lowrank_cases.py:
M in {1, 127, 129, 1029} x (D, r) in {(128, 32), (256, 8), (768, 192), (1024, 256)} x G in {1, 3} x alpha in {1, 2}, with a
row-strided X, slab-strided Y_g and dY_g, the fp32 form with its residual, H stored and not, and every call run twice."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowrank_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", lc.cases(), ids=lambda c: c.name)
def test_lowrank_against_float64(case):
    from aim_amd import ops
    rec = lc.run_case(ops, case, torch.device("cuda"))
    print(case.name, {k: round(v, 3) for k, v in rec["checks"].items()})
    want = {f"{k}{i}" for k in ("H", "dH", "Y") for i in range(case.G)} | {"dX"} | ({"Y32"} if case.G == 1 else set())
    assert set(rec["checks"]) == want
    assert all(rec["finite"].values()), rec["finite"]
    assert all(rec["pad"].values()), rec["pad"]           # nothing written beside the [M, D] / [M, r] views
    assert all(rec["same"].values()), rec["same"]         # reruns, and the H = NULL form, give equal bits
    assert max(rec["checks"].values()) <= 1.0, rec["checks"]


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
