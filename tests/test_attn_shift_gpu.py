"""The head-shifted attention kernels (aim_attn_fwd_shift / aim_attn_bwd_shift) on every route of the backward.

No tolerance anywhere: the shift only moves the base address of an item's K / V (and dK / dV), so the results must be the bits
of the unshifted kernels on a qkv whose K and V were rolled by torch (tests/attn_shift_cases.py).  One child process per route
of attn_cases.ROUTES, one after another; the first child that fails ends the fixture and nothing more is started on the GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_shift_cases as sc  # noqa: E402


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    out = {}
    for route in sc.ROUTES:
        env = {k: v for k, v in os.environ.items() if k not in sc.ROUTE_VARS}
        env.update(sc.ROUTE_ENV[route])
        path = str(tmp_path_factory.mktemp("attn_shift") / f"{route}.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "attn_shift_cases.py"), route, path], env=env, timeout=300,
                           capture_output=True, text=True)
        if p.returncode != 0:        # stop at the first failing child: nothing more is started on the GPU
            pytest.fail(f"route {route}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[route] = json.load(f)
    return out


def test_every_case_ran_on_every_route_and_every_plan(routes):
    names = [c.name for c in sc.cases()]
    for route, res in routes.items():
        assert list(res["cases"]) == names, f"route {route} did not run every case"
        plans = {tuple(rec["plan"]) for rec in res["cases"].values()}
        want = {("two", False)} if route == "two" else {("two", False), ("pipe", False)} if route == "xt0" else \
            {("two", False), ("pipe", False), ("pipe", True)}
        assert plans == want, (route, plans)
    for c in sc.cases():
        assert len(c.shifts) == c.H and all(abs(s) < c.T for s in c.shifts)
    # the arbitrary tables hold both extremes
    assert all(c.T - 1 in c.shifts and -(c.T - 1) in c.shifts for c in sc.cases() if "arbitrary" in c.name)
    assert {(c.B, c.T, c.N, c.H) for c in sc.cases()} >= {(2, 8, 198, 12), (1, 32, 198, 12), (2, 16, 258, 16), (2, 8, 197, 12),
                                                         (3, 8, 5, 2)}


def test_shifted_kernels_equal_the_unshifted_ones_on_rolled_kv(routes):
    bad, n = [], 0
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            if "equal" not in rec:
                continue
            n += 1
            for k, ok in rec["equal"].items():
                if not ok:
                    bad.append(f"{route} {name} {k}: bits differ from the unshifted kernel on rolled K / V")
            if any(rec["shifts"]) and not rec["shift_matters"]:
                bad.append(f"{route} {name}: the shift changed nothing; the case cannot fail")
    assert n > 0
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_zero_table_is_the_unshifted_entry_point(routes):
    bad, n = [], 0
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            if "zero_is_unshifted" in rec:
                n += 1
                bad += [f"{route} {name} {k}" for k, ok in rec["zero_is_unshifted"].items() if not ok]
    assert n >= len(sc.SHAPES) * len(routes)
    assert not bad, "an all-zero table differs from aim_attn_fwd / aim_attn_bwd:\n" + "\n".join(bad[:60])


def test_clips_are_independent(routes):
    bad, n = [], 0
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            if "clips_kept" in rec:
                n += 1
                assert rec["poison_seen"], f"{route} {name}: the NaN clip produced finite output"
                bad += [f"{route} {name} {k}" for k, ok in rec["clips_kept"].items() if not ok]
    assert n > 0
    assert not bad, "NaN K / V in clip 1 changed clips 0 or 2:\n" + "\n".join(bad[:60])


def test_repeatable_finite_and_inside_the_buffers(routes):
    bad = []
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            bad += [f"{route} {name} {k}: a second run gave other bits" for k, ok in rec["repeat"].items() if not ok]
            # delta is written by the two-kernel form only; either way nothing outside an output changes
            bad += [f"{route} {name} {k}: write outside the output (NaN padding changed)" for k, ok in rec["pad"].items() if not ok]
            if "clips_kept" not in rec:
                bad += [f"{route} {name} {k}: non-finite element" for k, ok in rec["finite"].items() if not ok]
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_refusals_are_loud(routes):
    for route, res in routes.items():
        assert len(res["refusals"]) == 4
        for name, msg in res["refusals"].items():
            assert msg and "outside (-T, T)" in msg, (route, name, msg)
