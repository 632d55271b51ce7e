"""The Swin attention kernels (aim_swin_win_attn_*, aim_swin_tattn_*, aim_swin_bias_scatter) against float64 within the bounds
of tests/swin_attn_cases.py: the whole case list runs once, in one child process, and the tests read its record."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_attn_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("swin_attn") / "record.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "swin_attn_cases.py"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(path) as f:
        return json.load(f)


def test_every_case_ran(record):
    assert sorted(record["cases"]) == sorted(c.name for c in W.cases())


def test_forward_backward_and_bias_gradients_within_bounds(record):
    bad = []
    for name, rec in record["cases"].items():
        assert set(rec["checks"]) == {"out", "lse", "dq", "dk", "dv", "dbias", "dtable"}, name
        for k, r in rec["checks"].items():
            print(f"{name} {k}: {r:.3f}")
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3f}")
    assert not bad, "\n".join(bad)


def test_two_runs_are_bit_identical_bias_gradients_included(record):
    for name, rec in record["cases"].items():
        assert set(rec["repeat"]) >= {"out", "lse2", "dqkv", "dbias", "dtable"}, name
        assert all(rec["repeat"].values()), (name, rec["repeat"])


def test_nothing_is_written_past_the_results(record):
    for name, rec in record["cases"].items():
        assert all(rec["spare_intact"].values()), (name, rec["spare_intact"])
        assert rec["slots_past_S_intact"], name
        assert all(rec["finite"].values()), (name, rec["finite"])


def test_dqkv_does_not_depend_on_whether_the_bias_gradient_is_wanted(record):
    for name, rec in record["cases"].items():
        assert rec["dqkv_without_dbias_same_bits"], name


def test_unsupported_geometry_is_refused_before_any_launch(record):
    assert set(record["refusals"]) == {"window over 64 tokens", "window does not divide", "shift outside the window",
                                       "shift on a window that spans the grid", "more than 32 frame tokens"}
    for name, rec in record["refusals"].items():
        assert rec["fwd"] and "swin_" in rec["fwd"], (name, rec)
        assert rec["bwd"] and "swin_" in rec["bwd"], (name, rec)
        assert rec["nothing_written"], name
