"""The 3-D window attention kernels (aim_win_attn_fwd / aim_win_attn_bwd) against float64 within the bounds of
tests/win_attn_cases.py: the whole case list runs once, in one child process, and the tests read its record."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("win_attn") / "record.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "win_attn_cases.py"), path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(path) as f:
        return json.load(f)


def test_every_case_ran(record):
    assert sorted(record["cases"]) == sorted(c.name for c in W.cases())


def test_forward_and_backward_within_bounds(record):
    bad = []
    for name, rec in record["cases"].items():
        assert set(rec["checks"]) == {"out", "lse", "delta", "dq@a", "dk@a", "dv@a", "dq@b", "dk@b", "dv@b"}, name
        for k, r in rec["checks"].items():
            print(f"{name} {k}: {r:.3f}")
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3f}")
    assert not bad, "\n".join(bad)


def test_two_runs_are_bit_identical(record):
    for name, rec in record["cases"].items():
        assert all(rec["repeat"].values()), (name, rec["repeat"])


def test_class_rows_and_spare_elements_keep_their_sentinel(record):
    for name, rec in record["cases"].items():
        assert all(rec["class_intact"].values()), (name, rec["class_intact"])
        assert all(rec["spare_intact"].values()), (name, rec["spare_intact"])
        assert all(rec["finite"].values()), (name, rec["finite"])


def test_a_nan_window_stays_in_its_window_and_nan_class_rows_are_not_read(record):
    assert len(record["poison"]) >= 4
    for name, rec in record["poison"].items():
        assert rec["independent"], name
        assert rec["finite_with_nan_class_rows"], name
        assert rec["poisoned_window_is_nan"], name


def test_unsupported_geometry_is_refused_before_any_launch(record):
    assert set(record["refusals"]) == {"S over the cap", "wt does not divide", "wh does not divide", "N - 1 not a square"}
    for name, rec in record["refusals"].items():
        assert rec["fwd"] and "win_attn_fwd" in rec["fwd"], (name, rec)
        assert rec["bwd"] and "win_attn_bwd" in rec["bwd"], (name, rec)
        assert rec["nothing_written"], name


def test_a_wider_frame_stride_gives_the_same_bits_and_leaves_the_spare_rows(record):
    assert len(record["stride"]) == len(W.SHAPES)
    for name, rec in record["stride"].items():
        assert rec["identical"], name
        assert rec["spare_rows_intact"], name
