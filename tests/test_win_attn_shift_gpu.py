"""The shifted 3-D window attention kernels (aim_win_attn_fwd_shift / aim_win_attn_bwd_shift) against float64 within the
bounds of tests/win_attn_shift_cases.py: the whole case list runs once, in one child process, and the tests read its record."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_shift_cases as WS  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = [c for c in WS.cases() if c.family == "unit"]


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("win_attn_shift") / "record.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "win_attn_shift_cases.py"), path], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(path) as f:
        return json.load(f)


def test_every_case_ran(record):
    assert sorted(record["cases"]) == sorted(c.name for c in WS.cases())


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


def test_a_nan_box_stays_in_its_box_even_beside_its_window_mates(record):
    assert sorted(record["poison"]) == sorted(c.name for c in UNIT)
    for name, rec in record["poison"].items():
        assert rec["independent"], name
        assert rec["window_mates"] >= 1 and rec["window_mates_independent"], name
        assert rec["finite_with_nan_class_rows"], name
        assert rec["poisoned_box_is_nan"], name


def test_a_nan_clip_leaves_the_other_clip(record):
    two = [c.name for c in UNIT if c.B > 1]
    assert two
    for name in two:
        assert record["poison"][name]["clip0_independent_of_clip1"], name


def test_a_wider_frame_stride_gives_the_same_bits_and_leaves_the_spare_rows(record):
    assert sorted(record["stride"]) == sorted(c.name for c in UNIT)
    for name, rec in record["stride"].items():
        assert rec["identical"], name
        assert rec["spare_rows_intact"], name


def test_zero_shift_gives_the_bits_of_the_unshifted_kernels(record):
    assert sorted(record["zero_shift"]) == sorted(c.name for c in UNIT)
    for name, rec in record["zero_shift"].items():
        assert set(rec) == {"out", "lse", "dqkv", "delta"} and all(rec.values()), (name, rec)


def test_t_only_shift_gives_the_bits_of_the_unshifted_kernels_on_rolled_frames(record):
    assert sorted(record["t_shift"]) == sorted(c.name for c in UNIT if c.shift[0])
    assert len(record["t_shift"]) >= 4
    for name, rec in record["t_shift"].items():
        assert rec.pop("roll_matters"), name
        assert set(rec) == {"out", "lse", "dqkv", "delta"} and all(rec.values()), (name, rec)


def test_unsupported_geometry_and_shifts_are_refused_before_any_launch(record):
    assert set(record["refusals"]) == set(WS.REFUSALS)
    for name, rec in record["refusals"].items():
        assert rec["fwd"] and "win_attn_fwd_shift" in rec["fwd"], (name, rec)
        assert rec["bwd"] and "win_attn_bwd_shift" in rec["bwd"], (name, rec)
        assert rec["nothing_written"], name
