"""The cut 3-D window attention kernels (aim_win_attn_fwd_cut / aim_win_attn_bwd_cut) against float64 within the bounds of
tests/win_attn_cut_cases.py: the whole case list runs once, in one child process, and the tests read its record.  Every result
buffer is pre-filled with NaN, so a row that must not be written (class rows, the spare row of P = N + 1, the elements behind a
buffer) is seen if it is."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import win_attn_cut_cases as WC  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = [c for c in WC.cases() if c.family == "unit"]
NAMES = ("out", "lse", "delta", "dq@a", "dk@a", "dv@a", "dq@b", "dk@b", "dv@b")


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("win_attn_cut") / "record.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "win_attn_cut_cases.py"), path], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(path) as f:
        return json.load(f)


def test_every_case_ran(record):
    assert sorted(record["cases"]) == sorted(c.name for c in WC.cases())


def test_forward_and_backward_within_bounds_at_both_strides(record):
    bad = []
    for name, rec in record["cases"].items():
        assert set(rec["checks"]) == {f"{k}/{p}" for k in NAMES for p in ("N", "N+1")}, name
        for k, r in rec["checks"].items():
            print(f"{name} {k}: {r:.3f}")
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3f}")
    assert not bad, "\n".join(bad)


def test_two_runs_and_both_strides_are_bit_identical(record):
    for name, rec in record["cases"].items():
        assert all(rec["repeat"].values()), (name, rec["repeat"])
        assert rec["same_bits_at_both_strides"], name
        assert all(rec["finite"].values()), (name, rec["finite"])


def test_class_rows_spare_rows_and_spare_elements_keep_their_nan(record):
    for name, rec in record["cases"].items():
        assert set(rec["untouched"]) == {"N", "N+1"} and all(rec["untouched"].values()), (name, rec["untouched"])


def test_zero_t_shift_gives_the_bits_of_the_shift_entries(record):
    assert sorted(record["bits"]) == sorted(c.name for c in UNIT)
    for name, rec in record["bits"].items():
        assert set(rec["st0_vs_shift"]) == {"out", "lse", "dqkv", "delta"} and all(rec["st0_vs_shift"].values()), (name, rec)


def test_zero_shift_gives_the_bits_of_the_unshifted_kernels(record):
    for name, rec in record["bits"].items():
        assert set(rec["zero_vs_plain"]) == {"out", "lse", "dqkv", "delta"} and all(rec["zero_vs_plain"].values()), (name, rec)


def test_the_t_cut_is_live(record):
    live = [name for name, rec in record["bits"].items() if "t_cut_matters" in rec]
    assert len(live) == len(UNIT)
    for name in live:
        assert record["bits"][name]["t_cut_matters"], name


def test_unsupported_geometry_and_shifts_are_refused_before_any_launch(record):
    assert set(record["refusals"]) == set(WC.REFUSALS)
    for name, rec in record["refusals"].items():
        assert rec["fwd"] and "win_attn_fwd_cut" in rec["fwd"], (name, rec)
        assert rec["bwd"] and "win_attn_bwd_cut" in rec["bwd"], (name, rec)
        assert rec["nothing_written"], name
