"""The 3-D Swin attention kernels (aim_swin3d_attn_fwd / _bwd) against float64 within the bounds of tests/swin3d_attn_cases.py:
the whole case list runs once, in one child process, and the tests read its record."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin3d_attn_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("swin3d_attn") / "record.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "swin3d_attn_cases.py"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(path) as f:
        return json.load(f)


def test_every_case_ran(record):
    assert sorted(record["cases"]) == sorted(c.name for c in W.cases())


def test_forward_backward_and_table_gradient_within_bounds(record):
    bad = []
    for name, rec in record["cases"].items():
        assert set(rec["checks"]) == {"out", "lse", "dq", "dk", "dv", "dtable", "dtable_added"}, name
        for k, r in rec["checks"].items():
            print(f"{name} {k}: {r:.3f}")
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3f}")
    assert not bad, "\n".join(bad)


def test_two_runs_are_bit_identical_table_gradient_included(record):
    for name, rec in record["cases"].items():
        assert set(rec["repeat"]) >= {"out", "lse2", "delta", "dqkv", "dtable"}, name
        assert all(rec["repeat"].values()), (name, rec["repeat"])


def test_nothing_is_written_past_the_results(record):
    for name, rec in record["cases"].items():
        assert all(rec["spare_intact"].values()), (name, rec["spare_intact"])
        assert all(rec["finite"].values()), (name, rec["finite"])


def test_dqkv_does_not_depend_on_whether_the_table_gradient_is_wanted(record):
    for name, rec in record["cases"].items():
        assert rec["dqkv_without_dtable_same_bits"], name


def test_a_zero_head_of_dout_gives_exact_zeros(record):
    seen = 0
    for name, rec in record["cases"].items():
        if name.endswith("/zero_do"):
            assert all(rec["zero_head"].values()), (name, rec["zero_head"])
            seen += 1
    assert seen == len(W.SHAPES)


def test_a_single_token_box_copies_v_and_dout_bit_for_bit(record):
    seen = 0
    for name, rec in record["cases"].items():
        if "one_key" in rec:
            assert rec["one_key"]["tokens"] > 0 and all(rec["one_key"].values()), (name, rec["one_key"])
            seen += 1
    assert seen >= len(W.FAMILIES)


def test_the_walk_case_ran_three_or_more_boxes_per_workgroup(record):
    recs = [rec for name, rec in record["cases"].items() if name.startswith("walk/")]
    assert recs and all(rec["walks"][1] >= 3 for rec in recs)


def test_unsupported_geometry_is_refused_before_any_launch(record):
    assert set(record["refusals"]) == {"window does not divide D", "window does not divide G", "shift outside the window", "negative shift",
                                       "shift on a window that spans its axis", "too many tokens", "too many table entries",
                                       "full window smaller than the window", "rows overflow 32-bit offsets"}
    for name, rec in record["refusals"].items():
        assert rec["fwd"] and "swin3d_attn_fwd" in rec["fwd"], (name, rec)
        assert rec["bwd"] and "swin3d_attn_bwd" in rec["bwd"], (name, rec)
        assert rec["nothing_written"], name


def test_bad_pointers_and_workspaces_are_refused_before_any_launch(record):
    assert len(record["pointer_refusals"]) == 8 + 14
    for name, rec in record["pointer_refusals"].items():
        assert rec["rc"] != 0 and rec["message"] and "swin3d_attn" in rec["message"], (name, rec)
        assert rec["nothing_written"], name


def test_a_workspace_of_exactly_the_reported_size_is_enough(record):
    g = record["workspace_guard"]
    assert g["rc"] == 0, g
    assert g["workspace_bytes"][0] == g["workspace_bytes"][1] > 0
    assert g["sentinels_intact"] and g["workspace_written"] and g["other_spares_intact"], g
    assert g["dtable_same_bits"] and g["dqkv_same_bits"], g
