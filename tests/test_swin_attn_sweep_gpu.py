"""The Swin attention kernels at every size and shift, and on the backward's walk over several sequences per workgroup
(`chunk_cases` and `sweep_cases` of tests/swin_attn_cases.py), against float64 within the bounds `expected()` derives; the exact
properties of one-key regions, of a zero dO head and of neighbouring sequences; the refusals of bad pointers and workspaces; the
workspace's end and the scatter's addition.  The lists run once, in one child process (`swin_attn_cases.py --sweep`), and the
tests read its record.

The window backward runs per = 3 sequences per workgroup at S = 49, 64 and 16, the temporal backward per = 3 at T' = 5 and 32,
and one window case runs per = 8 (256 chunks, the last one of 3).

Measured on the MI355X, worst error / bound (pass: <= 1.0):
                       out    lse    dq     dk     dv     dbias  dtable
  chunk cases (12)     0.891  0.041  0.929  0.905  0.945  0.007  0.005
  temporal sweep (44)  0.812  0.068  0.832  0.881  0.857  0.042  0.017
  window sweep (68)    0.844  0.086  0.873  0.918  0.966  0.044  0.035
  scatter onto a non-zero table: window index 0.789, temporal index 0.505
Every exact property held and no kernel defect was found.  Wall time of the child: 10.0 s, 8.0 s of it in the cases
(tests/test_swin_attn_gpu.py's child: 2.6 s); the timeout is ten times that, and no less than 120 s."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_attn_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {c.name: c for c in W.chunk_cases() + W.sweep_cases()}
RESULTS = ("out", "lse", "dq", "dk", "dv", "dbias", "dtable")


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("swin_attn_sweep") / "record.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "swin_attn_cases.py"), "--sweep", path], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(path) as f:
        return json.load(f)


def test_every_case_ran(record):
    assert sorted(record["cases"]) == sorted(CASES) and len(CASES) == 124
    print(f"child: {record['seconds']:.1f} s")


def test_forward_backward_and_bias_gradients_within_bounds(record):
    bad, worst = [], {}
    for name, rec in record["cases"].items():
        assert set(rec["checks"]) == set(RESULTS), name
        for k, r in rec["checks"].items():
            if not r <= worst.get(k, (0.0, ""))[0]:
                worst[k] = (r, name)
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3f}")
    for k in RESULTS:
        print(f"worst {k}: {worst[k][0]:.3f} ({worst[k][1]})")
    for group in ("chunk/", "sweep/t/", "sweep/win/"):
        print(group, {k: round(max(rec["checks"][k] for n, rec in record["cases"].items() if n.startswith(group)), 3) for k in RESULTS})
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


def test_workspace_size_is_chunks_times_the_dense_gradient(record):
    for name, rec in record["cases"].items():
        c = CASES[name]
        nch, _ = W.chunks(c.nseq, c.H)
        assert rec["workspace_bytes"] == [nch * c.H * c.S * c.S * 4] * 2, (name, rec["workspace_bytes"])


def test_a_zero_dO_head_has_exactly_zero_gradients(record):
    n = 0
    for name, rec in record["cases"].items():
        assert ("zero_head" in rec) == (CASES[name].family == "zero_do"), name
        if "zero_head" in rec:
            assert set(rec["zero_head"]) == {"dq", "dk", "dv", "dbias", "dtable", "other_heads_live"}
            assert all(rec["zero_head"].values()), (name, rec["zero_head"])
            n += 1
    assert n == 4 + 8


def test_a_token_alone_in_its_region_is_copied_and_has_no_score_gradient(record):
    """s = 1 or s = w - 1: out = v and dv = dO bit for bit, dq = dk = 0, and the bias gradients keep every bit when the
    token's q, k, v and dO are replaced (dS = 0 exactly inside a masked window)"""
    n = 0
    for name, rec in record["cases"].items():
        c = CASES[name]
        want = c.kind == "win" and c.dims[2] > 1 and c.dims[3] in (1, c.dims[2] - 1)
        assert ("one_key" in rec) == want, name
        if want:
            ok = rec["one_key"]
            lone = int(W.lone_tokens(c).sum())
            assert lone > 0 and ok.pop("tokens") == lone, name
            assert len(ok) == 10 and all(ok.values()), (name, ok)
            n += 1
    assert n == 2 + (1 + 2 * 2) + 4 * 2 * 5           # the deep chunk case; w = 2 .. 4; w = 5 .. 8 in every family


def test_replacing_one_sequence_of_a_chunk_changes_no_other_sequence(record):
    """the stale-LDS check of the per > 1 walk: a mid-chunk sequence's rows replaced, all other rows keep their bits"""
    n = 0
    for name, rec in record["cases"].items():
        c = CASES[name]
        nch, per = W.chunks(c.nseq, c.H)
        assert ("no_leak" in rec) == (per > 1) == name.startswith("chunk/"), name
        if per > 1:
            nl = rec["no_leak"]
            assert nl["per"] == per and nl["sequence"] == nl["chunk"] * per + 1 and 0 < nl["chunk"] < nch - 1, (name, nl)
            assert all(nl[k] for k in ("out", "dqkv", "dqkv_nobias", "lse2", "replaced_sequence_differs")), (name, nl)
            n += 1
    assert n == 12


def test_bad_pointers_and_workspaces_are_refused_before_any_launch(record):
    want = set()
    for entry in ("swin_win_attn_", "swin_tattn_"):
        want |= {f"{entry}fwd: null {k}" for k in ("qkv", "bias", "out", "lse")}
        want |= {f"{entry}fwd: {k} off by 2 bytes" for k in ("qkv", "out")}
        want |= {f"{entry}bwd: null {k}" for k in ("qkv", "bias", "dout", "lse", "dqkv")}
        want |= {f"{entry}bwd: {k} off by 2 bytes" for k in ("qkv", "dout", "dqkv")}
        want |= {f"{entry}bwd: workspace 4 bytes short", f"{entry}bwd: null workspace"}
    assert set(record["pointer_refusals"]) == want and len(want) == 32
    for name, rec in record["pointer_refusals"].items():
        assert rec["rc"] != 0 and rec["message"] and name.split(":")[0] in rec["message"], (name, rec)
        assert rec["nothing_written"], name


def test_the_backward_stays_inside_a_workspace_of_the_reported_size(record):
    g = record["workspace_guard"]
    c = W.chunk_cases()[0]
    assert g["rc"] == 0 and g["workspace_bytes"] == W.chunks(c.nseq, c.H)[0] * c.H * c.S * c.S * 4, g
    assert g["workspace_written"] and g["sentinels_intact"] and g["other_spares_intact"], g
    assert g["dbias_same_bits"] and g["dqkv_same_bits"], g


def test_the_scatter_adds_to_what_the_table_gradient_holds(record):
    assert set(record["scatter_adds"]) == {"window", "temporal"}
    for name, rec in record["scatter_adds"].items():
        print(f"scatter {name}: {rec['ratio']:.3f}")
        assert rec["ratio"] <= 1.0, (name, rec)
        assert rec["unnamed_rows"] == 4 and rec["unnamed_rows_keep_their_bits"] and rec["spare_intact"] and rec["start_nonzero"], (name, rec)
        assert rec["ntable_H"] % 128 != 0, (name, rec)
