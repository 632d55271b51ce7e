"""Every call form of the LayerNorm, embedding, reduction, row-add and cast kernels (tests/rowwise_cases.py) against float64.

None of these kernels reads an environment switch, so one module-scoped fixture runs every case once in this process.  A
record holds, per output, the worst error as a fraction of the bound derived in rowwise_cases.py, whether every element is
finite, whether the NaN padding behind the output survived, the bit identities (a second run, strided against dense
operands, a row of a launch against the row alone, NaN neighbours, bf16 / e4m3 twins of one call, dy = 0) and what the
NaN-filled workspaces show of the route taken.

Measured on MI355X (377 cases; worst error / bound): ln_fwd y and y_fp8 together 1.000 (e4m3 ties), y_bf16 0.995, mean 0.15,
rstd 0.25; embed_ln x 0.21, mean 0.21, rstd 0.08; ln_bwd dx 0.94, dx_bf16 0.996, dgamma 0.29, dbeta 0.25; ln_fsum dx_bf16
0.996, partial 0.49; ln_gb dgamma 0.08, dbeta 0.06; embed_bwd dtemporal 0.10; frame_sum 0.50; colsum 0.29; embed_nopre_bwd
dcls 0.22, dpos 0.41, dtemporal 0.26, dbias 0.11; casts, row adds, scale_rows, embed_nopre_fwd and dtok exact (0).  All cases
run in 1.6 s, the module in 3.8 s."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rowwise_cases as rc  # noqa: E402


@pytest.fixture(scope="module")
def res():
    r = rc.run("cuda")
    if "fatal" in r:              # nothing more was started on the GPU after it
        pytest.fail(f"{r['fatal']}: {r['errors'][r['fatal']]}")
    print(f"rowwise_cases.run: {len(r['cases'])} cases in {r['seconds']:.1f} s")
    return r


def test_every_case_is_inside_its_bound(res):
    names = [c.name for c in rc.cases()]
    assert not res["errors"], "\n".join(f"{k}: {v}" for k, v in list(res["errors"].items())[:20])
    assert list(res["cases"]) == names, "not every case ran"
    bad, worst = [], {}
    for name, rec in res["cases"].items():
        assert rec["checks"], name
        for k, r in rec["checks"].items():
            key = f"{rec['kind']} {'dst' if k.startswith('dst') else k}"
            worst[key] = max(worst.get(key, 0.0), r)
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3g}")
        for k, ok in rec["finite"].items():
            if not ok:
                bad.append(f"{name} {k}: non-finite element")
        for k, ok in rec["pad"].items():
            if not ok:
                bad.append(f"{name} {k}: write outside the output (NaN padding changed)")
        assert set(rec["finite"]) == set(rec["pad"]) == set(rec["checks"]), name
    print(f"{len(names)} cases, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_the_route_ran(res):
    """workspaces go in filled with NaN: a two-stage route leaves exactly its partials finite, a one-block or atomic route
    (the scalar colsum kernel included, whatever workspace it is given) leaves all of it NaN"""
    bad, seen = [], {}
    for name, rec in res["cases"].items():
        if rec["kind"] not in ("colsum", "embed_bwd", "ln_gb", "nopre_bwd"):
            continue
        assert rec["evidence"], name
        seen[(rec["kind"], str(rec["route"]))] = seen.get((rec["kind"], str(rec["route"])), 0) + 1
        two_stage = rec["route"] == "two_stage" or rec["kind"] in ("ln_gb", "nopre_bwd")
        assert ("workspace_untouched" in rec["evidence"]) != two_stage, (name, rec["evidence"])
        for k, ok in rec["evidence"].items():
            if not ok:
                bad.append(f"{name} ({rec['route']}): {k} does not hold")
    print("routes: " + ", ".join(f"{k[0]} {k[1]} x{v}" for k, v in sorted(seen.items())))
    for route in ("two_stage", "one_block", "atomic8", "scalar"):
        assert seen.get(("colsum", route), 0) > 0, route
    assert seen.get(("embed_bwd", "two_stage"), 0) > 0 and seen.get(("embed_bwd", "atomic"), 0) > 0
    dp = {rec["route"] for rec in res["cases"].values() if rec["kind"] == "ln_bwd" and rec["route"]}
    assert dp == {"ordered", "atomic"}          # (not visible from outside: rests on ln_dparam_route and the CPU coverage test)
    assert not bad, "\n".join(bad[:40])


def test_bit_identities(res):
    bad, count = [], {}
    for name, rec in res["cases"].items():
        for k, ok in rec["ident"].items():
            count[k] = count.get(k, 0) + 1
            if not ok:
                bad.append(f"{name}: {k} does not hold")
    print("identities: " + ", ".join(f"{k} x{v}" for k, v in sorted(count.items())))
    for k in ("repeat", "strided_eq_dense", "row_alone", "nan_neighbours", "yb_is_bf16_of_y", "y8_is_e4m3_of_y", "x16_eq_f32_of_bf16",
              "other_rows_kept", "zero_dy_exact", "dx_eq_layernorm_bwd", "cast_multi_eq_cast_bf16", "routes_as_mirrored",
              "workspace_bytes_as_mirrored"):
        assert count.get(k, 0) > 0, k
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_large_offsets(res):
    rec = res["large"]
    if not rec["ran"]:
        print(f"large-offset case not run: it needs {rec['need'] / 2 ** 30:.1f} GiB, {rec['free'] / 2 ** 30:.1f} GiB free")
        return
    assert rec["bytes"] > 2 ** 32
    assert all(r <= 1.0 for r in rec["checks"].values()), rec["checks"]
    assert all(rec["finite"].values()), rec["finite"]
    assert rec["identical"], "row 1, beyond 2^32 bytes, differs from the same row launched densely"


def test_refusals_are_loud(res):
    assert set(res["refusals"]) == set(rc.REFUSAL_TEXT)
    for name, rec in res["refusals"].items():
        assert rec["message"] and rc.REFUSAL_TEXT[name] in rec["message"], (name, rec["message"])
        assert rec["untouched"], f"{name}: refused, yet an output or the workspace was written"
