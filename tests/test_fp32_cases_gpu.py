"""Every call form of the reference-precision kernels of csrc/fp32.hip (tests/fp32_cases.py) against float64.

None of these kernels reads an environment switch, so one module-scoped fixture runs every case once in this process,
through ctypes, with every output and workspace handed in filled with NaN.  A record holds, per output, the worst error as a
fraction of the bound derived in fp32_cases.py, whether every element is finite, whether the NaN padding behind the output
survived, the bit identities (a second run, strided against dense operands, a row block against the whole launch, out2 with
and without the column split, an attention item among NaN frames and heads against the item alone, the rows a class-token
backward must not touch, a blend that blends nothing against aim_patchify_f32) and what the NaN-filled workspaces hold after
the call.

Measured on MI355X (1891 cases; worst error / bound): gemm out 0.30, out2 0.98 (the bound of out2 is the one rounding of acc +
bias plus the accumulation, so a `bigpre` row comes close to it); attn_fwd out 0.014; attn_bwd dq 0.012, dk 0.017, dv 0.030;
cls_fwd out 0.03, cls_bwd dq 0.25, dk 0.30, dv 0.32; tattn_fwd out 0.04, tattn_bwd dq 0.62, dk 0.52, dv 0.54; lambda lam 0.07,
one_minus 0.49; wgrad dW 0.21, db 0.11; embed_ln x 0.22, mean 0.22, rstd 0.23, pre exact (0); patchify and patchify_blend exact
(0).  Activation probe, worst error / (1 + |x|): ACT QuickGELU 1.56 u, ACT GELU 1.34 u, DACT QuickGELU 2.03 u, DACT GELU
0.98 u against E_ACT = E_DACT = 16 u.  All cases run in 5.5 s, the module in 7.6 s (test_rowwise_gpu.py: 3.8 s; most of it is
the 1245 attention launches of the N sweep with their float64 references; the docstring of test_attn_routes_gpu.py records
no run time to compare with: its fixture takes minutes, one child process per route)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fp32_cases as fc  # noqa: E402


@pytest.fixture(scope="module")
def res():
    r = fc.run("cuda")
    if "fatal" in r:              # nothing more was started on the GPU after it
        pytest.fail(f"{r['fatal']}: {r['errors'][r['fatal']]}")
    print(f"fp32_cases.run: {len(r['cases'])} cases in {r['seconds']:.1f} s, with the refusals and the probe {r['seconds_all']:.1f} s")
    return r


def test_every_case_is_inside_its_bound(res):
    names = [c.name for c in fc.cases()]
    assert not res["errors"], "\n".join(f"{k}: {v}" for k, v in list(res["errors"].items())[:20])
    assert list(res["cases"]) == names, "not every case ran"
    bad, worst = [], {}
    for name, rec in res["cases"].items():
        assert rec["checks"], name
        for k, r in rec["checks"].items():
            key = f"{rec['kind']} {k}"
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


def test_workspaces_show_the_route(res):
    """workspaces go in filled with NaN.  attn_bwd_f32 leaves exactly BT H N 2 finite floats (the rows' log-sum-exp and
    rowsum(P o dP)); wgrad_f32 leaves exactly chunks (Nw Kw [+ Nw]) finite floats, partial z is the product over the rows of chunk
    z (so chunks and chunk are what the mirrors say), and a chunk with no rows holds zeros"""
    bad, seen = [], {}
    for name, rec in res["cases"].items():
        if rec["kind"] not in ("attn_bwd", "wgrad"):
            continue
        assert rec["evidence"], name
        for k, ok in rec["evidence"].items():
            seen[(rec["kind"], k)] = seen.get((rec["kind"], k), 0) + 1
            if not ok:
                bad.append(f"{name}: {k} does not hold")
    print("evidence: " + ", ".join(f"{k[0]} {k[1]} x{v}" for k, v in sorted(seen.items())))
    for key in (("attn_bwd", "workspace_bytes_as_mirrored"), ("attn_bwd", "stats_exactly_finite"), ("wgrad", "workspace_bytes_as_mirrored"),
                ("wgrad", "partials_exactly_finite"), ("wgrad", "partials_are_the_chunks"), ("wgrad", "empty_chunk_is_zero")):
        assert seen.get(key, 0) > 0, key
    assert not bad, "\n".join(bad[:40])


def test_bit_identities(res):
    bad, count = [], {}
    for name, rec in res["cases"].items():
        for k, ok in rec["ident"].items():
            count[k] = count.get(k, 0) + 1
            if not ok:
                bad.append(f"{name}: {k} does not hold")
    print("identities: " + ", ".join(f"{k} x{v}" for k, v in sorted(count.items())))
    for k in ("repeat", "strided_eq_dense", "row_alone", "out2_split", "nan_neighbours", "other_rows_kept", "base_plus_zero",
              "blend_noop_eq_patchify"):
        assert count.get(k, 0) > 0, k
    want = sum(len(c.p.get("ident", ())) for c in fc.cases())
    assert sum(v for k, v in count.items() if k not in ("other_rows_kept", "blend_noop_eq_patchify")) == want      # none fell out silently
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_refusals_are_loud(res):
    assert set(res["refusals"]) == set(fc.REFUSAL_TEXT)
    for name, rec in res["refusals"].items():
        assert rec["rc"] != 0 and rec["message"] and fc.REFUSAL_TEXT[name] in rec["message"], (name, rec)
        assert rec["untouched"], f"{name}: refused, yet an output or the workspace was written"


def test_activation_constants(res):
    """the K = 4 probe (pre = x exactly): E_ACT and E_DACT are at least twice the worst error / (1 + |x|) the GPU shows, and the
    worst recorded in fp32_cases.MEASURED_ACT is still what the GPU shows (within a factor of two)"""
    probe = res["probe"]
    print("activation probe, worst error / (1 + |x|): " + ", ".join(f"{k} {v:.3g} ({v / fc.U:.2f} u)" for k, v in sorted(probe.items())))
    assert set(probe) == set(fc.MEASURED_ACT)
    for k, v in probe.items():
        const = fc.E_ACT if k.startswith("act") else fc.E_DACT
        assert 2 * v <= const, (k, v, const)
        assert fc.MEASURED_ACT[k] is not None and v <= 2 * fc.MEASURED_ACT[k], (k, v, fc.MEASURED_ACT[k])
