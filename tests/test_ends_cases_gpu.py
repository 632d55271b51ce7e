"""Every call form of the head, loss, lamda, patch-gather and AdamW kernels (tests/ends_cases.py) against float64.

None of these kernels reads an environment switch, so one module-scoped fixture runs every case once in this process,
through ctypes.  A record holds, per output, the worst error as a fraction of the bound derived in ends_cases.py, whether
every element is finite wherever the reference is, whether the NaN guard behind the output (and the partial slots a call
does not own) survived, the bit identities (a second run, a sample or frame of a launch against the same one launched alone,
the 8-pixel loads against the scalar gather, NULL against a table of ones / zeros, a subset of head_bwd's outputs against
the full call, AdamW's n % 4 tail against the four-wide body) and, where the reference is NaN, which outputs were.

Measured on MI355X (350 cases; worst error / bound): head_fwd pooled 0.49, score 0.14; head_bwd dW 0.73, db 0.96 (B = 1: one
rounding against a bound of one), dfeat 0.30; ce_topk loss 0.22, per_sample 0.55, dscore 0.30, accuracies exact -- the two
__expf / __logf terms, given 4 x their model, are nowhere near their share; ce_soft out 0.09, per_sample 0.22, dscore 0.44;
qk_cross ss 0.02; qk_border ss 0.01, max 0.05, max + log(sum) 0.05; lambda lam 0.46, 1 - lam 0.40; lambda_partials lam
0.15, 1 - lam 0.20; patchify exact (0) and bit-identical to torch's bf16; adamw m 0.87, v 0.99, update 0.98 (g = 0: one rounding
against a bound of one).  NaN where the reference is NaN: out[0] of 19 ce_topk cases, out (and dscore when asked for) of 5
ce_soft cases.  Identities: repeat x350, row_alone x131 (head_fwd 18, ce_topk 42, ce_soft 35, lambda 20, qk_cross 6, qk_border 4,
lambda_partials 6), subset_eq_full x32, null_eq_ones x32 (head_fwd 27, ce_soft 5), fast_eq_scalar x24, exact_bits x54,
tail_eq_vector x45; 16 refusals.  All cases run in 1.1 s, the module in 3.3 s.
"""
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ends_cases as ec  # noqa: E402

T0 = time.time()


@pytest.fixture(scope="module")
def res():
    r = ec.run("cuda")
    if "fatal" in r:              # nothing more was started on the GPU after it
        pytest.fail(f"{r['fatal']}: {r['errors'][r['fatal']]}")
    print(f"ends_cases.run: {len(r['cases'])} cases in {r['seconds']:.1f} s")
    return r


def test_every_case_is_inside_its_bound(res):
    names = [c.name for c in ec.cases()]
    assert not res["errors"], "\n".join(f"{k}: {v}" for k, v in list(res["errors"].items())[:20])
    assert list(res["cases"]) == names, "not every case ran"
    bad, worst = [], {}
    for name, rec in res["cases"].items():
        assert rec["checks"], name
        for k, r in rec["checks"].items():
            key = f"{rec['kind']} {k}"
            worst[key] = max(worst.get(key, 0.0), r)
            print(f"  {name} {k}: {r:.4g}")
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3g}")
        for k, ok in rec["finite"].items():
            if not ok:
                bad.append(f"{name} {k}: non-finite element where the reference is finite")
        for k, ok in rec["pad"].items():
            if not ok:
                bad.append(f"{name} {k}: write outside the output (NaN guard changed)")
        assert set(rec["finite"]) == set(rec["pad"]) == set(rec["checks"]), name
    print(f"{len(names)} cases, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_nan_where_the_reference_is_nan(res):
    """all labels ignored (aim_ce_topk), class weights with sum w y = 0 (aim_ce_soft): 0 / 0.  That the output IS NaN there is
    part of the comparison above; this prints which outputs were and checks that both entry points have such a case"""
    seen = {}
    for name, rec in res["cases"].items():
        if rec["nan"] is not None:
            seen.setdefault(rec["kind"], []).append((name, sorted(k for k, v in rec["nan"].items() if v)))
    for kind, lst in sorted(seen.items()):
        print(f"{kind}: " + "; ".join(f"{n} -> NaN in {ks}" for n, ks in lst))
    assert set(seen) == {"ce_topk", "ce_soft"}
    assert all("loss" in ks for _, ks in seen["ce_topk"]) and all("out" in ks for _, ks in seen["ce_soft"])


def test_bit_identities(res):
    bad, count = [], {}
    for name, rec in res["cases"].items():
        assert "repeat" in rec["ident"], name
        for k, ok in rec["ident"].items():
            count[(rec["kind"], k)] = count.get((rec["kind"], k), 0) + 1
            if not ok:
                bad.append(f"{name}: {k} does not hold")
    print("identities: " + ", ".join(f"{k[0]} {k[1]} x{v}" for k, v in sorted(count.items())))
    for kind in ("head_fwd", "ce_topk", "ce_soft", "lambda", "qk_cross", "qk_border", "lam_part"):
        assert count.get((kind, "row_alone"), 0) > 0, kind
    for key in (("patchify", "fast_eq_scalar"), ("patchify", "exact_bits"), ("head_fwd", "null_eq_ones"), ("ce_soft", "null_eq_ones"),
                ("head_bwd", "subset_eq_full"), ("adamw", "tail_eq_vector")):
        assert count.get(key, 0) > 0, key
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_refusals_are_loud(res):
    assert set(res["refusals"]) == set(ec.REFUSAL_TEXT)
    for name, rec in res["refusals"].items():
        assert rec["message"] and ec.REFUSAL_TEXT[name] in rec["message"], (name, rec["message"])
        assert rec["untouched"], f"{name}: refused, yet an output was written"
    print(f"module: {time.time() - T0:.1f} s")
