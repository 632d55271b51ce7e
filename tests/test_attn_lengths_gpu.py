"""The attention kernels that no route switch reaches (tests/attn_cases.py: length_cases), at every length they accept,
against float64.

The class query of the last block (aim_attn_fwd_cls / aim_attn_bwd_cls, kind `clsq`) at every N from 1 to 288, seven input
families on every seventh N and at five product and edge geometries; the temporal kernels (aim_cls_attn_*, aim_tattn_*) at
every T from 1 to 32 at two geometries; aim_tattn_fwd_infer on the same T sweep in both output forms.  Two child processes,
started one after the other: `lengths` runs all of it under the default bf16 LDS staging of the inference kernel, `lds32`
runs the inference forms again with AIM_TATTN_LDS16=0 (the switch is read once per process).  A child that fails ends the
fixture: the next one is not started.

Per case the children report the worst error as a fraction of the bound derived in attn_cases.py, whether the NaN padding
behind every output survived, whether a second run gave the same bits and whether everything is finite; clsq cases also
whether out / lse are row 0 of aim_attn_fwd bit for bit, whether NaN in the q part of every non-class row changed a bit,
whether every non-class dQ row is exactly zero and whether a head without dO has exactly zero gradients.
tests/test_attn_cases_cpu.py proves that these comparisons reject the kernel bugs they are meant to catch.

Measured on MI355X (831 cases; worst error / bound, form a / form b of the backward):
  clsq   out 0.672, lse 0.020, dq 0.370 / 0.196, dk 0.860 / 0.507, dv 0.977 / 0.972 (all but lse equal the CPU emulation's
         figure to three digits; dK and dV of a key are single products rounded twice, the bound's two-rounding core)
  cls    out 0.975, probs 0.011, dcompact 0.996 / 0.982, dfull 0.996 / 0.993
  tattn  out 0.974, probs 0.014, dqkv 0.996 / 0.979
  aim_tattn_fwd_infer, fp8 bytes that are the neighbour of the float64 cast, per pool, the same under both stagings:
         B1N3H1 unit 0, peaked 0 of 101 376; B2N5H3 unit 0, peaked 8 of 1 013 760 (7.9e-6); none farther than one code
Both children together take 22 s.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_cases as ac  # noqa: E402

TIMEOUT = {"lengths": 90, "lds32": 45}         # seconds; most of a child is process start-up and the float64 references


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    out = {}
    for mode in ac.LENGTH_MODES:
        env = {k: v for k, v in os.environ.items() if k not in ac.ROUTE_VARS + ("AIM_TATTN_LDS16",)}
        env.update(ac.LENGTH_ENV[mode])
        path = str(tmp_path_factory.mktemp("attn_lengths") / f"{mode}.json")
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "attn_cases.py"), mode, path], env=env, timeout=TIMEOUT[mode],
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:      # nothing more is started on the GPU
            pytest.fail(f"{mode}: child did not finish within {TIMEOUT[mode]} s")
        if p.returncode != 0:
            pytest.fail(f"{mode}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[mode] = json.load(f)
    return out


def test_every_length_is_inside_its_bound(children):
    res = children["lengths"]
    names = [c.name for c in ac.length_cases()]
    assert list(res["cases"]) == names, "the child did not run every case"
    bad, worst = [], {}
    for name, rec in res["cases"].items():
        for k, r in rec["checks"].items():
            key = name.split("/")[0] + " " + k
            worst[key] = max(worst.get(key, 0.0), r)
            if not r <= 1.0:
                bad.append(f"{name} {k}: error / bound = {r:.3g}")
        for k, ok in rec["finite"].items():
            if not ok:
                bad.append(f"{name} {k}: non-finite element")
        for k, ok in rec["pad"].items():
            if not ok:
                bad.append(f"{name} {k}: write outside the output (NaN padding changed)")
        for k in rec:
            if k.startswith("other_rows_kept") and not rec[k]:
                bad.append(f"{name} {k}: cls_attn_bwd changed a row that is not a class row")
    print(f"{len(names)} cases, worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_class_query_exact_properties(children):
    res, bad, n = children["lengths"]["cases"], [], 0
    for case in ac.length_cases():
        if case.kind != "clsq":
            continue
        n += 1
        rec = res[case.name]
        assert set(rec["repeat"]) == set(rec["poison"]) == set(rec["pad"]) == {"out", "lse", "dqkv@a", "dqkv@b"}
        if not rec["row0_of_attn_fwd"]:
            bad.append(f"{case.name}: out_cls / lse_cls are not row 0 of aim_attn_fwd")
        for k, ok in rec["repeat"].items():
            if not ok:
                bad.append(f"{case.name} {k}: a second run gave other bits")
        for k, ok in rec["poison"].items():
            if not ok:
                bad.append(f"{case.name} {k}: depends on the q part of a non-class row")
        for form in "ab":
            if not rec[f"other_dq_zero@{form}"]:
                bad.append(f"{case.name} form {form}: a non-class dQ row is not exactly zero")
            if not rec[f"finite@{form}"]:
                bad.append(f"{case.name} form {form}: non-finite gradient")
            assert (f"zero_head@{form}" in rec) == (case.family == "zero_do")
            if not rec.get(f"zero_head@{form}", True):
                bad.append(f"{case.name} form {form}: dO = 0 for a head, but its gradients are not exactly zero")
    assert n == 575
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_temporal_kernels_repeat_their_bits(children):
    bad, n = [], 0
    for name, rec in children["lengths"]["cases"].items():
        if name.startswith("clsq/"):
            continue
        n += 1
        bad += [f"{name} {k}: a second run gave other bits" for k, ok in rec["repeat"].items() if not ok]
    assert n == 2 * 2 * 2 * ac.TMAX and not bad, "\n".join(bad[:40])


def test_tattn_infer_every_T_under_both_stagings(children):
    """bf16 form: the bits of aim_tattn_fwd's out.  fp8 form: every byte is the e4m3 cast of the float64 result or its
    neighbour on the grid, the two stagings give equal bytes, and per pool (all T of one geometry and family) at most 1e-3 of
    the bytes are neighbours (tests/test_attn_cases_cpu.py: an fp32 emulation of the kernel stays under a third of that)"""
    names = [c.name for c in ac.length_cases() if c.kind == "tattn"]
    bad, sat = [], 0
    for mode in ac.LENGTH_MODES:
        res = children[mode]["infer"]
        assert list(res) == names, f"{mode}: the child did not run every case"
        pools = {}
        for name, rec in res.items():
            if not rec["bf16_is_tattn_fwd"]:
                bad.append(f"{mode} {name}: the bf16 form differs from aim_tattn_fwd")
            if rec["farther"]:
                bad.append(f"{mode} {name}: {rec['farther']} bytes are farther than one code from the float64 cast")
            bad += [f"{mode} {name} {k}: write outside the output" for k, ok in rec["pad"].items() if not ok]
            bad += [f"{mode} {name} {k}: a second run gave other bits" for k, ok in rec["repeat"].items() if not ok]
            if rec["hash8"] != children["lengths"]["infer"][name]["hash8"]:
                bad.append(f"{name}: the fp8 bytes differ between the two stagings")
            if "saturates" in rec:
                sat += 1
                if not rec["saturates"]:
                    bad.append(f"{mode} {name}: |out| = 600 is not stored as +-448")
            n, d = pools.get(rec["pool"], (0, 0))
            pools[rec["pool"]] = (n + rec["bytes"], d + rec["neighbours"])
        assert len(pools) == 4
        for pool, (n, d) in sorted(pools.items()):
            print(f"TATTN8 {mode} {pool}: bytes {n} neighbours {d} ({d / n:.2e})")
            if d / n > ac.INFER_CAP:
                bad.append(f"{mode} {pool}: {d} of {n} bytes differ from the float64 cast")
    assert sat == 2 * len(ac.SAT_T) * len(ac.SWEEP_GEOMS)
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_class_query_refusals_are_loud(children):
    for mode in ac.LENGTH_MODES:
        ref = children[mode]["refusals"]
        for kernel in ("attn_fwd_cls", "attn_bwd_cls"):
            for tag in ("N=289", "N=0", "BT=0"):
                msg = ref[f"{kernel} {tag}"]
                assert msg and f"{kernel}: unsupported shape" in msg and "N <= 288" in msg, (mode, kernel, tag, msg)
            msg = ref[f"{kernel} null lse_cls"]
            assert msg and f"{kernel}: null pointer" in msg, (mode, kernel, msg)
        assert children[mode]["refusals_untouched"] == {"out_cls": True, "lse_cls": True, "dqkv": True}
