"""CPU self-check of tests/wgrad_cases.py: the bounds that test_wgrad_routes_gpu.py holds the bf16 weight-gradient kernels to
accept an fp32 emulation of the kernels' arithmetic in their summation order on every route, equal the float64 reference bit
for bit on the `exact` family, and reject the same emulation with one plausible kernel bug (a mutant).  Nothing is tuned in
between: the bounds are the derivations in the module docstring of wgrad_cases.py.

Also: the planning mirrors give every route the chunk counts the table is meant to reach (one chunk, 2..8, more than 8, more than
64, fp32 atomics, the bias through aim_colsum_bf16, wgrad_finish1_kernel), every shape, row count, token count, operand form and
workspace form of the issue has a case, and the refusal table matches the AIM_CHECK_ARG texts of the sources."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wgrad_cases as wc  # noqa: E402

CASES = wc.cases()
CSRC = os.path.join(os.path.dirname(HERE), "adapt-image-models_amd", "csrc")


@pytest.fixture(scope="module")
def inputs():
    return {c.name: wc.build_inputs(c) for c in CASES}


def _plans():
    """(case, route, plan) for every launch of the GPU test; routes whose plan repeats an earlier one of the case are left out"""
    for c in CASES:
        seen = set()
        for route in wc.ROUTES:
            if not wc.runs_on(c, route):
                continue
            pl = wc.plan(c, route)
            if pl.sig() not in seen:
                seen.add(pl.sig())
                yield c, route, pl


def test_case_names_are_unique():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


def test_mirrors_and_paths():
    # wgrad_chunks by hand: 1 000 rows of [768 x 192] (3 tiles): 86 workgroups asked, 32 steps -> 32 chunks of 32 rows
    assert wc.wgrad_chunks(1000, 3) == (32, 32)
    assert wc.wgrad_chunks(100864, 3) == (86, 1184)
    assert wc.wgrad_chunks(2100, 1, 3) == (3, 704)
    assert wc.range_chunks(100, 7) == (4, 32) and wc.range_chunks(613, 4) == (4, 160) and wc.range_chunks(700, 1) == (1, 704)
    assert wc.workspace_bytes(1000, 768, 192) == 32 * 768 * 193 * 4 and wc.workspace_bytes(32, 768, 192) == 0
    assert wc.balanced_grid(272, 256) == 136 and wc.balanced_grid(24, 256) == 24 and wc.balanced_grid(1182, 256) == 237
    seen = {}
    for c in CASES:
        for route in wc.ROUTES:
            if not wc.runs_on(c, route):
                continue
            pl = wc.plan(c, route)
            assert all(b < e for b, e in pl.segs) and pl.segs[0][0] == wc.row_range(c)[0] and pl.segs[-1][1] == wc.row_range(c)[1]
            assert all(a[1] == b[0] for a, b in zip(pl.segs, pl.segs[1:]))
            for key in (pl.path, pl.mode, "bias_" + str(pl.bias), "finish_" + pl.finish):
                seen.setdefault((route, key), []).append(c.name)
            if c.kind == "entry" and c.p["ws"] == "short" and pl.C > 1:
                assert pl.mode == "atomics" and pl.have == pl.need - 16
    for route, keys in {"default": wc.PATHS + ("atomics", "slabs", "direct", "bias_fused", "bias_colsum", "bias_direct", "bias_None"),
                        "few": ("C1", "C2_8"), "many": ("C65+",), "nofuse": ("bias_colsum", "C2_8", "C9_64", "C65+"),
                        "finish1": ("finish_one", "C9_64", "C65+")}.items():
        for k in keys:
            assert seen.get((route, k)), (route, k)
            print(f"{route} {k}: {len(seen[(route, k)])} cases")
    # many: one 32-row step per chunk -- 2 100 rows are 66 chunks
    c = next(c for c in CASES if c.kind == "entry" and c.p["rows"] == 2100 and (c.p["Nw"], c.p["Kw"]) == (768, 192))
    assert wc.plan(c, "many").C == 66 and wc.plan(c, "few").C == 1
    # the bias through aim_colsum_bf16 reaches its one-block and its atomic route
    routes = {wc.rw.colsum_plan(wc._colsum_twin(c, wc.build_inputs(c))[0].p)[0] for c, r, pl in _plans() if pl.bias == "colsum"}
    assert {"one_block", "atomic8"} <= routes, routes


def test_the_table_covers_the_issue():
    E = [c for c in CASES if c.kind == "entry"]
    S = [c for c in CASES if c.kind == "slabs"]
    R = [c for c in CASES if c.kind == "ride"]
    assert {c.p["rows"] for c in E} >= set(wc.ROWS)
    assert {(c.p["Nw"], c.p["Kw"]) for c in E} >= set(wc.SHAPES) | {(768, 3072)}
    assert {(c.p["Nw"], c.p["Kw"]) for c in E if c.family == "exact"} >= set(wc.SHAPES)
    assert {c.p["ntok"] for c in E if c.p["bias"] == "at"} >= set(wc.NTOKS)
    assert {(c.p["gf"] != "dense", c.p["af"] != "dense") for c in E} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(c.p["gf"] == "model" for c in E) and any(c.p["af"] == "model" for c in E)
    assert {c.p["xl"] for c in E} >= {0, 4, 64} and {c.p["bias"] for c in E} == {"none", "db", "at"}
    assert {c.p["ws"] for c in E} == {"exact", "null", "short", "large"}
    assert {c.p["atk"] for c in E if c.family != "exact" and c.p["bias"] == "at"} == {"drop", "ramp"}
    assert {c.family for c in CASES} == {"unit", "offset", "exact"}
    assert {r[0][0] for c in S for r in [c.p["ranges"]]} >= {0, 37, 224}
    mcs = {(mc, mc > wc._cdiv(me - mb, 32)) for c in S for mb, me, mc in c.p["ranges"]}
    assert {0, 1, 3, 7} <= {m for m, _ in mcs} and any(over for _, over in mcs)
    assert {wc.plan(c).C for c in S} >= {1, 7, 8, 9, 17, 70}
    assert {c.p["bias"] for c in S} == {"none", "db", "at"} and any(c.p["xl"] for c in S) and any(len(c.p["ranges"]) > 1 for c in S)
    assert len(R) == len(wc.RIDE_HOSTS) * len(wc.RIDE_GRADS) * len(wc.RIDE_CHUNKS)
    for c in R:
        steps = wc._cdiv(c.p["me"] - c.p["mb"], 32)
        C = wc.plan(c).C          # 1 chunk; 3 asked: 3 or, when the steps do not divide, fewer; more than steps: one step each
        assert C == {1: 1, 3: wc._cdiv(steps, wc._cdiv(steps, 3)), 1000: steps}[c.p["chunks"]], c.name


def test_bounds_accept_the_emulation(inputs):
    worst, n, exact = {}, 0, 0
    for c, route, pl in _plans():
        inp = inputs[c.name]
        got = wc.emulate(c, inp, route)
        exp = wc.expected(c, inp, route)
        for k, r in wc.compare(c, inp, got, route).items():
            key = (c.kind, k, "colsum" if k == "db" and pl.bias == "colsum" else pl.mode)
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, (c.name, route, k, r)
            assert bool(torch.isfinite(got[k]).all()), (c.name, route, k)
            if c.family == "exact":
                assert bool((got[k].double() == exp[k][0]).all()) and float(exp[k][1].max()) == 0.0, (c.name, route, k)
                exact += 1
        n += 1
    print(f"{n} launches of {len(CASES)} cases; {exact} outputs equal float64 bit for bit; worst emulation error / bound: "
          + ", ".join(f"{' '.join(k)} {v:.3f}" for k, v in sorted(worst.items())))
    assert exact > 0


@pytest.mark.parametrize("mut", wc.MUTANTS)
def test_bounds_reject_the_mutant(mut, inputs):
    """at least one case the mutant applies to lies outside its bound (the cheapest cases are tried first)"""
    if mut in wc.MUTANTS_UNSEEN:
        print(f"{mut}: listed as invisible -- {wc.MUTANTS_UNSEEN[mut]}")
        return
    todo = [(c, r, pl) for c, r, pl in _plans() if wc.applies(mut, c, pl)]
    assert todo, f"{mut}: applies to no case"
    todo.sort(key=lambda t: (t[0].p["Nw"] * t[0].p["Kw"] * (wc.row_range(t[0])[1] - wc.row_range(t[0])[0])))
    caught, tried = [], 0
    for c, route, pl in todo[:12]:
        inp = inputs[c.name]
        r = wc.compare(c, inp, wc.emulate(c, inp, route, mut), route)
        tried += 1
        if max(r.values()) > 1.0:
            caught.append((c.name, route, max(r.values())))
    print(f"{mut}: applies to {len(todo)} launches; {len(caught)} of the {tried} cheapest reject it"
          + (f", e.g. {caught[0][0]} on {caught[0][1]} at error / bound {caught[0][2]:.3g}" if caught else ""))
    assert caught, f"{mut}: no case sees it"


def test_refusal_texts_are_the_sources():
    src = ""
    for f in ("wgrad.hip", "gemm256.hip", "gemm.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            src += fh.read()
    for name, text in wc.REFUSAL_TEXT.items():
        assert text in src, (name, text)
