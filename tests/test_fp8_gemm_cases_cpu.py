"""CPU self-check of fp8_gemm_cases.py: the case table covers every `gemm_fp8(` call site of the package; the exact input
family is exact (its float64 reference round-trips through fp32, under every association of the epilogue's sum); the ACT8
byte interval stays sharp (the share of undecided roundings is bounded); and the comparison accepts the reference rounded
once and rejects each mutant -- the same result with one plausible kernel bug -- on every case the bug applies to."""
import dataclasses
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fp8_gemm_cases as fc  # noqa: E402

CASES = fc.cases(256)
BY_NAME = {c.name: c for c in CASES}
PKG = os.path.join(os.path.dirname(HERE), "adapt-image-models_amd")


@pytest.fixture(scope="module")
def world():
    """name -> (case, inputs, cache of the accumulations): built on first use, shared by the tests, never changed.  The
    peel cases are the same calls at 10 000 to 130 000 rows; every check here is per element, so they are held to it at
    their first 2 048 rows."""
    built = {}

    def get(name):
        if name not in built:
            case = BY_NAME[name]
            if name.endswith("/peel"):
                case = dataclasses.replace(case, spec=dataclasses.replace(case.spec, M=2048))
            built[name] = (case, fc.make_inputs(case), {})
        return built[name]
    return get


def test_every_call_site_has_a_form():
    sites = set()
    for fn in sorted(os.listdir(PKG)):
        if fn.endswith(".py") and fn != "ops.py":
            with open(os.path.join(PKG, fn)) as f:
                for i, line in enumerate(f, 1):
                    if re.search(r"\bgemm_fp8\(", line):
                        sites.add((fn, i))
    assert len(sites) >= 8, sites
    cited = set()
    for c in CASES:
        for fn, nums in re.findall(r"(\w+\.py):(\d+(?:,\d+)*)", c.site):
            cited.update((fn, int(n)) for n in nums.split(","))
    assert sites <= cited, f"gemm_fp8 call sites without a form in fp8_gemm_cases.forms: {sorted(sites - cited)}"
    assert cited <= sites, f"forms cite lines that hold no gemm_fp8 call: {sorted(cited - sites)}"


def test_case_table_and_route_plan():
    assert len(BY_NAME) == len(CASES)
    for geom in fc.GEOMS:
        for form in fc.PRODUCT_FORMS:
            fams = {c.family for c in CASES if c.form == form and f"/{geom}/" in c.name and not c.name.endswith("/peel")}
            assert fams == set(fc.FAMILIES), (form, geom)
    for c in CASES:
        s = c.spec
        assert c.site and s.M >= 1024 and s.N >= 64 and s.N % 8 == 0 and s.K % 16 == 0 and ((s.K + 127) // 128) % 2 == 0, c.name
        assert not s.vec or s.ntok >= 128, c.name
        if c.form.startswith("edge"):
            assert c.family == "exact" and s.ld_pad % 16 == 0 and s.ld_pad > 0, c.name
    assert BY_NAME["x2_f32/b16/M1182/exact"].spec.K % 128 == 64          # the last 128-byte K-step is half empty
    # route_plan against peel_rows: whole launches report every tile, peeled ones the tiles of the whole rounds
    for cus in (256, 304):
        peeled = []
        for c in fc.cases(cus):
            s = c.spec
            tn, tm = (s.N + 255) // 256, (s.M + 255) // 256
            assert fc.route_plan(c, "whole", cus) == ("256", tm * tn), c.name
            m0 = fc.peel_rows(s.M, s.N, cus)
            p = fc.route_plan(c, "peel", cus)
            if s.epi in ("f32", "act8") or s.K % 128 or not m0:
                assert p is None, c.name
            else:
                assert p == ("peel", (m0 // 256) * tn) and 0 < m0 < s.M, c.name
                peeled.append(c.name)
        assert len(peeled) == 4 and all(n.endswith("/peel") for n in peeled), (cus, peeled)
        assert {n.split("/")[0] for n in peeled} == set(fc.PEEL_FORMS) | {"peel_smallN"}


def test_q8_code_is_the_saturating_rne_cast():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(20000, generator=g).double() * s for s in (0.01, 1.0, 100.0, 1000.0)])
    grid = torch.arange(127, dtype=torch.uint8).view(fc.FP8).double()
    mids = (grid[:-1] + grid[1:]) / 2
    x = torch.cat([x, grid, -grid, mids, -mids, mids * (1 + 2.0 ** -20), mids * (1 - 2.0 ** -20)]).float().double()
    want = fc._code(x.clamp(-448, 448).float().to(fc.FP8).view(torch.uint8))          # the CPU cast rounds to nearest-even
    assert torch.equal(fc.q8_code(x), want)
    assert fc.q8_code(torch.tensor([449.0, -1e9, 448.0, 464.0])).tolist() == [126, -126, 126, 126]
    assert fc.code_bytes(torch.tensor([126, -126, 0, -1], dtype=torch.int32)).tolist() == [0x7E, 0xFE, 0, 0x81]


EXACT = [c.name for c in CASES if c.family == "exact"]


@pytest.mark.parametrize("name", EXACT)
def test_exact_family_is_exact(name, world):
    case, inp, cache = world(name)
    s = case.spec
    for k in ("A", "W"):
        v = inp[k].float()
        assert torch.equal(v, v.round()) and v.abs().max() <= (4 if k == "A" else 8)
    acc = cache.setdefault("acc", fc.accumulate(case, inp))[0]
    assert 4 * 8 * s.K < 2 ** 24                              # every partial sum of any subset of the products
    want, variants = fc.reassociations(case, inp, cache)
    assert torch.equal(want.float().double(), want), "the reference does not survive a round trip through fp32"
    for i, v in enumerate(variants):
        assert torch.equal(v, want), f"association {i} of the epilogue's sum is not exact in fp32"
    assert torch.equal(acc.float().double(), acc)
    if s.epi == "res16":
        assert torch.equal(inp["resid"].double(), inp["resid"].float().double())


ACT8 = [c.name for c in CASES if c.spec.epi == "act8"]


@pytest.mark.parametrize("name", ACT8)
def test_act8_interval_is_sharp(name, world):
    """a condition on the test itself: were most intervals two codes wide, nearly any wrong neighbour would pass"""
    case, inp, cache = world(name)
    y, e = fc.expected(case, inp, None, cache)
    lo, hi = fc.q8_code(y - e), fc.q8_code(y + e)
    share = float((lo != hi).double().mean())
    print(f"{name}: ambiguous share {share:.2e}, widest interval {int((hi - lo).max())} codes")
    if case.family == "exact":
        assert share <= fc.AMBIGUOUS_MAX, share
        # (two codes, -1 .. 1, only round the zeros of the saturation case's bias -1024 columns under a row factor of +-1)
        assert int((hi - lo).max()) <= (2 if case.spec.sat else 1)
    if case.spec.sat:
        s = case.spec
        tok = torch.arange(s.M) % s.ntok
        over = y.abs() > 448
        assert over.sum() >= 2 * (s.M // s.ntok) and (y[over] > 0).any() and (y[over] < 0).any()
        assert torch.equal(lo[over], hi[over]) and set(lo[over].abs().tolist()) == {126}
        quarter = (tok == 1)[:, None] & (inp["bias"] == 1024)[None, :]
        assert quarter.sum() >= 3 and set(lo[quarter].tolist()) == set(hi[quarter].tolist()) == {0x78}       # exactly 256


ALL = [c.name for c in CASES]


@pytest.mark.parametrize("name", ALL)
def test_reference_accepts_rounded_and_rejects_mutants(name, world):
    case, inp, cache = world(name)
    good = fc.check(case, inp, fc.simulate(case, inp, None, cache), cache)
    assert fc.passes(good), good
    muts = fc.mutants(case)
    assert {"ws_col+4", "ws_ignored"} <= set(muts)
    for mut in muts:
        bad = fc.check(case, inp, fc.simulate(case, inp, mut, cache), cache)
        assert not fc.passes(bad), (mut, bad)


def test_every_mutant_applies_somewhere():
    seen = {m for c in CASES for m in fc.mutants(c)}
    assert seen == set(fc.MUTANTS)
    for fam in fc.FAMILIES:
        assert {m for c in CASES if c.family == fam for m in fc.mutants(c)} >= set(fc.MUTANTS) - {"sat_nan", "nosat_wrap"}
