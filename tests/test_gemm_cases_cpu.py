"""CPU self-check of the float64 GEMM references in gemm_cases.py: for every call form, the comparison accepts the exact
reference rounded once to the output dtype, and rejects each mutant -- the same result with one plausible kernel bug (split
boundary 4 columns off, a neighbour token's DropPath factor, the next frame's 1 - lamda, `vec` read with ldv = N instead of
0, aux_grad semantics swapped, rs_bias_only ignored), also rounded.  So the bounds the GPU test holds the kernels to are
tight enough to see those bugs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

SELF_CHECK = [(name, geom, frames) for geom, frames in (("tiny", 8), ("b16", 2)) for name in
              gc.TOKEN_FORMS + gc.CLS_FORMS + gc.FP8_FORMS]


def _case(name, geom, frames):
    ntok = gc.GEOMS[geom][2]
    spec, site, opt = gc.forms(geom, frames * ntok)[name]
    return gc.Case(f"{name}/{geom}", name, site, spec, seed=7, **opt)


def test_every_form_has_a_site_and_runs_somewhere():
    cs = gc.cases(256)
    assert {c.form for c in cs} == set(gc.TOKEN_FORMS + gc.CLS_FORMS + gc.FP8_FORMS + ("expsum",))
    for c in cs:
        assert c.site and any(gc.route_plan(c, r, 256) for r in gc.ROUTES), c.name
    # every M >= 1024 bf16 form reaches all three kernels; every peel case is peeled
    for c in cs:
        if c.spec.M >= 1024 and c.spec.N >= 64 and c.spec.epi in ("bf16", "f32", "act", "dact") and c.spec.K % 64 == 0:
            kern = {gc.route_plan(c, r, 256)[0] for r in ("256", "128", "small")}
            if c.spec.epi != "f32" or not c.spec.vec or c.spec.ntok >= 128:
                assert kern == {"256", "128", "small"}, c.name
        if c.name.endswith("/peel"):
            assert gc.route_plan(c, "peel", 256)[0] == "peel", c.name


@pytest.mark.parametrize("name,geom,frames", SELF_CHECK)
def test_reference_accepts_rounded_and_rejects_mutants(name, geom, frames):
    case = _case(name, geom, frames)
    torch.manual_seed(0)
    inp = gc.make_inputs(case)
    good = gc.compare(case, inp, gc.simulate(case, inp))
    assert good and max(good.values()) <= 1.0, good
    muts = gc.mutants(case.spec)
    if case.spec.epi in ("act", "dact") or case.spec.ntok:
        assert muts or not (case.spec.at or case.spec.af or case.spec.vec), name
    for mut in muts:
        bad = gc.compare(case, inp, gc.simulate(case, inp, mut))
        assert max(bad.values()) > 1.0, (mut, bad)


def test_act_inputs_span_both_activations():
    """pre-activations over about [-4, 4]: there QuickGELU and GELU differ by far more than the bound"""
    case = _case("mlp_act", "b16", 2)
    inp = gc.make_inputs(case)
    pre = gc.expected(case, inp)["pre"][0]
    assert pre.min() < -3.5 and pre.max() > 3.5
    x = pre.flatten()
    assert ((gc.qgelu(x) - gc.gelu(x)).abs() > 8 * gc.U8 * gc.gelu(x).abs()).sum() > 100
