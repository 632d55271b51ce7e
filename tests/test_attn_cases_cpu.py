"""CPU self-check of tests/attn_cases.py: the bounds the GPU test holds the attention kernels to accept an emulation of the
kernels' arithmetic (float64 with their rounding points inserted) and reject each mutant -- the same emulation with one
plausible kernel bug.  The worst emulation error / bound per output is printed, so the slack is on record; on the tiny, the
N = 197 and the N = 257 item it lies between 0.1 and 0.9 for every output but lse (whose fp32 bound an exact exp does not
approach).  Also: the catalogue covers what it claims (every branch of the restated route rules has cases, the input
families have the logits they are named for)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402

SHAPES = ((2, 5, 2), (1, 197, 2), (1, 257, 2))          # BT, N, H: the tiny geometry, one item pair of each product shape
SPREAD = [(bt, n, h, fam) for bt, n, h in SHAPES for fam in ac.FAMILIES]


def _case(BT, N, H, fam):
    return ac.Case(f"cpu/{N}x{H}/{fam}", "spatial", BT, N, H, fam, seed=31 + N)


@pytest.mark.parametrize("BT,N,H,fam", SPREAD)
def test_bounds_accept_the_emulation(BT, N, H, fam):
    case = _case(BT, N, H, fam)
    inp = ac.make_inputs(case)
    for form, own in (("a", False), ("b", True)):
        r = ac.compare_spatial(case, inp, ac.emulate(case, inp, own=own), form)
        print(f"{case.name} form {form}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
        assert set(r) == {"out", "out8", "lse", "dq", "dk", "dv"}
        assert max(r.values()) <= 1.0, r


# mutant -> the outputs that must see it, and the families where it must be seen (None: all)
DETECT = {# a zero logit weighs exp(-lse): nothing where the row's largest logit is 16 or more (cls_sink, peaked), so the mutant
          # is listed as not detectable there; everywhere else lse must see it
          "pad_key": (("lse", "out"), ("unit", "diag", "neg40", "neg100", "zero_do")), # (the last key weighs nothing under a 16-logit sink, and at neg100 the fp32 score error of |q| = 104 rows is a third
          # of one key's 1 / N share)
          "last_key_last_tile": (("lse", "out"), ("unit", "peaked", "diag", "neg40", "zero_do")),
          # on a flat softmax sum p |v| is many times |out|: a one-ulp scale error is inside the honest bound there and is
          # listed as not detectable; on peaked rows (peaked, diag) the two are close and it must show
          "out_scale": (("out",), ("peaked", "diag")),
          "no_delta": (("dq", "dk"), None), "delta_next_head": (("dq", "dk"), None),
          "lse_next_head": (("dq", "dk", "dv"), None), "lse_next_query": (("dq", "dk", "dv"), None),
          "dkv_next_item": (("dk", "dv"), None), # (under a one-hot softmax dS, and so dQ, is ~ e^-12 of the bound that the rounding of `out` alone puts on delta)
          "dq_no_eighth": (("dq",), ("unit", "peaked", "diag", "neg40", "neg100", "zero_do")), "leftover_dq_zero": (("dq",), ("unit", "peaked", "diag", "neg40", "neg100", "zero_do"))}


@pytest.mark.parametrize("BT,N,H,fam", SPREAD)
def test_bounds_reject_every_mutant(BT, N, H, fam):
    case = _case(BT, N, H, fam)
    inp = ac.make_inputs(case)
    for mut in ac.FWD_MUTANTS + ac.BWD_MUTANTS:
        outs, fams = DETECT[mut]
        if fams is not None and fam not in fams:
            continue
        if mut == "leftover_dq_zero" and not 1 <= N % 64 <= 16:
            continue
        if mut == "pad_key" and N % 16 == 0:
            continue
        r = ac.compare_spatial(case, inp, ac.emulate(case, inp, mut), "a")
        assert max(r[k] for k in outs) > 1.0, (mut, r)
        if mut in ac.FWD_MUTANTS:                      # a forward defect leaves the backward of form (a) alone
            assert max(r[k] for k in ("dq", "dk", "dv")) <= 1.0, (mut, r)


def test_zero_do_head_is_exactly_zero_in_the_emulation():
    case = _case(2, 5, 2, "zero_do")
    inp = ac.make_inputs(case)
    got = ac.emulate(case, inp)
    assert all((got[k][:, 1] == 0).all() and (got[k][:, 0] != 0).any() for k in ("dq", "dk", "dv"))


@pytest.mark.parametrize("kind,B,T,N,H", [("cls", 2, 8, 5, 2), ("tattn", 1, 31, 3, 2), ("cls", 3, 1, 4, 1)])
def test_small_kernels_bounds(kind, B, T, N, H):
    """cls_attn / tattn: an fp32 emulation is inside the bounds; probabilities of the next head, a missing 1/8 on dq and
    dk / dv of the next item are outside"""
    case = ac.Case(f"cpu/{kind}", kind, B * T, N, H, "unit", seed=5, B=B, T=T)
    inp = ac.make_inputs(case)
    inp["do_small"] = torch.randn((B * T, H * 64), generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    q, k, v, do = ac.small_rows(case, inp)
    ref = ac.small_ref(q, k, v, do)
    f = lambda t: t.float().double()
    z = f(q @ k.transpose(-1, -2)) / 8
    p = f(torch.softmax(z, dim=-1))
    dP = f(do @ v.transpose(-1, -2))
    dS = f(p * (dP - f((p * dP).sum(-1, keepdim=True))) / 8)

    def outs(p_, dS_, scale=1.0):
        return {"probs": p_, "out": f(p_ @ v).to(torch.bfloat16), "dq": f(dS_ @ k * scale).to(torch.bfloat16),
                "dk": f(dS_.transpose(-1, -2) @ q).to(torch.bfloat16), "dv": f(p_.transpose(-1, -2) @ do).to(torch.bfloat16)}

    def worst(got):
        return {n: ac.ratio(got[n], ref[n][0], ref[n][1] if n == "probs" else ac.U8 * ref[n][0].abs() + (1 + ac.U8) * ref[n][1])
                for n in got if n != "out"} | {"out": ac.ratio(got["out"], *ref["out"])}

    good = worst(outs(p, dS))
    print(kind, good)
    assert max(good.values()) <= 1.0, good
    if T > 1:                                   # (T = 1: p = 1 and every gradient but dv is zero)
        assert worst(outs(p, dS, 8.0))["dq"] > 1.0
        bad = worst(outs(p.roll(1, dims=-3), dS))
        assert bad["probs"] > 1.0 and bad["out"] > 1.0 and bad["dv"] > 1.0
        assert worst(outs(p, dS.roll(1, dims=-3)))["dk"] > 1.0


def test_catalogue_covers_every_branch():
    cs = ac.cases()
    spatial = [c for c in cs if c.kind == "spatial" and not c.poison]
    ns = {c.N for c in spatial}
    assert ns == set(range(1, ac.NMAX + 1))
    # forward: every template of aim_attn_fwd, masked on every tile and on the last two only
    assert {ac.fwd_plan(n) for n in ns} == {(2, 0), (4, 2), (14, 0), (14, 12), (18, 0), (18, 16)}
    # backward: per route, every branch of the selection rule that the route can take, for every family
    want = {"default": {("two", False), ("pipe", False), ("pipe", True)}, "xt0": {("two", False), ("pipe", False)},
            "two": {("two", False)}}
    for route in ac.ROUTES:
        for fam in ac.FAMILIES:
            plans = {ac.bwd_plan(c.N, route) for c in spatial if c.family == fam}
            assert plans == want.get(route, want["default"]), (route, fam, plans)
    # the number of 32-key blocks, N % 32 == 0 and != 0, and the left-over form at both of its ends
    pipe = {c.N for c in spatial if ac.bwd_plan(c.N, "default")[0] == "pipe"}
    assert {(n + 31) // 32 for n in pipe} == {3, 4, 5, 6, 7}
    assert {129, 144, 145, 193, 208, 209, 224, 65, 128, 192} <= pipe and 225 not in pipe and 64 not in pipe
    # grid routes: one workgroup walks every item; three walk unequal shares; the product launch exceeds the reserve rule
    items = 9 * 12
    assert ac.pipe_grid(items, 256, "grid1") == 1 and ac.pipe_grid(items, 256, "grid3") == 3 and items % 3 == 0
    assert any((c.BT * c.H) % 3 for c in spatial if c.N in pipe)
    assert ac.pipe_grid(2400 * 12, 256, "default") == 224 and ac.pipe_grid(2400 * 12, 256, "reserve0") == 256
    # isolation cases and the small kernels' geometries
    assert sum(c.poison for c in cs) == 3 and sum(c.alone for c in cs) == 2
    assert {(c.B, c.T, c.N, c.H) for c in cs if c.kind == "cls"} == set(ac.SMALL_SHAPES)
    assert {(c.B, c.T, c.N, c.H) for c in cs if c.kind == "tattn"} == set(ac.SMALL_SHAPES)


@pytest.mark.parametrize("N,H", [(197, 12), (257, 16), (71, 2)])
def test_families_have_the_logits_they_are_named_for(N, H):
    def logits(fam):
        case = ac.Case("x", "spatial", 1, N, H, fam, seed=3)
        q, k, v = ac.split(ac.make_inputs(case)["qkv"], 1, N, H, 3)
        z = q @ k.transpose(-1, -2) / 8
        return z, torch.logsumexp(z, dim=-1)

    z, _ = logits("unit")
    assert z.abs().max() < 8
    z, _ = logits("peaked")
    assert z.abs().max() > 20
    z, _ = logits("cls_sink")
    assert ((z[..., 0] - z[..., 1:].amax(dim=-1)) >= 10).all()
    z, _ = logits("diag")
    assert (z.argmax(dim=-1) == torch.arange(N)).all() and (torch.softmax(z, -1).diagonal(dim1=-2, dim2=-1) > 0.5).float().mean() > 0.9
    rows = ac.sink_rows(N)
    z, lse = logits("neg40")
    assert (z[..., rows, :] < -30).all() and (z[..., rows, :] > -50).all() and (lse[..., rows] > -45).all()
    z, lse = logits("neg100")
    assert (lse[..., rows] < -90).all() and (lse[..., ~rows].abs() < 10).all()
