"""CPU self-check of tests/attn_cases.py: the bounds the GPU test holds the attention kernels to accept an emulation of the
kernels' arithmetic (float64 with their rounding points inserted) and reject each mutant -- the same emulation with one
plausible kernel bug.  The worst emulation error / bound per output is printed, so the slack is on record; on the tiny, the
N = 197 and the N = 257 item it lies between 0.1 and 0.9 for every output but lse (whose fp32 bound an exact exp does not
approach).  Also: the catalogue covers what it claims (every branch of the restated route rules has cases, the input
families have the logits they are named for).

The class-query kernels (kind `clsq`, emulate_clsq) are held to the same proof on their whole catalogue of 575 cases.  Worst
emulation error / bound, form a / form b: out 0.672, lse 0.011, dq 0.370 / 0.196, dk 0.860 / 0.507, dv 0.977 / 0.972 (dK and
dV of a key are single products rounded twice: the bound's two-rounding core).  The fp32 emulation of aim_tattn_fwd_infer's
fp8 form differs from the e4m3 cast of the float64 result on 0, 1, 1 and 10 bytes of the four pools (101 376 and 1 013 760
bytes each): at most 1e-5, against the GPU test's cap of 1e-3."""
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


# clsq mutant -> (the outputs of which at least one must leave its bound, the exact property that must fail, where it must show).
# No input family hides any of them; the geometries where one provably cannot show:
#   lse_transposed          BT = 1 or H = 1: element h BT + bt of a [BT, H] array is element bt H + h.  Elsewhere an item gets
#                           another item's lse, and p, dS and with them every gradient are off by the factor e^gap, gap the
#                           difference of the two.  The honest bound on dV is about 2 U8 |dV| (the roundings of p and of dV),
#                           so the mutant must leave it once e^gap - 1 > 4 U8 = 2^-6; it is required to show where some
#                           item's gap exceeds 2^-5: 516 of the 561 cases with BT, H > 1 (the others have lse that nearly coincide, near log N)
#   do_full_stride          BT = 1 or N = 1: row bt N is row bt.  Elsewhere a frame reads past the compact dO, into the NaN
#                           around a guarded input (frame 0 always reads its own row)
#   delta_next_head         H = 1: the next head is the same head
#   dk_no_eighth            N = 1: p = 1 and delta = dO . O = dP, so dS and with it dK is zero up to the rounding of O, inside
#                           the bound; zero_do with H = 1: dO, and so dK, is zero
#   keys_past_64_unwritten  N <= 64: the write loop's first trip covers every key
#   other_dq_untouched      N = 1: there is no other row
#   out_row_stride          BT = 1 or N = 1: row bt N is row bt.  `out` must show it everywhere else (the frames above 0 keep
#                           their NaN); the spare elements behind `out` see it only where the stray row lands inside them
#                           (bt N >= BT and (bt N + 1) D inside the buffer: N = 2 .. 7 of the sweep and 5x2/BT4), elsewhere it
#                           lies past the end of the whole buffer
CLSQ_DETECT = {
    "lse_transposed": (("dq", "dk", "dv"), None, lambda c, e: c.BT > 1 and c.H > 1 and _lse_gap(c, e) > 2.0 ** -5),
    "do_full_stride": (("dq", "dk", "dv"), "finite", lambda c, e: c.BT > 1 and c.N > 1),
    "delta_next_head": (("dq", "dk"), None, lambda c, e: c.H > 1),
    "dk_no_eighth": (("dk",), None, lambda c, e: c.N > 1 and not (c.family == "zero_do" and c.H == 1)),
    "keys_past_64_unwritten": (("dk", "dv"), "finite", lambda c, e: c.N > 64),
    "other_dq_untouched": ((), "other_dq_zero", lambda c, e: c.N > 1),
    "out_row_stride": (("out",), None, lambda c, e: c.BT > 1 and c.N > 1),
}


def _lse_gap(c, exp):
    lse = exp["lse"][0]
    return float((lse - lse.reshape(-1)[torch.arange(c.H)[None, :] * c.BT + torch.arange(c.BT)[:, None]]).abs().max())


def _stray_row_in_spare(c):
    D = c.H * 64
    size = c.BT * D + 8 + 3 * (c.BT * D + 8)
    return any(bt * c.N >= c.BT and (bt * c.N + 1) * D <= size for bt in range(1, c.BT))


def test_clsq_bounds_accept_the_emulation_and_reject_every_mutant():
    """the whole clsq catalogue: the emulation of aim_attn_fwd_cls / aim_attn_bwd_cls is inside the bounds in both backward
    forms and has the exact properties; each mutant is outside on the outputs named for it wherever it can show"""
    assert set(CLSQ_DETECT) == set(ac.CLSQ_MUTANTS)
    cs = [c for c in ac.length_cases() if c.kind == "clsq"]
    worst, bad, shown, spare_seen = {}, [], {m: 0 for m in ac.CLSQ_MUTANTS}, 0
    for c in cs:
        inp = ac.clsq_inputs(c)
        exp = ac.clsq_expected(c, inp)
        for form, own in (("a", False), ("b", True)):
            got = ac.emulate_clsq(c, inp, own=own, exp=exp)
            r = ac.compare_clsq(c, exp, got, form)
            assert set(r) == {"out", "lse", "dq", "dk", "dv"}
            for k, v in r.items():
                if v > worst.get((k, form), (0.0, ""))[0]:
                    worst[(k, form)] = (v, c.name)
                if not v <= 1.0:
                    bad.append(f"{c.name} form {form} {k}: emulation error / bound = {v:.3g}")
            ex = ac.clsq_exact(c, got)
            if not (all(ex.values()) and got["spare_intact"] and ("zero_head" in ex) == (c.family == "zero_do")):
                bad.append(f"{c.name} form {form}: exact properties {ex}")
        for mut, (outs, flag, where) in CLSQ_DETECT.items():
            got = ac.emulate_clsq(c, inp, mut, exp=exp)
            r = ac.compare_clsq(c, exp, got, "a")
            ex = ac.clsq_exact(c, got)
            seen = (not outs or max(r[k] for k in outs) > 1.0) and (flag is None or not ex[flag])
            if where(c, exp):
                shown[mut] += 1
                if not seen:
                    bad.append(f"{c.name}: mutant {mut} not rejected: {r} {ex}")
            if mut == "out_row_stride":
                spare_seen += not got["spare_intact"]
                if got["spare_intact"] == (where(c, exp) and _stray_row_in_spare(c)):
                    bad.append(f"{c.name}: mutant {mut}: spare elements intact = {got['spare_intact']}")
            elif not got["spare_intact"]:
                bad.append(f"{c.name}: mutant {mut} touched the spare elements")
            if mut not in ("out_row_stride",) and max(r["out"], r["lse"]) > 1.0:      # a backward defect leaves the forward alone
                bad.append(f"{c.name}: mutant {mut} changed the forward")
    print(f"clsq: {len(cs)} cases, worst emulation error / bound " +
          ", ".join(f"{k}@{f} {v:.3f} ({n})" for (k, f), (v, n) in sorted(worst.items())))
    print("clsq: cases on which each mutant had to show: " + ", ".join(f"{m} {n}" for m, n in shown.items()) +
          f"; out_row_stride seen by the spare elements on {spare_seen}")
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:40])
    assert all(n >= 0.7 * len(cs) for m, n in shown.items() if m != "keys_past_64_unwritten"), shown
    assert shown["keys_past_64_unwritten"] == sum(c.N > 64 for c in cs) and spare_seen >= 7


SWEEP_T = (1, 2, 16, 17, 31, 32)             # both ends, and both sides of tattn's switch from 4 to 2 waves per workgroup


@pytest.mark.parametrize("kind,B,T,N,H", [("cls", 2, 8, 5, 2), ("tattn", 1, 31, 3, 2), ("cls", 3, 1, 4, 1)] +
                         [(kind, B, T, N, H) for kind in ("cls", "tattn") for B, N, H in ac.SWEEP_GEOMS for T in SWEEP_T])
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
    if T > 1 and H > 1:                         # (H = 1: the next head is the same head)
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
    assert {(c.B, c.T, c.N, c.H) for c in cs if c.kind == "cls" and not c.sweep} == set(ac.SMALL_SHAPES)
    assert {(c.B, c.T, c.N, c.H) for c in cs if c.kind == "tattn" and not c.sweep} == set(ac.SMALL_SHAPES)
    # the routes run what they ran before; the length cases are the rest and have names of their own
    assert cs == ac.route_cases() + ac.length_cases() and len({c.name for c in cs}) == len(cs)
    assert not [c for c in ac.route_cases() if c.kind == "clsq" or c.sweep]
    # clsq: every N, every family on every 7th; all six forward templates <2|4|14|18, false, true> in both masking forms;
    # both parities of the backward's 32-key block count (its key-tile padding nkt = 2 ((N + 31) // 32)) and every count;
    # one, two, ... five trips of its write loop (64 keys per trip)
    clsq = [c for c in cs if c.kind == "clsq"]
    sweep = [c for c in clsq if "/sweep/" in c.name]
    assert sorted(c.N for c in sweep if c.family == "unit") == list(range(1, ac.NMAX + 1))
    assert all((c.BT, c.H) == (ac.SWEEP_BT, ac.SWEEP_H) for c in sweep)
    for fam in ac.FAMILIES:
        assert {c.N for c in sweep if c.family == fam} >= {n for n in range(1, ac.NMAX + 1) if n % ac.FAMILY_STRIDE == 1}
        assert {(c.BT, c.N, c.H) for c in clsq if c.family == fam and c not in sweep} == set(ac.CLSQ_SHAPES)
        ns = {c.N for c in clsq if c.family == fam}
        assert {ac.fwd_plan(n) for n in ns} == {(2, 0), (4, 2), (14, 0), (14, 12), (18, 0), (18, 16)}
        assert {(n + 31) // 32 for n in ns} == set(range(1, 10)) and {(n + 63) // 64 for n in ns} == {1, 2, 3, 4, 5}
    assert {1, 32, 33, 64, 65, 224, 225, 288} <= {c.N for c in sweep}
    # cls / tattn: every T at both geometries and both families
    for kind in ("cls", "tattn"):
        for fam in ("unit", "peaked"):
            got = sorted((c.B, c.N, c.H, c.T) for c in cs if c.kind == kind and c.sweep and c.family == fam)
            assert got == sorted((B, N, H, T) for B, N, H in ac.SWEEP_GEOMS for T in range(1, ac.TMAX + 1))
    # tattn (and its inference forms): 4 waves per workgroup up to T = 16, 2 above; each wave count has cases whose item
    # count B N H is not a multiple of it: (1, 3, 1) at both, (2, 5, 3) at 4 waves.  cls_attn launches one 64-thread
    # workgroup per (b, h) at every T (csrc/cls_attn.hip): one wave count, no partial workgroup to cover
    assert {ac.tattn_wpb(T) for T in range(1, 33)} == {4, 2} and ac.tattn_wpb(16) == 4 and ac.tattn_wpb(17) == 2
    partial = {(ac.tattn_wpb(c.T), (c.B, c.N, c.H)) for c in cs if c.kind == "tattn" and c.sweep and (c.B * c.N * c.H) % ac.tattn_wpb(c.T)}
    assert partial == {(4, (1, 3, 1)), (4, (2, 5, 3)), (2, (1, 3, 1))}
    assert set(ac.SAT_T) == {17, 32}


def test_infer_emulation_stays_under_a_third_of_the_neighbour_cap():
    """aim_tattn_fwd_infer's fp8 form: per pool (all T of one geometry and family), the share of bytes on which an fp32
    emulation of the kernel's arithmetic differs from the e4m3 cast of the float64 result is under a third of the cap the GPU
    test applies, and no byte is farther than the neighbouring code"""
    pools = {}
    for c in ac.length_cases():
        if c.kind != "tattn":
            continue
        qkv = ac.make_inputs(c)["qkv"]
        emu = ac.tattn_infer_emulate(qkv, c.B, c.T, c.N, c.H)
        want = ac.e4m3_bytes(ac.tattn_ref64(qkv, c.B, c.T, c.N, c.H))
        step = (ac.e4m3_code(emu) - ac.e4m3_code(want)).abs()
        assert int(step.max()) <= 1, c.name
        n, d = pools.get(ac.infer_pool(c), (0, 0))
        pools[ac.infer_pool(c)] = (n + emu.numel(), d + int((step == 1).sum()))
    assert len(pools) == 4
    for pool, (n, d) in pools.items():
        print(f"infer emulation {pool}: {n} bytes, {d} neighbours ({d / n:.2e})")
        assert n * ac.INFER_CAP >= 100 and d / n <= ac.INFER_CAP / 3, (pool, n, d)
    # the saturating input really exceeds the range, with either sign
    c = next(c for c in ac.length_cases() if c.kind == "tattn" and c.T == 17 and c.family == "unit")
    qkv, want = ac.saturating_qkv(c)
    assert torch.equal(ac.e4m3_bytes(ac.tattn_ref64(qkv, c.B, c.T, c.N, c.H)), want) and set(want.unique().tolist()) == {0x7E, 0xFE}


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
