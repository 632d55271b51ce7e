"""Every fp8 GEMM call form (tests/fp8_gemm_cases.py) on both routes of `aim_gemm_fp8`, per element against float64.

One child process per route, started one after another (AIM_GEMM_PEEL is read once per process): the persistent 256 x 256
block-scaled-MFMA kernel alone (`whole`, AIM_GEMM_PEEL=0), and the default environment (`peel`), where a thin last tile
round goes to the fp8 form of the 64 x 64 kernel.  Each child reports, per case and output: the number of elements unequal
to the exact reference (exact family, BF16 / F32 / RES16) or the worst error as a fraction of the derived bound (random
family); for ACT8 the bytes outside the interval of fp8_gemm_cases.expected and the NaN codes; a hash; whether the canary
round the output survived; and how many tiles the persistent kernel recorded in its probe buffer.  The first child that
fails ends the fixture: nothing more is started on the GPU.  `test_refusals` calls the C entry point directly with each
argument set it must turn down.

Measured on MI355X (256 CUs): 89 cases on `whole`, 4 on `peel` (504 to 512 of 513 to 516 tiles on the persistent kernel).
Exact family: 0 unequal elements for BF16, F32 and RES16 on both routes and at reserve_cus 0, 16 and 64, 0 ACT8 bytes
outside their interval, 0 NaN codes, every canary intact, peeled == whole; ambiguous share of the ACT8 cases 2.1e-4 to
8.0e-4 (cat1: 6.9e-4 at ViT-B/16, 8.0e-4 at ViT-L/14; the bound is 2e-3).  Random family, worst error / bound: BF16 0.91,
F32 0.06, RES16 0.95 (the bf16 outputs end in one bf16 rounding of an fp32 value); ACT8 0 bytes outside the interval, whose
ends differ for 42 % (ViT-B/16) and 53 % (ViT-L/14) of the outputs -- which is why the exact family exists.  Child times:
`whole` 4.6 s, `peel` 3.7 s (2.1 s and 1.2 s of them in the cases); CHILD_TIMEOUT is about five times the slower one."""
import ctypes
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fp8_gemm_cases as fc  # noqa: E402

CHILD_TIMEOUT = 30


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    out = {}
    for route in fc.ROUTES:
        env = {k: v for k, v in os.environ.items() if k not in fc.ROUTE_VARS}
        env.update(fc.ROUTE_ENV[route])
        path = str(tmp_path_factory.mktemp("fp8_routes") / f"{route}.json")
        t0 = time.time()
        p = subprocess.run([sys.executable, os.path.join(HERE, "fp8_gemm_cases.py"), route, path], env=env,
                           timeout=CHILD_TIMEOUT, capture_output=True, text=True)
        if p.returncode != 0:        # stop at the first failing child: nothing more is started on the GPU
            pytest.fail(f"route {route}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[route] = json.load(f)
        out[route]["child_seconds"] = time.time() - t0
    return out


def test_every_case_on_every_route_it_takes(routes):
    bad = []
    cus = routes["whole"]["cus"]
    for route, res in routes.items():
        want = [c.name for c in fc.cases(cus) if fc.route_plan(c, route, cus) is not None]
        assert list(res["cases"]) == want and want, f"route {route} did not run every case it takes"
        worst, ambiguous = {}, 0.0
        for name, rec in res["cases"].items():
            for k, fig in rec["checks"].items():
                if "ratio" in fig:
                    worst[rec["epi"]] = max(worst.get(rec["epi"], 0.0), fig["ratio"])
                if rec["family"] == "exact":
                    ambiguous = max(ambiguous, fig.get("ambiguous", 0.0))
                if not fc.passes(fig):
                    bad.append(f"{route} {name} {k}: {fig}")
                if not rec["pad"][k]:
                    bad.append(f"{route} {name} {k}: write outside the output (canary changed)")
        print(f"route {route}: {len(want)} cases, child {res['child_seconds']:.1f} s ({res['seconds']:.1f} s in the cases); "
              f"random family, worst error / bound { {k: round(v, 3) for k, v in worst.items()} }; "
              f"exact family, largest ambiguous share {ambiguous:.2e}")
    assert not bad, "\n".join(bad[:40])


def test_exact_family_has_no_unequal_element(routes):
    """stated apart from the bounds: BF16, F32 and RES16 on the exact family equal the reference on both routes, and every
    ACT8 byte lies in its interval, with the ambiguous share the CPU test bounds"""
    n = 0
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            if rec["family"] != "exact":
                continue
            for k, fig in rec["checks"].items():
                n += 1
                if rec["epi"] == "act8":
                    assert fig["outside"] == 0 and fig["nan_codes"] == 0, (route, name, fig)
                    assert fig["ambiguous"] <= fc.AMBIGUOUS_MAX, (route, name, fig)
                else:
                    assert fig == {"unequal": 0}, (route, name, k, fig)
    assert n > 80


def test_bit_identity_where_the_design_claims_it(routes):
    bad = []
    n_rc = 0
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            h = rec["hash"]
            for k in h:
                if "@rc" in k:
                    n_rc += 1
                    if h[k] != h["out"]:
                        bad.append(f"{route} {name}: reserve_cus {k} changed the bits")
    # the peeled launch writes what the whole launch writes (both already equal the exact reference)
    whole, peel = routes["whole"]["cases"], routes["peel"]["cases"]
    for name, rec in peel.items():
        assert rec["kernel"] == "peel" and whole[name]["kernel"] == "256" and rec["family"] == "exact", name
        if rec["hash"]["out"] != whole[name]["hash"]["out"]:
            bad.append(f"peel != whole: {name}")
    forms = {name.split("/")[0] for name in peel}
    assert forms >= set(fc.PEEL_FORMS) | {"peel_smallN"} and n_rc >= 8, (forms, n_rc)
    assert not bad, "\n".join(bad[:40])


def test_probe_count_matches_the_plan(routes):
    """the route really ran: the persistent kernel's probe holds one record per tile it processed, the 64 x 64 kernel
    leaves it alone"""
    bad = []
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            if rec["probe_written"] != rec["probe_expected"]:
                bad.append(f"{route} {name}: kernel {rec['kernel']} expected {rec['probe_expected']} probe records, "
                           f"got {rec['probe_written']}")
        if route == "peel":
            whole = routes["whole"]["cases"]
            assert all(rec["probe_expected"] < whole[name]["probe_expected"] for name, rec in res["cases"].items())
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------ refusals ----------------------------------------------
def test_refusals():
    """Each argument set `capi.hip::aim_gemm_fp8` must turn down returns non-zero before any launch: `aim_last_error` names
    the reason, the canary-filled output is untouched, and a valid call afterwards still gives the exact result."""
    sys.path.insert(0, os.path.dirname(HERE))
    from aim_amd import ops
    from aim_amd.lib import GemmArgs, load_library
    lib = load_library()
    dev = torch.device("cuda")
    M, N, K = 1024, 64, 256
    case = fc.Case("refusals", "refusals", "capi.hip::aim_gemm_fp8",
                   fc.Spec("res16", M, N, K, 128, bias=True, resid=True, af=True, vec="frame", bt=True), "exact", 77)
    inp = {k: v.to(dev) for k, v in fc.make_inputs(case).items()}
    resid32 = inp["resid"].float()
    ref, _ = fc.expected(case, inp)
    want = ref.float().to(torch.bfloat16)
    canary = torch.full((M + 8, N + 8), fc.CANARY, dtype=torch.uint8, device=dev).repeat(1, 4)       # room for fp32 rows
    stream = torch.cuda.current_stream().cuda_stream

    def args(out, **over):
        g = GemmArgs()
        g.A, g.W, g.lda, g.ldw = inp["A"].data_ptr(), inp["W"].data_ptr(), K, K
        g.M, g.N, g.K = M, N, K
        g.wscale, g.bias = inp["wscale"].data_ptr(), inp["bias"].data_ptr()
        g.out, g.ldo, g.scale = out.data_ptr(), N + 8, 1.0
        for k, v in over.items():
            setattr(g, k, v.data_ptr() if torch.is_tensor(v) else v)
        return g

    rows = dict(af=inp["af"], vec=inp["vec"], ldv=N, bt=inp["bt"], ntok=128)
    r16 = dict(resid=inp["resid"], ldr=N, **rows)
    B, F, A8, R = ops.EPI_BF16, ops.EPI_F32, ops.EPI_ACT8, ops.EPI_RES16
    refused = [
        ("M = 1023", B, dict(M=1023), "large-M"),
        ("N = 56", B, dict(N=56), "large-M"),
        ("K = 24", B, dict(K=24), "multiples of 16"),
        ("K = 128: ceil(K / 128) odd", B, dict(K=128), "must be even"),
        ("lda % 16 != 0", B, dict(K=240, lda=248), "multiples of 16"),
        ("N % 8 != 0", B, dict(N=68), "multiples of 8"),
        ("n_split % 8 != 0", A8, dict(n_split=4), "multiples of 8"),
        ("n_split > N", A8, dict(n_split=N + 8), "n_split must be in [0, N]"),
        ("ldo % 8 != 0", B, dict(ldo=N + 4), "multiples of 8"),
        ("xrow set", B, dict(xrow=inp["bias"]), "xrow"),
        ("row0 != 0", B, dict(row0=256), "row0"),
        ("RES16 without resid", R, dict(rows), "RES16 needs a bf16 residual"),
        ("RES16: vec with ntok = 127", R, dict(r16, ntok=127), "ntok >= 128 with vec"),
        ("F32: vec with ntok = 127", F, dict(rows, resid=resid32, ldr=N, ntok=127), "F32 epilogue"),
        ("af without ntok", B, dict(af=inp["af"]), "ntok required"),
        ("epilogue ACT", ops.EPI_ACT, {}, "unsupported epilogue"),
        ("epilogue DACT", ops.EPI_DACT, {}, "unsupported epilogue"),
        ("epilogue EXPSUM", ops.EPI_EXPSUM, {}, "unsupported epilogue"),
    ]
    for what, epi, over, reason in refused:
        out = canary.clone()
        rc = lib.aim_gemm_fp8(ctypes.byref(args(out, **over)), epi, stream)
        torch.cuda.synchronize()
        msg = lib.aim_last_error().decode()
        assert rc != 0, f"{what}: accepted"
        assert reason in msg and "gemm_fp8" in msg, f"{what}: aim_last_error says {msg!r}"
        assert torch.equal(out, canary), f"{what}: the output was written"
        # and the library is none the worse for it
        buf = torch.full((M + 3, N + 8), float("nan"), dtype=torch.bfloat16, device=dev)
        rc = lib.aim_gemm_fp8(ctypes.byref(args(buf, **r16)), R, stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.aim_last_error().decode()
        assert torch.equal(buf[:M, :N], want), f"after {what}: a valid call no longer gives the exact result"
        assert torch.isnan(buf[M:]).all() and torch.isnan(buf[:, N:]).all()
