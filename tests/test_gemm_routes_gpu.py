"""Every GEMM call form of the product (tests/gemm_cases.py) on every kernel route it can take, against float64.

One child process per route, started one after another (the route switches are read once per process): the persistent
256 x 256 kernel (AIM_GEMM_PEEL=0), the same with its thin last tile round peeled onto the 64 x 64 kernel (default), the
128 x 128 kernel, the 64 x 64 kernel, and the 128 x 128 EXPSUM layout (AIM_EXPSUM_256=0).  Each child reports, per case,
the worst error as a fraction of its derived bound (gemm_cases.expected), a hash per output, whether the NaN padding around
every output survived, and how many tiles the persistent kernel recorded in its probe buffer.  Bit-identity is asserted
where the design claims it: peeled == whole launch, 64 x 64 == 256 x 256 (BF16 / F32), reserve_cus 0 == 16 == 64,
aux_frag == row-major aux, aux_grad's `post` == plain `post`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_cases as gc  # noqa: E402


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    out = {}
    for route in gc.ROUTES:
        env = {k: v for k, v in os.environ.items() if k not in gc.ROUTE_VARS}
        env.update(gc.ROUTE_ENV[route])
        path = str(tmp_path_factory.mktemp("routes") / f"{route}.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "gemm_cases.py"), route, path], env=env, timeout=300,
                           capture_output=True, text=True)
        if p.returncode != 0:        # stop at the first failing child: nothing more is started on the GPU
            pytest.fail(f"route {route}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[route] = json.load(f)
    return out


def test_every_case_matches_fp64_on_every_route(routes):
    bad = []
    for route, res in routes.items():
        worst, n = 0.0, 0
        for name, rec in res["cases"].items():
            n += 1
            for k, r in rec["checks"].items():
                worst = max(worst, r)
                if not r <= 1.0:
                    bad.append(f"{route} {name} {k}: error / bound = {r:.3g}")
            for k in rec["finite"]:
                if not rec["finite"][k]:
                    bad.append(f"{route} {name} {k}: non-finite valid element")
                if not rec["pad"][k]:
                    bad.append(f"{route} {name} {k}: write outside the output (NaN padding changed)")
            # the route really ran: the persistent kernel's probe holds one record per tile it processed, other kernels
            # leave it alone
            if rec["probe_written"] != rec["probe_expected"]:
                bad.append(f"{route} {name}: kernel {rec['kernel']} expected {rec['probe_expected']} probe records, "
                           f"got {rec['probe_written']}")
        print(f"route {route}: {n} cases, worst error / bound {worst:.3f}")
        assert n > 0, route
    assert not bad, "\n".join(bad[:40])


def test_bit_identity_where_the_design_claims_it(routes):
    bad = []
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            h = rec["hash"]
            for k in h:
                if "@rc" in k:
                    if h[k] != h[k.split("@")[0]]:
                        bad.append(f"{route} {name}: reserve_cus {k} changed the bits")
            if "post_ag" in h and h["post_ag"] != h["post"]:
                bad.append(f"{route} {name}: aux_grad changed `post`")
            for t in ("", "_ag"):
                if "post_frag" + t in h:
                    if h["post_frag" + t] != h["post"]:
                        bad.append(f"{route} {name}: aux_frag{t} changed `post`")
                    if h["dact_frag" + t] != h["dact_rowmajor" + t]:
                        bad.append(f"{route} {name}: DACT from the fragment-ordered aux{t} differs from the row-major one")
    # the peel and the 64 x 64 kernel compute what the 256 x 256 kernel computes, bit for bit (BF16 / F32 / RES16)
    whole = routes["256"]["cases"]
    n_peel = n_small = 0
    for other in ("peel", "small"):
        for name, rec in routes[other]["cases"].items():
            if name not in whole or whole[name]["kernel"] != "256" or rec["kernel"] not in ("peel", "small"):
                continue
            if not any(name.startswith(f) for f in ("qkv", "x1", "x2", "dgrad", "aim_t_f32", "f32_", "cls_", "fp8_x2_res16")):
                continue
            if rec["hash"]["out"] != whole[name]["hash"]["out"]:
                bad.append(f"{other} != 256: {name}")
            n_peel += other == "peel"
            n_small += other == "small"
    print(f"bit-identity: {n_peel} peeled and {n_small} 64 x 64 launches compared with the 256 x 256 kernel")
    assert n_peel == len(gc.PEEL_FORMS) and n_small > 0
    assert not bad, "\n".join(bad[:40])
