"""Every attention call form that a route switch reaches (tests/attn_cases.py: route_cases) on every route of the backward,
against float64.

One child process per route, started one after another (the switches are read once per process): the default selection,
the pipelined backward without its extra-tile form (AIM_ATTN_PIPE_XT=0), the two-kernel backward at every N
(AIM_ATTN_BWD_PIPE=0), one and three persistent workgroups (AIM_ATTN_PIPE_GRID=1, 3: every item through one workgroup's
prefetch ring / unequal shares), and the whole grid (AIM_ATTN_PIPE_RESERVE=0).  Each child reports, per case and output, the
worst error as a fraction of the bound derived in attn_cases.py, whether the NaN padding behind every output survived,
whether a second run gave the same bits, and the isolation results: frame / head independence under NaN neighbours, a frame
of a 9-frame launch against the frame alone, buffers above 2^31 and 2^32 bytes.  The first child that fails ends the
fixture: nothing more is started on the GPU.

Measured on MI355X (612 cases per route; worst error / bound over all routes): attn out 0.80, out (fp8) 0.99, lse 0.03,
dq 0.48, dk 0.54, dv 0.91; cls_attn 0.996, tattn 0.996 (their last step is one bf16 rounding of an fp32 result, so the bound
is met to within the fp32 terms)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_cases as ac  # noqa: E402


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    out = {}
    for route in ac.ROUTES:
        env = {k: v for k, v in os.environ.items() if k not in ac.ROUTE_VARS}
        env.update(ac.ROUTE_ENV[route])
        path = str(tmp_path_factory.mktemp("attn_routes") / f"{route}.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "attn_cases.py"), route, path], env=env, timeout=300,
                           capture_output=True, text=True)
        if p.returncode != 0:        # stop at the first failing child: nothing more is started on the GPU
            pytest.fail(f"route {route}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[route] = json.load(f)
    return out


def test_every_case_is_inside_its_bound_on_every_route(routes):
    bad = []
    names = [c.name for c in ac.route_cases()]
    for route, res in routes.items():
        worst, n = {}, 0
        assert list(res["cases"]) == names, f"route {route} did not run every case"
        for name, rec in res["cases"].items():
            n += 1
            for k, r in rec["checks"].items():
                key = name.split("/")[0] + " " + k.split("@")[0]
                worst[key] = max(worst.get(key, 0.0), r)
                if not r <= 1.0:
                    bad.append(f"{route} {name} {k}: error / bound = {r:.3g}")
            for k, ok in rec["finite"].items():
                if not ok:
                    bad.append(f"{route} {name} {k}: non-finite element")
            for k, ok in rec["pad"].items():
                if not ok:
                    bad.append(f"{route} {name} {k}: write outside the output (NaN padding changed)")
            for k in rec:
                if k.startswith("zero_head") and not rec[k]:
                    bad.append(f"{route} {name} {k}: dO = 0 for a head, but its gradients are not exactly zero")
                if k.startswith("other_rows_kept") and not rec[k]:
                    bad.append(f"{route} {name} {k}: cls_attn_bwd changed a row that is not a class row")
        print(f"route {route}: {n} cases, worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
        assert n > 0, route
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_the_route_ran(routes):
    """delta goes in filled with NaN: the two-kernel backward writes all of it, the pipelined one none of it"""
    bad = []
    for route, res in routes.items():
        n = {"two": 0, "pipe": 0}
        for name, rec in res["cases"].items():
            if "plan" not in rec or "delta_written@a" not in rec:
                continue
            kernel = rec["plan"][0]
            n[kernel] += 1
            for form in "ab":
                if kernel == "two" and not rec[f"delta_written@{form}"]:
                    bad.append(f"{route} {name}: the two-kernel form should have written delta ({form})")
                if kernel == "pipe" and not rec[f"delta_untouched@{form}"]:
                    bad.append(f"{route} {name}: the pipelined form should have left delta alone ({form})")
        print(f"route {route}: {n['pipe']} pipelined and {n['two']} two-kernel backward cases")
        assert n["two"] > 0 and (n["pipe"] > 0) == (route != "two"), (route, n)
    assert not bad, "\n".join(bad[:40])


def test_bit_identities(routes):
    bad = []
    for route, res in routes.items():
        n_rep = n_alone = n_ind = 0
        for name, rec in res["cases"].items():
            for k, ok in rec["repeat"].items():
                n_rep += 1
                if not ok:
                    bad.append(f"{route} {name} {k}: a second run gave other bits")
            if "alone_identical" in rec:
                n_alone += 1
                if not rec["alone_identical"]:
                    bad.append(f"{route} {name}: a frame of the launch differs from the frame launched alone")
            if "independent" in rec:
                n_ind += 1
                if not rec["independent"]:
                    bad.append(f"{route} {name}: NaN neighbours (frames, heads) changed a clean item")
        print(f"route {route}: {n_rep} outputs repeated, {n_alone} launches against single frames, {n_ind} poisoned launches")
        assert n_rep > 0 and n_alone == 2 and n_ind == 3, route
    # the forward, cls_attn and tattn do not depend on the route; neither does a two-kernel backward
    base = routes["default"]["cases"]
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            for k, h in rec["hash"].items():
                fixed = not k.startswith(("dqkv", "delta")) or not name.startswith("attn/") or \
                    (rec["plan"][0] == "two" and base[name]["plan"][0] == "two" and k.startswith("dqkv"))
                if fixed and h != base[name]["hash"][k]:
                    bad.append(f"{route} {name} {k}: differs from the default route")
    # one workgroup, three, all but the reserve and all of them walk the items of the pipelined kernel to the same bits
    for route in ("grid1", "grid3", "reserve0"):
        for name, rec in routes[route]["cases"].items():
            for k, h in rec["hash"].items():
                if k.startswith("dqkv") and h != base[name]["hash"][k]:
                    bad.append(f"{route} {name} {k}: the pipelined backward depends on the grid")
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_large_offsets(routes):
    bad = []
    for route, res in routes.items():
        for tag, rec in res["large"].items():
            if not rec["ran"]:
                assert tag == "2^32", f"{route}: the 2^31 case needs {rec['need'] / 2 ** 30:.1f} GiB, {rec['free'] / 2 ** 30:.1f} free"
                print(f"route {route}: {tag} not run ({rec['free'] / 2 ** 30:.1f} GiB free)")
                continue
            assert rec["bytes"] > {"2^31": 2 ** 31, "2^32": 2 ** 32}[tag]
            for k, r in rec["checks"].items():
                if not r <= 1.0:
                    bad.append(f"{route} large {tag} {k}: error / bound = {r:.3g}")
            for k, ok in rec["finite"].items():
                if not ok:
                    bad.append(f"{route} large {tag} {k}: non-finite element")
            if not rec["identical"]:
                bad.append(f"{route} large {tag}: first / last frames differ from a four-frame launch")
    assert not bad, "\n".join(bad)


def test_refusals_are_loud(routes):
    for route, res in routes.items():
        for name, msg in res["refusals"].items():
            if name.endswith("null lse_cls"):
                assert msg and "null pointer" in msg, (route, name, msg)
                continue
            assert msg and "unsupported shape" in msg and ("N <= 288" in msg or "T <= 32" in msg), (route, name, msg)
        assert len(res["refusals"]) == 15 and all(res["refusals_untouched"].values()), (route, res["refusals_untouched"])
