"""Every call form of the bf16 weight gradient (tests/wgrad_cases.py) on every route it can take, against float64.

One child process per route, started one after another (the switches are read once per process): the default, AIM_WGRAD_WGS=3
(`few`: long chunks), AIM_WGRAD_WGS=1000000 (`many`: one 32-row step per chunk), AIM_WGRAD_FUSE_BIAS=0 (`nofuse`: the bias through
aim_colsum_bf16) and AIM_WGRAD_FINISH_V=0 (`finish1`: wgrad_finish1_kernel, cases without db).  The aim_wgrad_bias_bf16 cases run
on every route, the aim_wgrad_slabs_bf16 / aim_wgrad_finish cases, the riders of aim_gemm_bf16_ride and the refusals on the
default one.  A child stops at the first HIP error and exits non-zero; the fixture stops at the first such child.  A record
holds, per output, the worst error as a fraction of the bound derived in wgrad_cases.py, whether every element is finite,
whether every NaN guard, pad column, unused slab and workspace survived, the bit identities, and whether the planning mirrors
agree with aim_wgrad_workspace_bytes and every chunks_written.

Measured on MI355X (256 CUs; worst error / bound, dW then db): default entry 0.116 / 0.149, slabs + finish 0.104 / 0.077, riders
0.205 / 0.128; few 0.227 / 0.143; many 0.116 / 0.149; nofuse 0.116 / 0.149 (the bias aim_colsum_bf16's); finish1 0.083; every
output of the `exact` family 0.  Identities: repeat x186 (default 90, few / many / nofuse 30 each, finish1 6), plain_eq_bias x42,
ones_eq_null x12, slabs_eq_entry x82 (every shape class), rider_eq_slabs x48 -- it holds: a rider launch's slabs and bias slabs
have the bits of aim_wgrad_slabs_bf16's --, host_out x48 (the host's output has the bits of the launch without riders),
tile_alone x1, finish1_eq_finish x5.  277 mirror checks; the rider hosts run 24 tiles on 24 workgroups and 272 tiles on 136,
none peeled.  43 refusals.  195 launches of 92 cases: the children take 1.0 + 0.4 + 0.5 + 0.5 + 0.2 s, the module 13 s.
"""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wgrad_cases as wc  # noqa: E402

T0 = time.time()


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    out = {}
    for route in wc.ROUTES:
        env = {k: v for k, v in os.environ.items() if k not in wc.ROUTE_VARS}
        env.update(wc.ROUTE_ENV[route])
        path = str(tmp_path_factory.mktemp("wgrad") / f"{route}.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "wgrad_cases.py"), route, path], env=env, timeout=240,
                           capture_output=True, text=True)
        if p.returncode != 0:        # stop at the first failing child: nothing more is started on the GPU
            pytest.fail(f"route {route}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[route] = json.load(f)
        print(f"route {route}: {len(out[route]['cases'])} cases in {out[route]['seconds']:.1f} s")
    return out


def test_every_case_is_inside_its_bound_on_every_route(routes):
    bad, worst = [], {}
    for route, res in routes.items():
        assert not res["errors"], "\n".join(f"{route} {k}: {v}" for k, v in list(res["errors"].items())[:20])
        assert list(res["cases"]) == [c.name for c in wc.cases() if wc.runs_on(c, route)], f"{route}: not every case ran"
        for name, rec in res["cases"].items():
            if "refused" in rec:
                bad.append(f"{route} {name}: {rec['refused']}")
                continue
            assert rec["checks"] and set(rec["finite"]) == set(rec["checks"]) <= set(rec["pad"]), name
            for k, r in rec["checks"].items():
                key = (route, rec["kind"], k)
                worst[key] = max(worst.get(key, 0.0), r)
                print(f"  {route} {name} {k}: {r:.4g}")
                if not r <= 1.0:
                    bad.append(f"{route} {name} {k}: error / bound = {r:.3g}")
            for k, ok in rec["finite"].items():
                if not ok:
                    bad.append(f"{route} {name} {k}: non-finite element")
            for k, ok in rec["pad"].items():
                if not ok:
                    bad.append(f"{route} {name} {k}: a guard, pad column, unused slab or workspace changed, or a used slab stayed NaN")
    print("worst error / bound: " + ", ".join(f"{' '.join(k)} {v:.3f}" for k, v in sorted(worst.items())))
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_bit_identities(routes):
    bad, count = [], {}
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            for k, ok in rec["ident"].items():
                count[(route, k)] = count.get((route, k), 0) + 1
                if not ok:
                    bad.append(f"{route} {name}: {k} does not hold")
    # both finish kernels add the chunks in order
    n = 0
    for name, rec in routes["finish1"]["cases"].items():
        if rec["plan"]["finish"] == "one":
            n += 1
            if rec["hash"]["dW"] != routes["default"]["cases"][name]["hash"]["dW"]:
                bad.append(f"finish1 {name}: finish1_eq_finish does not hold")
    count[("finish1", "finish1_eq_finish")] = n
    print("identities: " + ", ".join(f"{k[0]} {k[1]} x{v}" for k, v in sorted(count.items())))
    for key in (("default", "repeat"), ("default", "plain_eq_bias"), ("default", "ones_eq_null"), ("default", "slabs_eq_entry"),
                ("default", "rider_eq_slabs"), ("default", "host_out"), ("default", "tile_alone"), ("finish1", "finish1_eq_finish"),
                ("few", "slabs_eq_entry"), ("many", "slabs_eq_entry"), ("nofuse", "repeat")):
        assert count.get(key, 0) > 0, key
    shapes = {tuple(c.p[k] for k in ("Nw", "Kw")) for c in wc.cases()
              if "slabs_eq_entry" in routes["default"]["cases"].get(c.name, {"ident": {}})["ident"]}
    assert shapes >= set(wc.SHAPES), "slabs_eq_entry: not every shape class"
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:60])


def test_mirrors_agree_with_the_library(routes):
    bad, n = [], 0
    for route, res in routes.items():
        for name, rec in res["cases"].items():
            for k, ok in rec["mirror"].items():
                n += 1
                if not ok:
                    bad.append(f"{route} {name}: the {k} mirror disagrees with the library")
    hosts = {rec["host"]["tiles"]: rec["host"] for rec in routes["default"]["cases"].values() if "host" in rec}
    print(f"{n} mirror checks; {routes['default']['cus']} CUs; rider hosts (tiles, grid, peeled rows): "
          + ", ".join(f"({h['tiles']}, {h['grid']}, {h['peel_rows']})" for h in hosts.values()))
    assert n > 0 and not bad, "\n".join(bad[:60])


def test_refusals_are_loud(routes):
    ref = routes["default"]["refusals"]
    assert set(ref) == set(wc.REFUSAL_TEXT)
    for name, rec in ref.items():
        assert rec["rc"] != 0, f"{name}: not refused"
        assert rec["message"] and wc.REFUSAL_TEXT[name] in rec["message"], (name, rec["message"])
        assert rec["untouched"], f"{name}: refused, yet an output was written"
    print(f"{len(ref)} refusals; module: {time.time() - T0:.1f} s")
