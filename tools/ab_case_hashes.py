#!/usr/bin/env python3
"""Same bits from two builds of the library: run the children of the kernel case tables once per build and compare digests.

usage: tools/ab_case_hashes.py PARENT_LIB --out DIR [--new NEW_LIB] [--tables attn_cases,wgrad_cases,...] [--routes default,...]

The C ABI must be the same in both builds: each build is selected with AIM_HIP_LIB under THIS tree's Python (the convention
of tools/README.md).  For every table and every route it defines, the child `python tests/<table>.py [ROUTE] OUT.json` runs
with the parent library, then with the new one (default: the in-tree library), one process per (table, route, library).
Every value under a "hash" key of the two JSON files is compared, except the outputs that wgrad_cases.py sums with fp32
atomics: they differ between two runs of ONE build, and the table exempts them from its own `repeat` identity.  How many
were left out is printed per route ("excluded").  attn_shift_cases.py records no digest (it compares tensors inside the
child), so for it the child is this script's own `--digest-child`: the table's cases, inputs and launches (Runner.launch,
shifted) with every output digested as the other tables digest theirs (gemm_cases._digest).
Each child runs under `timeout -k 10`.  The parent's child has no earlier run to be sized from, so it gets the limit its own
GPU test gives it; the new build's child gets the parent child's measured run time plus half (at least 30 s).  The first
non-zero exit status ends the script (nothing further is started, nothing is retried).
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
# table -> the limit (s) its own GPU test gives the child
TABLES = {"attn_cases": 300, "attn_shift_cases": 300, "win_attn_cases": 600, "win_attn_shift_cases": 600,
          "win_attn_cut_cases": 600, "wgrad_cases": 240}


def unordered(rec):
    """outputs of a record that the table itself takes for order-dependent: wgrad_cases.py sums dW by fp32 atomics in plan mode
    "atomics" and db by the column-sum kernel's atomics under bias "colsum", and exempts both from its own `repeat` identity"""
    plan = rec.get("plan")
    if not isinstance(plan, dict):
        return set()
    return ({"dW"} if plan.get("mode") == "atomics" else set()) | ({"db"} if plan.get("bias") == "colsum" else set())


def hashes(node, path=(), excluded=None):
    """{json path: digest} of everything below a "hash" key; a record's order-dependent outputs go to `excluded` instead"""
    out = {}
    excluded = {} if excluded is None else excluded
    if isinstance(node, dict):
        for k, v in node.items():
            if k == "hash":
                skip = unordered(node)
                for name, sub in (v.items() if isinstance(v, dict) else [("", v)]):
                    (excluded if name in skip else out).update(leaves(sub, path + (k, name)))
            else:
                out.update(hashes(v, path + (k,), excluded))
    elif isinstance(node, list):
        for i, v in enumerate(node):
            out.update(hashes(v, path + (str(i),), excluded))
    return out


def leaves(node, path):
    if isinstance(node, dict):
        out = {}
        for k, v in node.items():
            out.update(leaves(v, path + (k,)))
        return out
    return {"/".join(path): node}


NO_HASH = ("attn_shift_cases",)          # tables whose own child records no digest


def digest_child(table, route, out):
    """the cases of a NO_HASH table: forward and backward through its Runner, a digest per output"""
    import torch
    sys.path.insert(0, TESTS)
    sys.path.insert(0, ROOT)
    mod = importlib.import_module(table)
    from gemm_cases import _digest
    from aim_amd import ops
    dev = torch.device("cuda")
    run = mod.Runner(ops, route, dev)
    res = {"route": route, "cases": {}}
    with torch.no_grad():
        for case in mod.cases():
            qkv, do = (t.to(dev) for t in mod.make_inputs(case))
            got, _ = run.launch(case, qkv, do, True)
            res["cases"][case.name] = {"hash": {k: _digest(mod._bits(v)) for k, v in got.items()}}
    with open(out, "w") as f:
        json.dump(res, f)


def child(table, route, lib, env_extra, env_drop, limit, out):
    env = {k: v for k, v in os.environ.items() if k not in env_drop and k != "AIM_HIP_LIB"}
    env.update(env_extra)
    if lib:
        env["AIM_HIP_LIB"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(int(limit)), sys.executable]
    cmd += [os.path.abspath(__file__), "--digest-child", table] if table in NO_HASH else [os.path.join(TESTS, table + ".py")]
    cmd += ([route] if route is not None else []) + [out]
    t0 = time.time()
    rc = subprocess.run(cmd, env=env, cwd=ROOT).returncode
    dt = time.time() - t0
    if rc != 0:
        sys.exit(f"{table} route={route} lib={lib or 'in-tree'}: exit status {rc} after {dt:.0f} s (limit {int(limit)} s); stopping")
    excluded = {}
    with open(out) as f:
        got = hashes(json.load(f), excluded=excluded)
    if not got:
        sys.exit(f"{table} route={route}: the child records no hash; stopping")
    return got, len(excluded), dt


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--digest-child":
        return digest_child(*sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("--new", default=None, help="the other build (default: the in-tree library)")
    ap.add_argument("--tables", default=",".join(TABLES))
    ap.add_argument("--routes", default=None, help="only these routes of the tables that define routes (default: all)")
    ap.add_argument("--out", required=True, help="directory for the children's JSON files and summary.json")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    sys.path.insert(0, TESTS)
    bad, summary = 0, []
    for table in a.tables.split(","):
        mod = importlib.import_module(table)
        routes = getattr(mod, "ROUTES", (None,))
        if a.routes and routes != (None,):
            routes = [r for r in routes if r in a.routes.split(",")]
        for route in routes:
            extra = mod.ROUTE_ENV[route] if route is not None else {}
            drop = getattr(mod, "ROUTE_VARS", ())
            tag = f"{table}.{route or 'only'}"
            hp, xp, tp = child(table, route, a.parent_lib, extra, drop, TABLES[table], os.path.join(a.out, tag + ".parent.json"))
            hn, xn, tn = child(table, route, a.new, extra, drop, max(30.0, 1.5 * tp), os.path.join(a.out, tag + ".new.json"))
            diff = sorted(k for k in set(hp) | set(hn) if hp.get(k) != hn.get(k))
            line = {"table": table, "route": route, "digests": len(hp), "different": len(diff), "excluded": max(xp, xn), "parent_s": round(tp, 1), "new_s": round(tn, 1)}
            print(json.dumps(line), flush=True)
            for k in diff[:10]:
                print("   differs:", k, hp.get(k), hn.get(k), flush=True)
            bad += len(diff)
            summary.append(line)
    with open(os.path.join(a.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    nx = sum(l["excluded"] for l in summary)
    print(("ALL COMPARED DIGESTS EQUAL" if not bad else f"{bad} DIGESTS DIFFER") + f" ({sum(l['digests'] for l in summary)} compared, {nx} excluded)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
