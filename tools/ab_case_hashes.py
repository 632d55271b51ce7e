#!/usr/bin/env python3
"""Same bits from two builds of the library: run the children of the kernel case tables once per build and compare digests.

usage: tools/ab_case_hashes.py PARENT_LIB --out DIR [--new NEW_LIB] [--tables attn_cases,wgrad_cases,...] [--routes default,...]

The C ABI must be the same in both builds: each build is selected with AIM_HIP_LIB under THIS tree's Python (the convention
of tools/README.md).  For every table and every route it defines, the child `python tests/<table>.py [ROUTE] OUT.json` runs
with the parent library, then with the new one (default: the in-tree library), one process per (table, route, library).
Every value under a "hash" key of the two JSON files is compared, except the outputs that wgrad_cases.py sums with fp32
atomics: they differ between two runs of ONE build, and the table exempts them from its own `repeat` identity.  How many
were left out is printed per route ("excluded").  rowwise_cases.py has no command-line child: its child is this script's own
`--run-child TABLE OUT.json`, which imports the table, calls its `run("cuda")` and dumps the result; its outputs summed by
atomics (layernorm_bwd's dgamma / dbeta above 8192 rows, embed_bwd without a workspace, colsum where several blocks add into
`out`) are left out and counted in the same way.  `embed_ln_bwd` is no table: aim_embed_ln_bwd is in none, so the driver
digests every output of it itself (`--own-child embed_ln_bwd OUT.json`).  attn_shift_cases.py records no digest (it compares tensors inside the
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
          "win_attn_cut_cases": 600, "wgrad_cases": 240, "rowwise_cases": 300, "embed_ln_bwd": 120}


def unordered(rec):
    """outputs of a record that the table itself takes for order-dependent: wgrad_cases.py sums dW by fp32 atomics in plan mode
    "atomics" and db by the column-sum kernel's atomics under bias "colsum", and exempts both from its own `repeat` identity;
    rowwise_cases.py names the atomic sums in the record's route; for colsum the route and the number of row blocks that add
    into `out` (`blocks`, which run_child writes into the record from the table's colsum_plan): several blocks of the 8-wide
    kernel without a workspace (`atomic8`) or of the scalar kernel"""
    kind, route = rec.get("kind"), rec.get("route")
    if kind == "ln_bwd" and route == "atomic":
        return {"dgamma", "dbeta"}
    if kind == "embed_bwd" and route == "atomic":
        return {"dtemporal"}
    if kind == "colsum" and route in ("atomic8", "scalar") and rec["blocks"] > 1:
        return {"out"}
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
NO_CHILD = ("rowwise_cases",)            # tables without a command-line child: run(dev) in a process of this script


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


def run_child(table, out):
    """a NO_CHILD table: import it, run("cuda"), dump the result (the `hashes` walk finds its records' digests)"""
    sys.path.insert(0, TESTS)
    sys.path.insert(0, ROOT)
    mod = importlib.import_module(table)
    res = mod.run("cuda")
    for case in mod.cases():      # a parameter the exclusion reads: how many row blocks add into a column sum
        if case.kind == "colsum" and case.name in res["cases"]:
            res["cases"][case.name]["blocks"] = mod.colsum_plan(case.p)[1]
    with open(out, "w") as f:
        json.dump(res, f, default=str)
    if res.get("errors") or res.get("fatal"):
        sys.exit(f"{table}: {res.get('fatal') or res['errors']}")


def embed_ln_bwd_child(out):
    """every output of aim_embed_ln_bwd (ops.embed_ln_bwd): bf16 and f32; D covering NC = 1, 2, 3, 4 and 8; (B, T, N) giving a
    wave one and two clips and both the class-token block (n = 0) and token blocks"""
    import torch
    sys.path.insert(0, TESTS)
    sys.path.insert(0, ROOT)
    from gemm_cases import _digest
    from aim_amd import ops
    dev = torch.device("cuda")
    res = {"cases": {}}
    for dt in (torch.bfloat16, torch.float32):
        for D in (4, 260, 768, 1024, 1028):
            for B, T, N in ((2, 3, 3), (5, 2, 2)):
                g = torch.Generator().manual_seed(1000 * D + 100 * B + 10 * T + N)
                tok = torch.randn((B * T * (N - 1), D), generator=g).to(dt)
                cls, pos, tmp = torch.randn(D, generator=g), torch.randn((N, D), generator=g), torch.randn((T, D), generator=g)
                gamma = 1.0 + 0.5 * torch.randn(D, generator=g)
                dx = torch.randn((B * T * N, D), generator=g).to(dt)
                u = torch.cat([cls.expand(B * T, 1, D), tok.float().view(B * T, N - 1, D)], 1) + pos
                u = (u.view(B, T, N, D) + tmp[None, :, None, :]).reshape(B * T * N, D)
                mean = u.mean(1)
                rstd = (u.var(1, unbiased=False) + 1e-5).rsqrt()
                o = {"dtok": torch.zeros((B * T * (N - 1), D), dtype=dt), "dcls": torch.ones(D), "dpos": torch.ones((N, D)),
                     "dtemporal": torch.ones((T, D)), "dgamma": torch.ones(D), "dbeta": torch.ones(D)}
                o = {k: v.to(dev) for k, v in o.items()}
                ops.embed_ln_bwd(dx.to(dev), tok.to(dev), cls.to(dev), pos.to(dev), tmp.to(dev), gamma.to(dev), mean.to(dev),
                                 rstd.to(dev), B, T, N, D, **o)
                torch.cuda.synchronize()
                name = f"{'bf16' if dt == torch.bfloat16 else 'f32'}/D{D}/B{B}T{T}N{N}"
                res["cases"][name] = {"hash": {k: _digest(v.cpu()) for k, v in o.items()}}
    with open(out, "w") as f:
        json.dump(res, f)


OWN = {"embed_ln_bwd": embed_ln_bwd_child}          # digest children that belong to no table


def child(table, route, lib, env_extra, env_drop, limit, out):
    env = {k: v for k, v in os.environ.items() if k not in env_drop and k != "AIM_HIP_LIB"}
    env.update(env_extra)
    if lib:
        env["AIM_HIP_LIB"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(int(limit)), sys.executable]
    if table in NO_HASH:
        cmd += [os.path.abspath(__file__), "--digest-child", table]
    elif table in NO_CHILD:
        cmd += [os.path.abspath(__file__), "--run-child", table]
    elif table in OWN:
        cmd += [os.path.abspath(__file__), "--own-child", table]
    else:
        cmd += [os.path.join(TESTS, table + ".py")]
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
    if len(sys.argv) == 4 and sys.argv[1] == "--run-child":
        return run_child(*sys.argv[2:])
    if len(sys.argv) == 4 and sys.argv[1] == "--own-child":
        return OWN[sys.argv[2]](sys.argv[3])
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
        mod = None if table in OWN else importlib.import_module(table)
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
