"""Every call form of the bf16 weight gradient -- aim_wgrad_bf16, aim_wgrad_bias_bf16, aim_wgrad_slabs_bf16 + aim_wgrad_finish and
the rider workgroups of aim_gemm_bf16_ride, all of them wgrad_tile::run (csrc/wgrad_tile.h) -- on every route, against float64.

    dW[n][k] = dW0[n][k] + sum_m G[m][n] A[m][k]        db[n] = db0[n] + sum_m at[m % ntok] G[m][n]      m in [m_begin, m_end),

m the ABSOLUTE row of the problem.  The reference takes the bf16 / fp32 operand values to float64 on the CPU and never calls
the library.  This module is the case table, the Python mirrors of the host-side planning (wgrad_chunks in wgrad.hip,
aim_wgrad_range_chunks in gemm256.hip, the workspace formula), the bounds, an fp32 emulation of the kernels' summation order
with one plausible bug at a time (test_wgrad_cases_cpu.py proves on the CPU that the table rejects each of them), and the
launcher: `python wgrad_cases.py ROUTE OUT.json` runs every case of one route through ctypes (the route switches are read once
per process) and writes one record per case.

Bounds (u = 2^-24; a product of two bf16 values is exact in fp32).
  dW.  A chunk of rows is walked in 32-row steps, each one v_mfma_f32_16x16x32_bf16 into the accumulator: at most 32 roundings a
    step, in whatever order the unit adds, so a chain of 31 + S for the S steps of the longest chunk.  The C chunks are added in
    order (the finish kernels) or in any order (fp32 atomics), then dW0:
        |dW - ref| <= (31 + S + C + 1) u (sum_m |g a| + |dW0|)
    on every route; one chunk is added to dW directly (C = 1).
  db.  A thread of the 16 row groups adds f0 v0 + f1 v1 per step (one rounding per product, two additions: 2 S), the 16 groups are
    added in order (15), the chunks lane-strided (ceil(C / 64)) and through a 6-step butterfly, then db0 (1); with C = 1 the
    workgroup adds to db itself:
        |db - ref| <= (2 S + 15 + ceil(C / 64) + 6 + 1 + 1) u (sum_m |at g| + |db0|).
    Without bias slabs (AIM_WGRAD_FUSE_BIAS=0, no or a short workspace; C > 1) the bias is aim_colsum_bf16's: its bound is
    rowwise_cases.colsum_expected's for the route rowwise_cases.colsum_route names.
  The `exact` family (G, A in {-2..2}, at in {0, 1, 2}, small integer dW0 / db0) keeps every partial sum an integer below 2^24:
    bound 0, on the atomics route too.

Identities (each recorded as a flag, asserted by test_wgrad_routes_gpu.py): `repeat` (a second run; not for atomics with C > 1 nor
for aim_colsum_bf16's atomic route), `plain_eq_bias` (aim_wgrad_bf16 == aim_wgrad_bias_bf16 without `at`), `ones_eq_null` (a table
of ones == no table), `slabs_eq_entry` (aim_wgrad_slabs_bf16 with the library's chunking + aim_wgrad_finish == the one-call
entry), `rider_eq_slabs` (a rider launch's slabs == aim_wgrad_slabs_bf16's with max_chunks = chunks), `tile_alone` (the first
256 x 256 outputs of a 264 x 264 problem == the 256 x 256 problem on the same operand columns), and across routes
`finish1_eq_finish` (both finish kernels add the chunks in order).

Every output, workspace and slab goes in as NaN (the accumulated dW / db as random values), with 8 NaN elements behind it; the
columns Kw .. lddw of a strided dW, the rows of G / A outside [m_begin, m_end) and the columns outside an operand slice are NaN
as well: whatever reads or writes past its share shows.

Not in the table: riders with `batch = 2` (aim_gemm_bf16_ride has no batch argument: the library passes 1).
"""
import json
import os
import sys
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rowwise_cases as rw  # noqa: E402
from gemm_cases import U24, _digest, peel_rows, ratio  # noqa: E402
from rowwise_cases import _FATAL, _XOR, _bits_eq, _cdiv, _seq, _sum_bound  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
MSTEP, TILE = 32, 256

ROUTES = ("default", "few", "many", "nofuse", "finish1")
ROUTE_VARS = ("AIM_WGRAD_WGS", "AIM_WGRAD_FUSE_BIAS", "AIM_WGRAD_FINISH_V")
ROUTE_ENV = {"default": {}, "few": {"AIM_WGRAD_WGS": "3"}, "many": {"AIM_WGRAD_WGS": "1000000"},
             "nofuse": {"AIM_WGRAD_FUSE_BIAS": "0"}, "finish1": {"AIM_WGRAD_FINISH_V": "0"}}
TARGET = {"default": 256, "few": 3, "many": 1000000, "nofuse": 256, "finish1": 256}
PATHS = ("C1", "C2_8", "C9_64", "C65+")


@dataclass
class Case:
    name: str
    kind: str                     # entry | slabs | ride
    p: dict = field(default_factory=dict)
    family: str = "unit"
    seed: int = 0


# ---- mirrors of the host-side planning ---------------------------------------------------------------------------------------
def tiles_of(Nw: int, Kw: int) -> int:
    return _cdiv(Nw, TILE) * _cdiv(Kw, TILE)


def wgrad_chunks(M: int, tiles: int, target: int = 256) -> Tuple[int, int]:
    """csrc/wgrad.hip::wgrad_chunks -> (chunks, rows per chunk)"""
    n = min(_cdiv(target, tiles), _cdiv(M, MSTEP))
    chunk = _cdiv(_cdiv(M, n), MSTEP) * MSTEP
    return _cdiv(M, chunk), chunk


def range_chunks(rows: int, max_chunks: int) -> Tuple[int, int]:
    """csrc/gemm256.hip::aim_wgrad_range_chunks -> (non-empty chunks, rows per chunk)"""
    chunk = _cdiv(_cdiv(rows, MSTEP), max(max_chunks, 1)) * MSTEP
    return (_cdiv(rows, chunk) if rows > 0 else 0), chunk


def workspace_bytes(M: int, Nw: int, Kw: int, target: int = 256) -> int:
    """aim_wgrad_workspace_bytes: the weight slabs and one bias row per chunk"""
    n, _ = wgrad_chunks(M, tiles_of(Nw, Kw), target)
    return n * Nw * (Kw + 1) * 4 if n > 1 else 0


def balanced_grid(tiles: int, cus: int, reserve: int = 0) -> int:
    """csrc/gemm256.hip::balanced_grid (AIM_GEMM_BALANCED unset): workgroups of the persistent GEMM"""
    c = cus - reserve if cus - reserve > 8 else 8
    if tiles <= c:
        return tiles
    rounds = _cdiv(tiles, c)
    return min(c, _cdiv(tiles, rounds))


@dataclass
class Plan:
    segs: List[Tuple[int, int]]       # the chunks' absolute row ranges, in slab order
    calls: List[Tuple[int, int]]      # per launch: (chunks, rows per chunk)
    mode: str                         # direct (one chunk into dW) | slabs | atomics
    bias: Optional[str]               # None | direct | fused | colsum
    finish: str = "v"                 # v | one (wgrad_finish1_kernel)
    need: int = 0                     # workspace bytes the library asks for
    have: int = 0                     # workspace bytes the case passes

    @property
    def C(self):
        return len(self.segs)

    @property
    def S(self):
        return max(_cdiv(e - b, MSTEP) for b, e in self.segs)

    @property
    def path(self):
        C = self.C
        return "C1" if C == 1 else "C2_8" if C <= 8 else "C9_64" if C <= 64 else "C65+"

    def sig(self):
        return (tuple(self.segs), self.mode, self.bias, self.finish)


def row_range(case: Case) -> Tuple[int, int]:
    p = case.p
    if case.kind == "entry":
        return 0, p["rows"]
    if case.kind == "slabs":
        return p["ranges"][0][0], p["ranges"][-1][1]
    return p["mb"], p["me"]


def runs_on(case: Case, route: str) -> bool:
    if case.kind != "entry":
        return route == "default"
    return route != "finish1" or case.p["bias"] == "none"


def plan(case: Case, route: str = "default") -> Plan:
    p = case.p
    Nw, Kw = p["Nw"], p["Kw"]
    tiles, target = tiles_of(Nw, Kw), TARGET[route]
    if case.kind == "entry":
        M = p["rows"]
        C, chunk = wgrad_chunks(M, tiles, target)
        need = workspace_bytes(M, Nw, Kw, target)
        have = {"exact": need, "large": need + 4096, "short": max(need - 16, 0), "null": 0}[p["ws"]]
        slab = p["ws"] != "null" and C > 1 and have >= need
        mode = "direct" if C == 1 else "slabs" if slab else "atomics"
        bias = None if p["bias"] == "none" else "direct" if C == 1 else "fused" if slab and route != "nofuse" else "colsum"
        finish = "one" if mode == "slabs" and route == "finish1" and bias != "fused" else "v"
        segs = [(c * chunk, min(M, (c + 1) * chunk)) for c in range(C)]
        return Plan(segs, [(C, chunk)], mode, bias, finish, need, have)
    segs, calls = [], []
    ranges = p["ranges"] if case.kind == "slabs" else [(p["mb"], p["me"], p["chunks"])]
    for mb, me, mc in ranges:
        C, chunk = range_chunks(me - mb, mc) if mc > 0 else wgrad_chunks(me - mb, tiles, target)
        calls.append((C, chunk))
        segs += [(mb + c * chunk, min(me, mb + (c + 1) * chunk)) for c in range(C)]
    return Plan(segs, calls, "slabs", None if p["bias"] == "none" else "fused")


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _operand(vals, form, mb, me):
    """[me + 3, ld] bf16, NaN outside rows [mb, me) and outside the slice's columns -> (buffer, column offset)"""
    w = vals.shape[1]
    ld, off = {"dense": (w, 0), "slice": (w + 24, 16), "model": (3264, 3072)}[form]
    assert off + w <= ld
    buf = torch.full((me + 3, ld), NAN, dtype=BF16)
    buf[mb:me, off:off + w] = vals
    return buf, off


def build_inputs(case: Case) -> Dict[str, torch.Tensor]:
    p, g = case.p, torch.Generator().manual_seed(7000 + case.seed)
    Nw, Kw = p["Nw"], p["Kw"]
    mb, me = row_range(case)
    rows, fam = me - mb, case.family

    def rn(*shape):
        if fam == "exact":
            return torch.randint(-2, 3, shape, generator=g).float()
        return torch.randn(shape, generator=g) + (3.0 if fam == "offset" else 0.0)

    inp = {}
    inp["G_buf"], inp["g_off"] = _operand(rn(rows, Nw).to(BF16), p["gf"], mb, me)
    inp["A_buf"], inp["a_off"] = _operand(rn(rows, Kw).to(BF16), p["af"], mb, me)
    small = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if fam == "exact" else (lambda *s: torch.randn(s, generator=g))
    inp["dW0"] = small(Nw, Kw)
    if p["bias"] != "none":
        inp["db0"] = small(Nw)
    if p["bias"] == "at":
        n = p["ntok"]
        if fam == "exact":
            inp["at"] = torch.randint(0, 3, (n,), generator=g).float()
        elif p["atk"] == "ramp":
            inp["at"] = (1.0 + torch.arange(n, dtype=F64) / n).float()
        else:           # DropPath: {0, 1 / 0.7}
            inp["at"] = (torch.rand(n, generator=g) < 0.7).float() / 0.7
    return inp


def views(case: Case, inp):
    """G [me + 3, Nw] and A [me + 3, Kw]: the operand columns (row m is the problem's row m)"""
    p = case.p
    return (inp["G_buf"][:, inp["g_off"]:inp["g_off"] + p["Nw"]], inp["A_buf"][:, inp["a_off"]:inp["a_off"] + p["Kw"]])


def _factors(case, inp, mb, me, dtype):
    if "at" not in inp:
        return torch.ones(me - mb, dtype=dtype)
    return inp["at"].to(dtype)[torch.arange(mb, me) % case.p["ntok"]]


def _colsum_twin(case: Case, inp):
    """the aim_colsum_bf16 call the entry makes for its bias, as a rowwise_cases colsum case"""
    p = case.p
    G, _ = views(case, inp)
    cp = dict(M=p["rows"], C=p["Nw"], ldx=inp["G_buf"].shape[1], ws="none", ntok=p["ntok"] if "at" in inp else 0, at="at" in inp)
    cinp = {"X": G[:p["rows"]], "out0": inp["db0"]}
    if "at" in inp:
        cinp["at"] = inp["at"]
    return rw.Case(case.name + "/colsum", "colsum", cp), cinp


def expected(case: Case, inp, route: str = "default") -> Dict[str, tuple]:
    """{output: (float64 reference, bound)}"""
    pl = plan(case, route)
    mb, me = row_range(case)
    G, A = views(case, inp)
    Gd, Ad = G[mb:me].double(), A[mb:me].double()
    exact = case.family == "exact"
    dW0 = inp["dW0"].double()
    bound = (31 + pl.S + pl.C + 1) * U24 * (Gd.abs().T @ Ad.abs() + dW0.abs())
    out = {"dW": (dW0 + Gd.T @ Ad, torch.zeros_like(bound) if exact else bound)}
    if pl.bias:
        t = Gd * _factors(case, inp, mb, me, F64)[:, None]
        db0 = inp["db0"].double()
        if pl.bias == "colsum":
            ref, bound = rw.colsum_expected(*_colsum_twin(case, inp))["out"]
        else:
            ref = db0 + t.sum(0)
            bound = _sum_bound(2 * pl.S + 15 + _cdiv(pl.C, 64) + 6 + 1, 1, t.abs().sum(0), db0)
        out["db"] = (ref, torch.zeros_like(bound) if exact else bound)
    return out


def compare(case, inp, got, route="default") -> Dict[str, float]:
    exp = expected(case, inp, route)
    assert set(exp) == set(got), (case.name, sorted(exp), sorted(got))
    return {k: ratio(got[k].reshape(exp[k][0].shape), *exp[k]) for k in exp}


# ---- fp32 emulation ----------------------------------------------------------------------------------------------------------
MUTANTS = ("at_from_range", "bias_rows16", "drop_partial_step", "drop_last_chunk", "finish_tail", "assign", "lddw_as_Kw",
           "tile_shift8", "btok_nowrap", "bias_tile_col")
MUTANTS_UNSEEN: Dict[str, str] = {}        # mutant -> why no case can see it (none)


def applies(mut: str, case: Case, pl: Plan) -> bool:
    p = case.p
    own_bias = pl.bias in ("direct", "fused")
    with_at = own_bias and p["bias"] == "at"
    if mut == "at_from_range":
        return with_at and row_range(case)[0] % p["ntok"] != 0
    if mut == "bias_rows16":
        return own_bias
    if mut == "drop_partial_step":
        return any((e - b) % MSTEP for b, e in pl.segs)
    if mut == "drop_last_chunk":
        return pl.C > 1
    if mut == "finish_tail":
        return pl.mode == "slabs" and pl.finish == "v" and pl.C > 8 and pl.C % 8 != 0
    if mut == "assign":
        return True
    if mut == "lddw_as_Kw":
        return p.get("xl", 0) > 0 and p["Nw"] > 1
    if mut == "tile_shift8":
        return p["Kw"] % TILE > 8 or p["Nw"] % TILE > 8
    if mut == "btok_nowrap":
        return with_at and pl.S > 1 and MSTEP % p["ntok"] != 0
    if mut == "bias_tile_col":
        return own_bias and p["Nw"] > TILE
    raise KeyError(mut)


def _shift_last_tile(X):
    """the columns of the last, partial 256-wide tile rotated by one 8-column group"""
    w = X.shape[1]
    k0 = (w // TILE) * TILE
    X = X.clone()
    X[:, k0:] = torch.roll(X[:, k0:], -8, dims=1)
    return X


def _bias_chunk(case, inp, Gf, b, e, mut):
    """one workgroup's column sums of rows [b, e): thread (row group r of 16) adds f0 v0 + f1 v1 per step, the groups in order"""
    p = case.p
    steps = _cdiv(e - b, MSTEP)
    pad = torch.zeros((steps * MSTEP, Gf.shape[1]), dtype=F32)
    pad[:e - b] = Gf[b:e]
    m = torch.arange(b, b + steps * MSTEP)
    if "at" in inp:
        n, at = p["ntok"], inp["at"]
        if mut == "btok_nowrap":              # btok += bstep without the wrap: past the table the LDS holds something else (0 here)
            first = (m[:MSTEP] % n)[None, :] + (MSTEP % n) * torch.arange(steps)[:, None]
            f = torch.cat([at, torch.zeros(int(first.max()) + 1)])[first.reshape(-1)]
        else:
            f = at[(m - row_range(case)[0] if mut == "at_from_range" else m) % n]
    else:
        f = torch.ones(len(m))
    P = (f[:, None] * pad).view(steps, 2, 16, -1)
    bs = torch.zeros((16, Gf.shape[1]), dtype=F32)
    for s in range(steps):
        bs = bs + (P[s, 0] if mut == "bias_rows16" else P[s, 0] + P[s, 1])
    return _seq(bs)


def emulate(case: Case, inp, route: str = "default", mut: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """the kernels' arithmetic in fp32, in their order (a step's 32 products one after another); `mut`: one bug"""
    pl, p = plan(case, route), case.p
    Nw, Kw = p["Nw"], p["Kw"]
    G, A = views(case, inp)
    Gf, Af = G.float(), A.float()
    if mut == "tile_shift8":
        if Kw % TILE > 8:
            Af = _shift_last_tile(Af)
        else:
            Gf = _shift_last_tile(Gf)
    segs = pl.segs[:-1] if mut == "drop_last_chunk" else pl.segs
    slabs, bslabs = [], []
    for b, e in segs:
        if mut == "drop_partial_step":
            e = b + (e - b) // MSTEP * MSTEP
        acc = torch.zeros((Nw, Kw), dtype=F32)
        for m in range(b, e):
            acc = acc + Gf[m][:, None] * Af[m][None, :]
        slabs.append(acc)
        if pl.bias in ("direct", "fused"):
            bslabs.append(_bias_chunk(case, inp, Gf, b, e, mut) if e > b else torch.zeros(Nw))
    if mut == "finish_tail":
        slabs = slabs[:len(slabs) // 8 * 8]
    tot = _seq(torch.stack(slabs)) if slabs else torch.zeros((Nw, Kw))
    keep = 0.0 if mut == "assign" else 1.0
    out = {"dW": keep * inp["dW0"] + tot}
    if mut == "lddw_as_Kw":            # row n written at n * Kw of the lddw-strided buffer
        lddw = Kw + p["xl"]
        flat = torch.full((Nw * lddw,), NAN)
        flat.view(Nw, lddw)[:, :Kw] = inp["dW0"]
        flat[:Nw * Kw] = flat[:Nw * Kw] + tot.reshape(-1)
        out["dW"] = flat.view(Nw, lddw)[:, :Kw].clone()
    if pl.bias == "colsum":
        out["db"] = rw.colsum_emulate(*_colsum_twin(case, inp))["out"]
    elif pl.bias:
        if pl.bias == "direct":
            a = bslabs[0] if bslabs else torch.zeros(Nw)
        else:                              # lane l of the finish adds chunks l, l + 64, ...; wave_sum
            lanes = torch.zeros((64, Nw), dtype=F32)
            for c, v in enumerate(bslabs):
                lanes[c % 64] = lanes[c % 64] + v
            for o in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[_XOR[o]]
            a = lanes[0]
        db = keep * inp["db0"] + a
        if mut == "bias_tile_col":
            db = keep * inp["db0"]
            for n0 in range(0, Nw, TILE):
                w = min(TILE, Nw - n0)
                db[:w] = keep * inp["db0"][:w] + a[n0:n0 + w]
        out["db"] = db
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------
SHAPES = ((8, 16), (72, 200), (256, 256), (264, 8), (8, 264), (520, 72), (192, 768), (768, 192))
ROWS = (1, 31, 32, 33, 96, 97, 129, 613, 1000, 2100)
NTOKS = (1, 5, 31, 32, 33, 197, 257, 4096)
RIDE_HOSTS = ("a", "b", "c", "d")
RIDE_GRADS = (
    # (Nw, Kw), rows, G form, A form, bias, ntok, at table
    ((72, 200), (37, 134), "slice", "dense", "at", 197, "drop"),
    ((264, 8), (0, 33), "dense", "slice", "db", 0, None),
    ((520, 72), (100, 713), "dense", "dense", "at", 33, "ramp"),
    ((768, 192), (224, 837), "dense", "model", "at", 4096, "ramp"),
)
RIDE_CHUNKS = (1, 3, 1000)


def _forms(Nw, Kw, i):
    gf = ("dense", "slice", "dense", "slice")[i % 4]
    af = ("dense", "dense", "slice", "slice")[i % 4]
    if Nw == 192 and i % 2 == 0:
        gf = "model"
    if Kw == 192 and i % 2 == 0:
        af = "model"
    return gf, af


def cases() -> List[Case]:
    out, seed = [], [0]

    def add(name, kind, family="unit", **p):
        seed[0] += 1
        out.append(Case(name, kind, p, family, seed[0]))

    def entry(rows, shape, i, xl, bias, ntok, atk, ws, family="unit"):
        Nw, Kw = shape
        gf, af = _forms(Nw, Kw, i)
        add(f"entry/{family}/r{rows}/{Nw}x{Kw}/{gf[0]}{af[0]}/ld+{xl}/{bias}{ntok if bias == 'at' else ''}{atk or ''}/{ws}", "entry",
            family, rows=rows, Nw=Nw, Kw=Kw, gf=gf, af=af, xl=xl, bias=bias, ntok=ntok, atk=atk, ws=ws)

    E = "exact"
    entry(1, (8, 16), 0, 0, "at", 1, "ramp", "exact")
    entry(31, (72, 200), 1, 4, "db", 0, None, "exact")
    entry(32, (256, 256), 2, 0, "at", 5, "ramp", "exact", "offset")
    entry(33, (264, 8), 3, 64, "at", 31, "drop", "exact")
    entry(96, (8, 264), 0, 0, "at", 32, "ramp", "exact")
    entry(97, (520, 72), 0, 4, "at", 33, "ramp", "exact")
    entry(129, (192, 768), 0, 0, "db", 0, None, "exact")
    entry(129, (768, 192), 0, 0, "at", 197, "drop", "exact")
    entry(129, (768, 3072), 1, 0, "at", 197, "ramp", "exact")            # ViT_ImageNet's c_fc gradient
    entry(613, (768, 192), 0, 0, "at", 197, "drop", "exact", "offset")
    entry(1000, (192, 768), 0, 0, "at", 257, "ramp", "large")
    entry(2100, (72, 200), 1, 0, "at", 4096, "ramp", "exact")
    entry(2100, (768, 192), 1, 0, "none", 0, None, "exact")
    entry(2100, (8, 16), 0, 0, "at", 197, "drop", "null")
    entry(1000, (256, 256), 0, 0, "db", 0, None, "null")
    entry(613, (264, 8), 2, 0, "at", 33, "ramp", "short")
    entry(129, (8, 264), 3, 4, "none", 0, None, "short")
    entry(97, (72, 200), 2, 0, "at", 5, "drop", "null")
    entry(1000, (520, 72), 3, 64, "none", 0, None, "large")
    entry(257, (8, 16), 1, 4, "none", 0, None, "exact")
    entry(2100, (264, 8), 0, 0, "none", 0, None, "exact", "offset")
    entry(33, (768, 192), 0, 0, "at", 33, "ramp", "exact", "offset")
    # the exact family: every shape class, with and without a workspace
    for i, (shape, rows, ntok, ws) in enumerate(zip(SHAPES, (2100, 97, 129, 613, 1000, 33, 96, 1000), (197, 5, 31, 33, 32, 257, 1, 4096),
                                                    ("exact", "null", "exact", "null", "short", "exact", "large", "exact"))):
        entry(rows, shape, i, 4 if i % 3 == 0 else 0, "at", ntok, "drop", ws, E)
    entry(1000, (72, 200), 0, 0, "none", 0, None, "exact", E)
    entry(31, (8, 16), 0, 0, "none", 0, None, "null", E)

    def slabs(name, shape, ranges, i, xl=0, bias="at", ntok=197, atk="drop", family="unit", **extra):
        Nw, Kw = shape
        gf, af = _forms(Nw, Kw, i)
        add(f"slabs/{family}/{name}/{Nw}x{Kw}", "slabs", family, Nw=Nw, Kw=Kw, gf=gf, af=af, xl=xl, bias=bias, ntok=ntok, atk=atk,
            ranges=ranges, **extra)

    slabs("m37_r97_lib", (72, 200), [(37, 134, 0)], 1, ntok=33, atk="ramp")
    slabs("m224_7of100", (8, 16), [(224, 424, 100)], 0)
    slabs("m0_8of8", (8, 16), [(0, 256, 8)], 2, bias="db", family=E)
    slabs("m37_9_nobias", (264, 8), [(37, 294, 100)], 3, bias="none")
    slabs("m37_17_two_calls", (8, 264), [(37, 325, 100), (325, 575, 100)], 0, xl=4, ntok=5, atk="ramp", family=E)
    slabs("m0_70_three_calls", (8, 16), [(0, 1000, 100), (1000, 2000, 100), (2000, 2190, 7)], 1, ntok=4096, atk="ramp")
    slabs("m224_r613_3", (520, 72), [(224, 837, 3)], 0, ntok=257)
    slabs("m0_r129_1", (256, 256), [(0, 129, 1)], 2, bias="db", family=E)
    slabs("m37_r1000_7", (768, 192), [(37, 1037, 7)], 0, xl=64, family="offset")
    slabs("m224_r33_lib", (192, 768), [(224, 257, 0)], 0, ntok=31, atk="ramp")
    slabs("m37_r1_1", (72, 200), [(37, 38, 1)], 3, ntok=32, atk="ramp")
    slabs("tile_alone", (264, 264), [(37, 134, 3)], 1, ntok=5, atk="ramp", tile_alone=True)

    for h in RIDE_HOSTS:
        for gi, ((Nw, Kw), (mb, me), gf, af, bias, ntok, atk) in enumerate(RIDE_GRADS):
            for ci, ch in enumerate(RIDE_CHUNKS):
                fam = ("unit", "offset", E)[(gi + ci + RIDE_HOSTS.index(h)) % 3]
                add(f"ride/{h}/{fam}/{Nw}x{Kw}/m{mb}_{me}/c{ch}", "ride", fam, host=h, Nw=Nw, Kw=Kw, gf=gf, af=af, bias=bias, ntok=ntok,
                    atk=atk, mb=mb, me=me, chunks=ch)
    return out


# ---- the launcher ------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, route):
        sys.path.insert(0, os.path.dirname(HERE))
        from aim_amd import ops
        from aim_amd.lib import GemmArgs, WgradRideArgs, check, load_library
        self.ops, self.lib, self.check, self.stream = ops, load_library(), check, ops._stream
        self.GemmArgs, self.WgradRideArgs = GemmArgs, WgradRideArgs
        self.dev, self.route = torch.device("cuda"), route
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.hosts = {}

    def nan(self, n, dtype=F32):
        return torch.full((n + 8,), NAN, dtype=dtype, device=self.dev)

    def put(self, t):
        buf = self.nan(t.numel(), t.dtype)
        buf[:t.numel()] = t.reshape(-1).to(self.dev)
        return buf


def _ptr(buf, off=0):
    return None if buf is None else buf.data_ptr() + off * buf.element_size()


def _all_nan(t):
    return bool(torch.isnan(t).all())


class _Dev:
    """a case's operands on the device"""

    def __init__(self, ctx, case, inp):
        p = case.p
        self.Nw, self.Kw, self.lddw = p["Nw"], p["Kw"], p["Kw"] + p.get("xl", 0)
        self.G, self.A = ctx.put(inp["G_buf"]), ctx.put(inp["A_buf"])
        self.ldg, self.lda = inp["G_buf"].shape[1], inp["A_buf"].shape[1]
        self.Gp, self.Ap = _ptr(self.G, inp["g_off"]), _ptr(self.A, inp["a_off"])
        self.at = ctx.put(inp["at"]) if "at" in inp else None
        self.ntok = p["ntok"] if "at" in inp else 0
        self.ctx, self.inp = ctx, inp

    def dW(self, Nw=None, Kw=None):
        Nw, Kw = Nw or self.Nw, Kw or self.Kw
        buf = self.ctx.nan(Nw * self.lddw)
        buf[:Nw * self.lddw].view(Nw, self.lddw)[:, :Kw] = self.inp["dW0"][:Nw, :Kw].to(self.ctx.dev)
        return buf

    def db(self):
        return self.ctx.put(self.inp["db0"]) if "db0" in self.inp else None

    def take(self, dWb, dbb, Nw=None, Kw=None):
        """-> (got, pad): the outputs on the CPU; whether everything around them is still NaN"""
        Nw, Kw = Nw or self.Nw, Kw or self.Kw
        torch.cuda.synchronize()
        h = dWb.cpu()
        v = h[:Nw * self.lddw].view(Nw, self.lddw)
        got = {"dW": v[:, :Kw].clone()}
        v[:, :Kw] = NAN
        pad = {"dW": _all_nan(h)}
        if dbb is not None:
            h = dbb.cpu()
            got["db"], pad["db"] = h[:Nw].clone(), _all_nan(h[Nw:])
        return got, pad


def _entry_once(ctx, case, d, pl, at="case", plain=False):
    p = case.p
    dWb, dbb = d.dW(), d.db()
    nf = pl.have // 4
    ws = None if p["ws"] == "null" else ctx.nan(nf)
    atb, ntok = (d.at, d.ntok) if at == "case" else (at, len(at) - 8)
    if plain:
        rc = ctx.lib.aim_wgrad_bf16(d.Gp, d.ldg, d.Ap, d.lda, _ptr(dWb), d.lddw, _ptr(dbb), p["rows"], d.Nw, d.Kw, _ptr(ws), pl.have,
                                    ctx.stream())
    else:
        rc = ctx.lib.aim_wgrad_bias_bf16(d.Gp, d.ldg, d.Ap, d.lda, _ptr(dWb), d.lddw, _ptr(dbb), _ptr(atb), ntok, p["rows"], d.Nw, d.Kw,
                                         _ptr(ws), pl.have, ctx.stream())
    ctx.check(rc, "aim_wgrad_bias_bf16")
    got, pad = d.take(dWb, dbb)
    if ws is not None:
        used = pl.C * d.Nw * (d.Kw + (1 if pl.bias == "fused" else 0)) if pl.mode == "slabs" else 0
        h = ws.cpu()
        pad["ws"] = _all_nan(h[used:]) and bool(torch.isfinite(h[:pl.C * d.Nw * d.Kw if used else 0]).all())
    return got, pad


def _slabs_call(ctx, d, mb, me, mc, slabs, bslabs, Nw=None, Kw=None):
    n = ctx.c_int(-1)
    rc = ctx.lib.aim_wgrad_slabs_bf16(d.Gp, d.ldg, d.Ap, d.lda, _ptr(d.at) if bslabs is not None else None,
                                      d.ntok if bslabs is not None else 0, mb, me, Nw or d.Nw, Kw or d.Kw, slabs, bslabs, mc,
                                      ctx.byref(n), ctx.stream())
    ctx.check(rc, "aim_wgrad_slabs_bf16")
    return n.value


def _finish(ctx, d, slabs, bslabs, n, Nw=None, Kw=None):
    dWb, dbb = d.dW(Nw, Kw), (d.db() if bslabs is not None else None)
    ctx.check(ctx.lib.aim_wgrad_finish(_ptr(slabs), _ptr(bslabs), n, _ptr(dWb), d.lddw, _ptr(dbb), Nw or d.Nw, Kw or d.Kw, ctx.stream()),
              "aim_wgrad_finish")
    return d.take(dWb, dbb, Nw, Kw)


def _slabs_once(ctx, case, d, ranges, Nw=None, Kw=None):
    """the slabs entry over `ranges`, one call each into consecutive slabs, then one finish -> (got, pad, chunks written per call)"""
    Nw, Kw = Nw or d.Nw, Kw or d.Kw
    tiles = tiles_of(Nw, Kw)
    cap = sum((range_chunks(me - mb, mc) if mc > 0 else wgrad_chunks(me - mb, tiles, TARGET[ctx.route]))[0] for mb, me, mc in ranges)
    slabs = ctx.nan((cap + 1) * Nw * Kw)
    bslabs = ctx.nan((cap + 1) * Nw) if case.p["bias"] != "none" else None
    n, written = 0, []
    for mb, me, mc in ranges:
        w = _slabs_call(ctx, d, mb, me, mc, _ptr(slabs, n * Nw * Kw), _ptr(bslabs, n * Nw), Nw, Kw)
        written.append(w)
        n += w
    got, pad = _finish(ctx, d, slabs, bslabs, n, Nw, Kw)
    pad["slabs"] = _all_nan(slabs[n * Nw * Kw:]) and bool(torch.isfinite(slabs[:n * Nw * Kw]).all())
    if bslabs is not None:
        pad["bias_slabs"] = _all_nan(bslabs[n * Nw:]) and bool(torch.isfinite(bslabs[:n * Nw]).all())
    return got, pad, written, (slabs, bslabs)


def _same(a, b, keys=None):
    return all(_bits_eq(a[k], b[k]) for k in (keys or a))


def run_entry(ctx, case, inp, rec):
    pl, p = plan(case, ctx.route), case.p
    d = _Dev(ctx, case, inp)
    rec["mirror"]["workspace_bytes"] = int(ctx.lib.aim_wgrad_workspace_bytes(p["rows"], d.Nw, d.Kw)) == pl.need
    got, pad = _entry_once(ctx, case, d, pl)
    # what a second run must reproduce: not fp32 atomics over several chunks, not aim_colsum_bf16's atomic route
    keys = [k for k in got if not (k == "dW" and pl.mode == "atomics")]
    if pl.bias == "colsum" and rw.colsum_plan(_colsum_twin(case, inp)[0].p)[0] == "atomic8":
        keys.remove("db")
    if keys:
        rec["ident"]["repeat"] = _same(got, _entry_once(ctx, case, d, pl)[0], keys)
        if p["bias"] != "at":
            rec["ident"]["plain_eq_bias"] = _same(got, _entry_once(ctx, case, d, pl, plain=True)[0], keys)
        if p["bias"] == "db":
            ones = ctx.put(torch.ones(197))
            rec["ident"]["ones_eq_null"] = _same(got, _entry_once(ctx, case, d, pl, at=ones)[0], keys)
        if pl.mode != "atomics" and pl.bias != "colsum" and pl.finish == "v":
            g2, _, written, _ = _slabs_once(ctx, case, d, [(0, p["rows"], 0)])
            rec["ident"]["slabs_eq_entry"] = _same(got, g2)
            rec["mirror"]["chunks_written"] = written == [pl.C]
    return got, pad


def run_slabs(ctx, case, inp, rec):
    pl, p = plan(case, ctx.route), case.p
    d = _Dev(ctx, case, inp)
    got, pad, written, _ = _slabs_once(ctx, case, d, p["ranges"])
    rec["mirror"]["chunks_written"] = written == [c for c, _ in pl.calls]
    rec["ident"]["repeat"] = _same(got, _slabs_once(ctx, case, d, p["ranges"])[0])
    if p.get("tile_alone"):
        alone = _slabs_once(ctx, case, d, p["ranges"], TILE, TILE)[0]
        rec["ident"]["tile_alone"] = _bits_eq(got["dW"][:TILE, :TILE].contiguous(), alone["dW"]) and \
            _bits_eq(got["db"][:TILE].contiguous(), alone["db"])
    return got, pad


def _host(ctx, hid):
    """the host GEMM's operands and its output WITHOUT riders (computed once)"""
    if hid in ctx.hosts:
        return ctx.hosts[hid]
    ops, dev = ctx.ops, ctx.dev
    g = torch.Generator().manual_seed(900 + ord(hid))
    M, N, K = (4352, 4096, 64) if hid == "c" else (2048, 768, 256)
    a = torch.randn((M, K), generator=g).to(BF16).to(dev)
    w = (torch.randn((N, K), generator=g) * K ** -0.5).to(BF16).to(dev)
    kw, epi = {}, ops.EPI_BF16
    if hid == "b":          # the backward launch backbone.py makes: DACT from the fragment-ordered derivative the ACT launch saved
        x = torch.randn((M, K), generator=g).to(BF16).to(dev)
        w1 = (torch.randn((N, K), generator=g) * K ** -0.5).to(BF16).to(dev)
        fb = ops.frag_buffer(M, N, dev)
        post = torch.empty((M, N), dtype=BF16, device=dev)
        ops.gemm(x, w1, ops.EPI_ACT, post, out2=fb, act=ops.ACT_QGELU, aux_grad=True, aux_frag=True)
        at = ((torch.rand(197, generator=g) < 0.7).float() / 0.7).to(dev)
        kw, epi = dict(aux=fb, aux_grad=True, aux_frag=True, act=ops.ACT_QGELU, at=at, ntok=197), ops.EPI_DACT
    if hid == "d":
        kw = dict(reserve_cus=16)
    out = torch.empty((M, N), dtype=BF16, device=dev)
    ops.gemm(a, w, epi, out, **kw)
    torch.cuda.synchronize()
    tiles = _cdiv(M, 256) * _cdiv(N, 256)
    info = {"tiles": tiles, "grid": balanced_grid(tiles, ctx.cus, kw.get("reserve_cus", 0)),
            "peel_rows": peel_rows(M, N, ctx.cus, kw.get("reserve_cus", 0)) if epi == ops.EPI_BF16 else 0}
    ctx.hosts[hid] = (a, w, epi, kw, out, info)
    return ctx.hosts[hid]


def ride_args(ctx, d, mb, me, chunks, slabs, bslabs, **over):
    ra = ctx.WgradRideArgs()
    ra.G, ra.A, ra.ldg, ra.lda, ra.Nw, ra.Kw = d.Gp, d.Ap, d.ldg, d.lda, d.Nw, d.Kw
    ra.m_begin, ra.m_end, ra.chunks = mb, me, chunks
    ra.at, ra.ntok = (_ptr(d.at), d.ntok) if bslabs is not None else (None, 0)
    ra.slabs, ra.bias_slabs = _ptr(slabs), _ptr(bslabs)
    for k, v in over.items():
        setattr(ra, k, v)
    return ra


def run_ride(ctx, case, inp, rec):
    pl, p = plan(case, ctx.route), case.p
    a, w, epi, kw, out_ref, info = _host(ctx, p["host"])
    rec["host"] = info
    if info["peel_rows"]:
        rec["refused"] = (f"host {p['host']} would be peeled on {ctx.cus} CUs (aim_gemm_peel_rows = {info['peel_rows']}): "
                          "it cannot host riders")
        return None, None
    d = _Dev(ctx, case, inp)
    Nw, Kw, C = d.Nw, d.Kw, pl.C

    def once():
        slabs = ctx.nan((C + 1) * Nw * Kw)
        bslabs = ctx.nan((C + 1) * Nw) if p["bias"] != "none" else None
        out = ctx.nan(out_ref.numel(), BF16)
        ra = ride_args(ctx, d, p["mb"], p["me"], p["chunks"], slabs, bslabs)
        ctx.ops.gemm(a, w, epi, out[:out_ref.numel()].view(out_ref.shape), ride=ra, **kw)
        got, pad = _finish(ctx, d, slabs, bslabs, ra.written)
        pad["host_out"] = _all_nan(out[out_ref.numel():])
        pad["slabs"] = _all_nan(slabs[ra.written * Nw * Kw:]) and bool(torch.isfinite(slabs[:ra.written * Nw * Kw]).all())
        if bslabs is not None:
            pad["bias_slabs"] = _all_nan(bslabs[ra.written * Nw:]) and bool(torch.isfinite(bslabs[:ra.written * Nw]).all())
        return got, pad, ra.written, out, slabs, bslabs

    got, pad, written, out, slabs, bslabs = once()
    rec["mirror"]["chunks_written"] = written == C
    rec["ident"]["host_out"] = _bits_eq(out[:out_ref.numel()], out_ref.reshape(-1))
    again = once()
    rec["ident"]["repeat"] = _same(got, again[0]) and _bits_eq(slabs, again[4])
    _, _, sw, (s2, b2) = _slabs_once(ctx, case, d, [(p["mb"], p["me"], p["chunks"])])
    rec["ident"]["rider_eq_slabs"] = sw == [written] and _bits_eq(slabs[:C * Nw * Kw], s2[:C * Nw * Kw]) and \
        (bslabs is None or _bits_eq(bslabs[:C * Nw], b2[:C * Nw]))
    return got, pad


def run_case(ctx, case):
    rec = {"kind": case.kind, "checks": {}, "finite": {}, "pad": {}, "ident": {}, "hash": {}, "mirror": {}}
    pl = plan(case, ctx.route)
    rec["plan"] = {"C": pl.C, "S": pl.S, "mode": pl.mode, "bias": pl.bias, "finish": pl.finish, "path": pl.path}
    inp = build_inputs(case)
    got, pad = {"entry": run_entry, "slabs": run_slabs, "ride": run_ride}[case.kind](ctx, case, inp, rec)
    if got is None:
        return rec
    rec["checks"] = compare(case, inp, got, ctx.route)
    rec["finite"] = {k: bool(torch.isfinite(v).all()) for k, v in got.items()}
    rec["pad"] = pad
    rec["hash"] = {k: _digest(v) for k, v in got.items()}
    return rec


# ---- refusals: name -> the text of the AIM_CHECK_ARG that must answer (test_wgrad_cases_cpu.py holds them to the sources) -----
_E, _S, _F, _R = "wgrad: ", "wgrad_slabs: ", "wgrad_finish: ", "gemm_ride: "
REFUSAL_TEXT = {
    "entry/Nw12": _E + "Nw/Kw must be positive multiples of 8", "entry/Kw20": _E + "Nw/Kw must be positive multiples of 8",
    "entry/ldg%8": _E + "ldg/lda must be multiples of 8, lddw of 4", "entry/lda%8": _E + "ldg/lda must be multiples of 8, lddw of 4",
    "entry/lddw%4": _E + "ldg/lda must be multiples of 8, lddw of 4",
    "entry/ldg<Nw": _E + "ldg/lda/lddw must cover a row", "entry/lda<Kw": _E + "ldg/lda/lddw must cover a row",
    "entry/null_G": _E + "null pointer", "entry/null_A": _E + "null pointer", "entry/null_dW": _E + "null pointer",
    "entry/at_without_db": _E + "row factors need db", "entry/ntok0": _E + "row factors need db",
    "entry/ntok4097": _E + "row factors need db",
    "slabs/Nw12": _S + "Nw/Kw must be positive multiples of 8", "slabs/Kw20": _S + "Nw/Kw must be positive multiples of 8",
    "slabs/ldg%8": _S + "ldg/lda must be multiples of 8", "slabs/lda%8": _S + "ldg/lda must be multiples of 8",
    "slabs/ldg<Nw": _S + "ldg/lda must cover a row", "slabs/lda<Kw": _S + "ldg/lda must cover a row",
    "slabs/null_G": _S + "null pointer", "slabs/null_A": _S + "null pointer", "slabs/null_slabs": _S + "null pointer",
    "slabs/null_chunks_written": _S + "null pointer",
    "slabs/at_without_bias_slabs": _S + "row factors need bias slabs", "slabs/ntok0": _S + "row factors need bias slabs",
    "slabs/ntok4097": _S + "row factors need bias slabs",
    "slabs/m_end==m_begin": _S + "empty row range", "slabs/m_end<m_begin": _S + "empty row range",
    "finish/0chunks": _F + "null pointer or no slabs", "finish/null_slabs": _F + "null pointer or no slabs",
    "finish/null_dW": _F + "null pointer or no slabs", "finish/lddw%4": _F + "Nw/Kw multiples of 8, lddw of 4",
    "finish/bias_slabs_only": _F + "bias slabs and db go together", "finish/db_only": _F + "bias slabs and db go together",
    "ride/act": _R + "this launch cannot host riders", "ride/M512": _R + "this launch cannot host riders",
    "ride/small_tile": _R + "this launch cannot host riders", "ride/row0": _R + "this launch cannot host riders",
    "ride/ldg<Nw": _R + "ldg/lda must be multiples of 8 and cover a row", "ride/chunks0": _R + "empty row range or no chunks",
    "ride/ntok4097": _R + "row factors need bias slabs", "ride/at_without_bias_slabs": _R + "row factors need bias slabs",
    "ride/null_slabs": _R + "null pointer",
}


def run_refusals(ctx):
    """calls the library must refuse: {name: {message, every output still NaN}}"""
    dev, lib, out = ctx.dev, ctx.lib, {}
    M, Nw, Kw = 40, 16, 24
    G = torch.ones((M, 32), dtype=BF16, device=dev)
    A = torch.ones((M, 32), dtype=BF16, device=dev)
    at = torch.ones(4104, device=dev)
    dW, db, ws = ctx.nan(Nw * 32), ctx.nan(Nw), ctx.nan(4 * Nw * 32)
    slabs, bslabs = ctx.nan(4 * Nw * 32), ctx.nan(4 * Nw)
    watched = [dW, db, ws, slabs, bslabs]

    def attempt(name, rc):
        msg = lib.aim_last_error() if rc != 0 else None
        torch.cuda.synchronize()
        out[name] = {"rc": rc, "message": msg.decode() if msg else None, "untouched": all(_all_nan(t) for t in watched)}

    def entry(name, **o):
        a = dict(G=_ptr(G), ldg=32, A=_ptr(A), lda=32, dW=_ptr(dW), lddw=Kw, db=_ptr(db), at=None, ntok=0, M=M, Nw=Nw, Kw=Kw)
        a.update(o)
        attempt("entry/" + name, lib.aim_wgrad_bias_bf16(a["G"], a["ldg"], a["A"], a["lda"], a["dW"], a["lddw"], a["db"], a["at"],
                                                         a["ntok"], a["M"], a["Nw"], a["Kw"], _ptr(ws), 4 * Nw * 32 * 4, ctx.stream()))

    entry("Nw12", Nw=12)
    entry("Kw20", Kw=20, lddw=20)
    entry("ldg%8", ldg=28)
    entry("lda%8", lda=28)
    entry("lddw%4", lddw=26)
    entry("ldg<Nw", ldg=8)
    entry("lda<Kw", lda=16)
    entry("null_G", G=None)
    entry("null_A", A=None)
    entry("null_dW", dW=None)
    entry("at_without_db", at=_ptr(at), ntok=5, db=None)
    entry("ntok0", at=_ptr(at), ntok=0)
    entry("ntok4097", at=_ptr(at), ntok=4097)

    n = ctx.c_int(-1)

    def slab(name, **o):
        a = dict(G=_ptr(G), ldg=32, A=_ptr(A), lda=32, at=None, ntok=0, mb=3, me=M, Nw=Nw, Kw=Kw, slabs=_ptr(slabs), bslabs=_ptr(bslabs),
                 n=ctx.byref(n))
        a.update(o)
        attempt("slabs/" + name, lib.aim_wgrad_slabs_bf16(a["G"], a["ldg"], a["A"], a["lda"], a["at"], a["ntok"], a["mb"], a["me"], a["Nw"],
                                                          a["Kw"], a["slabs"], a["bslabs"], 2, a["n"], ctx.stream()))

    slab("Nw12", Nw=12)
    slab("Kw20", Kw=20)
    slab("ldg%8", ldg=28)
    slab("lda%8", lda=28)
    slab("ldg<Nw", ldg=8)
    slab("lda<Kw", lda=16)
    slab("null_G", G=None)
    slab("null_A", A=None)
    slab("null_slabs", slabs=None)
    slab("null_chunks_written", n=None)
    slab("at_without_bias_slabs", at=_ptr(at), ntok=5, bslabs=None)
    slab("ntok0", at=_ptr(at), ntok=0)
    slab("ntok4097", at=_ptr(at), ntok=4097)
    slab("m_end==m_begin", mb=7, me=7)
    slab("m_end<m_begin", mb=9, me=7)

    src = torch.zeros(4 * Nw * 32, device=dev)

    def fin(name, **o):
        a = dict(slabs=_ptr(src), bslabs=_ptr(src), n=2, dW=_ptr(dW), lddw=Kw, db=_ptr(db))
        a.update(o)
        attempt("finish/" + name, lib.aim_wgrad_finish(a["slabs"], a["bslabs"], a["n"], a["dW"], a["lddw"], a["db"], Nw, Kw, ctx.stream()))

    fin("0chunks", n=0)
    fin("null_slabs", slabs=None)
    fin("null_dW", dW=None)
    fin("lddw%4", lddw=26)
    fin("bias_slabs_only", db=None)
    fin("db_only", bslabs=None)

    # riders: a host that could carry them, and each reason why one cannot
    ops = ctx.ops
    hM, hN, hK = 2048, 768, 256
    ha = torch.zeros((hM, hK), dtype=BF16, device=dev)
    hw = torch.zeros((hN, hK), dtype=BF16, device=dev)
    hout = ctx.nan(hM * hN, BF16)
    hout2 = ctx.nan(hM * hN, BF16)
    watched += [hout, hout2]

    def ride(name, epi=ops.EPI_BF16, Mh=hM, host=None, **o):
        g = ctx.GemmArgs()
        g.A, g.W, g.M, g.N, g.K, g.lda, g.ldw = _ptr(ha), _ptr(hw), Mh, hN, hK, hK, hK
        g.out, g.ldo, g.out2, g.ldo2 = _ptr(hout), hN, _ptr(hout2), hN
        for k, v in (host or {}).items():
            setattr(g, k, v)
        ra = ctx.WgradRideArgs()
        ra.G, ra.A, ra.ldg, ra.lda, ra.Nw, ra.Kw, ra.m_begin, ra.m_end, ra.chunks = _ptr(G), _ptr(A), 32, 32, Nw, Kw, 3, M, 2
        ra.slabs, ra.bias_slabs = _ptr(slabs), _ptr(bslabs)
        for k, v in o.items():
            setattr(ra, k, v)
        attempt("ride/" + name, lib.aim_gemm_bf16_ride(ctx.byref(g), epi, ctx.byref(ra), ctx.byref(n), ctx.stream()))

    ride("act", epi=ops.EPI_ACT)
    ride("M512", Mh=512)
    ride("small_tile", host=dict(small_tile=1))
    ride("row0", host=dict(row0=256))
    ride("ldg<Nw", ldg=8)
    ride("chunks0", chunks=0)
    ride("ntok4097", at=_ptr(at), ntok=4097)
    ride("at_without_bias_slabs", at=_ptr(at), ntok=5, bias_slabs=None)
    ride("null_slabs", slabs=None)
    return out


def run(route: str):
    """every case of `route` and (on `default`) the refusals: {"cases": {name: record}, "errors", "refusals", "seconds"}"""
    from ctypes import byref, c_int
    ctx = _Ctx(route)
    ctx.byref, ctx.c_int = byref, c_int
    t0 = time.time()
    res = {"route": route, "cus": ctx.cus, "cases": {}, "errors": {}, "refusals": {}}

    def guarded(name, fn):
        try:
            return fn()
        except Exception as e:      # a refused or failed call is a finding of the test; after a GPU fault nothing more runs
            res["errors"][name] = f"{type(e).__name__}: {e}"
            if any(s in str(e) for s in _FATAL):
                res["fatal"] = name
            return None

    with torch.no_grad():
        for case in cases():
            if not runs_on(case, route):
                continue
            rec = guarded(case.name, lambda: run_case(ctx, case))
            if "fatal" in res:
                return res
            if rec is not None:
                res["cases"][case.name] = rec
        if route == "default":
            ref = guarded("refusals", lambda: run_refusals(ctx))
            if ref is not None:
                res["refusals"] = ref
    res["seconds"] = time.time() - t0
    return res


def main(argv):
    route, path = argv
    res = run(route)
    with open(path, "w") as f:
        json.dump(res, f)
    if "fatal" in res:
        print(f"{res['fatal']}: {res['errors'][res['fatal']]}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
