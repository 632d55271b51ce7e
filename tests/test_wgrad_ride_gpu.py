"""Rider workgroups of the persistent GEMM (aim_gemm_bf16_ride): an adapter weight gradient summed by extra workgroups of a
dgrad GEMM launch, against an fp64 product of the same bf16 operands.

Host: M = 2 048, N = 768, K = 256 (24 tiles: the persistent kernel with a 24-workgroup grid), BF16 and DACT epilogues.
Gradients: [768 x 192] and [192 x 768] (three 256 x 256 tiles each) over rows of a 1 000-row problem, with the strided operand
the model has (a column slice of a 3 264-wide tensor).  The rider count is explicit here; the policy is tested at model level
(test_wgrad_ride_model_gpu.py).

Bound: test_kernels_gpu.py::test_wgrad's -- atol 2e-5 * sqrt(rows) * 4 + 1e-4, rtol 1e-4 -- with the fp64 reference.
Measured: largest |error| 4.6e-5 (dW) and 1.3e-5 (db) against bounds of 9e-4 .. 2.6e-3.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MW, NTOK = 1000, 197
GUARD = 1024            # floats / elements of sentinel around every buffer the launch writes
SENT = -7777.0


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def close(got, ref, atol, rtol, what=""):
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} elements off; max err {err.max().item():.4e} "
                           f"(ref max {ref.abs().max().item():.3e}) at {torch.nonzero(bad)[0].tolist()}")


def guarded(shape, dtype):
    """A tensor of `shape` inside a sentinel-filled allocation: (view, whole allocation, offset)."""
    n = math.prod(shape)
    whole = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(shape), whole


def guards_intact(whole):
    return bool((whole[:GUARD] == SENT).all() and (whole[-GUARD:] == SENT).all())


_HOST = {}


def host(epi_name):
    """The host GEMM's operands and its output WITHOUT riders (computed once per epilogue)."""
    if epi_name not in _HOST:
        from aim_amd import ops
        M, N, K = 2048, 768, 256
        a, w = rnd((M, K), 1, 1.0, torch.bfloat16), rnd((N, K), 2, 0.05, torch.bfloat16)
        kw = {}
        if epi_name == "dact":
            kw = dict(aux=rnd((M, N), 3, 1.0, torch.bfloat16), act=ops.ACT_QGELU, at=rnd((NTOK,), 4).abs(), ntok=NTOK)
        epi = ops.EPI_DACT if epi_name == "dact" else ops.EPI_BF16
        out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
        ops.gemm(a, w, epi, out, **kw)
        _HOST[epi_name] = (a, w, epi, kw, out)
    return _HOST[epi_name]


_PROBLEM = {}


def problem(shape):
    """G, A of the gradient (one of them a column slice of a 3 264-wide tensor, as dcat[:, H4:] / hcat[:, H4:]), `at`."""
    if shape not in _PROBLEM:
        Nw, Kw = shape
        wide = rnd((MW, 3264), 10 + Nw, 1.0, torch.bfloat16)
        if Nw == 192:       # D_fc1: G = dcat[:, 3072:], A = xn
            g, a = wide[:, 3072:], rnd((MW, Kw), 11, 1.0, torch.bfloat16)
        else:               # D_fc2: G = dyb, A = hcat[:, 3072:]
            g, a = rnd((MW, Nw), 12, 1.0, torch.bfloat16), wide[:, 3072:]
        at = ((torch.rand(NTOK, generator=torch.Generator().manual_seed(13)) < 0.7).float() / 0.7).to(DEV)
        _PROBLEM[shape] = (g, a, at)
    return _PROBLEM[shape]


def reference(g, a, at, mb, me):
    gd, ad = g[mb:me].double(), a[mb:me].double()
    rs = at.double()[torch.arange(mb, me, device=DEV) % NTOK] if at is not None else torch.ones(me - mb, dtype=torch.float64, device=DEV)
    return gd.T @ ad, (gd * rs[:, None]).sum(0)


# (epilogue, (Nw, Kw), m_begin, m_end, chunks asked, slabs expected, at?)
CASES = [
    ("bf16", (768, 192), 37, 650, 4, 4, True),       # starts off 0 / off a multiple of ntok, 613 rows: not a multiple of 32
    ("dact", (192, 768), 37, 650, 4, 4, False),      # bias without `at`, strided G
    ("dact", (768, 192), 0, 100, 7, 4, True),        # more chunks than 32-row steps: 4 steps -> 4 slabs, 3 empty chunks
    ("bf16", (192, 768), 300, 1000, 1, 1, True),     # one chunk per tile
    ("bf16", (768, 192), 0, 1000, 3, 3, False),      # the whole problem, bias without `at`
]


@pytest.mark.parametrize("epi_name,shape,mb,me,chunks,expect,use_at", CASES)
def test_riders(epi_name, shape, mb, me, chunks, expect, use_at):
    from aim_amd import ops
    a_h, w_h, epi, kw, out_ref = host(epi_name)
    g, a, at = problem(shape)
    at = at if use_at else None
    Nw, Kw = shape
    dw0, db0 = rnd((Nw, Kw), 20), rnd((Nw,), 21)
    results = []
    for _ in range(2):
        slabs, slabs_all = guarded((chunks, Nw, Kw), torch.float32)
        bslabs, bslabs_all = guarded((chunks, Nw), torch.float32)
        out, out_all = guarded(tuple(out_ref.shape), torch.bfloat16)
        ra = ops.ride_args(g, a, mb, me, chunks, slabs, bslabs, at=at, ntok=NTOK if use_at else 0)
        ops.gemm(a_h, w_h, epi, out, ride=ra, **kw)
        assert ra.written == expect
        dw, db = dw0.clone(), db0.clone()
        ops.wgrad_finish(slabs, ra.written, dw, bslabs, db)
        torch.cuda.synchronize()
        assert torch.equal(out, out_ref), "the host's output changed under riders"
        assert guards_intact(out_all) and guards_intact(slabs_all) and guards_intact(bslabs_all)
        assert bool((slabs[ra.written:] == SENT).all() and (bslabs[ra.written:] == SENT).all()), "an empty chunk wrote"
        results.append((dw, db))
    rw, rb = reference(g, a, at, mb, me)
    tol = 2e-5 * math.sqrt(me - mb) * 4 + 1e-4
    print(f"max |dW err| {(results[0][0].double() - dw0.double() - rw).abs().max().item():.3e}  "
          f"max |db err| {(results[0][1].double() - db0.double() - rb).abs().max().item():.3e}  bound atol {tol:.3e}")
    close(results[0][0], dw0.double() + rw, tol, 1e-4, "dW")
    close(results[0][1], db0.double() + rb, tol, 1e-4, "db")
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "not reproducible"


@pytest.mark.parametrize("shape", [(768, 192), (192, 768)])
def test_riders_and_stand_alone_share_slabs(shape):
    """Rows [0, 420) on riders, [420, 1000) through the stand-alone launch behind them; one finish sums all slabs."""
    from aim_amd import ops
    a_h, w_h, epi, kw, out_ref = host("dact")
    g, a, at = problem(shape)
    Nw, Kw = shape
    cap, cut = 8, 420
    dw0, db0 = rnd((Nw, Kw), 30), rnd((Nw,), 31)
    results = []
    for _ in range(2):
        slabs, slabs_all = guarded((cap, Nw, Kw), torch.float32)
        bslabs, bslabs_all = guarded((cap, Nw), torch.float32)
        out = torch.empty_like(out_ref)
        ra = ops.ride_args(g, a, 0, cut, 2, slabs, bslabs, at=at, ntok=NTOK)
        ops.gemm(a_h, w_h, epi, out, ride=ra, **kw)
        n = ra.written
        n += ops.wgrad_slabs(g, a, cut, MW, slabs[n:], bslabs[n:], at=at, ntok=NTOK, max_chunks=3)
        assert n == 5
        dw, db = dw0.clone(), db0.clone()
        ops.wgrad_finish(slabs, n, dw, bslabs, db)
        torch.cuda.synchronize()
        assert torch.equal(out, out_ref)
        assert guards_intact(slabs_all) and guards_intact(bslabs_all)
        assert bool((slabs[n:] == SENT).all() and (bslabs[n:] == SENT).all())
        results.append((dw, db))
    rw, rb = reference(g, a, at, 0, MW)
    tol = 2e-5 * math.sqrt(MW) * 4 + 1e-4
    close(results[0][0], dw0.double() + rw, tol, 1e-4, "dW")
    close(results[0][1], db0.double() + rb, tol, 1e-4, "db")
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_stand_alone_entry_keeps_its_bits():
    """aim_wgrad_bias_bf16 through the shared device function: the slabs entry over the whole problem, with the library's own
    chunking, sums to the same bits."""
    from aim_amd import ops
    g, a, at = problem((768, 192))
    dw0, db0 = rnd((768, 192), 40), rnd((768,), 41)
    dw1, db1 = dw0.clone(), db0.clone()
    ops.wgrad(g, a, dw1, db1, at=at, ntok=NTOK)
    slabs = torch.empty((96, 768, 192), dtype=torch.float32, device=DEV)
    bslabs = torch.empty((96, 768), dtype=torch.float32, device=DEV)
    n = ops.wgrad_slabs(g, a, 0, MW, slabs, bslabs, at=at, ntok=NTOK)
    dw2, db2 = dw0.clone(), db0.clone()
    ops.wgrad_finish(slabs, n, dw2, bslabs, db2)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


def test_plan_rejects_what_cannot_ride():
    """The policy from shapes alone: no spare CUs, a host too short for half the gradient, a token table too large."""
    from ctypes import byref, c_int
    from aim_amd import ops
    from aim_amd.lib import GemmArgs, load_library
    lib = load_library()

    def plan(M, N, K, epi, Nw, Kw, ntok, rows):
        g = GemmArgs()
        g.M, g.N, g.K, g.lda, g.ldw, g.ldo, g.ldaux = M, N, K, K, K, N, N
        ch, rw = c_int(-1), c_int(-1)
        assert lib.aim_wgrad_ride_plan(byref(g), epi, Nw, Kw, ntok, rows, rows, byref(ch), byref(rw)) == 0
        return ch.value, rw.value

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus == 256:
        # ViT-L/14, 8 clips x 8 frames x 257 tokens... the DACT launch of 131 584 rows: 6 spare CUs, 4 tiles, a fifth of the rows
        assert plan(131584, 4096 + 256, 1024, ops.EPI_DACT, 1024, 256, 257, 131584) == (0, 0)
        # the flagship's DACT launch takes D_fc2
        ch, rw = plan(100864, 3264, 768, ops.EPI_DACT, 768, 192, 197, 100864)
        assert ch == 4 and rw * 2 >= 100864
    assert plan(2048, 768, 256, ops.EPI_BF16, 768, 192, 197, 1000) == (0, 0)            # one round of 7 steps: too short to host
    assert plan(100864, 3264, 768, ops.EPI_DACT, 768, 192, 5000, 100864) == (0, 0)      # 20 000-byte table: no room in LDS
    assert plan(100864, 3264, 768, ops.EPI_ACT, 768, 192, 197, 100864) == (0, 0)        # not a hosting epilogue
