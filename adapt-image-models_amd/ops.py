"""Thin tensor-level wrappers over the C ABI (include/aim_kernels.h).

PyTorch is used for device memory and streams only; every function here launches exactly the HIP
kernel(s) of the same name on the current stream and returns without synchronising.
"""
from ctypes import byref, c_int
from typing import Optional

import torch

from .lib import GemmArgs, LowrankArgs, WgradRideArgs, check, load_library

EPI_BF16, EPI_ACT, EPI_DACT, EPI_F32, EPI_EXPSUM, EPI_ACT8, EPI_RES16 = 0, 1, 2, 3, 4, 5, 6
FP8 = torch.float8_e4m3fn          # OCP e4m3 (gfx950); stored as bytes
ACT_QGELU, ACT_GELU = 0, 1

BF16 = torch.bfloat16
F32 = torch.float32


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The raw hipStream_t of torch's current stream on the current device.  (`torch.cuda.current_stream()` builds a Stream
    object behind several Python-level device lookups: 8 us a call, 5 ms per forward at one sample x 3 views of ViT-L/14.)"""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(_RAW_DEVICE())
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event timing of the large GEMM launches (bench.py roofline leg).  Events are
    recorded on the stream the kernel is launched on; durations are read after the timed region."""

    def __init__(self, min_flops: float = 1e10):
        self.min_flops = min_flops
        self.enabled = False
        self.records = []          # (epi, flops, start_event, end_event)

    def start(self):
        self.records, self.enabled = [], True

    def stop(self):
        self.enabled = False

    def summary(self):
        """-> {epi: dict(launches, flops, ms)} ; call after torch.cuda.synchronize()."""
        out = {}
        for epi, fl, e0, e1 in self.records:
            d = out.setdefault(epi, dict(launches=0, flops=0.0, ms=0.0))
            d["launches"] += 1
            d["flops"] += fl
            d["ms"] += e0.elapsed_time(e1)
        return out


GEMM_TIMER = KernelTimer()


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: Optional[torch.Tensor], dtype, name: str):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")


def frag_elems(M: int, N: int) -> int:
    """Elements of the fragment-ordered side buffer of an ``[M, N]`` ACT / DACT pair (aim_gemm_args.aux_frag)."""
    return ((M + 255) // 256) * ((N + 255) // 256) * 65536


def frag_buffer(M: int, N: int, device) -> torch.Tensor:
    return torch.empty((frag_elems(M, N),), dtype=BF16, device=device)


def gemm(a: torch.Tensor, w: torch.Tensor, epi: int, out: torch.Tensor, *, bias=None, resid=None,
         af=None, at=None, vec=None, bt=None, ntok: int = 0, aux=None, out2=None, act: int = 0,
         scale: float = 1.0, rs_bias_only: bool = False, batch: int = 1, stride_a: int = 0,
         stride_w: int = 0, M: Optional[int] = None, N: Optional[int] = None, K: Optional[int] = None,
         lda: Optional[int] = None, ldw: Optional[int] = None, ldv: Optional[int] = None, n_split: int = 0,
         act2: int = 0, xrow=None, reserve_cus: int = 0, probe=None, aux_grad: bool = False, aux_frag: bool = False,
         slot_stride: int = 0, small_tile: bool = False, ride=None):
    """``out = epilogue(a @ w.T)``; ``a`` is ``[M, K]`` (row stride ``lda``), ``w`` is ``[N, K]``.
    ``ride``: a list of ``WgradRide`` objects -- the launch may carry rider workgroups for one of them, as the library's
    policy decides -- or one ``ride_args(...)``: the launch carries exactly those riders (``.written`` = slabs filled)."""
    lib = load_library()
    _chk(a, BF16, "a"); _chk(w, BF16, "w")
    for n_, t_ in (("bias", bias), ("resid", resid), ("af", af), ("at", at), ("vec", vec), ("bt", bt)):
        _chk(t_, F32, n_)
    _chk(aux, BF16, "aux"); _chk(out2, BF16, "out2")
    g = GemmArgs()
    g.A, g.W = a.data_ptr(), w.data_ptr()
    g.M = a.shape[0] if M is None else M
    g.K = a.shape[1] if K is None else K
    g.N = w.shape[0] if N is None else N
    g.lda = a.stride(0) if lda is None else lda
    g.ldw = w.stride(0) if ldw is None else ldw
    g.strideA, g.strideW = stride_a, stride_w
    g.bias, g.resid = _p(bias), _p(resid)
    g.ldr = resid.stride(0) if resid is not None else 0
    g.af, g.at, g.vec, g.bt = _p(af), _p(at), _p(vec), _p(bt)
    g.ldv = (vec.stride(0) if ldv is None else ldv) if vec is not None else 0
    g.ntok = ntok
    g.aux = _p(aux)
    g.ldaux = aux.stride(0) if aux is not None else 0
    g.out = out.data_ptr()
    # EXPSUM: ldo = float stride between the (max, sum) slot groups of consecutive batch items (0: packed, expsum_tiles pairs
    # per item; 16 | 32 floats on the one-tile-per-item path)
    g.ldo = (out.stride(0) if out.dim() >= 2 else 0) if epi != EPI_EXPSUM else int(slot_stride)
    g.out2 = _p(out2)
    g.ldo2 = out2.stride(0) if out2 is not None else 0
    g.scale, g.act, g.rs_bias_only = scale, act, int(rs_bias_only)
    g.n_split, g.act2 = n_split, act2
    _chk(xrow, BF16, "xrow")
    g.xrow = _p(xrow)
    g.ldx = xrow.stride(0) if xrow is not None else 0
    g.reserve_cus = int(reserve_cus)       # per-call: CUs this persistent launch leaves to other streams
    g.aux_grad = int(bool(aux_grad))       # ACT: out2 = act'(pre) instead of pre; DACT: aux holds act'(pre)
    g.small_tile = int(bool(small_tile))   # the 64 x 64 kernel at any M: the large kernel's K order (aim_gemm_args.small_tile)
    g.aux_frag = int(bool(aux_frag))       # ACT / DACT: out2 / aux is a fragment-ordered buffer (frag_buffer)
    if aux_frag:
        t_ = out2 if epi == EPI_ACT else aux
        if epi not in (EPI_ACT, EPI_DACT) or batch != 1 or g.M < 1024 or t_ is None or not t_.is_contiguous() \
                or t_.numel() < frag_elems(g.M, g.N):
            raise ValueError("aux_frag: ACT / DACT on the large-tile kernel (M >= 1024, batch 1) with a frag_buffer(M, N)")
        g.ldo2 = g.ldaux = 0               # (no row stride: the buffer is fragment-ordered)
    if probe is not None:                  # diagnostics (tools/probe_gemm.py): [cap, 4] int64 device tensor
        g.probe, g.probe_cap = probe.data_ptr(), probe.shape[0]
    if epi in (EPI_BF16, EPI_ACT, EPI_DACT):
        _chk(out, BF16, "out")
    else:
        _chk(out, F32, "out")
    timed = GEMM_TIMER.enabled and 2.0 * g.M * g.N * g.K * batch >= GEMM_TIMER.min_flops
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if isinstance(ride, WgradRideArgs):
        n = c_int(0)
        check(lib.aim_gemm_bf16_ride(byref(g), epi, byref(ride), byref(n), _stream()), "aim_gemm_bf16_ride")
        ride.written = n.value
    elif not (ride and batch == 1 and _launch_with_riders(lib, g, epi, ride)):
        check(lib.aim_gemm_bf16(byref(g), epi, batch, _stream()), "aim_gemm_bf16")
    if timed:
        e1.record()
        GEMM_TIMER.records.append((epi, 2.0 * g.M * g.N * g.K * batch, e0, e1))
    return out


def ride_args(g, a, m_begin: int, m_end: int, chunks: int, slabs, bias_slabs=None, at=None, ntok: int = 0) -> WgradRideArgs:
    """Riders for rows ``[m_begin, m_end)`` of ``sum_m g[m,n] a[m,k]`` in ``chunks`` row chunks per 256 x 256 tile; chunk c
    goes to ``slabs[c]`` ([Nw, Kw] f32 each) and, with ``bias_slabs``, its ``at``-weighted column sums to ``bias_slabs[c]``."""
    _chk(g, BF16, "g"); _chk(a, BF16, "a"); _chk(slabs, F32, "slabs"); _chk(bias_slabs, F32, "bias_slabs"); _chk(at, F32, "at")
    assert g.shape[0] == a.shape[0] and 0 <= m_begin < m_end <= g.shape[0]
    assert slabs.is_contiguous() and slabs.numel() >= chunks * g.shape[1] * a.shape[1]
    assert bias_slabs is None or (bias_slabs.is_contiguous() and bias_slabs.numel() >= chunks * g.shape[1])
    ra = WgradRideArgs()
    ra.G, ra.A, ra.ldg, ra.lda = g.data_ptr(), a.data_ptr(), g.stride(0), a.stride(0)
    ra.Nw, ra.Kw, ra.m_begin, ra.m_end = g.shape[1], a.shape[1], m_begin, m_end
    ra.at, ra.ntok, ra.chunks = _p(at), ntok, chunks
    ra.slabs, ra.bias_slabs = slabs.data_ptr(), _p(bias_slabs)
    ra.keep = (g, a, slabs, bias_slabs, at)
    return ra


def wgrad_slabs(g, a, m_begin: int, m_end: int, slabs, bias_slabs=None, at=None, ntok: int = 0, max_chunks: int = 0) -> int:
    """The stand-alone launch for rows ``[m_begin, m_end)``: partial sums into ``slabs`` / ``bias_slabs`` as the riders
    write them; returns the number of slabs filled."""
    _chk(g, BF16, "g"); _chk(a, BF16, "a"); _chk(slabs, F32, "slabs"); _chk(bias_slabs, F32, "bias_slabs"); _chk(at, F32, "at")
    assert g.shape[0] == a.shape[0] and 0 <= m_begin < m_end <= g.shape[0] and slabs.is_contiguous()
    assert bias_slabs is None or bias_slabs.is_contiguous()
    n = c_int(0)
    check(load_library().aim_wgrad_slabs_bf16(g.data_ptr(), g.stride(0), a.data_ptr(), a.stride(0), _p(at), ntok, m_begin, m_end,
                                              g.shape[1], a.shape[1], slabs.data_ptr(), _p(bias_slabs), max_chunks, byref(n),
                                              _stream()), "aim_wgrad_slabs_bf16")
    return n.value


def wgrad_finish(slabs, nchunks: int, dw, bias_slabs=None, db=None):
    """``dw += sum_c slabs[c]`` and ``db += sum_c bias_slabs[c]`` over the first ``nchunks`` slabs, in that order."""
    _chk(slabs, F32, "slabs"); _chk(bias_slabs, F32, "bias_slabs"); _chk(dw, F32, "dw"); _chk(db, F32, "db")
    check(load_library().aim_wgrad_finish(slabs.data_ptr(), _p(bias_slabs), nchunks, dw.data_ptr(), dw.stride(0), _p(db),
                                          dw.shape[0], dw.shape[1], _stream()), "aim_wgrad_finish")


RIDE_STATS = {"launches": 0, "rows": 0}      # rider launches / rows they summed, since import (tests, diagnostics)


class WgradRide:
    """An adapter weight gradient ``dw[n,k] += sum_m g[m,n] a[m,k]`` (``db[n] += sum_m at[m % ntok] g[m,n]``) whose rows are
    summed by rider workgroups of the GEMM launches it is offered to (``gemm(..., ride=[...])``: each takes the rows the
    library's policy gives it, ``aim_wgrad_ride_plan``), the rest by a stand-alone launch in ``finish``.  All partial sums
    lie in one workspace in row order and ``finish`` adds them up in that order: bitwise reproducible."""
    CAP = 48          # slabs of the workspace (flagship: 4 + 6 + 6 + 6 riders' chunks and the remainder's)

    def __init__(self, g, a, dw, db=None, at=None, ntok: int = 0):
        _chk(g, BF16, "g"); _chk(a, BF16, "a"); _chk(dw, F32, "dw"); _chk(db, F32, "db"); _chk(at, F32, "at")
        assert g.shape[0] == a.shape[0] and dw.shape == (g.shape[1], a.shape[1])
        self.g, self.a, self.dw, self.db, self.at, self.ntok = g, a, dw, db, at, ntok
        self.M, self.Nw, self.Kw = g.shape[0], g.shape[1], a.shape[1]
        self.next_row = 0       # rows [0, next_row) have riders
        self.used = 0           # slabs written
        self.ws = None
        self.open = True        # still offered to host launches

    @property
    def left(self) -> int:
        return self.M - self.next_row

    def _slabs(self):
        """The slab views behind the ones already written."""
        if self.ws is None:
            self.ws = torch.empty(self.CAP * self.Nw * (self.Kw + 1), dtype=F32, device=self.g.device)
        w = self.ws[:self.CAP * self.Nw * self.Kw].view(self.CAP, self.Nw, self.Kw)
        b = self.ws[self.CAP * self.Nw * self.Kw:].view(self.CAP, self.Nw) if self.db is not None else None
        return w, b

    def finish(self):
        """The rows no rider took (stand-alone launch into the slabs behind the riders'), then the sum of all slabs."""
        assert self.used > 0
        w, b = self._slabs()
        if self.left > 0:
            self.used += wgrad_slabs(self.g, self.a, self.next_row, self.M, w[self.used:], b[self.used:] if b is not None else None,
                                     at=self.at, ntok=self.ntok, max_chunks=max(1, min(self.CAP - self.used, self.left // 1024)))
            self.next_row = self.M
        wgrad_finish(w, self.used, self.dw, b, self.db)
        self.open = False


def _launch_with_riders(lib, g: GemmArgs, epi: int, rides) -> bool:
    """Offer the launch to the gradients with rows left, the one with the most first; True: launched (with riders)."""
    for r in sorted((r for r in rides if r.open and r.left > 0), key=lambda r: -r.left):
        chunks, rows = c_int(0), c_int(0)
        check(lib.aim_wgrad_ride_plan(byref(g), epi, r.Nw, r.Kw, r.ntok if r.at is not None else 0, r.M, r.left,
                                      byref(chunks), byref(rows)), "aim_wgrad_ride_plan")
        if chunks.value <= 0 or r.used + chunks.value >= r.CAP:      # (one slab stays free for the remainder)
            continue
        w, b = r._slabs()
        ra = ride_args(r.g, r.a, r.next_row, r.next_row + rows.value, chunks.value, w[r.used:], b[r.used:] if b is not None else None,
                       at=r.at, ntok=r.ntok)
        n = c_int(0)
        check(lib.aim_gemm_bf16_ride(byref(g), epi, byref(ra), byref(n), _stream()), "aim_gemm_bf16_ride")
        r.used += n.value
        r.next_row += rows.value
        RIDE_STATS["launches"] += 1
        RIDE_STATS["rows"] += rows.value
        return True
    return False


def gemm_fp8(a8: torch.Tensor, w8: torch.Tensor, wscale: torch.Tensor, epi: int, out: torch.Tensor, *, bias=None,
             resid=None, af=None, at=None, vec=None, bt=None, ntok: int = 0, act: int = 0, n_split: int = 0, act2: int = 0,
             ldv: Optional[int] = None, reserve_cus: int = 0, probe=None):
    """``out = epilogue(wscale[n] * (a8 @ w8.T))``: fp8 e4m3 operands on the block-scaled MFMA (inference only).
    ``a8`` [M, K], ``w8`` [N, K] are float8_e4m3fn (or uint8 views); ``out`` bf16 (EPI_BF16), f32 (EPI_F32) or fp8
    (EPI_ACT8)."""
    lib = load_library()
    for n_, t_ in (("a8", a8), ("w8", w8)):
        if not t_.is_cuda or t_.element_size() != 1 or t_.stride(-1) != 1:
            raise TypeError(f"{n_}: expected a GPU fp8 (1-byte) tensor with a contiguous last dimension")
    for n_, t_ in (("wscale", wscale), ("bias", bias), ("af", af), ("at", at), ("vec", vec), ("bt", bt)):
        _chk(t_, F32, n_)
    _chk(resid, BF16 if epi == EPI_RES16 else F32, "resid")       # RES16: the bf16 residual stream of the fp8 inference path
    g = GemmArgs()
    g.A, g.W = a8.data_ptr(), w8.data_ptr()
    g.M, g.K, g.N = a8.shape[0], a8.shape[1], w8.shape[0]
    g.lda, g.ldw = a8.stride(0), w8.stride(0)
    g.bias, g.resid, g.wscale = _p(bias), _p(resid), wscale.data_ptr()
    g.ldr = resid.stride(0) if resid is not None else 0
    g.af, g.at, g.vec, g.bt = _p(af), _p(at), _p(vec), _p(bt)
    g.ldv = (vec.stride(0) if ldv is None else ldv) if vec is not None else 0
    g.ntok = ntok
    g.out, g.ldo = out.data_ptr(), out.stride(0)
    g.act, g.n_split, g.act2, g.scale = act, n_split, act2, 1.0
    g.reserve_cus = int(reserve_cus)
    if probe is not None:                  # diagnostics: [cap, 4] int64 device tensor (as in gemm)
        g.probe, g.probe_cap = probe.data_ptr(), probe.shape[0]
    if epi in (EPI_BF16, EPI_RES16):
        _chk(out, BF16, "out")
    elif epi == EPI_F32:
        _chk(out, F32, "out")
    elif out.element_size() != 1:
        raise TypeError("out: EPI_ACT8 writes fp8 bytes")
    timed = GEMM_TIMER.enabled and 2.0 * g.M * g.N * g.K >= GEMM_TIMER.min_flops
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib.aim_gemm_fp8(byref(g), epi, _stream()), "aim_gemm_fp8")
    if timed:
        e1.record()
        GEMM_TIMER.records.append((100 + epi, 2.0 * g.M * g.N * g.K, e0, e1))
    return out


def quantize_fp8_rows(w: torch.Tensor):
    """Per-output-channel fp8 quantisation of a weight ``[N, K]`` (one-off host-side staging, not a hot-path op):
    ``scale[n] = amax_n / 448``, ``w8 = e4m3(w / scale)``.  Returns (w8 as float8_e4m3fn on w's device, scale f32)."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1).clamp_min(1e-12)
    scale = amax / 448.0
    q = (wf / scale[:, None]).clamp_(-448.0, 448.0)
    # the cast itself runs on the CPU: every torch build rounds f32 -> e4m3fn to nearest-even there
    w8 = q.cpu().to(FP8).to(w.device)
    return w8.contiguous(), scale.contiguous()


def layernorm_fwd_fp8(x, gamma, beta, rows, D, ldx, y8, ldy=None, eps: float = 1e-5):
    _chk(x, F32, "x"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta")
    if y8.element_size() != 1 or not y8.is_cuda:
        raise TypeError("y8: expected a GPU fp8 (1-byte) tensor")
    check(load_library().aim_layernorm_fwd_fp8(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), y8.data_ptr(),
                                               D if ldy is None else ldy, rows, D, eps, _stream()), "aim_layernorm_fwd_fp8")


def layernorm_fwd_x16(x, gamma, beta, rows, D, ldx, *, y_bf16=None, y_f32=None, y8=None, ldy=None, eps: float = 1e-5):
    """LayerNorm over bf16 rows (the fp8 inference path's residual stream); any subset of bf16 / f32 / fp8 outputs."""
    _chk(x, BF16, "x"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta"); _chk(y_bf16, BF16, "y_bf16"); _chk(y_f32, F32, "y_f32")
    if y8 is not None and (y8.element_size() != 1 or not y8.is_cuda):
        raise TypeError("y8: expected a GPU fp8 (1-byte) tensor")
    check(load_library().aim_layernorm_fwd_x16(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), _p(y_bf16), _p(y_f32), _p(y8),
                                               D if ldy is None else ldy, rows, D, eps, _stream()), "aim_layernorm_fwd_x16")


def attn_fwd_fp8(qkv, out8, BT, N, H, lse=None):
    _chk(qkv, BF16, "qkv"); _chk(lse, F32, "lse")
    if out8.element_size() != 1 or not out8.is_cuda:
        raise TypeError("out8: expected a GPU fp8 (1-byte) tensor")
    check(load_library().aim_attn_fwd_fp8(qkv.data_ptr(), out8.data_ptr(), _p(lse), BT, N, H, _stream()), "aim_attn_fwd_fp8")


def expsum_tiles(M: int, N: int) -> int:
    return load_library().aim_gemm_expsum_tiles(M, N)


def wgrad(g: torch.Tensor, a: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor] = None, at=None, ntok: int = 0):
    """``dw[n,k] += sum_m g[m,n] a[m,k]``; ``db[n] += sum_m at[m % ntok] g[m,n]`` (``at`` None: 1) in the same pass
    (fp32 accumulate in place; split-M partial slabs summed in a fixed order: no atomics)."""
    _chk(g, BF16, "g"); _chk(a, BF16, "a"); _chk(dw, F32, "dw"); _chk(db, F32, "db"); _chk(at, F32, "at")
    assert g.shape[0] == a.shape[0] and dw.shape == (g.shape[1], a.shape[1])
    lib = load_library()
    nbytes = lib.aim_wgrad_workspace_bytes(g.shape[0], g.shape[1], a.shape[1])
    ws = torch.empty(nbytes // 4, dtype=F32, device=g.device) if nbytes else None
    check(lib.aim_wgrad_bias_bf16(g.data_ptr(), g.stride(0), a.data_ptr(), a.stride(0), dw.data_ptr(), dw.stride(0), _p(db),
                                  _p(at), ntok, g.shape[0], g.shape[1], a.shape[1], _p(ws), nbytes, _stream()), "aim_wgrad_bias_bf16")


def layernorm_fwd(x, gamma, beta, rows, D, ldx, *, y_bf16=None, y_f32=None, ldy=None, mean=None, rstd=None,
                  eps: float = 1e-5):
    _chk(x, F32, "x"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta")
    _chk(y_bf16, BF16, "y_bf16"); _chk(y_f32, F32, "y_f32"); _chk(mean, F32, "mean"); _chk(rstd, F32, "rstd")
    check(load_library().aim_layernorm_fwd(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), _p(y_bf16),
                                           _p(y_f32), D if ldy is None else ldy, _p(mean), _p(rstd), rows, D,
                                           eps, _stream()), "aim_layernorm_fwd")


def layernorm_bwd(dy, x, gamma, mean, rstd, rows, D, *, lddy, ldx, lddx, dres=None, dx=None, dx_bf16=None,
                  dgamma=None, dbeta=None, lddres=None):
    """``lddres``: row stride of ``dres`` (default: ``lddx``, the rows of ``dx``)."""
    for n_, t_ in (("x", x), ("gamma", gamma), ("mean", mean), ("rstd", rstd),
                   ("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        _chk(t_, F32, n_)
    _chk(dx_bf16, BF16, "dx_bf16")
    _chk(dy, dy.dtype if dy.dtype in (F32, BF16) else F32, "dy")
    if dres is not None:
        _chk(dres, dres.dtype if dres.dtype in (F32, BF16) else F32, "dres")
    check(load_library().aim_layernorm_bwd(dy.data_ptr(), int(dy.dtype == BF16), lddy, x.data_ptr(), ldx, gamma.data_ptr(),
                                           mean.data_ptr(), rstd.data_ptr(), _p(dres),
                                           int(dres is not None and dres.dtype == BF16),
                                           lddx if lddres is None else lddres, _p(dx), _p(dx_bf16), lddx,
                                           _p(dgamma), _p(dbeta), rows, D, _stream()), "aim_layernorm_bwd")


LN_FSUM_GROUPS = 13     # token groups per frame of layernorm_bwd_fsum's partial sums (16 tokens at 197: 4 rows per wave;
                        # with 4 groups the 2 048 workgroups ran as one full round and a nearly empty one)


def layernorm_bwd_fsum(dy, x, gamma, mean, rstd, dres, dx_bf16, w, partial, frames, ntok, D):
    """layernorm_bwd for bf16 dy / dres / dx (contiguous rows) that also writes partial[frames, LN_FSUM_GROUPS, D]: the
    per-frame sums of w[n] * dx over each token group; ``frame_sum(partial, None, out, frames, LN_FSUM_GROUPS, D)`` finishes."""
    _chk(dy, BF16, "dy"); _chk(dres, BF16, "dres"); _chk(dx_bf16, BF16, "dx_bf16")
    for n_, t_ in (("x", x), ("gamma", gamma), ("mean", mean), ("rstd", rstd), ("w", w), ("partial", partial)):
        _chk(t_, F32, n_)
    assert partial.numel() >= frames * LN_FSUM_GROUPS * D
    check(load_library().aim_layernorm_bwd_fsum(dy.data_ptr(), D, x.data_ptr(), D, gamma.data_ptr(), mean.data_ptr(),
                                                rstd.data_ptr(), dres.data_ptr(), dx_bf16.data_ptr(), D, _p(w),
                                                partial.data_ptr(), LN_FSUM_GROUPS, frames, ntok, D, _stream()),
          "aim_layernorm_bwd_fsum")


def attn_fwd(qkv, out, lse, BT, N, H):
    _chk(qkv, BF16, "qkv"); _chk(out, BF16, "out"); _chk(lse, F32, "lse")
    check(load_library().aim_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), BT, N, H, _stream()),
          "aim_attn_fwd")


def attn_bwd(qkv, out, dout, lse, delta, dqkv, BT, N, H):
    _chk(qkv, BF16, "qkv"); _chk(out, BF16, "out"); _chk(dout, BF16, "dout"); _chk(dqkv, BF16, "dqkv")
    _chk(lse, F32, "lse"); _chk(delta, F32, "delta")
    check(load_library().aim_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                      delta.data_ptr(), dqkv.data_ptr(), BT, N, H, _stream()), "aim_attn_bwd")


def _shift_table(shifts, H):
    """H ints for aim_attn_*_shift (host memory, read during the call): a shorter table leaves the remaining heads unshifted"""
    import ctypes
    s = [int(x) for x in shifts]
    if len(s) > H:
        raise ValueError(f"{len(s)} shifts for {H} heads")
    return (ctypes.c_int * H)(*(s + [0] * (H - len(s))))


def attn_fwd_shift(qkv, out, lse, B, T, N, H, shifts):
    """attn_fwd over B clips of T frames where head h reads the K / V of frame (t - shifts[h]) mod T of the same clip."""
    _chk(qkv, BF16, "qkv"); _chk(out, BF16, "out"); _chk(lse, F32, "lse")
    check(load_library().aim_attn_fwd_shift(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B * T, N, H, B, T,
                                            _shift_table(shifts, H), _stream()), "aim_attn_fwd_shift")


def attn_bwd_shift(qkv, out, dout, lse, delta, dqkv, B, T, N, H, shifts):
    """backward of attn_fwd_shift: dq in the query's frame, dk / dv in the frame the keys were read from."""
    _chk(qkv, BF16, "qkv"); _chk(out, BF16, "out"); _chk(dout, BF16, "dout"); _chk(dqkv, BF16, "dqkv")
    _chk(lse, F32, "lse"); _chk(delta, F32, "delta")
    check(load_library().aim_attn_bwd_shift(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                            delta.data_ptr(), dqkv.data_ptr(), B * T, N, H, B, T,
                                            _shift_table(shifts, H), _stream()), "aim_attn_bwd_shift")


WIN_ATTN_MAX_S = 4096   # AIM_WIN_ATTN_MAX_S of include/aim_kernels.h (ABI 11)


def _ints3(v):
    a, b, c = (int(x) for x in v)
    return a, b, c


def _win_attn_fwd(entry, qkv, out, lse, B, T, N, H, window, shift, P):
    """the three forward entries: ``entry`` names the library's function, ``shift`` is None for the one that takes none"""
    _chk(qkv, BF16, "qkv"); _chk(out, BF16, "out"); _chk(lse, F32, "lse")
    geom = _ints3(window) + (() if shift is None else _ints3(shift))
    check(getattr(load_library(), entry)(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, T, N, N if P is None else P, H,
                                         *geom, _stream()), entry)


def _win_attn_bwd(entry, qkv, out, dout, lse, delta, dqkv, B, T, N, H, window, shift, P):
    """the three backward entries, as ``_win_attn_fwd``"""
    _chk(qkv, BF16, "qkv"); _chk(out, BF16, "out"); _chk(dout, BF16, "dout"); _chk(dqkv, BF16, "dqkv")
    _chk(lse, F32, "lse"); _chk(delta, F32, "delta")
    geom = _ints3(window) + (() if shift is None else _ints3(shift))
    check(getattr(load_library(), entry)(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                         dqkv.data_ptr(), B, T, N, N if P is None else P, H, *geom, _stream()), entry)


def win_attn_fwd(qkv, out, lse, B, T, N, H, window, P=None):
    """Attention inside the (wt, wh, ww) windows of the patch grid of B clips of T frames (class rows untouched); the
    partition is addressing inside the kernel.  P (default N): token rows per frame of the buffers, the rows behind a
    frame's N tokens are untouched too.  out [B*T*P, D], lse [B*T, H, P]."""
    _win_attn_fwd("aim_win_attn_fwd", qkv, out, lse, B, T, N, H, window, None, P)


def win_attn_bwd(qkv, out, dout, lse, delta, dqkv, B, T, N, H, window, P=None):
    """backward of win_attn_fwd: writes the patch rows of dqkv [B*T*P, 3D] and of delta [B*T, H, P]."""
    _win_attn_bwd("aim_win_attn_bwd", qkv, out, dout, lse, delta, dqkv, B, T, N, H, window, None, P)


def win_attn_fwd_shift(qkv, out, lse, B, T, N, H, window, shift, P=None):
    """win_attn_fwd on windows shifted by (st, sh, sw): the h and w axes are cut at 0, s, s + w, ..., the t windows start at st
    and wrap round the clip's end (include/aim_kernels.h).  A zero shift gives win_attn_fwd's bits."""
    _win_attn_fwd("aim_win_attn_fwd_shift", qkv, out, lse, B, T, N, H, window, shift, P)


def win_attn_bwd_shift(qkv, out, dout, lse, delta, dqkv, B, T, N, H, window, shift, P=None):
    """backward of win_attn_fwd_shift: writes the patch rows of dqkv [B*T*P, 3D] and of delta [B*T, H, P]."""
    _win_attn_bwd("aim_win_attn_bwd_shift", qkv, out, dout, lse, delta, dqkv, B, T, N, H, window, shift, P)


def win_attn_fwd_cut(qkv, out, lse, B, T, N, H, window, shift, P=None):
    """win_attn_fwd_shift with the t axis cut like h and w, at 0, st, st + wt, ..., T, instead of wrapping round the clip's end
    (AIM's masked shifted windows; include/aim_kernels.h).  st = 0 gives win_attn_fwd_shift's bits."""
    _win_attn_fwd("aim_win_attn_fwd_cut", qkv, out, lse, B, T, N, H, window, shift, P)


def win_attn_bwd_cut(qkv, out, dout, lse, delta, dqkv, B, T, N, H, window, shift, P=None):
    """backward of win_attn_fwd_cut: writes the patch rows of dqkv [B*T*P, 3D] and of delta [B*T, H, P]."""
    _win_attn_bwd("aim_win_attn_bwd_cut", qkv, out, dout, lse, delta, dqkv, B, T, N, H, window, shift, P)


def swin_attn_cap(S: int) -> int:
    """token slots per sequence of the Swin attention kernels' lse rows (include/aim_kernels.h, ABI 18)"""
    return 32 if S <= 32 else 64


def _swin_bwd(entry, geom, rows, nseq, H, S, qkv, bias, dout, lse, dqkv, dbias):
    _chk(qkv, BF16, "qkv"); _chk(dout, BF16, "dout"); _chk(dqkv, BF16, "dqkv"); _chk(dbias, F32, "dbias")
    _swin_sizes(entry, qkv, bias, dout, lse, rows, nseq, H, S)
    if not dqkv.is_contiguous() or dqkv.numel() != qkv.numel() or \
            (dbias is not None and (not dbias.is_contiguous() or dbias.numel() != bias.numel())):
        raise ValueError(f"{entry}: dqkv / dbias must be contiguous with the sizes of qkv / bias")
    lib = load_library()
    nbytes = lib.aim_swin_attn_bwd_workspace_bytes(nseq, H, S) if dbias is not None else 0
    ws = torch.empty((nbytes // 4,), dtype=F32, device=qkv.device) if nbytes else None
    check(getattr(lib, entry)(qkv.data_ptr(), bias.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), _p(dbias), *geom,
                              _p(ws), nbytes, _stream()), entry)


def _swin_sizes(entry, qkv, bias, out, lse, rows, nseq, H, S):
    """the sizes of the buffers every Swin attention entry shares (``out``: out of the forward, dout of the backward)"""
    _chk(qkv, BF16, "qkv"); _chk(bias, F32, "bias"); _chk(out, BF16, "out"); _chk(lse, F32, "lse")
    C = 32 * H
    want = dict(qkv=(qkv, rows * 3 * C), bias=(bias, H * S * S), out=(out, rows * C), lse=(lse, nseq * H * swin_attn_cap(S)))
    for n_, (t_, numel) in want.items():
        if not t_.is_contiguous() or t_.numel() != numel:
            raise ValueError(f"{entry}: {n_} must be contiguous with {numel} elements, got {tuple(t_.shape)}")


def swin_win_attn_fwd(qkv, bias, out, lse, frames, res, H, window, shift):
    """Swin window attention (head width 32) on the fused qkv [frames*res*res, 96 H]: the windows of the grid rolled by
    -shift, masked pairs at weight exactly 0, ``bias`` [H, S, S] f32 (S = window^2).  out [rows, 32 H] bf16; lse
    [frames*(res/window)^2, H, swin_attn_cap(S)] f32 (base 2)."""
    if window > 0 and res > 0 and res % window == 0:
        _swin_sizes("swin_win_attn_fwd", qkv, bias, out, lse, frames * res * res, frames * (res // window) ** 2, H, window * window)
    check(load_library().aim_swin_win_attn_fwd(qkv.data_ptr(), bias.data_ptr(), out.data_ptr(), lse.data_ptr(), frames, res, H,
                                               window, shift, _stream()), "aim_swin_win_attn_fwd")


def swin_win_attn_bwd(qkv, bias, dout, lse, dqkv, dbias, frames, res, H, window, shift):
    """backward of swin_win_attn_fwd from d(out) and the forward's lse: writes dqkv [rows, 96 H] and, unless None, the dense
    bias gradient dbias [H, S, S] (two-stage fixed-order sum over the windows: equal bits on every run)."""
    _swin_bwd("aim_swin_win_attn_bwd", (frames, res, H, window, shift), frames * res * res, frames * (res // window) ** 2, H,
              window * window, qkv, bias, dout, lse, dqkv, dbias)


def swin_tattn_fwd(qkv, bias, out, lse, B, T, L, H):
    """Swin temporal attention (head width 32) over the T <= 32 frame tokens of every (clip, position) of the fused qkv
    [B*T*L, 96 H]; ``bias`` [H, T, T] f32.  out [rows, 32 H] bf16; lse [B*L, H, 32] f32 (base 2)."""
    if 0 < T <= 32:
        _swin_sizes("swin_tattn_fwd", qkv, bias, out, lse, B * T * L, B * L, H, T)
    check(load_library().aim_swin_tattn_fwd(qkv.data_ptr(), bias.data_ptr(), out.data_ptr(), lse.data_ptr(), B, T, L, H, _stream()),
          "aim_swin_tattn_fwd")


def swin_tattn_bwd(qkv, bias, dout, lse, dqkv, dbias, B, T, L, H):
    """backward of swin_tattn_fwd: writes dqkv and, unless None, the dense bias gradient dbias [H, T, T]."""
    _swin_bwd("aim_swin_tattn_bwd", (B, T, L, H), B * T * L, B * L, H, T, qkv, bias, dout, lse, dqkv, dbias)


def swin_bias_scatter(dense, index, dtable):
    """dtable [ntable, H] f32 += the dense bias gradient ``dense`` [H, S, S] folded along ``index`` [S*S] int32 (the
    relative-position index), entries of one table row summed in ascending order."""
    _chk(dense, F32, "dense"); _chk(index, torch.int32, "index"); _chk(dtable, F32, "dtable")
    H, SS = dense.shape[0], dense.shape[1] * dense.shape[2]
    if not (dense.is_contiguous() and index.is_contiguous() and dtable.is_contiguous()) or index.numel() != SS \
            or dtable.dim() != 2 or dtable.shape[1] != H:
        raise ValueError("swin_bias_scatter: dense [H, S, S], index [S*S] and dtable [ntable, H], all contiguous")
    check(load_library().aim_swin_bias_scatter(dense.data_ptr(), index.data_ptr(), dtable.data_ptr(), H, SS, dtable.shape[0],
                                               _stream()), "aim_swin_bias_scatter")


def _swin3d_sizes(entry, named, rows, H, table, full):
    """the sizes of the buffers the 3-D Swin attention entries share: ``named`` maps a name to (tensor, dtype, columns)"""
    for n_, (t_, dt_, cols) in named.items():
        _chk(t_, dt_, n_)
        if not t_.is_contiguous() or t_.numel() != rows * cols:
            raise ValueError(f"{entry}: {n_} must be contiguous with {rows * cols} elements, got {tuple(t_.shape)}")
    _chk(table, F32, "table")
    ntab = (2 * full[0] - 1) * (2 * full[1] - 1) * (2 * full[2] - 1)
    if not table.is_contiguous() or tuple(table.shape) != (ntab, H):
        raise ValueError(f"{entry}: table must be contiguous [{ntab}, {H}], got {tuple(table.shape)}")


def swin3d_attn_fwd(qkv, table, out, lse, clips, D, G, H, window, shift, full_window):
    """3-D Swin window attention (head width 32) on the fused qkv [clips*D*G*G, 96 H], rows (clip, d, y, x): softmax attention
    inside the boxes that cut each axis at 0, s, s + w, ... (the reference's rolled, masked windows; masked pairs at weight
    exactly 0) under the bias table [(2Wt-1)(2Wh-1)(2Ww-1), H] f32 of ``full_window``.  ``window`` is the effective window,
    ``shift`` its shift.  out [rows, 32 H] bf16; lse [rows, H] f32 (base 2)."""
    rows, C = clips * D * G * G, 32 * H
    _swin3d_sizes("swin3d_attn_fwd", dict(qkv=(qkv, BF16, 3 * C), out=(out, BF16, C), lse=(lse, F32, H)), rows, H, table, full_window)
    check(load_library().aim_swin3d_attn_fwd(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), lse.data_ptr(), clips, D, G, H,
                                             *window, *shift, *full_window, _stream()), "aim_swin3d_attn_fwd")


def swin3d_attn_bwd(qkv, table, dout, lse, delta, dqkv, dtable, clips, D, G, H, window, shift, full_window):
    """backward of swin3d_attn_fwd from d(out) and the forward's lse: writes delta [rows, H] f32 and dqkv [rows, 96 H] and,
    unless None, ADDS the table gradient onto dtable [table, H] f32 (fixed-order sums: equal bits on every run)."""
    rows, C = clips * D * G * G, 32 * H
    _swin3d_sizes("swin3d_attn_bwd", dict(qkv=(qkv, BF16, 3 * C), dout=(dout, BF16, C), lse=(lse, F32, H), delta=(delta, F32, H),
                                          dqkv=(dqkv, BF16, 3 * C)), rows, H, table, full_window)
    _chk(dtable, F32, "dtable")
    if dtable is not None and (not dtable.is_contiguous() or dtable.shape != table.shape):
        raise ValueError("swin3d_attn_bwd: dtable must be contiguous with the shape of table")
    lib = load_library()
    nbytes = lib.aim_swin3d_attn_bwd_workspace_bytes(clips, D, G, H, *window, *shift) if dtable is not None else 0
    ws = torch.empty((nbytes // 4,), dtype=F32, device=qkv.device) if nbytes else None
    check(lib.aim_swin3d_attn_bwd(qkv.data_ptr(), table.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                  dqkv.data_ptr(), _p(dtable), clips, D, G, H, *window, *shift, *full_window, _p(ws), nbytes,
                                  _stream()), "aim_swin3d_attn_bwd")


def attn_fwd_cls(qkv, out_cls, lse_cls, BT, N, H):
    """attn_fwd for the class query of every (frame, head) alone: out_cls [BT, D], lse_cls [BT, H]."""
    _chk(qkv, BF16, "qkv"); _chk(out_cls, BF16, "out_cls"); _chk(lse_cls, F32, "lse_cls")
    check(load_library().aim_attn_fwd_cls(qkv.data_ptr(), out_cls.data_ptr(), lse_cls.data_ptr(), BT, N, H, _stream()),
          "aim_attn_fwd_cls")


def attn_bwd_cls(qkv, out_cls, dout_cls, lse_cls, dqkv, BT, N, H):
    """attn_bwd where only the class row of dout is non-zero: writes the whole dqkv [BT*N, 3D] (zeros in the other dq rows)."""
    _chk(qkv, BF16, "qkv"); _chk(out_cls, BF16, "out_cls"); _chk(dout_cls, BF16, "dout_cls"); _chk(dqkv, BF16, "dqkv")
    _chk(lse_cls, F32, "lse_cls")
    check(load_library().aim_attn_bwd_cls(qkv.data_ptr(), out_cls.data_ptr(), dout_cls.data_ptr(), lse_cls.data_ptr(),
                                          dqkv.data_ptr(), BT, N, H, _stream()), "aim_attn_bwd_cls")


def cls_attn_fwd(qkv, out_cls, probs, B, T, N, H):
    _chk(qkv, BF16, "qkv"); _chk(out_cls, BF16, "out_cls"); _chk(probs, F32, "probs")
    check(load_library().aim_cls_attn_fwd(qkv.data_ptr(), out_cls.data_ptr(), probs.data_ptr(), B, T, N, H,
                                          _stream()), "aim_cls_attn_fwd")


def cls_attn_bwd(qkv, probs, dout_cls, dqkv, B, T, N, H, compact: bool = False):
    """compact=False: add into the class rows of dqkv [B*T*N, 3D]; compact=True: write dqkv [B*T, 3D]."""
    _chk(qkv, BF16, "qkv"); _chk(dout_cls, BF16, "dout_cls"); _chk(dqkv, BF16, "dqkv"); _chk(probs, F32, "probs")
    check(load_library().aim_cls_attn_bwd(qkv.data_ptr(), probs.data_ptr(), dout_cls.data_ptr(), dqkv.data_ptr(),
                                          int(compact), B, T, N, H, _stream()), "aim_cls_attn_bwd")


def tattn_fwd(qkv, out, probs, B, T, N, H):
    """Temporal attention over the T frames of every token position (stock-AIM block): out [M, D], probs [B*N, H, T, T]."""
    _chk(qkv, BF16, "qkv"); _chk(out, BF16, "out"); _chk(probs, F32, "probs")
    check(load_library().aim_tattn_fwd(qkv.data_ptr(), out.data_ptr(), probs.data_ptr(), B, T, N, H, _stream()), "aim_tattn_fwd")


def tattn_fwd_infer(qkv, out, B, T, N, H):
    """``tattn_fwd`` for a forward without a backward: no probabilities are stored.  ``out`` [M, D] bf16 gets the bits
    ``tattn_fwd`` writes; a 1-byte dtype (fp8 e4m3 / uint8) gets the saturating e4m3 cast of the same fp32 accumulators."""
    _chk(qkv, BF16, "qkv")
    if not out.is_cuda or not out.is_contiguous():
        raise TypeError("out: expected a contiguous GPU tensor")
    if out.dtype == BF16:
        o16, o8 = out.data_ptr(), None
    elif out.element_size() == 1:
        o16, o8 = None, out.data_ptr()
    else:
        raise TypeError(f"out: expected bf16 or a 1-byte (fp8) dtype, got {out.dtype}")
    check(load_library().aim_tattn_fwd_infer(qkv.data_ptr(), o16, o8, B, T, N, H, _stream()), "aim_tattn_fwd_infer")


def tattn_bwd(qkv, probs, dout, dqkv, B, T, N, H):
    _chk(qkv, BF16, "qkv"); _chk(probs, F32, "probs"); _chk(dout, BF16, "dout"); _chk(dqkv, BF16, "dqkv")
    check(load_library().aim_tattn_bwd(qkv.data_ptr(), probs.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), B, T, N, H, _stream()),
          "aim_tattn_bwd")


def add_bf16(a, b, out):
    """out = a + b (bf16, 2-D, row-strided)."""
    _chk(a, BF16, "a"); _chk(b, BF16, "b"); _chk(out, BF16, "out")
    R, C = a.shape
    check(load_library().aim_add_bf16(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), R, C,
                                      _stream()), "aim_add_bf16")
    return out


def acc_bf16(x, s):
    """x (f32, dense 2-D) += s (bf16, row-strided)."""
    _chk(x, F32, "x"); _chk(s, BF16, "s")
    assert x.is_contiguous() and x.shape == s.shape
    check(load_library().aim_acc_bf16(x.data_ptr(), s.data_ptr(), s.stride(0), x.shape[0], x.shape[1], _stream()), "aim_acc_bf16")
    return x


def _lowrank_args(xs, wa, ba, hs, wb, bb, ys, alpha, y32=None, resid=None) -> LowrankArgs:
    """``aim_lowrank_args`` of G = len(wa) adapters; every list entry of hs / ys / ba / bb may be None"""
    G = len(wa)
    r, D = wa[0].shape
    for t in list(xs) + list(wa) + list(wb) + list(hs) + list(ys):
        _chk(t, BF16, "lowrank operand")
    for t in list(ba) + list(bb) + [y32, resid]:
        _chk(t, F32, "lowrank bias / fp32 operand")
    for w in list(wa) + list(wb):
        if not w.is_contiguous():
            raise ValueError("lowrank: the weights must be dense")
    if any(tuple(w.shape) != (r, D) for w in wa) or any(tuple(w.shape) != (D, r) for w in wb):
        raise ValueError("lowrank: the first weights must be [r, D] and the second [D, r], the same for every adapter")

    def one_stride(ts, what):
        s = {t.stride(0) for t in ts if t is not None}
        if len(s) > 1:
            raise ValueError(f"lowrank: every {what} must have the same row stride")
        return s.pop() if s else max(D, r)

    a = LowrankArgs()
    M = xs[0].shape[0]
    for g in range(G):
        a.x[g] = _p(xs[g]) if g < len(xs) else None
        a.wa[g], a.wb[g] = wa[g].data_ptr(), wb[g].data_ptr()
        a.ba[g], a.bb[g] = _p(ba[g]), _p(bb[g])
        a.h[g], a.y[g] = _p(hs[g]), (_p(ys[g]) if g < len(ys) else None)
    a.ldx, a.ldh, a.ldy = one_stride(xs, "input"), one_stride(hs, "intermediate"), one_stride(ys, "output")
    a.y32, a.resid = _p(y32), _p(resid)
    a.ld32 = y32.stride(0) if y32 is not None else 0
    a.ldr = resid.stride(0) if resid is not None else 0
    a.M, a.D, a.r, a.G, a.alpha = M, D, r, G, float(alpha)
    return a


def lowrank_fwd(x, w1, b1, w2, b2, *, h=None, y=None, alpha: float = 1.0, y32=None, resid=None):
    """G fused linear bottleneck adapters on one input (``aim_lowrank_fwd``; G = len(w1) in {1, 3}):
    ``h[g] = bf16(x w1[g]^T + b1[g])`` (stored where ``h[g]`` is given), ``y[g] = alpha x + h[g] w2[g]^T + b2[g]``.  x [M, D]
    bf16 and every y[g] may be row-strided; w1[g] [r, D], w2[g] [D, r] bf16 dense; biases fp32.  G == 1: ``y32 = resid + `` the
    same sum before its rounding (fp32), beside or instead of y[0]."""
    G = len(w1)
    h = [None] * G if h is None else list(h)
    y = [None] * G if y is None else list(y)
    a = _lowrank_args([x], w1, b1, h, w2, b2, y, alpha, y32, resid)
    check(load_library().aim_lowrank_fwd(byref(a), _stream()), "aim_lowrank_fwd")


def lowrank_bwd(dy, w2t, w1t, dh, dx, *, alpha: float = 1.0):
    """Backward of ``lowrank_fwd`` towards its input (``aim_lowrank_bwd``): ``dh[g] = bf16(dy[g] w2[g])`` from the transposed
    copy w2t[g] [r, D], ``dx = bf16(alpha sum_g dy[g] + sum_g dh[g] w1[g])`` from w1t[g] [D, r].  The dy[g] share one row stride
    (column slabs of one buffer); every dh[g] is an output."""
    G = len(w2t)
    a = _lowrank_args(list(dy), w2t, [None] * G, list(dh), w1t, [None] * G, [dx], alpha)
    check(load_library().aim_lowrank_bwd(byref(a), _stream()), "aim_lowrank_bwd")


def lambda_partials(partials, lam, one_minus, BT):
    """lamda from [BT, 16, 2] (max, sum) slots: 8 ``ow`` partials, 8 ``cw`` partials (EXPSUM GEMM with ``xrow``)."""
    _chk(partials, F32, "partials"); _chk(lam, F32, "lam"); _chk(one_minus, F32, "one_minus")
    check(load_library().aim_lambda_partials(partials.data_ptr(), lam.data_ptr(), _p(one_minus), BT, _stream()),
          "aim_lambda_partials")


def qk_cross(qkv, kx, ss, BT, N, D, scale):
    """ss[bt, i] = scale * q_i . kx[bt] (full width D): the pass over q of lamda's cw statistic."""
    _chk(qkv, BF16, "qkv"); _chk(kx, BF16, "kx"); _chk(ss, F32, "ss")
    check(load_library().aim_qk_cross(qkv.data_ptr(), kx.data_ptr(), kx.stride(0), ss.data_ptr(), BT, N, D, scale,
                                      _stream()), "aim_qk_cross")


def qk_border(qkv, kx, ss, partials, slot0: int, BT, N, D, scale):
    """Border of the lamda statistics for N = 257 (see aim_qk_border): fills ss [BT, N] and partials[:, slot0:slot0 + 2]."""
    _chk(qkv, BF16, "qkv"); _chk(kx, BF16, "kx"); _chk(ss, F32, "ss"); _chk(partials, F32, "partials")
    assert partials.dim() == 3 and partials.shape[0] == BT and partials.shape[2] == 2 and partials.is_contiguous()
    check(load_library().aim_qk_border(qkv.data_ptr(), kx.data_ptr(), kx.stride(0), ss.data_ptr(), partials.data_ptr(), slot0,
                                       partials.shape[1], BT, N, D, scale, _stream()), "aim_qk_border")


def lambda_(qkv, kx, partials, ntiles, lam, one_minus, BT, N, D, scale, ss=None):
    """lamda = cw / (cw + ow); ``ss`` = precomputed cross scores (qk_cross), else computed here from q and kx."""
    _chk(qkv, BF16, "qkv"); _chk(kx, BF16, "kx"); _chk(partials, F32, "partials"); _chk(lam, F32, "lam")
    _chk(one_minus, F32, "one_minus"); _chk(ss, F32, "ss")
    check(load_library().aim_lambda(qkv.data_ptr(), kx.data_ptr(), kx.stride(0), _p(ss), partials.data_ptr(), ntiles,
                                    lam.data_ptr(), _p(one_minus), BT, N, D, scale, _stream()), "aim_lambda")


_IN_DTYPES = {torch.float32: 0, torch.uint8: 1, torch.bfloat16: 2}


def patchify(imgs, A, B, T, H, W, p, Kp, mean3=None, std3=None, blend=None):
    """The patch matrix ``A`` (bf16, or f32 for the fp32 path) of the clips ``imgs`` (float32 or uint8; bfloat16 only into a
    bf16 ``A`` without a blend), with the uint8 normalisation fused when ``mean3`` / ``std3`` are given.  ``blend``
    (``blending.FusedBlend``): a mixup / cutmix of clip b and clip ``blend.partner[b]`` applied while gathering.  The kernel
    writes ``A`` 16 bytes at a time, so ``A`` starts on a 16-byte boundary."""
    f32_out = A.dtype == F32
    _chk(A, F32 if f32_out else BF16, "A"); _chk(mean3, F32, "mean3"); _chk(std3, F32, "std3")
    if A.data_ptr() % 16:
        raise ValueError("patchify: A must be 16-byte aligned")
    entry = "aim_patchify" + ("_blend" if blend is not None else "") + ("_f32" if f32_out else "")
    if imgs.dtype not in _IN_DTYPES or (imgs.dtype == BF16 and entry != "aim_patchify"):
        raise TypeError(f"patchify: unsupported input dtype {imgs.dtype} for {entry} (float32, uint8; bfloat16 only for aim_patchify)")
    if not imgs.is_cuda or not imgs.is_contiguous():
        raise ValueError("patchify: imgs must be a contiguous GPU tensor")
    args = ()
    if blend is not None:
        _chk(blend.partner, torch.int32, "partner")
        if blend.partner.numel() != B or not blend.partner.is_contiguous():
            raise ValueError(f"patchify: partner must hold one index per clip ({B}), got {tuple(blend.partner.shape)}")
        args = (blend.partner.data_ptr(), blend.mode, blend.lam, blend.oml, *blend.box)
    check(getattr(load_library(), entry)(imgs.data_ptr(), _IN_DTYPES[imgs.dtype], _p(mean3), _p(std3), A.data_ptr(),
                                         B, T, H, W, p, Kp, *args, _stream()), entry)


def embed_ln(tok, cls, pos, temporal, gamma, beta, x, mean, rstd, B, T, N, D, eps=1e-5):
    _chk(tok, BF16, "tok")
    for n_, t_ in (("cls", cls), ("pos", pos), ("temporal", temporal), ("gamma", gamma), ("beta", beta), ("x", x),
                   ("mean", mean), ("rstd", rstd)):
        _chk(t_, F32, n_)
    check(load_library().aim_embed_ln(tok.data_ptr(), cls.data_ptr(), pos.data_ptr(), temporal.data_ptr(),
                                      gamma.data_ptr(), beta.data_ptr(), x.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), B, T, N, D, eps, _stream()), "aim_embed_ln")


def embed_bwd(dx, tok, cls, pos, temporal, gamma, mean, rstd, dtemporal, B, T, N, D):
    _chk(tok, BF16, "tok")
    for n_, t_ in (("cls", cls), ("pos", pos), ("temporal", temporal), ("gamma", gamma), ("mean", mean),
                   ("rstd", rstd), ("dtemporal", dtemporal)):
        _chk(t_, F32, n_)
    _chk(dx, dx.dtype if dx.dtype in (F32, BF16) else F32, "dx")
    lib = load_library()
    nbytes = lib.aim_embed_bwd_workspace_bytes(B, T, N, D)
    ws = torch.empty((nbytes // 4,), dtype=F32, device=dx.device)      # two-stage, bitwise reproducible reduction
    check(lib.aim_embed_bwd(dx.data_ptr(), int(dx.dtype == BF16), tok.data_ptr(), cls.data_ptr(), pos.data_ptr(),
                            temporal.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                            dtemporal.data_ptr(), B, T, N, D, ws.data_ptr(), nbytes, _stream()), "aim_embed_bwd")


def embed_ln_bwd(dx, tok, cls, pos, temporal, gamma, mean, rstd, B, T, N, D, *, dtok=None, dcls=None, dpos=None, dtemporal=None,
                 dgamma=None, dbeta=None):
    """Full backward of ``embed_ln`` / ``embed_ln_f32`` from dx [B*T*N, D]: WRITES dtok [B*T*(N-1), D] (the token rows of
    d(ln_pre's input)) and ADDS into dcls [D], dpos [N, D], dtemporal [T, D], dgamma [D], dbeta [D] (fp32); any output may be
    None.  dx, tok and dtok share one dtype: bf16 (the bf16 path) or f32.  Two ordered stages (reproducible, no atomics)."""
    _chk(dx, dx.dtype if dx.dtype in (F32, BF16) else F32, "dx")
    _chk(tok, dx.dtype, "tok"); _chk(dtok, dx.dtype, "dtok")
    for n_, t_ in (("cls", cls), ("pos", pos), ("temporal", temporal), ("gamma", gamma), ("mean", mean), ("rstd", rstd),
                   ("dcls", dcls), ("dpos", dpos), ("dtemporal", dtemporal), ("dgamma", dgamma), ("dbeta", dbeta)):
        _chk(t_, F32, n_)
    sizes = dict(dx=(dx, B * T * N * D), tok=(tok, B * T * (N - 1) * D), cls=(cls, D), pos=(pos, N * D), temporal=(temporal, T * D),
                 gamma=(gamma, D), mean=(mean, B * T * N), rstd=(rstd, B * T * N), dtok=(dtok, B * T * (N - 1) * D), dcls=(dcls, D),
                 dpos=(dpos, N * D), dtemporal=(dtemporal, T * D), dgamma=(dgamma, D), dbeta=(dbeta, D))
    for n_, (t_, numel) in sizes.items():
        if t_ is not None and (not t_.is_contiguous() or t_.numel() != numel):
            raise ValueError(f"embed_ln_bwd: {n_} must be contiguous with {numel} elements, got {tuple(t_.shape)}")
    lib = load_library()
    nbytes = lib.aim_embed_ln_bwd_workspace_bytes(B, T, N, D)
    ws = torch.empty((max(nbytes, 16) // 4,), dtype=F32, device=dx.device)
    check(lib.aim_embed_ln_bwd(dx.data_ptr(), int(dx.dtype == BF16), tok.data_ptr(), cls.data_ptr(), pos.data_ptr(),
                               temporal.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dtok), _p(dcls), _p(dpos),
                               _p(dtemporal), _p(dgamma), _p(dbeta), B, T, N, D, ws.data_ptr(), nbytes, _stream()),
          "aim_embed_ln_bwd")


def embed_nopre_fwd(tok, cls, pos, temporal, x, B, T, N, D):
    """ViT_ImageNet embedding (no ln_pre): x [B*T*N, D] = ((cls | tok) + pos) + temporal; tok f32 [B*T*(N-1), D] (conv + bias)."""
    for n_, t_ in (("tok", tok), ("cls", cls), ("pos", pos), ("temporal", temporal), ("x", x)):
        _chk(t_, F32, n_)
    check(load_library().aim_embed_nopre_fwd(tok.data_ptr(), cls.data_ptr(), pos.data_ptr(), temporal.data_ptr(), x.data_ptr(),
                                             B, T, N, D, _stream()), "aim_embed_nopre_fwd")


def embed_nopre_bwd(dx, B, T, N, D, *, dtok=None, dcls=None, dpos=None, dtemporal=None, dbias=None):
    """Backward of ``embed_nopre_fwd`` from dx [B*T*N, D] (bf16 or f32): ADDS into dcls [D], dpos [N, D], dtemporal [T, D] and
    dbias [D] (fp32) and writes dtok [B*T*(N-1), D] (dx's dtype); any output may be None.  Fixed-order sums (reproducible)."""
    _chk(dx, dx.dtype if dx.dtype in (F32, BF16) else F32, "dx")
    _chk(dtok, dx.dtype, "dtok")
    for n_, t_ in (("dcls", dcls), ("dpos", dpos), ("dtemporal", dtemporal), ("dbias", dbias)):
        _chk(t_, F32, n_)
    assert dx.is_contiguous() and (dtok is None or dtok.is_contiguous())
    lib = load_library()
    nbytes = lib.aim_embed_nopre_bwd_workspace_bytes(B, T, N, D)
    ws = torch.empty((nbytes // 4,), dtype=F32, device=dx.device)
    check(lib.aim_embed_nopre_bwd(dx.data_ptr(), int(dx.dtype == BF16), _p(dtok), _p(dcls), _p(dpos), _p(dtemporal), _p(dbias),
                                  B, T, N, D, ws.data_ptr(), nbytes, _stream()), "aim_embed_nopre_bwd")


def layernorm_gb_bwd(dy, x, mean, rstd, rows, D, dgamma, dbeta, *, lddy=None, ldx=None):
    """LayerNorm affine gradients over ``rows`` rows: dgamma += sum dy * (x - mean) * rstd, dbeta += sum dy (fp32, ADDED).
    Two-stage, fixed order: bitwise reproducible at any row count (aim_layernorm_bwd's own dgamma / dbeta use fp32 atomics
    above 8 192 rows)."""
    _chk(dy, dy.dtype if dy.dtype in (F32, BF16) else F32, "dy")
    for n_, t_ in (("x", x), ("mean", mean), ("rstd", rstd), ("dgamma", dgamma), ("dbeta", dbeta)):
        _chk(t_, F32, n_)
    lib = load_library()
    nbytes = lib.aim_layernorm_gb_bwd_workspace_bytes(rows, D)
    ws = torch.empty((nbytes // 4,), dtype=F32, device=dy.device)
    check(lib.aim_layernorm_gb_bwd(dy.data_ptr(), int(dy.dtype == BF16), dy.stride(0) if lddy is None else lddy, x.data_ptr(),
                                   x.stride(0) if ldx is None else ldx, mean.data_ptr(), rstd.data_ptr(), _p(dgamma), _p(dbeta),
                                   rows, D, ws.data_ptr(), nbytes, _stream()), "aim_layernorm_gb_bwd")


def frame_sum(x, w, out, frames, ntok, D):
    _chk(x, x.dtype if x.dtype in (F32, BF16) else F32, "x"); _chk(w, F32, "w"); _chk(out, F32, "out")
    check(load_library().aim_frame_sum(x.data_ptr(), int(x.dtype == BF16), _p(w), out.data_ptr(), frames, ntok, D, _stream()),
          "aim_frame_sum")


def colsum(X, out, *, af=None, at=None, ntok=0):
    _chk(X, BF16, "X"); _chk(out, F32, "out"); _chk(af, F32, "af"); _chk(at, F32, "at")
    ws = None
    if X.shape[0] > 64:             # two-stage through a scratch buffer: no atomics, bitwise reproducible
        ws = torch.empty((min(1024, (X.shape[0] + 63) // 64), X.shape[1]), dtype=F32, device=X.device)
    check(load_library().aim_colsum_bf16(X.data_ptr(), X.stride(0), _p(af), _p(at), ntok, out.data_ptr(),
                                         X.shape[0], X.shape[1], _p(ws), ws.numel() * 4 if ws is not None else 0,
                                         _stream()), "aim_colsum_bf16")


def cast_bf16(src, dst, transpose=False):
    """``dst = bf16(src)`` or ``bf16(src.T)``; ``dst`` may be a column slice of a wider matrix (row-strided)."""
    _chk(src, F32, "src"); _chk(dst, BF16, "dst")
    R, C = src.shape
    assert tuple(dst.shape) == ((C, R) if transpose else (R, C)) and src.is_contiguous()
    check(load_library().aim_cast_bf16(src.data_ptr(), dst.data_ptr(), R, C, int(transpose), dst.stride(0), _stream()),
          "aim_cast_bf16")


def scale_rows(x, s, y=None, y_f32=None):
    _chk(x, F32, "x"); _chk(s, F32, "s"); _chk(y, BF16, "y"); _chk(y_f32, F32, "y_f32")
    R, C = x.shape
    check(load_library().aim_scale_rows(x.data_ptr(), s.data_ptr(), _p(y), _p(y_f32), R, C, _stream()),
          "aim_scale_rows")


def add_rows(dst, dst_row_stride: int, src):
    """dst[r * dst_row_stride + c] += src[r, c]  (bf16 += fp32)."""
    _chk(dst, BF16, "dst"); _chk(src, F32, "src")
    R, C = src.shape
    check(load_library().aim_add_rows_bf16(dst.data_ptr(), int(dst_row_stride), src.data_ptr(), R, C, _stream()),
          "aim_add_rows_bf16")


def adamw_flat(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale: float = 1.0):
    for n_, t_ in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t_, F32, n_)
    check(load_library().aim_adamw_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1,
                                        beta2, eps, weight_decay, step, grad_scale, _stream()), "aim_adamw_flat")


def head_fwd(feat, drop, W, bias):
    """feat [B, T, D] f32 -> (pooled [B, D], score [B, C]) ; drop [B, D] factor table or None."""
    _chk(feat, F32, "feat"); _chk(drop, F32, "drop"); _chk(W, F32, "W"); _chk(bias, F32, "bias")
    B, T, D = feat.shape
    C = W.shape[0]
    assert feat.is_contiguous() and W.is_contiguous() and W.shape[1] == D
    pooled = torch.empty((B, D), dtype=F32, device=feat.device)
    score = torch.empty((B, C), dtype=F32, device=feat.device)
    check(load_library().aim_head_fwd(feat.data_ptr(), _p(drop), W.data_ptr(), _p(bias), pooled.data_ptr(),
                                      score.data_ptr(), B, T, D, C, _stream()), "aim_head_fwd")
    return pooled, score


def head_bwd(dscore, pooled, drop, W, T, need_dfeat=True):
    """-> (dW [C, D], db [C], dfeat [B, T, D] or None)."""
    _chk(dscore, F32, "dscore"); _chk(pooled, F32, "pooled"); _chk(drop, F32, "drop"); _chk(W, F32, "W")
    B, C = dscore.shape
    D = W.shape[1]
    assert dscore.is_contiguous() and pooled.is_contiguous()
    dW = torch.zeros((C, D), dtype=F32, device=W.device)
    db = torch.zeros((C,), dtype=F32, device=W.device)
    dfeat = torch.empty((B, T, D), dtype=F32, device=W.device) if need_dfeat else None
    check(load_library().aim_head_bwd(dscore.data_ptr(), pooled.data_ptr(), _p(drop), W.data_ptr(), dW.data_ptr(),
                                      db.data_ptr(), _p(dfeat), B, T, D, C, _stream()), "aim_head_bwd")
    return dW, db, dfeat


def ce_soft(score, label, class_weight=None, need_grad: bool = True):
    """-> (out [1] f32 = soft / class-weighted CE, dscore [B, C] or None): ``aim_ce_soft`` (label [B, C] f32)."""
    _chk(score, F32, "score"); _chk(label, F32, "label"); _chk(class_weight, F32, "class_weight")
    B, C = score.shape
    assert score.is_contiguous() and label.is_contiguous() and label.shape == score.shape
    assert class_weight is None or (class_weight.is_contiguous() and class_weight.numel() == C)
    dscore = torch.empty_like(score) if need_grad else None
    ws = torch.empty((B, 2), dtype=F32, device=score.device)
    out = torch.empty((1,), dtype=F32, device=score.device)
    check(load_library().aim_ce_soft(score.data_ptr(), label.data_ptr(), _p(class_weight), _p(dscore), ws.data_ptr(),
                                     out.data_ptr(), B, C, _stream()), "aim_ce_soft")
    return out, dscore


def ce_topk(score, label, k2: int = 5, need_grad: bool = True):
    """-> (out3 = [mean CE, top-1, top-k2] f32, dscore [B, C] = (softmax - onehot) / B or None)."""
    _chk(score, F32, "score")
    if label.dtype != torch.int64 or not label.is_cuda:
        raise TypeError("ce_topk: label must be an int64 GPU tensor")
    B, C = score.shape
    assert score.is_contiguous() and label.numel() == B
    dscore = torch.empty_like(score) if need_grad else None
    ws = torch.empty((B, 4), dtype=F32, device=score.device)
    out3 = torch.empty((3,), dtype=F32, device=score.device)
    check(load_library().aim_ce_topk(score.data_ptr(), label.data_ptr(), _p(dscore), ws.data_ptr(), out3.data_ptr(), B, C,
                                     k2, _stream()), "aim_ce_topk")
    return out3, dscore


class CastTable:
    """Device-resident table of (fp32 src -> bf16 dst [transposed]) casts, run in one launch."""

    def __init__(self, entries, device):
        import struct
        self.keep = entries            # keep the tensors alive: the table holds raw pointers
        raw = b"".join(struct.pack("<QQiiii", src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1], dst.stride(0),
                                   int(tr)) for src, dst, tr in entries)
        for src, dst, tr in entries:       # tr: False / True = bf16 cast (plain / transposed); 2 = fp32 copy
            _chk(src, F32, "src"); _chk(dst, F32 if tr == 2 else BF16, "dst")
            assert src.dim() == 2 and src.is_contiguous() and src.numel() < 2 ** 31
            assert tuple(dst.shape) == ((src.shape[1], src.shape[0]) if tr is True or tr == 1 else tuple(src.shape))
        self.n = len(entries)
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        self.ptrs = tuple(src.data_ptr() for src, _, _ in entries)

    def run(self):
        check(load_library().aim_cast_multi(self.table.data_ptr(), self.n, _stream()), "aim_cast_multi")


# ---- reference-precision (fp32) forward path: include/aim_kernels.h, "Reference-precision" section ----------------------
def gemm_f32(a: torch.Tensor, w: torch.Tensor, epi: int, out: torch.Tensor, *, bias=None, resid=None, af=None, at=None,
             vec=None, bt=None, ntok: int = 0, act: int = 0, n_split: int = 0, act2: int = 0, ldv: Optional[int] = None,
             batch: int = 1, stride_a: int = 0, stride_w: int = 0, M: Optional[int] = None, N: Optional[int] = None,
             K: Optional[int] = None, lda: Optional[int] = None, ldw: Optional[int] = None, ldo: Optional[int] = None,
             out2=None, aux=None):
    """``out(f32) = epilogue(a @ w.T)`` with fp32 operands on the f32 MFMA; ``epi`` in (EPI_BF16 = linear, EPI_ACT, EPI_DACT,
    EPI_F32).  ``out2`` (EPI_ACT): receives the f32 pre-activation; ``aux`` (EPI_DACT): that pre-activation."""
    for n_, t_ in (("a", a), ("w", w), ("out", out), ("bias", bias), ("resid", resid), ("af", af), ("at", at), ("vec", vec), ("bt", bt),
                   ("out2", out2), ("aux", aux)):
        _chk(t_, F32, n_)
    g = GemmArgs()
    g.A, g.W = a.data_ptr(), w.data_ptr()
    g.M = a.shape[0] if M is None else M
    g.K = a.shape[1] if K is None else K
    g.N = w.shape[0] if N is None else N
    g.lda = a.stride(0) if lda is None else lda
    g.ldw = w.stride(0) if ldw is None else ldw
    g.strideA, g.strideW = stride_a, stride_w
    g.bias, g.resid = _p(bias), _p(resid)
    g.ldr = resid.stride(0) if resid is not None else 0
    g.af, g.at, g.vec, g.bt = _p(af), _p(at), _p(vec), _p(bt)
    g.ldv = (vec.stride(0) if ldv is None else ldv) if vec is not None else 0
    g.ntok = ntok
    g.out = out.data_ptr()
    g.ldo = (out.stride(-2) if out.dim() >= 2 else g.N) if ldo is None else ldo
    g.act, g.n_split, g.act2, g.scale = act, n_split, act2, 1.0
    if out2 is not None:
        g.out2, g.ldo2 = out2.data_ptr(), out2.stride(0)
    if aux is not None:
        g.aux, g.ldaux = aux.data_ptr(), aux.stride(0)
    check(load_library().aim_gemm_f32(byref(g), epi, batch, _stream()), "aim_gemm_f32")
    return out


def attn_fwd_f32(qkv, out, BT, N, H):
    _chk(qkv, F32, "qkv"); _chk(out, F32, "out")
    check(load_library().aim_attn_fwd_f32(qkv.data_ptr(), out.data_ptr(), BT, N, H, _stream()), "aim_attn_fwd_f32")


def cls_attn_fwd_f32(qkv, row_stride: int, out_cls, B, T, H):
    _chk(qkv, F32, "qkv"); _chk(out_cls, F32, "out_cls")
    check(load_library().aim_cls_attn_fwd_f32(qkv.data_ptr(), int(row_stride), out_cls.data_ptr(), B, T, H, _stream()),
          "aim_cls_attn_fwd_f32")


def lambda_f32(scores, qkv, kx, lam, one_minus, BT, N, D, scale):
    for n_, t_ in (("scores", scores), ("qkv", qkv), ("kx", kx), ("lam", lam), ("one_minus", one_minus)):
        _chk(t_, F32, n_)
    check(load_library().aim_lambda_f32(scores.data_ptr(), scores.stride(-2), qkv.data_ptr(), kx.data_ptr(), kx.stride(0),
                                        lam.data_ptr(), _p(one_minus), BT, N, D, scale, _stream()), "aim_lambda_f32")


def embed_ln_f32(tok, cls, pos, temporal, gamma, beta, x, B, T, N, D, eps=1e-5, pre=None, mean=None, rstd=None):
    """``pre`` / ``mean`` / ``rstd`` (all or none): ln_pre's input rows and statistics, for the backward."""
    for n_, t_ in (("tok", tok), ("cls", cls), ("pos", pos), ("temporal", temporal), ("gamma", gamma), ("beta", beta), ("x", x),
                   ("pre", pre), ("mean", mean), ("rstd", rstd)):
        _chk(t_, F32, n_)
    check(load_library().aim_embed_ln_f32(tok.data_ptr(), cls.data_ptr(), pos.data_ptr(), temporal.data_ptr(), gamma.data_ptr(),
                                          beta.data_ptr(), x.data_ptr(), _p(pre), _p(mean), _p(rstd), B, T, N, D, eps, _stream()),
          "aim_embed_ln_f32")


def attn_bwd_f32(qkv, dout, dqkv, BT, N, H):
    """dqkv [BT*N, 3D] (written) from the fused f32 qkv rows and d(out) [BT*N, D]; probabilities recomputed."""
    for n_, t_ in (("qkv", qkv), ("dout", dout), ("dqkv", dqkv)):
        _chk(t_, F32, n_)
    lib = load_library()
    nbytes = lib.aim_attn_bwd_f32_workspace_bytes(BT, N, H)
    ws = torch.empty((nbytes // 4,), dtype=F32, device=qkv.device)
    check(lib.aim_attn_bwd_f32(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), BT, N, H, ws.data_ptr(), nbytes, _stream()),
          "aim_attn_bwd_f32")


def cls_attn_bwd_f32(qkv, row_stride: int, dout_cls, dqkv, B, T, H):
    """d(out_cls) [B*T, D] -> ADDED into the class rows of dqkv (call after ``attn_bwd_f32``)."""
    for n_, t_ in (("qkv", qkv), ("dout_cls", dout_cls), ("dqkv", dqkv)):
        _chk(t_, F32, n_)
    check(load_library().aim_cls_attn_bwd_f32(qkv.data_ptr(), int(row_stride), dout_cls.data_ptr(), dqkv.data_ptr(), B, T, H,
                                              _stream()), "aim_cls_attn_bwd_f32")


def tattn_fwd_f32(qkv, out, B, T, N, H):
    """Stock-AIM temporal attention over the T frames of every token (fp32, frame-major fused qkv rows)."""
    _chk(qkv, F32, "qkv"); _chk(out, F32, "out")
    check(load_library().aim_tattn_fwd_f32(qkv.data_ptr(), out.data_ptr(), B, T, N, H, _stream()), "aim_tattn_fwd_f32")


def tattn_bwd_f32(qkv, dout, dqkv, B, T, N, H):
    """... its backward, ADDED into ``dqkv`` [B*T*N, 3D]."""
    for n_, t_ in (("qkv", qkv), ("dout", dout), ("dqkv", dqkv)):
        _chk(t_, F32, n_)
    check(load_library().aim_tattn_bwd_f32(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), B, T, N, H, _stream()),
          "aim_tattn_bwd_f32")


def wgrad_f32(g, a, dw, db=None, at=None, ntok: int = 0):
    """``dw [Nw, Kw] += g.T @ a``; ``db [Nw] += sum_m at[m % ntok] * g[m]`` (fp32; row-strided views allowed)."""
    for n_, t_ in (("g", g), ("a", a), ("dw", dw), ("db", db), ("at", at)):
        _chk(t_, F32, n_)
    M, Nw = g.shape
    Kw = a.shape[1]
    assert a.shape[0] == M and tuple(dw.shape) == (Nw, Kw) and dw.is_contiguous() and g.stride(1) == 1 and a.stride(1) == 1
    lib = load_library()
    nbytes = lib.aim_wgrad_f32_workspace_bytes(M, Nw, Kw)
    ws = torch.empty((nbytes // 4,), dtype=F32, device=g.device)
    check(lib.aim_wgrad_f32(g.data_ptr(), g.stride(0), a.data_ptr(), a.stride(0), dw.data_ptr(), M, Nw, Kw, _p(db), _p(at), ntok,
                            ws.data_ptr(), nbytes, _stream()), "aim_wgrad_f32")
