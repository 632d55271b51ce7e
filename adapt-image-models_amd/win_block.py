"""What the windowed backbones share (``AIM_FLASH_WIN`` / ``AIM_FLASH`` in aim_flash_win.py, the windowed ``AIM`` in
aim_variant.py), as plain functions called in place: the window geometry and its checks, the residual
stream's layout with a prompt slot, and the temporal window step of a block -- steps 1-3 and the out-projection of the two
module docstrings -- with its backward.  Steps 4, 5 and 6 differ between the two blocks and stay with them.
"""
from . import ops
from .backbone import _DP_RESERVE, BF16, F32, _empty, _Frozen


def clip_window(window_size, T: int, G: int):
    """the reference's ``get_window_size`` (:51-64): an extent that reaches the grid's is clipped to it"""
    return tuple(min(int(w), x) for w, x in zip(window_size, (T, G, G)))


def clip_shift(window_size, T: int, G: int):
    """the shift of the reference's ``get_window_size`` (:51-64): half a window, 0 where the grid does not exceed the window"""
    return tuple(0 if x <= int(w) else int(w) // 2 for w, x in zip(window_size, (T, G, G)))


def check_window(window_size, T: int, G: int, divide_note: str = ""):
    """a constructor's check of its ``window_size`` on the T x G x G grid; ``divide_note`` ends the first message"""
    win = clip_window(window_size, T, G)
    if len(tuple(window_size)) != 3 or any(w <= 0 for w in win) or T % win[0] or G % win[1] or G % win[2]:
        raise ValueError(f"window_size={tuple(window_size)} (clipped to {win}) does not divide the {T} x {G} x {G} grid{divide_note}")
    if win[0] * win[1] * win[2] > ops.WIN_ATTN_MAX_S:
        raise ValueError(f"{win[0] * win[1] * win[2]} tokens per window: the window attention kernels take at most "
                         f"{ops.WIN_ATTN_MAX_S}")


def check_win_clip(T: int, N: int, prompt):
    """the limits on a forward's clip: T frames of N tokens (and the prompt's slot)"""
    if N + int(prompt) > 288:
        raise ValueError(f"{N + int(prompt)} tokens per frame: the spatial attention kernels take at most 288")
    if T > 32:
        raise ValueError(f"{T} frames: the class-token attention kernels take at most 32")


def to_slot_layout(x0, BT, N, P):
    """the embedding [BT*N, D] in the residual stream's layout of P rows per frame"""
    if P == N:
        return x0
    # once per forward: into the P-row layout (row N = the prompt's slot, zero until block 0 fills it)
    D = x0.shape[1]
    x = _empty((BT * P, D), F32, x0.device)
    x.view(BT, P, D)[:, :N] = x0.view(BT, N, D)
    x.view(BT, P, D)[:, N] = 0
    return x


def from_slot_layout(dxb, BT, N, P):
    """the stream's gradient [BT*P, D] as the embedding's [BT*N, D]"""
    if P == N:
        return dxb
    # once per backward: back to the embedding's N tokens per frame (the slot's row is zero)
    D = dxb.shape[1]
    return dxb.view(BT, P, D)[:, :N].contiguous().view(BT * N, D)


def win_temporal_forward(x, fz: _Frozen, B, T, N, P, H, window, shift, cut_t: bool):
    """x [B*T*P, D] f32 -> ta = [cls_attn | windows_attn] Wo^T + bo [B*T*P, D] bf16 (zero-input slot rows), and what the
    backward reads.  shift: None or the block's (st, sh, sw); cut_t: whether the t axis is then cut at st like h and w (AIM)
    or keeps whole windows that wrap (AIM_FLASH) -- ``win_geom``'s argument of that name in csrc/win_attn.hip."""
    dev = x.device
    M, D = x.shape
    BT = B * T
    xv = lambda t: t.view(BT, P, -1)
    # ---- 1: ln_1 and the QKV projection over every row
    xl = _empty((M, D), BF16, dev)
    mean1, rstd1 = _empty((M,), F32, dev), _empty((M,), F32, dev)
    ops.layernorm_fwd(x, fz.g1, fz.b1, M, D, D, y_bf16=xl, mean=mean1, rstd=rstd1)
    qkv = _empty((M, 3 * D), BF16, dev)
    ops.gemm(xl, fz.Wqkv, ops.EPI_BF16, qkv, bias=fz.bqkv)
    del xl
    # ---- 2, 3: window attention on the patch rows, class-token attention on the class rows, into one [M, D] buffer
    at_ = _empty((M, D), BF16, dev)
    lse_w = _empty((BT, H, P), F32, dev)
    if shift is None:
        ops.win_attn_fwd(qkv, at_, lse_w, B, T, N, H, window, P=P)
    elif cut_t:
        ops.win_attn_fwd_cut(qkv, at_, lse_w, B, T, N, H, window, shift, P=P)
    else:
        ops.win_attn_fwd_shift(qkv, at_, lse_w, B, T, N, H, window, shift, P=P)
    ot, probs = _empty((BT, D), BF16, dev), _empty((B, H, T, T), F32, dev)
    ops.cls_attn_fwd(qkv, ot, probs, B, T, P, H)
    xv(at_)[:, 0] = ot
    if P != N:
        xv(at_)[:, N] = 0
    # ---- out_proj
    ta = _empty((M, D), BF16, dev)
    ops.gemm(at_, fz.Wo, ops.EPI_BF16, ta, bias=fz.bo)
    return ta, dict(mean1=mean1, rstd1=rstd1, qkv=qkv, at=at_, lse_w=lse_w, probs=probs)


def win_prompt_grad(dx1b, BT, N, P):
    """the slot's row of d(loss)/d(x1) as fp32 [BT, D], or None without a prompt; the row is zeroed"""
    if P == N:
        return None
    # the slot's row IS d(prompt) = one more gradient of ta's class rows; nothing else flows through the slot
    dprompt = dx1b.view(BT, P, -1)[:, N].to(F32, copy=True).contiguous()
    dx1b.view(BT, P, -1)[:, N] = 0
    return dprompt


def win_temporal_backward(dta, dx1b, c, fz: _Frozen, dqkv, delta, dxl, B, T, N, P, H, window, shift, cut_t: bool, dprompt):
    """dta = d(loss)/d(ta) without the prompt's share, dx1b = d(loss)/d(x1) -> d(loss)/d(x) [M, D] bf16 with zero slot rows.
    dqkv, delta, dxl: the spatial step's buffers of those shapes, overwritten, as is dta, whose storage the result takes.
    window, shift, cut_t: the forward's."""
    dev = dta.device
    M, D = dta.shape
    BT = B * T
    xv = lambda t: t.view(BT, P, -1)
    if dprompt is not None:
        ops.add_rows(dta, P * D, dprompt)             # class rows: row 0 of every frame
    dat = _empty((M, D), BF16, dev)
    ops.gemm(dta, fz.WoT, ops.EPI_BF16, dat, reserve_cus=_DP_RESERVE)
    # ---- 2, 3: the two attentions write disjoint rows of d(qkv): the window kernel the patch rows, cls_attn_bwd ADDS into
    # the class rows (zeroed first, with the slot's)
    xv(dqkv)[:, 0] = 0
    if P != N:
        xv(dqkv)[:, N] = 0
    if shift is None:
        ops.win_attn_bwd(c["qkv"], c["at"], dat, c["lse_w"], delta, dqkv, B, T, N, H, window, P=P)
    elif cut_t:
        ops.win_attn_bwd_cut(c["qkv"], c["at"], dat, c["lse_w"], delta, dqkv, B, T, N, H, window, shift, P=P)
    else:
        ops.win_attn_bwd_shift(c["qkv"], c["at"], dat, c["lse_w"], delta, dqkv, B, T, N, H, window, shift, P=P)
    ops.cls_attn_bwd(c["qkv"], c["probs"], xv(dat)[:, 0].contiguous(), dqkv, B, T, P, H)
    del dat
    ops.gemm(dqkv, fz.WqkvT, ops.EPI_BF16, dxl, reserve_cus=_DP_RESERVE)
    dxb = dta           # dead since the WoT GEMM, and the caller's frame holds it (and dqkv) until this returns: no new buffer
    ops.layernorm_bwd(dxl, c["x"], fz.g1, c["mean1"], c["rstd1"], M, D, lddy=D, ldx=D, lddx=D, dres=dx1b, dx_bf16=dxb)
    if P != N:
        xv(dxb)[:, N] = 0
    return dxb
