"""tests/swin_attn_cases.py judged on the CPU: its address rule is the reference's roll / partition / mask, its bounds accept an
emulation of the kernels' arithmetic and reject the defects they are meant to catch."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_attn_cases as W  # noqa: E402

CASES = {c.name: c for c in W.cases()}
# the case each defect is planted in: a shifted window case for the mask and the shift, the temporal case with the most
# frame tokens for the temporal index
PLANTED = {"bias_T": ("win/f2r14w7s3h1/unit", "t/B1T16L64h4/unit"), "no_mask": ("win/f2r14w7s3h1/unit", "win/f3r8w4s2h3/peaked"),
           "shift_sign": ("win/f2r14w7s3h1/unit", "win/f1r16w8s4h2/unit"), "swap_hw": ("win/f1r7w7s0h2/unit", "win/f1r56w7s3h4/unit"),
           "t_neg": ("t/B1T3L10h1/unit", "t/B1T32L8h1/peaked")}


def test_the_case_list_is_the_one_the_kernels_were_asked_to_pass():
    assert tuple(c.dims for c in W.cases() if c.kind == "win" and c.family == "unit") == W.WIN_SHAPES
    assert tuple(c.dims for c in W.cases() if c.kind == "t" and c.family == "unit") == W.T_SHAPES
    assert W.WIN_SHAPES == ((2, 14, 7, 3, 1), (1, 7, 7, 0, 2), (1, 16, 8, 4, 2), (3, 8, 4, 2, 3), (1, 56, 7, 3, 4))
    assert W.T_SHAPES == ((1, 1, 5, 1), (2, 2, 49, 2), (1, 3, 10, 1), (1, 16, 64, 4), (1, 32, 8, 1))
    assert {c.family for c in W.cases()} == {"unit", "peaked"} and len(CASES) == 20


@pytest.mark.parametrize("dims", W.WIN_SHAPES + ((1, 12, 4, 1, 1), (2, 8, 8, 0, 1)))
def test_address_and_mask_rule_is_the_reference_roll_partition_and_mask(dims):
    frames, res, w, s, H = dims
    idx, allow = W.geometry(W.Case("g", "win", dims))
    ridx, rallow = W.rolled_geometry(frames, res, w, s)
    assert torch.equal(idx, ridx) and torch.equal(allow, rallow)
    assert sorted(idx.reshape(-1).tolist()) == list(range(frames * res * res))          # every row has one writer
    if dims == (2, 14, 7, 3, 1):           # 1, 2, 2 and 4 regions in the four windows of a frame
        assert [len({tuple(r.tolist()) for r in a}) for a in allow[:4]] == [1, 2, 2, 4]


def test_peaked_logits_are_peaked():
    for name in ("win/f1r16w8s4h2", "t/B1T32L8h1"):
        tops = {}
        for fam in W.FAMILIES:
            c = CASES[f"{name}/{fam}"]
            inp = W.make_inputs(c)
            idx, _ = W.geometry(c)
            q, k, _ = W.gather(inp["qkv"], idx, c.H, 3)
            tops[fam] = float((q @ k.transpose(-1, -2) * W.SCALE).abs().amax())
        assert tops["peaked"] > 3 * tops["unit"] and tops["peaked"] > 15


@pytest.mark.parametrize("name", sorted(CASES))
def test_bounds_accept_the_emulated_kernels(name):
    c = CASES[name]
    inp = W.make_inputs(c)
    res = W.compare(c, inp, W.emulate(c, inp))
    assert set(res) == {"out", "lse", "dq", "dk", "dv", "dbias", "dtable"}
    assert all(r <= 1.0 for r in res.values()), res


def test_one_key_sequences_have_zero_score_gradients():
    c = CASES["t/B1T1L5h1/peaked"]
    inp = W.make_inputs(c)
    got = W.emulate(c, inp)
    C = c.H * W.HD
    assert not got["dqkv"][:, :2 * C].any() and not got["dbias"].any() and not got["dtable"].any()
    assert got["dqkv"][:, 2 * C:].any()


# ------------------------------------------------------------------ the chunk and sweep lists -------------------------------
NEW = {c.name: c for c in W.chunk_cases() + W.sweep_cases()}
# where geometry lets each new defect show:
#   stale_region      a shifted chunk case: per = 3 (or 8) is coprime to the 4 (or 9) windows of a frame, so a chunk's later
#                     windows have other region patterns than its first one
#   db_last_only      any chunk case (per >= 3: two or more sequences of every full chunk are lost)
#   drop_ragged_chunk any chunk case (the last chunk is short in all of them); in the deep case the 3 lost sequences of 2043 are
#                     frame 226's bottom row of windows, whose two-token regions still carry a gradient
#   max_before_mask,
#   penalty_mask      cross_hot on one-coordinate shifts: every masked score is 126 or more above every allowed one
#   dbias_scaled      anywhere with S > 1; planted at per = 3, on a temporal and on a window sweep case
NEW_PLANTED = {"stale_region": ("chunk/win/f35r14w7s3h16/unit", "chunk/win/f35r8w4s2h16/peaked", "chunk/win/f227r6w2s1h4/unit"),
               "db_last_only": ("chunk/win/f35r16w8s4h16/unit", "chunk/t/B1T5L140h16/unit", "chunk/win/f227r6w2s1h4/unit"),
               "drop_ragged_chunk": ("chunk/win/f35r14w7s3h16/unit", "chunk/t/B1T32L70h32/unit", "chunk/win/f227r6w2s1h4/peaked"),
               "max_before_mask": ("sweep/win/w7s1/cross_hot", "sweep/win/w8s7/cross_hot", "sweep/win/w5s4/cross_hot"),
               "penalty_mask": ("sweep/win/w7s1/cross_hot", "sweep/win/w8s7/cross_hot", "sweep/win/w5s4/cross_hot"),
               "dbias_scaled": ("chunk/win/f35r14w7s3h16/unit", "sweep/t/T9/unit", "sweep/win/w3s1/unit")}


def test_the_new_lists_are_the_ones_asked_for():
    assert len(NEW) == len(W.chunk_cases()) + len(W.sweep_cases()) and not set(NEW) & set(CASES)
    sweep = W.sweep_cases()
    t = [c for c in sweep if c.kind == "t"]
    assert sorted({c.dims for c in t}) == [(2, T, 5, 2) for T in range(1, 33)]
    win = [c for c in sweep if c.kind == "win"]
    assert sorted({c.dims for c in win}) == [(2, 3 * w, w, s, 2) for w in range(1, 9) for s in range(w)] and len({c.dims for c in win}) == 36
    for c in sweep:
        fams = {d.family for d in sweep if d.kind == c.kind and d.dims == c.dims}
        if c.kind == "t":
            assert fams == ({"unit", "peaked", "bias_big", "zero_do"} if c.dims[1] % 7 == 0 else {"unit"}), c.name
        else:
            w, s = c.dims[2], c.dims[3]
            assert fams == (set(W.ALL_FAMILIES) if w >= 5 and s in (1, w - 1) else {"unit"}), c.name
    assert {c.family for c in W.chunk_cases()} == {"unit", "peaked"}
    assert len({c.seed for c in list(NEW.values()) + list(CASES.values())}) == len(NEW) + len(CASES)


def test_chunks_is_the_kernels_rule_on_the_shapes_the_tests_and_the_recipe_run():
    assert all(W.chunks(c.nseq, c.H)[1] == 1 for c in CASES.values())           # the 20 first cases never walk
    assert W.chunks(16384, 4) == (256, 64)                                     # the k400 step's first stage
    assert W.chunks(1, 1) == (1, 1) and W.chunks(1024, 1) == (1024, 1) and W.chunks(1025, 1) == (513, 2)


def test_chunk_cases_walk_several_sequences_with_a_short_last_chunk():
    seen = set()
    for c in W.chunk_cases():
        nch, per = W.chunks(c.nseq, c.H)
        last = c.nseq - (nch - 1) * per
        assert per >= 3 and 0 < last < per, (c.name, nch, per, last)
        if c.kind == "win":
            frames, res, w, s, _ = c.dims
            assert s > 0 and math.gcd(per, (res // w) ** 2) == 1, c.name
            # consecutive sequences of one workgroup with different region patterns, and chunks that straddle frames
            _, allow = W.geometry(c)
            assert any(not torch.equal(allow[q], allow[q + 1]) for q in range(0, per - 1)), c.name
            assert any((k * per) // (res // w) ** 2 != (k * per + per - 1) // (res // w) ** 2 for k in range(nch - 1)), c.name
        seen.add((c.kind, W.cap(c.S), c.S, per, nch, last))
    assert seen == {("win", 64, 49, 3, 47, 2), ("win", 64, 64, 3, 47, 2), ("win", 32, 16, 3, 47, 2), ("t", 32, 5, 3, 47, 2),
                    ("t", 32, 32, 3, 24, 1), ("win", 32, 4, 8, 256, 3)}


@pytest.mark.parametrize("w", range(1, 9))
def test_address_and_mask_rule_at_every_sweep_geometry(w):
    for s in range(w):
        c = NEW[f"sweep/win/w{w}s{s}/unit"]
        frames, res = c.dims[0], c.dims[1]
        idx, allow = W.geometry(c)
        ridx, rallow = W.rolled_geometry(frames, res, w, s)
        assert torch.equal(idx, ridx) and torch.equal(allow, rallow), c.name
        assert sorted(idx.reshape(-1).tolist()) == list(range(frames * res * res))
        assert torch.equal(W.row_regions(c)[idx][:, :, None] == W.row_regions(c)[idx][:, None, :], allow)
        lone = W.lone_tokens(c)
        if w > 1 and s in (1, w - 1):      # a one-coordinate region: the corner token of the corner window is alone
            assert lone.any() and lone[-1, 0 if s == w - 1 and w > 2 else -1], c.name
        if s == 0:
            assert not lone.any() or w == 1


@pytest.mark.parametrize("name", sorted(NEW))
def test_bounds_accept_the_emulated_kernels_on_the_new_cases(name):
    c = NEW[name]
    inp = W.make_inputs(c)
    got = W.emulate(c, inp)
    res = W.compare(c, inp, got)
    assert set(res) == {"out", "lse", "dq", "dk", "dv", "dbias", "dtable"}
    assert all(r <= 1.0 for r in res.values()), res
    C = c.H * W.HD
    if c.family == "zero_do":
        h = W.zero_head(c)
        d = got["dqkv"].view(c.rows, 3, C)[:, :, h * W.HD:(h + 1) * W.HD]
        assert not d.any() and not got["dbias"][h].any() and not got["dtable"][:, h].any()
        assert c.H > 1 and got["dqkv"].any() and got["dbias"].any()
    lone = W.lone_tokens(c)
    if lone.any() and c.S > 1:             # p = 1: out = v, dv = dO, dq = dk = 0 bit for bit
        rows = W.geometry(c)[0][lone]
        d, qkv = got["dqkv"].view(c.rows, 3, C), inp["qkv"].view(c.rows, 3, C)
        assert torch.equal(got["out"][rows], qkv[rows, 2]) and torch.equal(d[rows, 2], inp["do"][rows])
        assert not d[rows, 0].any() and not d[rows, 1].any()


def test_cross_hot_puts_every_masked_score_far_above_every_allowed_one():
    for c in NEW.values():
        if c.family != "cross_hot":
            continue
        inp = W.make_inputs(c)
        assert torch.equal(inp["qkv"].float().to(W.BF16), inp["qkv"]) and W.HOT_Q * W.HOT_K * W.SCALE > 135
        idx, allow = W.geometry(c)
        q, k, _ = W.gather(inp["qkv"], idx, c.H, 3)
        z = q @ k.transpose(-1, -2) * W.SCALE + W.dense_bias(inp["table"].double(), W.bias_index(c), c.S)[None]
        al = allow[:, None].expand_as(z)
        assert (~al).any() and float(z[~al].min()) - float(z[al].max()) > 40, c.name
        assert float(z[~al].min()) - float(z[al].max()) > 110, c.name       # the -100 mask and the fp32 exp2 both give way
        # the one-hot features add exactly nothing to a pair of one region
        hot = q[..., :9] @ k[..., :9].transpose(-1, -2)
        assert not hot[al].any() and float(hot[~al].min()) == W.HOT_Q * W.HOT_K, c.name


def test_bias_big_makes_the_bias_the_larger_term():
    n = 0
    for c in NEW.values():
        if c.family != "bias_big":
            continue
        inp = W.make_inputs(c)
        idx, allow = W.geometry(c)
        q, k, _ = W.gather(inp["qkv"], idx, c.H, 3)
        z = q @ k.transpose(-1, -2) * W.SCALE
        bias = W.dense_bias(inp["table"].double(), W.bias_index(c), c.S)[None]
        al = allow[:, None].expand_as(z)
        assert abs(float(bias.abs().amax()) - 40.0) < 1e-4 and float(bias.abs().amax()) > 4 * float(z[al].abs().amax()), c.name
        # the row's largest logit sits where its largest bias sits (but where two table entries nearly tie), and the row's
        # largest logit, so its lse, is within the q k term of its largest bias
        ninf = torch.full((), -float("inf"), dtype=torch.float64)
        top_z = torch.where(al, z + bias, ninf).amax(dim=-1)
        top_b = torch.where(al, bias.expand_as(z), ninf).amax(dim=-1)
        assert float((top_z - top_b).abs().amax()) <= float(z[al].abs().amax()) and float(top_b.abs().mean()) > 8, c.name
        same = torch.where(al, z + bias, ninf).argmax(dim=-1) == torch.where(al, bias.expand_as(z), ninf).argmax(dim=-1)
        assert float(same.double().mean()) > 0.75, c.name
        n += 1
    assert n == 4 + 8


@pytest.mark.parametrize("mut", W.NEW_MUTANTS)
def test_bounds_reject_the_new_planted_defect(mut):
    assert set(NEW_PLANTED) == set(W.NEW_MUTANTS)
    for name in NEW_PLANTED[mut]:
        c = NEW[name]
        inp = W.make_inputs(c)
        res = W.compare(c, inp, W.emulate(c, inp, mut))
        assert max(res.values()) > 1.0, (mut, name, res)
        if mut in ("db_last_only", "drop_ragged_chunk", "dbias_scaled"):      # defects of the bias gradient alone
            assert res["dbias"] > 1.0 and res["dtable"] > 1.0 and max(res[k] for k in ("out", "lse", "dq", "dk", "dv")) <= 1.0, (mut, name, res)
        if mut in ("max_before_mask", "penalty_mask"):
            assert res["out"] > 1.0 and res["lse"] > 1.0, (mut, name, res)
        if mut == "stale_region":
            assert res["out"] > 1.0 and res["dbias"] > 1.0, (mut, name, res)


@pytest.mark.parametrize("mut", W.MUTANTS)
def test_bounds_reject_the_planted_defect(mut):
    assert set(PLANTED) == set(W.MUTANTS)
    for name in PLANTED[mut]:
        c = CASES[name]
        inp = W.make_inputs(c)
        res = W.compare(c, inp, W.emulate(c, inp, mut))
        assert max(res.values()) > 1.0, (mut, name, res)
        if mut in ("bias_T", "t_neg"):      # a defect of the bias alone shows in the bias gradient's fold too
            assert res["out"] > 1.0 and res["dtable"] > 1.0, (mut, name, res)
