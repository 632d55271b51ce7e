"""The windowed AIM (``AIM(wind_attn=True, not_shift=False)``) on the MI355X: the whole backbone against the real reference's
stored outputs and autograd gradients (tests/golden/aim_win_tiny_{a..d}.npz: the reference's roll and -100 mask; eval, train
mode with the drawn per-token-position DropPath masks, no prompt, one head, a t cut), at the recipes' real window geometry
(224 / 16, 32 frames, (32,2,2) cut at (0,1,1) and (16,7,7) cut at (8,3,3)) against the fp32 restatement tests/aim_win_ref.py
(itself held to the fixtures by tests/test_aim_win_cpu.py), the requires_grad contract, and three training steps of the
hmdb51 recipe.

Bounds: 1.5e-2 rel-L2 on the bf16 output and 2.5e-2 on every trainable gradient, as tests/test_aim_flash_gpu.py: the cut
kernels have the rounding points of the shifted and unshifted ones, the rest of the block is the stock AIM block's.  The
fixtures' outputs move by at least 7.5e-2 rel-L2 when the shift is removed, so a backbone that ignored it could not pass.

Measured on MI355X (worst over a case's tensors): see DESIGN.md section 2g."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aim_win_ref as R  # noqa: E402
import test_aim_win_cpu as C  # noqa: E402  (load_case, build)
from test_aim_flash_win_cpu import stored_grad  # noqa: E402
from test_aim_flash_win_gpu import rel  # noqa: E402

OUT_BOUND, GRAD_BOUND = 1.5e-2, 2.5e-2


def inject_masks(m, masks):
    """the drawn DropPath factors (per layer a (d1, d2) pair over the N token positions, or None) as the model's
    factor-times-scale table [L, 2, N] (the block divides the scale out of the first)"""
    blocks = m.transformer.resblocks

    def fake(N, training, dev):
        rows = [torch.stack([torch.ones(N), torch.ones(N)] if mk is None else [t.float() for t in mk]) * float(b.scale)
                for b, mk in zip(blocks, masks)]
        return torch.stack(rows).to(dev).contiguous()

    m._drop_masks = fake


def build(c):
    m = C.build(c)
    m.load_state_dict(c["st"], strict=True)
    m = m.to(DEV).train(c["train"])
    if c["masks"] is not None:
        inject_masks(m, c["masks"])
    return m


@pytest.mark.parametrize("tag", C.TAGS)
def test_bf16_against_reference_fixture(tag):
    c = C.load_case(tag)
    z = c["z"]
    m = build(c)
    y = m(c["imgs"].to(DEV))
    names = [str(n) for n in z["trainable"]]
    byname = dict(m.named_parameters())
    grads = torch.autograd.grad(y, [byname[n] for n in names], c["g"].to(DEV))
    errs = {"y": rel(y, torch.from_numpy(z["y"]))}
    for k, (n, g) in enumerate(zip(names, grads)):
        ref, got, rsum, rsq = stored_grad(z, n, k, c["seed"], g.cpu())
        if float(ref.abs().max()) == 0:
            assert float(g.abs().max()) == 0, n
            continue
        errs[n] = rel(got, ref)
        if rsq is not None:                     # the elements that were not sampled
            errs[n + "|norm"] = abs(float(g.double().norm()) - rsq ** 0.5) / rsq ** 0.5
            errs[n + "|sum"] = abs(float(g.double().sum()) - rsum) / (rsq ** 0.5 * g.numel() ** 0.5)
    worst_g = max((kv for kv in errs.items() if kv[0] != "y"), key=lambda kv: kv[1])
    print(f"aim_win fixture {tag}: output {errs['y']:.3e}, worst gradient {worst_g[1]:.3e} ({worst_g[0]})")
    assert errs["y"] <= OUT_BOUND, errs["y"]
    assert worst_g[1] <= GRAD_BOUND, sorted(errs.items(), key=lambda kv: -kv[1])[:8]


def test_frozen_tensors_get_no_gradient_and_no_grad_forward_is_identical():
    c = C.load_case("a")
    m = build(c)
    imgs = c["imgs"].to(DEV)
    y = m(imgs)
    y.backward(c["g"].to(DEV))
    train = {str(n) for n in c["z"]["trainable"]}
    for n, p in m.named_parameters():
        assert (p.grad is not None) == (n in train), n
        assert p.requires_grad == (n in train), n
    with torch.no_grad():
        y2 = m(imgs)
    assert torch.equal(y.detach(), y2) and not y2.requires_grad
    # a second grad-mode run: same bits, output and gradients (fixed summation orders, no atomics)
    g1 = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    y3 = m(imgs)
    y3.backward(c["g"].to(DEV))
    assert torch.equal(y3.detach(), y.detach())
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g1[n]), n


@pytest.mark.parametrize("tag", ("a", "d"))
def test_the_shift_moves_the_output_by_the_fixtures_shift_effect(tag):
    """the model's blocks with plain windows everywhere (what not_shift=True would issue) against the cut ones: the outputs
    differ by the reference's own figure"""
    c = C.load_case(tag)
    m = build(c)
    imgs = c["imgs"].to(DEV)
    with torch.no_grad():
        y = m(imgs)
        m._block_shift = lambda i, T, G: None
        y0 = m(imgs)
    e = float(c["z"]["shift_effect"])
    assert abs(rel(y0, y) - e) <= OUT_BOUND * (2 + e)


def test_fp8_request_warns_and_runs_bf16(caplog):
    c = C.load_case("d")
    m = build(c)
    imgs = c["imgs"].to(DEV)
    with torch.no_grad():
        y = m(imgs)
        m.set_inference_precision('fp8')
        with caplog.at_level("WARNING", logger="aim_amd"):
            y8 = m(imgs)
    assert torch.equal(y, y8)
    assert any("fp8" in r.getMessage() and "bf16" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("masked", [False, True], ids=["eval", "droppath"])
@pytest.mark.parametrize("window", [(32, 2, 2), (16, 7, 7)], ids=["32x2x2", "16x7x7"])
def test_real_window_geometry_against_the_restatement(window, masked):
    """224 / 16 (G = 14, 198 tokens with the prompt), 32 frames, one clip, 128 wide, 2 heads, 2 layers (block 1 is cut):
    boxes of 32 .. 128 tokens under (32,2,2) / (0,1,1), the recipes' form, and of 72 .. 784 under (16,7,7) / (8,3,3), the t
    cut; reference = tests/aim_win_ref.py in fp32 on the CPU"""
    import aim_amd
    from oracle import vit_clip_oracle as O
    D, H, L, T, B, N = 128, 2, 2, 32, 1, 197
    st = O.synth_state_dict(R.backbone_param_shapes(224, T, 16, D, L), seed=93)
    m = aim_amd.AIM(224, T, 16, D, L, H, drop_path_rate=0.3 if masked else 0.0, adapter_scale=0.5, wind_attn=True,
                    window_size=window, not_shift=False)
    assert m._block_shift(1, T, 14) == {(16, 7, 7): (8, 3, 3), (32, 2, 2): (0, 1, 1)}[window]
    m.init_weights()
    m.load_state_dict(st, strict=True)
    m = m.to(DEV).train(masked)
    masks = None
    if masked:
        gen = torch.Generator().manual_seed(8)
        masks = [tuple((torch.rand(N, generator=gen) < 0.7).float() / 0.7 for _ in range(2)) for _ in range(L)]
        inject_masks(m, masks)
    gen = torch.Generator().manual_seed(9)
    imgs = torch.randn((B, 3, T, 224, 224), generator=gen)
    g = torch.randn((B, D, T, 1, 1), generator=gen)
    y = m(imgs.to(DEV))
    names = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert len(names) == 12 * L + 3
    byname = dict(m.named_parameters())
    grads = torch.autograd.grad(y, [byname[n] for n in names], g.to(DEV))
    sr = {k: v.clone().requires_grad_(k in names) for k, v in st.items()}
    torch.set_num_threads(16)
    yr = R.backbone(imgs, sr, H, T, window, 0.5, True, masks)
    gr = torch.autograd.grad(yr, [sr[n] for n in names], g)
    errs = {n: rel(a, b) for n, a, b in zip(names, grads, gr)}
    ey = rel(y, yr.detach())
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"aim_win real geometry {window} ({'droppath' if masked else 'eval'}): output {ey:.3e}, "
          f"worst gradient {worst[1]:.3e} ({worst[0]})")
    assert ey <= OUT_BOUND, ey
    assert worst[1] <= GRAD_BOUND, sorted(errs.items(), key=lambda kv: -kv[1])[:8]


@pytest.fixture(scope="module")
def training_runs(tmp_path_factory):
    """the reduced hmdb51 recipe's training steps in child processes: default streams twice, then every side / detached
    stream off"""
    off = {"AIM_SIDE_STREAM": "0", "AIM_DETACH_WGRAD": "0", "AIM_DETACH_BIG": "0"}
    out = {}
    for tag, extra in (("run1", {}), ("run2", {}), ("streams_off", off)):
        env = {k: v for k, v in os.environ.items() if k not in off}
        env.update(extra)
        path = str(tmp_path_factory.mktemp("aim_win_train") / f"{tag}.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "aim_win_train_child.py"), path], env=env, timeout=600,
                           capture_output=True, text=True)
        if p.returncode != 0:        # stop at the first failing child: nothing more is started on the GPU
            pytest.fail(f"{tag}: child exited with status {p.returncode}\n{p.stderr[-4000:]}")
        with open(path) as f:
            out[tag] = json.load(f)
    return out


def test_recipe_training_is_finite_and_changes_exactly_the_trainable_set(training_runs):
    r = training_runs["run1"]
    assert r["backbone"] == "AIM" and r["wind_attn"] and r["optimizer"] == "FlatAdamW" and r["window"] == [32, 2, 2] and r["prompt"]
    assert r["frames"] == 32 and r["shifts"] == [None, [0, 1, 1]]
    assert r["in_place"] and r["finite"] and len(r["losses"]) == 3 and all(v == v and abs(v) < 1e4 for v in r["losses"])
    assert len(r["trainable"]) == 12 * 2 + 3 + 2
    changed = sorted(n for n in r["before"] if r["before"][n] != r["after"][n])
    assert changed == r["trainable"]


def test_recipe_training_is_bitwise_reproducible(training_runs):
    a, b = training_runs["run1"], training_runs["run2"]
    assert a["loss_bits"] == b["loss_bits"] and a["after"] == b["after"]


def test_recipe_training_does_not_depend_on_the_streams(training_runs):
    a, b = training_runs["run1"], training_runs["streams_off"]
    assert a["before"] == b["before"]
    assert a["loss_bits"] == b["loss_bits"]
    assert [n for n in a["after"] if a["after"][n] != b["after"][n]] == []
