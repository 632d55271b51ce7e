#!/usr/bin/env python3
"""Generate the ViT_CLIP_ZEROI2V ``linear_adapter=True`` golden vectors under tests/golden/ from the REAL reference.

Runs only where the reference tree is (no test needs it); modelled on make_golden_zeroi2v.py, whose loader it uses.  No
reference source is copied: only the reference's numeric outputs are stored; weights are ``oracle.synth_state_dict`` of the
backbone's parameter shapes (name-seeded: every ``D_fc2`` is live), the adapters' weights scaled by ``ADAPTER_SCALE``; the
inputs are rebuilt from seeds by the tests.

    python tests/golden/make_golden_zeroi2v_linear.py

Writes zeroi2v_linear_tiny_{a,b,c,d}.npz.  Geometry: img 32, patch 16 (N = 5), head width 64, B = 2.  Gradients of more than
``WHOLE`` elements are stored as ``SAMPLE`` elements at seeded positions plus their fp64 sum and sum of squares, every
parameter's shape as ``shape.<name>``.  Three further numbers per case, the rel-L2 change of the reference's output when
  ``attn_effect``  the attention adapters are replaced by the identity,
  ``mlp_effect``   the two MLP adapters are replaced by the identity,
  ``skip_effect``  the two MLP adapters' skip is counted once instead of twice (they return only their low-rank term):
the generator refuses a case where any of them is below 7.5e-2 (five times the bf16 output bound of the GPU test, the rule
make_golden_zeroi2v.py's ``MIN_SHIFT_EFFECT`` follows), so that a backbone that drops an adapter family or un-doubles the skip
cannot pass.  Case a runs in train mode: the linear branch draws no DropPath factor, which the generator asserts.
"""
import logging
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_imagenet import SAMPLE, WHOLE, randn, sample_index  # noqa: E402,F401
from make_golden_zeroi2v import load_reference_zeroi2v  # noqa: E402

IMG, PATCH, B = 32, 16, 2
# name -> (T, width, heads, layers, bottleneck, train, with_t_cls_token, share_adapter, seed)
CASES = {
    "a": (8, 256, 4, 3, 64, True, True, False, 5100),
    "b": (16, 256, 4, 2, 64, False, True, True, 5200),
    "c": (32, 384, 6, 2, 96, False, True, False, 5300),
    "d": (8, 128, 2, 2, 32, False, False, True, 5400),
}
DROP_RATE = 0.5
MIN_EFFECT = 7.5e-2
ADAPTER_SCALE = 0.5          # on every linear adapter's two weights: the low-rank term is a quarter of synth_state_dict's


def case_state(tag):
    """the case's fp32 state dict (shared with the tests)"""
    import zeroi2v_linear_ref as ZL
    from oracle import vit_clip_oracle as O
    T, D, H, L, r, train, tcls, share, seed = CASES[tag]
    st = O.synth_state_dict(ZL.backbone_param_shapes(IMG, T, PATCH, D, L, tcls, share, r), seed=seed)
    for k in st:
        if ("Attn_Adapter" in k or "MLP_Adapter" in k) and k.endswith(".weight"):
            st[k] = st[k] * ADAPTER_SCALE
    return st


class _LowRankOnly(nn.Module):
    """a Linear_Adapter without its skip connection"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner.D_fc2(self.inner.D_fc1(x))


def _swapped(m, names, make):
    """context: the modules `names` of every block replaced by make(module)"""
    class Ctx:
        def __enter__(self_):
            self_.saved = [(blk, n, getattr(blk, n)) for blk in m.transformer.resblocks for n in names if hasattr(blk, n)]
            for blk, n, mod_ in self_.saved:
                setattr(blk, n, make(mod_))

        def __exit__(self_, *exc):
            for blk, n, mod_ in self_.saved:
                setattr(blk, n, mod_)
    return Ctx()


def gen_case(mod, tag):
    from oracle import vit_clip_oracle as O
    logging.getLogger("ref").setLevel(logging.ERROR)
    T, D, H, L, r, train, tcls, share, seed = CASES[tag]
    m = mod.ViT_CLIP_ZEROI2V(IMG, T, PATCH, D, L, H, drop_path_rate=DROP_RATE if train else 0.0, adapter_scale=0.5,
                             with_t_cls_token=tcls, share_adapter=share, bottleneck=r, linear_adapter=True)
    m.init_weights()
    # the init quirks the package must keep: only the names that contain 'MLP_Adapter' are matched by the zeroing loops
    for n, p in m.named_parameters():
        if "D_fc2" in n and "Attn_Adapter" in n and n.endswith("weight"):
            assert float(p.abs().max()) > 0, n
        if "D_fc2" in n and ("MLP_Adapter" in n or "T_Adapter" in n):
            assert float(p.abs().max()) == 0, n
    st = case_state(tag)
    msg = m.load_state_dict(st, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    m.train() if train else m.eval()
    imgs = randn((B, 3, T, IMG, IMG), seed + 1)
    g = randn((B, D, T, 1, 1), seed + 2)
    drawn = sys.modules["timm.models.layers"].DropPath.drawn
    del drawn[:]
    y = m(imgs)
    assert not drawn                                   # no DropPath in the linear branch, train mode or not
    params = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(n for n, _ in params) == sorted(O.trainable_names(st))
    per = (12 if share else 20) + 4 + (4 if tcls else 0)
    assert len(params) == per * L + 3 and per in (28, 24, 20, 16)
    grads = torch.autograd.grad(y, [p for _, p in params], g)
    assert all(float(gr.abs().max()) > 0 for gr in grads)
    attn = ("Attn_Adapter_in", "Attn_Adapter_q", "Attn_Adapter_k", "Attn_Adapter_v", "Attn_Adapter_out")
    mlp = ("MLP_Adapter_in", "MLP_Adapter_out")
    effects = {}
    for key, names, make in (("attn_effect", attn, lambda _: nn.Identity()), ("mlp_effect", mlp, lambda _: nn.Identity()),
                             ("skip_effect", mlp, _LowRankOnly)):
        with _swapped(m, names, make), torch.no_grad():
            y0 = m(imgs)
        effects[key] = float((y.detach() - y0).norm() / y.detach().norm())
        assert effects[key] >= MIN_EFFECT, (tag, key, effects[key])
    names = [n for n, _ in m.named_parameters()]
    out = dict(y=y.detach(), meta=np.array([D, H, L, B, T, seed, int(train), int(tcls), int(share), r]), names=np.array(names),
               trainable=np.array([n for n, _ in params]), **{k: np.float64(v) for k, v in effects.items()})
    out.update({"shape." + n: np.array(tuple(p.shape), dtype=np.int64) for n, p in m.named_parameters()})
    for k, ((n, _), gr) in enumerate(zip(params, grads)):
        if gr.numel() <= WHOLE:
            out["grad." + n] = gr
        else:
            flat = gr.reshape(-1)
            out["grad." + n + ".val"] = flat[sample_index(flat.numel(), seed * 1000 + k)]
            out["grad." + n + ".sum"] = flat.double().sum()
            out["grad." + n + ".sq"] = (flat.double() ** 2).sum()
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, f"zeroi2v_linear_tiny_{tag}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 400_000, os.path.getsize(path)
    print(f"{tag}: effects {effects}, {os.path.getsize(path)} bytes")


def main():
    torch.set_num_threads(8)
    mod = load_reference_zeroi2v()
    for tag in CASES:
        gen_case(mod, tag)


if __name__ == "__main__":
    main()
