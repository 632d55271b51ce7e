"""The MLP_Adapter weight gradients as rider workgroups of the block's dgrad GEMMs (backbone.py, ops.WgradRide; DESIGN.md
section 4), at model level: the same seed and clips with AIM_WGRAD_RIDE=0 and =1 in child processes (the library reads the
switch once).

Model: two layers, width 768, patch 16, 14 clips x 8 frames = 22 064 rows -- 261 N = 768 tiles, the smallest shape at which
256 CUs leave spare workgroups in the balanced grid (131 workgroups in two rounds).  The last block runs on its class rows, so
the riders are block 0's.

Riding changes where the rows of D_fc1 / D_fc2's weight and bias gradients are summed and in which chunks, nothing else:
every output and every other gradient must be bit-identical; those four tensors differ by the fp32 summation order of sums of
at most 22 064 terms (expected ~1e-6 relative) and are held to relative L2 1e-4, 25 times inside the 2.5e-3 the top-block
test allows between two forms of the step.  Measured: D_fc1 / D_fc2 of block 0 3.0e-7 (weights) and 7.8e-8 (biases), everything
else bit-identical; 2 rider launches, 44 128 rows (all of both gradients).
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, torch
sys.path.insert(0, %r)
import aim_amd
from aim_amd import ops
from oracle import vit_clip_oracle as O
res, T, patch, D, L, H, B, drop = 224, 8, 16, 768, 2, 12, 14, 0.1
m = aim_amd.ViT_CLIP(res, T, patch, D, L, H, drop)
m.init_weights()
m.load_state_dict(O.synth_state_dict(O.backbone_param_shapes(res, T, patch, D, L), seed=11), strict=True)
m = m.to("cuda").train()
g = torch.Generator().manual_seed(5)
clips = torch.randn((B, 3, T, res, res), generator=g).to("cuda")
head = (torch.randn((D, 16), generator=g) * D ** -0.5).to("cuda")
labels = torch.randint(0, 16, (B,), generator=g).to("cuda")
torch.manual_seed(7)                  # the DropPath draws
y = m(clips)
loss = torch.nn.functional.cross_entropy(y.flatten(2).mean(-1) @ head, labels)
loss.backward()
torch.cuda.synchronize()
out = {"loss": loss.detach().cpu(), "features": y.detach().cpu(),
       "ride.launches": torch.tensor(ops.RIDE_STATS["launches"]), "ride.rows": torch.tensor(ops.RIDE_STATS["rows"])}
for n, p in m.named_parameters():
    if p.requires_grad:
        assert p.grad is not None, n
        out["grad." + n] = p.grad.detach().float().cpu()
torch.save(out, sys.argv[1])
''' % ROOT


def _run(ride: str, path: str):
    env = dict(os.environ, AIM_WGRAD_RIDE=ride)
    subprocess.run([sys.executable, "-c", CHILD, path], check=True, env=env, timeout=600)
    return torch.load(path, weights_only=True)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def test_riding_changes_only_the_summation_order(tmp_path):
    off = _run("0", str(tmp_path / "off.pt"))
    on = _run("1", str(tmp_path / "on.pt"))
    assert set(off) == set(on)
    assert int(off["ride.launches"]) == 0
    # block 0: D_fc2 on the DACT launch, D_fc1 on the K = 4D + r dgrad -- all 22 064 rows of both
    print(f"rider launches {int(on['ride.launches'])}, rows {int(on['ride.rows'])}")
    assert int(on["ride.launches"]) >= 2 and int(on["ride.rows"]) >= 22064
    ridden = 0
    for k in sorted(off):
        if k.startswith("ride."):
            continue
        assert torch.isfinite(on[k]).all(), k
        if "MLP_Adapter.D_fc" in k:
            e = _rel(on[k], off[k])
            print(f"{k}: relative L2 {e:.3e}")
            assert off[k].norm() > 0, k
            assert e <= 1e-4, (k, e)
            ridden += 1
        else:
            assert torch.equal(on[k], off[k]), k
    assert ridden == 2 * 4          # weight and bias of D_fc1 and D_fc2 in both layers
