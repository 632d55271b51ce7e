"""SwinTransformer3D on the MI355X against the reference's own outputs and gradients (tests/golden/swin3d_tiny_{a,b,c,d}.npz),
the requires_grad contract, bitwise repeatability and three optimizer steps of the k400 base recipe.  Every GPU run is a child
process of tests/swin3d_runs.py under its own timeout; they run one after the other and the parent stops at the first that
fails.

The bound, 2.5e-2 rel-L2 on the output and on every gradient, is the bf16 bound the other full-parameter backbones are held to
(tests/test_swin2d_adapter_gpu.py), at the same rounding points: bf16 GEMM operands and P, fp32 accumulation, LayerNorm and
residual stream.  The fixtures' seeds are chosen by the reference alone (golden/make_golden_swin3d.py): their ``bf16_floor`` is
between 0.88e-2 and 1.21e-2.

Measured on an MI355X (worst rel-L2 over the output and every gradient figure of a case; the output alone):
    a  1.43e-2 (96 figures; output 6.15e-3)     b  1.38e-2 (98; 4.78e-3)     c  1.37e-2 (96; 5.66e-3)     d  1.16e-2 (51; 5.54e-3)
The worst figure of a is on layers.0.blocks.0.norm2.bias, the tensor its bf16_floor is on; those of b, c and d are on a
relative_position_bias_table gradient."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 2.5e-2
RUNS = ("fixture:a", "fixture:b", "fixture:c", "fixture:d", "bitwise", "recipe")
TIMEOUT = 150


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("swin3d")
    out = {}
    for what in RUNS:
        path = str(tmp / (what.replace(":", "_") + ".json"))
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "swin3d_runs.py"), what, path], capture_output=True, text=True,
                               timeout=TIMEOUT)
        except subprocess.TimeoutExpired:
            out[what] = f"{what}: no result within {TIMEOUT} s"
            break
        if r.returncode != 0:
            out[what] = f"{what}: exit status {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
            break                                   # nothing more is started on the GPU after a failed child
        with open(path) as f:
            out[what] = json.load(f)
    return out


def _rec(records, what):
    assert what in records, f"{what} was not run: an earlier run failed: {[v for v in records.values() if isinstance(v, str)]}"
    assert not isinstance(records[what], str), records[what]
    return records[what]


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_bf16_against_reference_fixture(records, tag):
    rec = _rec(records, f"fixture:{tag}")
    worst = max(rec["errs"].items(), key=lambda kv: kv[1])
    print(f"case {tag}: worst rel-L2 {worst[1]:.3e} ({worst[0]}) over {len(rec['errs'])} figures; y {rec['errs'].get('y', rec['errs'].get('y|norm')):.3e}")
    assert rec["finite"]
    assert worst[1] <= BOUND, sorted(rec["errs"].items(), key=lambda kv: -kv[1])[:8]
    assert all(rec["zeros"].values()), [k for k, v in rec["zeros"].items() if not v]     # exactly 0 in the reference: exactly 0
    assert rec["none"] == rec["frozen"]


def test_frozen_stage_gets_none_and_the_rest_keep_their_bits(records):
    rec = _rec(records, "fixture:d")
    assert rec["frozen"] and all(n.startswith(("patch_embed.", "layers.0.")) for n in rec["frozen"])
    assert rec["none"] == rec["frozen"]
    assert rec["full_has_all"] and rec["frozen_none_rest_same_bits"]


def test_no_grad_forward_and_second_backward_give_the_same_bits(records):
    rec = _rec(records, "bitwise")
    assert rec["tensors"] > 50
    assert rec["no_grad_forward_same_bits"] and rec["second_forward_same_bits"] and rec["second_backward_same_bits"]


def test_three_recipe_steps_finite_exact_trainable_set_and_reproducible(records):
    rec = _rec(records, "recipe")
    print("losses", rec["losses"])
    assert rec["optimizer"] == "FlatAdamW"
    assert rec["finite"] and rec["params_finite"]
    assert rec["trainable"] > 100 and rec["unchanged_trainable"] == [] and rec["changed_frozen"] == []
    assert rec["same_bits"]
