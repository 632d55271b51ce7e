"""SwinTransformer2D_Adapter on the MI355X against the reference's own outputs and gradients
(tests/golden/swin2d_adapter_tiny_{a,b,c,d}.npz), the requires_grad contract, bitwise repeatability and three optimizer steps
of the k400 recipe.  Every GPU run is a child process of tests/swin2d_adapter_runs.py under its own timeout; they run one after
the other and the parent stops at the first that fails.

The bound, 2.5e-2 rel-L2 on the output and on every gradient, is the bf16 bound tests/test_vit_imagenet_gpu.py and
tests/test_timesformer_gpu.py hold the other full-parameter backbones to, at the same rounding points: bf16 GEMM operands and P,
fp32 accumulation, LayerNorm and residual stream.

Measured on an MI355X (worst rel-L2 over the output and every gradient figure of a case; the output alone):
    a  2.36e-2 (314 figures; output 7.76e-3)     b  1.76e-2 (162; 7.78e-3)     c  2.29e-2 (142; 8.92e-3)     d  1.48e-2 (88; 7.81e-3)
The fixtures' seeds are chosen by the reference alone (golden/make_golden_swin2d_adapter.py): a case is refused where the
reference itself, with nothing but the operands of its nn.Linear products rounded to bf16, is more than this bound away from its
fp32 gradients on some tensor (``bf16_floor``; a bias-table gradient is a sum of signed terms over thousands of sequences and
where that sum cancels, bf16 alone costs up to 1.4e-1 on it)."""
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
    tmp = tmp_path_factory.mktemp("swin2d_adapter")
    out = {}
    for what in RUNS:
        path = str(tmp / (what.replace(":", "_") + ".json"))
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "swin2d_adapter_runs.py"), what, path], capture_output=True, text=True,
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


def test_one_key_temporal_softmax_has_exactly_zero_bias_gradient(records):
    rec = _rec(records, "fixture:c")
    keys = [k for k in rec["zeros"] if k.endswith("temporal_position_bias_table")]
    assert len(keys) == 3 and all(rec["zeros"][k] for k in keys)      # the even blocks of depths [1, 3]


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
    assert rec["trainable"] > 200 and rec["unchanged_trainable"] == [] and rec["changed_frozen"] == []
    assert rec["same_bits"]
