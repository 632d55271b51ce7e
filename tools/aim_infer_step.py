"""Stock-AIM multi-view inference, bf16 beside fp8, for DESIGN.md section 2h and profiles/aim_fp8_inference.json.

    python tools/aim_infer_step.py [--layers 24] [--frames 32] [--views 3] [--rounds 5] [--warmup 2] [--precisions bf16,fp8]
                                   [--root DIR] [--parent-json FILE ...] [--json OUT]

The model is stock AIM (``AIM(wind_attn=False)``) at ViT-L/14 width, 24 layers, 32 frames, 224 x 224: BASELINE configs[4]'s
shape, one sample x 3 views per call (24 672 token rows), pretrained=None with non-zero D_fc2.  A round is one no-grad forward
of the backbone per precision, the precisions interleaved in the same process, each forward between two hipEvents; the figure
is the median over the rounds behind the warm-up rounds, with their min and max.

``--root DIR`` imports the package from another checkout of this repository (an earlier commit, built there), so that the
same script times both trees; a tree without an fp8 path for this model is timed with ``--precisions bf16``.  ``--parent-json``
takes result files of such runs and records their bf16 rounds as ``parent_bf16`` in this run's result (devices differ by ~5 %:
only runs interleaved in one job compare).  Under ``rocprofv3 --kernel-trace --stats -- python tools/aim_infer_step.py --rounds 1
--warmup 1`` the per-kernel table (tools/prof_summary.py) says where each precision's time goes."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(ms):
    s = sorted(ms)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1], rounds_ms=[round(v, 3) for v in ms])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precisions", default="bf16,fp8")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed (default: this one)")
    ap.add_argument("--parent-json", nargs="*", default=[], help="result files of runs on the parent commit's checkout")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import aim_amd
    dev = torch.device("cuda")
    precisions = a.precisions.split(",")
    torch.manual_seed(0)
    m = aim_amd.AIM(224, a.frames, 14, 1024, a.layers, 16, 0.2, adapter_scale=0.5, pretrained=None)
    m.init_weights()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "D_fc2" in n:
                p.normal_(0, 0.02)
    m = m.to(dev).eval()
    views = torch.randn((a.views, 3, a.frames, 224, 224), generator=torch.Generator().manual_seed(1234)).to(dev)
    rows = a.views * a.frames * ((224 // 14) ** 2 + 1)
    times = {p: [] for p in precisions}
    outs = {}
    with torch.no_grad():
        for r in range(a.warmup + a.rounds):
            for p in precisions:
                m.set_inference_precision(p)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                y = m(views)
                e1.record()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[p].append(e0.elapsed_time(e1))
                outs[p] = y
    res = dict(model="AIM (stock) ViT-L/14", layers=a.layers, frames=a.frames, views=a.views, rows=rows, warmup=a.warmup,
               root=os.path.relpath(os.path.abspath(a.root), HERE))
    for p in precisions:
        res[p] = dict(_stats(times[p]), views_per_s=a.views * 1e3 / _stats(times[p])["median_ms"])
    if "bf16" in outs and "fp8" in outs:
        d = (outs["fp8"].double() - outs["bf16"].double()).norm() / outs["bf16"].double().norm()
        res["fp8_vs_bf16_rel"] = float(d)
    parent = []
    for f in a.parent_json:
        with open(f) as fh:
            parent += json.loads(fh.readline())["bf16"]["rounds_ms"]
    if parent:
        res["parent_bf16"] = dict(_stats(parent), views_per_s=a.views * 1e3 / _stats(parent)["median_ms"])
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:                                     # (profiles/aim_fp8_inference.json is such a line)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
