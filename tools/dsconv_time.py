"""Time YOLOv13's DSConv (yolov13/src/block.cpp:491-586) as the one fused launch of kernels/conv_dw_pw.hip against the two launches of the same plan
lowered with TRTX_DSCONV=0 (conv_dw, then the 1x1; TRTX_DSCONV=2 on the fused side, so that the widths the lowering declines are timed too - the switch is
read when the plan is built and when the engine is created): DSBottleneck networks
(tests/dsconv_cases.py) at three shapes a yolov13n and one a yolov13x reaches, fp16, 640 x 640, batch 32, one execution context, same process, alternating
pairs; the median of each side, every run and both spreads go to profiles/dsconv_time.jsonl.

  python tools/dsconv_time.py

The layout passes of the bindings (fp32 NCHW <-> fp16 NHWC) are in both sides' times; the difference is the DSConvs'."""
import argparse
import collections
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tensorrtx_amd import engine  # noqa: E402
from tests import dsconv_cases as dc  # noqa: E402

# (name, dsbottleneck_net's arguments but the batch; stride = the map's stride in the 640 x 640 model)
NETS = [("n_16ch_160_k3_k7", 4, dict(C=16, k1=3, k2=7, shortcut=True, stride=1)), ("n_64ch_80_k3_k7", 8, dict(C=64, k1=3, k2=7, shortcut=True, stride=1)),
        ("n_128_to_128_s2_80", 8, dict(C=128, k1=3, k2=3, shortcut=False, stride=2, single=True)),
        ("x_768_to_768_s2_40", 16, dict(C=768, k1=3, k2=3, shortcut=False, stride=2, single=True))]


def run(B, kw, steps, warmup, two):
    if two:
        os.environ["TRTX_DSCONV"] = "0"
    else:
        os.environ["TRTX_DSCONV"] = "2"   # the one launch at every width, also where the lowering would decline it
    plan, layers = dc.dsbottleneck_net(B, **kw)
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert kinds["dsconv"] == (0 if two else len(layers)) and kinds["conv"] == (2 * len(layers) if two else 0), kinds
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    bufs = []
    for i in range(e.nb_bindings):
        n = B * int(np.prod(e.dims[i]))
        bufs.append(torch.randn(n, dtype=torch.float32, device=dev) if e.is_input[i] else torch.empty(n, dtype=torch.float32, device=dev))
    for _ in range(warmup):
        e.enqueue(B, bufs)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        e.enqueue(B, bufs)
    t1.record()
    torch.cuda.synchronize()
    e.close()
    return t0.elapsed_time(t1) / steps, dict(kinds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsconv_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    os.environ.setdefault("TRTX_TUNE", "0")   # the static default kernel of the 1x1 on the two-launch side
    for name, stride, kw in NETS:
        kw = dict(kw, H=a.size // stride, W=a.size // stride)
        fused, two, ops = [], [], {}
        for _ in range(a.pairs):
            ms, ops["fused"] = run(a.batch, kw, a.steps, a.warmup, False)
            fused.append(ms)
            ms, ops["two"] = run(a.batch, kw, a.steps, a.warmup, True)
            two.append(ms)
        spread = max(max(fused) - min(fused), max(two) - min(two))
        saved = statistics.median(two) - statistics.median(fused)
        rec = {"net": name, **kw, "batch": a.batch, "fp16": True, "pairs": a.pairs, "fused_ms": round(statistics.median(fused), 4),
               "two_launch_ms": round(statistics.median(two), 4), "fused_ms_all": [round(v, 4) for v in fused], "two_launch_ms_all": [round(v, 4) for v in two],
               "saved_ms": round(saved, 4), "larger_spread_ms": round(spread, 4), "fused_wins": bool(saved > spread), "ops": ops}
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
