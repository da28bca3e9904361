"""Time YOLOv13's FullPad_Tunnel (yolov13/src/block.cpp:889-900: a + gate * b, a learned scalar) and the gamma residual of A2C2f (block.cpp:473-484: a
per-channel gate) between two 1x1 convolutions at the three pyramid levels of a yolov13n / yolov13l, fp16, 640 x 640, batch 32, one execution
context: the `gated_add` op against the generic lowering of the same graph (TRTX_GATED_ADD=0, read when the engine is created), in alternating
pairs; the median of five per side, every run and the spread go to profiles/gated_add_time.jsonl.

  python tools/gated_add_time.py

The graph: x -> 1x1 conv -> a; x -> 1x1 conv -> b; a + gate * b -> 1x1 conv to 8 channels -> output.  The convolutions and the layout passes of the
bindings are in both sides' times; the difference is the fold's.  Seeded synthetic weights."""
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
from tensorrtx_amd import builder, engine  # noqa: E402

# (name, channels, stride): the three maps FullPad_Tunnel runs on (yolov13/src/model.cpp), n and l widths
LEVELS = [("n_p3", 64, 8), ("n_p4", 128, 16), ("n_p5", 256, 32), ("l_p3", 256, 8), ("l_p4", 512, 16), ("l_p5", 512, 32)]


def build(B, C, H, W, per_channel):
    rng = np.random.default_rng(C)
    w = lambda co, ci: (rng.standard_normal((co, ci, 1, 1)) / np.sqrt(ci)).astype(np.float32)   # noqa: E731
    net = builder.Network(fp16=True, explicit_batch=True)
    try:
        x = net.input("x", (B, C, H, W))
        a, b = net.out(net.conv(x, w(C, C))), net.out(net.conv(x, w(C, C)))
        gate = rng.uniform(0.2, 0.8, C).astype(np.float32).reshape(1, C, 1, 1) if per_channel else np.full((1, 1, 1, 1), 0.37, np.float32)
        p = net.out(net.elementwise(net.out(net.constant(gate)), b, "prod") if per_channel else net.elementwise(b, net.out(net.constant(gate)), "prod"))
        y = net.out(net.elementwise(a, p, "sum"))
        net.mark_output(net.out(net.conv(y, w(8, C))), "y")
        return net.build()
    finally:
        net.close()


def run(B, C, H, W, per_channel, steps, warmup, generic):
    if generic:
        os.environ["TRTX_GATED_ADD"] = "0"
    else:
        os.environ.pop("TRTX_GATED_ADD", None)
    plan = build(B, C, H, W, per_channel)
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert (kinds["gated_add"] == 0) == generic, kinds
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    bufs = []
    for i in range(e.nb_bindings):
        n = int(np.prod(e.dims[i]))
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gated_add_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    os.environ.setdefault("TRTX_TUNE", "0")   # the static default kernel of every convolution on both sides: the pairs differ by the fold alone
    for name, C, stride in LEVELS:
        for per_channel in (False, True):
            H = W = a.size // stride
            fused, generic, ops = [], [], {}
            for _ in range(a.pairs):
                ms, ops["fused"] = run(a.batch, C, H, W, per_channel, a.steps, a.warmup, False)
                fused.append(ms)
                ms, ops["generic"] = run(a.batch, C, H, W, per_channel, a.steps, a.warmup, True)
                generic.append(ms)
            diffs = [g - f for f, g in zip(fused, generic)]
            rec = {"block": "gamma residual" if per_channel else "FullPad_Tunnel", "level": name, "C": C, "H": H, "W": W, "batch": a.batch, "fp16": True,
                   "pairs": a.pairs, "fused_ms": round(statistics.median(fused), 4), "generic_ms": round(statistics.median(generic), 4),
                   "fused_ms_all": [round(v, 4) for v in fused], "generic_ms_all": [round(v, 4) for v in generic],
                   "saved_ms_per_pair": [round(v, 4) for v in diffs], "pair_spread_ms": round(max(diffs) - min(diffs), 4),
                   "gated_add_bytes": 3 * 2 * a.batch * C * H * W, "ops": ops}
            print(json.dumps(rec))
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
