"""Time YOLOv13's AAttn interior (yolov13/src/block.cpp:303-423: the qk and v 1x1 convolutions, the 5x5 depthwise `pe`, the area attention, `proj`) at the
widths and maps of model.6 (area 4, the 40 x 40 map) and model.8 (area 1, 20 x 20) of a yolov13n / yolov13l, fp16, 640 x 640, batch 32, one execution
context: the `attention_split` op against the generic lowering of the same graph (TRTX_AATTN_SPLIT=0, read when the engine is created), in alternating
pairs; the median of five per side, every run and the spread go to profiles/aattn_split_time.jsonl.  Then the kernel alone, through the C ABI, against
area_attention_f16 on the same values packed as YOLOv12 has them (that one also writes the V image).

  python tools/aattn_split_time.py

The convolutions and the layout passes of the bindings are in both sides' times; the difference is the attention's.  Seeded synthetic weights
(tests/aattn_split_cases.py)."""
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
from tensorrtx_amd import capi, engine  # noqa: E402
from tests import aattn_split_cases as sc  # noqa: E402

# (name, C = A2C2f's inner width 0.5 * c2, stride, area): heads = C / 32 (block.cpp:447-449; yolov13/src/model.cpp:80-87)
BLOCKS = [("n_model6", 64, 16, 4), ("n_model8", 128, 32, 1), ("l_model6", 256, 16, 4), ("l_model8", 256, 32, 1)]


def run(B, C, H, W, area, steps, warmup, generic):
    if generic:
        os.environ["TRTX_AATTN_SPLIT"] = "0"
    else:
        os.environ.pop("TRTX_AATTN_SPLIT", None)
    plan, _, _ = sc.aattn13_net(B, C // 32, H, W, area, tail="proj", cin=C, seed=C)
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert (kinds["attention_split"] == 0) == generic, kinds
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


def kernel_alone(B, C, N, area, steps, warmup, pairs):
    """ms per launch of (area_attention_split_f16, area_attention_f16) on equal values, alternating; the two O must be bit-equal"""
    heads, dev = C // 32, torch.device("cuda:0")
    g = torch.Generator().manual_seed(C + N)
    qkv = torch.randn((B, N, heads, 96), generator=g).half()
    flat = lambda t: t.reshape(B, N, -1)   # noqa: E731
    qk = torch.cat([flat(qkv[..., :32]), flat(qkv[..., 32:64])], -1).contiguous().to(dev)
    v = flat(qkv[..., 64:]).contiguous().to(dev)
    qkv = flat(qkv).contiguous().to(dev)
    o_split, o_packed, vimg = (torch.empty((B, N, C), dtype=torch.float16, device=dev) for _ in range(3))
    launch = {"split": lambda: capi.area_attention_split(qk[..., :C], qk[..., C:], v, heads, area, sc.SCALE, out=o_split),
              "packed": lambda: capi.area_attention(qkv, heads, area, sc.SCALE, out=o_packed, vimg=vimg)}
    ms = {"split": [], "packed": []}
    for _ in range(pairs):
        for side in ("split", "packed"):
            for _ in range(warmup):
                launch[side]()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                launch[side]()
            t1.record()
            torch.cuda.synchronize()
            ms[side].append(t0.elapsed_time(t1) / steps)
    assert torch.equal(o_split, o_packed)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aattn_split_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    os.environ.setdefault("TRTX_TUNE", "0")   # the static default kernel of every convolution on both sides: the pairs differ by the attention alone
    for name, C, stride, area in BLOCKS:
        H = W = a.size // stride
        fused, generic, ops = [], [], {}
        for _ in range(a.pairs):
            ms, ops["fused"] = run(a.batch, C, H, W, area, a.steps, a.warmup, False)
            fused.append(ms)
            ms, ops["generic"] = run(a.batch, C, H, W, area, a.steps, a.warmup, True)
            generic.append(ms)
        diffs = [g - f for f, g in zip(fused, generic)]
        alone = kernel_alone(a.batch, C, H * W, area, a.steps, a.warmup, a.pairs)
        rec = {"block": name, "C": C, "heads": C // 32, "H": H, "W": W, "area": area, "batch": a.batch, "fp16": True, "pairs": a.pairs,
               "fused_ms": round(statistics.median(fused), 4), "generic_ms": round(statistics.median(generic), 4),
               "fused_ms_all": [round(v, 4) for v in fused], "generic_ms_all": [round(v, 4) for v in generic],
               "saved_ms_per_pair": [round(v, 4) for v in diffs], "pair_spread_ms": round(max(diffs) - min(diffs), 4),
               "kernel_split_ms": round(statistics.median(alone["split"]), 4), "kernel_packed_ms": round(statistics.median(alone["packed"]), 4),
               "kernel_split_ms_all": [round(v, 4) for v in alone["split"]], "kernel_packed_ms_all": [round(v, 4) for v in alone["packed"]], "ops": ops}
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
