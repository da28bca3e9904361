"""Time YOLOv9's downsamplers as "pool_conv" ops (kernels/conv_pool.hip: the average pool, and ADown's max-pool, inside the convolution's launch) against the same
engine lowered with TRTX_POOL_CONV=0 (pool ops in front of the convolutions; TRTX_POOL_CONV=2 on the fused side, so that shapes the lowering declines are timed too): yolov9c (ADown) and yolov9t (AConv), synthetic weights, fp16, 640 x 640, batch 32, one
execution context.  Both engines of a model live in one process and are timed in alternating windows, five pairs; then one profiled enqueue of each gives the per-op
rows of the downsamplers.  Every window, both medians, both spreads and the rows go to profiles/pool_conv_time.jsonl.

  python tools/pool_conv_time.py

The switch is read when the plan is lowered at engine creation; the tactic timing of the other convolutions runs on both sides as it does for a user."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tensorrtx_amd import engine  # noqa: E402
from test_yolov9_cpu import yolov9_wts  # noqa: E402


def make(plan, B, switch):
    os.environ["TRTX_POOL_CONV"] = switch
    e = engine.Engine(plan)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    dev = torch.device("cuda:0")
    bufs = [torch.randn(B * int(np.prod(e.dims[i])), dtype=torch.float32, device=dev) if e.is_input[i] else
            torch.empty(B * int(np.prod(e.dims[i])), dtype=torch.float32, device=dev) for i in range(e.nb_bindings)]
    return e, bufs, ops


def window(e, bufs, B, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        e.enqueue(B, bufs)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def rows(e, bufs, B, ops):
    """the downsamplers' ops of one profiled enqueue: pool_conv ops, pool ops, and the convolutions a pool_conv op of the other side stands for"""
    prof = e.profile(B, bufs)
    prof = prof["ops"] if isinstance(prof, dict) else prof
    assert len(prof) == len(ops)
    total = sum(x["ms"] for x in prof)
    by = collections.Counter()
    for x in prof:
        by[x["kind"]] += x["ms"]
    keep = [dict(kind=o["kind"], name=o["name"], ms=round(x["ms"], 4), **{k: o[k] for k in ("mode", "cin", "cout", "hw_in", "k") if k in o})
            for x, o in zip(prof, ops) if o["kind"] in ("pool_conv", "pool") or (o["kind"] == "conv" and o["stride"] == [2, 2] and o["cin"] > 4)]
    return dict(profiled_ms=round(total, 4), by_kind={k: round(v, 4) for k, v in sorted(by.items())}, rows=keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--models", default="yolov9c,yolov9t")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_conv_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    for model in a.models.split(","):
        plan = engine.build_plan(model, yolov9_wts(model)[0], batch=a.batch, h=a.size, w=a.size, fp16=1)
        sides = {"fused": make(plan, a.batch, "2"), "pools": make(plan, a.batch, "0")}   # 2: also where the lowering declines the one launch
        os.environ.pop("TRTX_POOL_CONV")
        kinds = {s: collections.Counter(o["kind"] for o in v[2]) for s, v in sides.items()}
        assert kinds["fused"]["pool_conv"] > 0 and kinds["pools"]["pool_conv"] == 0, kinds
        ms = {s: [] for s in sides}
        for s, (e, bufs, _) in sides.items():
            window(e, bufs, a.batch, a.warmup)
        for _ in range(a.pairs):
            for s, (e, bufs, _) in sides.items():
                ms[s].append(window(e, bufs, a.batch, a.steps))
        spread = max(max(v) - min(v) for v in ms.values())
        saved = statistics.median(ms["pools"]) - statistics.median(ms["fused"])
        rec = {"model": model, "batch": a.batch, "size": a.size, "fp16": True, "pairs": a.pairs, "steps": a.steps, "fused_ms": round(statistics.median(ms["fused"]), 4),
               "pools_ms": round(statistics.median(ms["pools"]), 4), "fused_ms_all": [round(v, 4) for v in ms["fused"]], "pools_ms_all": [round(v, 4) for v in ms["pools"]],
               "saved_ms": round(saved, 4), "larger_spread_ms": round(spread, 4), "fused_wins_every_pair": all(p - f > spread for f, p in zip(ms["fused"], ms["pools"])),
               "ops": {s: dict(k) for s, k in kinds.items()}, "profile": {s: rows(e, bufs, a.batch, ops) for s, (e, bufs, ops) in sides.items()}}
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        for e, _, _ in sides.values():
            e.close()


if __name__ == "__main__":
    main()
