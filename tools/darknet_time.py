"""Build Darknet YOLO engines (YOLOv3-tiny, YOLOv3, YOLOv4) from the seeded synthetic weights (tensorrtx_amd.synth.darknet_state) and time them
through one execution context, fp16.
Usage: python tools/darknet_time.py [--runs yolov3-tiny:32:416,yolov3:8:608,yolov4:8:608] [--steps 20] [--warmup 5] [--pairs 5]
[--out profiles/darknet_time.jsonl].  A run is model:batch:size.
Per run, one JSON line each for:
  * "head_ab": the fused head against TRTX_DARKNET_HEAD=0 (one layout pass per level and the 7-float YoloLayer_TRT plugin), two engines of the
    same build alive at once and timed in alternating pairs in this one process: median and range of the pairs, the per-pair gains, and the
    run-to-run spread of one engine (the range of the fused engine's own runs).  A difference counts only beyond that spread;
  * "ops": the per-op times of one profiled enqueue (trtx_context_profile) summed by kind, with the shares of the first convolution (the
    stride-1 stem at full resolution), of the pools, the pad, the SPP pool chain, the upsamples and the head - the largest shares that are
    no convolution are what to look at next.
Lines are printed and appended to --out."""
import argparse
import collections
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrtx_amd import engine, synth, wts  # noqa: E402


def make(name, path, batch, size, switch=None):
    """(plan ops, engine, buffers); the switch is read when the plan is lowered: at build and at engine creation"""
    if switch:
        os.environ[switch] = "0"
    try:
        plan = engine.build_plan(name, path, batch=batch, h=size, w=size, fp16=1)
        ops = engine.describe_plan(plan, lowered=True)["ops"]
        e = engine.Engine(plan)
    finally:
        if switch:
            os.environ.pop(switch, None)
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(synth.images(batch, size, size, seed=1)).to(dev)]
    for i in range(1, e.nb_bindings):
        bufs.append(torch.empty(batch * int(np.prod(e.dims[i])), dtype=torch.float32, device=dev))
    return ops, e, bufs


def timed(e, bufs, batch, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        e.enqueue(batch, bufs)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "runs": [round(v, 4) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="yolov3-tiny:32:416,yolov3:8:608,yolov4:8:608")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "darknet_time.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)

    def emit(ln):
        print(json.dumps(ln), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(ln) + "\n")

    for spec in a.runs.split(","):
        name, batch, size = spec.split(":")
        batch, size = int(batch), int(size)
        path = os.path.join(tempfile.gettempdir(), f"{name}_synth_time.wts")
        wts.write_wts(path, synth.darknet_state(name))
        base = {"model": name, "batch": batch, "size": size, "fp16": True, "steps": a.steps, "pairs": a.pairs}
        ops, e, bufs = make(name, path, batch, size)
        kinds = [o["kind"] for o in ops]
        assert kinds.count("darknet_head") == 1 and "plugin" not in kinds and "to_linear" not in kinds
        rops, r, rbufs = make(name, path, batch, size, "TRTX_DARKNET_HEAD")
        rkinds = [o["kind"] for o in rops]
        assert rkinds.count("plugin") == 1 and rkinds.count("darknet_head") == 0
        for _ in range(a.warmup):
            e.enqueue(batch, bufs)
            r.enqueue(batch, rbufs)
        torch.cuda.synchronize()
        on, off = [], []
        for _ in range(a.pairs):   # alternating pairs: both engines see the same machine state
            on.append(timed(e, bufs, batch, a.steps))
            off.append(timed(r, rbufs, batch, a.steps))
        r.close()
        f, p = spread(on), spread(off)
        out = bufs[e.names.index("prob")].reshape(batch, -1)
        anchors = 3 * sum((size // s) ** 2 for s in synth.DARKNET_STRIDES[name])
        emit(dict(base, what="head_ab", fused_ms=f, plugin_route_ms=p, img_per_s=round(batch * 1000.0 / f["median"], 1), fused_ops=len(kinds),
                  plugin_route_ops=len(rkinds), plugin_route_to_linear=rkinds.count("to_linear"), gain_ms_median=round(p["median"] - f["median"], 4),
                  pair_gain_ms=[round(y - x, 4) for x, y in zip(on, off)], one_engine_spread_ms=round(f["max"] - f["min"], 4),
                  candidates_image0=int(out[0, 0].item()), anchors=anchors, max_out=(out.shape[1] - 1) // 7))
        prof = e.profile(batch, bufs)
        by = collections.Counter()
        total = sum(x["ms"] for x in prof)
        for x in prof:
            by[x["kind"]] += x["ms"]
        extra = {}
        if len(prof) == len(ops):
            extra["first_conv_ms"] = round(prof[0]["ms"], 4)   # the stride-1 3x3 stem at full resolution (Mish in yolov4)
            extra["first_conv_share"] = round(prof[0]["ms"] / total, 4)
        not_conv = {k: v for k, v in by.items() if k not in ("conv", "conv_group")}
        emit(dict(base, what="ops", profiled_ms=round(total, 4), ms_by_kind={k: round(v, 4) for k, v in sorted(by.items(), key=lambda kv: -kv[1])},
                  count_by_kind=dict(collections.Counter(kinds)), share_by_kind_not_conv={k: round(v / total, 4) for k, v in sorted(not_conv.items(), key=lambda kv: -kv[1])},
                  head_ms=round(by.get("darknet_head", 0.0), 4), **extra))
        e.close()


if __name__ == "__main__":
    main()
