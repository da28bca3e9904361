"""Build YOLOv9 / GELAN engines from the seeded synthetic weights (tensorrtx_amd.synth.yolov9_state) and time them through one execution
context.  Usage: python tools/yolov9_time.py [--models yolov9t,yolov9c] [--batch 32] [--size 640] [--steps 40] [--warmup 10] [--pairs 5]
[--out profiles/yolov9_time.jsonl].  Per model, one JSON line each for:
  * "time": img/s of the fused-head fp16 engine over --steps enqueues after --warmup, repeated --pairs times (median, min, max);
  * "head_ab": the fused head against TRTX_YOLO9_HEAD=0 (layout passes, the DFL chain, the YoloLayer_TRT plugin), two engines of the same
    build alive at once and timed in alternating pairs in this one process;
  * "ops" (the last model only): the per-op times of one profiled enqueue (trtx_context_profile) summed by kind, with the shares of the
    pools (ADown / AConv's avg-pool and max-pool, SPPELAN's chain) and of the convolutions left on the direct kernel.
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


def make(name, path, a, plugin_head):
    """(plan ops, engine, buffers); TRTX_YOLO9_HEAD is read when the plan is lowered: at build and at engine creation"""
    if plugin_head:
        os.environ["TRTX_YOLO9_HEAD"] = "0"
    try:
        # max_out above the cell count: the synthetic weights keep more candidates than a trained model, and a full buffer would hide writes
        cells = sum((a.size // s) ** 2 for s in (8, 16, 32))
        plan = engine.build_plan(name, path, batch=a.batch, h=a.size, w=a.size, fp16=1, max_out=cells + 16)
        ops = engine.describe_plan(plan, lowered=True)["ops"]
        e = engine.Engine(plan)
    finally:
        os.environ.pop("TRTX_YOLO9_HEAD", None)
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(synth.images(a.batch, a.size, a.size, seed=1)).to(dev)]
    for i in range(1, e.nb_bindings):
        bufs.append(torch.empty(a.batch * int(np.prod(e.dims[i])), dtype=torch.float32, device=dev))
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
    ap.add_argument("--models", default="yolov9t,yolov9c")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "yolov9_time.jsonl"))
    a = ap.parse_args()
    lines = []
    models = a.models.split(",")
    for name in models:
        path = os.path.join(tempfile.gettempdir(), f"{name}_synth_time.wts")
        wts.write_wts(path, synth.yolov9_state(name))
        ops, e, bufs = make(name, path, a, False)
        rops, r, rbufs = make(name, path, a, True)
        kinds, rkinds = [o["kind"] for o in ops], [o["kind"] for o in rops]
        assert kinds.count("yolo9_head") == 1 and rkinds.count("plugin") == 1
        for _ in range(a.warmup):
            e.enqueue(a.batch, bufs)
            r.enqueue(a.batch, rbufs)
        torch.cuda.synchronize()
        fused, route = [], []
        for _ in range(a.pairs):   # alternating pairs: both engines see the same machine state
            fused.append(timed(e, bufs, a.batch, a.steps))
            route.append(timed(r, rbufs, a.batch, a.steps))
        out = bufs[e.names.index("output")].reshape(a.batch, -1)
        base = {"model": name, "batch": a.batch, "size": a.size, "fp16": True, "steps": a.steps, "pairs": a.pairs}
        f, p = spread(fused), spread(route)
        lines.append(dict(base, what="time", head="fused", ops=len(kinds), ms_per_step=f, img_per_s=round(a.batch * 1000.0 / f["median"], 1),
                          candidates_image0=int(out[0, 0].item()), max_out=(out.shape[1] - 1) // 38))
        lines.append(dict(base, what="head_ab", fused_ms=f, plugin_route_ms=p, fused_ops=len(kinds), plugin_route_ops=len(rkinds),
                          plugin_route_to_linear=rkinds.count("to_linear"), gain_ms_median=round(p["median"] - f["median"], 4),
                          pair_gain_ms=[round(y - x, 4) for x, y in zip(fused, route)]))
        if name == models[-1]:
            prof = e.profile(a.batch, bufs)
            by = collections.Counter()
            total = sum(x["ms"] for x in prof)
            direct = 0.0
            if len(prof) == len(ops):
                for x, o in zip(prof, ops):
                    if o["kind"] == "conv" and not (o["igemm"] or o["stem"] or o.get("dw") or o.get("grouped")):
                        direct += x["ms"]
            for x in prof:
                by[x["kind"]] += x["ms"]
            pools = by.get("pool", 0.0) + by.get("pool_chain", 0.0)
            lines.append(dict(base, what="ops", profiled_ms=round(total, 4), ms_by_kind={k: round(v, 4) for k, v in sorted(by.items(), key=lambda kv: -kv[1])},
                              count_by_kind=dict(collections.Counter(kinds)), pool_share=round(pools / total, 4), direct_conv_share=round(direct / total, 4),
                              head_ms=round(by.get("yolo9_head", 0.0), 4)))
        e.close()
        r.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        for ln in lines:
            print(json.dumps(ln))
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
