"""Build YOLOv5{n,s,m,l,x}[6] detection from the seeded synthetic weights (tensorrtx_amd.synth.yolov5_state) and time one execution
context: img/s over --steps enqueues after --warmup.  Usage: python tools/yolov5_time.py --scale n --batch 32 [--size 640] [--p6] [--fp32]
[--plugin-head] [--ops].  --plugin-head lowers the same graph with TRTX_YOLO5_HEAD=0: the detect convolutions keep their 255 channels
and the tail is one layout pass per level to fp32 planes followed by the YoloLayer_TRT plugin (the A side of DESIGN §5's YOLOv5 table).
--ops adds the per-op times of one profiled enqueue (trtx_context_profile) for the detect convolutions and the tail."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrtx_amd import engine, synth, wts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", default="n")
    ap.add_argument("--p6", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--plugin-head", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ops", action="store_true")
    a = ap.parse_args()
    if a.plugin_head:
        os.environ["TRTX_YOLO5_HEAD"] = "0"   # read when the plan is lowered (build and engine creation)
    name = "yolov5" + a.scale + ("6" if a.p6 else "")
    path = os.path.join(tempfile.gettempdir(), f"{name}_synth_time.wts")
    wts.write_wts(path, synth.yolov5_state(a.scale, p6=a.p6))
    plan = engine.build_plan(name, path, batch=a.batch, h=a.size, w=a.size, fp16=0 if a.fp32 else 1)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    kinds = [o["kind"] for o in ops]
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(synth.images(a.batch, a.size, a.size, seed=1)).to(dev)]
    for i in range(1, e.nb_bindings):
        bufs.append(torch.empty(a.batch * int(np.prod(e.dims[i])), dtype=torch.float32, device=dev))
    for _ in range(a.warmup):
        e.enqueue(a.batch, bufs)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        e.enqueue(a.batch, bufs)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    out = {"model": name, "batch": a.batch, "size": a.size, "fp16": not a.fp32, "head": "fused" if kinds.count("yolo5_head") else "plugin",
           "to_linear_ops": kinds.count("to_linear"), "ops": len(kinds), "candidates_image0": int(bufs[-1][0].item()),
           "ms_per_step": round(ms, 4), "img_per_s": round(a.batch * 1000.0 / ms, 1)}
    if a.ops:
        out["profile"] = e.profile(a.batch, bufs)
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
