"""Build YOLO11{n,s,...} from the seeded synthetic weights (tensorrtx_amd.synth.yolo11_state) and time one execution context:
img/s over --steps enqueues after --warmup.  Usage: python tools/yolo11_time.py --scale n --batch 32 [--size 640] [--fp32]
[--task det|seg|pose|obb|cls] [--mark-heads].  Without --size the task's reference input size is used (yolo11/include/config.h:
kInputH 640, kObbInputH 1024, kClsInputH 224).  --mark-heads times the debugging plan whose heads are outputs, i.e. the generic tail
and the YoloLayer_TRT plugin instead of the fused head (the A side of DESIGN §5's tail profile)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrtx_amd import engine, synth, wts  # noqa: E402

TASKS = {"det": (0, 80, 640), "seg": (1, 80, 640), "pose": (2, 1, 640), "obb": (3, 15, 1024), "cls": (4, 1000, 224)}   # id, classes, size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", default="n")
    ap.add_argument("--task", default="det", choices=sorted(TASKS))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--mark-heads", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    tid, nc, size = TASKS[a.task]
    size = a.size or size
    path = os.path.join(tempfile.gettempdir(), f"yolo11{a.scale}_{a.task}_synth_time.wts")
    wts.write_wts(path, synth.yolo11_state(a.scale, num_class=nc, task=tid))
    plan = engine.build_plan("yolo11" + a.scale, path, batch=a.batch, h=size, w=size, fp16=0 if a.fp32 else 1, task=tid,
                             mark_heads=int(a.mark_heads))
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(synth.images(a.batch, size, size, seed=1)).to(dev)]
    for i in range(1, e.nb_bindings):
        bufs.append(torch.empty(int(np.prod(e.dims[i])), dtype=torch.float32, device=dev))
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
    line = {"model": "yolo11" + a.scale, "batch": a.batch, "size": size, "fp16": not a.fp32, "ms_per_step": round(ms, 4),
            "img_per_s": round(a.batch * 1000.0 / ms, 1)}
    if a.task != "det":   # the det line keeps its earlier keys
        line["task"] = a.task
    if a.mark_heads:
        line["mark_heads"] = True
    print(json.dumps(line))
    e.close()


if __name__ == "__main__":
    main()
