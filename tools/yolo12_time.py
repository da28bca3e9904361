"""Build YOLOv12{n,s,...} detection from the seeded synthetic weights (tensorrtx_amd.synth.yolo12_state) and time one execution context:
img/s over --steps enqueues after --warmup.  Usage: python tools/yolo12_time.py --scale n --batch 32 [--size 640] [--fp32]
[--generic-attention].  --generic-attention lowers the same fp16 graph with TRTX_AREA_ATTENTION=0: the eight area-attention blocks run
as shuffles, matmuls and softmax on fp32 linear tensors instead of the MFMA kernel (the A side of DESIGN §5's YOLOv12 table)."""
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--generic-attention", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.generic_attention:
        os.environ["TRTX_AREA_ATTENTION"] = "0"   # read when the plan is lowered (engine creation)
    path = os.path.join(tempfile.gettempdir(), f"yolo12{a.scale}_synth_time.wts")
    wts.write_wts(path, synth.yolo12_state(a.scale))
    plan = engine.build_plan("yolo12" + a.scale, path, batch=a.batch, h=a.size, w=a.size, fp16=0 if a.fp32 else 1)
    kinds = [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]]
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(synth.images(a.batch, a.size, a.size, seed=1)).to(dev)]
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
    print(json.dumps({"model": "yolo12" + a.scale, "batch": a.batch, "size": a.size, "fp16": not a.fp32,
                      "attention": "generic" if kinds.count("attention") == 0 else "mfma", "attention_ops": kinds.count("attention"),
                      "ops": len(kinds), "ms_per_step": round(ms, 4), "img_per_s": round(a.batch * 1000.0 / ms, 1)}))
    e.close()


if __name__ == "__main__":
    main()
