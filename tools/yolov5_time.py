"""Build YOLOv5{n,s,m,l,x}[6] from the seeded synthetic weights (tensorrtx_amd.synth.yolov5_state) and time one execution context:
img/s over --steps enqueues after --warmup.  Usage: python tools/yolov5_time.py --scale n --batch 32 [--task 0|1|4] [--size 640] [--p6]
[--fp32] [--plugin-head] [--ops] [--masks].  --task: 0 det, 1 seg, 4 cls (--size defaults to 224 for cls).  --plugin-head lowers the
det graph with TRTX_YOLO5_HEAD=0: the detect convolutions keep their 255 channels and the tail is one layout pass per level to fp32
planes followed by the YoloLayer_TRT plugin (the A side of DESIGN §5's YOLOv5 table).  --ops adds the per-op times of one profiled
enqueue (trtx_context_profile).  --masks (seg): a step is engine + trtx_yolov5_nms + trtx_seg_masks on the engine's device buffers
(--conf / --max-keep), and the result line carries the kept counts, the rect areas and the bytes trtx_seg_masks must move."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrtx_amd import capi, engine, synth, wts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", default="n")
    ap.add_argument("--p6", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--task", type=int, default=0, choices=[0, 1, 4])
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--masks", action="store_true")
    ap.add_argument("--conf", type=float, default=0.4)
    ap.add_argument("--max-keep", type=int, default=64)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--plugin-head", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ops", action="store_true")
    a = ap.parse_args()
    if a.size is None:
        a.size = 224 if a.task == 4 else 640
    assert not a.masks or a.task == 1, "--masks needs --task 1"
    if a.plugin_head:
        os.environ["TRTX_YOLO5_HEAD"] = "0"   # read when the plan is lowered (build and engine creation)
    name = "yolov5" + a.scale + ("6" if a.p6 else "")
    path = os.path.join(tempfile.gettempdir(), f"{name}_task{a.task}_synth_time.wts")
    wts.write_wts(path, synth.yolov5_state(a.scale, p6=a.p6, task=a.task, num_class=1000 if a.task == 4 else 80))
    plan = engine.build_plan(name, path, batch=a.batch, h=a.size, w=a.size, fp16=0 if a.fp32 else 1, task=a.task)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    kinds = [o["kind"] for o in ops]
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(synth.images(a.batch, a.size, a.size, seed=1)).to(dev)]
    for i in range(1, e.nb_bindings):
        bufs.append(torch.empty(a.batch * int(np.prod(e.dims[i])), dtype=torch.float32, device=dev))
    prob = bufs[e.names.index("prob")].reshape(a.batch, -1)
    max_out = (prob.shape[1] - 1) // 38   # det / seg: 1 + max_out Detection records of 38 floats (yolov5/src/types.h)
    post = {}

    def step():
        e.enqueue(a.batch, bufs)
        if a.masks:
            proto = bufs[e.names.index("proto")].reshape(a.batch, 32, a.size // 4, a.size // 4)
            post["idx"], post["cnt"], _ = capi.yolov5_nms(prob, max_out, conf_thresh=a.conf)
            post["masks"] = capi.seg_masks(prob, post["idx"], post["cnt"], proto, a.size, a.size, a.max_keep, out=post.get("masks"))

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    head = "fused" if kinds.count("yolo5_head") else ("plugin" if kinds.count("plugin") else "none")
    out = {"model": name, "task": a.task, "batch": a.batch, "size": a.size, "fp16": not a.fp32, "head": head,
           "to_linear_ops": kinds.count("to_linear"), "ops": len(kinds), "ms_per_step": round(ms, 4), "img_per_s": round(a.batch * 1000.0 / ms, 1)}
    if a.task != 4:
        out["candidates_image0"] = int(prob[0, 0].item())
    if a.masks:
        # a written pixel is non-zero exactly inside its clipped rect (the sigmoid never returns 0 on these logits)
        cnt = post["cnt"].cpu().numpy()
        kept = np.minimum(cnt, a.max_keep)
        live = torch.arange(a.max_keep, device=dev)[None, :] < post["cnt"][:, None]
        area = int((post["masks"] != 0)[live].sum().item())
        plane = (a.size // 4) ** 2 * 4
        out.update(step="engine + yolov5_nms + seg_masks", conf=a.conf, max_keep=a.max_keep, nms_kept=cnt.tolist(), masks_written=int(kept.sum()),
                   rect_pixels=area, plane_bytes_written=int(kept.sum()) * plane, proto_bytes_read=area * 128)
    if a.ops:
        out["profile"] = e.profile(a.batch, bufs)
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
