"""Time YOLOv9m (fp16, one execution context, seeded synthetic weights) with its 40 unaligned-view convolutions on kernels/conv_view.hip against
TRTX_CONV_VIEW=0, whose lowering and kernels are those of the code before the kernel (the scalar direct kernel for these layers).
Usage: python tools/conv_view_time.py [--batch 32] [--size 640] [--steps 40] [--warmup 10] [--pairs 5] [--tune 0] [--out profiles/conv_view_time.jsonl]
Two engines of one build are alive in this one process and are timed in alternating pairs.  JSON lines, printed and appended to --out:
  * "engine_ab": ms per enqueue of both engines (median, min, max, runs), the gain of every pair and the run-to-run spread of each engine;
  * "shapes": one profiled enqueue of each engine (trtx_context_profile), the per-op times of the view layers summed by (Cin, Cout, k), both kernels;
  * "match": the largest difference between the two engines' decoded outputs for one batch (the kernels sum in different orders: not bit-equal).
--tune 0 (the default) builds both engines on the static tactics, so that the implicit-GEMM layers around the view layers run the same kernels in both."""
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


def make(path, a, view):
    """(lowered ops, engine, buffers); TRTX_CONV_VIEW is read when the plan is lowered: at build and at engine creation"""
    if not view:
        os.environ["TRTX_CONV_VIEW"] = "0"
    try:
        cells = sum((a.size // s) ** 2 for s in (8, 16, 32))
        plan = engine.build_plan("yolov9m", path, batch=a.batch, h=a.size, w=a.size, fp16=1, max_out=cells + 16)
        ops = engine.describe_plan(plan, lowered=True)["ops"]
        e = engine.Engine(plan)
    finally:
        os.environ.pop("TRTX_CONV_VIEW", None)
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(synth.images(a.batch, a.size, a.size, seed=1)).to(dev)]
    for i in range(1, e.nb_bindings):
        bufs.append(torch.zeros(a.batch * int(np.prod(e.dims[i])), dtype=torch.float32, device=dev))
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


def by_shape(prof, ops, ref_ops):
    """ms per (Cin, Cout, k) of the ops that are view layers in ref_ops (the default engine's plan: both plans have the same ops in the same order)"""
    out = collections.defaultdict(lambda: [0, 0.0])
    for x, o, r in zip(prof, ops, ref_ops):
        if r["kind"] == "conv" and r.get("view"):
            key = f"{o['cin']}x{o['cout']}k{o['k'][0]}"
            out[key][0] += 1
            out[key][1] += x["ms"]
    return {k: {"count": v[0], "ms": round(v[1], 4)} for k, v in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--tune", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "conv_view_time.jsonl"))
    a = ap.parse_args()
    os.environ["TRTX_TUNE"] = str(a.tune)
    path = os.path.join(tempfile.gettempdir(), "yolov9m_synth_time.wts")
    wts.write_wts(path, synth.yolov9_state("yolov9m"))
    vops, v, vbufs = make(path, a, True)
    dops, d, dbufs = make(path, a, False)
    convs = [o for o in vops if o["kind"] == "conv"]
    nview = sum(1 for o in convs if o.get("view"))
    assert nview and len(vops) == len(dops) and not any(o.get("view") for o in dops)
    for _ in range(a.warmup):
        v.enqueue(a.batch, vbufs)
        d.enqueue(a.batch, dbufs)
    torch.cuda.synchronize()
    vt, dt = [], []
    for _ in range(a.pairs):   # alternating pairs: both engines see the same machine state
        vt.append(timed(v, vbufs, a.batch, a.steps))
        dt.append(timed(d, dbufs, a.batch, a.steps))
    base = {"model": "yolov9m", "batch": a.batch, "size": a.size, "fp16": True, "steps": a.steps, "pairs": a.pairs, "tune": a.tune}
    vs, ds = spread(vt), spread(dt)
    lines = [dict(base, what="engine_ab", view_layers=nview, convs=len(convs), view_ms=vs, direct_ms=ds,
                  img_per_s_view=round(a.batch * 1000.0 / vs["median"], 1), img_per_s_direct=round(a.batch * 1000.0 / ds["median"], 1),
                  pair_gain_ms=[round(y - x, 4) for x, y in zip(vt, dt)], spread_ms_view=round(vs["max"] - vs["min"], 4),
                  spread_ms_direct=round(ds["max"] - ds["min"], 4))]
    vp, dp = v.profile(a.batch, vbufs), d.profile(a.batch, dbufs)
    if len(vp) == len(vops) and len(dp) == len(dops):
        lines.append(dict(base, what="shapes", view=by_shape(vp, vops, vops), direct=by_shape(dp, dops, vops),
                          profiled_ms_view=round(sum(x["ms"] for x in vp), 4), profiled_ms_direct=round(sum(x["ms"] for x in dp), 4)))
    i = v.names.index("output")
    a_out, b_out = vbufs[i].reshape(a.batch, -1), dbufs[i].reshape(a.batch, -1)
    lines.append(dict(base, what="match", candidates_view=[int(c) for c in a_out[:4, 0].tolist()], candidates_direct=[int(c) for c in b_out[:4, 0].tolist()],
                      finite=bool(torch.isfinite(a_out).all().item())))
    v.close()
    d.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        for ln in lines:
            print(json.dumps(ln))
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
