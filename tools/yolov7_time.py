"""Build YOLOv7 engines from the seeded synthetic weights (tensorrtx_amd.synth.yolov7_state) and time them through one execution context.
Usage: python tools/yolov7_time.py [--models yolov7tiny,yolov7,yolov7w6] [--batch 32] [--size 640] [--p6-batch 8] [--p6-size 1280]
[--steps 20] [--warmup 5] [--pairs 5] [--out profiles/yolov7_time.jsonl].  The P6 models (w6, e6) take --p6-batch / --p6-size.
Per model, one JSON line each for:
  * "head_ab": the fused head against TRTX_YOLO7_HEAD=0 (one layout pass per level and the 6-float YoloLayer_TRT plugin), two engines of
    the same build alive at once and timed in alternating pairs in this one process: median and range of the pairs, and the run-to-run
    spread of one engine (the range of the fused engine's own runs);
  * "reorg_ab" (yolov7w6 only): the folded ReOrg against TRTX_REORG_FOLD=0 (four gathers, a concat and a layout pass), the same way;
  * "ops": the per-op times of one profiled enqueue (trtx_context_profile) summed by kind, with the shares of the stride-1 3x3 stem and
    the stride-2 3x3 convolution behind it (the P5 stem pair), of the MP / DownC pools, of the SPP pool chain and of the head.
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

P6 = ("yolov7w6", "yolov7e6")


def make(name, path, batch, size, switch=None):
    """(plan ops, engine, buffers); the switches are read when the plan is lowered: at build and at engine creation"""
    if switch:
        os.environ[switch] = "0"
    try:
        # max_out above the anchor count: the synthetic weights keep more candidates than a trained model, and a full buffer would hide writes
        anchors = 3 * sum((size // s) ** 2 for s in ((8, 16, 32, 64) if name in P6 else (8, 16, 32)))
        plan = engine.build_plan(name, path, batch=batch, h=size, w=size, fp16=1, max_out=anchors + 16)
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


def pairs(e, bufs, r, rbufs, batch, a):
    for _ in range(a.warmup):
        e.enqueue(batch, bufs)
        r.enqueue(batch, rbufs)
    torch.cuda.synchronize()
    on, off = [], []
    for _ in range(a.pairs):   # alternating pairs: both engines see the same machine state
        on.append(timed(e, bufs, batch, a.steps))
        off.append(timed(r, rbufs, batch, a.steps))
    return on, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="yolov7tiny,yolov7,yolov7w6")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--p6-batch", type=int, default=8)
    ap.add_argument("--p6-size", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "yolov7_time.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)

    def emit(ln):
        print(json.dumps(ln), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(ln) + "\n")

    for name in a.models.split(","):
        batch, size = (a.p6_batch, a.p6_size) if name in P6 else (a.batch, a.size)
        path = os.path.join(tempfile.gettempdir(), f"{name}_synth_time.wts")
        wts.write_wts(path, synth.yolov7_state(name))
        base = {"model": name, "batch": batch, "size": size, "fp16": True, "steps": a.steps, "pairs": a.pairs}
        ops, e, bufs = make(name, path, batch, size)
        kinds = [o["kind"] for o in ops]
        assert kinds.count("yolo7_head") == 1 and kinds.count("pool_chain") == 1 and "gather" not in kinds
        rops, r, rbufs = make(name, path, batch, size, "TRTX_YOLO7_HEAD")
        rkinds = [o["kind"] for o in rops]
        assert rkinds.count("plugin") == 1 and rkinds.count("yolo7_head") == 0
        on, off = pairs(e, bufs, r, rbufs, batch, a)
        r.close()
        f, p = spread(on), spread(off)
        out = bufs[e.names.index("prob")].reshape(batch, -1)
        emit(dict(base, what="head_ab", fused_ms=f, plugin_route_ms=p, img_per_s=round(batch * 1000.0 / f["median"], 1), fused_ops=len(kinds),
                  plugin_route_ops=len(rkinds), plugin_route_to_linear=rkinds.count("to_linear"), gain_ms_median=round(p["median"] - f["median"], 4),
                  pair_gain_ms=[round(y - x, 4) for x, y in zip(on, off)], one_engine_spread_ms=round(f["max"] - f["min"], 4),
                  candidates_image0=int(out[0, 0].item()), max_out=(out.shape[1] - 1) // 6))
        if name == "yolov7w6":
            gops, g, gbufs = make(name, path, batch, size, "TRTX_REORG_FOLD")
            gkinds = [o["kind"] for o in gops]
            assert gkinds.count("gather") == 4
            on, off = pairs(e, bufs, g, gbufs, batch, a)
            g.close()
            f, p = spread(on), spread(off)
            emit(dict(base, what="reorg_ab", folded_ms=f, gathers_ms=p, folded_ops=len(kinds), gathers_ops=len(gkinds),
                      gain_ms_median=round(p["median"] - f["median"], 4), pair_gain_ms=[round(y - x, 4) for x, y in zip(on, off)],
                      one_engine_spread_ms=round(f["max"] - f["min"], 4)))
        prof = e.profile(batch, bufs)
        by = collections.Counter()
        total = sum(x["ms"] for x in prof)
        for x in prof:
            by[x["kind"]] += x["ms"]
        extra = {}
        if len(prof) == len(ops):
            named = list(zip(prof, ops))
            extra["first_two_convs_ms"] = round(sum(x["ms"] for x, o in named[:3] if o["kind"] == "conv"), 4)   # the P5 stem pair (P6: the folded stem and its successor)
            extra["direct_conv_ms"] = round(sum(x["ms"] for x, o in named if o["kind"] == "conv" and not (o["igemm"] or o["stem"] or o.get("dw") or o.get("grouped"))), 4)
        emit(dict(base, what="ops", profiled_ms=round(total, 4), ms_by_kind={k: round(v, 4) for k, v in sorted(by.items(), key=lambda kv: -kv[1])},
                  count_by_kind=dict(collections.Counter(kinds)), mp_pool_share=round(by.get("pool", 0.0) / total, 4),
                  spp_chain_share=round(by.get("pool_chain", 0.0) / total, 4), head_ms=round(by.get("yolo7_head", 0.0), 4), **extra))
        e.close()


if __name__ == "__main__":
    main()
