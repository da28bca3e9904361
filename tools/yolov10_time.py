"""Build YOLOv10 engines from the seeded synthetic weights (tensorrtx_amd.synth.yolov10_state) and time them through one execution context, fp16.
Usage: python tools/yolov10_time.py [--runs yolov10n:32:640,yolov10m:8:640] [--steps 20] [--warmup 5] [--pairs 5]
[--out profiles/yolov10_time.jsonl].  A run is model:batch:size.
Per run, one JSON line each for:
  * "head_ab": the default engine against TRTX_YOLO10_HEAD=0 (layout passes, the DFL chain, concat scatters and the 6-float YoloLayer_TRT plugin);
  * "fold_ab": the default engine against TRTX_REPVGGDW_FOLD=0 (RepVGGDW as two depthwise launches, a sigmoid and a product) - only for a
    model that has a RepVGGDW block (yolov10n, yolov10s);
    both: two engines of the same build alive at once and timed in alternating pairs in this one process: median and range of the pairs, the
    per-pair gains, and the run-to-run spread of one engine (the range of the default engine's own runs).  A difference counts only beyond
    that spread ("verdict");
  * "ops": the per-op times of one profiled enqueue (trtx_context_profile) summed by kind, with the shares of the depthwise convolutions, the
    attention and the head.
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


def convs_of(ops):
    return [o for o in ops if o["kind"] == "conv"] + [m for o in ops if o["kind"] == "conv_group" for m in o["members"]]


def ab(e, bufs, r, rbufs, batch, a):
    for _ in range(a.warmup):
        e.enqueue(batch, bufs)
        r.enqueue(batch, rbufs)
    torch.cuda.synchronize()
    on, off = [], []
    for _ in range(a.pairs):   # alternating pairs: both engines see the same machine state
        on.append(timed(e, bufs, batch, a.steps))
        off.append(timed(r, rbufs, batch, a.steps))
    f, p = spread(on), spread(off)
    gain, noise = round(p["median"] - f["median"], 4), round(f["max"] - f["min"], 4)
    return dict(default_ms=f, switched_off_ms=p, gain_ms_median=gain, pair_gain_ms=[round(y - x, 4) for x, y in zip(on, off)],
                one_engine_spread_ms=noise, verdict="gain beyond the spread" if gain > noise else "no measurable difference")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="yolov10n:32:640,yolov10m:8:640")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "yolov10_time.jsonl"))
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
        wts.write_wts(path, synth.yolov10_state(name), dialect="double")
        base = {"model": name, "batch": batch, "size": size, "fp16": True, "steps": a.steps, "pairs": a.pairs}
        ops, e, bufs = make(name, path, batch, size)
        kinds = [o["kind"] for o in ops]
        folds = sum(bool(o.get("repvggdw_fold")) for o in convs_of(ops))
        assert kinds.count("yolo10_head") == 1 and kinds.count("attention") == 1 and "plugin" not in kinds and "to_linear" not in kinds
        rops, r, rbufs = make(name, path, batch, size, "TRTX_YOLO10_HEAD")
        rkinds = [o["kind"] for o in rops]
        assert rkinds.count("plugin") == 1 and rkinds.count("yolo10_head") == 0
        res = ab(e, bufs, r, rbufs, batch, a)
        r.close()
        out = bufs[e.names.index("output")]   # (explicit batch: the binding's dims hold the batch; image 0's row comes first either way)
        emit(dict(base, what="head_ab", switch="TRTX_YOLO10_HEAD=0", img_per_s=round(batch * 1000.0 / res["default_ms"]["median"], 1), default_ops=len(kinds),
                  switched_off_ops=len(rkinds), candidates_image0=int(out[0].item()), cells=sum((size // s) ** 2 for s in (8, 16, 32)),
                  max_out=(int(np.prod(e.dims[e.names.index("output")][-3:])) - 1) // 6, **res))
        if folds:
            rops, r, rbufs = make(name, path, batch, size, "TRTX_REPVGGDW_FOLD")
            assert not any(o.get("repvggdw_fold") for o in convs_of(rops))
            res = ab(e, bufs, r, rbufs, batch, a)
            r.close()
            emit(dict(base, what="fold_ab", switch="TRTX_REPVGGDW_FOLD=0", folded_blocks=folds, default_ops=len(kinds), switched_off_ops=len(rops), **res))
        prof = e.profile(batch, bufs)
        by = collections.Counter()
        total = sum(x["ms"] for x in prof)
        for x in prof:
            by[x["kind"]] += x["ms"]
        extra = {}
        if len(prof) == len(ops):   # one profile row per op: the depthwise convolutions that stand alone
            dw = sum(p["ms"] for p, o in zip(prof, ops) if o["kind"] == "conv" and o.get("dw"))
            extra["depthwise_ms"] = round(dw, 4)
            extra["depthwise_share"] = round(dw / total, 4)
            extra["depthwise_ops"] = sum(1 for o in ops if o["kind"] == "conv" and o.get("dw"))
        emit(dict(base, what="ops", profiled_ms=round(total, 4), ms_by_kind={k: round(v, 4) for k, v in sorted(by.items(), key=lambda kv: -kv[1])},
                  count_by_kind=dict(collections.Counter(kinds)), attention_ms=round(by.get("attention", 0.0), 4),
                  attention_share=round(by.get("attention", 0.0) / total, 4), head_ms=round(by.get("yolo10_head", 0.0), 4),
                  head_share=round(by.get("yolo10_head", 0.0) / total, 4), **extra))
        e.close()


if __name__ == "__main__":
    main()
