"""Time the grouped and channel-view convolutions of fp32 engines on kernels/conv_patch_f32.hip (TRTX_CONV_F32_PATCH=1) against the same plan with the switch
unset (the scalar direct kernel): one-layer fp32 engines of YOLOv9's DDetect box branch (64 -> 64, g = 4, 3x3, at 80 x 80 / 40 x 40 / 20 x 20), of YOLOv9m's
90-channel RepNCSP layers behind a channel slice (3x3 and 1x1), and whole fp32 yolov9t and yolov9m engines at 640 x 640; batch 32, one execution context.  Both
engines of a comparison stay alive in one process (the switch is read when a plan is lowered and when its engine is created) and are timed in alternating
pairs; the median of each side, every run and both spreads go to profiles/conv_patch_f32_time.jsonl.

  python tools/conv_patch_f32_time.py

The layout passes of the bindings (fp32 NCHW <-> NHWC) are in both sides' times; the difference is the convolutions'."""
import argparse
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
from tests import conv_patch_f32_cases as pc  # noqa: E402

SWITCH = "TRTX_CONV_F32_PATCH"
# (name, Cin, Cout, groups, k, map side, input view)
LAYERS = [("ddetect_g4_3x3_80", 64, 64, 4, 3, 80, None), ("ddetect_g4_3x3_40", 64, 64, 4, 3, 40, None), ("ddetect_g4_3x3_20", 64, 64, 4, 3, 20, None),
          ("v9m_90_3x3_40", 90, 90, 1, 3, 40, (90, 180)), ("v9m_90_1x1_40", 90, 90, 1, 1, 40, (90, 180))]
MODELS = ["yolov9t", "yolov9m"]


def make_engine(build, on):
    """(engine, bindings, convolutions on the new kernel, convolutions on the direct kernel) of build() lowered with the switch set or unset"""
    if on:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    plan = build()
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    convs = [o for o in ops if o["kind"] == "conv"] + [m for o in ops if o["kind"] == "conv_group" for m in o["members"]]
    patched = sum(1 for o in convs if o.get("patch_f32"))
    direct = sum(1 for o in convs if not (o["igemm"] or o["stem"] or o.get("dw") or o.get("patch_f32")))
    e = engine.Engine(plan)
    os.environ.pop(SWITCH, None)
    return e, patched, direct


def timed(e, B, bufs, steps, warmup):
    for _ in range(warmup):
        e.enqueue(B, bufs)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        e.enqueue(B, bufs)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def compare(name, build, B, steps, warmup, pairs, out, extra):
    (on, n_on, d_on), (off, n_off, d_off) = make_engine(build, True), make_engine(build, False)
    assert n_on > 0 and d_on == 0 and n_off == 0 and d_off == n_on, (name, n_on, d_on, n_off, d_off)
    dev = torch.device("cuda:0")
    bufs = [torch.randn(B * int(np.prod(on.dims[i])), dtype=torch.float32, device=dev) if on.is_input[i] else
            torch.empty(B * int(np.prod(on.dims[i])), dtype=torch.float32, device=dev) for i in range(on.nb_bindings)]
    t_on, t_off = [], []
    for _ in range(pairs):
        t_on.append(timed(on, B, bufs, steps, warmup))
        t_off.append(timed(off, B, bufs, steps, warmup))
    on.close()
    off.close()
    spread = max(max(t_on) - min(t_on), max(t_off) - min(t_off))
    saved = statistics.median(t_off) - statistics.median(t_on)
    rec = {"what": name, **extra, "batch": B, "fp16": False, "pairs": pairs, "steps": steps, "convs_moved": n_on, "patch_f32_ms": round(statistics.median(t_on), 4),
           "direct_ms": round(statistics.median(t_off), 4), "patch_f32_ms_all": [round(v, 4) for v in t_on], "direct_ms_all": [round(v, 4) for v in t_off],
           "saved_ms": round(saved, 4), "larger_spread_ms": round(spread, 4), "patch_f32_wins": bool(saved > spread)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=100, help="steps per timed window of a one-layer engine")
    ap.add_argument("--model-steps", type=int, default=5, help="steps per timed window of a whole model (a direct-kernel step takes a large part of a second)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated names; default: everything")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_patch_f32_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    os.environ.setdefault("TRTX_TUNE", "0")   # static tactics for every other convolution, on both sides
    only = set(filter(None, a.only.split(",")))
    for name, cin, cout, groups, k, side, view in LAYERS:
        if only and name not in only:
            continue
        case = pc.PCase(name, cin, cout, groups, k, side, side, a.batch, in_view=view)
        compare(name, lambda case=case: pc.build_plan(case)[0], a.batch, a.steps, a.warmup, a.pairs, a.out,
                dict(cin=cin, cout=cout, groups=groups, k=k, hw=side, in_view=view))
    from test_yolov9_cpu import yolov9_wts
    for name in MODELS:
        if only and name not in only:
            continue
        path, _ = yolov9_wts(name)
        compare(name, lambda name=name, path=path: engine.build_plan(name, path, batch=a.batch, h=a.size, w=a.size, fp16=0), a.batch, a.model_steps, 2, a.pairs,
                a.out, dict(hw=a.size))


if __name__ == "__main__":
    main()
