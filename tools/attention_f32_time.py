"""Time attention in fp32 engines (kernels/attention_f32.hip, attention_f32) against the generic lowering it replaces.

The kernel alone, through the C ABI, at the project's standard shapes - B 32 with 2 heads / N 400 / (32, 64), 4 heads / N 400 / area 1 / (32, 32) and
2 heads / N 1600 / area 4 / (32, 32) - alternating with the generic op sequence of the same attention: a one-attention fp32 engine (the networks of
tests/test_attention_f32_cpu.py) lowered with TRTX_ATTENTION_F32 unset minus the same engine's time with the switch on plus the kernel's own, so that
the 1x1 qkv convolution and the final sum cancel; both engine times are recorded as they are.  Then whole fp32 engines - yolo11n, yolov10n, yolov12n,
batch 32, 640 x 640, one execution context, static default kernels - lowered with TRTX_ATTENTION_F32=1 and with it unset (read when the engine is
created), in alternating pairs.  Every run, the medians and the spreads go to profiles/attention_f32_time.jsonl.

  python tools/attention_f32_time.py [--only kernel|engines]

Seeded synthetic weights (tensorrtx_amd/synth.py)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tensorrtx_amd import capi, engine, synth, wts  # noqa: E402
from tests.test_attention_f32_cpu import attention_net  # noqa: E402

SHAPES = [("psa", 2, 20, 20, 1, 32, 64), ("area", 4, 20, 20, 1, 32, 32), ("area", 2, 40, 40, 4, 32, 32)]   # kind, heads, H, W, area, kd, hd at B 32
ENGINES = [("yolo11n", lambda: synth.yolo11_state("n"), 32), ("yolov10n", lambda: synth.yolov10_state("yolov10n"), 32),
           ("yolo12n", lambda: synth.yolo12_state("n"), 32)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def run_engine(plan, B, steps, warmup, fused):
    os.environ.pop("TRTX_ATTENTION_F32", None)
    if fused:
        os.environ["TRTX_ATTENTION_F32"] = "1"
    low = engine.describe_plan(plan, lowered=True)["ops"]
    kinds = {k: sum(o["kind"] == k for o in low) for k in ("attention", "matmul", "softmax")}
    assert all(o.get("f32") for o in low if o["kind"] == "attention") and (kinds["attention"] > 0) == fused
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    per = 1 if engine.describe_plan(plan)["explicit_batch"] else B
    bufs = []
    for i in range(e.nb_bindings):
        n = per * int(np.prod(e.dims[i]))
        bufs.append(torch.randn(n, dtype=torch.float32, device=dev) if e.is_input[i] else torch.empty(n, dtype=torch.float32, device=dev))
    ms = timed(lambda: e.enqueue(B, bufs), steps, warmup)
    e.close()
    return ms, kinds


def spread(v):
    return round(max(v) - min(v), 4)


def kernel_record(kind, heads, H, W, area, kd, hd, a):
    B, N, dev = 32, H * W, torch.device("cuda:0")
    qkv = torch.randn((B, N, heads * (2 * kd + hd)), generator=torch.Generator().manual_seed(kd + hd)).to(dev)
    o, v = (torch.empty((B, N, heads * hd), dtype=torch.float32, device=dev) for _ in range(2))
    plan, _, _ = attention_net(kind, area, kd, hd, B=B, heads=heads, H=H, W=W)
    ms = {"kernel": [], "engine_fused": [], "engine_generic": []}
    for _ in range(a.pairs):
        ms["kernel"].append(timed(lambda: capi.attention_f32(qkv, heads, area, kd ** -0.5, o, v, kd=kd, hd=hd), 200, 20))
        ms["engine_fused"].append(run_engine(plan, B, a.steps, a.warmup, True)[0])
        ms["engine_generic"].append(run_engine(plan, B, a.steps, a.warmup, False)[0])
    generic = [g - f + k for g, f, k in zip(ms["engine_generic"], ms["engine_fused"], ms["kernel"])]
    rec = {"what": "kernel", "kd": kd, "hd": hd, "B": B, "heads": heads, "N": N, "area": area, "pairs": a.pairs,
           "kernel_us": round(1e3 * statistics.median(ms["kernel"]), 2), "generic_ops_us": round(1e3 * statistics.median(generic), 2),
           "generic_ops_us_all": [round(1e3 * g, 2) for g in generic]}
    for k, vals in ms.items():
        rec[k + "_us_all"] = [round(1e3 * x, 2) for x in vals]
    return rec


def engine_record(name, state, B, a):
    path = os.path.join(tempfile.gettempdir(), f"{name}_attention_f32_time.wts")
    wts.write_wts(path, state(), dialect="double")
    plan = engine.build_plan(name, path, batch=B, h=a.size, w=a.size, fp16=0)
    side, kinds = {"fused": [], "generic": []}, {}
    for _ in range(a.pairs):
        for s in side:
            ms, kinds[s] = run_engine(plan, B, a.steps, a.warmup, s == "fused")
            side[s].append(ms)
    return {"what": "engine", "model": name, "batch": B, "size": a.size, "fp16": False, "pairs": a.pairs, "ops": kinds,
            "fused_ms": round(statistics.median(side["fused"]), 4), "generic_ms": round(statistics.median(side["generic"]), 4),
            "fused_ms_all": [round(v, 4) for v in side["fused"]], "generic_ms_all": [round(v, 4) for v in side["generic"]],
            "fused_spread_ms": spread(side["fused"]), "generic_spread_ms": spread(side["generic"]),
            "saved_ms_per_pair": [round(g - f, 4) for f, g in zip(side["fused"], side["generic"])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only", choices=("kernel", "engines"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_f32_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    os.environ.setdefault("TRTX_TUNE", "0")   # the static default kernel of every convolution on both sides: the pairs differ by the attention alone
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    jobs = [lambda s=s: kernel_record(*s, a) for s in SHAPES] if a.only != "engines" else []
    jobs += [lambda e=e: engine_record(*e, a) for e in ENGINES] if a.only != "kernel" else []
    for job in jobs:
        rec = job()
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
