"""Time PSA attention on the matrix pipe (kernels/attention_mfma.hip, psa_attention_mfma_f16) against the vector-ALU kernel (kernels/attention.hip).

The kernel alone, through the C ABI: B 32, 2 heads, N 400 (YOLO11n's C2PSA at 640 x 640) for the head shapes (32, 64) and (36, 72), alternating with
psa_attention_f16 on the same tensor.  Then whole fp16 engines - yolo11n b32, yolov10n b32, yolov10m b8, 640 x 640, one execution context, static default
kernels - lowered with TRTX_PSA_MFMA=2 (the MFMA kernel for both head shapes) and with TRTX_PSA_MFMA=0 (read when the engine is created), in alternating
pairs.  Every run, the medians and the spreads go to profiles/psa_mfma_time.jsonl.

  python tools/psa_mfma_time.py

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

ENGINES = [("yolo11n", lambda: synth.yolo11_state("n"), 32), ("yolov10n", lambda: synth.yolov10_state("yolov10n"), 32),
           ("yolov10m", lambda: synth.yolov10_state("yolov10m"), 8)]


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


def kernel_alone(kd, hd, B, heads, N, steps, warmup, pairs):
    dev = torch.device("cuda:0")
    qkv = torch.randn((B, N, heads * (2 * kd + hd)), generator=torch.Generator().manual_seed(kd)).half().to(dev)
    bufs = {side: [torch.empty((B, N, heads * hd), dtype=torch.float16, device=dev) for _ in range(2)] for side in ("mfma", "vector")}
    launch = {"mfma": lambda: capi.psa_attention_mfma(qkv, heads, kd ** -0.5, *bufs["mfma"], kd=kd, hd=hd),
              "vector": lambda: capi.psa_attention(qkv, heads, kd ** -0.5, *bufs["vector"], kd=kd, hd=hd)}
    ms = {"mfma": [], "vector": []}
    for _ in range(pairs):
        for side in ms:
            ms[side].append(timed(launch[side], steps, warmup))
    assert torch.equal(bufs["mfma"][1], bufs["vector"][1])   # the V images
    worst = (bufs["mfma"][0].float() - bufs["vector"][0].float()).abs().max().item()
    return ms, worst


def run_engine(name, path, B, size, steps, warmup, vector):
    os.environ["TRTX_PSA_MFMA"] = "0" if vector else "2"   # 2: the MFMA kernel for every head shape it takes, also where the default keeps the vector kernel
    plan = engine.build_plan(name, path, batch=B, h=size, w=size, fp16=1)
    att = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "attention"]
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    per = 1 if engine.describe_plan(plan)["explicit_batch"] else B
    bufs = []
    for i in range(e.nb_bindings):
        n = per * int(np.prod(e.dims[i]))
        bufs.append(torch.randn(n, dtype=torch.float32, device=dev) if e.is_input[i] else torch.empty(n, dtype=torch.float32, device=dev))
    ms = timed(lambda: e.enqueue(B, bufs), steps, warmup)
    e.close()
    return ms, [(o["kd"], o["hd"], bool(o.get("mfma"))) for o in att]


def spread(v):
    return round(max(v) - min(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psa_mfma_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    os.environ.setdefault("TRTX_TUNE", "0")   # the static default kernel of every convolution on both sides: the pairs differ by the attention alone
    recs = []
    for kd, hd in ((32, 64), (36, 72)):
        ms, worst = kernel_alone(kd, hd, 32, 2, 400, 200, 20, a.pairs)
        recs.append({"what": "kernel", "kd": kd, "hd": hd, "B": 32, "heads": 2, "N": 400, "pairs": a.pairs,
                     "mfma_us": round(1e3 * statistics.median(ms["mfma"]), 2), "vector_us": round(1e3 * statistics.median(ms["vector"]), 2),
                     "mfma_us_all": [round(1e3 * v, 2) for v in ms["mfma"]], "vector_us_all": [round(1e3 * v, 2) for v in ms["vector"]],
                     "max_abs_diff_of_O": worst})
    for name, state, B in ENGINES:
        path = os.path.join(tempfile.gettempdir(), f"{name}_psa_mfma_time.wts")
        wts.write_wts(path, state(), dialect="double")
        side = {"mfma": [], "vector": []}
        att = {}
        for _ in range(a.pairs):
            for s in side:
                ms, att[s] = run_engine(name, path, B, a.size, a.steps, a.warmup, s == "vector")
                side[s].append(ms)
        saved = [v - m for m, v in zip(side["mfma"], side["vector"])]
        recs.append({"what": "engine", "model": name, "batch": B, "size": a.size, "fp16": True, "pairs": a.pairs, "attention": att,
                     "mfma_ms": round(statistics.median(side["mfma"]), 4), "vector_ms": round(statistics.median(side["vector"]), 4),
                     "mfma_ms_all": [round(v, 4) for v in side["mfma"]], "vector_ms_all": [round(v, 4) for v in side["vector"]],
                     "mfma_spread_ms": spread(side["mfma"]), "vector_spread_ms": spread(side["vector"]),
                     "saved_ms_per_pair": [round(v, 4) for v in saved]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
