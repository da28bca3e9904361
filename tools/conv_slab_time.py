"""Time the 3x3 convolutions of 32 narrow groups on kernels/conv_slab.hip against the same plan under TRTX_CONV_SLAB=0 (the scalar direct kernel): one-layer
fp16 engines (conv + ReLU) of ResNeXt-50 32x4d's four stride-1 layers and three stride-2 layers at the maps of a 224 x 224 input, the whole resnext50_32x4d
engine at 224 x 224, and the resnet50 engine as the known quantity beside them (no layer of it moves: one side); batch 32, one execution context, static
tactics.  Both engines of a comparison stay alive in one process (the switch is read when a plan is lowered and when its engine is created) and are timed in
five alternating pairs; the median of each side, every run and both spreads go to profiles/conv_slab_time.jsonl.

  python tools/conv_slab_time.py

The layout passes of a one-layer engine's bindings (fp32 NCHW <-> NHWC fp16) are in both sides' times; the difference is the convolution's.  The kernel alone is
timed through the C ABI (TRTX_OP_REPS launches per call between two events): kernel_us, and hbm_share = (input + output bytes) / kernel time over the HBM peak
of bench.py's roofline."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 50
os.environ["TRTX_OP_REPS"] = str(REPS)   # read once, at the library's first launch; kernel_us divides by it, so a preset value does not stand
from tensorrtx_amd import builder, capi, engine, synth, wts  # noqa: E402

SWITCH = "TRTX_CONV_SLAB"
HBM_PEAK_GBPS = 8000.0   # bench.py's roofline figure
# (name, channels, input map side, stride): resnet/resnext50_32x4d.cpp:111-154 at a 224 x 224 input
LAYERS = [("s1_c128_56", 128, 56, 1), ("s1_c256_28", 256, 28, 1), ("s1_c512_14", 512, 14, 1), ("s1_c1024_7", 1024, 7, 1),
          ("s2_c256_56", 256, 56, 2), ("s2_c512_28", 512, 28, 2), ("s2_c1024_14", 1024, 14, 2)]


def layer_plan(C, side, stride, batch):
    rng = np.random.default_rng(C + stride)
    net = builder.Network(max_batch=batch, fp16=True)
    try:
        x = net.out(net.pooling(net.input("x", (C, side, side)), 1, 1))
        w = (rng.standard_normal((C, C // 32, 3, 3)) / np.sqrt(9 * C // 32)).astype(np.float32)
        net.mark_output(net.out(net.activation(net.out(net.conv(x, w, np.zeros(C, np.float32), stride, 1, groups=32)), "relu")), "y")
        return net.build()
    finally:
        net.close()


def make_engine(plan, on):
    """(engine, convolutions on the slab kernel, convolutions on the direct kernel) of the plan lowered with the switch unset or 0"""
    if not on:
        os.environ[SWITCH] = "0"
    convs = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "conv"]
    e = engine.Engine(plan)
    os.environ.pop(SWITCH, None)
    return e, sum(1 for o in convs if o.get("slab")), sum(1 for o in convs if not (o["igemm"] or o["stem"] or o.get("slab")))


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


def kernel_us(C, side, stride, B):
    """the kernel alone: REPS launches per C-ABI call, three calls timed after one warm-up, the median"""
    dev = torch.device("cuda:0")
    x = torch.randn((B, side, side, C), dtype=torch.float16, device=dev)
    w = torch.from_numpy(capi.pack_conv_weights_slab_f16(np.ones((C, C // 32, 3, 3), np.float32) / (9 * C // 32), 32).view(np.float16)).to(dev)
    out, ts = None, []
    for _ in range(4):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = capi.conv2d_slab_nhwc_f16(x, w, None, 32, stride, "relu", out=out)
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3 / REPS)
    return statistics.median(ts[1:]), (x.numel() + out.numel()) * 2


def compare(name, plan, B, steps, warmup, pairs, out, extra, one_side=False):
    (on, n_on, d_on), (off, n_off, d_off) = make_engine(plan, True), make_engine(plan, False)
    assert one_side or (n_on > 0 and d_on == 0 and n_off == 0 and d_off == n_on), (name, n_on, d_on, n_off, d_off)
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
    rec = {"what": name, **extra, "batch": B, "fp16": True, "pairs": pairs, "steps": steps, "convs_moved": n_on, "slab_ms": round(statistics.median(t_on), 4),
           "direct_ms": round(statistics.median(t_off), 4), "slab_ms_all": [round(v, 4) for v in t_on], "direct_ms_all": [round(v, 4) for v in t_off],
           "saved_ms": round(saved, 4), "larger_spread_ms": round(spread, 4), "slab_wins": None if one_side else bool(saved > spread)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100, help="steps per timed window of a one-layer engine")
    ap.add_argument("--model-steps", type=int, default=10, help="steps per timed window of a whole model")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated names; default: everything")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_slab_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    os.environ.setdefault("TRTX_TUNE", "0")   # static tactics for every other convolution, on both sides
    only = set(filter(None, a.only.split(",")))
    for name, C, side, stride in LAYERS:
        if only and name not in only:
            continue
        us, nbytes = kernel_us(C, side, stride, a.batch)
        extra = dict(channels=C, groups=32, hw=side, stride=stride, kernel_us=round(us, 2), io_bytes=nbytes, hbm_share=round(nbytes / (us * 1e-6) / (HBM_PEAK_GBPS * 1e9), 4))
        compare(name, layer_plan(C, side, stride, a.batch), a.batch, a.steps, a.warmup, a.pairs, a.out, extra)
    for name in ("resnext50_32x4d", "resnet50"):
        if only and name not in only:
            continue
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"conv_slab_time_{name}.wts")
        wts.write_wts(path, synth.STATE[name](seed=0), dialect="double")
        plan = engine.build_plan(name, path, batch=a.batch, h=224, w=224, fp16=1)
        compare(name, plan, a.batch, a.model_steps, 2, a.pairs, a.out, dict(hw=224), one_side=name == "resnet50")


if __name__ == "__main__":
    main()
