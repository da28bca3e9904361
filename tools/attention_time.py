"""The two fused attention kernels alone, on equal-sized shapes, for a `rocprofv3 --kernel-trace --stats` run: YOLO11's PSA subgraph
(B 32, 2 heads, 400 pixels, kd 32, hd 64: 1.97 GFLOP, psa_attention_kernel on the vector ALU) and YOLOv12's AAttn subgraph (B 32, 2 heads,
area 1, 400 pixels, kd = hd = 32: 1.31 GFLOP, area_attention_mfma_kernel), plus the two YOLOv12n shapes (2 heads, 1600 pixels, area 4;
4 heads, 400 pixels, area 1).  Each subgraph is a 1x1 qkv convolution, the attention op and the sum O + V, enqueued --steps times; the
kernels' durations are read from the trace.  Prints the ops' algorithmic FLOP so that the trace can be turned into FLOP/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tensorrtx_amd import builder, engine  # noqa: E402


def psa_net(B, heads, H, W, kd=32, hd=64):
    N, C = H * W, heads * (2 * kd + hd)
    wq = (np.random.default_rng(0).standard_normal((C, 16, 1, 1)) / 4).astype(np.float32)
    net = builder.Network(explicit_batch=True, fp16=True)
    try:
        qkv = net.out(net.conv(net.input("x", (B, 16, H, W)), wq))
        v4 = net.out(net.shuffle(qkv, reshape=(B, heads, -1, N)))
        q = net.out(net.slice(v4, (0, 0, 0, 0), (B, heads, kd, N)))
        k = net.out(net.slice(v4, (0, 0, kd, 0), (B, heads, kd, N)))
        v = net.out(net.slice(v4, (0, 0, 2 * kd, 0), (B, heads, hd, N)))
        s = net.out(net.scale_uniform(net.out(net.matmul(net.out(net.shuffle(q, perm1=(0, 1, 3, 2))), k)), kd ** -0.5))
        pt = net.out(net.shuffle(net.out(net.softmax(s, axes=1 << 3)), perm1=(0, 1, 3, 2)))
        o = net.out(net.shuffle(net.out(net.matmul(v, pt)), reshape=(B, -1, H, W)))
        net.mark_output(net.out(net.elementwise(o, net.out(net.shuffle(v, reshape=(B, -1, H, W))))), "y")
        return net.build()
    finally:
        net.close()


def aattn_net(B, heads, H, W, area, hd=32):
    N = H * W
    wq = (np.random.default_rng(0).standard_normal((3 * heads * hd, 16, 1, 1)) / 4).astype(np.float32)
    net = builder.Network(explicit_batch=True, fp16=True)
    try:
        qkv = net.out(net.conv(net.input("x", (B, 16, H, W)), wq))
        t = net.out(net.shuffle(qkv, reshape=(B, -1, N), perm2=(0, 2, 1)))
        t = net.out(net.shuffle(t, reshape=(B * area, N // area, heads, 3 * hd), perm2=(0, 2, 3, 1)))
        part = (B * area, heads, hd, N // area)
        q, k, v = (net.out(net.slice(t, (0, 0, i * hd, 0), part)) for i in range(3))
        s = net.out(net.scale_uniform(net.out(net.matmul(net.out(net.shuffle(q, perm1=(0, 1, 3, 2))), k)), 0.176777))
        pt = net.out(net.shuffle(net.out(net.softmax(s, axes=1 << 3)), perm1=(0, 1, 3, 2)))

        def image(z):
            z = net.out(net.shuffle(net.out(net.shuffle(z, perm1=(0, 3, 1, 2))), reshape=(B, H, W, -1)))
            return net.out(net.shuffle(z, perm1=(0, 3, 1, 2)))
        net.mark_output(net.out(net.elementwise(image(net.out(net.matmul(v, pt))), image(v))), "y")
        return net.build()
    finally:
        net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = [("psa B32 heads2 N400 kd32 hd64", psa_net(32, 2, 20, 20), (32, 20, 20)),
             ("area B32 heads2 N400 area1", aattn_net(32, 2, 20, 20, 1), (32, 20, 20)),
             ("area B32 heads4 N400 area1", aattn_net(32, 4, 20, 20, 1), (32, 20, 20)),
             ("area B32 heads2 N1600 area4", aattn_net(32, 2, 40, 40, 4), (32, 40, 40))]
    for name, plan, (B, H, W) in cases:
        (att,) = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "attention"]
        e = engine.Engine(plan)
        x = torch.randn(B, 16, H, W, device=dev)
        y = torch.empty(int(np.prod(e.dims[1])), dtype=torch.float32, device=dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(a.steps + 5):
            if i == 5:
                torch.cuda.synchronize()
                t0.record()
            e.enqueue(B, [x, y])
        t1.record()
        torch.cuda.synchronize()
        print(json.dumps({"case": name, "attention_flops": att["flops"], "attention_bytes": att["bytes"], "launches": a.steps + 5,
                          "subgraph_ms_per_step": round(t0.elapsed_time(t1) / a.steps, 4)}))
        e.close()


if __name__ == "__main__":
    main()
