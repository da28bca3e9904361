"""Time YOLOv13's C3AH block (cv1, cv2, AdaHGComputation, cv3; yolov13/src/block.cpp:814-829) at the yolov13 n / s / x widths of its HyperACE branch, fp16,
640 x 640 (the stride-16 map: 40 x 40 tokens), batch 32, one execution context: the fused `hgconv` op against the generic lowering of the same graph
(TRTX_HGCONV=0, read when the engine is created), in alternating pairs; the median of five per side goes to profiles/hgconv_time.jsonl.

  python tools/hgconv_time.py                      # the three widths, A/B
  python tools/hgconv_time.py --scale x --chain    # one width, fused only, a few steps: the program for `rocprofv3 --kernel-trace --stats -- python ...`

Seeded synthetic weights (tests/hgconv_cases.py's generator shapes); 1x1 convolutions without activation stand in for C3AH's Conv blocks."""
import argparse
import collections
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tensorrtx_amd import engine  # noqa: E402
from tests import hgconv_cases as hc  # noqa: E402

# C3AH's inner width c_ = 0.5 * c and the hyperedge count per scale (yolov13/src/model.cpp: HyperACE(..., num_hyperedges = 4 / 8 / 12))
SCALES = {"n": (64, 4), "s": (128, 8), "x": (384, 12)}


def weights(D, E, N, seed=0):
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731
    return {"w_ctx": n(E * D, 2 * D) / np.float32(np.sqrt(2 * D)), "b_ctx": 0.1 * n(E * D), "proto": n(E, D), "w_pre": 0.3 * n(D, D), "b_pre": n(D),
            "w_edge": n(D, D) * np.float32(2 / np.sqrt(D)), "b_edge": 0.5 * n(D), "w_node": n(D, D) * np.float32(N / (2 * E) / np.sqrt(D)), "b_node": 0.5 * n(D)}


def bytes_moved(B, N, D, E):
    """Algorithmic bytes per launch of the fused chain (kernels/hgconv.hip), from the shapes"""
    nt, ed = -(-N // 128), E * D
    x = 2 * B * N * D
    return {"hg_colstat": x + 8 * B * D, "hg_proto": 4 * (ed * 2 * D * -(-B // 8) + 2 * B * D + 2 * ed + B * ed), "hg_rows<Q>": 4 * (D * D + 2 * B * ed),
            "hg_logits": x + 4 * B * (ed + N * E + nt * (2 * E + ed)), "hg_merge": 4 * B * (nt * (2 * E + ed) + ed + 2 * E),
            "hg_rows<edge>": 4 * (D * D + D + 2 * B * ed), "hg_rows<node>": 4 * (D * D + 2 * B * ed), "hg_node": 2 * x + 4 * B * (N * E + ed + 2 * E) + 4 * D}


def run(scale, B, size, steps, warmup, generic):
    D, E = SCALES[scale]
    H = W = size // 16
    if generic:
        os.environ["TRTX_HGCONV"] = "0"
    else:
        os.environ.pop("TRTX_HGCONV", None)
    # the block's input has the 2 D channels C3AH reads (e = 0.5); its fp32 -> NHWC layout pass and the output's are in both sides' times
    cw = hc.c3ah_weights(D, cin=2 * D, cout=2 * D, seed=1)
    plan = hc.subgraph_net(B, D, E, H, W, weights(D, E, H * W), cw)
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert (kinds["hgconv"] == 0) == generic, kinds
    e = engine.Engine(plan)
    dev = torch.device("cuda:0")
    bufs = []
    for i in range(e.nb_bindings):
        n = int(np.prod(e.dims[i]))
        bufs.append(torch.randn(n, dtype=torch.float32, device=dev) if e.is_input[i] else torch.empty(n, dtype=torch.float32, device=dev))
    for _ in range(warmup):
        e.enqueue(B, bufs)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        e.enqueue(B, bufs)
    t1.record()
    torch.cuda.synchronize()
    e.close()
    return t0.elapsed_time(t1) / steps, sum(kinds.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", default="n,s,x")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--chain", action="store_true", help="fused only, once: the program to run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hgconv_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about time"
    for scale in a.scale.split(","):
        D, E = SCALES[scale]
        N = (a.size // 16) ** 2
        if a.chain:
            ms, ops = run(scale, a.batch, a.size, a.steps, a.warmup, False)
            print(json.dumps({"scale": scale, "D": D, "E": E, "N": N, "batch": a.batch, "fused_ms": round(ms, 4), "ops": ops,
                              "bytes_per_launch": bytes_moved(a.batch, N, D, E)}))
            continue
        fused, generic, ops = [], [], {}
        for _ in range(a.pairs):
            ms, ops["fused"] = run(scale, a.batch, a.size, a.steps, a.warmup, False)
            fused.append(ms)
            ms, ops["generic"] = run(scale, a.batch, a.size, max(3, a.steps // 5), 2, True)
            generic.append(ms)
        rec = {"block": "C3AH", "scale": scale, "D": D, "E": E, "N": N, "batch": a.batch, "size": a.size, "fp16": True, "pairs": a.pairs,
               "fused_ms": round(statistics.median(fused), 4), "generic_ms": round(statistics.median(generic), 4),
               "fused_ms_all": [round(v, 4) for v in fused], "generic_ms_all": [round(v, 4) for v in generic],
               "ratio_generic_over_fused": round(statistics.median(generic) / statistics.median(fused), 2), "ops": ops,
               "hgconv_bytes_per_launch": bytes_moved(a.batch, N, D, E)}
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
