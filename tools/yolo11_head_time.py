"""The det head (trtx_yolo_head_decode_nhwc) and the seg task head (trtx_yolo_task_head_decode_nhwc) on the same seeded NHWC fp16 heads
(YOLO11n 640² batch 32 shapes, ld 144, ~3 % of the cells past the 0.1 gate), each launched alone on one stream, alternating.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel times (profiles/yolo11n_heads_isolated_kstats.csv)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrtx_amd import capi  # noqa: E402

dev = torch.device("cuda:0")
B, S, nc = 32, 640, 80
rng = np.random.default_rng(0)
heads, branches = [], []
for s in (8, 16, 32):
    g = S // s
    x = rng.normal(0, 1.5, size=(B, g, g, 144)).astype(np.float32)
    x[..., 64:] = rng.normal(-7.2, 1.5, size=(B, g, g, 80))
    heads.append(torch.from_numpy(x).half().to(dev))
    branches.append(torch.from_numpy(rng.normal(0, 1, size=(B, g, g, 32)).astype(np.float32)).half().to(dev))
dfl = torch.arange(16.0, device=dev)
runs = {"det": lambda: capi.yolo_head_decode_nhwc(heads, nc, S, S, [8, 16, 32], dfl),
        "seg": lambda: capi.yolo_task_head_decode_nhwc(heads, branches, nc, S, S, [8, 16, 32], dfl, seg=True)}
for rnd in range(3):
    for name, fn in runs.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        for _ in range(50):
            out = fn()
        torch.cuda.synchronize()
        print(name, rnd, "candidates per image", float(out[:, 0].float().mean()))
