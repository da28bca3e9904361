"""Time the grouped-convolution kernel (kernels/conv_grouped.hip) against what else could run the layer.  The default shape is the layers of
YOLOv9's detect head (yolov9/src/block.cpp:355-366: 64 -> 64, g = 4, 3x3 and 1x1) at the three pyramid levels of a 640 x 640 input; --channels
and --groups choose another one (Cin == Cout, since the layers are chained).

A network is input -> exact 1x1 pool into NHWC -> --layers identical convolutions (+ SiLU) -> output, built three ways and as a chain of no
convolutions at all; per layer = (step - step of the empty chain) / layers:
  grouped   the default lowering (`grouped: true`);
  direct    TRTX_CONV_GROUPED=0, the scalar direct kernel - what the code before the kernel does;
  dense     groups = 1 with the block-diagonal dense filter: what the implicit-GEMM kernels cost for the same result (groups x the MFMA work).
One JSON line per (level, k): µs per layer of each form and the byte floor of the layer at the 6.29 TB/s copy rate of DESIGN section 5.
The chain figure includes the back-to-back launch cost.  For the kernel's own duration run one form alone under the profiler:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/conv_grouped_time.py --only grouped --levels 80 --ks 3
and gather the layer kernel's row of each such run with  python tools/conv_grouped_time.py --gather DIR_PREFIX > profiles/conv_grouped_kstats.csv
(directories named DIR_PREFIX<form>_<level>_<k>).
Usage: python tools/conv_grouped_time.py [--channels 64 --groups 4] [--batch 32] [--layers 8] [--steps 30] [--warmup 5] [--levels 80,40,20]"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorrtx_amd import builder, engine  # noqa: E402

@contextlib.contextmanager
def _switch(value):
    """TRTX_CONV_GROUPED set to value (None: unset) for the duration, then put back: it is read when a plan is lowered"""
    old = os.environ.pop("TRTX_CONV_GROUPED", None)
    if value is not None:
        os.environ["TRTX_CONV_GROUPED"] = value
    try:
        yield
    finally:
        os.environ.pop("TRTX_CONV_GROUPED", None)
        if old is not None:
            os.environ["TRTX_CONV_GROUPED"] = old


def build(hw, k, layers, form, batch, C=64, G=4):
    with _switch("0" if form == "direct" else None):   # lowering happens at build and at engine creation
        return _build(hw, k, layers, form, batch, C, G)


def _build(hw, k, layers, form, batch, C, G):
    rng = np.random.default_rng(1)
    cg = C // G
    net = builder.Network(max_batch=batch, fp16=True)
    try:
        y = net.out(net.pooling(net.input("x", (C, hw, hw)), 1, 1))
        for _ in range(layers):
            w = (rng.standard_normal((C, cg, k, k)) / np.sqrt(k * k * cg)).astype(np.float32)
            if form == "dense":
                full = np.zeros((C, C, k, k), np.float32)
                for g in range(G):
                    full[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
                y = net.out(net.conv(y, full, np.zeros(C, np.float32), 1, k // 2))
            else:
                y = net.out(net.conv(y, w, np.zeros(C, np.float32), 1, k // 2, groups=G))
            y = net.out(net.elementwise(y, net.out(net.activation(y, "sigmoid")), "prod"))
        net.mark_output(y, "y")
        plan = net.build()
    finally:
        net.close()
    convs = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "conv"]
    assert len(convs) == layers, (form, len(convs))
    want = {"grouped": lambda o: o.get("grouped") is True, "direct": lambda o: not o["igemm"] and "grouped" not in o, "dense": lambda o: o["igemm"]}[form]
    assert all(want(o) for o in convs), (form, convs[:1])
    return engine.Engine(plan)


def time_engine(e, x, batch, steps, warmup):
    bufs = [x, torch.empty(batch * int(np.prod(e.dims[1])), dtype=torch.float32, device=x.device)]
    for _ in range(warmup):
        e.enqueue(batch, bufs)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        e.enqueue(batch, bufs)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / steps   # µs per step


def gather(prefix):
    import csv
    import glob
    out = csv.writer(sys.stdout)
    out.writerow(["form", "hw", "k", "kernel", "calls", "avg_us", "min_us", "max_us"])
    for d in sorted(glob.glob(prefix + "*")):
        form, hw, k = os.path.basename(d)[len(os.path.basename(prefix)):].split("_")
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f)) if "conv" in r["Name"]]
        # the kernel the plan runs is the most-called one; the dense form's tactic timer also launches its other candidates a few times each
        r = max(rows, key=lambda r: int(r["Calls"]))
        out.writerow([form, hw, k, r["Name"], r["Calls"], round(float(r["AverageNs"]) / 1e3, 2), round(float(r["MinNs"]) / 1e3, 2), round(float(r["MaxNs"]) / 1e3, 2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--levels", default="80,40,20")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ks", default="3,1")
    ap.add_argument("--only", choices=("grouped", "direct", "dense"), help="run this form alone and time nothing: the process to put under a kernel trace")
    ap.add_argument("--gather", metavar="DIR_PREFIX", help="print one CSV: the layer kernel's row of each kernel-stats file under DIR_PREFIX*")
    a = ap.parse_args()
    if a.gather:
        return gather(a.gather)
    C, G = a.channels, a.groups
    dev = torch.device("cuda:0")
    for hw in [int(v) for v in a.levels.split(",")]:
        x = torch.randn(a.batch * C * hw * hw, device=dev)
        for k in [int(v) for v in a.ks.split(",")]:
            if a.only:   # per-kernel times come from the profiler's own records of this process
                e = build(hw, k, a.layers, a.only, a.batch, C, G)
                time_engine(e, x, a.batch, a.steps, a.warmup)
                e.close()
                continue
            row = {"cin": C, "cout": C, "groups": G, "hw": hw, "k": k, "batch": a.batch, "layers": a.layers, "byte_floor_us": round(a.batch * hw * hw * C * 2 * 2 / 6.29e12 * 1e6, 2)}
            engines = {"empty": build(hw, k, 0, "grouped", a.batch, C, G)}
            for form in ("grouped", "direct", "dense"):
                engines[form] = build(hw, k, a.layers, form, a.batch, C, G)
            for rep in range(a.repeats):   # the forms alternate inside a repeat: same box, same minute
                t = {f: time_engine(e, x, a.batch, a.steps, a.warmup) for f, e in engines.items()}
                for form in ("grouped", "direct", "dense"):
                    row.setdefault(form + "_us_per_layer", []).append(round((t[form] - t["empty"]) / a.layers, 2))
                row.setdefault("empty_us", []).append(round(t["empty"], 2))
            for e in engines.values():
                e.close()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
