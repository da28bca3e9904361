"""Convolutions over unaligned channel views: the table of tests/test_gpu_conv_view.py (kernels/conv_view.hip, and the direct kernel under TRTX_CONV_VIEW=0).
Reference and bound as in tests/conv_grouped_cases.py: torch fp64 on fp16-grid inputs and weights, per element under tests/layer_cases.py's
fp32_bound(Out) + fp16_walk(1 site) with k * k * Cin + 2 terms (products, bias, shortcut) and ONE fp16 site, the store.  SiLU (slope <= 1.0998) carries
the fp32 part as Out.amp = 0.1 x that part; LeakyReLU (slope 0.1f, multiplied in float32 by the reference too) adds one term."""
import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from tests import layer_cases as lc
from tests.parity import fp16_walk


@dataclass(frozen=True)
class VCase:
    name: str
    Cin: int
    Cout: int
    k: int
    H: int
    W: int
    N: int
    in_view: tuple            # (channel offset, channels of the wider input): every case reads a view, or the implicit-GEMM family would take it
    act: str = "silu"
    out_view: tuple = None    # (channel offset, channels of the concat buffer); the neighbour's channels lie in front
    res_view: tuple = None    # (channel offset, channels of the wider tensor the shortcut is a slice of)


CASES = [
    VCase("c60_3x3", 60, 60, 3, 5, 7, 2, (60, 120)),              # 8-byte granule, last k-step 28 of 32 live; map smaller than a tile
    VCase("c60_1x1", 60, 60, 1, 13, 17, 3, (60, 120)),            # ... 1x1, ragged last tile
    VCase("c90_3x3", 90, 90, 3, 13, 17, 3, (90, 180)),            # 4-byte granule, offset 180 bytes, ragged tiles on both axes
    VCase("c90_1x1", 90, 90, 1, 5, 7, 2, (90, 180), act="none"),  # ... 1x1, bias only
    VCase("c180_to90_1x1", 180, 90, 1, 13, 17, 3, (180, 360)),    # six k-steps per tap; a 6-fragment block with 6 dead columns
    VCase("c180_3x3", 180, 180, 3, 13, 17, 2, (180, 360)),        # two column blocks
    VCase("c6_3x3", 6, 60, 3, 13, 17, 2, (6, 12)),                # less than one k-step per tap
    VCase("c34_1x1", 34, 60, 1, 13, 17, 2, (34, 68), act="leaky"),   # one k-step plus one granule; LeakyReLU
    VCase("out_at_60", 60, 60, 3, 13, 17, 2, (60, 120), out_view=(60, 120)),   # output view at an unaligned offset of a concat buffer
    VCase("cout18", 60, 18, 3, 5, 7, 2, (60, 120)),               # one full fragment plus a fragment with 2 live columns
    VCase("res_at_90", 90, 90, 3, 13, 17, 2, (90, 180), res_view=(90, 180)),   # shortcut that is itself a view at offset 90
    VCase("map_2x2", 90, 90, 3, 2, 2, 3, (90, 180)),              # map smaller than the filter
]
BY_NAME = {c.name: c for c in CASES}
LEAKY_ALPHA = 0.1
_REF = {}


def gen(case):
    """{x [N, in total, H, W], w KCRS, b [Cout], r [N, res total, H, W] | None, z [N, out offset, H, W] | None}: fp32 numpy, all but b on the fp16 grid"""
    def grid(what, shape, scale=1.0):
        rng = np.random.default_rng(zlib.crc32((case.name + "/" + what).encode()))
        return (rng.standard_normal(shape) * scale).astype(np.float16).astype(np.float32)
    hw = (case.H, case.W)
    return {"x": grid("x", (case.N, case.in_view[1]) + hw), "w": grid("w", (case.Cout, case.Cin, case.k, case.k), 1 / math.sqrt(case.k * case.k * case.Cin)),
            "b": np.random.default_rng(zlib.crc32((case.name + "/b").encode())).standard_normal(case.Cout).astype(np.float32),
            "r": grid("r", (case.N, case.res_view[1]) + hw) if case.res_view else None,
            "z": grid("z", (case.N, case.out_view[0]) + hw) if case.out_view else None}


def reference(case):
    """(y fp64 [N, Cout, H, W], per-element bound); computed once per case"""
    if case.name not in _REF:
        d = gen(case)
        x = torch.from_numpy(d["x"]).double()[:, case.in_view[0]:case.in_view[0] + case.Cin]
        w, b = torch.from_numpy(d["w"]).double(), torch.from_numpy(d["b"]).double()
        z = F.conv2d(x, w, b, 1, case.k // 2)
        mag = F.conv2d(x.abs(), w.abs(), b.abs(), 1, case.k // 2)
        n = case.k * case.k * case.Cin + 2 + (case.act == "leaky")
        y = {"silu": z * torch.sigmoid(z), "none": z, "leaky": torch.where(z > 0, z, z * float(np.float32(LEAKY_ALPHA)))}[case.act]
        amp = 0.1 * (1e-5 + n * lc.U32) if case.act == "silu" else 0.0
        if case.res_view:
            r = torch.from_numpy(d["r"]).double()[:, case.res_view[0]:case.res_view[0] + case.Cout]
            y, mag = y + r, mag + r.abs()
        o = lc.Out(y, mag, n=n, amp=amp, sites=1)
        _REF[case.name] = (y, lc.fp32_bound(o) + fp16_walk(o.sites, o.mag))
    return _REF[case.name]


def build_plan(case):
    """(plan, its one lowered convolution): inputs through the exact 1x1 pool into NHWC (tests/layer_cases.py nhwc), a channel slice, conv (+ Sigmoid x
    Prod | Leaky) (+ a sliced shortcut), optionally written into a concat buffer behind the neighbour's channels"""
    from tensorrtx_amd import builder, engine
    d = gen(case)
    net = builder.Network(max_batch=case.N, fp16=True)
    try:
        hw = (case.H, case.W)
        x = lc.nhwc(net, net.input("x", (case.in_view[1],) + hw))
        x = net.out(net.slice_channels(x, case.in_view[0], case.Cin, (case.in_view[1],) + hw))
        y = net.out(net.conv(x, d["w"], d["b"], 1, case.k // 2))
        if case.act == "silu":
            y = net.out(net.elementwise(y, net.out(net.activation(y, "sigmoid")), "prod"))
        elif case.act == "leaky":
            y = net.out(net.activation(y, "leaky", LEAKY_ALPHA))
        if case.res_view:
            r = lc.nhwc(net, net.input("r", (case.res_view[1],) + hw))
            y = net.out(net.elementwise(y, net.out(net.slice_channels(r, case.res_view[0], case.Cout, (case.res_view[1],) + hw)), "sum"))
        if case.out_view:
            y = net.out(net.concat([lc.nhwc(net, net.input("z", (case.out_view[0],) + hw)), y]))
        net.mark_output(y, "y")
        plan = net.build()
    finally:
        net.close()
    (conv,) = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "conv"]
    return plan, conv
