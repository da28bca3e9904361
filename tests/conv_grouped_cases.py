"""The grouped-convolution table shared by tests/test_conv_grouped_cpu.py (lowering, packing) and tests/test_gpu_conv_grouped.py (the kernel of
kernels/conv_grouped.hip through the C ABI and through engines, and the direct kernel under TRTX_CONV_GROUPED=0).

Reference and bound: torch fp64 on the fp16-rounded inputs with fp16-rounded weights, per element under the bound of tests/layer_cases.py:
fp32_bound(Out) + fp16_walk(1 site) with 9 * Cin_g + 2 terms (k * k * Cin_g products, the bias, the shortcut) and ONE fp16 site, the store of
the fused result.  The weights are GENERATED on the fp16 grid, so that the MFMA kernel (fp16 weights) and the direct kernel (fp32 weights) multiply
the same numbers and one reference serves both.  SiLU has a slope of at most 1.0998, so the fp32 part of the bound, an error of SiLU's argument, is
carried as Out.amp = 0.1 x that part; |SiLU(z)| <= |z| keeps the magnitude.  LeakyReLU (slope 0.1f, the C ABI's and the builder's alpha here) has a
slope of at most 1 and |leaky(z)| <= |z|: the bound of its argument holds for it, with one more term for the product z * 0.1f; the reference multiplies
by the same float32 slope."""
import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from tests import layer_cases as lc
from tests.parity import fp16_walk


@dataclass(frozen=True)
class GCase:
    name: str
    Cin: int
    Cout: int
    groups: int
    k: int
    H: int
    W: int
    N: int
    act: str = "silu"
    res: bool = False
    in_view: tuple = None    # (channel offset, channels of the wider input tensor)
    out_view: tuple = None   # (channel offset, channels of the wider output tensor)
    what: str = ""

    @property
    def pad(self):
        return self.k // 2

    @property
    def cin_g(self):
        return self.Cin // self.groups


CASES = [
    GCase("g4_3x3_5x7", 64, 64, 4, 3, 5, 7, 2, what="map smaller than a tile, borders on every side"),
    GCase("g4_3x3_13x17", 64, 64, 4, 3, 13, 17, 3, what="ragged last tile"),
    GCase("g4_1x1_13x17", 64, 64, 4, 1, 13, 17, 3, act="none", what="1x1 form, bias, no activation"),
    GCase("g4_3x3_64to128", 64, 128, 4, 3, 13, 17, 3, what="16 -> 32 per group"),
    GCase("g2_3x3_32per", 64, 64, 2, 3, 13, 17, 3, what="32 -> 32 per group, one tap per step"),
    GCase("g2_3x3_64per", 128, 128, 2, 3, 20, 20, 2, what="64 per group"),
    GCase("g4_3x3_inview", 64, 64, 4, 3, 13, 17, 3, in_view=(64, 128), what="input is a channel-offset view at offset 64 of a 128-channel tensor"),
    GCase("g4_3x3_outview", 64, 64, 4, 3, 13, 17, 3, out_view=(0, 144), what="output goes into channels [0, 64) of a 144-wide tensor"),
    GCase("g4_3x3_res", 64, 64, 4, 3, 13, 17, 3, res=True, what="residual add"),
]
# One case per remaining instantiation <taps, Cin_g / 16, units per wave> the lowering can select (conv_grouped.hip, GR_CASE), so that every form
# a user layer can reach has run on a device.  9 x 19 x 2: two tile columns and three tile rows (3x3) or six 64-pixel tiles (1x1), the last ragged.
PATH_CASES = [
    GCase("g2_3x3_32to64", 64, 128, 2, 3, 9, 19, 2, what="<9, 2, 2>: 32 per group, two units per wave"),
    GCase("g2_3x3_48to16", 96, 32, 2, 3, 9, 19, 2, what="<9, 3, 1>: 48 per group, k-steps straddle taps, two of four waves idle"),
    GCase("g2_3x3_48per", 96, 96, 2, 3, 9, 19, 2, what="<9, 3, 2>: 48 per group, six units on four waves"),
    GCase("g2_3x3_64to32", 128, 64, 2, 3, 9, 19, 2, what="<9, 4, 1>: 64 per group, one unit per wave"),
    GCase("g3_3x3_192to96", 192, 96, 3, 3, 9, 19, 2, res=True, what="<9, 4, 2> with 53.5 KB of LDS (above 48 KB), residual"),
    GCase("g4_1x1_64to128", 64, 128, 4, 1, 9, 19, 2, what="<1, 1, 2>"),
    GCase("g2_1x1_32per", 64, 64, 2, 1, 9, 19, 2, what="<1, 2, 1>"),
    GCase("g2_1x1_32to64", 64, 128, 2, 1, 9, 19, 2, res=True, what="<1, 2, 2>, residual"),
    GCase("g2_1x1_48to16", 96, 32, 2, 1, 9, 19, 2, what="<1, 3, 1>: K = 48, the second k-step half live"),
    GCase("g2_1x1_48per", 96, 96, 2, 1, 9, 19, 2, what="<1, 3, 2>"),
    GCase("g2_1x1_64to32", 128, 64, 2, 1, 9, 19, 2, what="<1, 4, 1>"),
    GCase("g2_1x1_64per", 128, 128, 2, 1, 9, 19, 2, what="<1, 4, 2>"),
]
# A rare activation kind (the out-of-line branch of the kernel's activation) on both forms, at the shape of the path cases.
RARE_ACT_CASES = [
    GCase("g4_3x3_leaky", 64, 64, 4, 3, 9, 19, 2, act="leaky", what="<9, 1, 1>, LeakyReLU 0.1"),
    GCase("g4_1x1_leaky", 64, 64, 4, 1, 9, 19, 2, act="leaky", what="<1, 1, 1>, LeakyReLU 0.1"),
]
LEAKY_ALPHA = 0.1
ISSUE_CASES = list(CASES)
CASES = CASES + PATH_CASES + RARE_ACT_CASES
BY_NAME = {c.name: c for c in CASES}


def _rng(case, what):
    return np.random.default_rng(zlib.crc32((case.name + "/" + what).encode()))


def _on_f16_grid(a):
    return a.astype(np.float16).astype(np.float32)


def gen(case):
    """{x [N, Cin_total, H, W], w KCRS, b [Cout], r [N, Cout, H, W] or None, z [N, out_total - Cout, H, W] or None}: fp32 numpy, x / w / r / z on
    the fp16 grid.  x holds the channels of the whole (wider) input tensor when the case reads a view."""
    cin_total = case.in_view[1] if case.in_view else case.Cin
    d = {"x": _on_f16_grid(_rng(case, "x").standard_normal((case.N, cin_total, case.H, case.W))),
         "w": _on_f16_grid(_rng(case, "w").standard_normal((case.Cout, case.cin_g, case.k, case.k)) / math.sqrt(case.k * case.k * case.cin_g)),
         "b": _rng(case, "b").standard_normal(case.Cout).astype(np.float32), "r": None, "z": None}
    if case.res:
        d["r"] = _on_f16_grid(_rng(case, "r").standard_normal((case.N, case.Cout, case.H, case.W)))
    if case.out_view:
        d["z"] = _on_f16_grid(_rng(case, "z").standard_normal((case.N, case.out_view[1] - case.Cout, case.H, case.W)))
    return d


_REF = {}


def reference(case):
    """(y fp64 [N, Cout, H, W], per-element bound); computed once per case"""
    if case.name not in _REF:
        d = gen(case)
        x = torch.from_numpy(d["x"]).double()
        if case.in_view:
            x = x[:, case.in_view[0]:case.in_view[0] + case.Cin]
        w, b = torch.from_numpy(d["w"]).double(), torch.from_numpy(d["b"]).double()
        z = F.conv2d(x, w, b, 1, case.pad, 1, case.groups)
        mag = F.conv2d(x.abs(), w.abs(), b.abs(), 1, case.pad, 1, case.groups)
        n = case.k * case.k * case.cin_g + 2 + (case.act == "leaky")
        y = z * torch.sigmoid(z) if case.act == "silu" else z
        if case.act == "leaky":
            y = torch.where(z > 0, z, z * float(np.float32(LEAKY_ALPHA)))
        amp = 0.1 * (1e-5 + n * lc.U32) if case.act == "silu" else 0.0
        if case.res:
            r = torch.from_numpy(d["r"]).double()
            y, mag = y + r, mag + r.abs()
        o = lc.Out(y, mag, n=n, amp=amp, sites=1)
        _REF[case.name] = (y, lc.fp32_bound(o) + fp16_walk(o.sites, o.mag))
    return _REF[case.name]


def build_plan(case, fp16=True, max_batch=None):
    """the layer as a network: inputs through the exact 1x1 pool into NHWC (tests/layer_cases.py nhwc), conv (+ Sigmoid x Prod) (+ shortcut),
    optionally read from a channel slice / written into a concat buffer"""
    from tensorrtx_amd import builder
    d = gen(case)
    net = builder.Network(max_batch=max_batch or case.N, fp16=bool(fp16))
    try:
        cin_total = case.in_view[1] if case.in_view else case.Cin
        x = lc.nhwc(net, net.input("x", (cin_total, case.H, case.W)))
        if case.in_view:
            x = net.out(net.slice_channels(x, case.in_view[0], case.Cin, (cin_total, case.H, case.W)))
        y = net.out(net.conv(x, d["w"], d["b"], 1, case.pad, groups=case.groups))
        if case.act == "silu":
            y = net.out(net.elementwise(y, net.out(net.activation(y, "sigmoid")), "prod"))
        elif case.act == "leaky":
            y = net.out(net.activation(y, "leaky", LEAKY_ALPHA))
        if case.res:
            y = net.out(net.elementwise(y, lc.nhwc(net, net.input("r", (case.Cout, case.H, case.W))), "sum"))
        if case.out_view:
            y = net.out(net.concat([y, lc.nhwc(net, net.input("z", (case.out_view[1] - case.Cout, case.H, case.W)))]))
        net.mark_output(y, "y")
        return net.build()
    finally:
        net.close()


def convs_of(plan):
    from tensorrtx_amd import engine
    return [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "conv"]
