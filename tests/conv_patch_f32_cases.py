"""Grouped and channel-view convolutions of fp32 engines: the table of tests/test_conv_patch_f32_cpu.py and tests/test_gpu_conv_patch_f32.py
(kernels/conv_patch_f32.hip under TRTX_CONV_F32_PATCH=1, and the direct kernel with the switch unset).

Reference and bound: torch fp64 conv2d on ordinary fp32 values (no fp16 site), per element under tests/layer_cases.py's fp32_bound with k * k * Cin_g + 2
terms (products, bias, shortcut), nothing fitted.  SiLU (slope <= 1.0998, |SiLU(z)| <= |z|) carries its argument's bound as Out.amp = 0.1 x that part; LeakyReLU
(0.1f, multiplied in float32 by the reference too) adds one term.  `what` names the instantiation <taps; pixel, column fragments per wave>: all eight are reached."""
import collections
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import layer_cases as lc


# in_view: (channel offset, channels of the wider input tensor); out_view: (channel offset, channels of the concat buffer), the neighbour's channels lie in
# front; res_view: (channel offset, channels of the tensor the shortcut is a slice of); stride / dil other than 1: only what the lowering must leave alone
PCase = collections.namedtuple("PCase", "name Cin Cout groups k H W N act in_view out_view res_view what stride dil", defaults=("silu", None, None, None, "", 1, 1))

CASES = [
    PCase("c90_3x3", 90, 90, 1, 3, 5, 7, 2, in_view=(90, 180), what="<9; 2, 3>: map smaller than a tile, every side a border, three chunks of 32"),
    PCase("c6_3x3", 6, 20, 1, 3, 9, 19, 2, in_view=(1, 9), what="<9; 2, 1>: everything odd, CinK 8: two taps per k-step, the last one half live"),
    PCase("c90_1x1", 90, 90, 1, 1, 9, 19, 2, in_view=(90, 180), what="<1; 2, 3>: ragged last 64-pixel tile, chunks of 64 and 32"),
    PCase("c144_1x1", 144, 56, 1, 1, 9, 19, 2, in_view=(2, 148), what="<1; 2, 2>: chunks 64 + 64 + 16, 16-byte loads ruled out by the offset alone"),
    PCase("c90_to180", 90, 180, 1, 3, 5, 7, 2, in_view=(90, 180), what="two column blocks of six fragments"),
    PCase("out_at_7", 6, 40, 1, 3, 13, 17, 2, in_view=(1, 9), out_view=(7, 47), what="<9; 2, 2>: element-wise stores, a dead fourth fragment"),
    PCase("res_at_3", 36, 24, 1, 3, 13, 17, 2, in_view=(2, 40), res_view=(3, 29), what="shortcut read from a view at an odd offset"),
    PCase("g4_3x3", 64, 64, 4, 3, 13, 17, 3, what="<9; 1, 1>: the DDetect shape, ragged last tile"),
    PCase("g4_1x1", 64, 64, 4, 1, 13, 17, 3, act="none", what="<1; 1, 1>: bias, no activation"),
    PCase("g2_20to32", 40, 64, 2, 3, 9, 19, 2, what="Cin_g 20: a multiple of 4 but not of 16, k-steps straddle taps, pitch 20"),
    PCase("g3_1x1", 48, 96, 3, 1, 9, 19, 2, what="<1; 2, 1>: 16 -> 32 per group"),
    PCase("g4_inview", 64, 64, 4, 3, 9, 19, 2, act="leaky", in_view=(3, 70), what="grouped input view at an odd offset: 4-byte loads; LeakyReLU"),
    PCase("g4_outview", 64, 64, 4, 1, 9, 19, 2, out_view=(5, 69), what="grouped output at an odd offset of a concat buffer: element-wise stores"),
    PCase("g2_64per_res", 128, 128, 2, 3, 9, 19, 2, res_view=(0, 128), what="<9; 2, 2> at 57 KB of LDS, 16-byte shortcut loads"),
]
BY_NAME = {c.name: c for c in CASES}
LEAKY_ALPHA = 0.1
_REF = {}


def gen(case):
    """{x [N, in total, H, W], w KCRS, b [Cout], r [N, res total, H, W] | None, z [N, out offset, H, W] | None}: fp32 numpy"""
    def rnd(what, shape, scale=1.0):
        rng = np.random.default_rng(zlib.crc32((case.name + "/" + what).encode()))
        return (rng.standard_normal(shape) * scale).astype(np.float32)
    hw, cg = (case.H, case.W), case.Cin // case.groups
    return {"x": rnd("x", (case.N, (case.in_view or (0, case.Cin))[1]) + hw), "w": rnd("w", (case.Cout, cg, case.k, case.k), 1 / math.sqrt(case.k * case.k * cg)),
            "b": rnd("b", (case.Cout,)), "r": rnd("r", (case.N, case.res_view[1]) + hw) if case.res_view else None,
            "z": rnd("z", (case.N, case.out_view[0]) + hw) if case.out_view else None}


def reference(case):
    """(y fp64 [N, Cout, H, W], per-element bound); computed once per case"""
    if case.name not in _REF:
        d = gen(case)
        x = torch.from_numpy(d["x"]).double()[:, (case.in_view or (0,))[0]:][:, :case.Cin]
        w, b = torch.from_numpy(d["w"]).double(), torch.from_numpy(d["b"]).double()
        z = F.conv2d(x, w, b, 1, case.k // 2, 1, case.groups)
        mag = F.conv2d(x.abs(), w.abs(), b.abs(), 1, case.k // 2, 1, case.groups)
        n = case.k * case.k * (case.Cin // case.groups) + 2 + (case.act == "leaky")
        y = {"silu": z * torch.sigmoid(z), "none": z, "leaky": torch.where(z > 0, z, z * float(np.float32(LEAKY_ALPHA)))}[case.act]
        amp = 0.1 * (1e-5 + n * lc.U32) if case.act == "silu" else 0.0
        if case.res_view:
            r = torch.from_numpy(d["r"]).double()[:, case.res_view[0]:case.res_view[0] + case.Cout]
            y, mag = y + r, mag + r.abs()
        _REF[case.name] = (y, lc.fp32_bound(lc.Out(y, mag, n=n, amp=amp)))
    return _REF[case.name]


def build_plan(case, fp16=False):
    """(plan, its lowered ops): inputs through the exact 1x1 pool into NHWC, a channel slice, conv (+ Sigmoid x Prod | Leaky) (+ a sliced shortcut) (+ concat)"""
    from tensorrtx_amd import builder, engine
    d = gen(case)
    net = builder.Network(max_batch=case.N, fp16=bool(fp16))
    try:
        hw = (case.H, case.W)
        cin_total = case.in_view[1] if case.in_view else case.Cin
        x = lc.nhwc(net, net.input("x", (cin_total,) + hw))
        if case.in_view:
            x = net.out(net.slice_channels(x, case.in_view[0], case.Cin, (cin_total,) + hw))
        y = net.out(net.conv(x, d["w"], d["b"], case.stride, case.dil * (case.k // 2), groups=case.groups, dilation=case.dil))
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
    return plan, engine.describe_plan(plan, lowered=True)["ops"]
