"""The convolution geometry table: single convolutions for the MFMA kernels (kernels/igemm_tile.h behind conv_igemm.hip - fp16 and int8 -,
conv_igemm_f32.hip, and the special-case kernels conv_ws / conv_res / the resident patch that the tactic lists name), shared by
tests/test_conv_cases_cpu.py (acceptance, coverage, conditioning of the references) and tests/test_gpu_conv_geometry.py (the kernels through
the C ABI).  The launchers accept any kh x kw up to 30 taps, any stride pair, any padding pair; this table is where that surface is walked:
rectangular and even kernels, the 30-tap limit, a k-step window that is rebuilt, strides that differ per axis or exceed the kernel, no padding,
one-sided padding, padding beyond k / 2 and beyond k (whole output rows without a valid tap), maps smaller than the filter, and the channel
counts that change the path through the gather (two taps per k-step, ragged chunks, both k-step widths) and through the epilogue (padded column
tiles, element-wise stores).  The axes are crossed with each other rather than tried once each.

Every case is small: N * Ho * Wo between about 130 and 1000 rows (more than one 128-row tile and a ragged last one); the degenerate maps are
smaller by nature.  Data is seeded by the case name (zlib.crc32, as in tests/layer_cases.py).

References are torch fp64 on the operands as the engine stores them, with the per-element error model of tests/test_gpu_layers.py:
    |err| <= fp32_bound(n, mag) + fp16_walk(sites, mag)
  * mag: the same convolution on absolute values (+ |bias|, + |shortcut|) - every activation used here has |act(v)| <= |v|;
  * fp16: operands x.half(), w.half(), fp32 bias; n = kh * kw * Cin + 2 (the products, the bias, the shortcut); sites = 1 (the fp16 store), 2 with a
    shortcut (the kernel rounds to fp16 before the add and after it);
  * fp32: n the same, no fp16 site;
  * int8: the accumulator is an exact integer (int32 on the device, fp64 here), so the fp32 arithmetic is what follows it - accumulator * scale, + bias,
    the activation: n = 3 - and the fp16 sites are those of the fp16 engine.  With int8 output the final rounding is written out in the reference
    (round(half(y) / s_out)), so it is no site: an element may differ by one step only where moving the fp64 value by +- fp32_bound(3, mag) changes that
    rounding; the share of such elements is a property of the reference and is capped at 2 % by the host test."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from tests.layer_cases import Out, fp32_bound
from tests.parity import fp16_walk

S_IN, S_RES = 0.02, 0.05     # int8: the input tensor's scale (the existing int8 test's)
I8_NEAR_CAP = 0.02           # the project's cap on requantised values that may sit on a rounding boundary (tests/test_gpu_int8.py)


@dataclass(frozen=True)
class ConvCase:
    name: str
    N: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: tuple
    s: tuple
    p: tuple
    act1: str = "none"
    res: bool = False
    act2: str = "none"
    engines: tuple = ("f16", "f32")
    degenerate: bool = False   # a map smaller than the filter / a single row, column or pixel: exempt from the row-count rule

    @property
    def out_hw(self):
        return (self.H + 2 * self.p[0] - self.k[0]) // self.s[0] + 1, (self.W + 2 * self.p[1] - self.k[1]) // self.s[1] + 1

    @property
    def rows(self):
        return self.N * self.out_hw[0] * self.out_hw[1]

    @property
    def taps(self):
        return self.k[0] * self.k[1]


CASES = []


def add(name, N, H, W, Cin, Cout, k, s=1, p=0, act1="none", res=False, act2="none", engines=("f16", "f32"), degenerate=False):
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)  # noqa: E731
    c = ConvCase(name, N, H, W, Cin, Cout, pair(k), pair(s), pair(p), act1, res, act2, tuple(engines), degenerate)
    assert all(o.name != name for o in CASES), name
    CASES.append(c)


ALL = ("f16", "f32", "i8")
# ---- kernel shape (x channels x epilogue) ------------------------------------------------------------------------------------------------------------
add("k1x3_c16_o16", 2, 9, 11, 16, 16, (1, 3), 1, (0, 1), "silu", engines=ALL)                 # Cin 16, 3 taps: two taps per k-step, odd count
add("k3x1_c24_o40_leaky", 2, 13, 9, 24, 40, (3, 1), 1, (1, 0), "leaky")                        # ragged chunk, padded column tile, the slow activation
add("k1x7_p0_c48_o21", 1, 10, 23, 48, 21, (1, 7), 1, 0, "relu")                                # no padding under a 1x7, element-wise stores
add("k7x1_c64_o80_res", 1, 15, 10, 64, 80, (7, 1), 1, (3, 0), "none", True, "relu", engines=ALL)   # rectangular + shortcut + second activation
add("k3x5_c160_o128", 1, 12, 12, 160, 128, (3, 5), 1, (1, 2), "silu")                          # 75 k-steps of 32: the 64-step window is rebuilt
add("k5x3_s2x1_c80_o8", 1, 24, 12, 80, 8, (5, 3), (2, 1), (2, 1))                              # stride (2, 1), Cin 80 (2.5 steps per tap), Cout 8
add("k5x6_c32_o64", 1, 12, 14, 32, 64, (5, 6), 1, (2, 2), "silu", engines=ALL)                 # 30 taps: the limit of the tap mask
add("k5x6_c128_o16_s1x2", 2, 10, 21, 128, 16, (5, 6), (1, 2), (2, 3), "relu")                  # ... with 64-wide k-steps possible and a stride pair
add("k2x2_s2_c128_o16", 2, 18, 20, 128, 16, (2, 2), 2, 0, "relu", engines=ALL)                 # even kernel, stride = kernel
add("k4x4_s1x2_p1x2_c8_o40", 2, 12, 21, 8, 40, (4, 4), (1, 2), (1, 2), "silu")                 # even kernel, stride (1, 2), padding (1, 2), Cin 8
add("k3x5_s2x1_c4_o16", 2, 20, 12, 4, 16, (3, 5), (2, 1), (1, 2), "silu", engines=("f32",))    # fp32 Cin 4: two taps per 16-float step, 15 taps
add("k1x3_c8_o32", 1, 10, 17, 8, 32, (1, 3), 1, (0, 1), "none")                                # fp32 Cin 8 rectangular; fp16 Cin 8 -> CinK 16
add("k5x5_c16_o128_res", 1, 13, 11, 16, 128, (5, 5), 1, 2, "silu", True)                       # Cin 16, 25 taps: the last k-step holds one tap
# ---- stride ------------------------------------------------------------------------------------------------------------------------------------------
add("k3x3_s3_c64_o64_res", 2, 26, 29, 64, 64, (3, 3), 3, 1, "relu", True, "relu", engines=ALL)  # stride 3 + shortcut + second activation
add("k1x1_s2_c64_o128", 2, 17, 19, 64, 128, (1, 1), 2, 0, engines=ALL)                         # the ResNet shortcut: stride beyond the kernel
add("k2x3_s3x4_c48_o80", 3, 20, 30, 48, 80, (2, 3), (3, 4), (0, 1), "silu", engines=ALL)       # stride beyond the kernel on both axes, differently
add("k3x1_s1x2_c128_o21", 1, 12, 30, 128, 21, (3, 1), (1, 2), (1, 0), "relu")                  # stride (1, 2) under a one-column filter
# ---- padding -----------------------------------------------------------------------------------------------------------------------------------------
add("k3x3_p0_c24_o16", 2, 12, 14, 24, 16, (3, 3), 1, 0, "relu")
add("k1x7_p0x3_c128_o40_res", 1, 8, 20, 128, 40, (1, 7), 1, (0, 3), "none", True, "relu", engines=ALL)   # 1x7 with a shortcut
add("k7x1_p3x0_c16_o8", 2, 11, 9, 16, 8, (7, 1), 1, (3, 0), "silu")                             # Cin 16, 7 taps, Cout 8
add("k3x3_p1x2_c48_o128", 1, 12, 11, 48, 128, (3, 3), 1, (1, 2), "silu")                        # padding (1, 2): the map grows along W only
add("k3x3_p2_c64_o16", 1, 10, 12, 64, 16, (3, 3), 1, 2, "silu", engines=ALL)                    # border rows and columns see one tap row / column only
add("k1x1_p1_c64_o64", 1, 10, 13, 64, 64, (1, 1), 1, 1, "relu", engines=ALL)                    # the border has no valid tap: act(bias); not a plain GEMM
add("k3x3_p3_c32_o80", 1, 8, 9, 32, 80, (3, 3), 1, 3)                                           # ... two border rows / columns are act(bias), here the bias itself
add("k1x3_p2x0_s2_c80_o40", 2, 9, 25, 80, 40, (1, 3), 2, (2, 0), "leaky")                       # padding beyond k along H under stride 2: whole rows of bias
# ---- maps smaller than the filter or degenerate: every 3x3 s1 p1 tactic ---------------------------------------------------------------------------------
add("deg_1x9_c64_o64", 1, 1, 9, 64, 64, (3, 3), 1, 1, "silu", degenerate=True)
add("deg_9x1_c32_o32", 1, 9, 1, 32, 32, (3, 3), 1, 1, "relu", degenerate=True)
add("deg_1x1_n5_c64_o80", 5, 1, 1, 64, 80, (3, 3), 1, 1, "silu", degenerate=True)
add("deg_1x16_c16_o16", 1, 1, 16, 16, 16, (3, 3), 1, 1, "silu", True, degenerate=True)
add("deg_3x2_c64_o64_res", 1, 3, 2, 64, 64, (3, 3), 1, 1, "silu", True, "relu", degenerate=True)
add("deg_2x3_c128_o128", 2, 2, 3, 128, 128, (3, 3), 1, 1, "none", degenerate=True, engines=ALL)
add("deg_1x16_n1024_c32_o32", 1024, 1, 16, 32, 32, (3, 3), 1, 1, "silu", degenerate=True)     # the weight-stationary kernel (ws 2) is listed from 1024 tiles on: one row each
add("deg_2x2_k5x6_c32_o32", 3, 2, 2, 32, 32, (5, 6), 1, (2, 3), "relu", degenerate=True)       # a 30-tap filter over a 2x2 map

# the launch families (fp16: ws of a tactic; fp32: the operand path of a tile) the degenerate 3x3 s1 p1 maps are in the table for, spelled out per map.
# The host test demands them of the lists at an aligned slice, the device test of what it actually forced.  1: the implicit-GEMM tile; 2: weight-stationary
# (conv_ws.hip: Cin 32, Cout <= 32, rows of 16 pixels, 1024 tiles and more - hence the batch of 1024); 3: the resident patch (fp16: Cout a multiple of 64 / 80 /
# 128); 7: the resident-operand 3x3 kernel (conv_res.hip's shape table); 8: its thin two-tap form (Cin 16, whole 16-pixel rows)
EXPECT_WS = {
    "deg_1x9_c64_o64": {"f16": {1, 3, 7}, "f32": {1, 3, 7}},
    "deg_9x1_c32_o32": {"f16": {1, 7}, "f32": {1, 3, 7}},
    "deg_1x1_n5_c64_o80": {"f16": {1, 3, 7}, "f32": {1, 3, 7}},
    "deg_1x16_c16_o16": {"f16": {1, 8}, "f32": {1, 3, 7}},
    "deg_3x2_c64_o64_res": {"f16": {1, 3, 7}, "f32": {1, 3, 7}},
    "deg_2x3_c128_o128": {"f16": {1, 3}, "f32": {1, 3}},
    "deg_1x16_n1024_c32_o32": {"f16": {1, 2, 7}, "f32": {1, 3, 7}},
}

BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

# the axis values every engine type must see (tests/test_conv_cases_cpu.py); fp16 takes Cin % 8 == 0 only, so Cin 4 is an fp32 axis
AXES = {
    "k": [(1, 3), (3, 1), (1, 7), (7, 1), (3, 5), (5, 3), (5, 6), (2, 2), (4, 4)],
    "s": [(2, 1), (1, 2), (3, 3)],
    "p": [(0, 3), (3, 0), (1, 2), (2, 2)],
    "Cin": [16, 24, 48, 80, 64, 128, 8],
    "Cout": [8, 16, 21, 40, 80, 128],
}

ACT = {"none": lambda t: t, "relu": torch.relu, "silu": F.silu, "leaky": lambda t: F.leaky_relu(t, 0.1)}


def _rng(case, what):
    return np.random.default_rng(zlib.crc32((case.name + "/" + what).encode()))


@functools.lru_cache(maxsize=None)
def gen_inputs(name):
    """{x [N, H, W, Cin], w [Cout, Cin, kh, kw] (He-scaled), bias [Cout], res [N, Ho, Wo, Cout], xq: the int8 engine's input}, fp32 / int32 torch"""
    c = BY_NAME[name]
    Ho, Wo = c.out_hw
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return dict(x=t(_rng(c, "x").standard_normal((c.N, c.H, c.W, c.Cin))),
                w=t(_rng(c, "w").standard_normal((c.Cout, c.Cin, *c.k)) * (2.0 / (c.Cin * c.taps)) ** 0.5),
                bias=t(_rng(c, "bias").standard_normal(c.Cout) * 0.5),
                res=t(_rng(c, "res").standard_normal((c.N, Ho, Wo, c.Cout))),
                xq=torch.from_numpy(_rng(c, "xq").integers(-127, 128, (c.N, c.H, c.W, c.Cin)).astype(np.int32)))


def quantise_weights(w):
    """per-output-channel symmetric int8 weights, restated independently of the packer: (integers as fp64, scales)"""
    amax = w.abs().reshape(w.shape[0], -1).max(1).values
    sw = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    return torch.clamp(torch.round(w / sw[:, None, None, None]), -127, 127).double(), sw


def operands(case, engine):
    """(x NCHW, w, bias, res NCHW or None) in fp64, as the engine stores them; int8: x and w in real units (integers times their scales)"""
    d = gen_inputs(case.name)
    res = d["res"].permute(0, 3, 1, 2) if case.res else None
    if engine == "f16":
        return d["x"].half().double().permute(0, 3, 1, 2), d["w"].half().double(), d["bias"].double(), None if res is None else res.half().double()
    if engine == "f32":
        return d["x"].double().permute(0, 3, 1, 2), d["w"].double(), d["bias"].double(), None if res is None else res.double()
    wq, sw = quantise_weights(d["w"])
    cscale = (torch.tensor(S_IN, dtype=torch.float32) * sw).double()   # the fp32 product the kernel is handed
    return d["xq"].double().permute(0, 3, 1, 2), wq * cscale[:, None, None, None], d["bias"].double(), None if res is None else res.half().double()


def _conv(case, x, w, b):
    return F.conv2d(x, w, b, case.s, case.p)


@dataclass
class Ref:
    y: torch.Tensor        # [N, Ho, Wo, Cout] fp64
    mag: torch.Tensor
    bound: torch.Tensor    # the per-element bound of a floating-point output
    pre: torch.Tensor      # the convolution in front of the activation (NCHW)
    n: int
    sites: int


@functools.lru_cache(maxsize=None)
def reference(name, engine):
    case = BY_NAME[name]
    x, w, b, res = operands(case, engine)
    pre = _conv(case, x, w, b)
    mag = _conv(case, x.abs(), w.abs(), b.abs())
    y = ACT[case.act1](pre)
    if res is not None:
        y, mag = y + res, mag + res.abs()
    y = ACT[case.act2](y)
    n = 3 if engine == "i8" else case.taps * case.Cin + 2
    sites = 0 if engine == "f32" else (2 if case.res else 1)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    y, mag = nhwc(y), nhwc(mag)
    return Ref(y, mag, bound_of(mag, n, sites), pre, n, sites)


def bound_of(mag, n, sites):
    """the layer suite's fp32 bound over n terms of magnitude mag, plus its fp16 walk over the storage sites"""
    return fp32_bound(Out(None, mag, n=n)) + (fp16_walk(sites, mag) if sites else 0.0)


def requantise(y, s_out):
    """what the int8 epilogue stores for the value y: round-to-nearest-even of half(y) * fp32(1 / s_out), clamped"""
    inv = float(np.float32(1.0 / s_out))
    return torch.clamp(torch.round(y.half().double() * inv), -127, 127)


def i8_out_scale(ref):
    return float(ref.y.abs().max()) / 127.0


def i8_expected(name):
    """(q, near, s_out) of an int8-output launch: the expected integers, and where +- the fp32 bound around the fp64 value changes them"""
    ref = reference(name, "i8")
    assert ref.sites == 1, "int8-output cases carry no shortcut (its fp16 rounding in front of the add would be a site the reference cannot write out)"
    s_out = i8_out_scale(ref)
    b = bound_of(ref.mag, ref.n, 0)
    q = requantise(ref.y, s_out)
    near = (requantise(ref.y - b, s_out) != q) | (requantise(ref.y + b, s_out) != q)
    return q, near, s_out


def tap_share(name, engine):
    """per filter tap (r, q): the share of outputs, among those where the tap lies inside the image, at which the tap's own contribution to the sum
    exceeds the element's bound - what a kernel that dropped, doubled or misplaced that tap would have to get past.  {(r, q): share}"""
    case = BY_NAME[name]
    x, w, _, _ = operands(case, engine)
    ref = reference(name, engine)
    bound = ref.bound.permute(0, 3, 1, 2)
    ones = torch.ones(1, 1, case.H, case.W, dtype=torch.float64)
    out = {}
    for r in range(case.k[0]):
        for q in range(case.k[1]):
            w1 = torch.zeros_like(w)
            w1[:, :, r, q] = w[:, :, r, q]
            m1 = torch.zeros(1, 1, *case.k, dtype=torch.float64)
            m1[0, 0, r, q] = 1.0
            inside = _conv(case, ones, m1, None)[0, 0] > 0.5   # [Ho, Wo]
            if not inside.any():
                continue
            contrib = _conv(case, x, w1, None).abs()
            out[(r, q)] = float((contrib > bound)[:, :, inside].double().mean())
    return out
