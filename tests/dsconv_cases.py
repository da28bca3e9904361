"""YOLOv13's DSConv (depthwise k x k -> 1x1 -> BatchNorm -> SiLU; kernels/conv_dw_pw.hip): the case table of tests/test_gpu_dsconv.py, its torch fp64
reference with the per-element bound, and the DSBottleneck network (yolov13/src/block.cpp:491-586) that tests/test_dsconv_cpu.py and the GPU test lower.

Reference: the depthwise convolution in fp64 on the fp16 input, ROUNDED to fp16 (the storage site between the halves: the kernel's LDS operand), the 1x1 in
fp64 on the fp16 weights, then bias, activation, residual, second activation in fp64.  Bound, per element, nothing fitted:
    2 u mag_pw                       the fp32 depthwise sum may fall on the other side of a rounding boundary: the operand is then the neighbouring fp16
                                     value, one ulp = 2 u |dw| away, on every channel at worst (u = 2^-11, mag_pw = sum |w_pw| |dw|)
  + fp32_bound(k^2 + Cin + 3, mag)   the conv table's fp32 model (its 1e-5 mag + 1e-7 floor included) over the depthwise and 1x1 terms, bias, residual
  + fp16_walk(1, mag)                the output rounding; mag = mag_pw + |bias| + |residual| (|act(v)| <= |v|)
An error bound on the INPUT (a bottleneck's second DSConv) goes through both halves on absolute weights, times 1.1 (SiLU's largest slope)."""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.layer_cases import Out, fp32_bound
from tests.parity import EPS16, fp16_walk

ACT = {"none": lambda v: v, "relu": torch.relu, "silu": lambda v: v * torch.sigmoid(v)}
Case = collections.namedtuple("Case", "name B H W cin cout k s act res act2 bias", defaults=("silu", False, "none", True))
CASES = {c.name: c for c in [
    Case("cin16_k3_ragged_tile", 1, 20, 19, 16, 16, 3, 1, res=True),               # less than one k-step; H and W no multiples of the 16 x 16 tile
    Case("cin40_cout24_s2_odd", 1, 9, 11, 40, 24, 3, 2),                          # a ragged k-step, a ragged column block, 9 x 11 -> 5 x 6
    Case("cin72_cout8_k5", 1, 10, 18, 72, 8, 5, 1, act="relu", bias=False),      # two k-steps and a ragged one; under one column block; no bias
    Case("cin32_cout136_passes", 1, 6, 17, 32, 136, 3, 1),                        # 16-row tile (Cin <= 128, over 4 rows): three passes of 64, ragged last block
    Case("cin136_cout264_passes", 1, 6, 17, 136, 264, 3, 1, res=True),            # 4-row tile: four k-steps and a ragged one, two passes of 256, ragged last block
    Case("k5_s2", 1, 13, 13, 24, 16, 5, 2, act="none"),
    Case("k7_map3x3", 2, 3, 3, 16, 16, 7, 1),                                     # a map smaller than the filter (4-row tile: 3 rows)
    Case("k7_s2_relu_res_relu", 1, 12, 21, 16, 32, 7, 2, act="relu", res=True, act2="relu"),
    Case("batch3", 3, 7, 9, 64, 64, 3, 1, res=True)]}                             # tiles never span images
out_hw = lambda H, W, k, s: ((H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1)  # noqa: E731
_rng = lambda *key: np.random.default_rng(zlib.crc32(repr(key).encode()))  # noqa: E731   (seeded by what the data is for)


def dsconv_ref(x, wd, wp, bias, k, s, act, res=None, act2="none", x_bound=None):
    """NCHW fp64 operands as the engine stores them -> (y, bound), NCHW fp64"""
    C = x.shape[1]
    dwc = lambda t, w: F.conv2d(t, w[:, None], None, s, k // 2, 1, C)  # noqa: E731
    pwc = lambda t, w: F.conv2d(t, w[:, :, None, None])  # noqa: E731
    a = dwc(x, wd).half().double()
    y = ACT[act](pwc(a, wp) + bias[None, :, None, None])
    mag_pw = pwc(a.abs(), wp.abs())
    mag = mag_pw + bias.abs()[None, :, None, None]
    if res is not None:
        y, mag = y + res, mag + res.abs()
    bound = 2 * EPS16 * mag_pw + fp32_bound(Out(None, mag, n=k * k + C + 3)) + fp16_walk(1, mag)
    if x_bound is not None:
        bound = bound + 1.1 * pwc(dwc(x_bound, wd.abs()), wp.abs())
    return ACT[act2](y), bound


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, y, bound) of a table case, once: x [B,H,W,Cin], wd [Cin,k,k], wp [Cout,Cin], bias, res or None, fp32, mixed sign; y and bound NHWC fp64"""
    c = CASES[name]
    t = lambda what, *shape: torch.from_numpy(_rng(name, what).standard_normal(shape).astype(np.float32))  # noqa: E731
    d = dict(x=t("x", c.B, c.H, c.W, c.cin), wd=t("wd", c.cin, c.k, c.k) / c.k, wp=t("wp", c.cout, c.cin) * (2.0 / c.cin) ** 0.5,
             bias=t("b", c.cout) * 0.5 if c.bias else None, res=t("r", c.B, *out_hw(c.H, c.W, c.k, c.s), c.cout) if c.res else None)
    nchw = lambda v: None if v is None else v.half().double().permute(0, 3, 1, 2)  # noqa: E731
    y, bound = dsconv_ref(nchw(d["x"]), d["wd"].double(), d["wp"].half().double(), torch.zeros(c.cout).double() if d["bias"] is None else d["bias"].double(),
                          c.k, c.s, c.act, nchw(d["res"]), c.act2)
    return d, y.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def dsbottleneck_net(B, C, H, W, k1, k2, shortcut, stride, cout=None, single=False, miss=None, fp16=True, int8=False):
    """conv (depthwise) -> conv (1x1) -> scale (BatchNorm, eps 1e-3) -> sigmoid -> prod, twice (once with `single`), then the sum with the input.
    miss: a near miss on the FIRST DSConv - "scale" / "act" behind its depthwise convolution, a "bias" on it, a second "reader" of its output, its output
    a network "output", "dilation" 2.  -> (plan, [(wd, folded fp16 1x1 weights as fp32, shift, k, stride)] for the reference)"""
    from tensorrtx_amd import builder, calibrator, engine
    net = builder.Network(max_batch=B, fp16=fp16, int8=int8)
    x = net.input("data", (C, H, W))
    layers, t, cin = [], x, C
    for j, (k, s, co) in enumerate([(k1, stride, cout or C)] if single else [(k1, stride, C), (k2, 1, cout or C)]):
        r = _rng(C, H, W, k, s, co, j)
        wd = (r.standard_normal((cin, 1, k, k)) / k).astype(np.float32)
        wp = (r.standard_normal((co, cin, 1, 1)) * (2.0 / cin) ** 0.5).astype(np.float32)
        scale = (r.uniform(0.5, 1.5, co) / np.sqrt(r.uniform(0.5, 1.5, co) + 1e-3)).astype(np.float32)   # gamma / sqrt(var + eps)
        shift = (r.standard_normal(co) * 0.2).astype(np.float32)
        m = miss if j == 0 else None
        dil = 2 if m == "dilation" else 1
        d = net.out(net.conv(t, wd, bias=np.ones(cin, np.float32) if m == "bias" else None, stride=s, padding=dil * (k // 2), groups=cin, dilation=dil))
        if m in ("reader", "output"):
            net.mark_output(net.out(net.activation(d, "relu")) if m == "reader" else d, "dw_" + m)
        if m in ("scale", "act"):
            d = net.out(net.scale(d, np.zeros(cin, np.float32), np.ones(cin, np.float32)) if m == "scale" else net.activation(d, "relu"))
        p = net.out(net.scale(net.out(net.conv(d, wp)), shift, scale))
        t = net.out(net.elementwise(p, net.out(net.activation(p, "sigmoid")), "prod"))
        layers.append((wd[:, 0], torch.from_numpy(wp[:, :, 0, 0] * scale[:, None]).half().float().numpy(), shift, k, s))
        cin = co
    net.mark_output(net.out(net.elementwise(x, t, "sum")) if shortcut else t, "y")
    if int8:   # the builder wants a scale for every tensor of the definition: a calibration cache by the names of the same network built without the flag
        names = [q["name"] or f"(Unnamed Tensor* {q['id']})" for q in engine.describe_plan(dsbottleneck_net(B, C, H, W, k1, k2, shortcut, stride)[0])["tensors"]]
        net.set_int8_calibrator(calibrator.Calibrator(cache=b"TRT-8601-EntropyCalibration2\n" + b"".join(f"{nm}: {np.float32(0.05).view(np.uint32):08x}\n".encode() for nm in names)))
    plan = net.build()
    net.close()
    return plan, layers


def net_reference(x, layers, shortcut):
    """x [B,C,H,W] fp32 -> (y, bound) of the network's output, NCHW fp64; every DSConv's output bound is the next one's input bound"""
    x16, f64 = x.half().double(), lambda v: torch.from_numpy(v).double()  # noqa: E731
    t, tb = x16, None
    for j, (wd, wp, shift, k, s) in enumerate(layers):
        t, tb = dsconv_ref(t, f64(wd), f64(wp), f64(shift), k, s, "silu", x16 if shortcut and j == len(layers) - 1 else None, x_bound=tb)
    return t, tb
