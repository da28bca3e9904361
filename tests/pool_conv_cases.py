"""YOLOv9's AConv / ADown halves with the pools inside the convolution's launch (kernels/conv_pool.hip): the case table of tests/test_gpu_pool_conv.py, its torch
fp64 reference with the per-element bound, and the small AConv / ADown networks that tests/test_pool_conv_cpu.py and the GPU test lower.

Reference: fp64 on the fp16 input and the folded fp16 weights, the average NOT rounded.  Bound, per element, nothing fitted; P = |pooled| (avgmax_c1: its 3x3 maximum -
rounding is monotone, so the rounded maximum is the maximum of the rounded values), A = the same pools of |x|:  1.1 (SiLU's largest slope) x [u sum |w| P (the kernel
rounds its pooled operand to fp16 once: half an ulp, u = 2^-11) + fp32_bound(K + 5, sum |w| A + |shift|) (the conv table's fp32 model over the K products, the pool's
three sums and scaling, the shift)] + fp16_walk(1, |y|) (the output rounding)."""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.layer_cases import Out, fp32_bound
from tests.parity import EPS16, fp16_walk

Case = collections.namedtuple("Case", "name mode B H W cin cout negative", defaults=(False,))
_both = lambda tag, *a: [Case(f"{tag}_{m}", m, *a) for m in ("avg_c3", "avgmax_c1")]  # noqa: E731
CASES = {c.name: c for c in
         _both("c32_64_16x16", 2, 16, 16, 32, 64)          # even H and W: the last pooled row and column do not exist - zero (avg_c3) / excluded (avgmax_c1)
         + _both("c32_64_13x17", 2, 13, 17, 32, 64)        # odd sizes, ragged tiles
         + _both("c40_72_9x9", 2, 9, 9, 40, 72)            # a chunk tail of 8 channels, a ragged channel tile (128-wide, five column blocks)
         + _both("c96_136_19x35", 2, 19, 35, 96, 136)      # over the 8- and the 16-pixel tile edge, three chunks, two column tiles
         + _both("c16_16_2x2", 2, 2, 2, 16, 16)            # one pooled pixel
         + _both("c16_16_4x4", 2, 4, 4, 16, 16)            # yolov9c's smallest map
         + [Case("negative_avgmax_c1", "avgmax_c1", 2, 6, 7, 32, 16, True),   # every input negative: a zero where -inf belongs would win the maximum
            Case("batch3_avg_c3", "avg_c3", 3, 10, 18, 32, 64)]}              # tiles never span images
_rng = lambda *key: np.random.default_rng(zlib.crc32(repr(key).encode()))  # noqa: E731   (seeded by what the data is for)
silu = lambda v: v * torch.sigmoid(v)  # noqa: E731


def pool_conv_ref(x, w, shift, mode):
    """NCHW fp64 x (fp16 values), w [Cout, Cin, k, k] fp64 (folded, fp16 values), shift fp64 -> (y, bound), NCHW fp64"""
    pools = lambda t: F.avg_pool2d(t, 2, 1) if mode == "avg_c3" else F.max_pool2d(F.avg_pool2d(t, 2, 1), 3, 2, 1)  # noqa: E731
    conv = lambda t, k: F.conv2d(t, k, None, 2, 1) if mode == "avg_c3" else F.conv2d(t, k)  # noqa: E731
    P = F.avg_pool2d(x, 2, 1).abs() if mode == "avg_c3" else F.max_pool2d(F.avg_pool2d(x, 2, 1).abs(), 3, 2, 1)
    y = silu(conv(pools(x), w) + shift[None, :, None, None])
    mag = conv(pools(x.abs()), w.abs()) + shift.abs()[None, :, None, None]
    K = w[0].numel()
    return y, 1.1 * (EPS16 * conv(P, w.abs()) + fp32_bound(Out(None, mag, n=K + 5))) + fp16_walk(1, y.abs())


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, y, bound) of a table case, once: x [B,H,W,Cin] fp32, w [Cout,Cin,k,k] fp32 of fp16 values, bias fp32; y and bound NHWC fp64"""
    c = CASES[name]
    k = 3 if c.mode == "avg_c3" else 1
    t = lambda what, *shape: torch.from_numpy(_rng(name, what).standard_normal(shape).astype(np.float32))  # noqa: E731
    x = t("x", c.B, c.H, c.W, c.cin)
    d = dict(x=-x.abs() - 0.01 if c.negative else x, w=(t("w", c.cout, c.cin, k, k) * (2.0 / (c.cin * k * k)) ** 0.5).half().float(), bias=t("b", c.cout) * 0.5)
    y, bound = pool_conv_ref(d["x"].half().double().permute(0, 3, 1, 2), d["w"].double(), d["bias"].double(), c.mode)
    return d, y.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def down_net(kind, B, C, H, W, cout, miss=None, fp16=True, int8=False):
    """AConv ("aconv": avg-pool 2x2 / 1 -> conv 3x3 / 2 pad 1 -> scale -> sigmoid -> prod) or ADown ("adown": the pool's channel halves through that block to cout / 2
    and through max-pool 3x3 / 2 pad 1 -> the 1x1 block to cout / 2, concatenated), as yolov9/src/block.cpp:256-290 spells them.  miss: the pooled tensor has a
    third "reader", or is a network "output".  -> (plan, [(mode, first input channel, channels, folded fp16 weights as fp32, shift)] for the reference)"""
    from tensorrtx_amd import builder, calibrator, engine
    net = builder.Network(max_batch=B, fp16=fp16, int8=int8)
    x = net.input("data", (C, H, W))
    p = net.out(net.pooling(x, 2, 1, 0, avg=True))
    layers = []

    def cbs(t, mode, c0, cin, co):
        r, k = _rng(kind, C, H, W, mode), 3 if mode == "avg_c3" else 1
        w = (r.standard_normal((co, cin, k, k)) * (2.0 / (cin * k * k)) ** 0.5).astype(np.float32)
        scale = (r.uniform(0.5, 1.5, co) / np.sqrt(r.uniform(0.5, 1.5, co) + 1e-3)).astype(np.float32)   # gamma / sqrt(var + eps)
        shift = (r.standard_normal(co) * 0.2).astype(np.float32)
        q = net.out(net.scale(net.out(net.conv(t, w, stride=2 if k == 3 else 1, padding=k // 2)), shift, scale))
        layers.append((mode, c0, cin, torch.from_numpy(w * scale[:, None, None, None]).half().float(), torch.from_numpy(shift)))
        return net.out(net.elementwise(q, net.out(net.activation(q, "sigmoid")), "prod"))

    if miss == "reader":
        net.mark_output(net.out(net.activation(p, "relu")), "pooled_relu")
    if miss == "output":
        net.mark_output(p, "pooled")
    if kind == "aconv":
        y = cbs(p, "avg_c3", 0, C, cout)
    else:
        h = C // 2
        s1, s2 = (net.out(net.slice(p, (c0, 0, 0), (h, H - 1, W - 1))) for c0 in (0, h))
        y = net.out(net.concat([cbs(s1, "avg_c3", 0, h, cout // 2), cbs(net.out(net.pooling(s2, 3, 2, 1)), "avgmax_c1", h, h, cout // 2)]))
    net.mark_output(y, "y")
    if int8:   # the builder wants a scale for every tensor of the definition: a calibration cache by the names of the same network built without the flag
        names = [q["name"] or f"(Unnamed Tensor* {q['id']})" for q in engine.describe_plan(down_net(kind, B, C, H, W, cout)[0])["tensors"]]
        net.set_int8_calibrator(calibrator.Calibrator(cache=b"TRT-8601-EntropyCalibration2\n" + b"".join(f"{nm}: {np.float32(0.05).view(np.uint32):08x}\n".encode() for nm in names)))
    plan = net.build()
    net.close()
    return plan, layers


def net_reference(x, layers):
    """x [B,C,H,W] fp32 -> (y, bound) of the network's output "y", NCHW fp64"""
    x16 = x.half().double()
    parts = [pool_conv_ref(x16[:, c0:c0 + cin], w.double(), shift.double(), mode) for mode, c0, cin, w, shift in layers]
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
