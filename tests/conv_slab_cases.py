"""The case table of kernels/conv_slab.hip (tests/test_gpu_conv_slab.py) and the torch twin of ResNeXt-50 32x4d (test_conv_slab_cpu.py, test_gpu_resnext50.py).
Reference and bound as in tests/conv_grouped_cases.py: inputs and weights GENERATED on the fp16 grid, torch fp64 conv2d, per element fp32_bound(n = 9 cg + 2:
the products, the bias, the shortcut) + fp16_walk(1 site, the store).  ReLU: slope <= 1 and |relu(z)| <= |z|, the bound of its argument holds.  Nothing fitted."""
import math
import os
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import layer_cases as lc
from tests.parity import fp16_walk


# in_view / out_view: (channel offset, channels of the wider tensor); 9 x 19: two tile columns and three tile rows at stride 1, the last of each ragged
SCase = namedtuple("SCase", "name C groups stride H W N act1 act2 res in_view out_view", defaults=(9, 19, 2, "none", "none", False, None, None))
CASES = [SCase(f"cg{64 // g}_s{s}_13x17", 64, g, s, 13, 17) for g in (16, 8, 4, 2) for s in (1, 2)] + [   # ragged tiles, an odd map under stride 2
    SCase("s2_even_12x16", 64, 16, 2, 12, 16),            # the right and bottom padding is never read
    SCase("s1_5x7", 64, 8, 1, 5, 7), SCase("s2_5x7", 64, 8, 2, 5, 7),   # a map smaller than one tile, borders on all sides
    SCase("c96_g24", 96, 24, 1),                          # a ragged last chunk of 32 channels: two idle waves
    SCase("c128_g32", 128, 32, 1),                        # ResNeXt's stage-1 layer: two chunks
    SCase("c64_g2", 64, 2, 2),                            # 32 per group: S = 32, one tap per step
    SCase("in_view", 64, 16, 1, in_view=(64, 128)), SCase("out_view", 64, 8, 2, out_view=(0, 144)),
    SCase("res_relu2", 64, 16, 1, res=True, act2="relu"), SCase("relu1", 64, 4, 2, act1="relu"),   # the block's and the model's epilogue
    # the persistent walk: 16 chunks get 768 / 16 = 48 workgroups each for 9 x 6 x 2 = 108 tiles (21 x 17 output pixels, ragged both ways), so a workgroup
    # takes two or three tiles: the prefetch, both patch buffers and staging tiles (stride 1), the single buffer and its second barrier (stride 2)
    SCase("walk_s1_cg8", 1024, 128, 1, 21, 17, 9, res=True, act2="relu"), SCase("walk_s2_cg32", 1024, 32, 2, 41, 33, 9, act1="relu"),
]


def gen(case):
    """x [N, Cin_total, H, W], w KCRS, r [N, C, Ho, Wo] or None on the fp16 grid, b [C] fp32: numpy"""
    rng = lambda what: np.random.default_rng(zlib.crc32((case.name + "/" + what).encode()))
    grid = lambda a: a.astype(np.float16).astype(np.float32)
    cg, ho, wo = case.C // case.groups, (case.H - 1) // case.stride + 1, (case.W - 1) // case.stride + 1
    return {"x": grid(rng("x").standard_normal((case.N, case.in_view[1] if case.in_view else case.C, case.H, case.W))),
            "w": grid(rng("w").standard_normal((case.C, cg, 3, 3)) / math.sqrt(9 * cg)), "b": rng("b").standard_normal(case.C).astype(np.float32),
            "r": grid(rng("r").standard_normal((case.N, case.C, ho, wo))) if case.res else None}


def reference(case, d):
    """(y fp64 [N, C, Ho, Wo], per-element bound)"""
    x = torch.from_numpy(d["x"]).double()[:, case.in_view[0]:case.in_view[0] + case.C] if case.in_view else torch.from_numpy(d["x"]).double()
    w, b = torch.from_numpy(d["w"]).double(), torch.from_numpy(d["b"]).double()
    y = F.conv2d(x, w, b, case.stride, 1, 1, case.groups)
    mag = F.conv2d(x.abs(), w.abs(), b.abs(), case.stride, 1, 1, case.groups)
    y = y.relu() if case.act1 == "relu" else y
    if case.res:
        r = torch.from_numpy(d["r"]).double()
        y, mag = y + r, mag + r.abs()
    y = y.relu() if case.act2 == "relu" else y
    return y, lc.fp32_bound(lc.Out(y, mag, n=9 * (case.C // case.groups) + 2, sites=1)) + fp16_walk(1, mag)


def resnext50_wts(folder):
    """(state, path of its .wts in `folder`): the seeded synthetic weights, written as bench.py writes a model's"""
    from tensorrtx_amd import synth, wts
    sd, path = synth.STATE["resnext50_32x4d"](seed=0), os.path.join(str(folder), "resnext50_32x4d.wts")
    wts.write_wts(path, sd, dialect="double")
    return sd, path


def resnext50_twin(sd, x):
    """ResNeXt-50 32x4d (resnet/resnext50_32x4d.cpp:111-230) as torch functions in x's dtype on a name -> array state; the average pool over the whole last map"""
    p = {k: torch.as_tensor(v).to(x.dtype) for k, v in sd.items()}
    bn = lambda t, n: F.batch_norm(t, p[n + ".running_mean"], p[n + ".running_var"], p[n + ".weight"], p[n + ".bias"], False, 0.0, 1e-5)
    x = F.max_pool2d(bn(F.conv2d(x, p["conv1.weight"], None, 2, 3), "bn1").relu(), 3, 2, 1)
    for stage, blocks in enumerate((3, 4, 6, 3)):
        for b in range(blocks):
            l, s = f"layer{stage + 1}.{b}.", 2 if (b == 0 and stage > 0) else 1
            y = bn(F.conv2d(x, p[l + "conv1.weight"]), l + "bn1").relu()
            y = bn(F.conv2d(y, p[l + "conv2.weight"], None, s, 1, 1, 32), l + "bn2").relu()
            y = bn(F.conv2d(y, p[l + "conv3.weight"]), l + "bn3")
            if l + "downsample.0.weight" in p:
                x = bn(F.conv2d(x, p[l + "downsample.0.weight"], None, s), l + "downsample.1")
            x = (x + y).relu()
    return F.linear(x.mean((2, 3)), p["fc.weight"], p["fc.bias"])
