"""Convolutions over unaligned channel views (kernels/conv_view.hip), CPU side: which layers the lowering hands to the kernel, the switch, the ABI."""
import collections
import os
import re

import pytest

from tensorrtx_amd import capi
from tests.test_yolov9_cpu import convs_of, lowered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(batch=1, h=64, w=64)
# YOLOv9m's RepNCSPELAN4 stages at 120 and 180 inner channels, (Cin, Cout, k) -> count: 40 of 159 convolutions; the converted model (no auxiliary
# branch) has 54 of 155, its 180-channel stage appearing three times, not twice
YOLOV9M_VIEWS = {0: {(60, 60, 1): 4, (60, 60, 3): 8, (90, 90, 1): 4, (90, 90, 3): 8, (180, 90, 1): 8, (180, 180, 1): 4, (180, 180, 3): 4},
                 1: {(60, 60, 1): 4, (60, 60, 3): 8, (90, 90, 1): 6, (90, 90, 3): 12, (180, 90, 1): 12, (180, 180, 1): 6, (180, 180, 3): 6}}


def _views(low):
    return collections.Counter((o["cin"], o["cout"], o["k"][0]) for o in convs_of(low) if o.get("view"))


@pytest.mark.parametrize("converted", [0, 1])
def test_yolov9m_has_no_convolution_on_the_direct_kernel(converted):
    _, low = lowered("yolov9m", converted, fp16=1, **KW)
    convs = convs_of(low)
    direct = [(o["name"], o["cin"], o["cout"], o["k"]) for o in convs if not (o["igemm"] or o["stem"] or o.get("dw") or o.get("grouped") or o.get("view"))]
    assert not direct, direct
    assert not any(o["igemm"] and o.get("view") for o in convs)
    assert dict(_views(low)) == YOLOV9M_VIEWS[converted] and len(convs) == (155 if converted else 159)


@pytest.mark.parametrize("name,fp16,switch_off", [("yolov9m", 1, True), ("yolov9m", 0, False), ("yolov9t", 1, False), ("yolov9s", 1, False),
                                                  ("yolov9c", 1, False), ("gelanc", 1, False)])
def test_no_view_layer_with_the_switch_off_in_fp32_and_in_the_other_models(name, fp16, switch_off, monkeypatch):
    if switch_off:
        monkeypatch.setenv("TRTX_CONV_VIEW", "0")
    assert not _views(lowered(name, 0, fp16=fp16, **KW)[1])


def test_abi_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    for sym in ("trtx_op_conv2d_view_nhwc_f16", "trtx_conv_view_supported"):
        assert hasattr(L, sym) and re.search(r"\b%s\(" % sym, header), sym
    assert callable(capi.conv2d_view_nhwc_f16)
    # (N, H, W, Cin, in offset, ld_in, Cout, out offset, ld_out, k, stride, pad, dilation, groups, residual?, its offset, its ld)
    ok = L.trtx_conv_view_supported
    assert ok(1, 8, 8, 90, 90, 180, 90, 0, 90, 3, 1, 1, 1, 1, 1, 90, 180) == 1
    assert ok(1, 8, 8, 256, 0, 256, 90, 0, 90, 3, 1, 1, 1, 1, 0, 0, 0) == 1 and ok(1, 8, 8, 258, 0, 258, 90, 0, 90, 3, 1, 1, 1, 1, 0, 0, 0) == 0
    assert ok(1, 8, 8, 90, 45, 180, 90, 0, 90, 3, 1, 1, 1, 1, 0, 0, 0) == 0 and ok(1, 8, 8, 90, 90, 180, 90, 0, 90, 3, 1, 1, 1, 2, 0, 0, 0) == 0
