"""Grouped and channel-view convolutions of fp32 engines (kernels/conv_patch_f32.hip), CPU side: which layers the lowering hands to the kernel under
TRTX_CONV_F32_PATCH=1, what stays on the direct kernel, the switch, the packed filter and the C entries."""
import ctypes
import os
import re

import numpy as np
import pytest

from tensorrtx_amd import capi
from tests import conv_patch_f32_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("trtx_op_conv2d_patch_nhwc_f32", "trtx_conv_patch_f32_supported", "trtx_conv_pack_weights_patch_f32")
INVALID, UNSUPPORTED = 1, 4


def _on_direct(conv):
    return not (conv["igemm"] or conv["stem"] or conv.get("dw") or conv.get("grouped") or conv.get("view") or conv.get("patch_f32"))


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_table_cases_lower_to_one_fused_patch_f32_convolution(case, monkeypatch):
    _, off = pc.build_plan(case)
    monkeypatch.setenv("TRTX_CONV_F32_PATCH", "1")
    _, on = pc.build_plan(case)
    for ops, patched in ((off, False), (on, True)):
        (conv,) = [o for o in ops if o["kind"] == "conv"]
        assert not any(o["kind"] in ("act_nhwc", "ew_nhwc") for o in ops), [o["kind"] for o in ops]
        assert (conv.get("patch_f32") is True) == patched and _on_direct(conv) == (not patched), conv
        assert conv["residual"] == bool(case.res_view) and conv["act1"] == capi.ACT[case.act] and (conv["cin"], conv["cout"]) == (case.Cin, case.Cout)


@pytest.mark.parametrize("what,base,kw", [("stride 2", "c90_3x3", dict(stride=2)), ("dilation 2", "c90_3x3", dict(dil=2)), ("5x5", "c90_3x3", dict(k=5)),
                                          ("16 groups", "g4_3x3", dict(Cout=256, groups=16)), ("Cin_g 6", "g4_3x3", dict(Cin=12, Cout=32, groups=2)),
                                          ("an fp16 engine", "c6_3x3", dict())])
def test_layers_outside_the_scope_keep_the_direct_kernel(what, base, kw, monkeypatch):
    monkeypatch.setenv("TRTX_CONV_F32_PATCH", "1")
    _, ops = pc.build_plan(pc.BY_NAME[base]._replace(name=what, H=8, W=8, N=1, **kw), fp16=what == "an fp16 engine")
    (conv,) = [o for o in ops if o["kind"] == "conv"]
    assert _on_direct(conv), (what, conv)


def test_symbols_are_bound_and_the_predicate_and_refusals_are_decided_on_the_host():
    header = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    for sym in SYMBOLS:
        assert hasattr(capi.lib(), sym) and re.search(r"\b%s\(" % sym, header), sym
    assert callable(capi.conv2d_patch_nhwc_f32) and callable(capi.pack_conv_weights_patch_f32) and "yolov9/src/block.cpp" in header
    # (N, H, W, Cin, in offset, ld_in, Cout, out offset, ld_out, k, stride, pad, dilation, groups, residual?, its offset, its ld)
    ok = capi.lib().trtx_conv_patch_f32_supported
    assert ok(2, 5, 7, 90, 90, 180, 90, 7, 107, 3, 1, 1, 1, 1, 1, 3, 93) == 1 and ok(1, 8, 8, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0) == 1
    assert ok(1, 8, 8, 64, 3, 70, 64, 5, 69, 3, 1, 1, 1, 4, 0, 0, 0) == 1 and ok(1, 8, 8, 512, 0, 512, 128, 0, 128, 1, 1, 0, 1, 8, 0, 0, 0) == 1
    for bad in ((1, 8, 8, 90, 0, 90, 90, 0, 90, 3, 2, 1, 1, 1, 0, 0, 0), (1, 8, 8, 90, 0, 90, 90, 0, 90, 3, 1, 2, 2, 1, 0, 0, 0), (1, 8, 8, 90, 0, 90, 90, 0, 90, 5, 1, 2, 1, 1, 0, 0, 0),
                (1, 8, 8, 144, 0, 144, 144, 0, 144, 3, 1, 1, 1, 9, 0, 0, 0), (1, 8, 8, 12, 0, 12, 32, 0, 32, 3, 1, 1, 1, 2, 0, 0, 0), (1, 8, 8, 64, 0, 64, 160, 0, 160, 3, 1, 1, 1, 2, 0, 0, 0),
                (1, 8, 8, 90, 91, 180, 90, 0, 90, 3, 1, 1, 1, 1, 0, 0, 0), (1, 8, 8, 90, 0, 90, 90, 0, 90, 3, 1, 1, 1, 1, 1, 0, 89)):
        assert ok(*bad) == 0, bad
    fn = capi.lib().trtx_op_conv2d_patch_nhwc_f32
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.c_void_p])
    fn.restype = ctypes.c_int32
    p = 0x10000     # never dereferenced: every call below returns before a launch (there is no device here to launch on)

    def call(x=p, w=p, out=p + (1 << 30), cin=64, ld_in=64, cout=64, ld_out=64, groups=4, k=3, pad=1):
        return fn(x, 2, 8, 8, cin, ld_in, w, None, out, cout, ld_out, groups, k, pad, 0, None, 0, 0, None)
    assert call(x=None) == call(w=None) == call(out=None) == call(k=0) == INVALID
    for kw in (dict(pad=2), dict(k=5, pad=2), dict(groups=9, cin=144, ld_in=144, cout=144, ld_out=144), dict(groups=2, cin=12, ld_in=12), dict(ld_in=63),
               dict(x=p + 2), dict(out=p + (1 << 30) + 1)):
        assert call(**kw) == UNSUPPORTED, kw
    # an output on the input's bytes; another channel slice of the same map is none (it gets as far as the missing device or launches on one: not tried here)
    assert call(out=p) == call(out=p + 64, ld_in=128, ld_out=128) == call(w=p + 4) == INVALID


@pytest.mark.parametrize("cout,cin_g,k,groups", [(20, 6, 3, 1), (90, 90, 1, 1), (64, 16, 3, 4), (64, 20, 3, 2)])
def test_packed_filter_is_the_numpy_restatement(cout, cin_g, k, groups):
    rng = np.random.default_rng(cout * 131 + cin_g)
    w, sc = rng.standard_normal((cout, cin_g, k, k)).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    cink = cin_g if groups > 1 else (8 if cin_g <= 8 else (cin_g + 15) // 16 * 16)
    rows, kpad = (cout, (k * k * cin_g + 31) // 32 * 32) if groups > 1 else ((cout + 15) // 16 * 16, (k * k * cink + 15) // 16 * 16)
    want = np.zeros((rows, kpad), np.float32)
    taps = (w * sc[:, None, None, None]).transpose(0, 2, 3, 1).reshape(cout, k * k, cin_g)   # [cout][tap][c]
    for t in range(k * k):
        want[:cout, t * cink:t * cink + cin_g] = taps[:, t]
    got = capi.pack_conv_weights_patch_f32(w, groups, sc)
    assert got.shape == want.shape and np.array_equal(got, want)
