"""Lowering and packing of grouped convolutions (kernels/conv_grouped.hip), host only: which layers the plan marks `grouped`, what the A/B
switch and the other engine kinds do with them, and the packed filter against a NumPy restatement.  The device side is
tests/test_gpu_conv_grouped.py."""
import numpy as np
import pytest

from tensorrtx_amd import builder, capi, engine
from tests import conv_grouped_cases as gc
from tests import layer_cases as lc


def _the_conv(plan):
    convs = gc.convs_of(plan)
    assert len(convs) == 1, convs
    return convs[0]


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_fp16_plan_marks_the_layer_grouped_with_its_whole_epilogue(case):
    plan = gc.build_plan(case)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    c = _the_conv(plan)
    assert c.get("grouped") is True and not c["igemm"] and not c["stem"] and "dw" not in c, c
    assert c["act1"] == {"silu": 3, "leaky": 4}.get(case.act, 0) and c["act2"] == 0 and c["residual"] == case.res
    assert not {o["kind"] for o in ops} & {"act_nhwc", "ew_nhwc"}, [o["kind"] for o in ops]
    if case.in_view:
        assert c["ld_in"] == case.in_view[1]
    if case.out_view:
        assert c["ld_out"] == case.out_view[1]


@pytest.mark.parametrize("case", gc.CASES[:3], ids=lambda c: c.name)
def test_switch_off_puts_the_layer_back_on_the_direct_kernel(case, monkeypatch):
    monkeypatch.setenv("TRTX_CONV_GROUPED", "0")
    c = _the_conv(gc.build_plan(case))
    assert "grouped" not in c and not c["igemm"] and "dw" not in c, c


def test_fp32_plans_keep_the_direct_kernel():
    c = _the_conv(gc.build_plan(gc.BY_NAME["g4_3x3_13x17"], fp16=False))
    assert "grouped" not in c and not c["igemm"], c


def _single(Cin, Cout, groups, k, stride=1, pad=None, dilation=1, H=12, W=12):
    net = builder.Network(max_batch=2, fp16=True)
    try:
        x = lc.nhwc(net, net.input("x", (Cin, H, W)))
        w = np.zeros((Cout, Cin // groups, k, k), np.float32)
        net.mark_output(net.out(net.conv(x, w, None, stride, k // 2 if pad is None else pad, groups=groups, dilation=dilation)), "y")
        return _the_conv(net.build())
    finally:
        net.close()


@pytest.mark.parametrize("kw", [dict(Cin=32, Cout=32, groups=4, k=3),        # 8 per group
                                dict(Cin=64, Cout=64, groups=4, k=3, stride=2),
                                dict(Cin=64, Cout=64, groups=4, k=3, pad=2, dilation=2),
                                dict(Cin=64, Cout=64, groups=4, k=5),
                                dict(Cin=64, Cout=64, groups=4, k=3, pad=0),
                                dict(Cin=256, Cout=256, groups=16, k=3),     # more than 8 groups
                                dict(Cin=256, Cout=256, groups=2, k=3),      # 128 per group
                                dict(Cin=128, Cout=256, groups=8, k=3)],     # more output fragments than the waves hold in registers
                         ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()))
def test_layers_outside_the_scope_keep_the_direct_kernel(kw):
    c = _single(**kw)
    assert "grouped" not in c and not c["igemm"], c


@pytest.mark.parametrize("kw", [dict(Cin=48, Cout=96, groups=3, k=1), dict(Cin=96, Cout=96, groups=2, k=3), dict(Cin=128, Cout=128, groups=8, k=1),
                                dict(Cin=64, Cout=64, groups=4, k=3, H=1, W=1)],
                         ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()))
def test_layers_inside_the_scope_are_grouped(kw):
    assert _single(**kw).get("grouped") is True


@pytest.mark.parametrize("shape", [(64, 16, 3, 3), (64, 32, 3, 3), (96, 48, 3, 3), (32, 16, 1, 1), (128, 64, 3, 3)], ids=str)
def test_packed_filter_is_tap_major_with_the_scale_folded_before_rounding(shape):
    rng = np.random.default_rng(5)
    w = rng.standard_normal(shape).astype(np.float32)
    s = (0.5 + rng.random(shape[0])).astype(np.float32)
    cout, cg, kh, kw = shape
    K = kh * kw * cg
    kpad = (K + 31) // 32 * 32
    want = np.zeros((cout, kpad), np.float16)
    want[:, :K] = (w * s[:, None, None, None]).transpose(0, 2, 3, 1).reshape(cout, K).astype(np.float16)   # k = (r * kw + q) * Cin_g + c
    got = capi.pack_conv_weights_grouped_f16(w, ch_scale=s)
    assert got.shape == (cout, kpad) and np.array_equal(got, want.view(np.uint16))
    assert np.array_equal(capi.pack_conv_weights_grouped_f16(w), np.pad(w.transpose(0, 2, 3, 1).reshape(cout, K).astype(np.float16),
                                                                        ((0, 0), (0, kpad - K))).view(np.uint16))
