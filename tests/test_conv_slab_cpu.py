"""3x3 convolutions of many narrow groups (kernels/conv_slab.hip) and the resnext50_32x4d builder, host side: what the lowering hands to the kernel, the
switch, the packed filter, the predicate's refusals, and the builder's graph against the torch twin.  The device side is tests/test_gpu_conv_slab.py."""
import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from tensorrtx_amd import builder, capi, engine
from tests import conv_slab_cases as sc
from tests import layer_cases as lc


def _one_layer(fp16, C=128, groups=32, stride=2):
    """the convolution of conv -> ReLU -> + shortcut -> ReLU in the lowered plan, and the plan's op kinds"""
    net = builder.Network(max_batch=2, fp16=fp16)
    try:
        x = lc.nhwc(net, net.input("x", (C, 12, 12)))
        y = net.out(net.conv(x, np.zeros((C, C // groups, 3, 3), np.float32), np.zeros(C, np.float32), stride, 1, groups=groups))
        y = net.out(net.elementwise(net.out(net.activation(y, "relu")), lc.nhwc(net, net.input("r", (C, 12 // stride, 12 // stride))), "sum"))
        net.mark_output(net.out(net.activation(y, "relu")), "y")
        ops = engine.describe_plan(net.build(), lowered=True)["ops"]
    finally:
        net.close()
    (conv,) = [o for o in ops if o["kind"] == "conv"]
    return conv, {o["kind"] for o in ops}


def test_lowering_takes_32_groups_in_fp16_plans_only_and_the_switch_puts_them_back(monkeypatch):
    c, kinds = _one_layer(True)
    assert c.get("slab") is True and not c["igemm"] and (c["act1"], c["residual"], c["act2"]) == (capi.ACT["relu"], True, capi.ACT["relu"]), c
    assert not kinds & {"act_nhwc", "ew_nhwc"}, kinds
    f32 = _one_layer(False)[0]
    monkeypatch.setenv("TRTX_CONV_SLAB", "0")
    for o in (f32, _one_layer(True)[0]):
        assert not (o.get("slab") or o.get("grouped") or o["igemm"]), o


@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_packed_filter_is_the_numpy_restatement_of_the_block_diagonal_rows(cg):
    C, S = 96 if cg < 32 else 64, max(16, cg)
    rng = np.random.default_rng(cg)
    w, scale = rng.standard_normal((C, cg, 3, 3)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
    want = np.zeros((C, (9 * S + 31) // 32 * 32), np.float16)
    for co in range(C):
        first = co % S // cg * cg   # the row's group's first channel inside its slab
        for tap in range(9):
            want[co, tap * S + first:tap * S + first + cg] = (w[co, :, tap // 3, tap % 3] * scale[co]).astype(np.float16)
    assert np.array_equal(capi.pack_conv_weights_slab_f16(w, C // cg, scale), want.view(np.uint16))
    with pytest.raises(capi.TrtxError):   # 2 per group: what the kernel refuses, the packer refuses
        capi.pack_conv_weights_slab_f16(np.zeros((64, 2, 3, 3), np.float32), 32)


BASE = dict(N=1, H=8, W=8, Cin=64, in_off=0, ld_in=64, Cout=64, out_off=0, ld_out=64, k=3, stride=1, pad=1, dilation=1, groups=16, res=0, res_off=0, ld_res=0)


@pytest.mark.parametrize("ok,kw", [
    (1, dict(N=2, H=13, W=17, in_off=64, ld_in=128, out_off=8, ld_out=144, stride=2, res=1, res_off=16, ld_res=80)),   # 4 per group, stride 2, views
    (1, dict(H=7, W=7, Cin=1024, ld_in=1024, Cout=1024, ld_out=1024, groups=32)), (0, dict(groups=32)), (0, dict(Cin=128, ld_in=128, Cout=128, ld_out=128, groups=2)),
    (0, dict(Cout=128, ld_out=128)), (0, dict(k=1, pad=0)), (0, dict(k=5, pad=2)), (0, dict(pad=0)), (0, dict(pad=2, dilation=2)), (0, dict(stride=3)),
    (0, dict(in_off=4, ld_in=72)), (0, dict(ld_out=68)), (0, dict(res=1, res_off=12, ld_res=80))], ids=str)
def test_predicate(ok, kw):
    assert capi.lib().trtx_conv_slab_supported(*{**BASE, **kw}.values()) == ok, kw


def test_builder_graph_matches_the_twin_and_its_fp16_plan_at_224_has_all_sixteen_grouped_layers_on_the_slab_kernel(tmp_path):
    sd, path = sc.resnext50_wts(tmp_path)
    plan = engine.build_plan("resnext50_32x4d", path, batch=2, fp16=0, h=64, w=64)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    with torch.inference_mode():
        got, ref = gi.run(engine.describe_plan(plan), plan, {"data": x})["prob"].reshape(2, 1000), sc.resnext50_twin(sd, x)
    assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    plan = engine.build_plan("resnext50_32x4d", path, batch=32, fp16=1, h=224, w=224)
    convs = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "conv"]
    assert len(convs) == 54 and all(o["igemm"] or o["stem"] or o.get("slab") for o in convs)   # 53 convolutions and the fc, which runs as a 1x1
    assert sorted(o["stride"][0] for o in convs if o.get("slab")) == [1] * 13 + [2] * 3
