"""YOLOv13's area attention on separate qk and v (kernels/attention_mfma.hip's split instantiation, the attention_split plan op, match_aattn_split):
CPU-side checks of the lowering, the near misses, the switch, what must not change, the repacking of the attention table and the C entry."""
import collections
import ctypes
import os
import re

import pytest
import torch

from oracle import graph_interp as gi
from tensorrtx_amd import capi, engine
from test_yolo12_cpu import aattn_net, lowered
from tests import aattn_split_cases as sc
from tests import attention_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE_KINDS = {"scale_nhwc", "scale_lin"}
UNSUPPORTED = 4


def _ops(plan):
    return engine.describe_plan(plan, lowered=True)["ops"]


def _kinds(plan):
    return collections.Counter(o["kind"] for o in _ops(plan))


# ---- lowering -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("softmax", ["chain", "layer"])
@pytest.mark.parametrize("B,heads,hw,area", [(3, 2, (12, 14), 4), (1, 4, (10, 10), 1), (2, 1, (4, 8), 4)])
def test_aattn13_subgraph_lowers_to_one_op(B, heads, hw, area, softmax):
    H, W = hw
    for tail in ("v", "pe"):
        plan, _, _ = sc.aattn13_net(B, heads, H, W, area, softmax=softmax, tail=tail)
        ops = _ops(plan)
        kinds = collections.Counter(o["kind"] for o in ops)
        (att,) = [o for o in ops if o["kind"] == "attention_split"]
        assert (att["heads"], att["n"], att["kd"], att["hd"], att["area"]) == (heads, H * W, 32, 32, area)
        # as emit_attention counts flops; bytes = q, k, v read and O written, no V image (the description prints six digits)
        assert att["k_offset"] == heads * 32 and att["flops"] == pytest.approx(2 * B * heads * (H * W) * (H * W // area) * 64, rel=1e-5)
        assert att["bytes"] == pytest.approx(2 * B * H * W * 4 * heads * 32, rel=1e-5)
        assert not {"matmul", "softmax", "gather", "attention"} & set(kinds) and not SCALE_KINDS & set(kinds), (tail, kinds)
        # besides the input's and the output's layout passes:
        if tail == "pe":   # the qk, v and pe convolutions and the op; the sum is pe's residual epilogue
            assert not {"ew_nhwc", "ew_lin"} & set(kinds), kinds
            assert kinds == {"to_nhwc": 1, "conv": 3, "attention_split": 1, "to_linear": 1}, kinds
            (pe,) = [o for o in ops if o["kind"] == "conv" and o.get("dw")]
            assert pe["residual"]
        else:
            assert kinds == {"to_nhwc": 1, "conv": 2, "attention_split": 1, "ew_nhwc": 1, "to_linear": 1}, kinds


@pytest.mark.parametrize("softmax", ["chain", "layer"])
@pytest.mark.parametrize("miss", sc.MISSES)
def test_near_miss_graphs_lower_generically(miss, softmax):
    """One matcher condition broken at a time: no attention_split op, and the plan still builds and lowers"""
    plan, _, _ = sc.aattn13_net(2, 2, 8, 8, 4, softmax=softmax, miss=miss, hd=16 if miss == "hd16" else 32)
    kinds = _kinds(plan)
    assert kinds["attention_split"] == 0 and kinds["matmul"] == 2 and kinds["softmax"] == 1, kinds


def test_area_1_near_misses_lower_generically():
    """model.8's spelling (no 3-d reshapes) refuses the same breaks"""
    for miss in ("slice_start", "shift", "axis", "reader", "v_reshape"):
        kinds = _kinds(sc.aattn13_net(1, 2, 6, 6, 1, miss=miss)[0])
        assert kinds["attention_split"] == 0 and kinds["matmul"] == 2 and kinds["softmax"] == 1, (miss, kinds)


def test_switch_and_fp32_engines_keep_the_generic_ops(monkeypatch):
    for area in (4, 1):
        plan, _, _ = sc.aattn13_net(2, 2, 8, 8, area)
        assert _kinds(plan)["attention_split"] == 1
        plan32, _, _ = sc.aattn13_net(2, 2, 8, 8, area, fp16=False)
        kinds = _kinds(plan32)
        assert kinds["attention_split"] == 0 and kinds["matmul"] == 2 and kinds["softmax"] == 1, kinds
        monkeypatch.setenv("TRTX_AATTN_SPLIT", "0")
        kinds = _kinds(plan)
        assert kinds["attention_split"] == 0 and kinds["matmul"] == 2 and kinds["softmax"] == 1, kinds
        monkeypatch.setenv("TRTX_AATTN_SPLIT", "1")
        assert _kinds(plan)["attention_split"] == 1
        monkeypatch.delenv("TRTX_AATTN_SPLIT")


def test_yolo12_lowerings_do_not_change_with_the_switch(monkeypatch):
    """YOLOv12's packed-qkv AAttn and the yolo12n plan lower exactly as before, whatever the new switch says"""
    sub, _, _ = aattn_net(3, 2, 12, 14, 4)
    plan, _ = lowered("n", batch=2, h=128, w=128, fp16=1)
    seen = []
    for value in (None, "0", "1"):
        if value is not None:
            monkeypatch.setenv("TRTX_AATTN_SPLIT", value)
        seen.append((_ops(sub), _ops(plan)))
        ks, kp = _kinds(sub), _kinds(plan)
        assert ks["attention"] == 1 and ks["attention_split"] == 0 and not {"matmul", "softmax", "gather"} & set(ks)
        assert kp["attention"] == 8 and kp["attention_split"] == 0 and kp["yolo_head"] == 1
    assert seen[0] == seen[1] == seen[2]


@pytest.mark.parametrize("tail", ["v", "pe"])
@pytest.mark.parametrize("B,heads,hw,area", [(3, 2, (12, 14), 4), (1, 4, (10, 10), 1)])
def test_reference_formula_is_what_the_graph_computes(B, heads, hw, area, tail):
    """The oracle's interpreter on the literal graph (ISoftMaxLayer spelling: it has no IUnaryLayer; fp32, no storage sites) against the torch formula
    the GPU tests use as their reference, unrounded"""
    H, W = hw
    plan, x, weights = sc.aattn13_net(B, heads, H, W, area, softmax="layer", tail=tail, fp16=False)
    got = gi.run(engine.describe_plan(plan), plan, {"x": x}, batch=B)["y"].reshape(B, heads * 32, H, W).double()
    o, other, *_ = sc.aattn13_reference(x, weights, heads, area, tail, rounded=False)
    err = (got - (o + other)).abs().max().item()
    print(f"{tail} B{B} heads {heads} {H}x{W} area {area}: interpreter vs fp64 formula {err:.3g}, |y| {(o + other).abs().max().item():.3g}")
    assert err <= 1e-5 * max(1.0, (o + other).abs().max().item())


# ---- the table, repacked ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.AREA, ids=lambda c: c.name)
def test_split_operands_round_trip_and_keep_the_reference(case):
    qkv = ac.gen_inputs(case.name)
    qk, v = sc.split_operands(case, qkv)
    C = case.heads * 32
    assert qk.shape == (case.B, case.N, 2 * C) and v.shape == (case.B, case.N, C)
    assert torch.equal(sc.join_operands(case, qk, v), qkv)
    q0, k0, v0 = ac.split(case, qkv)
    for h in range(case.heads):
        assert torch.equal(qk[..., h * 32:(h + 1) * 32], q0[:, h]) and torch.equal(qk[..., C + h * 32:C + (h + 1) * 32], k0[:, h])
        assert torch.equal(v[..., h * 32:(h + 1) * 32], v0[:, h])
    o, _, _, _ = sc.attention_f64(qk[..., :C].double(), qk[..., C:].double(), v.double(), case.heads, case.area)
    ref = ac.reference(case.name)
    # the same fp64 formula on the same values, the scale as the fp32 constant instead of 32 ** -0.5: 6e-9 relative on a score
    assert (o - ref.o).abs().max().item() <= 1e-6 * max(1.0, ref.o.abs().max().item())
    assert torch.equal(v, ref.v)


# ---- the C entry --------------------------------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    L = capi.lib()
    sym = "trtx_op_area_attention_split_f16"
    assert re.search(r"\b%s\s*\(" % sym, src) and hasattr(L, sym)
    proto = re.search(sym + r"\((.*?)\);", src, re.S).group(1)
    assert re.findall(r"(\w+)\s*(?:,|$)", proto) == ["q", "ld_q", "k", "ld_k", "v", "ld_v", "out", "ld_out", "B", "heads", "N", "area", "kd", "hd", "scale", "stream"]
    assert "yolov13/src/block.cpp:303-423" in src
    assert L.trtx_abi_version() == 1


def test_refusals_are_decided_on_the_host():
    fn = capi.lib().trtx_op_area_attention_split_f16
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int] * 4 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_void_p]
    fn.restype = ctypes.c_int32
    p = 0x10000     # never dereferenced: every call below returns before a launch (there is no device here to launch on)

    def call(q=p, k=p, v=p, out=p, ld_q=128, ld_k=128, ld_v=64, ld_out=64, B=1, heads=2, N=32, area=4, kd=32, hd=32):
        return fn(q, ld_q, k, ld_k, v, ld_v, out, ld_out, B, heads, N, area, kd, hd, 0.25, None)
    assert call(q=None) == call(k=None) == call(v=None) == call(out=None) == 1   # TRTX_ERR_INVALID
    for kw in (dict(N=30), dict(kd=16), dict(hd=64), dict(hd=16), dict(ld_q=63), dict(ld_k=63), dict(ld_v=63), dict(ld_out=63), dict(B=0), dict(heads=0),
               dict(N=0, area=1), dict(area=0), dict(B=65536), dict(heads=16384, area=4, ld_q=1 << 20, ld_k=1 << 20, ld_v=1 << 20, ld_out=1 << 20)):
        assert call(**kw) == UNSUPPORTED, kw
