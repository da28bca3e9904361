"""YOLO11 detection (host builder, explicit-batch plugin rule, batched matmul, depthwise kernel selection): CPU-side checks."""
import collections
import os

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import builder, engine, synth
from tensorrtx_amd import wts as wts_writer
from util import CACHE
from yolo11_twin import Yolo11


def yolo11_wts(scale, seed=0):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"yolo11{scale}_synth_s{seed}.wts")
    sd = synth.yolo11_state(scale, seed=seed)
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def lowered(scale, **kw):
    path, _ = yolo11_wts(scale)
    plan = engine.build_plan("yolo11" + scale, path, **kw)
    return plan, engine.describe_plan(plan, lowered=True)


@pytest.mark.parametrize("scale", ["n", "m"])
def test_yolo11_builder_matches_pytorch_twin(scale):
    """The host builder's graph (run by the oracle's interpreter, explicit batch) against an independent restatement of the
    ultralytics modules; yolo11m takes the C3k path"""
    path, sd = yolo11_wts(scale)
    B, S = 2, 128
    plan = engine.build_plan("yolo11" + scale, path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    desc = engine.describe_plan(plan)
    assert desc["explicit_batch"]
    x = torch.from_numpy(synth.images(B, S, S, seed=5))
    out = gi.run(desc, plan, {"images": x.numpy()}, batch=B)
    with torch.inference_mode():
        heads, strides = Yolo11(sd, scale).heads(x)
    assert strides == [8, 16, 32]
    for i, h in enumerate(heads):
        assert tuple(out[f"head{i}"].shape) == tuple(h.shape) == (B, 84, (S // strides[i]) ** 2)
        assert (out[f"head{i}"] - h).abs().max().item() < 2e-4
    # the plugin decodes every image of the batch (explicit-batch plugin rule), bit-exact against the reference decode
    got = out["output"].reshape(B, -1).numpy()
    dec = yp.decode_c([out[f"head{i}"].numpy() for i in range(3)], 80, S, S, strides)
    assert np.array_equal(got, dec)
    ref = yp.decode_c([h.numpy() for h in heads], 80, S, S, strides)
    assert np.array_equal(got[:, 0], ref[:, 0]) and (got[:, 0] > 0).all()


LINEAR_KINDS = {"to_linear", "gather", "scatter", "ew_lin", "act_lin", "scale_lin", "reduce_lin", "copy_lin", "softmax", "matmul", "plugin"}


def test_yolo11n_fp16_lowering_640_b32():
    _, low = lowered("n", batch=32, h=640, w=640, fp16=1)
    ops = low["ops"]
    kinds = collections.Counter(o["kind"] for o in ops)
    assert set(kinds) <= {"conv", "conv_group", "pool_chain", "attention", "yolo_head", "copy_nhwc"}, kinds
    assert not set(kinds) & LINEAR_KINDS
    # one channel copy remains: C2PSA's concat of cv1's first half (a view of cv1's output, which cannot move into the concat
    # buffer because its second half is the PSA block's input) with the block's output (block.cpp:366-415)
    assert kinds["copy_nhwc"] == 1
    assert kinds["attention"] == 1 and kinds["yolo_head"] == 1
    (att,) = [o for o in ops if o["kind"] == "attention"]
    assert (att["heads"], att["n"], att["kd"], att["hd"]) == (2, 400, 32, 64)
    convs = [o for o in ops if o["kind"] == "conv"] + [m for o in ops if o["kind"] == "conv_group" for m in o["members"]]
    dw = [o for o in convs if o.get("dw")]
    assert len(dw) == 7, [o["name"] for o in dw]   # six DWConv of the class branches + the attention's pe
    assert all(o["cin"] == o["cout"] for o in dw)
    assert sorted({tuple(o["hw_in"]) for o in dw}) == [(20, 20), (40, 40), (80, 80)]
    assert all(o["igemm"] or o["stem"] or o.get("dw") for o in convs)   # every other convolution: stem or implicit GEMM
    assert sum(o["stem"] for o in convs) == 1


def test_yolo11n_fp32_lowering_has_no_direct_depthwise():
    """fp32 engines keep the generic attention path (the tolerance build) and use the depthwise kernel's fp32 instantiation"""
    _, low = lowered("n", batch=2, h=256, w=256, fp16=0)
    convs = [o for o in low["ops"] if o["kind"] == "conv"]
    assert sum(bool(o.get("dw")) for o in convs) == 7
    assert not [o for o in convs if not (o["igemm"] or o["stem"] or o.get("dw"))]
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["attention"] == 0 and kinds["matmul"] == 2 and kinds["yolo_head"] == 1 and kinds["plugin"] == 0


def test_yolo11s_has_four_heads():
    _, low = lowered("s", batch=2, h=128, w=128, fp16=1)
    (att,) = [o for o in low["ops"] if o["kind"] == "attention"]
    assert att["heads"] == 4 and att["n"] == 16


def test_yolo11_marked_heads_keep_the_plugin():
    """Heads exposed as outputs cannot be fused away: the YoloLayer_TRT plugin then runs in the explicit-batch plan"""
    _, low = lowered("n", batch=4, h=128, w=128, fp16=1, mark_heads=1)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo_head"] == 0 and kinds["attention"] == 1


def test_yolo11_unknown_scale_is_rejected():
    path, _ = yolo11_wts("n")
    with pytest.raises(RuntimeError):
        engine.build_plan("yolo11q", path, batch=1)


def test_generic_batched_matmul_lowers_with_broadcast():
    net = builder.Network(explicit_batch=True)
    try:
        a = net.input("a", (2, 3, 5, 7))
        b = net.input("b", (1, 3, 7, 4))
        mm = net.matmul(a, b)
        net.mark_output(net.out(mm), "y")
        plan = net.build()
    finally:
        net.close()
    desc = engine.describe_plan(plan)
    t = {x["id"]: x for x in desc["tensors"]}
    assert t[desc["layers"][-1]["outputs"][0]]["dims"] == [2, 3, 5, 4]
    low = engine.describe_plan(plan, lowered=True)
    assert [o["kind"] for o in low["ops"]].count("matmul") == 1
    # the interpreter agrees with torch on the graph itself
    rng = np.random.default_rng(0)
    xa, xb = rng.standard_normal((2, 3, 5, 7)).astype(np.float32), rng.standard_normal((1, 3, 7, 4)).astype(np.float32)
    out = gi.run(desc, plan, {"a": xa, "b": xb})["y"]
    assert torch.allclose(out, torch.from_numpy(xa) @ torch.from_numpy(xb), atol=1e-5)


def test_explicit_batch_plugin_gets_batch_prepended():
    """YoloLayer_TRT fed (B, 4 + nc, g) in an explicit-batch network: getOutputDimensions sees (4 + nc, g), the output gets B
    prepended (TensorRT's IPluginV2 rule).  The enqueue side (batchSize = B) is checked on the GPU: test_gpu_yolo11.py decodes
    every image of a batch of 8 through the plugin"""
    B = 3
    path, _ = yolo11_wts("n")
    plan = engine.build_plan("yolo11n", path, batch=B, h=128, w=128, fp16=1)
    desc = engine.describe_plan(plan)
    t = {x["id"]: x for x in desc["tensors"]}
    (pl,) = [l for l in desc["layers"] if l.get("plugin_type") == "YoloLayer_TRT"]
    assert [t[i]["dims"] for i in pl["inputs"]] == [[B, 84, 16 * 16], [B, 84, 8 * 8], [B, 84, 4 * 4]]
    assert t[pl["outputs"][0]]["dims"] == [B, 1 + 1000 * yp.DET_FLOATS, 1, 1]   # the per-image dims of the plugin, B prepended
