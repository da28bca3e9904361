"""YOLOv5 detection (host builder, synthetic weights, the fused anchor head's lowering): CPU-side checks."""
import collections
import copy
import os

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import builder, capi, engine, synth
from tensorrtx_amd import wts as wts_writer
from util import CACHE
from yolov5_twin import Yolov5

KERNEL = np.dtype([("width", "<i4"), ("height", "<i4"), ("anchors", "<f4", (6,))])   # YoloKernel, yolov5/src/types.h:5-9
GENERIC_KINDS = {"plugin", "to_linear", "to_nhwc", "gather", "scatter"}


def yolov5_wts(name, seed=0):
    """name: "n" ... "x", or "n6" ... "x6" for the P6 models"""
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"yolov5{name}_synth_s{seed}_v2.wts")
    sd = synth.yolov5_state(name[0], seed=seed, p6=name.endswith("6"))
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def lowered(name, **kw):
    path, _ = yolov5_wts(name)
    plan = engine.build_plan("yolov5" + name, path, **kw)
    return plan, engine.describe_plan(plan, lowered=True)


def convs_of(low):
    return [o for o in low["ops"] if o["kind"] == "conv"] + [m for o in low["ops"] if o["kind"] == "conv_group" for m in o["members"]]


def without_plugin(desc):
    """oracle/graph_interp.py reads every YoloLayer_TRT blob with the YOLOv8 layout: hand it the graph up to the detect convolutions"""
    d = copy.deepcopy(desc)
    gone = [l for l in d["layers"] if l["kind"] == gi.L_PLUGIN]
    assert len(gone) == 1 and gone[0]["plugin_type"] == "YoloLayer_TRT"
    d["layers"] = [l for l in d["layers"] if l["kind"] != gi.L_PLUGIN]
    for t in gone[0]["outputs"]:
        d["tensors"][t]["is_output"] = False
    return d


@pytest.mark.parametrize("name,B,S", [("n", 2, 128), ("m", 1, 64), ("s6", 1, 128)])
def test_yolov5_builder_matches_pytorch_twin(name, B, S):
    """The host builder's graph (run by the oracle's interpreter) against an independent restatement of the modules: yolov5m has other
    depths (2 / 4 / 6 bottlenecks) and widths that are no power of two, s6 is the four-level graph.  Both sides are fp32 / fp64 on the
    CPU: the bound is test_yolo12_builder_matches_pytorch_twin's."""
    path, sd = yolov5_wts(name)
    plan = engine.build_plan("yolov5" + name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    desc = engine.describe_plan(plan)
    assert not desc["explicit_batch"]
    x = torch.from_numpy(synth.images(B, S, S, seed=5))
    out = gi.run(without_plugin(desc), plan, {"data": x.numpy()}, batch=B)
    tw = Yolov5(sd, name[0], p6=name.endswith("6"))
    with torch.inference_mode():
        heads, strides = tw.heads(x)
    assert strides == ([8, 16, 32, 64] if name.endswith("6") else [8, 16, 32])
    assert sorted(k for k in out) == [f"head{i}" for i in range(len(heads))]
    for i, h in enumerate(heads):
        assert tuple(out[f"head{i}"].shape) == (B, 255, S // strides[i], S // strides[i])
        d = (out[f"head{i}"].reshape(h.shape) - h).abs().max().item()
        print(f"yolov5{name} head{i}: |diff| {d:.3g}, |head| {h.abs().max().item():.3g}")
        assert d < 2e-4
    # what synth.yolov5_state promises: candidates well above zero and well below the anchor count, in every image
    grids = [(S // s, S // s) for s in strides]
    anchors = 3 * sum(gw * gh for gw, gh in grids)
    dec = yp.v5_decode_c([out[f"head{i}"].reshape(B, 255, -1).numpy() for i in range(len(heads))], 80, S, S, grids, tw.anchors(), anchors + 1)
    print(f"yolov5{name} {S}x{S}: candidates per image {dec[:, 0].astype(int).tolist()} of {anchors} anchors")
    assert dec[:, 0].min() >= 20 and dec[:, 0].max() <= 0.6 * anchors


@pytest.mark.parametrize("name,kw", [("n", dict(batch=32, h=640, w=640)), ("s6", dict(batch=1, h=128, w=128))])
def test_yolov5_lowering_has_one_fused_head(name, kw):
    levels = 4 if name.endswith("6") else 3
    for fp16 in (1, 0):
        _, low = lowered(name, fp16=fp16, **kw)
        kinds = collections.Counter(o["kind"] for o in low["ops"])
        print(f"yolov5{name} fp16={fp16}: {dict(kinds)}")
        assert kinds["yolo5_head"] == 1 and not set(kinds) & GENERIC_KINDS, kinds
        (head,) = [o for o in low["ops"] if o["kind"] == "yolo5_head"]
        assert (head["classes"], head["levels"], head["anchor_levels"]) == (80, levels, levels) and head["ld"] == [256] * levels
        S = kw["h"]
        assert head["grids"] == [[S // s, S // s] for s in (8, 16, 32, 64)[:levels]]
        convs = convs_of(low)
        det = [o for o in convs if o.get("cout_real")]
        assert len(det) == levels and all(o["cout_real"] == 255 and o["cout"] == 256 and o["cout"] % 8 == 0 and o["igemm"] for o in det)
        assert all(o["cout"] % 8 == 0 for o in convs)
        if fp16:
            assert all(o["igemm"] or o["stem"] or o.get("dw") for o in convs), [o["name"] for o in convs if not (o["igemm"] or o["stem"] or o.get("dw"))]


def test_yolov5_marked_heads_and_the_switch_keep_the_plugin(monkeypatch):
    _, low = lowered("n", batch=2, h=128, w=128, fp16=1, mark_heads=1)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo5_head"] == 0 and kinds["to_linear"] == 3
    assert not any(o.get("cout_real") for o in convs_of(low))
    plan, low = lowered("n", batch=2, h=128, w=128, fp16=1)
    assert collections.Counter(o["kind"] for o in low["ops"])["yolo5_head"] == 1
    monkeypatch.setenv("TRTX_YOLO5_HEAD", "0")
    low = engine.describe_plan(plan, lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo5_head"] == 0 and kinds["to_linear"] == 3
    det = [o for o in convs_of(low) if o["cout"] == 255]
    assert len(det) == 3 and not any(o.get("cout_real") for o in convs_of(low))   # the 255-channel convolutions lower as they did


def head_net(miss=None, fp16=True, classes=4, gw=6, gh=4):
    """One input, three 1x1 detect convolutions, the anchor plugin created from its fields.  `miss` breaks one thing the matcher
    checks: 'reader' (a detect output has a second reader), 'output' (a detect output is a network output), 'k3' (a 3x3 detect
    convolution), 'channels' (twice the channels on half the cells: the same volume, which is all the plugin's configure checks),
    'seg' (is_segmentation = 1, with the 32 mask channels per anchor), 'grid' (the kernels name the transposed grid)."""
    info = 5 + classes + (32 if miss == "seg" else 0)
    rng = np.random.default_rng(3)
    net = builder.Network(max_batch=2, fp16=fp16)
    try:
        x = net.input("x", (16, gh, gw))
        dets = []
        for lv in range(3):
            k = 3 if (miss == "k3" and lv == 1) else 1
            src, cout = x, 3 * info
            if miss == "channels" and lv == 2:
                src = net.out(net.pooling(x, (1, 2), (1, 2)))   # (16, gh, gw / 2)
                cout = 6 * info
            w = (rng.standard_normal((cout, 16, k, k)) / 4).astype(np.float32)
            dets.append(net.out(net.conv(src, w, bias=rng.standard_normal(cout).astype(np.float32), padding=k // 2)))
        if miss == "reader":
            net.mark_output(net.out(net.activation(dets[0], "relu")), "aux")
        if miss == "output":
            net.mark_output(dets[1], "aux")
        kern = np.zeros(3, dtype=KERNEL)
        for lv in range(3):
            kern[lv] = ((gh, gw) if miss == "grid" else (gw, gh)) + (synth.YOLOV5_ANCHORS[lv],)
        fields = [("netinfo", np.array([classes, 8 * gw, 8 * gh, 50, 1 if miss == "seg" else 0], np.int32)), ("kernels", kern.view(np.uint8), 3)]
        net.mark_output(net.out(net.plugin(dets, "YoloLayer_TRT", fields=fields)), "prob")
        return net.build()
    finally:
        net.close()


@pytest.mark.parametrize("fp16", [True, False])
def test_small_anchor_head_graph_fuses(fp16):
    low = engine.describe_plan(head_net(fp16=fp16), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["yolo5_head"] == 1 and kinds["plugin"] == 0 and kinds["to_linear"] == 0, kinds
    (head,) = [o for o in low["ops"] if o["kind"] == "yolo5_head"]
    ld = 32 if fp16 else 28   # 27 channels rounded up to 16 bytes
    assert (head["classes"], head["levels"], head["grids"], head["ld"]) == (4, 3, [[6, 4]] * 3, [ld] * 3)
    assert [(o["cout"], o["cout_real"], o["ld_out"]) for o in convs_of(low)] == [(ld, 27, ld)] * 3


@pytest.mark.parametrize("miss", ["reader", "output", "k3", "channels", "seg", "grid"])
def test_near_miss_graphs_keep_the_plugin(miss):
    """One matcher condition broken at a time: the plugin stays, no detect convolution is padded, and the plan still builds and lowers"""
    low = engine.describe_plan(head_net(miss=miss), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo5_head"] == 0, kinds
    assert not any(o.get("cout_real") for o in convs_of(low))


def test_plugin_without_fields_is_unchanged():
    """builder.Network.plugin without `fields` still hands the creator the empty collection (Mish_TRT)"""
    net = builder.Network(fp16=True)
    try:
        x = net.input("x", (8, 4, 4))
        net.mark_output(net.out(net.plugin([x], "Mish_TRT")), "y")
        plan = net.build()
    finally:
        net.close()
    assert [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]].count("act_nhwc") + \
        [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]].count("act_lin") == 1


def test_yolov5_build_errors_and_bindings():
    path, _ = yolov5_wts("n")
    for bad in (dict(model="yolov5q"), dict(model="yolov5n", h=100), dict(model="yolov5n7"), dict(model="yolov5n", w=72)):
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(bad.pop("model"), path, batch=1, **bad)
        assert e.value.status == 1   # TRTX_ERR_INVALID
    path6, _ = yolov5_wts("s6")
    with pytest.raises(capi.TrtxError) as e:   # 96 = 3 x 32: fine for P5, not for the stride-64 level
        engine.build_plan("yolov5s6", path6, batch=1, h=96, w=96)
    assert e.value.status == 1
    plan = engine.build_plan("yolov5n", path, batch=4, h=96, w=160, max_out=300)
    desc = engine.describe_plan(plan)
    io = [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_input"] or t["is_output"]]
    assert io == [("data", [3, 96, 160]), ("prob", [1 + 300 * 38, 1, 1])]
    assert desc["max_batch"] == 4
