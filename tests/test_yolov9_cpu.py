"""YOLOv9 / GELAN detection (host builder, synthetic weights, the built-in plugin, the fused DDetect head's lowering): CPU-side checks.
Also holds the helpers the GPU tests of tests/test_gpu_yolov9.py share."""
import collections
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import builder, capi, engine, synth
from tensorrtx_amd import wts as wts_writer
from util import CACHE
from yolov9_twin import Yolov9

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC_KINDS = {"plugin", "to_linear", "to_nhwc", "gather", "scatter", "softmax"}
MODELS = ("yolov9t", "yolov9s", "yolov9m", "yolov9c", "gelanc")
STRIDES = (8, 16, 32)


def yolov9_wts(name, converted=0, seed=0):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"{name}_c{int(converted)}_synth_s{seed}_v2.wts")
    sd = synth.yolov9_state(name, seed=seed, converted=bool(converted))
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def lowered(name, converted=0, **kw):
    path, _ = yolov9_wts(name, converted)
    plan = engine.build_plan(name, path, converted=converted, **kw)
    return plan, engine.describe_plan(plan, lowered=True)


def convs_of(low):
    return [o for o in low["ops"] if o["kind"] == "conv"] + [m for o in low["ops"] if o["kind"] == "conv_group" for m in o["members"]]


def without_plugin(desc):
    """oracle/graph_interp.py reads every YoloLayer_TRT blob with the YOLOv8 layout: hand it the graph up to the plugin's inputs"""
    d = copy.deepcopy(desc)
    gone = [l for l in d["layers"] if l["kind"] == gi.L_PLUGIN]
    assert len(gone) == 1 and gone[0]["plugin_type"] == "YoloLayer_TRT"
    d["layers"] = [l for l in d["layers"] if l["kind"] != gi.L_PLUGIN]
    for t in gone[0]["outputs"]:
        d["tensors"][t]["is_output"] = False
    return d


def cells_of(h, w):
    return sum((h // s) * (w // s) for s in STRIDES)


def corner_to_centre_f32(dec, max_out):
    """The conversion of the reference's nms() (yolov9/src/postprocess.cpp:59-62) on a decode buffer [B, 1 + max_out * 38]: every record's
    corner box becomes (cx, cy, w, h) by four fp32 operations - in fp32 NumPy computes exactly what C computes: one rounding per
    operation, the division by 2 exact.  Records beyond an image's count are converted as well; nothing reads them."""
    dec = np.array(dec, dtype=np.float32, copy=True)
    rec = dec[:, 1:].reshape(dec.shape[0], max_out, 38)
    x1, y1, x2, y2 = (rec[:, :, k].copy() for k in range(4))
    two = np.float32(2)
    rec[:, :, 0] = (x1 + x2) / two
    rec[:, :, 1] = (y1 + y2) / two
    rec[:, :, 2] = x2 - x1
    rec[:, :, 3] = y2 - y1
    return dec


@pytest.mark.parametrize("name,conv,B,S", [("yolov9t", 0, 2, 128), ("yolov9t", 1, 2, 128), ("yolov9s", 0, 1, 64), ("yolov9m", 0, 1, 64),
                                           ("yolov9c", 0, 1, 64), ("gelanc", 0, 1, 64)])
def test_yolov9_builder_matches_pytorch_twin(name, conv, B, S):
    """The host builder's graph (run by the oracle's interpreter) against an independent restatement of the modules.  s / m / c / gelanc
    cover CBLinear / CBFuse, ADown, and m's 240 / 120 / 60-channel blocks.  Both sides are fp32 / fp64 on the CPU: the bound is
    test_yolov5_builder_matches_pytorch_twin's."""
    path, sd = yolov9_wts(name, conv)
    plan = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1, converted=conv)
    desc = engine.describe_plan(plan)
    assert not desc["explicit_batch"]
    x = torch.from_numpy(synth.images(B, S, S, seed=5))
    out = gi.run(without_plugin(desc), plan, {"images": x.numpy()}, batch=B)
    with torch.inference_mode():
        heads, strides = Yolov9(sd, name, bool(conv)).heads(x)
    assert strides == list(STRIDES)
    assert sorted(out) == ["head0", "head1", "head2"]
    for i, h in enumerate(heads):
        got = torch.as_tensor(out[f"head{i}"])
        assert tuple(got.shape) == (B, 84, (S // strides[i]) ** 2)
        d = (got.reshape(h.shape) - h).abs().max().item()
        print(f"{name} converted={conv} head{i}: |diff| {d:.3g}, |head| {h.abs().max().item():.3g}")
        assert d < 2e-4
    # what synth.yolov9_state promises, for every model: candidates well above zero and well below the cell count, in every image
    cells = cells_of(S, S)
    dec = yp.decode_c([np.ascontiguousarray(out[f"head{i}"], dtype=np.float32).reshape(B, 84, -1) for i in range(3)], 80, S, S, list(STRIDES), cells + 1)
    print(f"{name} converted={conv} {S}x{S}: candidates per image {dec[:, 0].astype(int).tolist()} of {cells} cells")
    assert dec[:, 0].min() >= (10 if S == 128 else 5) and dec[:, 0].max() <= 0.5 * cells


@pytest.mark.parametrize("name,conv,kw", [("yolov9t", 0, dict(batch=32, h=640, w=640)), ("yolov9t", 1, dict(batch=2, h=128, w=160)),
                                          ("yolov9s", 0, dict(batch=1, h=64, w=64)), ("yolov9m", 0, dict(batch=1, h=64, w=64)),
                                          ("yolov9m", 1, dict(batch=1, h=64, w=64)), ("yolov9c", 0, dict(batch=1, h=64, w=64)),
                                          ("gelanc", 0, dict(batch=1, h=64, w=64))])
def test_yolov9_lowering_has_one_fused_head(name, conv, kw):
    for fp16 in (1, 0):
        _, low = lowered(name, conv, fp16=fp16, **kw)
        kinds = collections.Counter(o["kind"] for o in low["ops"])
        print(f"{name} converted={conv} fp16={fp16}: {dict(kinds)}")
        assert kinds["yolo9_head"] == 1 and not set(kinds) & GENERIC_KINDS, kinds
        (head,) = [o for o in low["ops"] if o["kind"] == "yolo9_head"]
        assert low["ops"][-1] is head
        H, W = kw["h"], kw["w"]
        assert (head["classes"], head["levels"]) == (80, 3)
        assert head["grids"] == [[W // s, H // s] for s in STRIDES] and head["strides"] == list(STRIDES)
        assert head["box_ld"] == [64] * 3 and head["cls_ld"] == [80] * 3
        convs = convs_of(low)
        if fp16:
            # the six grouped layers of the head: cv2.l.1 (3x3, g = 4) and the biased 1x1 cv2.l.2 (g = 4), per level
            grouped = sorted((o["k"][0], o["cin"], o["cout"]) for o in convs if o.get("grouped"))
            c2 = grouped[0][1]
            assert grouped == sorted([(1, c2, 64), (3, c2, c2)] * 3), grouped
            direct = [o for o in convs if not (o["igemm"] or o["stem"] or o.get("dw") or o.get("grouped"))]
            if name == "yolov9m":
                # 60 / 90 / 180-channel blocks: Cin is no multiple of 8 behind a channel slice, so the MFMA path declines them (DESIGN, "YOLOv9")
                print(f"{name} converted={conv}: {len(direct)} of {len(convs)} convolutions on the direct kernel: "
                      f"{sorted(collections.Counter((o['cin'], o['cout'], o['k'][0]) for o in direct).items())}")
            else:
                assert not direct, [(o["name"], o["cin"], o["cout"], o["k"]) for o in direct]


def test_yolov9_class_count_that_is_no_multiple_of_8_pads_the_class_convolutions():
    path = os.path.join(CACHE, "yolov9t_c1_nc13_synth_s0_v1.wts")
    os.makedirs(CACHE, exist_ok=True)
    wts_writer.write_wts(path, synth.yolov9_state("yolov9t", seed=0, num_class=13, converted=True), dialect="double")
    for fp16, ld in ((1, 16), (0, 16)):
        plan = engine.build_plan("yolov9t", path, batch=1, h=64, w=64, fp16=fp16, classes=13, converted=1)
        low = engine.describe_plan(plan, lowered=True)
        (head,) = [o for o in low["ops"] if o["kind"] == "yolo9_head"]
        assert head["classes"] == 13 and head["cls_ld"] == [ld] * 3 and head["box_ld"] == [64] * 3
        det = [o for o in convs_of(low) if o.get("cout_real")]
        assert [(o["cout_real"], o["cout"]) for o in det] == [(13, ld)] * 3


def test_yolov9_marked_heads_and_the_switch_keep_the_plugin(monkeypatch):
    def route(low):
        kinds = collections.Counter(o["kind"] for o in low["ops"])
        # per level: the box tensor and the class tensor to fp32 planes, and the DFL convolution's output back from NHWC
        assert kinds["plugin"] == 1 and kinds["yolo9_head"] == 0 and kinds["to_linear"] == 9 and kinds["softmax"] == 3, kinds
        assert not any(o.get("cout_real") for o in convs_of(low))
    route(lowered("yolov9t", batch=2, h=128, w=128, fp16=1, mark_heads=1)[1])
    plan, low = lowered("yolov9t", batch=2, h=128, w=128, fp16=1)
    assert collections.Counter(o["kind"] for o in low["ops"])["yolo9_head"] == 1
    monkeypatch.setenv("TRTX_YOLO9_HEAD", "0")
    route(engine.describe_plan(plan, lowered=True))


def head_net(miss=None, fp16=True, classes=5, H=64, W=96, netinfo=None, int8=False, feat=0):
    """One input per level, the DDetect tail on it: a grouped 1x1 box convolution, a class convolution, the DFL chain, the reshape, the
    concat, and the YOLOv9 plugin created from its one field.  `miss` breaks one thing the matcher checks: 'reader' (the box tensor has a
    second reader), 'output' (a class tensor is a network output), 'dfl15' (a 15-weight DFL convolution over 15 bins), 'bias' (a biased
    DFL convolution), 'seg' (isSeg = 1, with 32 more channels per cell), 'grid' (the tensors hold the transposed grid: the same cell
    count, which is all the plugin's configure checks).  feat > 0: two 3x3 convolutions + ReLU to `feat` channels feed both branches;
    int8: a kINT8 engine, every tensor calibrated from a cache (scale 0.05), so that with feat = 64 and 16 classes the class convolution
    is one whose input and output a kINT8 engine would keep in int8."""
    rng = np.random.default_rng(3)
    net = builder.Network(max_batch=2, fp16=fp16, int8=int8)
    try:
        dets = []
        bins = 15 if miss == "dfl15" else 16
        for lv, s in enumerate(STRIDES):
            gh, gw = H // s, W // s
            if miss == "grid":
                gh, gw = gw, gh
            x, cin = net.input(f"x{lv}", (16, gh, gw)), 16
            if feat:
                for c in (16, feat):   # two of them: the tensor between them has convolutions on both sides
                    x = net.out(net.activation(net.out(net.conv(x, (rng.standard_normal((feat, c, 3, 3)) / 12).astype(np.float32), bias=np.zeros(feat, np.float32), padding=1)), "relu"))
                cin = feat
            box = net.out(net.conv(x, (rng.standard_normal((4 * bins, cin // 4, 1, 1)) / 2).astype(np.float32), bias=rng.standard_normal(4 * bins).astype(np.float32), groups=4))
            cls = net.out(net.conv(x, (rng.standard_normal((classes, cin, 1, 1)) / 2).astype(np.float32), bias=rng.standard_normal(classes).astype(np.float32)))
            if miss == "reader" and lv == 0:
                net.mark_output(net.out(net.activation(box, "relu")), "aux")
            if miss == "output" and lv == 1:
                net.mark_output(cls, "aux")
            t = net.out(net.shuffle(box, reshape=(4, bins, gh * gw), perm2=(1, 0, 2)))
            t = net.out(net.softmax(t))
            t = net.out(net.conv(t, np.arange(bins, dtype=np.float32).reshape(1, bins, 1, 1), bias=np.ones(1, np.float32) if miss == "bias" else None))
            parts = [net.out(net.shuffle(t, reshape=(4, gh * gw))), net.out(net.shuffle(cls, reshape=(classes, gh * gw)))]
            if miss == "seg":
                seg = net.out(net.conv(x, (rng.standard_normal((32, cin, 1, 1)) / 2).astype(np.float32)))
                parts.append(net.out(net.shuffle(seg, reshape=(32, gh * gw))))
            dets.append(net.out(net.concat(parts)))
        fields = [("netinfo", np.array(netinfo if netinfo is not None else [classes, W, H, 50, 1 if miss == "seg" else 0], np.int32))]
        net.mark_output(net.out(net.plugin(dets, "YoloLayer_TRT", fields=fields)), "output")
        if int8:
            import struct
            from tensorrtx_amd import calibrator
            names = [t["name"] or f"(Unnamed Tensor* {t['id']})" for t in engine.describe_plan(head_net(miss, fp16, classes, H, W, netinfo, False, feat))["tensors"]]
            cache = b"TRT-8601-EntropyCalibration2\n" + b"".join(f"{nm}: {struct.unpack('<I', struct.pack('<f', 0.05))[0]:08x}\n".encode() for nm in names)
            net.set_int8_calibrator(calibrator.Calibrator(cache=cache))
        return net.build()
    finally:
        net.close()


@pytest.mark.parametrize("fp16", [True, False])
def test_small_ddetect_graph_fuses(fp16):
    low = engine.describe_plan(head_net(fp16=fp16), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    # (the three to_nhwc are the network's 16-channel inputs on their way to the convolutions)
    assert dict(kinds) == {"to_nhwc": 3, "conv": 6, "yolo9_head": 1}, kinds
    (head,) = [o for o in low["ops"] if o["kind"] == "yolo9_head"]
    assert (head["classes"], head["levels"], head["grids"], head["box_ld"]) == (5, 3, [[12, 8], [6, 4], [3, 2]], [64] * 3)
    assert head["cls_ld"] == [8] * 3   # 5 classes rounded up to 16-byte pieces: 8 halves, 8 floats
    assert [(o["cout_real"], o["cout"]) for o in convs_of(low) if o.get("cout_real")] == [(5, 8)] * 3


def test_int8_engine_keeps_the_plugin():
    """The head fuses in fp16 and fp32 engines only.  In a kINT8 engine the class convolutions (64 -> 16 here, input and output calibrated)
    would write int8, which the fused op cannot read: the plugin route stays, and its layout passes keep those outputs in fp16."""
    kw = dict(classes=16, feat=64)
    low = engine.describe_plan(head_net(**kw), lowered=True)
    assert collections.Counter(o["kind"] for o in low["ops"])["yolo9_head"] == 1   # the same graph without kINT8 fuses
    low = engine.describe_plan(head_net(int8=True, **kw), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo9_head"] == 0, kinds
    convs = convs_of(low)
    assert any(o["i8"][0] for o in convs), "the int8 graph must really run a convolution on int8 input"
    cls = [o for o in convs if o["cout"] == 16 and o["cin"] == 64]
    assert len(cls) == 3 and not any(o["i8"][1] for o in cls), [o["i8"] for o in cls]
    assert not any(t["dtype"] == 2 for o in low["ops"] if o["kind"] in ("to_linear", "plugin") for t in (low["tensors"][i] for i in o["in"]))


@pytest.mark.parametrize("miss", ["reader", "output", "dfl15", "bias", "seg", "grid"])
def test_near_miss_graphs_keep_the_plugin(miss):
    """One matcher condition broken at a time: the plugin stays, no class convolution is padded, and the plan still builds and lowers"""
    low = engine.describe_plan(head_net(miss=miss), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo9_head"] == 0, kinds
    assert not any(o.get("cout_real") for o in convs_of(low))


def test_yolov9_plugin_state_is_the_references_21_bytes():
    """Created with "netinfo"[5]; the serialized plan is read back (describe_plan deserializes the layer and serializes it again)"""
    desc = engine.describe_plan(head_net(miss="seg", classes=7, H=96, W=160))
    (pl,) = [l for l in desc["layers"] if l["kind"] == gi.L_PLUGIN]
    blob = bytes.fromhex(pl["plugin_blob"])
    assert pl["plugin_type"] == "YoloLayer_TRT" and len(blob) == 21
    # yolov9/plugin/yololayer.cu:48-60: mClassCount, mThreadCount (256), mYoloV8NetWidth, mYoloV8netHeight, mMaxOutObject, is_segmentation_
    assert np.frombuffer(blob[:20], "<i4").tolist() == [7, 256, 160, 96, 50] and blob[20] == 1
    out = [t for t in desc["tensors"] if t["is_output"] and t["name"] == "output"]
    assert out[0]["dims"] == [1 + 50 * 38, 1, 1]
    blob0 = bytes.fromhex([l for l in engine.describe_plan(head_net())["layers"] if l["kind"] == gi.L_PLUGIN][0]["plugin_blob"])
    assert len(blob0) == 21 and blob0[20] == 0 and np.frombuffer(blob0[:20], "<i4").tolist() == [5, 256, 96, 64, 50]


@pytest.mark.parametrize("netinfo", [[5, 96, 64, 50], [5, 96, 64, 50, 0, 0], [0, 96, 64, 50, 0], [5, 96, 64, 0, 0], [5, 16, 64, 50, 0]])
def test_yolov9_plugin_refuses_other_netinfo(netinfo):
    with pytest.raises(RuntimeError, match="createPlugin"):
        head_net(netinfo=netinfo)


def test_yolov9_build_errors_and_bindings():
    path, _ = yolov9_wts("yolov9t")
    bad_cases = [dict(model="yolov9q"), dict(model="yolov9e"), dict(model="gelane"), dict(model="yolov9t", h=100), dict(model="yolov9t", w=16, h=32),
                 dict(model="yolov9t", w=72), dict(model="yolov9t", batch=0), dict(model="yolov9t", classes=0), dict(model="yolov9t", max_out=0),
                 dict(model="yolov9t", task=1), dict(model="yolov9c", converted=1), dict(model="gelanc", converted=1)]
    for bad in bad_cases:
        kw = dict(batch=1)
        kw.update(bad)
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(kw.pop("model"), path, **kw)
        assert e.value.status == 1, bad   # TRTX_ERR_INVALID
    with pytest.raises(capi.TrtxError) as e:
        engine.build_plan("yolov9t", path, batch=1, h=64, w=64, int8=1)
    assert e.value.status == 4   # TRTX_ERR_UNSUPPORTED
    plan = engine.build_plan("yolov9t", path, batch=4, h=96, w=160, max_out=300)
    desc = engine.describe_plan(plan)
    io = [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_input"] or t["is_output"]]
    assert io == [("images", [3, 96, 160]), ("output", [1 + 300 * 38, 1, 1])]
    assert desc["max_batch"] == 4
    plan = engine.build_plan("yolov9t", path, batch=1, h=64, w=96, mark_heads=1)
    desc = engine.describe_plan(plan)
    io = [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_output"]]
    assert sorted(io) == [("head0", [84, 96]), ("head1", [84, 24]), ("head2", [84, 6]), ("output", [38001, 1, 1])]


def test_yolov9_state_holds_only_what_the_builder_reads():
    """Every key but BatchNorm's num_batches_tracked is read: the layers the reference creates and never connects are not in the dict"""
    for name, conv in (("yolov9t", 0), ("yolov9s", 1), ("yolov9m", 0), ("yolov9m", 1), ("yolov9c", 0), ("gelanc", 0)):
        sd = synth.yolov9_state(name, converted=bool(conv))
        layers = sorted({int(k.split(".")[1]) for k in sd})
        main = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 18, 19, 21]
        aux = [1, 2, 3, 4, 5, 6, 7, 8, 9, 23, 24, 25, 26, 27, 28, 29, 31, 32, 34, 35, 37, 38]
        want = aux if (name == "yolov9c" or (name == "yolov9m" and not conv)) else main + [29 if (name in ("yolov9t", "yolov9s") and not conv) else 22]
        assert layers == sorted(want), (name, conv, layers)


def test_yolov9_abi_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    for sym in ("trtx_yolov9_decode", "trtx_yolov9_decode_workspace", "trtx_yolov9_head_decode_workspace", "trtx_yolov9_head_decode_nhwc",
                "trtx_yolov9_head_decode_nhwc_f32", "trtx_yolov9_nms"):
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, header), sym
    L.trtx_yolov9_head_decode_workspace.restype = ctypes.c_size_t
    L.trtx_yolov9_decode_workspace.restype = ctypes.c_size_t
    cells = cells_of(64, 96)
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    assert L.trtx_yolov9_decode_workspace(2, 64, 96) == 2 * up(2 * cells * 4) + up(2 * ((cells + 511) // 512) * 4)
    assert L.trtx_yolov9_head_decode_workspace(2, 64, 96) > L.trtx_yolov9_decode_workspace(2, 64, 96)
    for name in ("yolov9_decode", "yolov9_head_decode_nhwc", "yolov9_nms"):
        assert callable(getattr(capi, name))


def test_corner_to_centre_is_the_references_four_operations():
    dec = np.zeros((1, 1 + 2 * 38), np.float32)
    dec[0, 0] = 2
    dec[0, 1:7] = [10.5, 20.25, 30.75, 41.0, 0.9, 3]
    dec[0, 39:45] = [np.float32(0.1), np.float32(0.2), np.float32(0.7), np.float32(1.1), 0.5, 1]
    got = corner_to_centre_f32(dec, 2)
    assert got[0, 1:7].tolist() == [20.625, 30.625, 20.25, 20.75, np.float32(0.9), 3.0]
    a, b = np.float32(0.1), np.float32(0.7)
    assert got[0, 39] == np.float32(np.float32(a + b) / np.float32(2)) and got[0, 41] == np.float32(b - a)
    assert dec[0, 1] == np.float32(10.5)   # the input is not modified
