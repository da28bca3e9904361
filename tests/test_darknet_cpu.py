"""Darknet YOLO (YOLOv3, YOLOv3-tiny, YOLOv4) without a GPU: the case table of tests/darknet_cases.py reaches the edges it is there for, the
three host builders record the reference's layer lists, the lowering makes one darknet_head (or, switched off, the plugin route),
IPaddingLayer infers its shape and refuses to crop, the five forms of "YoloLayer_TRT" come back from their blobs as themselves, and the
builder's refusals."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

import darknet_cases as dc
from oracle import graph_interp as gi
from tensorrtx_amd import builder, capi, engine, synth
from tensorrtx_amd import wts as wts_writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE = os.path.join(ROOT, "build", "test_cache")
MODELS = synth.DARKNET_MODELS
L_PADDING = 19


def darknet_wts(name, seed=0, num_class=80):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"{name}_nc{num_class}_synth_s{seed}_v2.wts")
    sd = synth.darknet_state(name, seed=seed, num_class=num_class)
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def convs_of(low):
    return [o for o in low["ops"] if o["kind"] == "conv"] + [m for o in low["ops"] if o["kind"] == "conv_group" for m in o["members"]]


# ---- the case table --------------------------------------------------------------------------------------------------------------------

def test_nets_are_what_they_are_for():
    a, b, c = (dc.NETS[k] for k in "ABC")
    assert [dc.cells_of(n) for n in (a, b, c)] == [22, 709, 20]
    assert a.grids[0][0] * a.grids[0][1] < 16 < dc.cells_of(a) - 1 and a.grids[-1] == (1, 1)   # both level boundaries inside the first wave's 16 cells
    assert b.grids[0][0] * b.grids[0][1] > 512 and dc.cells_of(b) > 512                        # the chunk edge inside level 0, two counters
    assert len(c.grids) == 2 and c.grids[0][0] < c.grids[1][0]                                 # coarsest first
    for classes in dc.CLASSES:
        paths = [p for _, p in dc.lds_of(classes)]
        assert "vector" in paths and "element" in paths, classes
        for ld, path in dc.lds_of(classes):
            assert ld >= 3 * (5 + classes) and (path == "vector") == (ld % 8 == 0)
    assert (255, "element") in dc.lds_of(80) and (256, "vector") in dc.lds_of(80) and (18, "element") in dc.lds_of(1)
    assert dc.lds_of(3) == [(24, "vector"), (25, "element"), (32, "vector")]


def test_every_axis_value_is_in_the_table():
    seen = {(c.net.name, c.classes, c.batch) for c in dc.cases() if c.name.startswith("random")}
    assert seen == {(n, k, b) for n in "ABC" for k in dc.CLASSES for b in dc.BATCHES}
    names = [c.name for c in dc.cases()]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c.name)
def test_case_reaches_its_edge(case):
    info = 5 + case.classes
    assert [x.shape for x in case.planes] == [(case.batch, 3 * info, gw * gh) for gw, gh in case.net.grids]
    for x in case.planes:
        assert x.dtype == np.float32 and np.array_equal(dc.fp16_values(x), x, equal_nan=True), "values must be fp16-representable"
    bp, mp, ci = dc.probabilities(case.planes, case.classes)
    anchors = 3 * dc.cells_of(case.net)
    assert bp.shape == (case.batch, anchors)
    assert not np.isnan(mp).any()
    # nothing within 1e-4 of either gate (a NaN objectness is no probability)
    assert (np.abs(mp - 0.1) > 1e-4).all(), np.abs(mp - 0.1).min()
    assert (np.isnan(bp) | (np.abs(bp - 0.1) > 1e-4)).all()
    assert np.isnan(bp).any() == case.nan, case.name
    kept = ~(mp < dc.GATE) & ~(bp < dc.GATE)
    ref = dc.reference(case.name, 0.0)
    assert np.array_equal(ref[:, 0], np.minimum(kept.sum(1), case.max_out))
    if case.name.startswith("random"):
        for b in range(case.batch):
            obj_only = (~(bp[b] < dc.GATE) & (mp[b] < dc.GATE)).sum()
            cls_only = ((bp[b] < dc.GATE) & ~(mp[b] < dc.GATE)).sum()
            # some kept, some dropped by each gate alone: the second gate is what YOLOv5's kernel does not have
            assert 0 < kept[b].sum() < anchors and obj_only > 0 and cls_only > 0, (b, kept[b].sum(), obj_only, cls_only)
            assert kept[b].sum() < case.max_out
    if case.name.startswith("full"):
        assert kept.all() and anchors > case.max_out and (ref[:, 0] == case.max_out).all()
    if case.name.startswith("planted"):
        assert case.batch == 3 and kept[1].sum() == 0 and ref[1, 0] == 0, "image 1 is the empty one"
        assert len(case.planted) >= 10
        for b, g, want, cls, what in case.planted:
            assert bool(kept[b, g]) == want, what
            if want and cls is not None:
                assert ci[b, g] == cls, what
        if case.max_out > 1:
            rec = dc.records(ref[0])
            assert len(rec) == kept[0].sum() == sum(1 for p in case.planted if p[2])
            assert np.isnan(rec[:, 4]).sum() == 1 and np.isinf(rec[:, 2]).sum() == 1 and np.isnan(rec[:, 1]).sum() == 1
            assert not np.isnan(rec[:, 6]).any() and (rec[:, 6] >= dc.GATE).all()
            near = np.abs(rec[:, 4] - 0.1) < 0.006
            assert near.sum() == 1 and (np.abs(rec[:, 6] - 0.1) < 0.006).sum() == 1   # the two records just above a gate
        else:
            assert ref[0, 0] == 1 and ref[2, 0] == 1 and kept[0].sum() > 1


def test_restatement_by_hand():
    """one anchor, worked through: Logist in double, (col + p) * net_w / grid_w, exp(tw) * anchor, two stored probabilities"""
    net = dc.Net("hand", [(2, 1)], 64, 32, [[10, 20, 30, 40, 50, 60]])
    x = np.full((1, 3 * 6, 2), -9.0, np.float32)
    x[0, 6:12, 1] = [0.5, -0.25, 0.125, 1.0, 2.0, 1.5]   # anchor 1 of cell 1
    out = dc.decode_ref([x], 1, net, 4, fill=-1.0)
    assert out[0, 0] == 1 and (out[0, 8:] == -1.0).all()
    sg = lambda v: np.float32(1.0 / (1.0 + float(np.exp(np.float32(-v)))))  # noqa: E731
    want = [(np.float32(1) + sg(0.5)) * np.float32(64) / np.float32(2), (np.float32(0) + sg(-0.25)) * np.float32(32) / np.float32(1),
            np.exp(np.float32(0.125)) * np.float32(30), np.exp(np.float32(1.0)) * np.float32(40), sg(2.0), 0.0, sg(1.5)]
    assert np.array_equal(out[0, 1:8], np.array(want, np.float32))


# ---- the builders ----------------------------------------------------------------------------------------------------------------------

EXPECT = {   # convolutions with BatchNorm, of which Mish; shortcuts; concatenations; pools; upsamples; pads; detect modules
    "yolov3": dict(conv=72, mish=0, add=23, cat=2, pool=0, up=2, pad=0, det=(81, 93, 105)),
    "yolov3-tiny": dict(conv=11, mish=0, add=0, cat=1, pool=6, up=1, pad=1, det=(15, 22)),
    "yolov4": dict(conv=107, mish=72, add=23, cat=10, pool=3, up=2, pad=0, det=(138, 149, 160)),
}


# Rows read off the reference files themselves, line by line - [module, kind, channels, k, s, p, from]: the two tables are generated by helpers
# of the same shape, so what pins them is this list (and the counts above), not their agreement with each other.
PINNED = {
    "yolov3": [   # yolov3/yolov3.cpp:201-325
        [0, "L", 32, 3, 1, 1, []], [1, "L", 64, 3, 2, 1, []], [2, "L", 32, 1, 1, 0, []], [3, "L", 64, 3, 1, 1, []], [4, "S", 0, 0, 0, 0, [3, 1]],
        [11, "S", 0, 0, 0, 0, [10, 8]], [12, "L", 256, 3, 2, 1, []], [36, "S", 0, 0, 0, 0, [35, 33]], [37, "L", 512, 3, 2, 1, []],
        [61, "S", 0, 0, 0, 0, [60, 58]], [62, "L", 1024, 3, 2, 1, []], [74, "S", 0, 0, 0, 0, [73, 71]], [75, "L", 512, 1, 1, 0, []],
        [80, "L", 1024, 3, 1, 1, []], [83, "R", 0, 0, 0, 0, [79]], [84, "L", 256, 1, 1, 0, []], [86, "R", 0, 0, 0, 0, [85, 61]],
        [87, "L", 256, 1, 1, 0, []], [92, "L", 512, 3, 1, 1, []], [95, "R", 0, 0, 0, 0, [91]], [96, "L", 128, 1, 1, 0, []],
        [98, "R", 0, 0, 0, 0, [97, 36]], [99, "L", 128, 1, 1, 0, []], [104, "L", 256, 3, 1, 1, []]],
    "yolov3-tiny": [   # yolov3-tiny/yolov3-tiny.cpp:232-273
        [0, "L", 16, 3, 1, 1, []], [1, "P", 0, 2, 2, 0, []], [8, "L", 256, 3, 1, 1, []], [9, "P", 0, 2, 2, 0, []], [10, "L", 512, 3, 1, 1, []],
        [11, "Z", 0, 0, 0, 0, []], [12, "L", 1024, 3, 1, 1, []], [13, "L", 256, 1, 1, 0, []], [14, "L", 512, 3, 1, 1, []], [17, "R", 0, 0, 0, 0, [13]],
        [18, "L", 128, 1, 1, 0, []], [20, "R", 0, 0, 0, 0, [19, 8]], [21, "L", 256, 3, 1, 1, []]],
    "yolov4": [   # yolov4/yolov4.cpp:243-467
        [0, "M", 32, 3, 1, 1, []], [1, "M", 64, 3, 2, 1, []], [2, "M", 64, 1, 1, 0, []], [3, "R", 0, 0, 0, 0, [1]], [4, "M", 64, 1, 1, 0, []],
        [5, "M", 32, 1, 1, 0, []], [6, "M", 64, 3, 1, 1, []], [7, "S", 0, 0, 0, 0, [6, 4]], [8, "M", 64, 1, 1, 0, []], [9, "R", 0, 0, 0, 0, [8, 2]],
        [10, "M", 64, 1, 1, 0, []], [11, "M", 128, 3, 2, 1, []], [12, "M", 64, 1, 1, 0, []], [15, "M", 64, 1, 1, 0, []], [16, "M", 64, 3, 1, 1, []],
        [20, "S", 0, 0, 0, 0, [19, 17]], [22, "R", 0, 0, 0, 0, [21, 12]], [23, "M", 128, 1, 1, 0, []], [53, "R", 0, 0, 0, 0, [52, 25]],
        [54, "M", 256, 1, 1, 0, []], [84, "R", 0, 0, 0, 0, [83, 56]], [85, "M", 512, 1, 1, 0, []], [86, "M", 1024, 3, 2, 1, []],
        [89, "M", 512, 1, 1, 0, []], [103, "R", 0, 0, 0, 0, [102, 87]], [104, "M", 1024, 1, 1, 0, []], [105, "L", 512, 1, 1, 0, []],
        [106, "L", 1024, 3, 1, 1, []], [107, "L", 512, 1, 1, 0, []], [108, "P", 0, 5, 1, 2, []], [109, "R", 0, 0, 0, 0, [107]],
        [110, "P", 0, 9, 1, 4, []], [112, "P", 0, 13, 1, 6, []], [113, "R", 0, 0, 0, 0, [112, 110, 108, 107]], [117, "L", 256, 1, 1, 0, []],
        [119, "R", 0, 0, 0, 0, [85]], [120, "L", 256, 1, 1, 0, []], [121, "R", 0, 0, 0, 0, [120, 118]], [126, "L", 256, 1, 1, 0, []],
        [127, "L", 128, 1, 1, 0, []], [129, "R", 0, 0, 0, 0, [54]], [131, "R", 0, 0, 0, 0, [130, 128]], [137, "L", 256, 3, 1, 1, []],
        [140, "R", 0, 0, 0, 0, [136]], [141, "L", 256, 3, 2, 1, []], [142, "R", 0, 0, 0, 0, [141, 126]], [148, "L", 512, 3, 1, 1, []],
        [151, "R", 0, 0, 0, 0, [147]], [152, "L", 512, 3, 2, 1, []], [153, "R", 0, 0, 0, 0, [152, 116]], [159, "L", 1024, 3, 1, 1, []]],
}


@pytest.mark.parametrize("name", MODELS)
def test_module_tables_agree_and_name_the_references_modules(name):
    rows = synth.darknet_rows(name)
    assert engine.darknet_rows(name) == rows, "host/darknet.cpp and synth.darknet_rows restate the same cfg"
    assert engine.darknet_rows(name) == rows, "a second call returns its own string"
    for want in PINNED[name]:
        assert rows[want[0]] == want, (name, rows[want[0]], want)
    e = EXPECT[name]
    kinds = collections.Counter(r[1] for r in rows)
    assert kinds["L"] + kinds["M"] == e["conv"] and kinds["M"] == e["mish"] and kinds["S"] == e["add"] and kinds["U"] == e["up"]
    assert kinds["P"] + kinds["Z"] == e["pool"] and kinds["Z"] == e["pad"]
    assert len([r for r in rows if r[1] == "R" and len(r[6]) > 1]) == e["cat"]
    assert tuple(r[0] for r in rows if r[1] == "D") == e["det"]
    assert all(rows[i + 1][1] == "Y" for i in e["det"]), "a yolo module behind every detect convolution"
    with pytest.raises(ValueError):
        engine.darknet_rows("yolov3-spp")


@pytest.mark.parametrize("name,H,W,nc", [("yolov3", 64, 64, 80), ("yolov3-tiny", 96, 64, 80), ("yolov3-tiny", 64, 64, 3), ("yolov4", 64, 96, 80)])
def test_builder_records_the_references_layers(name, H, W, nc):
    path, sd = darknet_wts(name, num_class=nc)
    plan = engine.build_plan(name, path, batch=2, h=H, w=W, fp16=1, mark_heads=1, classes=nc)
    desc = engine.describe_plan(plan)
    assert not desc["explicit_batch"] and desc["max_batch"] == 2
    e = EXPECT[name]
    kinds = collections.Counter(l["kind"] for l in desc["layers"])
    nd = len(e["det"])
    assert kinds[gi.L_CONV] == e["conv"] + nd and kinds[gi.L_SCALE] == e["conv"]
    assert kinds[gi.L_ACTIVATION] == e["conv"] - e["mish"] and kinds[gi.L_ELEMENTWISE] == e["add"] and kinds[gi.L_CONCAT] == e["cat"]
    assert kinds[gi.L_POOLING] == e["pool"] and kinds[gi.L_DECONV] == e["up"] and kinds.get(L_PADDING, 0) == e["pad"]
    plugins = [l for l in desc["layers"] if l["kind"] == gi.L_PLUGIN]
    assert collections.Counter(p["plugin_type"] for p in plugins) == ({"Mish_TRT": e["mish"], "YoloLayer_TRT": 1} if e["mish"] else {"YoloLayer_TRT": 1})
    assert sum(kinds.values()) == sum(kinds[k] for k in (gi.L_CONV, gi.L_SCALE, gi.L_ACTIVATION, gi.L_ELEMENTWISE, gi.L_CONCAT, gi.L_POOLING, gi.L_DECONV,
                                                          gi.L_PLUGIN)) + e["pad"]
    for l in desc["layers"]:
        if l["kind"] == gi.L_ACTIVATION:
            assert l["op"] == 3 and l["alpha"] == pytest.approx(0.1), "kLEAKY_RELU with alpha 0.1"
        if l["kind"] == gi.L_DECONV:
            assert l["kernel"] == [2, 2] and l["stride"] == [2, 2] and l["groups"] == l["nb_out"] and l["w"][0][1] == 4 * l["nb_out"]
    # every weight key the builder reads is one the state holds, under its module number
    names = {l["name"] for l in desc["layers"] if l["kind"] == gi.L_CONV}
    assert names == {k[:-len(".weight")] for k in sd if k.endswith(".Conv2d.weight")}
    # the detect convolutions, in the plugin's input order, are the marked heads
    (yolo,) = [p for p in plugins if p["plugin_type"] == "YoloLayer_TRT"]
    by_out = {l["outputs"][0]: l for l in desc["layers"]}
    dets = [by_out[t] for t in yolo["inputs"]]
    assert [d["name"] for d in dets] == [f"module_list.{i}.Conv2d" for i in e["det"]]
    strides = synth.DARKNET_STRIDES[name]
    for j, (d, s) in enumerate(zip(dets, strides)):
        assert d["nb_out"] == 3 * (5 + nc) and d["kernel"] == [1, 1] and d["w"][1][1] == d["nb_out"], "biased 1x1, 3 * (classes + 5) outputs"
        t = desc["tensors"][d["outputs"][0]]
        assert (t["name"], t["dims"], t["is_output"]) == (f"head{j}", [3 * (5 + nc), H // s, W // s], True)
    io = [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_input"] or (t["is_output"] and t["name"] == "prob")]
    assert io == [("data", [3, H, W]), ("prob", [1 + 1000 * 7, 1, 1])]
    # the plugin's state: the reference's blob (classCount, threadCount, kernelCount, YoloKernels) and the net size behind it
    blob = bytes.fromhex(yolo["plugin_blob"])
    assert len(blob) == 20 + 32 * nd
    assert np.frombuffer(blob[:12], "<i4").tolist() == [nc, 256, nd] and np.frombuffer(blob[-8:], "<i4").tolist() == [W, H]
    for j, s in enumerate(strides):
        k = blob[12 + 32 * j:44 + 32 * j]
        assert np.frombuffer(k[:8], "<i4").tolist() == [W // s, H // s]
        assert np.frombuffer(k[8:], "<f4").tolist() == [float(v) for v in synth.DARKNET_ANCHORS[name][j]]
    if e["pad"]:
        (pad,) = [l for l in desc["layers"] if l["kind"] == L_PADDING]
        assert pad["start"] == [0, 0] and pad["size"] == [1, 1]
        tin, tout = desc["tensors"][pad["inputs"][0]], desc["tensors"][pad["outputs"][0]]
        assert tout["dims"] == [512, H // 32 + 1, W // 32 + 1] and tin["dims"] == [512, H // 32, W // 32]
        (pool,) = [l for l in desc["layers"] if l["kind"] == gi.L_POOLING and l["inputs"] == pad["outputs"]]
        assert pool["kernel"] == [2, 2] and pool["stride"] == [1, 1] and pool["padding"] == [0, 0]
        assert desc["tensors"][pool["outputs"][0]]["dims"] == tin["dims"]
    if name == "yolov4":
        spp = [l for l in desc["layers"] if l["kind"] == gi.L_POOLING]
        assert [(l["kernel"], l["stride"], l["padding"]) for l in spp] == [([k, k], [1, 1], [k // 2, k // 2]) for k in (5, 9, 13)]
        assert len({tuple(l["inputs"]) for l in spp}) == 1
        (cat,) = [l for l in desc["layers"] if l["kind"] == gi.L_CONCAT and len(l["inputs"]) == 4]
        assert cat["inputs"] == [spp[2]["outputs"][0], spp[1]["outputs"][0], spp[0]["outputs"][0], spp[0]["inputs"][0]], "13, 9, 5, then the input"


@pytest.mark.parametrize("name", MODELS)
def test_lowered_plans(name, monkeypatch):
    path, _ = darknet_wts(name)
    nd = len(EXPECT[name]["det"])
    for fp16 in (1, 0):
        low = engine.describe_plan(engine.build_plan(name, path, batch=2, h=64, w=64, fp16=fp16), lowered=True)
        kinds = collections.Counter(o["kind"] for o in low["ops"])
        assert kinds["darknet_head"] == 1 and kinds["plugin"] == 0 and kinds["to_linear"] == 0 and kinds["to_nhwc"] == 0, (fp16, kinds)
        (head,) = [o for o in low["ops"] if o["kind"] == "darknet_head"]
        assert (head["classes"], head["levels"], head["anchor_levels"]) == (80, nd, nd)
        assert head["grids"] == [[64 // s, 64 // s] for s in synth.DARKNET_STRIDES[name]] and head["ld"] == [256] * nd
        assert [(o["cout_real"], o["cout"]) for o in convs_of(low) if o.get("cout_real")] == [(255, 256)] * nd
        # the first convolution: 3 input channels, 3x3 stride 1, on the stem kernel in fp16 and fp32 (no layout pass in front of it), with its activation folded in
        first = low["ops"][0]
        assert first["kind"] == "conv" and first["stem"] and not first["igemm"] and (first["cin"], first["k"], first["stride"]) == (3, [3, 3], [1, 1])
        assert first["cout"] == (16 if name == "yolov3-tiny" else 32)
        assert (first["act1"], first["alpha1"]) == ((6, 0) if name == "yolov4" else (4, pytest.approx(0.1))), "ACT_MISH / ACT_LEAKY as the epilogue"
        acts = collections.Counter(o["act1"] for o in convs_of(low))
        e = EXPECT[name]
        assert acts == {k: v for k, v in ((6, e["mish"]), (4, e["conv"] - e["mish"]), (0, nd)) if v}, "every Mish_TRT and LeakyReLU is an epilogue"
        assert kinds["act_nhwc"] == 0 and kinds["deconv"] == 0, "the all-ones deconvolutions are upsamples"
        assert kinds["pad_nhwc"] == e["pad"]
        if name == "yolov4":
            assert kinds["pool_chain"] == 1 and kinds["pool"] == 0
        if name == "yolov3-tiny":
            (pad,) = [o for o in low["ops"] if o["kind"] == "pad_nhwc"]
            assert pad["pre"] == [0, 0] and low["tensors"][pad["out"][0]]["dims"] == [512, 3, 3]
            nxt = low["ops"][low["ops"].index(pad) + 1]
            assert nxt["kind"] == "pool" and nxt["in"] == pad["out"] and nxt["k"] == [2, 2] and nxt["stride"] == [1, 1], "the pad is an op of its own in front of the pool"
    monkeypatch.setenv("TRTX_DARKNET_HEAD", "0")
    low = engine.describe_plan(engine.build_plan(name, path, batch=2, h=64, w=64, fp16=1), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["darknet_head"] == 0 and kinds["to_linear"] == nd, kinds
    monkeypatch.delenv("TRTX_DARKNET_HEAD")
    low = engine.describe_plan(engine.build_plan(name, path, batch=2, h=64, w=64, fp16=1, mark_heads=1), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["darknet_head"] == 0 and kinds["to_linear"] == nd, "marked heads keep the plugin"


def test_build_refusals_and_bindings():
    path, _ = darknet_wts("yolov3-tiny")
    for bad in (dict(max_out=999), dict(max_out=1001), dict(max_out=0), dict(h=100), dict(w=72), dict(h=16, w=32), dict(batch=0), dict(classes=0), dict(task=1)):
        kw = dict(batch=1, h=64, w=64)
        kw.update(bad)
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan("yolov3-tiny", path, **kw)
        assert e.value.status == 1, bad   # TRTX_ERR_INVALID
    for name in MODELS:
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(name, path, batch=1, h=64, w=64, int8=1)
        assert e.value.status == 4, name   # TRTX_ERR_UNSUPPORTED
    for name in ("yolov3-spp", "yolov4-tiny", "yolov3tiny"):
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(name, path, batch=1, h=64, w=64)
        assert e.value.status == 1, name   # an unknown name answers as it always has
    plan = engine.build_plan("yolov3-tiny", path, batch=4, h=96, w=160, max_out=1000)
    desc = engine.describe_plan(plan)
    assert [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_input"] or t["is_output"]] == [("data", [3, 96, 160]), ("prob", [7001, 1, 1])]
    assert desc["max_batch"] == 4


def test_state_holds_only_what_the_builder_reads():
    for name in MODELS:
        sd = synth.darknet_state(name)
        e = EXPECT[name]
        assert len([k for k in sd if k.endswith(".Conv2d.weight")]) == e["conv"] + len(e["det"])
        assert len([k for k in sd if k.endswith(".running_var")]) == e["conv"]
        assert sorted(int(k.split(".")[1]) for k in sd if k.endswith(".Conv2d.bias")) == list(e["det"])
        assert all(re.fullmatch(r"module_list\.\d+\.(Conv2d\.(weight|bias)|BatchNorm2d\.(weight|bias|running_mean|running_var|num_batches_tracked))", k) for k in sd)


# ---- IPaddingLayer ---------------------------------------------------------------------------------------------------------------------

def pad_net(pre, post, chw=(8, 5, 7), fp16=True, pool=True):
    net = builder.Network(max_batch=2, fp16=fp16)
    try:
        x = net.input("x", chw)
        y = net.out(net.padding(x, pre, post))
        net.mark_output(y, "padded")
        if pool:
            net.mark_output(net.out(net.pooling(y, 2, 1)), "pooled")
        return net.build()
    finally:
        net.close()


@pytest.mark.parametrize("pre,post", [((0, 0), (1, 1)), ((2, 1), (0, 3)), ((0, 0), (0, 0))])
def test_padding_layer_infers_its_shape(pre, post):
    plan = pad_net(pre, post)
    desc = engine.describe_plan(plan)
    (pad,) = [l for l in desc["layers"] if l["kind"] == L_PADDING]
    assert pad["start"] == list(pre) and pad["size"] == list(post)
    H, W = 5 + pre[0] + post[0], 7 + pre[1] + post[1]
    outs = {t["name"]: t["dims"] for t in desc["tensors"] if t["is_output"]}
    assert outs == {"padded": [8, H, W], "pooled": [8, H - 1, W - 1]}
    low = engine.describe_plan(plan, lowered=True)
    kinds = [o["kind"] for o in low["ops"]]
    assert kinds[:2] == ["to_nhwc", "pad_nhwc"] and sorted(kinds[2:]) == ["pool", "to_linear", "to_linear"], kinds
    (op,) = [o for o in low["ops"] if o["kind"] == "pad_nhwc"]
    assert op["pre"] == list(pre)
    # a plan with the new layer kind comes back from its bytes as itself
    assert engine.describe_plan(plan)["layers"] == desc["layers"]


@pytest.mark.parametrize("pre,post", [((-1, 0), (1, 1)), ((0, 0), (0, -2))])
def test_cropping_pad_is_refused_at_build_time(pre, post, capfd):
    with pytest.raises(capi.TrtxError) as e:
        pad_net(pre, post)
    assert e.value.status == 1   # TRTX_ERR_INVALID, and the builder's log says why
    assert "negative (cropping) padding is not implemented" in capfd.readouterr().err


# ---- the plugin's forms ----------------------------------------------------------------------------------------------------------------

def darknet_head_net(order="v4", classes=5, H=64, W=96, fp16=True, miss=None):
    """one 16-channel input per level, a biased 1x1 detect convolution on it, and YoloLayer_TRT created with no fields.
    order: 'v4' (strides 8, 16, 32), 'v3' (32, 16, 8), 'tiny' (32, 16), or a miss: 'one' (a single input), 'same' (three inputs of one size),
    'mixed' (16, 8, 32)"""
    strides = dict(v4=(8, 16, 32), v3=(32, 16, 8), tiny=(32, 16), one=(32,), same=(16, 16, 16), mixed=(16, 8, 32))[order]
    rng = np.random.default_rng(3)
    net = builder.Network(max_batch=2, fp16=fp16)
    try:
        dets = []
        info = 3 * (5 + classes) + (1 if miss == "channels" else 0)
        for lv, s in enumerate(strides):
            x = net.input(f"x{lv}", (16, H // s, W // s))
            dets.append(net.out(net.conv(x, (rng.standard_normal((info, 16, 1, 1)) / 2).astype(np.float32), bias=rng.standard_normal(info).astype(np.float32))))
        net.mark_output(net.out(net.plugin(dets, "YoloLayer_TRT")), "prob")
        return net.build()
    finally:
        net.close()


@pytest.mark.parametrize("order,table", [("v4", "yolov4"), ("v3", "yolov3"), ("tiny", "yolov3-tiny")])
def test_zero_field_plugin_learns_its_family_from_its_inputs(order, table):
    plan = darknet_head_net(order)
    desc = engine.describe_plan(plan)
    (pl,) = [l for l in desc["layers"] if l["kind"] == gi.L_PLUGIN]
    blob = bytes.fromhex(pl["plugin_blob"])
    n = len(synth.DARKNET_STRIDES[table])
    assert len(blob) == 20 + 32 * n and np.frombuffer(blob[:12], "<i4").tolist() == [5, 256, n] and np.frombuffer(blob[-8:], "<i4").tolist() == [96, 64]
    for j, s in enumerate(synth.DARKNET_STRIDES[table]):
        k = blob[12 + 32 * j:44 + 32 * j]
        assert np.frombuffer(k[:8], "<i4").tolist() == [96 // s, 64 // s]
        assert np.frombuffer(k[8:], "<f4").tolist() == [float(v) for v in synth.DARKNET_ANCHORS[table][j]]
    assert [t for t in desc["tensors"] if t["is_output"]][0]["dims"] == [7001, 1, 1]
    low = engine.describe_plan(plan, lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert dict(kinds) == {"to_nhwc": n, "conv": n, "darknet_head": 1}, kinds
    (head,) = [o for o in low["ops"] if o["kind"] == "darknet_head"]
    assert head["ld"] == [32] * n and head["classes"] == 5


@pytest.mark.parametrize("order,miss", [("one", None), ("same", None), ("mixed", None), ("v4", "channels")])
def test_zero_field_plugin_refuses_other_inputs(order, miss):
    with pytest.raises(Exception):
        darknet_head_net(order, miss=miss)


def test_five_forms_come_back_as_themselves():
    """YOLOv8's (35 + 4 n bytes), YOLOv5's (25 + 32 n), YOLOv9's (21), YOLOv7's (24 + 32 n) and Darknet's (20 + 32 n): each plan is read back
    (describe_plan deserializes every layer and serializes it again) with its own blob and its own record length"""
    import test_yolov7_cpu as t7
    import test_yolov9_cpu as t9
    from util import synth_wts
    seen = {}
    d = engine.describe_plan(t7.head_net(miss="netinfo5", classes=7))
    seen["v5"] = (d, 25 + 32 * 3, 1 + 50 * 38)
    d = engine.describe_plan(t7.head_net(classes=7))
    seen["v7"] = (d, 24 + 32 * 3, 1 + 50 * 6)
    d = engine.describe_plan(t9.head_net())
    seen["v9"] = (d, 21, 1 + 50 * 38)
    d = engine.describe_plan(darknet_head_net("v3"))
    seen["darknet"] = (d, 20 + 32 * 3, 1 + 1000 * 7)
    path, _ = synth_wts("yolov8n")
    d = engine.describe_plan(engine.build_plan("yolov8n", path, batch=1, h=64, w=64, fp16=1))
    seen["v8"] = (d, 35 + 4 * 3, None)
    for form, (d, size, floats) in seen.items():
        (pl,) = [l for l in d["layers"] if l["kind"] == gi.L_PLUGIN]
        assert pl["plugin_type"] == "YoloLayer_TRT" and len(bytes.fromhex(pl["plugin_blob"])) == size, form
        if floats:
            assert [t for t in d["tensors"] if t["is_output"]][0]["dims"] == [floats, 1, 1], form
    lengths = {"v8": {35 + 4 * n for n in range(0, 9)}, "v5": {25 + 32 * n for n in range(1, 9)}, "v9": {21}, "v7": {24 + 32 * n for n in range(1, 9)},
               "darknet": {20 + 32 * n for n in range(0, 9)}}
    for a in lengths:
        for b in lengths:
            assert a == b or not (lengths[a] & lengths[b]), (a, b)


def test_abi_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    for sym in ("trtx_darknet_decode_workspace", "trtx_darknet_decode", "trtx_darknet_head_decode_workspace", "trtx_darknet_head_decode_nhwc",
                "trtx_darknet_head_decode_nhwc_f32", "trtx_darknet_nms", "trtx_add_padding"):
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, header), sym
    L.trtx_darknet_decode_workspace.restype = ctypes.c_size_t
    L.trtx_darknet_head_decode_workspace.restype = ctypes.c_size_t
    L.trtx_yolov7_decode_workspace.restype = ctypes.c_size_t
    gw, gh = (ctypes.c_int * 2)(12, 6), (ctypes.c_int * 2)(8, 4)
    assert L.trtx_darknet_decode_workspace(2, gw, gh, 2) == L.trtx_darknet_head_decode_workspace(2, gw, gh, 2) == L.trtx_yolov7_decode_workspace(2, gw, gh, 2) > 0
    assert L.trtx_darknet_decode_workspace(2, gw, gh, 9) == 0
    for name in ("darknet_decode", "darknet_head_decode_nhwc", "darknet_head_decode_workspace", "darknet_nms"):
        assert callable(getattr(capi, name))
    assert capi.DARKNET_DET_FLOATS == dc.DET == 7
