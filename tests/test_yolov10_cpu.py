"""YOLOv10 without a GPU: the case tables reach the edges they name (on the restatements' output), the 6-float plugin form and its blob, the
host builder's six models (plans, weight names, lowered ops with and without the two switches), the RepVGGDW fold's arithmetic, the new
symbols, and the refusals that happen before the device is touched."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from tensorrtx_amd import builder, capi, engine, synth
from tensorrtx_amd import wts as wts_writer
from tests import yolov10_cases as yc
from util import CACHE
from yolov10_twin import STAGES, Yolov10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = synth.YOLOV10_MODELS


def yolov10_wts(name, seed=0):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"{name}_synth_v1_s{seed}.wts")
    sd = synth.yolov10_state(name, seed=seed)
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def lowered(name, **kw):
    path, _ = yolov10_wts(name)
    plan = engine.build_plan(name, path, **kw)
    return plan, engine.describe_plan(plan, lowered=True)


def convs_of(low):
    return [o for o in low["ops"] if o["kind"] == "conv"] + [m for o in low["ops"] if o["kind"] == "conv_group" for m in o["members"]]


# ---- the tables ------------------------------------------------------------------------------------------------------------------------

def test_decode_table_covers_what_it_claims():
    cs = yc.DECODE_CASES
    assert {c.family for c in cs} == set(yc.FAMILIES)
    assert {c.classes for c in cs} == {80, 8, 3, 1} and {c.B for c in cs} == {1, 2, 3} and {c.max_out for c in cs} == {1, 7, 1000}
    assert {len(c.net[2]) for c in cs} == {1, 2, 3}
    assert yc.level_cells("5x7") == [35] and yc.level_cells("3x3+1x1") == [9, 1]
    off = yc.level_offsets("126")
    assert 64 < off[1] < 128 and 64 < off[2] < 128, "both level boundaries inside the second wave"
    assert yc.cells_of("525") > 512, "more than one emit chunk"


@pytest.mark.parametrize("dt", yc.DTYPES)
@pytest.mark.parametrize("case", yc.DECODE_CASES, ids=lambda c: c.name)
def test_decode_case_reaches_its_edge(case, dt):
    bt, ref = yc.build(case.name, dt), yc.reference(case.name, dt)
    H, W, strides = case.net
    n = ref[:, 0].astype(int)
    kept = yc.kept_cells(case.name, dt)
    free = yc.reference(case.name, dt, max_out=case.cells + 1)
    assert [len(k) for k in kept] == free[:, 0].astype(int).tolist(), "the restatement's gate against float64"
    assert (n == np.minimum(free[:, 0], case.max_out)).all()
    for b in range(case.B):   # a clamped row holds the first max_out records of the canonical order
        assert np.array_equal(yc.records(ref, b), yc.records(free, b)[:case.max_out], equal_nan=True)
        assert not ref[b, 1 + n[b] * yc.REC:].any()
    # nothing of the table sits where a device expf could decide differently, but for the gate cells, which are placed on purpose
    with np.errstate(all="ignore"):
        m = np.nan_to_num(bt.logits.astype(np.float64), nan=-np.inf).max(-1)
        p = 1.0 / (1.0 + np.exp(-m))
    # (3e-6 is 400 ulps of 0.1; the fp32 gate cells sit 16 float steps of the logit = 45 ulps of p = 3.4e-7 off, a device expf is good to one)
    assert (np.abs(p - yc.GATE) > (3e-7 if case.family == "gate" else 3e-6)).all(), float(np.abs(p - yc.GATE).min())
    fam = case.family
    if fam == "seeded":
        assert (free[:, 0] >= 1).all() and (free[:, 0] < case.cells).all(), free[:, 0]
    elif fam == "empty":
        assert (n == 0).all()
    elif fam == "full":
        assert (n == case.cells).all()
        assert len({tuple(yc.records(ref, b)[:, 5]) for b in range(case.B)}) == (case.B if case.classes > 1 else 1)
    elif fam == "overflow":
        assert n[0] == case.max_out < free[0, 0] == case.cells
    elif fam == "gate":
        placed = bt.expect["gate"]
        assert {k for _, k in placed.values()} == {True, False}
        for (b, g), (v, keep) in placed.items():
            assert (g in kept[b]) == keep, (b, g, v)
            assert bt.logits[b, g].max() == np.float32(v), "the storage type holds the value exactly"
    elif fam == "ties":
        for b in range(case.B):
            assert np.array_equal(yc.records(ref, b)[:, 5], bt.expect["classes"][b]) and n[b] == case.cells
        assert (bt.expect["classes"][case.B - 1][0] > 0) or case.classes == 1
    elif fam == "naninf":
        for b, g in bt.expect["dropped"] + bt.expect["neginf"]:
            assert g not in kept[b]
        for b, g, cls in bt.expect["nan_beside"]:
            r = yc.records(ref, b)[list(kept[b]).index(g)]
            assert r[5] == cls and np.isfinite(r[4])
        for b, g in bt.expect["inf"]:
            assert yc.records(ref, b)[list(kept[b]).index(g), 4] == 1.0
    elif fam == "dfl":
        st = yc.cell_strides(case.geom)
        for b, g, idx in bt.expect["onehot"]:
            r = yc.records(ref, b)[list(kept[b]).index(g)]
            assert np.allclose((r[2] - r[0]) / st[g], 2 * bt.dfl_w[idx], rtol=1e-6), "both sides are dfl_w[idx] wide"


def test_topk_table_covers_what_it_claims():
    cs = yc.TOPK_CASES
    counts = {n for c in cs for n in c.counts}
    assert {0, 1, 63, 64, 65, 1000, yc.CAP} <= counts and any(n > c.max_out for c in cs for n in c.counts)
    assert any(c.topk < 0 for c in cs) and any(c.topk == 0 for c in cs) and any(c.topk == 1 for c in cs)
    for c in cs:
        dec = yc.topk_input(c.name)
        out = yc.topk_ref(dec, c.max_out, c.thresh, c.topk)
        free = yc.topk_ref(dec, c.max_out, c.thresh, 0)
        for b in range(dec.shape[0]):
            got, all_ = yc.records(out, b), yc.records(free, b)
            assert len(got) == (min(c.topk, len(all_)) if c.topk > 0 else len(all_))
            assert (got[:, 4] > np.float32(c.thresh)).all() and not np.isnan(got[:, 4]).any()
            if c.topk > 0 and len(got) > 1:
                assert (np.diff(got[:, 4]) <= 0).all()
        if c.kind == "at_thresh":
            r = dec[0, 1:].reshape(-1, yc.REC)
            kept = {tuple(x) for x in yc.records(free, 0)}
            assert tuple(r[1]) not in kept and tuple(r[5]) not in kept and tuple(r[3]) in kept
        if c.kind == "ties":
            g = yc.records(out, 0)
            assert (g[:, 4] == g[0, 4]).all() and (yc.records(free, 0)[:, 4] == g[0, 4]).sum() > c.topk, "the cut falls inside a tie"
            src = dec[0, 1:].reshape(-1, yc.REC)
            slots = [int(np.nonzero((src == r).all(1))[0][0]) for r in g]
            assert slots == sorted(slots), "ties in slot order"
        if c.kind == "nan":
            assert np.isnan(dec[0, 1 + 4]) and len(yc.records(free, 0)) < c.counts[0]
    tk = yc.TOPK_BY_NAME
    assert yc.topk_ref(yc.topk_input("topk_equals_survivors"), 64, -1.0, 30)[0, 0] == 30
    assert yc.topk_ref(yc.topk_input("topk_one_below_survivors"), 64, -1.0, 29)[0, 0] == 29
    assert yc.topk_ref(yc.topk_input("topk_above_survivors"), 64, -1.0, 31)[0, 0] == 30
    assert yc.topk_ref(yc.topk_input("header_above_max_out"), 8, -1.0, 0)[0, 0] == 8 and tk["header_above_max_out"].counts[0] > 8


# ---- the plugin form -------------------------------------------------------------------------------------------------------------------

def head_net(info=None, classes=5, H=64, W=96, strides=(8, 16, 32), B=2, name="combinedInfo"):
    """one (B, 4 + classes, cells) input per level into YoloLayer_TRT created with one field"""
    net = builder.Network(explicit_batch=True)
    try:
        dets = [net.input(f"x{i}", (B, 4 + classes, (H // s) * (W // s))) for i, s in enumerate(strides)]
        ci = info if info is not None else [classes, W, H, 50] + list(strides)
        net.mark_output(net.out(net.plugin(dets, "YoloLayer_TRT", fields=[(name, np.array(ci, np.int32))])), "output")
        return net.build()
    finally:
        net.close()


def plugin_of(plan):
    desc = engine.describe_plan(plan)
    (pl,) = [l for l in desc["layers"] if l["kind"] == gi.L_PLUGIN]
    return desc, pl, bytes.fromhex(pl["plugin_blob"])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_plugin_blob_is_the_references_and_round_trips(n):
    """yololayer.cu:64-79: classes, threadCount (256), netW, netH, maxOut, nStrides, strides = 24 + 4 n bytes; describe_plan deserializes the
    layer from the plan and serializes it again"""
    strides = [8, 16, 32, 64, 128][:n]
    plan = head_net(classes=7, H=256, W=384, strides=strides)
    desc, pl, blob = plugin_of(plan)
    assert pl["plugin_type"] == "YoloLayer_TRT" and len(blob) == 24 + 4 * n
    assert np.frombuffer(blob, "<i4").tolist() == [7, 256, 384, 256, 50, n] + strides
    out = [t for t in desc["tensors"] if t["is_output"]]
    assert out[0]["dims"] == [2, 1 + 50 * 6, 1, 1]
    # the length collides with no other form's: YOLOv8's 35 + 4 k, YOLOv5's 25 + 32 k, YOLOv7's 24 + 32 k (k >= 1), Darknet's 20 + 32 k, YOLOv9's 21
    others = {35 + 4 * k for k in range(9)} | {25 + 32 * k for k in range(1, 9)} | {24 + 32 * k for k in range(1, 9)} | {20 + 32 * k for k in range(9)} | {21}
    assert len(blob) not in others


@pytest.mark.parametrize("info", [[5, 96, 64, 50], [5, 96, 64], [0, 96, 64, 50, 8], [5, 96, 64, 50, 0], [5, 96, 64, 50, 8, -16], [5, 0, 64, 50, 8]])
def test_plugin_refuses_other_fields(info):
    with pytest.raises(RuntimeError, match="createPlugin"):
        head_net(info=info, strides=(8,) * max(1, len(info) - 4))


def test_ten_int_field_is_still_yolov8s():
    """ten and more ints: {classes, keypoints, kpt_conf, W, H, maxOut, seg, pose, obb, strides...}, the YOLOv8 / YOLO11 plugin with 90-float records"""
    plan = head_net(info=[5, 17, 0, 96, 64, 50, 0, 0, 0, 8, 16, 32])
    desc, pl, blob = plugin_of(plan)
    assert len(blob) == 35 + 4 * 3
    assert [t for t in desc["tensors"] if t["is_output"]][0]["dims"] == [2, 1 + 50 * 90, 1, 1]


# ---- the builder -----------------------------------------------------------------------------------------------------------------------

def folds_of(name):
    """how many lk CIB blocks the model has: yolov10/src/model.cpp, restated in the twin"""
    tw = Yolov10({}, name)
    depth = (tw.depth(6), tw.depth(3), tw.depth(3), tw.depth(3), tw.depth(3))
    return sum(d for (kind, lk), d in zip(STAGES[name[-1]], depth) if lk)


@pytest.mark.parametrize("name", MODELS)
def test_model_builds_and_lowers(name, monkeypatch):
    path, sd = yolov10_wts(name)
    B, S = 2, 64
    plan = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1)
    desc = engine.describe_plan(plan)
    assert desc["explicit_batch"]
    io = [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_input"] or t["is_output"]]
    assert io == [("images", [B, 3, S, S]), ("output", [B, 1 + 1000 * 6, 1, 1])]
    # every weight the state holds is read, and nothing else: one convolution per weight, one scale per BatchNorm
    n_w = len([k for k in sd if k.endswith(".weight") and not k.endswith(".bn.weight")])
    assert len([l for l in desc["layers"] if l["kind"] == gi.L_CONV]) == n_w + 2   # (the DFL weight serves three levels)
    assert len([l for l in desc["layers"] if l["kind"] == gi.L_SCALE]) == len([k for k in sd if k.endswith(".running_var")]) + 1   # + the attention's scale
    low = engine.describe_plan(plan, lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["attention"] == 1 and kinds["yolo10_head"] == 1 and kinds["plugin"] == 0, kinds
    assert not {"softmax", "gather", "scatter", "to_linear", "matmul"} & set(kinds), kinds
    (head,) = [o for o in low["ops"] if o["kind"] == "yolo10_head"]
    assert (head["classes"], head["levels"], head["strides"]) == (80, 3, [8, 16, 32]) and all(ld >= 144 for ld in head["ld"])
    convs = convs_of(low)
    assert all(o["igemm"] or o["stem"] or o.get("dw") for o in convs), [o["name"] for o in convs if not (o["igemm"] or o["stem"] or o.get("dw"))]
    dw = [o for o in convs if o.get("dw")]
    folded = [o for o in dw if o.get("repvggdw_fold")]
    assert len(folded) == folds_of(name) and all(o["k"] == [7, 7] and o["act1"] != 0 for o in folded)
    assert not [o for o in dw if o["k"] == [7, 7] and not o.get("repvggdw_fold")], "no 7-tap + 3-tap pair left"
    assert {tuple(o["stride"]) for o in dw} == {(1, 1), (2, 2)} and {o["act1"] != 0 for o in dw if o["k"] == [3, 3]} == {True, False}
    # both switches off: the plugin route and the pairs
    monkeypatch.setenv("TRTX_YOLO10_HEAD", "0")
    monkeypatch.setenv("TRTX_REPVGGDW_FOLD", "0")
    low0 = engine.describe_plan(engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1), lowered=True)
    k0 = collections.Counter(o["kind"] for o in low0["ops"])
    assert k0["plugin"] == 1 and k0["yolo10_head"] == 0 and k0["softmax"] == 3, k0
    dw0 = [o for o in convs_of(low0) if o.get("dw")]
    assert len([o for o in dw0 if o["k"] == [7, 7]]) == folds_of(name) and not [o for o in dw0 if o.get("repvggdw_fold")]
    assert len(dw0) == len(dw) + folds_of(name)


def test_weight_names_are_the_states():
    """the twin, written from the reference's builders, reads exactly the state's keys (num_batches_tracked aside); that the host builder
    reads every one of them and no other is test_model_builds_and_lowers' layer counts (a name it asked for and did not find stops the build)"""
    for name in MODELS:
        sd = synth.yolov10_state(name)
        used = set()

        class Spy(dict):
            def __getitem__(self, k):
                used.add(k)
                return dict.__getitem__(self, k)
        tw = Yolov10(sd, name)
        tw.sd = Spy(tw.sd)
        with torch.inference_mode():
            tw.heads(torch.zeros(1, 3, 32, 32))
        assert used == {k for k in sd if not k.endswith("num_batches_tracked")}, name

def test_marked_heads_keep_the_plugin_and_mixed_sizes_build():
    plan, low = lowered("yolov10n", batch=3, h=96, w=64, fp16=0, mark_heads=1, max_out=300, classes=80)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo10_head"] == 0
    desc = engine.describe_plan(plan)
    io = sorted((t["name"], t["dims"]) for t in desc["tensors"] if t["is_output"])
    assert io == [("head0", [3, 84, 96]), ("head1", [3, 84, 24]), ("head2", [3, 84, 6]), ("output", [3, 1 + 300 * 6, 1, 1])]
    _, pl, blob = plugin_of(plan)
    assert np.frombuffer(blob, "<i4").tolist() == [80, 256, 64, 96, 300, 3, 8, 16, 32]


def test_build_refusals():
    path, _ = yolov10_wts("yolov10n")
    for bad in (dict(model="yolov10q"), dict(model="yolov10"), dict(model="yolov10nn"), dict(h=100), dict(w=72), dict(h=16, w=32), dict(batch=0),
                dict(classes=0), dict(max_out=0), dict(task=1)):
        kw = dict(model="yolov10n", batch=1, h=64, w=64)
        kw.update(bad)
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(kw.pop("model"), path, **kw)
        assert e.value.status == 1, bad   # TRTX_ERR_INVALID
    for name in MODELS:
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(name, path, batch=1, h=64, w=64, int8=1)
        assert e.value.status == 4, name   # TRTX_ERR_UNSUPPORTED


# ---- the RepVGGDW fold -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 8, 24, 40])
def test_fold_is_the_numpy_fold_bit_for_bit(C):
    """scale7 * w7 with scale3 * w3 added into the centre, shift7 + shift3: float64, rounded once to fp32"""
    rng = np.random.default_rng(C)
    w7, w3 = rng.standard_normal((C, 1, 7, 7)).astype(np.float32), rng.standard_normal((C, 1, 3, 3)).astype(np.float32)
    s7, s3 = rng.uniform(0.5, 2, C).astype(np.float32), rng.uniform(-2, 2, C).astype(np.float32)
    h7, h3 = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    w, sh = capi.repvggdw_fold_weights(w7, s7, h7, w3, s3, h3)
    want = w7.astype(np.float64) * s7.astype(np.float64)[:, None, None, None]
    want[:, :, 2:5, 2:5] += w3.astype(np.float64) * s3.astype(np.float64)[:, None, None, None]
    assert np.array_equal(w.view(np.int32), want.astype(np.float32).view(np.int32))
    assert np.array_equal(sh.view(np.int32), (h7.astype(np.float64) + h3.astype(np.float64)).astype(np.float32).view(np.int32))
    # and it is the two convolutions' sum
    x = torch.from_numpy(rng.standard_normal((2, C, 9, 5)))
    F = torch.nn.functional
    two = (F.conv2d(x, torch.from_numpy(w7).double(), None, 1, 3, 1, C) * torch.from_numpy(s7).double()[:, None, None] + torch.from_numpy(h7).double()[:, None, None] +
           F.conv2d(x, torch.from_numpy(w3).double(), None, 1, 1, 1, C) * torch.from_numpy(s3).double()[:, None, None] + torch.from_numpy(h3).double()[:, None, None])
    one = F.conv2d(x, torch.from_numpy(w).double(), torch.from_numpy(sh).double(), 1, 3, 1, C)
    assert (one - two).abs().max().item() < 1e-5


def repdw_net(miss=None, fp16=True, C=8, H=6, W=5):
    """RepVGGDW on one NHWC tensor.  `miss`: 'reader' (the 3x3 branch has a second reader), 'stride' (a stride-2 pair), 'k5' (5x5 in place of 7x7)"""
    rng = np.random.default_rng(11)
    net = builder.Network(explicit_batch=True, fp16=fp16)
    try:
        x = net.input("x", (2, C, H, W))
        k7 = 5 if miss == "k5" else 7
        st = 2 if miss == "stride" else 1
        bn = lambda: (rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32))  # noqa: E731  (shift, scale)
        a = net.out(net.scale(net.out(net.conv(x, rng.standard_normal((C, 1, k7, k7)).astype(np.float32), padding=k7 // 2, stride=st, groups=C)), *bn()))
        b = net.out(net.scale(net.out(net.conv(x, rng.standard_normal((C, 1, 3, 3)).astype(np.float32), padding=1, stride=st, groups=C)), *bn()))
        s = net.out(net.elementwise(a, b, "sum"))
        y = net.out(net.elementwise(s, net.out(net.activation(s, "sigmoid")), "prod"))
        net.mark_output(y, "y")
        if miss == "reader":
            net.mark_output(net.out(net.activation(b, "relu")), "z")
        return net.build()
    finally:
        net.close()


@pytest.mark.parametrize("fp16", [True, False])
def test_small_repvggdw_graph_folds(fp16, monkeypatch):
    low = engine.describe_plan(repdw_net(fp16=fp16), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["conv"] == 1 and not {"ew_nhwc", "act_nhwc"} & set(kinds), kinds
    (cv,) = convs_of(low)
    assert cv.get("dw") and cv.get("repvggdw_fold") and cv["k"] == [7, 7] and cv["act1"] != 0
    monkeypatch.setenv("TRTX_REPVGGDW_FOLD", "0")
    low = engine.describe_plan(repdw_net(fp16=fp16), lowered=True)
    assert len(convs_of(low)) == 2 and not any(o.get("repvggdw_fold") for o in convs_of(low))


@pytest.mark.parametrize("miss", ["reader", "stride", "k5"])
def test_near_miss_repvggdw_keeps_two_convolutions(miss):
    low = engine.describe_plan(repdw_net(miss=miss), lowered=True)
    assert len(convs_of(low)) == 2 and not any(o.get("repvggdw_fold") for o in convs_of(low))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    for sym in ("trtx_yolov10_decode", "trtx_yolov10_head_decode_workspace", "trtx_yolov10_head_decode_nhwc", "trtx_yolov10_head_decode_nhwc_f32",
                "trtx_yolov10_topk", "trtx_repvggdw_fold_weights"):
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, header), sym
    for name in ("yolov10_decode", "yolov10_head_decode_workspace", "yolov10_head_decode_nhwc", "yolov10_topk", "repvggdw_fold_weights"):
        assert callable(getattr(capi, name))
    st = (ctypes.c_int * 3)(8, 16, 32)
    L.trtx_yolov10_head_decode_workspace.restype = ctypes.c_size_t
    L.trtx_yolo_head_decode_workspace.restype = ctypes.c_size_t
    assert L.trtx_yolov10_head_decode_workspace(2, 64, 96, st, 3) == L.trtx_yolo_head_decode_workspace(2, 64, 96, st, 3) > 0
    assert L.trtx_yolov10_head_decode_workspace(2, 64, 96, (ctypes.c_int * 3)(8, 0, 32), 3) == 0


def test_refusals_come_before_the_device():
    """null pointers, zero levels, a stride < 1 and a capacity beyond the NMS's are answered from the arguments alone: the pointers handed over
    here are not device memory, and no device is needed"""
    L = capi.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 3)(p, p, p)
    ld = (ctypes.c_int * 3)(144, 144, 144)
    st, bad = (ctypes.c_int * 3)(8, 16, 32), (ctypes.c_int * 3)(8, 0, 32)
    ws = ctypes.c_size_t(1 << 20)
    dec = lambda **k: L.trtx_yolov10_decode(k.get("inputs", arr), k.get("n", 3), k.get("B", 1), k.get("nc", 80), 64, 96, k.get("st", st), k.get("mo", 10),  # noqa: E731
                                            k.get("out", p), k.get("ws", p), ws, None)
    assert dec(inputs=None) == 1 and dec(out=None) == 1 and dec(ws=None) == 1 and dec(st=None) == 1
    assert dec(inputs=(ctypes.c_void_p * 3)(p, None, p)) == 1, "a null level"
    assert dec(n=0) == 1 and dec(n=9) == 1 and dec(st=bad) == 1 and dec(B=0) == 1 and dec(nc=0) == 1 and dec(mo=0) == 1
    for fn in (L.trtx_yolov10_head_decode_nhwc, L.trtx_yolov10_head_decode_nhwc_f32):
        head = lambda **k: fn(k.get("heads", arr), k.get("ld", ld), k.get("n", 3), 1, k.get("nc", 80), 64, 96, k.get("st", st), k.get("w", p), 10,  # noqa: E731
                              k.get("out", p), k.get("ws", p), ws, None)
        assert head(heads=None) == 1 and head(ld=None) == 1 and head(w=None) == 1 and head(out=None) == 1 and head(ws=None) == 1 and head(st=None) == 1
        assert head(heads=(ctypes.c_void_p * 3)(p, p, None)) == 1 and head(n=0) == 1 and head(st=bad) == 1 and head(nc=0) == 1
        assert head(ld=(ctypes.c_int * 3)(144, 143, 144)) == 4 and head(ld=(ctypes.c_int * 3)(136, 144, 144)) == 4
    q = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    topk = lambda a, b, B, mo: L.trtx_yolov10_topk(a, B, mo, ctypes.c_float(0.5), 0, b, None)  # noqa: E731
    assert topk(None, q, 1, 10) == 1 and topk(p, None, 1, 10) == 1 and topk(p, p, 1, 10) == 1 and topk(p, q, 0, 10) == 1 and topk(p, q, 1, 0) == 1
    assert topk(p, q, 1, yc.CAP + 1) == 4, "the capacity trtx_yolov7_nms accepts, and its refusal beyond it"
