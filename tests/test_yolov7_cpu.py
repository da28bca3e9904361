"""YOLOv7 detection (host builders, synthetic weights, the 6-float plugin, the fused head's lowering, the ReOrg fold, the parallel SPP pools):
CPU-side checks.  Also holds the helpers the GPU tests of tests/test_gpu_yolov7.py share."""
import collections
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import builder, capi, engine, synth
from tensorrtx_amd import wts as wts_writer
from util import CACHE
from yolov7_twin import Yolov7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("yolov7tiny", "yolov7", "yolov7x", "yolov7w6", "yolov7e6")
P6 = ("yolov7w6", "yolov7e6")
GENERIC_KINDS = {"plugin", "to_linear", "gather", "scatter"}


def strides_of(name):
    return (8, 16, 32, 64) if name in P6 else (8, 16, 32)


def small(name):
    return 128 if name in P6 else 64


def yolov7_wts(name, seed=0, num_class=80):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"{name}_nc{num_class}_synth_s{seed}.wts")
    sd = synth.yolov7_state(name, seed=seed, num_class=num_class)
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def lowered(name, **kw):
    path, _ = yolov7_wts(name, num_class=kw.get("classes", 80))
    plan = engine.build_plan(name, path, **kw)
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


def records6(dec38, max_out):
    """The first six floats of every 38-float record of the YOLOv5 oracle: YOLOv7's record.  [B, 1 + max_out * 38] -> [B, 1 + max_out * 6]"""
    dec38 = np.asarray(dec38, dtype=np.float32)
    B = dec38.shape[0]
    out = np.zeros((B, 1 + max_out * 6), np.float32)
    out[:, 0] = dec38[:, 0]
    out[:, 1:] = dec38[:, 1:].reshape(B, max_out, 38)[:, :, :6].reshape(B, -1)
    return out


@pytest.mark.parametrize("name,B,H,W,nc", [("yolov7tiny", 2, 64, 64, 80), ("yolov7tiny", 1, 64, 96, 13), ("yolov7", 1, 64, 64, 80), ("yolov7", 2, 96, 64, 13),
                                            ("yolov7x", 1, 64, 64, 80), ("yolov7w6", 2, 128, 128, 80), ("yolov7w6", 1, 128, 192, 13),
                                            ("yolov7e6", 1, 128, 128, 80)])
def test_yolov7_builder_matches_pytorch_twin(name, B, H, W, nc):
    """The host builder's graph (run by the oracle's interpreter) against an independent restatement of the yamls.  Between them the
    models cover LeakyReLU and SPP (tiny), MP, SPPCSPC and RepConv (v7), the wide ELAN (x), ReOrg and four levels (w6), DownC (e6).
    Both sides are fp32 / fp64 on the CPU: the bound is test_yolov9_builder_matches_pytorch_twin's."""
    path, sd = yolov7_wts(name, num_class=nc)
    plan = engine.build_plan(name, path, batch=B, h=H, w=W, fp16=1, mark_heads=1, classes=nc)
    desc = engine.describe_plan(plan)
    assert not desc["explicit_batch"]
    x = torch.from_numpy(synth.images(B, H, W, seed=5))
    out = gi.run(without_plugin(desc), plan, {"data": x.numpy()}, batch=B)
    tw = Yolov7(sd, name)
    with torch.inference_mode():
        heads, strides = tw.heads(x)
    assert strides == list(strides_of(name))
    assert sorted(out) == [f"head{i}" for i in range(len(heads))]
    info = 3 * (5 + nc)
    for i, h in enumerate(heads):
        got = torch.as_tensor(out[f"head{i}"])
        assert tuple(got.shape) == (B, info, H // strides[i], W // strides[i])
        d = (got.reshape(h.shape) - h).abs().max().item()
        print(f"{name} nc={nc} head{i}: |diff| {d:.3g}, |head| {h.abs().max().item():.3g}")
        assert d < 2e-4
    # what synth.yolov7_state promises for 80 classes: small images keep 2 - 20 % of the anchors, in every image
    grids = [(W // s, H // s) for s in strides]
    anchors = 3 * sum(gw * gh for gw, gh in grids)
    dec = yp.v5_decode_c([np.asarray(out[f"head{i}"]).reshape(B, info, -1) for i in range(len(heads))], nc, H, W, grids, tw.anchors(), anchors + 1)
    print(f"{name} nc={nc} {H}x{W}: candidates per image {dec[:, 0].astype(int).tolist()} of {anchors} anchors")
    if nc == 80:   # (YOLOV7_OBJ_BIAS_OF is set for 80 classes: another count draws other detect rows)
        assert dec[:, 0].min() >= 4 and dec[:, 0].max() <= 0.6 * anchors


@pytest.mark.parametrize("name", MODELS)
def test_yolov7_lowered_plans(name, monkeypatch):
    S, levels = small(name), len(strides_of(name))
    for fp16 in (1, 0):
        plan, low = lowered(name, batch=2, h=S, w=S, fp16=fp16)
        kinds = collections.Counter(o["kind"] for o in low["ops"])
        print(f"{name} fp16={fp16}: {dict(kinds)}")
        assert kinds["yolo7_head"] == 1 and not set(kinds) & GENERIC_KINDS, kinds
        (head,) = [o for o in low["ops"] if o["kind"] == "yolo7_head"]
        assert low["ops"][-1] is head
        assert (head["classes"], head["levels"], head["anchor_levels"]) == (80, levels, levels) and head["ld"] == [256] * levels
        assert head["grids"] == [[S // s, S // s] for s in strides_of(name)]
        assert kinds["pool_chain"] == 1
        (chain,) = [o for o in low["ops"] if o["kind"] == "pool_chain"]
        assert chain["k"] == [5, 5] and chain["outputs"] == 3
        assert all(o["k"] == [2, 2] and o["stride"] == [2, 2] for o in low["ops"] if o["kind"] == "pool")   # the MP / DownC pools: none of 9 or 13
        first = convs_of(low)[0]
        # The image reaches the first convolution without a layout pass wherever conv_stem takes the layer (8 / 16 / 32 / 64 outputs in
        # fp16 engines, multiples of 16 in fp32 ones).  yolov7x's 40 outputs (both engines) and yolov7e6's 80 (fp16) are not among them:
        # those keep the one to_nhwc of the network input, as YOLOv5x's 80-output 6x6 stem does.
        stemless = name == "yolov7x" or (name == "yolov7e6" and fp16)
        assert kinds["to_nhwc"] == (1 if stemless else 0), kinds
        assert first["stem"] == (not stemless)
        if name in P6:
            assert (first["k"], first["stride"], first["cin"], first["hw_in"], first["reorg_cin"]) == ([6, 6], [2, 2], 3, [S, S], 3)
        else:
            assert "reorg_cin" not in first
        # each switch off: what it removes comes back
        for env, want in (("TRTX_YOLO7_HEAD", dict(plugin=1, to_linear=levels, yolo7_head=0)), ("TRTX_SPP_PARALLEL_CHAIN", dict(pool_chain=0)),
                          ("TRTX_REORG_FOLD", dict(gather=4 if name in P6 else 0))):
            with monkeypatch.context() as m:
                m.setenv(env, "0")
                off = engine.describe_plan(plan, lowered=True)
            k2 = collections.Counter(o["kind"] for o in off["ops"])
            for kind, n in want.items():
                assert k2[kind] == n, (env, kind, k2)
            if env == "TRTX_SPP_PARALLEL_CHAIN":
                assert sorted(o["k"][0] for o in off["ops"] if o["kind"] == "pool" and o["stride"] == [1, 1]) == [5, 9, 13]
                assert k2["pool"] == kinds["pool"] + 3


@pytest.mark.parametrize("name", MODELS)
def test_yolov7_convolutions_on_the_direct_kernel(name):
    """fp16 plans at the flagship size: every convolution is on an MFMA kernel or the stem kernel, but for yolov7e6's folded 6x6 stem over
    3 channels to 80 outputs, which takes what YOLOv5x's 80-output 6x6 stem takes (DESIGN, "YOLOv7 detection")."""
    S = 1280 if name in P6 else 640
    _, low = lowered(name, batch=8, h=S, w=S, fp16=1)
    convs = convs_of(low)
    direct = [(o["name"], o["cin"], o["cout"], o["k"]) for o in convs if not (o["igemm"] or o["stem"] or o.get("dw") or o.get("grouped"))]
    print(f"{name}: {len(direct)} of {len(convs)} convolutions on conv_direct_kernel: {direct}")
    if name == "yolov7e6":
        assert direct == [("model.1.conv [ReOrg folded]", 3, 80, [6, 6])]
    else:
        assert direct == []


def reorg(x):
    return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("cin", [3, 4])
@pytest.mark.parametrize("hw", [(8, 12), (2, 2)])
def test_reorg_fold_arithmetic(k, cin, hw):
    """conv(reorg(x), W, padding p) == conv(x, W', stride 2, padding 2p) in fp64, W' as the packer builds it (trtx_reorg_fold_weights)"""
    g = torch.Generator().manual_seed(k * 100 + cin * 10 + hw[0])
    x = torch.randn(2, cin, *hw, generator=g, dtype=torch.float64)
    w = torch.randn(5, 4 * cin, k, k, generator=g).float()   # (the ABI takes fp32: the same values on both sides)
    p = k // 2
    want = F.conv2d(reorg(x), w.double(), padding=p)
    w2 = torch.from_numpy(capi.reorg_fold_weights(w.numpy()))
    assert tuple(w2.shape) == (5, cin, 2 * k, 2 * k)
    assert sorted(w2.flatten().tolist()) == sorted(w.flatten().tolist())   # a permutation of the same values
    got = F.conv2d(x, w2.double(), stride=2, padding=2 * p)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("hw", [(2, 2), (4, 7), (20, 20)])
def test_parallel_pools_are_the_chain_of_three(hw):
    """max-pooling that skips its padding composes: mp9 = mp5 o mp5 and mp13 = mp5 o mp5 o mp5, bit for bit, with -inf and with ties"""
    g = torch.Generator().manual_seed(hw[0] * 31 + hw[1])
    x = torch.randn(1, 3, *hw, generator=g)
    x[0, 1] = torch.randint(0, 3, hw, generator=g).float()   # ties
    x[0, 2, 0, :] = float("-inf")
    x[0, 2, -1, -1] = float("-inf")
    y1 = F.max_pool2d(x, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    y3 = F.max_pool2d(y2, 5, 1, 2)
    for y, k in ((y1, 5), (y2, 9), (y3, 13)):
        want = F.max_pool2d(x, k, 1, k // 2)
        assert torch.equal(y.view(torch.int32), want.view(torch.int32)), k


# ---- small hand-built graphs ---------------------------------------------------------------------------------------------------------

ANCH = np.arange(1, 19, dtype=np.float32).reshape(3, 6) * 4


def head_net(miss=None, fp16=True, classes=5, H=64, W=96, levels=3, netinfo=None):
    """One 16-channel input per level, a biased 1x1 detect convolution on it, and the anchor plugin created from "netinfo" + "kernels".
    `miss`: 'netinfo5' (a fifth int: YOLOv5's plugin), 'reader' (a head convolution with a second reader), 'act' (a head convolution with
    an activation)."""
    rng = np.random.default_rng(3)
    net = builder.Network(max_batch=2, fp16=fp16)
    try:
        dets, kern = [], []
        info = 3 * (5 + classes)
        for lv in range(levels):
            s = 8 << lv
            gh, gw = H // s, W // s
            x = net.input(f"x{lv}", (16, gh, gw))
            det = net.out(net.conv(x, (rng.standard_normal((info, 16, 1, 1)) / 2).astype(np.float32), bias=rng.standard_normal(info).astype(np.float32)))
            if miss == "reader" and lv == 0:
                net.mark_output(net.out(net.activation(det, "relu")), "aux")
            if miss == "act" and lv == 1:
                det = net.out(net.activation(det, "relu"))
            dets.append(det)
            kern.append(np.concatenate([np.array([gw, gh], np.int32).view(np.float32), np.resize(ANCH, (8, 6))[lv]]))
        ni = netinfo if netinfo is not None else ([classes, W, H, 50, 0] if miss == "netinfo5" else [classes, W, H, 50])
        fields = [("netinfo", np.array(ni, np.int32)), ("kernels", np.concatenate(kern).astype(np.float32), levels)]
        net.mark_output(net.out(net.plugin(dets, "YoloLayer_TRT", fields=fields)), "prob")
        return net.build()
    finally:
        net.close()


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("levels", [3, 4])
def test_small_anchor_graph_fuses(fp16, levels):
    low = engine.describe_plan(head_net(fp16=fp16, levels=levels), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert dict(kinds) == {"to_nhwc": levels, "conv": levels, "yolo7_head": 1}, kinds
    (head,) = [o for o in low["ops"] if o["kind"] == "yolo7_head"]
    assert (head["classes"], head["levels"]) == (5, levels) and head["grids"] == [[96 >> (3 + l), 64 >> (3 + l)] for l in range(levels)]
    assert head["ld"] == [32] * levels   # 30 channels rounded up to 16-byte pieces
    assert [(o["cout_real"], o["cout"]) for o in convs_of(low) if o.get("cout_real")] == [(30, 32)] * levels


@pytest.mark.parametrize("miss", ["netinfo5", "reader", "act"])
def test_near_miss_heads_keep_their_plugin(miss):
    low = engine.describe_plan(head_net(miss=miss), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["yolo7_head"] == 0, kinds
    if miss == "netinfo5":   # YOLOv5's plugin and YOLOv5's fused head, 38-float records
        assert kinds["yolo5_head"] == 1 and kinds["plugin"] == 0
        out = [t for t in engine.describe_plan(head_net(miss=miss))["tensors"] if t["is_output"]]
        assert out[0]["dims"] == [1 + 50 * 38, 1, 1]
    else:
        assert kinds["plugin"] == 1 and kinds["yolo5_head"] == 0 and kinds["to_linear"] >= 3, kinds


def reorg_net(miss=None, fp16=True, C=3, H=16, W=24, k=3, cout=16):
    """ReOrg of the input in front of a k x k convolution.  `miss`: 'order' (slices 2 and 3 swapped), 'odd' (H = 15), 'twice' (the concat is
    read by a second convolution), 'start' (a slice starts at row 2)."""
    rng = np.random.default_rng(5)
    if miss == "odd":
        H = 15
    net = builder.Network(max_batch=2, fp16=fp16)
    try:
        x = net.input("data", (C, H, W))
        starts = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)]
        if miss == "order":
            starts[1], starts[2] = starts[2], starts[1]
        if miss == "start":
            starts[1] = (0, 2, 0)
        h2, w2 = H // 2, W // 2
        if miss == "start":
            h2 -= 1
        parts = [net.out(net.slice(x, st, (C, h2, w2), (1, 2, 2))) for st in starts]
        cat = net.out(net.concat(parts))
        w = (rng.standard_normal((cout, 4 * C, k, k)) / 6).astype(np.float32)
        y = net.out(net.activation(net.out(net.conv(cat, w, bias=rng.standard_normal(cout).astype(np.float32), padding=k // 2)), "relu"))
        net.mark_output(y, "y")
        if miss == "twice":
            net.mark_output(net.out(net.conv(cat, w[:8].copy(), padding=k // 2)), "z")
        return net.build(), w
    finally:
        net.close()


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("k", [3, 1])
def test_small_reorg_graph_folds(fp16, k):
    plan, _ = reorg_net(fp16=fp16, k=k)
    low = engine.describe_plan(plan, lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["gather"] == 0 and kinds["scatter"] == 0 and kinds["conv"] == 1, kinds
    (cv,) = convs_of(low)
    assert (cv["k"], cv["stride"], cv["cin"], cv["hw_in"], cv["hw_out"], cv["reorg_cin"]) == ([2 * k, 2 * k], [2, 2], 3, [16, 24], [8, 12], 3)


@pytest.mark.parametrize("miss", ["order", "odd", "twice", "start"])
def test_near_miss_reorg_keeps_the_gathers(miss):
    low = engine.describe_plan(reorg_net(miss=miss)[0], lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["gather"] == 4, kinds
    assert not any(o.get("reorg_cin") for o in convs_of(low))


def spp_net(ks=(5, 9, 13), miss=None, fp16=True, C=16, H=10, W=12, order=(0, 1, 2)):
    """Three parallel 'same' max-pools of a convolution's output, joined with it.  `miss`: 'inputs' (the third pool reads another tensor)"""
    rng = np.random.default_rng(7)
    net = builder.Network(max_batch=2, fp16=fp16)
    try:
        x = net.input("x", (C, H, W))
        a = net.out(net.activation(net.out(net.conv(x, (rng.standard_normal((C, C, 1, 1)) / 4).astype(np.float32))), "relu"))
        b = net.out(net.activation(net.out(net.conv(x, (rng.standard_normal((C, C, 1, 1)) / 4).astype(np.float32))), "relu"))
        pools = [None] * 3
        for j in order:
            src = b if (miss == "inputs" and j == 2) else a
            pools[j] = net.out(net.pooling(src, ks[j], 1, ks[j] // 2))
        net.mark_output(net.out(net.concat([a, b] + pools)), "y")
        return net.build()
    finally:
        net.close()


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_small_spp_graph_chains(fp16, order):
    low = engine.describe_plan(spp_net(fp16=fp16, order=order), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["pool_chain"] == 1 and kinds["pool"] == 0, kinds
    (chain,) = [o for o in low["ops"] if o["kind"] == "pool_chain"]
    assert chain["k"] == [5, 5] and chain["outputs"] == 3


@pytest.mark.parametrize("kw", [dict(ks=(5, 9, 11)), dict(miss="inputs"), dict(ks=(3, 5, 9))])
def test_near_miss_spp_keeps_three_pools(kw):
    low = engine.describe_plan(spp_net(**kw), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["pool_chain"] == 0 and kinds["pool"] == 3, kinds


# ---- plugin --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", [3, 4])
def test_yolov7_plugin_state_is_the_references(levels):
    """Created with "netinfo"[4] + "kernels"; the serialized plan is read back (describe_plan deserializes the layer and serializes it
    again): 24 + 32 n bytes, int classCount, threadCount, kernelCount, netW, netH, maxOut, then the YoloKernels"""
    desc = engine.describe_plan(head_net(classes=7, H=128, W=192, levels=levels))
    (pl,) = [l for l in desc["layers"] if l["kind"] == gi.L_PLUGIN]
    blob = bytes.fromhex(pl["plugin_blob"])
    assert pl["plugin_type"] == "YoloLayer_TRT" and len(blob) == 24 + 32 * levels == (120, 152)[levels - 3]
    assert np.frombuffer(blob[:24], "<i4").tolist() == [7, 256, levels, 192, 128, 50]
    for lv in range(levels):
        k = blob[24 + 32 * lv:56 + 32 * lv]
        assert np.frombuffer(k[:8], "<i4").tolist() == [192 >> (3 + lv), 128 >> (3 + lv)]
        assert np.frombuffer(k[8:], "<f4").tolist() == np.resize(ANCH, (8, 6))[lv].tolist()
    out = [t for t in desc["tensors"] if t["is_output"] and t["name"] == "prob"]
    assert out[0]["dims"] == [1 + 50 * 6, 1, 1]


@pytest.mark.parametrize("netinfo", [[5, 96, 64], [5], [0, 96, 64, 50], [5, 96, 64, 0], [5, 0, 64, 50]])
def test_yolov7_plugin_refuses_other_netinfo(netinfo):
    with pytest.raises(RuntimeError, match="createPlugin"):
        head_net(netinfo=netinfo)


def test_v5_and_v9_blobs_still_come_back_as_themselves():
    d5 = engine.describe_plan(head_net(miss="netinfo5", classes=7))
    b5 = bytes.fromhex([l for l in d5["layers"] if l["kind"] == gi.L_PLUGIN][0]["plugin_blob"])
    assert len(b5) == 25 + 32 * 3 and np.frombuffer(b5[:24], "<i4").tolist() == [7, 256, 3, 96, 64, 50] and b5[24] == 0
    import test_yolov9_cpu as t9
    d9 = engine.describe_plan(t9.head_net())
    b9 = bytes.fromhex([l for l in d9["layers"] if l["kind"] == gi.L_PLUGIN][0]["plugin_blob"])
    assert len(b9) == 21 and np.frombuffer(b9[:20], "<i4").tolist() == [5, 256, 96, 64, 50]
    assert [t for t in d9["tensors"] if t["is_output"]][0]["dims"] == [1 + 50 * 38, 1, 1]


# ---- trtx_host_build -----------------------------------------------------------------------------------------------------------------

def test_yolov7_build_errors_and_bindings():
    path, _ = yolov7_wts("yolov7tiny")
    bad_cases = [dict(model="yolov7d6"), dict(model="yolov7e6e"), dict(model="yolov7s"), dict(model="yolov7tiny", h=100), dict(model="yolov7tiny", w=16, h=32),
                 dict(model="yolov7tiny", w=72), dict(model="yolov7tiny", batch=0), dict(model="yolov7tiny", classes=0), dict(model="yolov7tiny", max_out=0),
                 dict(model="yolov7tiny", task=1), dict(model="yolov7w6", h=96, w=128), dict(model="yolov7e6", h=128, w=32)]
    for bad in bad_cases:
        kw = dict(batch=1)
        kw.update(bad)
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(kw.pop("model"), path, **kw)
        assert e.value.status == 1, bad   # TRTX_ERR_INVALID
    for name in MODELS:
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(name, path, batch=1, h=128, w=128, int8=1)
        assert e.value.status == 4, name   # TRTX_ERR_UNSUPPORTED
    # a weight map whose anchor_grid holds two levels for three detect convolutions
    sd = synth.yolov7_state("yolov7tiny")
    sd["model.77.anchor_grid"] = sd["model.77.anchor_grid"][:2]
    short = os.path.join(CACHE, "yolov7tiny_two_anchor_levels.wts")
    wts_writer.write_wts(short, sd, dialect="double")
    with pytest.raises(capi.TrtxError) as e:
        engine.build_plan("yolov7tiny", short, batch=1, h=64, w=64)
    assert e.value.status == 1
    plan = engine.build_plan("yolov7tiny", path, batch=4, h=96, w=160, max_out=300)
    desc = engine.describe_plan(plan)
    io = [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_input"] or t["is_output"]]
    assert io == [("data", [3, 96, 160]), ("prob", [1 + 300 * 6, 1, 1])]
    assert desc["max_batch"] == 4
    plan = engine.build_plan("yolov7tiny", path, batch=1, h=64, w=96, mark_heads=1)
    desc = engine.describe_plan(plan)
    io = [(t["name"], t["dims"]) for t in desc["tensors"] if t["is_output"]]
    assert sorted(io) == [("head0", [255, 8, 12]), ("head1", [255, 4, 6]), ("head2", [255, 2, 3]), ("prob", [6001, 1, 1])]
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo7_head"] == 0   # marked heads keep the plugin


def test_yolov7_state_holds_only_what_the_builder_reads():
    """Every tensor but BatchNorm's num_batches_tracked is read by the builder: no implicit ia / im, no strides, no RepConv identity"""
    for name in MODELS:
        sd = synth.yolov7_state(name)
        assert not [k for k in sd if ".ia." in k or ".im." in k or k.endswith(".strides") or "rbr_identity" in k]
        path, _ = yolov7_wts(name)
        S = small(name)
        desc = engine.describe_plan(engine.build_plan(name, path, batch=1, h=S, w=S))
        convs = [l for l in desc["layers"] if l["kind"] == gi.L_CONV]
        n_conv_w = len([k for k in sd if k.endswith(".conv.weight") or k.endswith(".0.weight") or re.search(r"\.m\.\d\.weight$", k)])
        assert len(convs) == n_conv_w, (name, len(convs), n_conv_w)
        n_bn = len([k for k in sd if k.endswith(".running_var")])
        assert len([l for l in desc["layers"] if l["kind"] == gi.L_SCALE]) == n_bn
        det = max(int(k.split(".")[1]) for k in sd)
        assert det == {"yolov7tiny": 77, "yolov7": 105, "yolov7x": 121, "yolov7w6": 118, "yolov7e6": 140}[name]
        assert tuple(sd[f"model.{det}.anchor_grid"].shape) == (len(strides_of(name)), 1, 3, 1, 1, 2)


def test_yolov7_abi_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    for sym in ("trtx_yolov7_decode_workspace", "trtx_yolov7_decode", "trtx_yolov7_head_decode_workspace", "trtx_yolov7_head_decode_nhwc",
                "trtx_yolov7_head_decode_nhwc_f32", "trtx_yolov7_nms", "trtx_reorg_fold_weights"):
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, header), sym
    assert "YOLOv5 / v7" not in header
    L.trtx_yolov7_decode_workspace.restype = ctypes.c_size_t
    L.trtx_yolov7_head_decode_workspace.restype = ctypes.c_size_t
    gw, gh = (ctypes.c_int * 2)(12, 6), (ctypes.c_int * 2)(8, 4)
    cells = 12 * 8 + 6 * 4
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    want = 2 * up(2 * cells * 3 * 4) + up(2 * ((cells + 511) // 512) * 4)
    assert L.trtx_yolov7_decode_workspace(2, gw, gh, 2) == want == L.trtx_yolov7_head_decode_workspace(2, gw, gh, 2)
    for name in ("yolov7_decode", "yolov7_head_decode_nhwc", "yolov7_nms", "reorg_fold_weights"):
        assert callable(getattr(capi, name))
