"""YOLOv12 detection (host builder, synthetic weights, area-attention lowering): CPU-side checks."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import builder, engine, synth
from tensorrtx_amd import wts as wts_writer
from util import CACHE
from yolo12_twin import Yolo12

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AATTN_SCALE = 0.176777   # the constant of yolov12/src/block.cpp:528
GENERIC_KINDS = {"matmul", "softmax", "gather", "scatter", "to_linear", "to_nhwc"}


def yolo12_wts(scale, seed=0):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"yolo12{scale}_synth_s{seed}.wts")
    sd = synth.yolo12_state(scale, seed=seed)
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def lowered(scale, **kw):
    path, _ = yolo12_wts(scale)
    plan = engine.build_plan("yolo12" + scale, path, **kw)
    return plan, engine.describe_plan(plan, lowered=True)


def aattn_net(B, heads, H, W, area, gain=1.0, seed=0, x=None, wq=None, miss=None, hd=32):
    """The AAttn interior of yolov12/src/block.cpp:522-625 on a 1x1 qkv convolution, built with the reference's own shuffles, O + V summed
    into the output (so that both of the fused op's results have a reader).  `miss` breaks one thing the matcher checks:
    'slice_start' (k starts one row early), 'shift' (score scale with shift 0.5), 'reader' (the softmax output has a second reader),
    'kd16' (16 channels per q / k / v: pass hd=16), 'area' (the output reshape folds the batch differently from the input one)."""
    C = heads * hd
    cin = 16
    rng = np.random.default_rng(seed)
    xr = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    x = xr if x is None else x
    if wq is None:
        wq = (rng.standard_normal((3 * C, cin, 1, 1)) / 4).astype(np.float32)
        for h in range(heads):   # q / k channels scaled by `gain`
            wq[h * 3 * hd:h * 3 * hd + 2 * hd] *= gain
    N = H * W
    Ba, Na = B * area, N // area
    net = builder.Network(explicit_batch=True, fp16=True)
    try:
        xi = net.input("x", (B, cin, H, W))
        qkv = net.out(net.conv(xi, wq))
        t = net.out(net.shuffle(qkv, reshape=(B, -1, N), perm2=(0, 2, 1)))
        t = net.out(net.shuffle(t, reshape=(Ba, Na, heads, 3 * hd), perm2=(0, 2, 3, 1)))
        part = (Ba, heads, hd, Na)
        q = net.out(net.slice(t, (0, 0, 0, 0), part))
        k = net.out(net.slice(t, (0, 0, hd - 1 if miss == "slice_start" else hd, 0), part))
        v = net.out(net.slice(t, (0, 0, 2 * hd, 0), part))
        qt = net.out(net.shuffle(q, perm1=(0, 1, 3, 2)))
        s = net.out(net.scale_uniform(net.out(net.matmul(qt, k)), AATTN_SCALE, shift=0.5 if miss == "shift" else 0.0))
        p = net.out(net.softmax(s, axes=1 << 3))
        pt = net.out(net.shuffle(p, perm1=(0, 1, 3, 2)))
        if miss == "reader":
            net.mark_output(net.out(net.shuffle(p, perm1=(0, 1, 3, 2))), "p2")
        o = net.out(net.matmul(v, pt))
        img = (2 * B, H // 2, W, -1) if miss == "area" else (B, H, W, -1)

        def image(z):
            z = net.out(net.shuffle(z, perm1=(0, 3, 1, 2)))
            z = net.out(net.shuffle(z, reshape=img))
            return net.out(net.shuffle(z, perm1=(0, 3, 1, 2)))
        net.mark_output(net.out(net.elementwise(image(o), image(v))), "y")
        plan = net.build()
    finally:
        net.close()
    return plan, x, wq


def aattn_reference(x, wq, heads, area, hd=32):
    """fp64 AAttn from the qkv tensor rounded to fp16 (the engine's storage site), ultralytics' formulation.  Returns O, V (images),
    the scores, softmax @ |v| as an image, and the largest |q|^T |k| * scale."""
    B, _, H, W = x.shape
    N, C = H * W, heads * hd
    qkv = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wq).double()).half().double()
    t = qkv.flatten(2).transpose(1, 2).reshape(B * area, N // area, heads, 3 * hd).permute(0, 2, 3, 1)
    q, k, v = t.split([hd, hd, hd], dim=2)
    sc = float(np.float32(AATTN_SCALE))
    scores = (q.transpose(-2, -1) @ k) * sc
    p = scores.softmax(-1)
    image = lambda z: z.permute(0, 3, 1, 2).reshape(B, H, W, C).permute(0, 3, 1, 2)  # noqa: E731
    s_abs = ((q.abs().transpose(-2, -1) @ k.abs()) * sc).max().item()
    return image(v @ p.transpose(-2, -1)), image(v), scores, image(v.abs() @ p.transpose(-2, -1)), s_abs


@pytest.mark.parametrize("scale,B,S", [("n", 2, 128), ("m", 1, 64)])
def test_yolo12_builder_matches_pytorch_twin(scale, B, S):
    """The host builder's graph (run by the oracle's interpreter) against an independent restatement of the modules; yolo12m takes the
    C3k path of C3K2.  Both sides are fp32 / fp64 on the CPU: the bound is test_yolo11_builder_matches_pytorch_twin's."""
    path, sd = yolo12_wts(scale)
    plan = engine.build_plan("yolo12" + scale, path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    desc = engine.describe_plan(plan)
    assert desc["explicit_batch"]
    x = torch.from_numpy(synth.images(B, S, S, seed=5))
    out = gi.run(desc, plan, {"images": x.numpy()}, batch=B)
    with torch.inference_mode():
        heads, strides = Yolo12(sd, scale).heads(x)
    assert strides == [8, 16, 32]
    for i, h in enumerate(heads):
        assert tuple(out[f"head{i}"].shape) == tuple(h.shape) == (B, 84, (S // strides[i]) ** 2)
        d = (out[f"head{i}"] - h).abs().max().item()
        print(f"yolo12{scale} head{i}: |diff| {d:.3g}, |head| {h.abs().max().item():.3g}")
        assert d < 2e-4
    got = out["output"].reshape(B, -1).numpy()
    dec = yp.decode_c([out[f"head{i}"].numpy() for i in range(3)], 80, S, S, strides)
    assert np.array_equal(got, dec)


def test_synthetic_attention_is_not_uniform():
    """A condition on the test input, not a measurement: in every one of the eight area-attention blocks of yolo12n at 640 x 640 the mean
    over queries of the largest softmax weight is at least 10 / (keys per area), ten times what uniform attention (the mean of V) has."""
    _, sd = yolo12_wts("n")
    tw = Yolo12(sd, "n")
    with torch.inference_mode():
        tw.heads(torch.from_numpy(synth.images(2, 640, 640, seed=5)))
    assert len(tw.attn_peak) == 8
    for name, (peak, keys) in tw.attn_peak.items():
        print(f"{name}: mean largest weight {peak:.4f} over {keys} keys ({peak * keys:.1f} x uniform)")
        assert keys == 400 and peak >= 10.0 / keys, name


def test_yolo12n_fp16_lowering():
    _, low = lowered("n", batch=2, h=128, w=128, fp16=1)
    ops = low["ops"]
    kinds = collections.Counter(o["kind"] for o in ops)
    assert kinds["attention"] == 8 and kinds["yolo_head"] == 1, kinds
    assert not set(kinds) & (GENERIC_KINDS | {"plugin"}), kinds
    att = [o for o in ops if o["kind"] == "attention"]
    assert [o["area"] for o in att] == [4, 4, 4, 4, 1, 1, 1, 1]
    assert [(o["heads"], o["n"], o["kd"], o["hd"]) for o in att] == [(2, 64, 32, 32)] * 4 + [(4, 16, 32, 32)] * 4
    assert all(o["kernel"] == "mfma" and o["flops"] > 0 and o["bytes"] > 0 for o in att)
    # 2 * B * heads * area * (N / area)^2 * (kd + hd)
    assert att[0]["flops"] == 2 * 2 * 2 * 4 * 16 * 16 * 64 and att[4]["flops"] == 2 * 2 * 4 * 16 * 16 * 64


def test_yolo12n_fp16_lowering_640_b32():
    _, low = lowered("n", batch=32, h=640, w=640, fp16=1)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert set(kinds) <= {"conv", "conv_group", "attention", "yolo_head", "copy_nhwc"}, kinds
    assert kinds["attention"] == 8 and kinds["yolo_head"] == 1
    att = [o for o in low["ops"] if o["kind"] == "attention"]
    assert [(o["heads"], o["n"], o["area"]) for o in att] == [(2, 1600, 4)] * 4 + [(4, 400, 1)] * 4
    convs = [o for o in low["ops"] if o["kind"] == "conv"] + [m for o in low["ops"] if o["kind"] == "conv_group" for m in o["members"]]
    dw = [o for o in convs if o.get("dw")]
    assert len(dw) == 14   # six DWConv of the class branches + the eight 7x7 `pe`
    assert all(o["igemm"] or o["stem"] or o.get("dw") for o in convs)


def test_yolo12_fp32_and_generic_option_keep_the_linear_path(monkeypatch):
    _, low = lowered("n", batch=2, h=128, w=128, fp16=0)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["attention"] == 0 and kinds["matmul"] == 16 and kinds["softmax"] == 8 and kinds["yolo_head"] == 1
    plan, low = lowered("n", batch=2, h=128, w=128, fp16=1)
    assert collections.Counter(o["kind"] for o in low["ops"])["attention"] == 8
    monkeypatch.setenv("TRTX_AREA_ATTENTION", "0")
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert kinds["attention"] == 0 and kinds["matmul"] == 16 and kinds["softmax"] == 8 and kinds["yolo_head"] == 1


def test_generic_option_leaves_psa_attention_alone(monkeypatch):
    from test_yolo11_cpu import yolo11_wts
    path, _ = yolo11_wts("n")
    plan = engine.build_plan("yolo11n", path, batch=2, h=128, w=128, fp16=1)
    monkeypatch.setenv("TRTX_AREA_ATTENTION", "0")
    assert [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]].count("attention") == 1


def test_yolo12_marked_heads_keep_the_plugin():
    _, low = lowered("n", batch=4, h=128, w=128, fp16=1, mark_heads=1)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo_head"] == 0 and kinds["attention"] == 8


def test_aattn_subgraph_lowers_to_one_op():
    plan, _, _ = aattn_net(3, 2, 12, 14, 4)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    (att,) = [o for o in ops if o["kind"] == "attention"]
    assert (att["heads"], att["n"], att["kd"], att["hd"], att["area"]) == (2, 168, 32, 32, 4)
    assert not {"matmul", "softmax", "gather"} & {o["kind"] for o in ops}


@pytest.mark.parametrize("miss", ["slice_start", "shift", "reader", "kd16", "area"])
def test_near_miss_graphs_lower_generically(miss):
    """One matcher condition broken at a time: no attention op, and the plan still builds and lowers"""
    plan, _, _ = aattn_net(2, 2, 8, 8, 4, miss=miss, hd=16 if miss == "kd16" else 32)
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert kinds["attention"] == 0 and kinds["matmul"] == 2 and kinds["softmax"] == 1, kinds


def _psa_net(B, heads, H, W, kd=32, hd=64, seed=0):
    """tests/test_gpu_yolo11.py's _attention_net (gain 1), restated: YOLO11's PSA attention subgraph"""
    C = heads * (2 * kd + hd)
    rng = np.random.default_rng(seed)
    rng.standard_normal((B, 16, H, W))
    wq = (rng.standard_normal((C, 16, 1, 1)) / 4).astype(np.float32)
    N = H * W
    net = builder.Network(explicit_batch=True, fp16=True)
    try:
        xi = net.input("x", (B, 16, H, W))
        qkv = net.out(net.conv(xi, wq))
        v4 = net.out(net.shuffle(qkv, reshape=(B, heads, -1, N)))
        q = net.out(net.slice(v4, (0, 0, 0, 0), (B, heads, kd, N)))
        k = net.out(net.slice(v4, (0, 0, kd, 0), (B, heads, kd, N)))
        v = net.out(net.slice(v4, (0, 0, 2 * kd, 0), (B, heads, hd, N)))
        qt = net.out(net.shuffle(q, perm1=(0, 1, 3, 2)))
        s = net.out(net.scale_uniform(net.out(net.matmul(qt, k)), kd ** -0.5))
        p = net.out(net.softmax(s, axes=1 << 3))
        pt = net.out(net.shuffle(p, perm1=(0, 1, 3, 2)))
        o = net.out(net.shuffle(net.out(net.matmul(v, pt)), reshape=(B, -1, H, W)))
        vr = net.out(net.shuffle(v, reshape=(B, -1, H, W)))
        net.mark_output(net.out(net.elementwise(o, vr)), "y")
        return net.build()
    finally:
        net.close()


def test_psa_subgraph_plan_and_lowering_unchanged(monkeypatch):
    """The serialized plan and the lowered op list of YOLO11's attention subgraph (no tactics: TRTX_TUNE=0), hashed on the commit before
    area attention existed"""
    monkeypatch.setenv("TRTX_TUNE", "0")
    with open(os.path.join(GOLDEN, "yolo11_psa_subgraph_sha256.json")) as f:
        want = json.load(f)
    for B, heads, H, W in [(3, 2, 10, 10), (32, 2, 20, 20)]:
        plan = _psa_net(B, heads, H, W, seed=heads * 7 + H)
        ops = engine.describe_plan(plan, lowered=True)["ops"]
        got = {"plan": hashlib.sha256(plan).hexdigest(), "lowered_ops": hashlib.sha256(json.dumps(ops, sort_keys=True).encode()).hexdigest()}
        assert got == want[f"B={B};heads={heads};H={H};W={W}"]


def test_yolo12_bad_arguments_are_errors():
    path, _ = yolo12_wts("n")
    with pytest.raises(RuntimeError):
        engine.build_plan("yolo12q", path, batch=1)
    with pytest.raises(RuntimeError):
        engine.build_plan("yolo12n", path, batch=1, task=1)
    with pytest.raises(RuntimeError):   # 48 x 48: the stride-16 grid has 3 x 3 = 9 pixels, which 4 areas do not divide (96 x 96 has 36)
        engine.build_plan("yolo12n", path, batch=1, h=48, w=48)
    engine.build_plan("yolo12n", path, batch=1, h=96, w=96)
