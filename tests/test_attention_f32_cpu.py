"""Attention in fp32 engines (kernels/attention_f32.hip) as the host sees it: the C entry is declared, exported and bound, and a one-attention fp32 network -
the PSA subgraph of tests/test_gpu_psa_mfma.py and the AAttn interior of tests/test_yolo12_cpu.py, built with fp16=False - lowers to gathers, two matmuls
and a softmax with TRTX_ATTENTION_F32 unset and to one `attention` op with "f32" under TRTX_ATTENTION_F32=1."""
import os
import re

import numpy as np
import pytest

from tensorrtx_amd import builder, capi, engine

NETS = [("psa", 1, 32, 64), ("psa", 1, 36, 72), ("area", 4, 32, 32)]


def attention_net(kind, area, kd, hd, B=2, heads=2, H=8, W=9, seed=0):
    """One attention block on a 1x1 qkv convolution, O + V summed into the output (both results have a reader), as an fp32 plan.  -> plan, x, wq"""
    C, cin, N = heads * (2 * kd + hd), 16, H * W
    rng = np.random.default_rng(seed)
    x, wq = rng.standard_normal((B, cin, H, W)).astype(np.float32), (rng.standard_normal((C, cin, 1, 1)) / 4).astype(np.float32)
    net = builder.Network(explicit_batch=True, fp16=False)
    try:
        qkv = net.out(net.conv(net.input("x", (B, cin, H, W)), wq))
        if kind == "psa":   # yolo11/src/block.cpp:287-339
            t, Ba, Na = net.out(net.shuffle(qkv, reshape=(B, heads, -1, N))), B, N
            image = lambda z: net.out(net.shuffle(z, reshape=(B, -1, H, W)))   # noqa: E731
        else:               # yolov12/src/block.cpp:522-625
            Ba, Na = B * area, N // area
            t = net.out(net.shuffle(net.out(net.shuffle(qkv, reshape=(B, -1, N), perm2=(0, 2, 1))), reshape=(Ba, Na, heads, 2 * kd + hd), perm2=(0, 2, 3, 1)))

            def image(z):
                z = net.out(net.shuffle(net.out(net.shuffle(z, perm1=(0, 3, 1, 2))), reshape=(B, H, W, -1)))
                return net.out(net.shuffle(z, perm1=(0, 3, 1, 2)))
        q, k, v = (net.out(net.slice(t, (0, 0, c, 0), (Ba, heads, n, Na))) for c, n in ((0, kd), (kd, kd), (2 * kd, hd)))
        s = net.out(net.scale_uniform(net.out(net.matmul(net.out(net.shuffle(q, perm1=(0, 1, 3, 2))), k)), kd ** -0.5))
        pt = net.out(net.shuffle(net.out(net.softmax(s, axes=1 << 3)), perm1=(0, 1, 3, 2)))
        net.mark_output(net.out(net.elementwise(image(net.out(net.matmul(v, pt))), image(v))), "y")
        return net.build(), x, wq
    finally:
        net.close()


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trtx_hip.h")).read()
    assert re.search(r"\btrtx_op_attention_f32\(", header)
    assert hasattr(capi.lib(), "trtx_op_attention_f32") and callable(capi.attention_f32)


@pytest.mark.parametrize("kind,area,kd,hd", NETS)
def test_fp32_attention_lowers_to_one_op_under_the_switch_only(kind, area, kd, hd, monkeypatch):
    plan, _, _ = attention_net(kind, area, kd, hd)
    count = lambda low, what: sum(o["kind"] == what for o in low["ops"])   # noqa: E731
    monkeypatch.delenv("TRTX_ATTENTION_F32", raising=False)
    low = engine.describe_plan(plan, lowered=True)
    assert (count(low, "attention"), count(low, "matmul")) == (0, 2)
    monkeypatch.setenv("TRTX_ATTENTION_F32", "1")   # read at every lowering
    low = engine.describe_plan(plan, lowered=True)
    (att,) = [o for o in low["ops"] if o["kind"] == "attention"]
    assert count(low, "matmul") == 0 and "mfma" not in att and (att["f32"], att["heads"], att["n"], att["kd"], att["hd"], att.get("area", 1)) == (True, 2, 72, kd, hd, area)
