"""YOLOv13's area attention (AAttn, yolov13/src/block.cpp:303-423: q | k from one 1x1 convolution, v from another, the softmax spelled out) as a
test network, its fp64 reference, and the attention table's "area" cases repacked into separate operands.  Shared by tests/test_aattn_split_cpu.py
(lowering, near misses, repacking) and tests/test_gpu_aattn_split.py (the kernel through the C ABI and the op inside plans)."""
import numpy as np
import torch

from tensorrtx_amd import builder
from tests import attention_cases as ac

HD = 32
SCALE = float(np.float32(1.0 / np.sqrt(HD)))   # block.cpp:371, 1 / sqrt(head_dim) stored as a float
MISSES = ("slice_start", "shift", "axis", "reader", "hd16", "area", "v_reshape")


def aattn13_net(B, heads, H, W, area, softmax="chain", tail="v", miss=None, gain=1.0, seed=0, x=None, weights=None, hd=HD, fp16=True, cin=16):
    """The AAttn interior on two 1x1 convolutions (qk: 2C channels, v: C channels, C = heads * hd) of a 16-channel input, with the reference's own
    shuffles and slices; the three 3-d reshapes exist only where area > 1, as in the reference.  softmax: "chain" = reduce-max / sub / exp /
    reduce-sum / div (block.cpp:384-394), "layer" = one ISoftMaxLayer.  tail: "v" ends in attn_x + v, "pe" in attn_x + pe(v) with the 5x5 depthwise
    `pe` (block.cpp:325), "proj" in the 1x1 convolution `proj` of that sum (block.cpp:420; tools/aattn_split_time.py, with cin = C the whole interior).
    `miss` breaks one thing the matcher checks: 'slice_start' (k starts at C - 1), 'shift' (score scale with shift 0.5),
    'axis' (softmax over 1 << 2), 'reader' (the probabilities have a second reader), 'hd16' (pass hd=16), 'area' (the way-out reshape folds the batch
    differently from the way in: (2B, N/2, C); needs area > 1), 'v_reshape' (v reshaped to (B', N', hd, heads); its transpose is {0,3,2,1} so that the
    matmul's shapes still agree: channel d * heads + h instead of h * hd + d).
    -> (plan, x, (wqk, wv, wpe, wproj))"""
    assert miss in (None,) + MISSES and softmax in ("chain", "layer") and tail in ("v", "pe", "proj")
    C, N = heads * hd, H * W
    Ba, Na = B * area, N // area
    rng = np.random.default_rng(seed)
    xr = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    x = xr if x is None else x
    if weights is None:
        wqk = (rng.standard_normal((2 * C, cin, 1, 1)) / np.sqrt(cin) * gain).astype(np.float32)
        wv = (rng.standard_normal((C, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
        wpe = (rng.standard_normal((C, 1, 5, 5)) / 5).astype(np.float32)
        wproj = (rng.standard_normal((C, C, 1, 1)) / np.sqrt(C)).astype(np.float32)
        weights = (wqk, wv, wpe, wproj)
    wqk, wv, wpe, wproj = weights
    net = builder.Network(explicit_batch=True, fp16=fp16)
    try:
        xi = net.input("x", (B, cin, H, W))
        qk = net.out(net.conv(xi, wqk))
        v = net.out(net.conv(xi, wv))
        qk3 = net.out(net.shuffle(qk, reshape=(B, -1, N), perm2=(0, 2, 1)))
        v3 = net.out(net.shuffle(v, reshape=(B, -1, N), perm2=(0, 2, 1)))
        if area > 1:
            qk3 = net.out(net.shuffle(qk3, reshape=(Ba, Na, 2 * C)))
            v3 = net.out(net.shuffle(v3, reshape=(Ba, Na, C)))
        q = net.out(net.slice(qk3, (0, 0, 0), (Ba, Na, C)))
        k = net.out(net.slice(qk3, (0, 0, C - 1 if miss == "slice_start" else C), (Ba, Na, C)))

        def to_heads(t, swapped=False):   # (B', N', C) -> (B', heads, hd, N')
            t = net.out(net.shuffle(t, reshape=(Ba, Na, hd, heads) if swapped else (Ba, Na, heads, hd)))
            return net.out(net.shuffle(t, perm1=(0, 3, 2, 1) if swapped else (0, 2, 3, 1)))
        qh, kh, vh = to_heads(q), to_heads(k), to_heads(v3, miss == "v_reshape")
        qt = net.out(net.shuffle(qh, perm1=(0, 1, 3, 2)))
        s = net.out(net.scale_uniform(net.out(net.matmul(qt, kh)), float(np.float32(1.0 / np.sqrt(hd))), shift=0.5 if miss == "shift" else 0.0))
        axes = 1 << (2 if miss == "axis" else 3)
        if softmax == "layer":
            p = net.out(net.softmax(s, axes=axes))
        else:
            m = net.out(net.reduce(s, "max", axes, True))
            e = net.out(net.unary(net.out(net.elementwise(s, m, "sub")), "exp"))
            p = net.out(net.elementwise(e, net.out(net.reduce(e, "sum", axes, True)), "div"))
        pt = net.out(net.shuffle(p, perm1=(0, 1, 3, 2)))
        if miss == "reader":
            net.mark_output(net.out(net.shuffle(p, perm1=(0, 1, 3, 2))), "p2")
        o = net.out(net.shuffle(net.out(net.matmul(vh, pt)), perm1=(0, 3, 1, 2)))
        if area > 1:
            o = net.out(net.shuffle(o, reshape=(2 * B, N // 2, C) if miss == "area" else (B, N, C)))
        attn_x = net.out(net.shuffle(o, reshape=(B, H, W, C), perm2=(0, 3, 1, 2)))
        other = v if tail == "v" else net.out(net.conv(v, wpe, padding=2, groups=C))
        y = net.out(net.elementwise(attn_x, other))
        net.mark_output(net.out(net.conv(y, wproj)) if tail == "proj" else y, "y")
        plan = net.build()
    finally:
        net.close()
    return plan, x, weights


def attention_f64(q, k, v, heads, area, hd=HD):
    """q, k, v: fp64 [B, N, heads * hd] -> (O [B, N, heads * hd], the scaled scores [B area, heads, Na, Na], softmax @ |v| laid out like O,
    the largest scale * |q|^T |k|): ultralytics' formulation, area a = the pixel range [a Na, (a + 1) Na) of an image"""
    B, N, C = v.shape
    to_heads = lambda t: t.reshape(B * area, N // area, heads, hd).permute(0, 2, 1, 3)   # noqa: E731  (B', heads, N', hd)
    qh, kh, vh = to_heads(q), to_heads(k), to_heads(v)
    scores = (qh @ kh.transpose(-2, -1)) * SCALE
    p = scores.softmax(-1)
    back = lambda z: z.permute(0, 2, 1, 3).reshape(B, N, C)   # noqa: E731
    s_abs = ((qh.abs() @ kh.abs().transpose(-2, -1)) * SCALE).max().item()
    return back(p @ vh), scores, back(p @ vh.abs()), s_abs


def aattn13_reference(x, weights, heads, area, tail="v", rounded=True):
    """fp64 AAttn from the qk and v convolution outputs rounded to fp16 (the engine's storage sites; after aattn_reference in tests/test_yolo12_cpu.py;
    rounded=False: no storage site, what an fp32 graph computes).
    -> O, the other summand (v, or pe(v) from the rounded v), the scores, softmax @ |v|, the largest scale * |q|^T |k|, |wpe| * |v| (pe's fp32 sum of
    magnitudes; None for tail "v"), max |v|: images (B, C, H, W)"""
    wqk, wv, wpe, _ = weights
    B, _, H, W = x.shape
    C = wv.shape[0]
    conv = lambda w, t, **kw: torch.nn.functional.conv2d(t, torch.from_numpy(w).double(), **kw)   # noqa: E731
    xd = torch.from_numpy(x).double()
    qk, v = conv(wqk, xd), conv(wv, xd)
    if rounded:
        qk, v = qk.half().double(), v.half().double()
    nhwc = lambda t: t.flatten(2).transpose(1, 2)               # noqa: E731  (B, N, channels)
    image = lambda t: t.reshape(B, H, W, C).permute(0, 3, 1, 2)   # noqa: E731
    o, scores, pv_abs, s_abs = attention_f64(nhwc(qk)[..., :C], nhwc(qk)[..., C:], nhwc(v), heads, area)
    other, pe_abs = v, None
    if tail == "pe":
        other = conv(wpe, v, padding=2, groups=C)
        pe_abs = conv(np.abs(wpe), v.abs(), padding=2, groups=C)
    return image(o), other, scores, image(pv_abs), s_abs, pe_abs, v.abs().max().item()


def split_operands(case, qkv):
    """An "area" case's qkv [B, N, heads * 96] (head h: q, k, v) -> (q | k [B, N, 2C] with head h's q at h * 32 and its k at C + h * 32, v [B, N, C])"""
    q, k, v = ac.split(case, qkv)   # [B, heads, N, 32] each
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(case.B, case.N, -1)   # noqa: E731
    return torch.cat([flat(q), flat(k)], -1).contiguous(), flat(v).contiguous()


def join_operands(case, qk, v):
    """split_operands' inverse"""
    C = case.heads * ac.KD
    heads = lambda t: t.reshape(case.B, case.N, case.heads, -1)   # noqa: E731
    return torch.cat([heads(qk[..., :C]), heads(qk[..., C:]), heads(v)], -1).reshape(case.B, case.N, case.width).contiguous()
