"""YOLO11 on the GPU: the depthwise kernel and the fused PSA attention against torch in fp64, the batched (broadcast) matmul, and
YOLO11 engines against the oracle's interpreter (fp32) and against the fp32 engine (fp16).

fp16 bounds come from parity.fp16_walk(sites, magnitude) with the rounding sites of each path counted:
  * depthwise op: the site count (3, against the unrounded fp32 input and residual) is derived next to the kernel-level bound in tests/dw_cases.py,
    on a magnitude of L * (|w| * |x|) + |r| per element (L = 1.1 bounds SiLU's slope);
  * attention op: the reference is computed from the qkv tensor rounded to fp16 (the storage site the engine has by design); the kernel
    then adds fp32 arithmetic and ONE rounding at the O store (P and O stay fp32): 1 site on |O|, plus the first-order effect of a one-ulp
    disagreement between the fp32 and the fp64 rounding of q / k (u * scale * sum_j |q_j k_j| on the scores, times max |v|);
  * engines: every convolution's packed weights and every stored activation is a site (counted from the plan: weights + outputs of the
    convolutions, + the attention's O), on the largest fp32 head value; the detections through the matched fraction / IoU of parity.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import builder, engine, synth
from test_yolo11_cpu import yolo11_wts
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk

pytestmark = pytest.mark.gpu
U16 = 2.0 ** -11


def _run(plan, inputs, gpu):
    e = engine.Engine(plan)
    explicit = engine.describe_plan(plan)["explicit_batch"]
    batch = next(iter(inputs.values())).shape[0]
    bufs = []
    for i in range(e.nb_bindings):
        if e.is_input[i]:
            bufs.append(torch.from_numpy(np.ascontiguousarray(inputs[e.names[i]], dtype=np.float32)).to(gpu))
        else:
            n = int(np.prod(e.dims[i])) * (1 if explicit else batch)
            bufs.append(torch.full((n,), float("nan"), dtype=torch.float32, device=gpu))
    e.enqueue(batch, bufs)
    torch.cuda.synchronize()
    out = {e.names[i]: bufs[i].cpu() for i in range(e.nb_bindings) if not e.is_input[i]}
    e.close()
    return out


CASES = [(c, hw, s, k, silu, res, fp16)
         for c, hw in ((24, (80, 80)), (64, (80, 80)), (80, (40, 40)), (128, (13, 17)), (256, (40, 40)), (64, (13, 17)), (20, (13, 17)), (36, (40, 40)))
         for s in (1, 2) for k in (3, 5)
         for silu, res in ((True, False), (False, True), (True, True))
         for fp16 in (0, 1)
         if not (res and s == 2)]


@pytest.mark.parametrize("c,hw,stride,k,silu,res,fp16", CASES)
def test_depthwise_op_matches_torch(c, hw, stride, k, silu, res, fp16, gpu):
    B = 2
    H, W = hw
    rng = np.random.default_rng(c * 131 + H + 7 * stride + k)
    x = rng.standard_normal((B, c, H, W)).astype(np.float32)
    w = (rng.standard_normal((c, 1, k, k)) / k).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32) * 0.1
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    r = rng.standard_normal((B, c, Ho, Wo)).astype(np.float32)
    net = builder.Network(max_batch=B, fp16=bool(fp16))
    try:
        xi = net.input("x", (c, H, W))
        y = net.out(net.conv(xi, w, bias, stride=stride, padding=k // 2, groups=c))
        if silu:
            y = net.out(net.elementwise(y, net.out(net.activation(y, "sigmoid")), op=1))
        if res:
            y = net.out(net.elementwise(y, net.input("r", (c, Ho, Wo)), op=0))
        net.mark_output(y, "y")
        plan = net.build()
    finally:
        net.close()
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    assert [o.get("dw", False) for o in ops if o["kind"] == "conv"] == [True]
    ins = {"x": x, "r": r} if res else {"x": x}
    got = _run(plan, ins, gpu)["y"].reshape(B, c, Ho, Wo).double()
    xd, wd = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    ref = F.conv2d(xd, wd, torch.from_numpy(bias).double(), stride, k // 2, 1, c)
    mag = F.conv2d(xd.abs(), wd.abs(), torch.from_numpy(bias).double().abs(), stride, k // 2, 1, c)
    if silu:
        ref = F.silu(ref)
    if res:
        ref = ref + torch.from_numpy(r).double()
    err = (got - ref).abs()
    if fp16:
        bound = fp16_walk(3, 1.1 * mag + (torch.from_numpy(r).double().abs() if res else 0))
        assert (err <= bound + 1e-7).all(), (err - bound).max().item()
    else:
        assert (err <= 1e-5 * (mag + ref.abs()) + 1e-7).all(), err.max().item()


@pytest.mark.parametrize("fp16", [0, 1])
def test_depthwise_writes_into_a_concat_slice(fp16, gpu):
    """The depthwise output lives at channel offset 8 of a concat buffer (ld = C + 8 != C): the kernel's strided store"""
    B, c, H, W = 2, 24, 20, 20
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, c, H, W)).astype(np.float32)
    w = (rng.standard_normal((c, 1, 3, 3)) / 3).astype(np.float32)
    w1 = (rng.standard_normal((8, c, 1, 1)) / 5).astype(np.float32)
    net = builder.Network(max_batch=B, fp16=bool(fp16))
    try:
        xi = net.input("x", (c, H, W))
        a = net.out(net.conv(xi, w1))
        d = net.out(net.conv(xi, w, None, stride=1, padding=1, groups=c))
        net.mark_output(net.out(net.concat([a, d])), "y")
        plan = net.build()
    finally:
        net.close()
    (dw,) = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o.get("dw")]
    assert dw["ld_out"] >= c + 8
    got = _run(plan, {"x": x}, gpu)["y"].reshape(B, c + 8, H, W)[:, 8:].double()
    xd = torch.from_numpy(x).double()
    ref = F.conv2d(xd, torch.from_numpy(w).double(), None, 1, 1, 1, c)
    mag = F.conv2d(xd.abs(), torch.from_numpy(w).double().abs(), None, 1, 1, 1, c)
    bound = fp16_walk(2, mag) if fp16 else 1e-5 * mag
    assert ((got - ref).abs() <= bound + 1e-7).all()


def _attention_net(B, heads, H, W, kd=32, hd=64, gain=1.0, seed=0):
    """The Attention subgraph of yolo11/src/block.cpp:287-339 on a 1x1 qkv convolution, O + V summed into the output (so that both
    of the fused op's results have a reader)"""
    C = heads * (2 * kd + hd)
    cin = 16
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    wq = (rng.standard_normal((C, cin, 1, 1)) / 4).astype(np.float32)
    for h in range(heads):   # q / k channels scaled by `gain`: scores up to +-60 for the large case
        wq[h * (2 * kd + hd):h * (2 * kd + hd) + 2 * kd] *= gain
    N = H * W
    net = builder.Network(explicit_batch=True, fp16=True)
    try:
        xi = net.input("x", (B, cin, H, W))
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
        plan = net.build()
    finally:
        net.close()
    return plan, x, wq


@pytest.mark.parametrize("heads,hw,B,gain", [(1, (7, 9), 1, 1.0), (2, (10, 10), 3, 1.0), (4, (20, 20), 3, 1.0), (6, (7, 9), 3, 1.0),
                                             (2, (20, 20), 32, 1.0), (1, (40, 40), 1, 1.0), (4, (40, 40), 3, 1.0), (2, (10, 10), 1, 6.0),
                                             (2, (7, 9), 3, 6.0)])
def test_attention_op_matches_torch(heads, hw, B, gain, gpu):
    H, W = hw
    kd, hd = 32, 64
    plan, x, wq = _attention_net(B, heads, H, W, gain=gain, seed=heads * 7 + H)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    assert [o["kind"] for o in ops].count("attention") == 1
    assert not {"matmul", "softmax", "gather"} & {o["kind"] for o in ops}
    got = _run(plan, {"x": x}, gpu)["y"].reshape(B, heads * hd, H, W).double()
    N = H * W
    qkv = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wq).double()).half().double()   # the fp16 storage site
    q, k, v = qkv.view(B, heads, 2 * kd + hd, N).split([kd, kd, hd], dim=2)
    sc = kd ** -0.5
    scores = (q.transpose(-2, -1) @ k) * sc
    if gain > 1:
        assert scores.abs().max().item() > 40   # the large-score case: softmax without max subtraction overflows
        assert (scores.softmax(-1).max(-1).values > 0.99).float().mean().item() > 0.3   # rows one key dominates
    o = (v @ scores.softmax(-1).transpose(-2, -1)).reshape(B, heads * hd, H, W)
    ref = o + v.reshape(B, heads * hd, H, W)
    s_abs = ((q.abs().transpose(-2, -1) @ k.abs()) * sc).max().item()
    vmax = v.abs().max().item()
    # O store + the V copy (exact) + the sum's own fp16 store: 2 sites on |O| + |V|; one-ulp q / k disagreements move a score by at most
    # 2 u s_abs, the output by that times max |v|
    bound = fp16_walk(2, o.abs() + v.abs().reshape(B, heads * hd, H, W)) + 2 * 2.0 ** -11 * s_abs * vmax + 1e-4 * vmax
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err - bound).max().item()


def test_batched_matmul_with_broadcast(gpu):
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((2, 3, 5, 7)).astype(np.float32), rng.standard_normal((1, 3, 7, 4)).astype(np.float32)
    net = builder.Network(explicit_batch=True)
    try:
        mm = net.matmul(net.input("a", a.shape), net.input("b", b.shape))
        net.mark_output(net.out(mm), "y")
        plan = net.build()
    finally:
        net.close()
    got = _run(plan, {"a": a, "b": b}, gpu)["y"].reshape(2, 3, 5, 4)
    assert torch.allclose(got, torch.from_numpy(a) @ torch.from_numpy(b), atol=1e-5)


@pytest.fixture(scope="module")
def y11n_fp32_640_b8():
    path, _ = yolo11_wts("n")
    B, S = 8, 640
    plan = engine.build_plan("yolo11n", path, batch=B, h=S, w=S, fp16=0, mark_heads=1)
    x = synth.images(B, S, S, seed=11)
    return plan, x


def test_yolo11n_fp32_engine_matches_interpreter(y11n_fp32_640_b8, gpu):
    plan, x = y11n_fp32_640_b8
    B = x.shape[0]
    got = _run(plan, {"images": x}, gpu)
    ref = gi.run(engine.describe_plan(plan), plan, {"images": x}, batch=B)
    for i in range(3):
        h = ref[f"head{i}"]
        err = (got[f"head{i}"].reshape(h.shape) - h).abs().max().item()
        assert err <= 1e-4 * max(1.0, h.abs().max().item()), (i, err)
    # the plugin decodes all 8 images (explicit-batch rule): the reference decode of the engine's own heads
    dec = yp.decode_c([got[f"head{i}"].reshape(ref[f"head{i}"].shape).numpy() for i in range(3)], 80, 640, 640, [8, 16, 32])
    out = got["output"].reshape(B, -1).numpy()
    for b in range(B):   # the plugin writes the count and that many detections; the rest of the binding is not its output
        n = min(int(out[b, 0]), 1000)
        assert n > 0 and out[b, 0] == dec[b, 0], b
        got_d = out[b, 1:1 + n * yp.DET_FLOATS].reshape(n, yp.DET_FLOATS)[:, :6]   # bbox, conf, class (a det plan writes no mask / keypoints)
        ref_d = dec[b, 1:1 + n * yp.DET_FLOATS].reshape(n, yp.DET_FLOATS)[:, :6]
        # the plugin appends through an atomic counter: slot order is not fixed - sort on (class, box rounded to 0.01 px)
        rows = lambda a: a[np.lexsort(np.round(a[:, [3, 2, 1, 0, 5]], 2).T)]  # noqa: E731
        g_, r_ = rows(got_d), rows(ref_d)
        # same cells, same classes; the device decode's exp / division round within a few ulp of the host restatement's
        assert np.array_equal(g_[:, 5], r_[:, 5]), b
        assert np.allclose(g_, r_, rtol=1e-5, atol=1e-4), (b, np.abs(g_ - r_).max())


def _match_detections(dec, dec_ref, max_out, conf_margin=0.02):
    """tests/test_gpu_engine.py's matching for a plan of `max_out` slots: every reference candidate not within `conf_margin` of the
    0.1 gate must appear with the same class and a box of IoU > 0.9 (candidates come from distinct cells: matched on box centre)"""
    st = dict(ref=0, matched=0, min_iou=1.0)
    for b in range(dec_ref.shape[0]):
        nr, ng = int(dec_ref[b, 0]), int(dec[b, 0])
        if nr >= max_out or ng >= max_out:
            continue
        R = dec_ref[b, 1:1 + nr * yp.DET_FLOATS].reshape(nr, yp.DET_FLOATS)[:, :6]
        G = dec[b, 1:1 + ng * yp.DET_FLOATS].reshape(ng, yp.DET_FLOATS)[:, :6]
        for r in R:
            if abs(r[4] - 0.1) < conf_margin:
                continue
            st["ref"] += 1
            same = np.nonzero(G[:, 5] == r[5])[0]
            if len(same) == 0:
                continue
            c = np.abs((G[same, 0] + G[same, 2]) - (r[0] + r[2])) + np.abs((G[same, 1] + G[same, 3]) - (r[1] + r[3]))
            g = G[same[np.argmin(c)]]
            ix = max(0.0, min(r[2], g[2]) - max(r[0], g[0])) * max(0.0, min(r[3], g[3]) - max(r[1], g[1]))
            ua = (r[2] - r[0]) * (r[3] - r[1]) + (g[2] - g[0]) * (g[3] - g[1]) - ix
            iou = ix / ua if ua > 0 else 0.0
            if iou > 0.9:
                st["matched"] += 1
                st["min_iou"] = min(st["min_iou"], float(iou))
    return st


def _sites(plan):
    """fp16 rounding sites of a plan: every convolution's packed weights and stored output, + the attention's O"""
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    convs = [o for o in ops if o["kind"] == "conv"] + [m for o in ops if o["kind"] == "conv_group" for m in o["members"]]
    return 2 * len(convs) + sum(o["kind"] == "attention" for o in ops)


@pytest.mark.parametrize("scale,B,S", [("n", 32, 640), ("s", 8, 640), ("n", 2, 1280)])
def test_yolo11_fp16_engine_tracks_fp32_engine(scale, B, S, gpu):
    """fp16 storage, fp32 accumulation, against the fp32 engine (pinned on the interpreter above, within 1e-4): head values within
    fp16_walk(sites, max |head|), detections of the fused head (no marked heads) matched as parity.py asks"""
    path, _ = yolo11_wts(scale)
    x = synth.images(B, S, S, seed=12)
    mo = 10000   # the synthetic class head passes a few thousand cells per image at 1280 / for yolo11s: room for all of them
    p16 = engine.build_plan("yolo11" + scale, path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    p16h = engine.build_plan("yolo11" + scale, path, batch=B, h=S, w=S, fp16=1, mark_heads=1, max_out=mo)
    p32h = engine.build_plan("yolo11" + scale, path, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo)
    kinds = [o["kind"] for o in engine.describe_plan(p16, lowered=True)["ops"]]
    assert kinds.count("attention") == 1 and kinds.count("yolo_head") == 1
    sites = _sites(p16)
    g16, g16h, g32 = _run(p16, {"images": x}, gpu), _run(p16h, {"images": x}, gpu), _run(p32h, {"images": x}, gpu)
    for i in range(3):
        h16, h32 = g16h[f"head{i}"], g32[f"head{i}"]
        assert torch.isfinite(h16).all()
        assert (h16 - h32).abs().max().item() <= fp16_walk(sites, h32.abs().max().item()), i
    st = _match_detections(g16["output"].reshape(B, -1).numpy(), g32["output"].reshape(B, -1).numpy(), mo)
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st
