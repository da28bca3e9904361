"""YOLOv5 on the GPU: the fused anchor head (trtx_yolov5_head_decode_nhwc{,_f32}) through the C ABI against the oracle's C restatement of
the reference plugin (oracle/csrc/yolov5_post_ref.c, pinned on the reference's own kernel in test_ref_pinning.py), and YOLOv5 engines
against the PyTorch twin (fp32), against the fp32 engine (fp16) and against the plugin route of the same build.

The head reads the values the plugin reads (an fp16 element converts to fp32 exactly) and applies the plugin's arithmetic, so the bound
is tests/test_gpu_yolo5.py's: counts, class ids and slot order equal, floats within rtol = atol = 2e-6 (every value passes through
expf: device against glibc, 1 ulp).

Candidates the synthetic models keep (synth.yolov5_state), measured with the fp32 twin (tests/yolov5_twin.py) on the CPU at the engine
tests' seed (12) and sizes, smallest and largest per-image count next to the anchor count 3 * cells:
  n, 32 x 640^2: 11698 - 13569 of 25200     s, 4 x 320^2: 417 - 521 of 6300     s6, 2 x 256^2: 78 - 79 of 4080
  n,  4 x 320^2:  3173 -  3368 of  6300     n, 8 x 128^2: 501 - 538 of 1008     n (seed 5), 2 x 128^2: 484 - 531 of 1008
MAX_OUT is above the anchor count in every engine test: no image can reach it."""
import functools

import numpy as np
import pytest
import torch

from oracle import yolo_post as yp
from tensorrtx_amd import capi, engine, synth
from test_yolov5_cpu import convs_of, yolov5_wts
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk
from yolov5_twin import Yolov5

pytestmark = pytest.mark.gpu
GRIDS = [(80, 80), (40, 40), (20, 20)]
DET = yp.DET5_FLOATS
MAX_OUT = {("n", 640): 25300, ("s", 320): 6400, ("s6", 256): 4200, ("n", 320): 6400, ("n", 128): 1100}   # 3 * cells + a little


def to_nhwc(planes, grid, ld, dtype, pad=(float("nan"),)):
    """[B, C, gh * gw] planes -> [B, gh, gw, ld] with the channels beyond C filled with the `pad` values in turn"""
    gw, gh = grid
    B, C, _ = planes.shape
    t = np.empty((B, gh, gw, ld), np.float32)
    for c in range(C, ld):
        t[..., c] = pad[(c - C) % len(pad)]
    t[..., :C] = planes.reshape(B, C, gh, gw).transpose(0, 2, 3, 1)
    return torch.from_numpy(t).to(dtype)


def as_seen(planes, dtype):
    """the values a tensor of `dtype` holds, as fp32 (what the oracle and the plugin kernel are given)"""
    return [torch.from_numpy(x).to(dtype).float().numpy() for x in planes]


def compare(got, ref):
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    for b in range(ref.shape[0]):
        n = int(ref[b, 0])
        g = got[b, 1:1 + n * DET].reshape(n, DET)
        r = ref[b, 1:1 + n * DET].reshape(n, DET)
        assert np.array_equal(g[:, 5], r[:, 5]), "class ids / slot order"
        assert np.allclose(g[:, :5], r[:, :5], rtol=2e-6, atol=2e-6, equal_nan=True), np.nanmax(np.abs(g[:, :5] - r[:, :5]))


def head(planes, grids, classes, net_h, net_w, anchors, max_out, dtype, gpu, ld, pad=(float("nan"),)):
    hs = [to_nhwc(x, g, ld, dtype, pad).to(gpu) for x, g in zip(planes, grids)]
    return capi.yolov5_head_decode_nhwc(hs, classes, net_h, net_w, grids, anchors, max_out).cpu().numpy()


@functools.lru_cache(maxsize=None)
def seeded(batch, seed, dtype):
    ins = as_seen(synth.yolov5_head_tensors(batch, seed=seed), dtype)
    return ins, yp.v5_decode_c(ins, 80, 640, 640, GRIDS, synth.YOLOV5_ANCHORS, 1000)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("batch,seed", [(1, 0), (4, 1), (32, 2)])
def test_head_matches_oracle(gpu, batch, seed, dtype):
    ins, ref = seeded(batch, seed, dtype)
    assert 50 < ref[:, 0].min() and ref[:, 0].max() < 1000
    got = head(ins, GRIDS, 80, 640, 640, synth.YOLOV5_ANCHORS, 1000, dtype, gpu, 256)
    plug = capi.yolov5_decode([torch.from_numpy(x).to(gpu) for x in ins], 80, 640, 640, GRIDS, synth.YOLOV5_ANCHORS, 1000).cpu().numpy()
    assert np.array_equal(plug[:, 0], ref[:, 0])
    d = max(np.abs(records(got[b]) - records(plug[b])).max() for b in range(batch))
    print(f"B {batch} seed {seed}: candidates {int(ref[:, 0].min())} - {int(ref[:, 0].max())}; largest |fused head - plugin kernel| {d:.3g}"
          f" ({'bit-equal' if d == 0 else 'differs'})")
    compare(got, ref)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("ld", [32, 27])
def test_head_ragged_levels_overflow_empty_and_padding(gpu, dtype, ld):
    """27 channels in pixels of 32 (16-byte loads; the padding holds NaN and a large finite value) and of 27 (element loads)"""
    grids = [(7, 5), (3, 2)]
    anchors = [[4, 5, 8, 9, 12, 7], [20, 30, 25, 18, 40, 44]]
    rng = np.random.default_rng(4)
    ins = [rng.normal(0, 2, size=(3, 3 * 9, gw * gh)).astype(np.float32) for gw, gh in grids]
    for x in ins:
        x[0, 4::9] -= 4.0     # image 0: about one anchor in eight passes
    ins[0][1, 4::9] = -30.0   # image 1: nothing passes
    ins[1][1, 4::9] = -30.0
    ins[0][2, 4::9] = 8.0     # image 2: every anchor of every cell passes -> overflows max_out = 40
    ins[1][2, 4::9] = 8.0
    ins = as_seen(ins, dtype)
    ref = yp.v5_decode_c(ins, 4, 40, 56, grids, anchors, 40)
    assert ref[1, 0] == 0 and ref[2, 0] == 40 and 0 < ref[0, 0] < 40
    got = head(ins, grids, 4, 40, 56, anchors, 40, dtype, gpu, ld, pad=(float("nan"), 60000.0))
    compare(got, ref)


def test_head_class_tie_takes_the_lower_index(gpu):
    """two equal maximal logits, in different lanes (classes 17 and 63) and inside one lane's chunk (40 and 41): the lower index wins"""
    grids = [(3, 2)]
    x = np.full((2, 255, 6), -5.0, np.float32)
    x[:, 4::85] = 3.0
    for k, (lo, hi) in enumerate([(17, 63), (40, 41), (2, 79)]):
        x[:, k * 85 + 5 + lo] = 2.0
        x[:, k * 85 + 5 + hi] = 2.0
    x[1, 5 + 63] = 2.5   # image 1, anchor 0: the higher index is the strict maximum
    for dtype in (torch.float16, torch.float32):
        ref = yp.v5_decode_c([x], 80, 16, 24, grids, synth.YOLOV5_ANCHORS[:1], 100)
        got = head([x], grids, 80, 16, 24, synth.YOLOV5_ANCHORS[:1], 100, dtype, gpu, 256)
        compare(got, ref)
        rec = got[:, 1:1 + 18 * DET].reshape(2, 6, 3, DET)
        assert got[0, 0] == 18 and (rec[0, :, :, 5] == [17, 40, 2]).all() and (rec[1, :, :, 5] == [63, 40, 2]).all()


def test_head_keeps_a_nan_objectness(gpu):
    grids = [(4, 4)]
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, size=(1, 255, 16)).astype(np.float32)
    x[:, 4::85] = -9.0
    x[0, 85 + 4, 5] = np.nan   # anchor 1 of cell 5
    x[0, 4, 11] = 4.0
    for dtype in (torch.float16, torch.float32):
        seen = as_seen([x], dtype)
        ref = yp.v5_decode_c(seen, 80, 32, 32, grids, synth.YOLOV5_ANCHORS[:1], 100)
        assert ref[0, 0] == 2 and np.isnan(ref[0, 1 + 4])   # the reference keeps it: "box_prob < thresh" is false for NaN
        compare(head(seen, grids, 80, 32, 32, synth.YOLOV5_ANCHORS[:1], 100, dtype, gpu, 256), ref)


def test_head_one_cell_level_next_to_a_two_by_two_one(gpu):
    """P6 at a small input: levels of 4 cells and of 1 cell, five cells in a wave of sixteen"""
    grids = [(2, 2), (1, 1)]
    anchors = synth.YOLOV5_P6_ANCHORS[2:]
    rng = np.random.default_rng(11)
    ins = [rng.normal(0, 2, size=(3, 255, gw * gh)).astype(np.float32) for gw, gh in grids]
    for dtype in (torch.float16, torch.float32):
        seen = as_seen(ins, dtype)
        ref = yp.v5_decode_c(seen, 80, 64, 64, grids, anchors, 20)
        assert ref[:, 0].min() > 0
        compare(head(seen, grids, 80, 64, 64, anchors, 20, dtype, gpu, 256), ref)


def test_head_is_batch_invariant(gpu):
    """image 0 of the B = 32 head tensors decodes bit-equal when run alone"""
    ins, _ = seeded(32, 2, torch.float16)
    all32 = head(ins, GRIDS, 80, 640, 640, synth.YOLOV5_ANCHORS, 1000, torch.float16, gpu, 256)
    alone = head([x[:1] for x in ins], GRIDS, 80, 640, 640, synth.YOLOV5_ANCHORS, 1000, torch.float16, gpu, 256)
    assert np.array_equal(all32[:1], alone)


def test_conv1x1_over_16_channels_on_the_mfma_path(gpu, cout=16):
    """YOLOv5n's 16 -> 16 bottleneck convolution now lowers to the implicit-GEMM kernel (two taps per k-step, the second one outside the
    1x1 filter).  Against fp64 on the fp16 operands: one fp16 rounding of the result, fp32 accumulation of 16 products."""
    rng = np.random.default_rng(cout)
    N, H, W = 3, 13, 11   # 429 pixels: ragged last tile
    w = rng.normal(0, 0.3, size=(cout, 16, 1, 1)).astype(np.float32)
    b = rng.normal(0, 0.5, size=cout).astype(np.float32)
    x = torch.from_numpy(rng.normal(0, 1, size=(N, H, W, 16)).astype(np.float32)).half()
    pk, cp, _, _ = capi.pack_conv_weights_f16(w, cin_pad=16)
    bias = torch.zeros(cp)
    bias[:cout] = torch.from_numpy(b)
    y = capi.conv2d_nhwc_f16(x.to(gpu), torch.from_numpy(pk.view(np.int16)).to(gpu), bias.to(gpu), cout, 1, 1, 1, 0, "silu").cpu().double()
    w16 = torch.from_numpy(w).half().double()
    xd = x.double().permute(0, 3, 1, 2)
    pre = torch.nn.functional.conv2d(xd, w16, torch.from_numpy(b).double())
    mag = torch.nn.functional.conv2d(xd.abs(), w16.abs(), torch.from_numpy(b).double().abs())
    ref = torch.nn.functional.silu(pre).permute(0, 2, 3, 1)
    bound = 2.0 ** -11 * ref.abs() + 1e-5 * (mag.permute(0, 2, 3, 1) + 1)
    err = (y - ref).abs()
    print(f"cout {cout}: max err {err.max().item():.3g}, max err / bound {(err / bound).max().item():.3g}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------- engines
def run(plan, x, gpu, batch=None, fill=float("nan")):
    e = engine.Engine(plan)
    B = x.shape[0] if batch is None else batch
    bufs = []
    for i in range(e.nb_bindings):
        if e.is_input[i]:
            bufs.append(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu))
        else:
            bufs.append(torch.full((e.max_batch * int(np.prod(e.dims[i])),), fill, dtype=torch.float32, device=gpu))
    e.enqueue(B, bufs)
    torch.cuda.synchronize()
    out = {e.names[i]: bufs[i].cpu() for i in range(e.nb_bindings) if not e.is_input[i]}
    e.close()
    return out


def kinds(plan):
    return [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]]


def records(row):
    n = int(row[0])
    return row[1:1 + n * DET].reshape(n, DET)[:, :6]


def match_detections(dec, dec_ref, max_out, gpu, skip=None):
    """tests/test_gpu_yolo12.py's matching on centre-format records (cx, cy, w, h, conf, class): per reference candidate the candidate of
    the same class with the nearest centre, matched when their IoU is above 0.9.  No image may be left out (every count is below
    max_out).  skip: per image a bool per reference record (candidates within 0.02 of the gate), or None."""
    st = dict(ref=0, matched=0, min_iou=1.0, unmatched_by_class={})
    for b in range(dec_ref.shape[0]):
        assert dec_ref[b, 0] < max_out and dec[b, 0] < max_out, (b, dec_ref[b, 0], dec[b, 0], max_out)
        R, G = torch.from_numpy(records(dec_ref[b])).to(gpu), torch.from_numpy(records(dec[b])).to(gpu)
        if skip is not None:
            R = R[~torch.from_numpy(skip[b]).to(gpu)]
        st["ref"] += len(R)
        for c in torch.unique(R[:, 5]).tolist():
            r, g = R[R[:, 5] == c], G[G[:, 5] == c]
            if len(g) == 0:
                st["unmatched_by_class"][int(c)] = st["unmatched_by_class"].get(int(c), 0) + len(r)
                continue
            # centre distance and IoU of every (reference, candidate) pair in plain element-wise arithmetic, then the IoU at the nearest
            # centre: the largest IoU among the candidates at the smallest distance
            d = (r[:, None, 0] - g[None, :, 0]).abs() + (r[:, None, 1] - g[None, :, 1]).abs()
            lo = lambda t, k: (t[:, k] - t[:, k + 2] / 2)  # noqa: E731
            hi = lambda t, k: (t[:, k] + t[:, k + 2] / 2)  # noqa: E731
            ix = (torch.minimum(hi(r, 0)[:, None], hi(g, 0)[None]) - torch.maximum(lo(r, 0)[:, None], lo(g, 0)[None])).clamp(min=0)
            iy = (torch.minimum(hi(r, 1)[:, None], hi(g, 1)[None]) - torch.maximum(lo(r, 1)[:, None], lo(g, 1)[None])).clamp(min=0)
            pair = ix * iy / ((r[:, 2] * r[:, 3])[:, None] + (g[:, 2] * g[:, 3])[None] - ix * iy)
            iou = torch.where(d <= d.min(1, keepdim=True).values, pair, torch.full_like(pair, -1.0)).max(1).values
            ok = iou > 0.9
            st["matched"] += int(ok.sum())
            if not ok.all():
                st["unmatched_by_class"][int(c)] = st["unmatched_by_class"].get(int(c), 0) + int((~ok).sum())
            if ok.any():
                st["min_iou"] = min(st["min_iou"], float(iou[ok].min()))
    return st


def near_gate(heads, counts, margin=0.02):
    """Per image, for the records an engine wrote from `heads` ([B, 255, cells] per level) in canonical (level, cell, anchor) order:
    is the objectness probability within `margin` of the 0.1 gate"""
    B = heads[0].shape[0]
    obj = np.concatenate([h.reshape(B, 3, 85, -1)[:, :, 4].transpose(0, 2, 1).reshape(B, -1) for h in heads], 1).astype(np.float32)
    p = np.float32(1) / (np.float32(1) + np.exp(-obj))
    out = []
    for b in range(B):
        kept = ~(p[b] < np.float32(0.1))
        assert kept.sum() == counts[b], (b, kept.sum(), counts[b])   # (an objectness within an ulp of the gate would break this: not at these seeds)
        out.append(np.abs(p[b][kept] - 0.1) < margin)
    return out


def test_yolov5n_fp32_engine_matches_twin(gpu):
    path, sd = yolov5_wts("n")
    B, S, mo = 2, 128, MAX_OUT[("n", 128)]
    plan = engine.build_plan("yolov5n", path, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo)
    x = synth.images(B, S, S, seed=5)
    got = run(plan, x, gpu)
    tw = Yolov5(sd, "n")
    with torch.inference_mode():
        heads, strides = tw.heads(torch.from_numpy(x))
    mine = []
    for i, h in enumerate(heads):
        g = got[f"head{i}"].reshape(h.shape)
        err = (g - h).abs().max().item()
        print(f"head{i}: err {err:.3g}, |head| {h.abs().max().item():.3g}")
        assert err <= 1e-4 * max(1.0, h.abs().max().item()), (i, err)
        mine.append(g.numpy())
    grids = [(S // s, S // s) for s in strides]
    ref = yp.v5_decode_c(mine, 80, S, S, grids, tw.anchors(), mo)
    assert 0 < ref[:, 0].min() and ref[:, 0].max() < mo
    compare(got["prob"].reshape(B, -1).numpy(), ref)


@pytest.mark.parametrize("name,B,S", [("n", 32, 640), ("s", 4, 320), ("s6", 2, 256)])
def test_yolov5_fp16_engine_tracks_fp32_engine(name, B, S, gpu):
    """fp16 storage, fp32 accumulation, against the fp32 engine: head values within fp16_walk(sites, max |head|) with two sites per
    convolution (packed weights, stored output); detections of the fused head (no marked heads) matched as parity.py asks, candidates
    whose objectness is within 0.02 of the 0.1 gate skipped, no image left out"""
    path, _ = yolov5_wts(name)
    x = synth.images(B, S, S, seed=12)
    mo = MAX_OUT[(name, S)]
    model = "yolov5" + name
    p16 = engine.build_plan(model, path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    p16h = engine.build_plan(model, path, batch=B, h=S, w=S, fp16=1, mark_heads=1, max_out=mo)
    p32h = engine.build_plan(model, path, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo)
    k = kinds(p16)
    assert k.count("yolo5_head") == 1 and "plugin" not in k and "to_linear" not in k
    sites = 2 * len(convs_of(engine.describe_plan(p16, lowered=True)))
    g16, g16h, g32 = run(p16, x, gpu), run(p16h, x, gpu), run(p32h, x, gpu)
    levels = 4 if name.endswith("6") else 3
    h32 = []
    for i in range(levels):
        a, r = g16h[f"head{i}"], g32[f"head{i}"]
        assert torch.isfinite(a).all()
        err, lim = (a - r).abs().max().item(), fp16_walk(sites, r.abs().max().item())
        print(f"{model} B{B} {S}: head{i} err {err:.3g}, bound {lim:.3g} ({sites} sites)")
        assert err <= lim, i
        h32.append(r.reshape(B, 255, -1).numpy())
    ref = g32["prob"].reshape(B, -1).numpy()
    st = match_detections(g16["prob"].reshape(B, -1).numpy(), ref, mo, gpu, skip=near_gate(h32, ref[:, 0]))
    print(st, "counts", ref[:, 0].min(), "-", ref[:, 0].max())
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_agrees_with_the_plugin_route(gpu, monkeypatch):
    """The fused fp16 plan against the plan the same build makes with TRTX_YOLO5_HEAD=0 (layout passes + plugin, 255-channel stores).
    Two plans, each with its own tactics: matched as above, not bit-compared - and with no candidate skipped."""
    path, _ = yolov5_wts("n")
    B, S = 4, 320
    mo = MAX_OUT[("n", S)]
    x = synth.images(B, S, S, seed=12)
    fused = engine.build_plan("yolov5n", path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    assert kinds(fused).count("yolo5_head") == 1
    a = run(fused, x, gpu)["prob"].reshape(B, -1).numpy()
    monkeypatch.setenv("TRTX_YOLO5_HEAD", "0")
    route = engine.build_plan("yolov5n", path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    k = kinds(route)
    assert k.count("plugin") == 1 and k.count("yolo5_head") == 0 and k.count("to_linear") == 3
    r = run(route, x, gpu)["prob"].reshape(B, -1).numpy()
    st = match_detections(a, r, mo, gpu)
    print(st, "counts fused", a[:, 0], "plugin route", r[:, 0])
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_below_its_maximum_batch(gpu):
    """a max_batch = 8 plan enqueued with batch 3 decodes three images and leaves the other output rows untouched"""
    path, _ = yolov5_wts("n")
    S, mo = 128, MAX_OUT[("n", 128)]
    plan = engine.build_plan("yolov5n", path, batch=8, h=S, w=S, fp16=1, max_out=mo)
    assert kinds(plan).count("yolo5_head") == 1
    x = synth.images(8, S, S, seed=12)
    full = run(plan, x, gpu)["prob"].reshape(8, -1).numpy()
    part = run(plan, x, gpu, batch=3)["prob"].reshape(8, -1).numpy()
    assert np.isnan(part[3:]).all()
    assert (part[:3, 0] > 0).all() and (part[:3, 0] < mo).all()
    for b in range(3):
        assert np.isfinite(records(part[b])).all()
    st = match_detections(part[:3], full[:3], mo, gpu)
    print(st, "counts", part[:3, 0], full[:, 0])
    assert st["ref"] > 0 and st["matched"] / st["ref"] >= 1 - FP16_MATCH and st["min_iou"] >= 1 - FP16_IOU, st
