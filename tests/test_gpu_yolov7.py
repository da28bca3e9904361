"""YOLOv7 on the GPU: trtx_yolov7_nms on 6-float records through the C ABI against the oracle's C restatement of the reference's YOLOv5
nms (oracle/csrc/yolov5_post_ref.c, pinned on the reference's own kernel in test_ref_pinning.py), and YOLOv7 engines against the PyTorch
twin (fp32), against the fp32 engine (fp16) and against the plugin route.  The 6-float decode kernels (trtx_yolov7_decode,
trtx_yolov7_head_decode_nhwc{,_f32}) are the YOLOv5 ones at another record length: tests/test_gpu_anchor_head.py runs both families.

The bound is tests/test_gpu_yolov5.py's: counts, class ids and slot order equal, floats within rtol = atol = 2e-6 (every value passes
through expf: device against glibc, 1 ulp).

Candidates the synthetic models keep (synth.yolov7_state, seed 0, 80 classes), measured with the fp64 twin (tests/yolov7_twin.py) on the
CPU at the engine tests' image seeds and sizes, smallest - largest per-image count next to the anchor count 3 * cells:
  yolov7tiny, 2 x 128^2 (seed 5): 99 - 191 of 1008      yolov7tiny, 4 x 128^2 (seed 12): 143 - 183 of 1008
  yolov7,     2 x 128^2 (seed 5): 71 - 71 of 1008       yolov7x,    1 x  64^2 (seed 5): 22 of 252
  yolov7w6,   1 x 128^2 (seed 5): 72 of 1020            yolov7w6,   1 x 128^2 (seed 12): 72 of 1020
  yolov7e6,   1 x 128^2 (seed 5): 85 of 1020            yolov7tiny, 8 x 128^2 (seed 12): 124 - 195 of 1008
(The SiLU models' random backbones give features that hardly depend on the image: their counts are the same from image to image.)
MAX_OUT is above the anchor count in every engine test: no image can reach it."""
import numpy as np
import pytest
import torch

from oracle import yolo_post as yp
from tensorrtx_amd import capi, engine, synth
from test_gpu_yolov5 import kinds, run
from test_yolov7_cpu import convs_of, records6, strides_of, yolov7_wts
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk
from yolov7_twin import Yolov7

pytestmark = pytest.mark.gpu
DET = capi.DET7_FLOATS


def oracle(ins, classes, net_h, net_w, grids, anchors, max_out):
    """the YOLOv5 oracle's 38-float records cut to YOLOv7's six"""
    return records6(yp.v5_decode_c(ins, classes, net_h, net_w, grids, anchors, max_out), max_out)


def records(row):
    n = int(row[0])
    return row[1:1 + n * DET].reshape(n, DET)


def compare(got, ref):
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    for b in range(ref.shape[0]):
        g, r = records(got[b]), records(ref[b])
        assert np.array_equal(g[:, 5], r[:, 5]), "class ids / slot order"
        assert np.allclose(g[:, :5], r[:, :5], rtol=2e-6, atol=2e-6, equal_nan=True), np.nanmax(np.abs(g[:, :5] - r[:, :5]))


def clustered(batch, max_out, seed, fill=None):
    """records in clusters of overlapping boxes: [B, 1 + max_out * 6]"""
    rng = np.random.default_rng(seed)
    out = np.zeros((batch, 1 + max_out * DET), np.float32)
    for b in range(batch):
        n = max_out if fill == "full" else (0 if fill == "empty" and b == 0 else int(rng.integers(max_out // 3, max_out - 3)))
        c = rng.uniform(50, 590, size=(max(n // 6, 1), 2))
        rec = np.zeros((n, DET), np.float32)
        k = rng.integers(0, len(c), size=n)
        rec[:, :2] = c[k] + rng.normal(0, 6, size=(n, 2))
        rec[:, 2:4] = rng.uniform(30, 90, size=(n, 2))
        rec[:, 4] = rng.uniform(0.05, 1.0, size=n)
        rec[:, 5] = rng.integers(0, 4, size=n)
        if n > 8:
            rec[3, 4] = rec[7, 4] = np.float32(0.5)   # exactly at the threshold: dropped
        out[b, 0] = n
        out[b, 1:1 + n * DET] = rec.flatten()
    return out


def widen(dec6, max_out):
    """the same boxes as 38-float records"""
    B = dec6.shape[0]
    out = np.zeros((B, 1 + max_out * 38), np.float32)
    out[:, 0] = dec6[:, 0]
    wide = out[:, 1:].reshape(B, max_out, 38)
    wide[:, :, :6] = dec6[:, 1:].reshape(B, max_out, DET)
    return out


@pytest.mark.parametrize("fill", [None, "empty", "full"])
def test_nms_matches_the_oracle(gpu, fill):
    mo = 300
    dec = clustered(3, mo, 21, fill)
    ki, kc, kd = yp.v5_batch_nms_c(widen(dec, mo), mo, 0.5, 0.45)
    gi_, gc, gd = capi.yolov7_nms(torch.from_numpy(dec).to(gpu), mo, 0.5, 0.45)
    gi_, gc, gd = gi_.cpu().numpy(), gc.cpu().numpy(), gd.cpu().numpy()
    print(f"nms {fill}: counts {dec[:, 0].astype(int).tolist()} -> kept {kc.tolist()}")
    assert np.array_equal(gc, kc)
    if fill == "empty":
        assert kc[0] == 0
    for b in range(3):
        n = int(kc[b])
        assert 0 < n < dec[b, 0] or dec[b, 0] == 0
        assert np.array_equal(gi_[b, :n], ki[b, :n])
        assert np.array_equal(gd[b, :n].view(np.int32), kd[b, :n].view(np.int32))
        at = records(dec[b])[gi_[b, :n]]
        assert (at[:, 4] > 0.5).all()   # the two records at exactly 0.5 are gone


# ---------------------------------------------------------------------------------------------------------------- engines
def max_out_of(name, S):
    return 3 * sum((S // s) ** 2 for s in strides_of(name)) + 92


def match_detections(dec, dec_ref, max_out, gpu, skip=None):
    """match_detections of tests/test_gpu_yolov9.py on centre-format 6-float records (cx, cy, w, h, conf, class): per reference candidate
    the candidate of the same class with the nearest centre, matched when their IoU is above 0.9.  No image may be left out (every count
    is below max_out).  skip: per image a bool per reference record (candidates within 0.02 of the gate), or None."""
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


@pytest.mark.parametrize("name,B,S,fold", [("yolov7tiny", 2, 128, 1), ("yolov7", 2, 128, 1), ("yolov7x", 1, 64, 1), ("yolov7w6", 1, 128, 1),
                                           ("yolov7w6", 1, 128, 0), ("yolov7e6", 1, 128, 1)])
def test_fp32_engine_matches_twin(gpu, monkeypatch, name, B, S, fold):
    """heads within 1e-4 * max(1, |head|) of the fp64 twin (the YOLOv9 tests' bound); tiny and v7: the engine's output against the oracle
    decode of its own heads; w6 once more with the gathers instead of the folded ReOrg"""
    if not fold:
        monkeypatch.setenv("TRTX_REORG_FOLD", "0")
    path, sd = yolov7_wts(name)
    mo = max_out_of(name, S)
    plan = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo)
    k = kinds(plan)
    assert k.count("gather") == (0 if fold else 4) and k.count("pool_chain") == 1
    x = synth.images(B, S, S, seed=5)
    got = run(plan, x, gpu)
    tw = Yolov7(sd, name)
    with torch.inference_mode():
        heads, strides = tw.heads(torch.from_numpy(x))
    mine = []
    for i, h in enumerate(heads):
        g = got[f"head{i}"].reshape(h.shape)
        err = (g - h).abs().max().item()
        print(f"{name} head{i}: err {err:.3g}, |head| {h.abs().max().item():.3g}")
        assert err <= 1e-4 * max(1.0, h.abs().max().item()), (i, err)
        mine.append(g.reshape(B, 255, -1).numpy())
    prob = got["prob"].reshape(B, -1).numpy()
    print(f"{name}: candidates {prob[:, 0].astype(int).tolist()} of {mo - 92} anchors")
    assert 0 < prob[:, 0].min() and prob[:, 0].max() < mo
    if name in ("yolov7tiny", "yolov7"):
        grids = [(S // s, S // s) for s in strides]
        compare(prob, oracle(mine, 80, S, S, grids, tw.anchors(), mo))


@pytest.mark.parametrize("name,B,S", [("yolov7tiny", 4, 128), ("yolov7w6", 1, 128)])
def test_fp16_engine_tracks_fp32_engine(name, B, S, gpu):
    """fp16 storage, fp32 accumulation, against the fp32 engine: head values within fp16_walk(sites, max |head|) with two sites per
    convolution (packed weights, stored output); detections of the fused head (no marked heads) matched as parity.py asks, candidates
    whose objectness is within 0.02 of the 0.1 gate skipped, no image left out"""
    path, _ = yolov7_wts(name)
    x = synth.images(B, S, S, seed=12)
    mo = max_out_of(name, S)
    p16 = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    p16h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1, max_out=mo)
    p32h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo)
    k = kinds(p16)
    assert k.count("yolo7_head") == 1 and "plugin" not in k and "to_linear" not in k and "gather" not in k
    sites = 2 * len(convs_of(engine.describe_plan(p16, lowered=True)))
    g16, g16h, g32 = run(p16, x, gpu), run(p16h, x, gpu), run(p32h, x, gpu)
    h32 = []
    for i in range(len(strides_of(name))):
        a, r = g16h[f"head{i}"], g32[f"head{i}"]
        assert torch.isfinite(a).all()
        err, lim = (a - r).abs().max().item(), fp16_walk(sites, r.abs().max().item())
        print(f"{name} B{B} {S}: head{i} err {err:.3g}, bound {lim:.3g} ({sites} sites)")
        assert err <= lim, i
        h32.append(r.reshape(B, 255, -1).numpy())
    ref = g32["prob"].reshape(B, -1).numpy()
    skip = near_gate(h32, ref[:, 0])
    st = match_detections(g16["prob"].reshape(B, -1).numpy(), ref, mo, gpu, skip=skip)
    print(st, "counts", ref[:, 0].min(), "-", ref[:, 0].max(), "skipped near the gate", [int(s.sum()) for s in skip])
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_agrees_with_the_plugin_route(gpu, monkeypatch):
    """The fused fp16 plan against the plan the same build makes with TRTX_YOLO7_HEAD=0 (layout passes + the 6-float plugin, 255-channel
    stores).  Two plans, each with its own tactics: matched as above, not bit-compared - and with no candidate skipped."""
    path, _ = yolov7_wts("yolov7tiny")
    B, S = 4, 128
    mo = max_out_of("yolov7tiny", S)
    x = synth.images(B, S, S, seed=12)
    fused = engine.build_plan("yolov7tiny", path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    assert kinds(fused).count("yolo7_head") == 1
    a = run(fused, x, gpu)["prob"].reshape(B, -1).numpy()
    monkeypatch.setenv("TRTX_YOLO7_HEAD", "0")
    route = engine.build_plan("yolov7tiny", path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    k = kinds(route)
    assert k.count("plugin") == 1 and k.count("yolo7_head") == 0 and k.count("to_linear") == 3
    r = run(route, x, gpu)["prob"].reshape(B, -1).numpy()
    st = match_detections(a, r, mo, gpu)
    print(st, "counts fused", a[:, 0], "plugin route", r[:, 0])
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_below_its_maximum_batch(gpu):
    """a max_batch = 8 plan enqueued with 3 images: rows 3 .. 7 of a NaN-filled output keep NaN"""
    path, _ = yolov7_wts("yolov7tiny")
    S = 128
    mo = max_out_of("yolov7tiny", S)
    plan = engine.build_plan("yolov7tiny", path, batch=8, h=S, w=S, fp16=1, max_out=mo)
    assert kinds(plan).count("yolo7_head") == 1
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
