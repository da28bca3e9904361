"""YOLOv5 seg / cls engines on the GPU: fp32 against the PyTorch twin (tests/yolov5_task_twin.py), fp16 against the fp32 engine, and
engine -> trtx_yolov5_nms -> trtx_seg_masks end to end against tests/seg_mask_ref.py.

Candidates the synthetic seg models keep (synth.yolov5_state(task=1)), measured with the fp32 twin on the CPU at the tests' seeds and
sizes, per image, next to the anchor count 3 * cells:
  n, 2 x 128^2 (seed 5): 165, 167 of 1008      n, 4 x 160^2 (seed 12): 265, 242, 247, 265 of 1575
  s (weight seed 1), 2 x 128^2 (seed 12): 345, 344 of 1008, of which 324 and 326 lie more than 0.02 from the 0.1 gate
The detect rows of a seg model are other draws than the det model's, and yolov5s at weight seed 0 passes 1 and 0 anchors at 128^2
(seeds 2 - 8: 16 to 663 per image), so the s case takes weight seed 1.  MAX_OUT is above the anchor count in the fp16 tests: no image
can reach it.
End to end (n, 2 x 160^2 of seed 12, conf_thresh 0.4, nms_thresh 0.45): the twin's records through the oracle's NMS keep 5 and 9
detections (0.3: 18 and 20; 0.5: fewer than 3), inside [3, MAX_KEEP = 16]."""
import numpy as np
import pytest
import torch

import seg_mask_ref as smr
from oracle import yolo_post as yp
from tensorrtx_amd import capi, engine, synth
from test_gpu_yolov5 import compare, match_detections, run
from test_yolov5_cpu import convs_of
from test_yolov5_tasks_cpu import task_wts
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk
from yolov5_task_twin import Yolov5Task

pytestmark = pytest.mark.gpu
DET, INFO = yp.DET5_FLOATS, 5 + 80 + 32
MAX_KEEP = 16


def grids_of(S):
    return [(S // s, S // s) for s in (8, 16, 32)]


def max_out_of(S):
    return 3 * sum(gw * gh for gw, gh in grids_of(S)) + 100


def near_gate(heads, counts, margin=0.02):
    """test_gpu_yolov5.near_gate for 117-value anchors: per image, for the records an engine wrote from `heads` ([B, 351, cells] per
    level) in canonical (level, cell, anchor) order, is the objectness probability within `margin` of the 0.1 gate"""
    B = heads[0].shape[0]
    obj = np.concatenate([h.reshape(B, 3, INFO, -1)[:, :, 4].transpose(0, 2, 1).reshape(B, -1) for h in heads], 1).astype(np.float32)
    p = np.float32(1) / (np.float32(1) + np.exp(-obj))
    out = []
    for b in range(B):
        kept = ~(p[b] < np.float32(0.1))
        assert kept.sum() == counts[b], (b, kept.sum(), counts[b])
        out.append(np.abs(p[b][kept] - 0.1) < margin)
    return out


def full_records(row):
    n = int(row[0])
    return row[1:1 + n * DET].reshape(n, DET)


def test_yolov5n_seg_fp32_engine_matches_twin(gpu):
    path, sd = task_wts("n", "seg")
    B, S = 2, 128
    mo = max_out_of(S)
    plan = engine.build_plan("yolov5n", path, batch=B, h=S, w=S, fp16=0, task=1, mark_heads=1, max_out=mo)
    x = synth.images(B, S, S, seed=5)
    got = run(plan, x, gpu)
    tw = Yolov5Task(sd, "n")
    with torch.inference_mode():
        heads, strides, proto = tw.seg_heads(torch.from_numpy(x))
    mine = []
    for i, h in enumerate(heads):
        g = got[f"head{i}"].reshape(h.shape)
        err, lim = (g - h).abs().max().item(), 1e-4 * max(1.0, h.abs().max().item())
        print(f"head{i}: err {err:.3g}, bound {lim:.3g}, err / bound {err / lim:.3g}")
        assert err <= lim, i
        mine.append(g.numpy())
    err, lim = (got["proto"].reshape(proto.shape) - proto).abs().max().item(), 1e-4 * max(1.0, proto.abs().max().item())
    print(f"proto: err {err:.3g}, bound {lim:.3g}, err / bound {err / lim:.3g}")
    assert err <= lim
    ref = yp.v5_decode_c(mine, 80, S, S, grids_of(S), tw.anchors(), mo, is_seg=True)
    assert 0 < ref[:, 0].min() and ref[:, 0].max() < mo
    prob = got["prob"].reshape(B, -1).numpy()
    compare(prob, ref)   # counts, class ids and slot order equal; box and conf within 2e-6
    for b in range(B):
        assert np.array_equal(full_records(prob[b])[:, 6:].view(np.int32), full_records(ref[b])[:, 6:].view(np.int32)), "coefficients are copies"


@pytest.mark.parametrize("name,B,S,wseed", [("n", 4, 160, 0), ("s", 2, 128, 1)])
def test_yolov5_seg_fp16_engine_tracks_fp32_engine(name, B, S, wseed, gpu):
    """Heads and proto within fp16_walk(2 * convolutions, max |ref|); detections matched as test_gpu_yolov5.match_detections does
    (candidates within 0.02 of the 0.1 gate skipped, no image left out); the coefficients of matched pairs (same class, nearest centre,
    IoU above 0.9) within fp16_walk(sites, largest |head|).  Every image has candidates clear of the gate (module docstring)."""
    path, _ = task_wts(name, "seg", seed=wseed)
    x = synth.images(B, S, S, seed=12)
    mo = max_out_of(S)
    model = "yolov5" + name
    p16 = engine.build_plan(model, path, batch=B, h=S, w=S, fp16=1, task=1, mark_heads=1, max_out=mo)
    p32 = engine.build_plan(model, path, batch=B, h=S, w=S, fp16=0, task=1, mark_heads=1, max_out=mo)
    sites = 2 * len(convs_of(engine.describe_plan(p16, lowered=True)))
    g16, g32 = run(p16, x, gpu), run(p32, x, gpu)
    h32, hmax = [], 0.0
    for key in ("head0", "head1", "head2", "proto"):
        a, r = g16[key], g32[key]
        assert torch.isfinite(a).all()
        err, lim = (a - r).abs().max().item(), fp16_walk(sites, r.abs().max().item())
        print(f"{model}-seg B{B} {S}: {key} err {err:.3g}, bound {lim:.3g} ({sites} sites), err / bound {err / lim:.3g}")
        assert err <= lim, key
        if key != "proto":
            h32.append(r.reshape(B, 3 * INFO, -1).numpy())
            hmax = max(hmax, r.abs().max().item())
    dec, ref = g16["prob"].reshape(B, -1).numpy(), g32["prob"].reshape(B, -1).numpy()
    skip = near_gate(h32, ref[:, 0])
    st = match_detections(dec, ref, mo, gpu, skip=skip)
    print(st, "counts", ref[:, 0])
    assert all((~k).sum() >= 100 for k in skip), [int((~k).sum()) for k in skip]   # every image takes part
    assert st["ref"] > 200
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st
    lim, worst, pairs = fp16_walk(sites, hmax), 0.0, 0
    for b in range(B):
        G, R = full_records(dec[b]), full_records(ref[b])[~skip[b]]
        for r in R:
            same = np.nonzero(G[:, 5] == r[5])[0]
            if not len(same):
                continue
            g = G[same]
            d = np.abs(g[:, 0] - r[0]) + np.abs(g[:, 1] - r[1])
            j = int(np.argmin(d))
            ix = max(min(g[j, 0] + g[j, 2] / 2, r[0] + r[2] / 2) - max(g[j, 0] - g[j, 2] / 2, r[0] - r[2] / 2), 0)
            iy = max(min(g[j, 1] + g[j, 3] / 2, r[1] + r[3] / 2) - max(g[j, 1] - g[j, 3] / 2, r[1] - r[3] / 2), 0)
            if ix * iy / (g[j, 2] * g[j, 3] + r[2] * r[3] - ix * iy) > 0.9:
                pairs += 1
                worst = max(worst, float(np.abs(g[j, 6:] - r[6:]).max()))
    print(f"{model}-seg: {pairs} matched pairs, coefficient err {worst:.3g}, bound {lim:.3g}, err / bound {worst / lim:.3g}")
    assert worst <= lim
    assert pairs >= 0.95 * st["matched"] > 0   # the same rule as match_detections up to ties in the centre distance


@pytest.mark.parametrize("S", [64, 224])
def test_yolov5n_cls_engines(S, gpu):
    """fp32 logits within 1e-4 max(1, max |logit|) of the twin, fp16 within fp16_walk(2 * convolutions, max |logit|) of fp32 (the fully
    connected layer lowers to a convolution and is counted), and the top-1 index equal where the twin's top-two gap exceeds twice that
    bound.  Checked with the twin on the CPU: at seed 9 the gaps are 0.086 and 0.093 (64^2), 0.107 and 0.113 (224^2) against a bound of
    0.0036 - every image of both cases qualifies (the test asserts at least one)."""
    B = 2
    path, sd = task_wts("n", "cls")
    x = synth.images(B, S, S, seed=9)
    with torch.inference_mode():
        ref, _ = Yolov5Task(sd, "n", 1000).classify(torch.from_numpy(x))
    p32 = engine.build_plan("yolov5n", path, batch=B, h=S, w=S, fp16=0, task=4)
    p16 = engine.build_plan("yolov5n", path, batch=B, h=S, w=S, fp16=1, task=4)
    g32 = run(p32, x, gpu)["prob"].reshape(B, 1000).double()
    g16 = run(p16, x, gpu)["prob"].reshape(B, 1000).double()
    mag = max(1.0, ref.abs().max().item())
    err = (g32 - ref).abs().max().item()
    print(f"cls {S}: fp32 err {err:.3g}, bound {1e-4 * mag:.3g}, err / bound {err / (1e-4 * mag):.3g}")
    assert err <= 1e-4 * mag
    sites = 2 * len(convs_of(engine.describe_plan(p16, lowered=True)))
    lim = fp16_walk(sites, g32.abs().max().item())
    err = (g16 - g32).abs().max().item()
    print(f"cls {S}: fp16 err {err:.3g}, bound {lim:.3g} ({sites} sites), err / bound {err / lim:.3g}")
    assert torch.isfinite(g16).all() and err <= lim
    top = ref.topk(2, 1).values
    clear = (top[:, 0] - top[:, 1]) > 2 * lim
    assert clear.any(), (top, lim)
    assert torch.equal(g16.argmax(1)[clear], ref.argmax(1)[clear]) and torch.equal(g32.argmax(1)[clear], ref.argmax(1)[clear])


def test_seg_engine_nms_masks_end_to_end(gpu):
    """yolov5n-seg fp16, a batch = 4 plan enqueued with 2 images of 160^2: engine, capi.yolov5_nms, capi.seg_masks, all on device buffers.
    The reference is the restatement fed with the prob, keep lists and proto read back from the GPU: the zero pattern exactly, the values
    within seg_mask_ref.bound.  conf_thresh 0.4: the fp32 twin's records through the oracle's NMS keep 5 and 9 detections per image
    (module docstring); the fp16 engine's counts must lie in [3, MAX_KEEP] as well.  Rows of the two unused batch slots stay untouched."""
    path, _ = task_wts("n", "seg")
    S, PB, B, mo = 160, 4, 2, 1000
    plan = engine.build_plan("yolov5n", path, batch=PB, h=S, w=S, fp16=1, task=1, max_out=mo)
    e = engine.Engine(plan)
    assert e.names == ["data", "prob", "proto"] and e.max_batch == PB
    x = synth.images(B, S, S, seed=12)
    bufs = [torch.from_numpy(x).to(gpu)]
    for i in range(1, e.nb_bindings):
        bufs.append(torch.full((PB * int(np.prod(e.dims[i])),), float("nan"), dtype=torch.float32, device=gpu))
    e.enqueue(B, bufs)
    prob = bufs[1].reshape(PB, -1)
    proto = bufs[2].reshape(PB, 32, S // 4, S // 4)
    keep_idx, keep_cnt, _ = capi.yolov5_nms(prob[:B].contiguous(), mo, conf_thresh=0.4, nms_thresh=0.45)
    masks = torch.full((PB, MAX_KEEP, S // 4, S // 4), float("nan"), dtype=torch.float32, device=gpu)
    capi.seg_masks(prob[:B].contiguous(), keep_idx, keep_cnt, proto[:B].contiguous(), S, S, MAX_KEEP, box_format=0, out=masks[:B])
    torch.cuda.synchronize()
    e.close()
    prob_h, proto_h, masks_h = prob.cpu().numpy(), proto.cpu().numpy(), masks.cpu().numpy()
    ki, kc = keep_idx.cpu().numpy(), keep_cnt.cpu().numpy()
    assert np.isnan(prob_h[B:]).all() and np.isnan(proto_h[B:]).all() and np.isnan(masks_h[B:]).all(), "unused batch slots"
    assert np.isfinite(proto_h[:B]).all() and (prob_h[:B, 0] > 0).all() and (prob_h[:B, 0] < mo).all()
    print("candidates", prob_h[:B, 0], "kept", kc)
    assert (kc >= 3).all() and (kc <= MAX_KEEP).all(), kc
    rki, rkc, _ = yp.v5_batch_nms_c(prob_h[:B], mo, 0.4, 0.45)
    assert np.array_equal(kc, rkc) and all(np.array_equal(ki[b, :kc[b]], rki[b, :kc[b]]) for b in range(B))
    want, inside, mag = smr.seg_masks(prob_h[:B], DET, 0, ki, kc, MAX_KEEP, proto_h[:B], S, S)
    got = masks_h[:B]
    written = ~np.isnan(want[:, :, 0, 0])
    assert np.array_equal(written, np.arange(MAX_KEEP)[None] < kc[:, None])
    assert np.isnan(got[~written]).all()
    assert np.array_equal(got[written] != 0, inside[written]) and inside.any()
    err, lim = np.abs(got.astype(np.float64) - want)[inside], smr.bound(mag)[inside]
    print(f"end to end: rect pixels {int(inside.sum())}, mask values {got[inside].min():.3g} .. {got[inside].max():.3g}, "
          f"max err {err.max():.3g}, max err / bound {(err / lim).max():.3g}")
    assert (err <= lim).all()
