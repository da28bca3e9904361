"""Darknet YOLO (YOLOv3, YOLOv3-tiny, YOLOv4) on the GPU.

Kernels: every case of tests/darknet_cases.py through trtx_darknet_decode (fp32 planes) and trtx_darknet_head_decode_nhwc{,_f32} (the detect
convolutions' NHWC layout, every pixel stride of the case's class count, padding channels holding NaN) against the NumPy restatement of the
reference's CalDetection.  Outputs are pre-filled with a sentinel and carry one row more than the batch.  Exact: counts, class ids, slot
order, every float behind a row's records and the extra row.  Floats: rtol = atol = 2e-6, tests/test_gpu_yolov5.py's bound (every value
passes one exp: device against the host's, 1 ulp).  The fused head and the planar decode agree bit for bit on the same fp32 values (a NaN
record value, which only a NaN logit makes, is a NaN in both; the sign bit of a NaN is not compared).

NMS: trtx_darknet_nms on 7-float records against the oracle's C restatement of the reference's YOLOv5 nms on the same boxes widened to 38
floats, bit for bit (the two iou bodies, yolov4/yolov4.cpp:81-94 and yolov5/src/postprocess.cpp:30-42, are the same arithmetic).

Pad: IPaddingLayer through tests/test_gpu_layers.py's checker, fp32 and fp16, into a tensor of its own and into a concat slice, on all-negative
maps so that a pool which skipped its border instead of reading the zeros would show; the padded tensor and the 2x2 stride-1 pool behind it,
both bit exact.

Engines: fp32 heads against the fp64 twin (tests/darknet_twin.py) and "prob" against the restatement's decode of the engine's own heads;
fp16 against the fp32 engine; the fused head against the plugin route; a partial batch.

Candidates the synthetic models keep (synth.darknet_state, seed 0, 80 classes), measured with the fp64 twin on the CPU at the engine tests'
image seeds and sizes, per image, next to the anchor count 3 * cells:
  yolov3,      1 x 64 x 64 (seed 5): 62 of 252             yolov4,      1 x 64 x 64 (seed 5): 61 of 252
  yolov3-tiny, 2 x 64 x 64 (seed 5): 12, 16 of 60          yolov3-tiny, 1 x 96 x 64 (seed 5): 34 of 90
  yolov3-tiny, 4 x 64 x 64 (seed 12): 14, 17, 19, 10 of 60  yolov4,      1 x 64 x 64 (seed 12): 66 of 252
  yolov3-tiny, 8 x 64 x 64 (seed 12): 17, 20, 13, 16, 19, 22, 19, 10 of 60
Every class maximum passes its gate in these models (the favoured class sits at 0.62); the objectness gate is what drops anchors.  The
plugin's 1000 records are out of reach of 252 anchors."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import darknet_cases as dc
import test_gpu_layers as tgl
from darknet_twin import Darknet
from oracle import yolo_post as yp
from tensorrtx_amd import capi, engine, synth
from test_darknet_cpu import convs_of, darknet_wts
from test_gpu_yolov5 import kinds, run
from tests import layer_cases as lc
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk

pytestmark = pytest.mark.gpu
DET = dc.DET
SENTINEL = -12345.5
MAX_OUT = 1000


# ---- the decode and head kernels -------------------------------------------------------------------------------------------------------

def framed(batch, max_out, gpu):
    """an output buffer one row longer than the batch, filled with a sentinel"""
    return torch.full((batch + 1, 1 + max_out * DET), SENTINEL, dtype=torch.float32, device=gpu)


def compare(got, ref, what):
    """got: [B + 1, ...] as the kernel left its frame; ref: the restatement's [B, ...] on the same sentinel"""
    B = ref.shape[0]
    assert (got[B] == SENTINEL).all(), f"{what}: the row behind the batch was written"
    assert np.array_equal(got[:B, 0], ref[:, 0]), (what, got[:B, 0], ref[:, 0])
    worst = 0.0
    for b in range(B):
        n = int(ref[b, 0])
        assert (got[b, 1 + n * DET:] == SENTINEL).all(), f"{what}: image {b}: written behind its {n} records"
        g, r = dc.records(got[b]), dc.records(ref[b])
        assert np.array_equal(g[:, 5], r[:, 5]), f"{what}: image {b}: class ids / slot order"
        fl = [0, 1, 2, 3, 4, 6]
        with np.errstate(invalid="ignore"):
            d = np.abs(g[:, fl] - r[:, fl])
        if d.size and np.isfinite(d).any():
            worst = max(worst, float(np.nanmax(np.where(np.isfinite(d), d / (2e-6 + 2e-6 * np.abs(r[:, fl])), 0.0))))
        assert np.allclose(g[:, fl], r[:, fl], rtol=2e-6, atol=2e-6, equal_nan=True), (what, b, np.nanmax(np.where(np.isfinite(d), d, 0)))
    return worst


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c.name)
def test_decode_and_head_kernels(gpu, case):
    net = case.net
    ref = dc.reference(case.name, SENTINEL)
    out = framed(case.batch, case.max_out, gpu)
    capi.darknet_decode([torch.from_numpy(x).to(gpu) for x in case.planes], case.classes, net.net_h, net.net_w, net.grids, net.anchors, case.max_out, out=out)
    plug = out.cpu().numpy()
    worst = compare(plug, ref, "planar decode")
    print(f"{case.name}: counts {ref[:, 0].astype(int).tolist()}; planar decode worst err / bound {worst:.3f}")
    ran = set()
    for ld, path in dc.lds_of(case.classes):
        for dtype in (torch.float16, torch.float32):
            heads = [torch.from_numpy(dc.to_nhwc(x, g, ld)).to(dtype).to(gpu) for x, g in zip(case.planes, net.grids)]
            assert all(h.data_ptr() % 16 == 0 for h in heads)
            out = framed(case.batch, case.max_out, gpu)
            capi.darknet_head_decode_nhwc(heads, case.classes, net.net_h, net.net_w, net.grids, net.anchors, case.max_out, out=out)
            got = out.cpu().numpy()
            what = f"head ld {ld} ({path} loads) {str(dtype)[6:]}"
            worst = compare(got, ref, what)
            # every float that is a number has the planar decode's bits; a NaN (from a NaN logit) must be a NaN in both - its sign bit is no value, and the
            # fp16 kernel's negation of a NaN leaves another one than the fp32 kernel's (0xffc00000 / 0x7fc00000 on an MI355X)
            at = np.argwhere((got.view(np.int32) != plug.view(np.int32)) & ~(np.isnan(got) & np.isnan(plug)))
            assert not len(at), (f"{what}: not bit-equal to the planar decode at (row, float)", at[:8].tolist(), [(float(got[i, j]), float(plug[i, j]), hex(int(got.view(np.uint32)[i, j])),
                                                                                                        hex(int(plug.view(np.uint32)[i, j]))) for i, j in at[:8]])
            ran.add(path)
    assert ran == {"vector", "element"}


def test_head_refusals_leave_the_buffers_untouched(gpu):
    case = {c.name: c for c in dc.cases()}["random-A-3-b1"]
    net = case.net
    for dtype in (torch.float16, torch.float32):
        hs = [torch.from_numpy(dc.to_nhwc(x, g, 32)).to(dtype).to(gpu) for x, g in zip(case.planes, net.grids)]
        need = capi.darknet_head_decode_workspace(1, net.grids)
        for what, kw, status in (("ld", dict(ld=[32, 32, 23]), 1), ("workspace", dict(short=True), 3), ("no levels", dict(n_levels=0), 1), ("nine levels", dict(n_levels=9), 1)):
            out = framed(1, 60, gpu)
            ws = torch.full((need - 256 if kw.pop("short", False) else need,), 0x5A, dtype=torch.uint8, device=gpu)
            st = capi.darknet_head_decode_nhwc(hs, 3, net.net_h, net.net_w, net.grids, net.anchors, 60, out=out, ws=ws, status_only=True, **kw)
            torch.cuda.synchronize()
            assert st == status, (what, st)
            assert (out == SENTINEL).all() and (ws == 0x5A).all(), what


# ---- NMS -------------------------------------------------------------------------------------------------------------------------------

def clustered(batch, max_out, seed, fill=None):
    """7-float records in clusters of overlapping boxes: [B, 1 + max_out * 7]; float 6 (class_confidence) plays no part in the nms"""
    rng = np.random.default_rng(seed)
    out = np.zeros((batch, 1 + max_out * DET), np.float32)
    for b in range(batch):
        n = max_out if fill == "full" else (0 if fill == "empty" and b == 0 else int(rng.integers(max_out // 3, max_out - 3)))
        c = rng.uniform(50, 558, size=(max(n // 6, 1), 2))
        rec = np.zeros((n, DET), np.float32)
        k = rng.integers(0, len(c), size=n)
        rec[:, :2] = c[k] + rng.normal(0, 6, size=(n, 2))
        rec[:, 2:4] = rng.uniform(30, 90, size=(n, 2))
        rec[:, 4] = rng.uniform(0.05, 1.0, size=n)
        rec[:, 5] = rng.integers(0, 4, size=n)
        rec[:, 6] = rng.uniform(0.1, 1.0, size=n)
        if n > 8:
            rec[3, 4] = rec[7, 4] = np.float32(0.5)   # exactly at the threshold: dropped
        out[b, 0] = n
        out[b, 1:1 + n * DET] = rec.flatten()
    return out


def widen(dec7, max_out):
    """the same boxes as YOLOv5's 38-float records: bbox, conf = det_confidence, class_id"""
    B = dec7.shape[0]
    out = np.zeros((B, 1 + max_out * 38), np.float32)
    out[:, 0] = dec7[:, 0]
    out[:, 1:].reshape(B, max_out, 38)[:, :, :6] = dec7[:, 1:].reshape(B, max_out, DET)[:, :, :6]
    return out


@pytest.mark.parametrize("fill", [None, "empty", "full"])
def test_nms_matches_the_oracle(gpu, fill):
    mo = 300
    dec = clustered(3, mo, 21, fill)
    ki, kc, kd = yp.v5_batch_nms_c(widen(dec, mo), mo, 0.5, 0.4)   # the reference's BBOX_CONF_THRESH / NMS_THRESH of yolov3 and yolov4
    gi_, gc, gd = capi.darknet_nms(torch.from_numpy(dec).to(gpu), mo, 0.5, 0.4)
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
        assert (dc.records(dec[b])[gi_[b, :n]][:, 4] > 0.5).all()   # the two records at exactly 0.5 are gone


# ---- IPaddingLayer ---------------------------------------------------------------------------------------------------------------------

def pad_case(C, H, W, B, pre, post, wrap, max_batch=None):
    """Pad -> max-pool 2x2 stride 1 on an all-negative map (lc.GEN["neg"]): both the padded tensor and the pooled one are outputs.
    wrap "plain": the pad writes a tensor of its own; "concat": it writes channels [12, 12 + C) of a concat buffer next to a convolution"""
    Hp, Wp = H + pre[0] + post[0], W + pre[1] + post[1]
    padded = lambda x: F.pad(x, (pre[1], post[1], pre[0], post[0]), value=0.0)  # noqa: E731
    if wrap == "plain":
        def build(net, t):
            y = net.out(net.padding(t["x"], pre, post))
            return {"padded": y, "pooled": net.out(net.pooling(y, 2, 1))}

        def ref(x):
            return {"padded": lc.Out(padded(x["x"])), "pooled": lc.Out(F.max_pool2d(padded(x["x"]), 2, 1))}
        inputs = {"x": ((C, H, W), "neg")}
        want = {"pad_nhwc", "pool"}
    else:
        def build(net, t):
            a = lc.select_conv(net, lc.nhwc(net, t["z"]), 8, lc.NEIGHBOUR)
            y = net.out(net.padding(t["x"], pre, post))
            return {"cat": net.out(net.concat([a, y])), "pooled": net.out(net.pooling(y, 2, 1))}

        def ref(x):
            return {"cat": [lc.Out(x["z"][:, lc.NEIGHBOUR], ch=slice(0, 12)), lc.Out(padded(x["x"]), ch=slice(12, None))],
                    "pooled": lc.Out(F.max_pool2d(padded(x["x"]), 2, 1))}
        inputs = {"x": ((C, H, W), "neg"), "z": ((8, Hp, Wp), "n")}
        want = {"pad_nhwc", "pool", "conv"}
    name = f"pad_{pre[0]}{pre[1]}_{post[0]}{post[1]}_c{C}_{H}x{W}_b{B}_{wrap}"
    return lc.Case(name=name, family="pad", inputs=inputs, build=build, ref=ref, kinds=want, batch=B, max_batch=max_batch)


PADS = [pad_case(8, 2, 2, 2, (0, 0), (1, 1), "plain"),            # yolov3-tiny's, on a 2 x 2 map: 16-byte pieces in fp32 and fp16
        pad_case(5, 3, 7, 3, (0, 0), (1, 1), "plain"),            # element path
        pad_case(16, 5, 4, 1, (2, 1), (0, 3), "plain", max_batch=3),   # padding in front too; a partial batch
        pad_case(8, 3, 5, 2, (0, 0), (1, 1), "concat"),           # channel offset 12: aligned in fp32 only
        pad_case(12, 3, 5, 2, (1, 2), (1, 0), "concat")]


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", PADS, ids=[c.name for c in PADS])
def test_pad_layer_is_exact_and_its_zeros_are_real(case, fp16, gpu):
    x = lc.ref_inputs(case, lc.gen_inputs(case), fp16)
    outs = lc.outs_of(case, x, fp16)
    assert (x["x"] < 0).all() and (outs["pooled"][0].ref.max() == 0), "the border maxima are the pad's zeros: a pool that skipped them would stay negative"
    assert all(o.mag is None for v in outs.values() for o in v), "data movement: compared bit for bit"
    tgl.test_layer_matches_fp64_reference(case, fp16, gpu)


# ---- engines ---------------------------------------------------------------------------------------------------------------------------

def net_of(name, H, W):
    return dc.Net(name, [(W // s, H // s) for s in synth.DARKNET_STRIDES[name]], W, H, synth.DARKNET_ANCHORS[name])


def match_detections(dec, dec_ref, gpu, skip=None):
    """tests/test_gpu_yolov7.py's matching on 7-float centre-format records (cx, cy, w, h, det_confidence, class, class_confidence): per reference
    candidate the candidate of the same class with the nearest centre, matched when their IoU is above 0.9.  No image is left out (every count is
    below the plugin's 1000).  skip: per image a bool per reference record, or None."""
    st = dict(ref=0, matched=0, min_iou=1.0, unmatched_by_class={})
    for b in range(dec_ref.shape[0]):
        assert dec_ref[b, 0] < MAX_OUT and dec[b, 0] < MAX_OUT, (b, dec_ref[b, 0], dec[b, 0])
        R, G = torch.from_numpy(dc.records(dec_ref[b]).copy()).to(gpu), torch.from_numpy(dc.records(dec[b]).copy()).to(gpu)
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


def near_a_gate(dec_ref, margin=0.02):
    """per image, per reference record: is its objectness or its class maximum within `margin` of the 0.1 gate"""
    return [(np.abs(dc.records(row)[:, 4] - 0.1) < margin) | (np.abs(dc.records(row)[:, 6] - 0.1) < margin) for row in dec_ref]


@pytest.mark.parametrize("name,B,H,W", [("yolov3", 1, 64, 64), ("yolov3-tiny", 2, 64, 64), ("yolov3-tiny", 1, 96, 64), ("yolov4", 1, 64, 64)])
def test_fp32_engine_matches_twin(gpu, name, B, H, W):
    """heads within 1e-4 * max(1, |head|) of the fp64 twin; "prob" is the restatement's decode of the engine's own heads"""
    path, sd = darknet_wts(name)
    plan = engine.build_plan(name, path, batch=B, h=H, w=W, fp16=0, mark_heads=1)
    k = kinds(plan)
    assert k.count("plugin") == 1 and k.count("pad_nhwc") == (1 if name == "yolov3-tiny" else 0)
    x = synth.images(B, H, W, seed=5)
    got = run(plan, x, gpu)
    tw = Darknet(sd, name)
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
    anchors = 3 * sum((H // s) * (W // s) for s in strides)
    print(f"{name}: candidates {prob[:, 0].astype(int).tolist()} of {anchors} anchors")
    assert 0 < prob[:, 0].min() and prob[:, 0].max() < min(MAX_OUT, anchors)
    ref = dc.decode_ref(mine, 80, net_of(name, H, W), MAX_OUT, fill=float("nan"))
    frame = np.concatenate([np.where(np.isnan(prob), SENTINEL, prob), np.full((1, prob.shape[1]), SENTINEL, np.float32)])
    compare(frame, np.where(np.isnan(ref), np.float32(SENTINEL), ref), f"{name} prob")   # (the bindings were NaN-filled: NaN behind the records = untouched)
    # the same fp32 engine without marked heads runs the fused head (trtx_darknet_head_decode_nhwc_f32 behind the padded 256-channel detect
    # convolutions): another plan with its own tactics, so matched against the plugin route's records, not bit-compared - nothing skipped
    fused = engine.build_plan(name, path, batch=B, h=H, w=W, fp16=0)
    k = kinds(fused)
    assert k.count("darknet_head") == 1 and "plugin" not in k and "to_linear" not in k
    fprob = run(fused, x, gpu)["prob"].reshape(B, -1).numpy()
    st = match_detections(fprob, prob, gpu)
    print(f"{name} fp32 fused head: counts {fprob[:, 0].astype(int).tolist()}", st)
    assert np.array_equal(fprob[:, 0], prob[:, 0]) and st["matched"] == st["ref"] > 0 and st["min_iou"] >= 0.999, st
    for b in range(B):
        n = int(fprob[b, 0])
        assert np.isnan(fprob[b, 1 + n * DET:]).all(), "written behind the records"


@pytest.mark.parametrize("name,B", [("yolov3-tiny", 4), ("yolov4", 1)])
def test_fp16_engine_tracks_fp32_engine(name, B, gpu):
    """fp16 storage, fp32 accumulation, against the fp32 engine: head values within fp16_walk(sites, max |head|) with two sites per convolution
    (packed weights, stored output); detections of the fused head (no marked heads) matched as parity.py asks, candidates whose objectness or
    class maximum is within 0.02 of a gate skipped, no image left out"""
    path, _ = darknet_wts(name)
    S = 64
    x = synth.images(B, S, S, seed=12)
    p16 = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1)
    p16h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    p32h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=0, mark_heads=1)
    k = kinds(p16)
    assert k.count("darknet_head") == 1 and "plugin" not in k and "to_linear" not in k
    sites = 2 * len(convs_of(engine.describe_plan(p16, lowered=True)))
    g16, g16h, g32 = run(p16, x, gpu), run(p16h, x, gpu), run(p32h, x, gpu)
    for i in range(len(synth.DARKNET_STRIDES[name])):
        a, r = g16h[f"head{i}"], g32[f"head{i}"]
        assert torch.isfinite(a).all()
        err, lim = (a - r).abs().max().item(), fp16_walk(sites, r.abs().max().item())
        print(f"{name} B{B} {S}: head{i} err {err:.3g}, bound {lim:.3g} ({sites} sites)")
        assert err <= lim, i
    ref = g32["prob"].reshape(B, -1).numpy()
    skip = near_a_gate(ref)
    st = match_detections(g16["prob"].reshape(B, -1).numpy(), ref, gpu, skip=skip)
    print(st, "counts", ref[:, 0].astype(int).tolist(), "skipped near a gate", [int(s.sum()) for s in skip])
    assert (ref[:, 0] > 0).all() and st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_agrees_with_the_plugin_route(gpu, monkeypatch):
    """The fused fp16 plan against the plan the same build makes with TRTX_DARKNET_HEAD=0 (layout passes + the 7-float plugin, 255-channel stores).
    Two plans, each with its own tactics: matched as above, not bit-compared - and with no candidate skipped."""
    path, _ = darknet_wts("yolov3-tiny")
    B, S = 4, 64
    x = synth.images(B, S, S, seed=12)
    fused = engine.build_plan("yolov3-tiny", path, batch=B, h=S, w=S, fp16=1)
    assert kinds(fused).count("darknet_head") == 1
    a = run(fused, x, gpu)["prob"].reshape(B, -1).numpy()
    monkeypatch.setenv("TRTX_DARKNET_HEAD", "0")
    route = engine.build_plan("yolov3-tiny", path, batch=B, h=S, w=S, fp16=1)
    k = kinds(route)
    assert k.count("plugin") == 1 and k.count("darknet_head") == 0 and k.count("to_linear") == 2
    r = run(route, x, gpu)["prob"].reshape(B, -1).numpy()
    st = match_detections(a, r, gpu)
    print(st, "counts fused", a[:, 0], "plugin route", r[:, 0])
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_below_its_maximum_batch(gpu):
    """a max_batch = 8 plan enqueued with 3 images: rows 3 .. 7 of a NaN-filled output keep NaN"""
    path, _ = darknet_wts("yolov3-tiny")
    S = 64
    plan = engine.build_plan("yolov3-tiny", path, batch=8, h=S, w=S, fp16=1)
    assert kinds(plan).count("darknet_head") == 1
    x = synth.images(8, S, S, seed=12)
    full = run(plan, x, gpu)["prob"].reshape(8, -1).numpy()
    part = run(plan, x, gpu, batch=3)["prob"].reshape(8, -1).numpy()
    assert np.isnan(part[3:]).all()
    assert (part[:3, 0] > 0).all() and (part[:3, 0] < 60).all()
    for b in range(3):
        assert np.isfinite(dc.records(part[b])).all()
    st = match_detections(part[:3], full[:3], gpu)
    print(st, "counts", part[:3, 0], full[:, 0])
    assert st["ref"] > 0 and st["matched"] / st["ref"] >= 1 - FP16_MATCH and st["min_iou"] >= 1 - FP16_IOU, st
