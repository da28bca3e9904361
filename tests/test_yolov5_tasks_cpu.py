"""YOLOv5 seg / cls (host builders, synthetic weights, lowering) and the mask-assembly restatement: CPU-side checks."""
import collections
import hashlib
import os

import numpy as np
import pytest
import torch

import seg_mask_ref as smr
from oracle import graph_interp as gi
from oracle import wts as owts
from tensorrtx_amd import capi, engine, synth
from tensorrtx_amd import wts as wts_writer
from test_yolov5_cpu import convs_of, lowered, without_plugin, yolov5_wts
from util import CACHE
from yolov5_task_twin import Yolov5Task

TASKS = {"seg": (1, 80), "cls": (4, 1000)}   # task id, default classes
# sha256 over the concatenated tensors of synth.yolov5_state("n"), recorded before the `task` keyword existed
YOLOV5N_DET_STATE_SHA256 = "cbf3560ccedf8048be500aa8b43d83a324ad1b2e17af55e96b1915e4a75f3fcb"


def task_wts(scale, task, seed=0):
    tid, nc = TASKS[task]
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"yolov5{scale}_{task}_synth_s{seed}.wts")
    sd = synth.yolov5_state(scale, seed=seed, num_class=nc, task=tid)
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def state_hash(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, dtype=np.float32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("scale,B,S", [("n", 2, 128), ("m", 1, 64)])
def test_yolov5_seg_builder_matches_twin(scale, B, S):
    """The seg graph (implicit batch, marked heads, the plugin layer dropped as test_yolov5_cpu.without_plugin does, `proto` kept) through
    the oracle's interpreter against the twin; the interpreter has every layer kind these graphs use (Proto's resize by scales included)"""
    path, sd = task_wts(scale, "seg")
    plan = engine.build_plan("yolov5" + scale, path, batch=B, h=S, w=S, fp16=1, task=1, mark_heads=1)
    desc = engine.describe_plan(plan)
    assert not desc["explicit_batch"]
    x = torch.from_numpy(synth.images(B, S, S, seed=5))
    out = gi.run(without_plugin(desc), plan, {"data": x.numpy()}, batch=B)
    with torch.inference_mode():
        heads, strides, proto = Yolov5Task(sd, scale).seg_heads(x)
    assert strides == [8, 16, 32] and sorted(out) == ["head0", "head1", "head2", "proto"]
    for i, h in enumerate(heads):
        assert tuple(out[f"head{i}"].shape) == (B, 351, S // strides[i], S // strides[i]) and tuple(h.shape) == (B, 351, (S // strides[i]) ** 2)
        d = (out[f"head{i}"].reshape(h.shape) - h).abs().max().item()
        print(f"yolov5{scale}-seg head{i}: |diff| {d:.3g}, |head| {h.abs().max().item():.3g}")
        assert d < 2e-4
    assert tuple(out["proto"].shape) == tuple(proto.shape) == (B, 32, S // 4, S // 4)
    d = (out["proto"] - proto).abs().max().item()
    print(f"yolov5{scale}-seg proto: |diff| {d:.3g}, |proto| {proto.abs().max().item():.3g}")
    assert d < 2e-4


@pytest.mark.parametrize("scale,B,S", [("n", 2, 64), ("m", 1, 224)])
def test_yolov5_cls_builder_matches_twin(scale, B, S):
    """64^2 pools a 2 x 2 map, 224^2 the reference's 7 x 7"""
    path, sd = task_wts(scale, "cls")
    plan = engine.build_plan("yolov5" + scale, path, batch=B, h=S, w=S, fp16=1, task=4)
    desc = engine.describe_plan(plan)
    assert not desc["explicit_batch"]
    x = torch.from_numpy(synth.images(B, S, S, seed=6))
    out = gi.run(desc, plan, {"data": x.numpy()}, batch=B)
    assert set(out) == {"prob"}
    with torch.inference_mode():
        ref, _ = Yolov5Task(sd, scale, 1000).classify(x)
    got = out["prob"].reshape(B, -1)
    assert tuple(got.shape) == (B, 1000)
    d = (got - ref.float()).abs().max().item()
    print(f"yolov5{scale}-cls {S}: |diff| {d:.3g}, |logit| {ref.abs().max().item():.3g}")
    assert d < 2e-4


def test_yolov5_cls_pools_a_map_that_is_not_square():
    """h / 32 by w / 32: 64 x 96 pools 2 x 3 (the reference's DimsHW{k, k} is the square case)"""
    path, sd = task_wts("n", "cls")
    plan = engine.build_plan("yolov5n", path, batch=1, h=64, w=96, fp16=1, task=4)
    x = torch.from_numpy(synth.images(1, 64, 96, seed=6))
    out = gi.run(engine.describe_plan(plan), plan, {"data": x.numpy()}, batch=1)
    with torch.inference_mode():
        ref, _ = Yolov5Task(sd, "n", 1000).classify(x)
    assert (out["prob"].reshape(1, -1) - ref.float()).abs().max().item() < 2e-4


def test_seg_and_cls_lowering():
    """The seg tail keeps the plugin (match_yolo5_heads declines mask coefficients): one layout pass per detect level, the plugin, and the
    proto conversion; no detect convolution is padded"""
    for fp16 in (1, 0):
        path, _ = task_wts("n", "seg")
        low = engine.describe_plan(engine.build_plan("yolov5n", path, batch=32, h=640, w=640, fp16=fp16, task=1), lowered=True)
        kinds = collections.Counter(o["kind"] for o in low["ops"])
        print(f"yolov5n-seg fp16={fp16}: {dict(kinds)}")
        assert kinds["plugin"] == 1 and kinds["yolo5_head"] == 0 and kinds["to_linear"] == 4, kinds
        lin = [o["name"] for o in low["ops"] if o["kind"] == "to_linear"]
        assert lin[3] == "to_linear:proto" and len(set(lin)) == 4, lin
        assert not any(o.get("cout_real") for o in convs_of(low))
        assert sorted(o["cout"] for o in convs_of(low) if o["cout"] == 351) == [351] * 3
        if fp16:
            assert dict(kinds) == {"conv": 63, "resize": 3, "pool_chain": 1, "to_linear": 4, "plugin": 1}
        path, _ = task_wts("n", "cls")
        low = engine.describe_plan(engine.build_plan("yolov5n", path, batch=32, fp16=fp16, task=4), lowered=True)
        kinds = collections.Counter(o["kind"] for o in low["ops"])
        print(f"yolov5n-cls fp16={fp16}: {dict(kinds)}")
        assert kinds["plugin"] == 0 and kinds["yolo5_head"] == 0
        if fp16:
            assert dict(kinds) == {"conv": 33, "pool": 1, "to_linear": 1}


def test_yolov5n_det_plan_lowers_as_before():
    """DESIGN §5 "YOLOv5 detection", "The plan": 60 conv, 2 resize, 1 pool_chain, 1 yolo5_head"""
    _, low = lowered("n", batch=32, h=640, w=640, fp16=1)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert dict(kinds) == {"conv": 60, "resize": 2, "pool_chain": 1, "yolo5_head": 1}, kinds
    assert [o["kind"] for o in low["ops"]][-1] == "yolo5_head"


def test_task_errors_and_bindings():
    seg, _ = task_wts("n", "seg")
    cls, _ = task_wts("n", "cls")
    det6, _ = yolov5_wts("s6")
    for model, path, kw in (("yolov5n", seg, dict(task=2)), ("yolov5n", seg, dict(task=3)), ("yolov5n", seg, dict(task=-1)),
                            ("yolov5s6", det6, dict(task=1, h=128, w=128)), ("yolov5s6", det6, dict(task=4, h=128, w=128)),
                            ("yolov5n", cls, dict(task=4, h=100)), ("yolov5n", cls, dict(task=4, w=72))):
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan(model, path, batch=1, **kw)
        assert e.value.status == 1, (model, kw)   # TRTX_ERR_INVALID
    for path, task in ((seg, 1), (cls, 4)):
        with pytest.raises(capi.TrtxError) as e:
            engine.build_plan("yolov5n", path, batch=1, task=task, int8=1)
        assert e.value.status == 4                # TRTX_ERR_UNSUPPORTED
    io = lambda d: [(t["name"], t["dims"]) for t in d["tensors"] if t["is_input"] or t["is_output"]]  # noqa: E731
    desc = engine.describe_plan(engine.build_plan("yolov5n", seg, batch=4, h=96, w=160, max_out=300, task=1))
    assert io(desc) == [("data", [3, 96, 160]), ("prob", [1 + 300 * 38, 1, 1]), ("proto", [32, 24, 40])]
    assert desc["max_batch"] == 4
    desc = engine.describe_plan(engine.build_plan("yolov5n", cls, batch=2, task=4))
    assert io(desc) == [("data", [3, 224, 224]), ("prob", [1000, 1, 1])]


def test_det_state_is_what_it_was():
    a, b = synth.yolov5_state("n"), synth.yolov5_state("n", task=0)
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert state_hash(a) == YOLOV5N_DET_STATE_SHA256
    path, _ = yolov5_wts("n")   # the cached det .wts of the existing tests
    disk = owts.load_wts(path)
    assert list(disk) == list(a)
    h = lambda d: hashlib.sha256(b"".join(np.ascontiguousarray(d[k], np.float32).tobytes() for k in a)).hexdigest()  # noqa: E731
    assert h(disk) == h(a)
    # the task models share every tensor drawn before their own: seg the backbone and neck, cls the backbone to model.8
    s, c = synth.yolov5_state("n", task=1), synth.yolov5_state("n", task=4, num_class=1000)
    assert all(np.array_equal(s[k], a[k]) for k in a if not k.startswith("model.24.m."))
    assert s["model.24.m.0.weight"].shape == (351, 64, 1, 1) and list(s)[-18:][0] == "model.24.proto.cv1.conv.weight"
    assert all(np.array_equal(c[k], a[k]) for k in c if not k.startswith("model.9."))
    assert c["model.9.conv.conv.weight"].shape == (1280, 256, 1, 1) and c["model.9.linear.weight"].shape == (1000, 1280)


def literal_masks(dec, det_floats, box_format, keep_idx, keep_cnt, max_keep, proto, net_h, net_w):
    """process_mask as written, scalar by scalar in fp32 (the rect's int conversion through Python's round-half-away / int), with the
    stated departures: writes outside the matrix are dropped, a non-finite edge gives an empty rect"""
    f = np.float32
    B, _, mh, mw = proto.shape
    out = np.full((B, max_keep, mh, mw), np.nan, np.float32)
    for b in range(B):
        for d in range(min(int(keep_cnt[b]), max_keep)):
            rec = dec[b, 1 + keep_idx[b, d] * det_floats:][:det_floats]
            bb = [f(v) for v in rec[:4]]
            if box_format == 0:
                left, top = f(bb[0] - f(bb[2] / f(2))), f(bb[1] - f(bb[3] / f(2)))
                right, bottom = f(bb[0] + f(bb[2] / f(2))), f(bb[1] + f(bb[3] / f(2)))
            else:
                left, top, right, bottom = bb[0], bb[1], f(bb[0] + bb[2]), f(bb[1] + bb[3])
                left, top = max(left, f(0)), max(top, f(0))
                right, bottom = min(right, f(net_w)), min(bottom, f(net_h))
            left, top, right, bottom = (f(v / f(4)) for v in (left, top, right, bottom))
            out[b, d] = 0
            if not all(np.isfinite(v) for v in (left, top, right, bottom)):
                continue

            def cvt(v):   # round(): half away from zero; int(): truncation
                v = float(v)
                return int(np.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)) if box_format == 0 else int(v)
            rx, ry, rw, rh = cvt(left), cvt(top), cvt(f(right - left)), cvt(f(bottom - top))
            for x in range(rx, rx + rw):
                for y in range(ry, ry + rh):
                    if not (0 <= x < mw and 0 <= y < mh):
                        continue
                    e = f(0)
                    for j in range(32):
                        e = f(e + f(f(rec[6 + j]) * proto[b, j, y, x]))
                    out[b, d, y, x] = f(1) / f(f(1) + np.exp(-e, dtype=np.float32))
    return out


@pytest.mark.parametrize("box_format", [0, 1])
def test_mask_restatement_against_the_literal_loop(box_format):
    """tests/seg_mask_ref.py (vectorised, fp32 mode) against the scalar triple loop on a 6 x 5 plane (net 24 x 20): the same bits"""
    rng = np.random.default_rng(box_format)
    mh, mw, max_out, det_floats = 5, 6, 16, 38
    boxes = [(4, 4, 16, 12), (-6, -2, 10, 30), (10, 6, 14, 10), (2, 2, 12, 16), (10, 2, 40, 8), (30, 4, 50, 12), (6, 10, 7, 18), (0, 0, 24, 20),
             (-10, 6, 6, 14), (3, 3, 3.9, 9)]
    dec = rng.normal(0, 1, size=(2, 1 + max_out * det_floats)).astype(np.float32)
    keep_idx = np.full((2, max_out), -1, np.int32)
    for b in range(2):
        for i, (l, t, r, bt) in enumerate(boxes):
            slot = (7 * i + 3 + b) % max_out
            rec = dec[b, 1 + slot * det_floats:1 + (slot + 1) * det_floats]
            rec[:4] = ((l + r) / 2, (t + bt) / 2, r - l, bt - t) if box_format == 0 else (l, t, r - l, bt - t)
            keep_idx[b, i] = slot
    dec[1, 1 + keep_idx[1, 2] * det_floats + 2] = np.inf
    dec[1, 1 + keep_idx[1, 3] * det_floats + 6 + 4] = np.nan
    keep_cnt = np.array([len(boxes), 7], np.int32)
    proto = rng.normal(0, 1, size=(2, 32, mh, mw)).astype(np.float32)
    with np.errstate(all="ignore"):
        want = literal_masks(dec, det_floats, box_format, keep_idx, keep_cnt, 8, proto, 20, 24)
    got, inside, _ = smr.seg_masks(dec, det_floats, box_format, keep_idx, keep_cnt, 8, proto, 20, 24, dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    written = np.zeros((2, 8, 1, 1), bool)
    written[0], written[1, :7] = True, True
    assert np.array_equal(inside & written, (want != 0) & written)   # a written pixel is 0.0f exactly outside the rect
    assert inside[0, :8].any((1, 2)).sum() >= 6 and np.isnan(want[1, 7]).all() and np.isnan(want[1, 3]).any() and not np.isnan(want[1, 3]).all()
    assert smr.c_round(np.float32(2.5)) == 3 and smr.c_round(np.float32(-2.5)) == -3 and smr.c_round(np.float32(0.49999997)) == 0
