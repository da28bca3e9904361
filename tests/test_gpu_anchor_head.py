"""The anchor-based YoloLayer kernels on the GPU, both families: the planar decode (trtx_yolov5_decode, trtx_yolov7_decode) and the fused
head on NHWC (trtx_yolov{5,7}_head_decode_nhwc{,_f32}) through the C ABI against the oracle's C restatement of the reference's YOLOv5
plugin (oracle/csrc/yolov5_post_ref.c, pinned on the reference's own kernel in test_ref_pinning.py).  The families share their kernels
(plugins/anchor_decode.hip, anchor_head.hip) and differ in the record: 38 floats for YOLOv5, of which a detection head writes the
first six and leaves the 32 mask coefficients alone, and those six floats for YOLOv7, whose CalDetection is the same arithmetic.  So
every case runs for both, against the same oracle on the same inputs, compared on floats 0 .. 5 of each record.

The bound is tests/test_gpu_yolov5.py's: counts, class ids and slot order equal, floats within rtol = atol = 2e-6 (every value passes
through expf: device against glibc, 1 ulp).  The candidate counts asserted below are the oracle's, so they are the same for both
families."""
import collections
import functools

import numpy as np
import pytest
import torch

from oracle import yolo_post as yp
from tensorrtx_amd import capi, synth
from test_gpu_yolov5 import as_seen, to_nhwc
from test_yolov7_cpu import records6

pytestmark = pytest.mark.gpu
GRIDS = [(80, 80), (40, 40), (20, 20)]
SENTINEL = -12345.5

Family = collections.namedtuple("Family", "det head_decode decode head_workspace")
V5 = Family(capi.DET5_FLOATS, capi.yolov5_head_decode_nhwc, capi.yolov5_decode, capi.yolov5_head_decode_workspace)
V7 = Family(capi.DET7_FLOATS, capi.yolov7_head_decode_nhwc, capi.yolov7_decode, capi.yolov7_head_decode_workspace)
families = pytest.mark.parametrize("fam", [V5, V7], ids=["v5", "v7"])


def oracle(ins, classes, net_h, net_w, grids, anchors, max_out):
    """floats 0 .. 5 of the YOLOv5 oracle's 38-float records: [B, 1 + 6 * max_out]"""
    return records6(yp.v5_decode_c(ins, classes, net_h, net_w, grids, anchors, max_out), max_out)


def records(row, det=6):
    """floats 0 .. 5 of the records of a row whose records are `det` floats long"""
    n = int(row[0])
    return row[1:1 + n * det].reshape(n, det)[:, :6]


def compare(fam, got, ref):
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    for b in range(ref.shape[0]):
        g, r = records(got[b], fam.det), records(ref[b])
        assert np.array_equal(g[:, 5], r[:, 5]), "class ids / slot order"
        assert np.allclose(g[:, :5], r[:, :5], rtol=2e-6, atol=2e-6, equal_nan=True), np.nanmax(np.abs(g[:, :5] - r[:, :5]))


def framed(fam, batch, max_out, gpu):
    """an output buffer one row longer than the batch, filled with a sentinel"""
    return torch.full((batch + 1, 1 + max_out * fam.det), SENTINEL, dtype=torch.float32, device=gpu)


def check_frame(fam, out, batch):
    """every float behind a row's 1 + det * count, the extra row, and floats 6 .. det - 1 of every record (the mask coefficients, which a
    detection head does not write) still hold the sentinel"""
    out = out.cpu().numpy()
    assert (out[batch] == SENTINEL).all(), "the row behind the batch was written"
    for b in range(batch):
        n = int(out[b, 0])
        assert (out[b, 1 + n * fam.det:] == SENTINEL).all(), (b, n, np.flatnonzero(out[b, 1 + n * fam.det:] != SENTINEL)[:8])
        assert (out[b, 1:1 + n * fam.det].reshape(n, fam.det)[:, 6:] == SENTINEL).all(), (b, n, "floats behind float 5 of a record were written")
    return out[:batch]


def head(fam, planes, grids, classes, net_h, net_w, anchors, max_out, dtype, gpu, ld, pad=(float("nan"),), offset=0):
    """the fused head on NHWC tensors made of the planes, into a sentinel frame; offset: elements by which each base is shifted off its
    16-byte alignment"""
    hs = []
    for x, g in zip(planes, grids):
        t = to_nhwc(x, g, ld, dtype, pad).to(gpu)
        if offset:
            buf = torch.empty(t.numel() + offset, dtype=dtype, device=gpu)
            buf[offset:].copy_(t.flatten())
            t = buf[offset:].view(t.shape)
        hs.append(t)
    B = planes[0].shape[0]
    out = framed(fam, B, max_out, gpu)
    fam.head_decode(hs, classes, net_h, net_w, grids, anchors, max_out, out=out)
    return check_frame(fam, out, B)


def planar(fam, planes, grids, classes, net_h, net_w, anchors, max_out, gpu):
    B = planes[0].shape[0]
    out = framed(fam, B, max_out, gpu)
    fam.decode([torch.from_numpy(x).to(gpu) for x in planes], classes, net_h, net_w, grids, anchors, max_out, out=out)
    return check_frame(fam, out, B)


def both(fam, planes, grids, classes, net_h, net_w, anchors, max_out, dtype, gpu, ld, what, **kw):
    """head and planar kernel against the oracle, and against each other: conf and class bit-equal, the boxes reported"""
    ref = oracle(planes, classes, net_h, net_w, grids, anchors, max_out)
    got = head(fam, planes, grids, classes, net_h, net_w, anchors, max_out, dtype, gpu, ld, **kw)
    plug = planar(fam, planes, grids, classes, net_h, net_w, anchors, max_out, gpu)
    compare(fam, got, ref)
    compare(fam, plug, ref)
    d = 0.0
    for b in range(ref.shape[0]):
        g, p = records(got[b], fam.det), records(plug[b], fam.det)
        assert np.array_equal(g[:, 4:].view(np.int32), p[:, 4:].view(np.int32)), "conf / class of the head and of the planar kernel"
        if len(g):
            d = max(d, float(np.nanmax(np.abs(g - p))))
    print(f"{what}: candidates {ref[:, 0].astype(int).tolist()}; largest |fused head - planar kernel| {d:.3g} ({'bit-equal' if d == 0 else 'differs'})")
    return ref


def small_case(grids, classes, batch, seed, shift):
    """random planes whose objectness sits `shift` below zero"""
    rng = np.random.default_rng(seed)
    ins = [rng.normal(0, 2, size=(batch, 3 * (5 + classes), gw * gh)).astype(np.float32) for gw, gh in grids]
    for x in ins:
        x[:, 4::5 + classes] -= shift
    return ins


@families
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("ld,offset", [(32, 0), (27, 0), (32, 1)])
def test_ragged_levels_vector_and_element_paths(gpu, fam, dtype, ld, offset):
    """27 channels in pixels of 32 (16-byte loads; the padding holds NaN and a large finite value), of 27 (element loads), and of 32 on a
    base that is no multiple of 16 bytes (element loads)"""
    grids = [(7, 5), (3, 2)]
    anchors = [[4, 5, 8, 9, 12, 7], [20, 30, 25, 18, 40, 44]]
    ins = as_seen(small_case(grids, 4, 2, 4, 3.0), dtype)
    ref = both(fam, ins, grids, 4, 40, 56, anchors, 60, dtype, gpu, ld, f"ld {ld} offset {offset}", pad=(float("nan"), 60000.0), offset=offset)
    assert 3 < ref[:, 0].min() and ref[:, 0].max() < 60


@families
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_chunk_boundary_inside_a_level(gpu, fam, dtype):
    """525 cells: the 512-cell chunk ends inside the last level"""
    grids = [(20, 20), (10, 10), (5, 5)]
    ins = as_seen(small_case(grids, 80, 2, 6, 4.5), dtype)
    ref = both(fam, ins, grids, 80, 160, 160, synth.YOLOV7_ANCHORS, 400, dtype, gpu, 256, "525 cells")
    assert 3 < ref[:, 0].min() and ref[:, 0].max() < 400


@families
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("ld", [56, 54])
def test_four_levels_odd_strides(gpu, fam, dtype, ld):
    """13 classes: 54 channels in pixels of 56 and of 54 (fp16: 108-byte rows, element loads)"""
    grids = [(16, 16), (8, 8), (4, 4), (2, 2)]
    ins = as_seen(small_case(grids, 13, 2, 7, 4.0), dtype)
    ref = both(fam, ins, grids, 13, 128, 128, synth.YOLOV7_P6_ANCHORS, 300, dtype, gpu, ld, f"four levels ld {ld}")
    assert 3 < ref[:, 0].min() and ref[:, 0].max() < 300


@functools.lru_cache(maxsize=None)
def bulk(dtype):
    return as_seen(synth.yolov5_head_tensors(3, seed=2), dtype)


@families
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_bulk_640(gpu, fam, dtype):
    ins = bulk(dtype)
    ref = both(fam, ins, GRIDS, 80, 640, 640, synth.YOLOV7_ANCHORS, 1000, dtype, gpu, 256, "3 x 640^2")
    assert 3 < ref[:, 0].min() and ref[:, 0].max() < 1000


@families
def test_batch_invariance(gpu, fam):
    """image 0 of the batch decodes bit-equal when run alone"""
    ins = bulk(torch.float16)
    all3 = head(fam, ins, GRIDS, 80, 640, 640, synth.YOLOV7_ANCHORS, 1000, torch.float16, gpu, 256)
    alone = head(fam, [x[:1] for x in ins], GRIDS, 80, 640, 640, synth.YOLOV7_ANCHORS, 1000, torch.float16, gpu, 256)
    assert np.array_equal(all3[:1].view(np.int32), alone.view(np.int32))
    p3 = planar(fam, ins, GRIDS, 80, 640, 640, synth.YOLOV7_ANCHORS, 1000, gpu)
    p1 = planar(fam, [x[:1] for x in ins], GRIDS, 80, 640, 640, synth.YOLOV7_ANCHORS, 1000, gpu)
    assert np.array_equal(p3[:1].view(np.int32), p1.view(np.int32))


@families
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_empty_and_full_images(gpu, fam, dtype):
    """max_out = 40: an image without a candidate, and one where every anchor passes, whose records are the first 40 of the canonical
    (level, cell, anchor) order"""
    grids = [(7, 5), (3, 2)]
    anchors = [[4, 5, 8, 9, 12, 7], [20, 30, 25, 18, 40, 44]]
    ins = small_case(grids, 4, 3, 4, 5.0)
    for x in ins:
        x[1, 4::9] = -30.0   # image 1: nothing passes
        x[2, 4::9] = 8.0     # image 2: every anchor of every cell passes
    ins = as_seen(ins, dtype)
    ref = both(fam, ins, grids, 4, 40, 56, anchors, 40, dtype, gpu, 32, "empty / full")
    assert ref[1, 0] == 0 and ref[2, 0] == 40 and 3 < ref[0, 0] < 40   # (the overflow case: the full image reaches max_out on purpose)
    everything = oracle(ins, 4, 40, 56, grids, anchors, 200)
    assert everything[2, 0] == 3 * 41
    got = head(fam, ins, grids, 4, 40, 56, anchors, 40, dtype, gpu, 32)
    assert np.allclose(records(got[2], fam.det), records(everything[2])[:40], rtol=2e-6, atol=2e-6)


@families
def test_class_ties_take_the_lower_index(gpu, fam):
    """equal maximal logits in different lanes (classes 17 and 63), inside one lane's chunk (40 and 41), first and last class (0 and 79)"""
    grids = [(3, 2)]
    x = np.full((2, 255, 6), -5.0, np.float32)
    x[:, 4::85] = 3.0
    for k, (lo, hi) in enumerate([(17, 63), (40, 41), (0, 79)]):
        x[:, k * 85 + 5 + lo] = 2.0
        x[:, k * 85 + 5 + hi] = 2.0
    x[1, 5 + 63] = 2.5   # image 1, anchor 0: the higher index is the strict maximum
    for dtype in (torch.float16, torch.float32):
        both(fam, [x], grids, 80, 16, 24, synth.YOLOV7_ANCHORS[:1], 100, dtype, gpu, 256, "ties")
        got = head(fam, [x], grids, 80, 16, 24, synth.YOLOV7_ANCHORS[:1], 100, dtype, gpu, 256)
        rec = got[:, 1:1 + 18 * fam.det].reshape(2, 6, 3, fam.det)
        assert got[0, 0] == 18 and (rec[0, :, :, 5] == [17, 40, 0]).all() and (rec[1, :, :, 5] == [63, 40, 0]).all()


@families
def test_nan_logits_beside_a_passing_one(gpu, fam):
    grids = [(4, 4)]
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, size=(1, 255, 16)).astype(np.float32)
    x[:, 4::85] = -9.0
    x[0, 85 + 4, 5] = np.nan      # anchor 1 of cell 5: NaN objectness, kept as the reference keeps it
    x[0, 4, 11] = 4.0             # anchor 0 of cell 11 passes ...
    x[0, 5 + 30, 11] = np.nan     # ... with a NaN class logit beside its others
    x[0, 2 * 85 + 4, 11] = 4.0    # anchor 2 of the same cell passes
    x[0, 2 * 85 + 1, 11] = np.nan   # ... with a NaN box value
    for dtype in (torch.float16, torch.float32):
        seen = as_seen([x], dtype)
        ref = both(fam, seen, grids, 80, 32, 32, synth.YOLOV7_ANCHORS[:1], 100, dtype, gpu, 256, "NaN")
        assert ref[0, 0] == 3 and np.isnan(ref[0, 1 + 4])


@families
def test_refusals_leave_the_buffers_untouched(gpu, fam):
    grids = [(7, 5), (3, 2)]
    anchors = [[4, 5, 8, 9, 12, 7], [20, 30, 25, 18, 40, 44]]
    ins = small_case(grids, 4, 2, 4, 3.0)
    for dtype in (torch.float16, torch.float32):
        hs = [to_nhwc(x, g, 32, dtype).to(gpu) for x, g in zip(ins, grids)]
        need = fam.head_workspace(2, grids)
        for what, kw, status in (("ld", dict(ld=[32, 26]), 1), ("workspace", dict(short=True), 3), ("no levels", dict(n_levels=0), 1),
                                 ("nine levels", dict(n_levels=9), 1)):
            out = framed(fam, 2, 60, gpu)
            ws = torch.full((need - 256 if kw.pop("short", False) else need,), 0x5A, dtype=torch.uint8, device=gpu)
            st = fam.head_decode(hs, 4, 40, 56, grids, anchors, 60, out=out, ws=ws, status_only=True, **kw)
            torch.cuda.synchronize()
            assert st == status, (what, st)
            assert (out == SENTINEL).all() and (ws == 0x5A).all(), what
