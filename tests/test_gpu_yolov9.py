"""YOLOv9 / GELAN on the GPU: the fused DDetect head (trtx_yolov9_head_decode_nhwc{,_f32}) and the planar YOLOv9 plugin kernel
(trtx_yolov9_decode) through the C ABI against the oracle's C restatement of CalDetection (oracle/csrc/yolo_post_ref.c: the YOLOv8
plugin's detection branch is the same text as yolov9/plugin/yololayer.cu:133-176; the first six floats of a record), trtx_yolov9_nms
against the YOLOv5 oracle on the fp32-converted records, and YOLOv9 engines against the PyTorch twin (fp32), against the fp32 engine
(fp16) and against the plugin route of the same build.

Bounds of the head tests are tests/test_gpu_yolo11_tasks.py's: counts, class ids and slot order equal; conf atol 2e-7 (one expf: device
against glibc); boxes rtol 1e-5, atol 1e-4 (the kernel's fp32 DFL against the float64 one of the test).

Candidates the synthetic models keep (synth.yolov9_state, class bias -9.5, gelanc -11.5), measured with the fp64 twin (tests/yolov9_twin.py) on the
CPU on synth.images(B, S, S, seed=5), per image, next to the cell count:
  yolov9t, 2 x 128^2: 81, 94 of 336        yolov9t converted, 2 x 128^2: 14, 28 of 336     yolov9t, 1 x 320^2: 711 of 2100
  yolov9s, 1 x 64^2: 26 of 84              yolov9m, 1 x 64^2: 30 of 84                      yolov9m converted, 1 x 64^2: 7 of 84
  yolov9c, 1 x 64^2: 28 of 84              yolov9c, 1 x 128^2: 173 of 336                   gelanc, 1 x 64^2: 13 of 84
  gelanc, 2 x 128^2 (seed 12): 29, 27 of 336     gelanc, 1 x 320^2: 76 of 2100
MAX_OUT is above the cell count in every engine test: no image can reach it."""
import functools

import numpy as np
import pytest
import torch

from oracle import yolo_post as yp
from tensorrtx_amd import capi, engine, synth
from test_yolov9_cpu import STRIDES, cells_of, convs_of, corner_to_centre_f32, yolov9_wts
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk
from util import time_limit
from yolov9_twin import Yolov9

pytestmark = pytest.mark.gpu
DET = 38
SENTINEL = -1234.0
MEAN = {80: -7.2, 13: -6.2, 3: -5.3}   # of the class logits (std 1.5): a few per cent of the cells pass the 0.1 gate


def r8(n):
    return -(-n // 8) * 8


@functools.lru_cache(maxsize=None)
def planes(B, H, W, classes, dtype, seed=0):
    """Seeded box bins [B, 64, cells] and class logits [B, classes, cells] per level, rounded to `dtype` (the values the tensors hold)"""
    rng = np.random.default_rng(seed + 17 * classes + H)
    out = []
    for s in STRIDES:
        n = (H // s) * (W // s)
        box = rng.normal(0, 1.5, size=(B, 64, n)).astype(np.float32)
        cls = rng.normal(MEAN[classes], 1.5, size=(B, classes, n)).astype(np.float32)
        out.append((torch.from_numpy(box).to(dtype).float().numpy(), torch.from_numpy(cls).to(dtype).float().numpy()))
    return out


def chw_of(pl):
    """the plugin inputs [B, 4 + classes, cells] of box / class planes, the DFL done in float64 (tests/test_gpu_yolo11_tasks.py::_heads)"""
    out = []
    for box, cls in pl:
        B, _, n = box.shape
        bins = torch.from_numpy(box.reshape(B, 4, 16, n)).double().softmax(2)
        dist = (bins * torch.arange(16.0, dtype=torch.float64)[None, None, :, None]).sum(2).float().numpy()
        out.append(np.concatenate([dist, cls], 1))
    return out


def nhwc(x, ld, dtype, gpu, pad=(float("nan"), 60000.0)):
    """[B, C, cells] -> device [B, cells, ld]; the channels beyond C hold the `pad` values in turn"""
    B, C, n = x.shape
    t = np.empty((B, n, ld), np.float32)
    for c in range(C, ld):
        t[..., c] = pad[(c - C) % len(pad)]
    t[..., :C] = x.transpose(0, 2, 1)
    return torch.from_numpy(t).to(dtype).to(gpu)


def fused(pl, classes, H, W, max_out, dtype, gpu, box_ld=64, cls_ld=None, **kw):
    cls_ld = r8(classes) if cls_ld is None else cls_ld
    box = [nhwc(b, box_ld, dtype, gpu) for b, _ in pl]
    cls = [nhwc(c, cls_ld, dtype, gpu) for _, c in pl]
    with time_limit():
        out = capi.yolov9_head_decode_nhwc(box, cls, classes, H, W, torch.arange(16.0).to(gpu), max_out, **kw)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def planar(chw, classes, H, W, max_out, gpu):
    with time_limit():
        out = capi.yolov9_decode([torch.from_numpy(x).to(gpu) for x in chw], classes, H, W, max_out)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def rows(dec, b, det=DET):
    n = int(dec[b, 0])
    return dec[b, 1:1 + n * det].reshape(n, det)[:, :6]


def compare(got, ref, what=""):
    """got: rows of 38 floats; ref: the oracle's rows of 90 floats (YOLOv8's Detection); the first six floats of every record"""
    assert np.array_equal(got[:, 0], ref[:, 0]), (what, got[:, 0], ref[:, 0])
    worst = 0.0
    for b in range(ref.shape[0]):
        G, R = rows(got, b), rows(ref, b, yp.DET_FLOATS)
        assert np.array_equal(G[:, 5], R[:, 5]), f"{what}: class ids / slot order"
        assert np.allclose(G[:, 4], R[:, 4], rtol=0, atol=2e-7), what
        assert np.isfinite(G[:, :4]).all()
        assert np.allclose(G[:, :4], R[:, :4], rtol=1e-5, atol=1e-4), (what, np.abs(G[:, :4] - R[:, :4]).max())
        if len(G):
            worst = max(worst, float(np.abs(G[:, :4] - R[:, :4]).max()))
    return worst


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("B,H,W,classes", [(2, 64, 96, 80), (2, 160, 160, 80), (2, 160, 160, 3), (2, 160, 160, 13), (3, 640, 640, 80)])
def test_head_and_plugin_kernel_match_oracle(gpu, B, H, W, classes, dtype):
    """64 x 96: 126 cells, below one workgroup, ragged levels.  160 x 160: 525 cells, the 512-cell chunk boundary inside level 1; 3 and 13
    classes read the element tail next to padding that holds NaN and 60000.  640^2 x 3: bulk.  Strides: box_ld 64 and 72, cls_ld the
    classes rounded up to 8 and 8 more."""
    pl = planes(B, H, W, classes, dtype)
    chw = chw_of(pl)
    cells = cells_of(H, W)
    mo = cells + 1 if cells < 1000 else 1000
    ref = yp.decode_c(chw, classes, H, W, list(STRIDES), mo)
    assert 3 <= ref[:, 0].min() and ref[:, 0].max() < mo, ref[:, 0]
    plug = planar(chw, classes, H, W, mo, gpu)
    wp = compare(plug, ref, "planar plugin kernel")
    for box_ld, cls_ld in ((64, r8(classes)), (72, r8(classes) + 8)) if cells < 1000 else ((64, r8(classes)),):
        got = fused(pl, classes, H, W, mo, dtype, gpu, box_ld, cls_ld)
        wf = compare(got, ref, f"fused head box_ld {box_ld} cls_ld {cls_ld}")
        same = all(np.array_equal(rows(got, b), rows(plug, b)) for b in range(B))
        same45 = all(np.array_equal(rows(got, b)[:, 4:], rows(plug, b)[:, 4:]) for b in range(B))
        print(f"{H}x{W} nc {classes} B {B} ld {box_ld}/{cls_ld}: candidates {ref[:, 0].astype(int).tolist()} of {cells}; |box - oracle| fused {wf:.3g}, "
              f"planar {wp:.3g}; fused head against the plugin kernel: conf / class {'bit-equal' if same45 else 'differ'}, "
              f"records {'bit-equal' if same else 'differ (the fp32 DFL against the float64 one the planes carry)'}")
        assert same45


def special_planes(dtype):
    """64 x 96, 3 images: image 0 seeded, image 1 nothing passes, image 2 everything passes"""
    pl = [(b.copy(), c.copy()) for b, c in planes(3, 64, 96, 80, dtype, seed=3)]
    for _, c in pl:
        c[1] = -30.0
        c[2] = 8.0
    return pl


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_head_empty_overflow_and_untouched_rows(gpu, dtype):
    """max_out = 40 below the 126 cells: the full image's count is 40 and its records are the first 40 in canonical order; the floats of a
    row beyond its records, and the row behind the batch, keep the sentinel"""
    pl, mo = special_planes(dtype), 40
    chw = chw_of(pl)
    ref = yp.decode_c(chw, 80, 64, 96, list(STRIDES), mo)
    assert ref[1, 0] == 0 and ref[2, 0] == mo and 0 < ref[0, 0] < mo
    full = yp.decode_c(chw, 80, 64, 96, list(STRIDES), 127)
    assert full[2, 0] == 126 and np.array_equal(rows(full, 2, 90)[:mo], rows(ref, 2, 90))
    out = torch.full((4, 1 + mo * DET), SENTINEL, dtype=torch.float32, device=gpu)
    got = fused(pl, 80, 64, 96, mo, dtype, gpu, out=out, batch=3)
    compare(got[:3], ref)
    assert (got[3] == SENTINEL).all()
    for b in range(3):
        n = int(got[b, 0])
        assert (got[b, 1 + n * DET:] == SENTINEL).all()
        assert (got[b, 1:1 + n * DET].reshape(n, DET)[:, 6:] == SENTINEL).all()   # a detection record's 32 mask floats are not written
    plug = planar(chw, 80, 64, 96, mo, gpu)
    compare(plug, ref, "planar")


def test_head_class_tie_takes_the_lower_index(gpu):
    """two equal maximal logits in different 16-byte pieces (classes 17 and 63), inside one piece (40 and 41) and in the first and the last
    class (0 and 79): the lower index wins, as the reference's strict '>' scan from (0.0, class 0) returns"""
    for dtype in (torch.float16, torch.float32):
        pl = [(b.copy(), np.full_like(c, -5.0)) for b, c in planes(2, 64, 96, 80, dtype, seed=5)]
        for k, (lo, hi) in enumerate([(17, 63), (40, 41), (0, 79)]):
            for _, c in pl:
                c[:, lo, k::3] = 2.0
                c[:, hi, k::3] = 2.0
        pl[0][1][1, 63, 0] = 2.5   # image 1, cell 0: the higher index is the strict maximum
        ref = yp.decode_c(chw_of(pl), 80, 64, 96, list(STRIDES), 200)
        got = fused(pl, 80, 64, 96, 200, dtype, gpu)
        compare(got, ref)
        assert got[0, 0] == 126
        n0 = 96
        assert (rows(got, 0)[:n0, 5].reshape(-1, 3) == [17, 40, 0]).all()
        assert rows(got, 1)[0, 5] == 63 and (rows(got, 1)[1:3, 5] == [40, 0]).all()


def test_head_nan_logits_and_extreme_dfl_bins(gpu):
    """NaN logits beside a passing one (a NaN fails 'p > best'), a cell of NaN logits only (dropped), all-equal DFL bins and bins of
    +-60000: finite boxes"""
    for dtype in (torch.float16, torch.float32):
        pl = [(b.copy(), c.copy()) for b, c in planes(2, 64, 96, 80, dtype, seed=7)]
        b0, c0 = pl[0]
        c0[0, :, 5] = np.nan
        c0[0, 33, 5] = 1.0        # passes, between NaNs
        c0[0, :, 6] = np.nan      # nothing to compare against: dropped
        c0[0, :, 7] = -30.0
        c0[0, 2, 7] = 3.0
        b0[0, :, 7] = 0.25        # all-equal bins: the expectation is 7.5 on every side
        c0[0, :, 8] = -30.0
        c0[0, 70, 8] = 3.0
        b0[0, :, 8] = -60000.0
        b0[0, [3, 16 + 15, 32 + 0, 48 + 9], 8] = 60000.0   # one-hot: distances 3, 15, 0, 9
        ref = yp.decode_c(chw_of(pl), 80, 64, 96, list(STRIDES), 200)
        got = fused(pl, 80, 64, 96, 200, dtype, gpu)
        compare(got, ref)
        plug = planar(chw_of(pl), 80, 64, 96, 200, gpu)
        compare(plug, ref, "planar")
        # level 0 is 12 x 8 cells of stride 8: cell 7 = (row 0, col 7), cell 8 = (row 0, col 8)
        r7 = [r for r in rows(got, 0) if r[5] == 2 and r[4] > 0.9]
        r8_ = [r for r in rows(got, 0) if r[5] == 70 and r[4] > 0.9]
        assert len(r7) == 1 and np.allclose(r7[0][:4], [(7.5 - 7.5) * 8, (0.5 - 7.5) * 8, (7.5 + 7.5) * 8, (0.5 + 7.5) * 8], atol=1e-4)
        assert len(r8_) == 1 and np.allclose(r8_[0][:4], [(8.5 - 3) * 8, (0.5 - 15) * 8, (8.5 + 0) * 8, (0.5 + 9) * 8], atol=1e-4)
        assert any(r[5] == 33 and abs(r[4] - 1 / (1 + np.exp(-1.0))) < 1e-6 for r in rows(got, 0))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_head_gate_and_the_pre_filter_in_front_of_it(gpu, dtype):
    """The score kernel flags a cell when its largest raw logit is above -2.3 and settles it with the exact sigmoid against 0.1 (logit
    -2.19722).  One cell per value of tests/yolo_head_cases.py's family (c) - below the pre-filter, between it and the gate (flagged, then
    dropped) and just above the gate (kept) - at the first and the last lane of a wave, the last cell of a level and the first of the next,
    on 160 x 160 (525 cells, three workgroups); all other classes of those cells at -30.  Against the oracle: count, order and class
    equal, conf within 2e-7, no record left out; boxes under the bound derived in tests/yolo_head_cases.py."""
    from tests import yolo_head_cases as hc
    dt = "f16" if dtype == torch.float16 else "f32"
    B, H, W, nc = 3, 160, 160, 80
    pl = [(b.copy(), c.copy()) for b, c in planes(B, H, W, nc, dtype, seed=9)]
    off, pos, th = hc.level_offsets("160x160"), hc.positions("160x160"), hc.thresholds(dt)
    placed = {}
    for k, kind in enumerate(hc.KINDS):   # every value at every kind of position, as far as three images have such cells (two boundaries each)
        for j in (range(len(th)) if k % 2 == 0 else reversed(range(len(th)))):
            free = [(b, g) for t in range(B) for b in [(j + k + t) % B] for g in pos[kind] if (b, g) not in placed]
            if free:
                placed[free[0]] = j
    for (b, g), j in placed.items():
        l = int(np.searchsorted(off, g, side="right")) - 1
        pl[l][1][b, :, g - off[l]] = -30.0
        pl[l][1][b, (7 * j + 3) % nc, g - off[l]] = th[j][0]
    at = {(j, k) for (b, g), j in placed.items() for k in hc.KINDS if g in pos[k]}
    assert at >= {(j, k) for j in range(len(th)) for k in hc.KINDS[:2]}
    assert all((j, "level_last") in at or (j, "level_first") in at for j in range(len(th)))
    logits = np.concatenate([c for _, c in pl], 2).astype(np.float64)                    # [B, classes, cells]
    p = 1 / (1 + np.exp(-logits.max(1)))
    kept = [np.nonzero(p[b] >= 0.1)[0] for b in range(B)]
    others = np.ones_like(p, bool)
    for b, g in placed:
        others[b, g] = False
    assert (np.abs(1 / (1 + np.exp(-logits)) - 0.1).min(1)[others] > 1e-6).all()        # nothing else sits at the gate
    for (b, g), j in placed.items():
        assert (g in kept[b]) == th[j][2]
    mo = 526
    ref = yp.decode_c(chw_of(pl), nc, H, W, list(STRIDES), mo)
    assert np.array_equal(ref[:, 0], [len(k) for k in kept])
    got = fused(pl, nc, H, W, mo, dtype, gpu)
    compare(got, ref, "the gate")
    # boxes: the derived bound instead of compare()'s rtol 1e-5 / atol 1e-4
    bins = np.concatenate([b for b, _ in pl], 2).transpose(0, 2, 1).reshape(B, 525, 4, 16)
    w = np.arange(16, dtype=np.float32)
    d, S, A = hc.dfl_terms(bins, w)
    bd = hc.bound_of(d, S, A, w)
    stride = hc.cell_geometry("160x160")[2]
    worst = 0.0
    for b in range(B):
        G, R = rows(got, b), rows(ref, b, yp.DET_FLOATS)
        bound = hc.coord_bound(bd[b][kept[b]], d[b][kept[b]], stride[kept[b]][:, None], R[:, :4].astype(np.float64))
        worst = max(worst, float((np.abs(G[:, :4].astype(np.float64) - R[:, :4]) / bound).max()))
    print(f"yolov9 head at the gate, {dt}: records {ref[:, 0].astype(int).tolist()} of 525, max err / bound {worst:.3f}")
    assert worst <= 1.0, worst


def test_head_is_batch_invariant(gpu):
    """image 0 of a batch decodes bit-equal when run alone"""
    pl = planes(3, 640, 640, 80, torch.float16)
    allb = fused(pl, 80, 640, 640, 1000, torch.float16, gpu)
    alone = fused([(b[:1], c[:1]) for b, c in pl], 80, 640, 640, 1000, torch.float16, gpu)
    assert allb[0, 0] > 0 and np.array_equal(allb[:1], alone)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_head_refusals_leave_the_buffers_untouched(gpu, dtype):
    H, W, nc, mo = 64, 96, 80, 50
    pl = planes(2, H, W, nc, dtype)
    dfl = torch.arange(16.0).to(gpu)
    box = [nhwc(np.concatenate([b, b[:, :16]], 1), 88, dtype, gpu) for b, _ in pl]    # 80 real channels and room for odd strides
    cls = [nhwc(np.concatenate([c, c[:, :8]], 1), 96, dtype, gpu) for _, c in pl]
    L = capi.lib()
    import ctypes
    L.trtx_yolov9_head_decode_workspace.restype = ctypes.c_size_t
    ws_bytes = L.trtx_yolov9_head_decode_workspace(2, H, W)

    def attempt(status, box_t=box, cls_t=cls, ws_n=ws_bytes, **kw):
        out = torch.full((2, 1 + mo * DET), SENTINEL, dtype=torch.float32, device=gpu)
        ws = torch.full((ws_n,), 0x5A, dtype=torch.uint8, device=gpu)
        with time_limit():
            with pytest.raises(capi.TrtxError) as e:
                capi.yolov9_head_decode_nhwc(box_t, cls_t, nc, H, W, dfl, mo, out=out, ws=ws, **kw)
            torch.cuda.synchronize()
        assert e.value.status == status, (e.value.status, kw)
        assert (out == SENTINEL).all() and (ws == 0x5A).all()

    vec = 8 if dtype == torch.float16 else 4
    attempt(4, box_ld=[88 - 1] * 3)                       # odd box stride
    attempt(4, cls_ld=[96 - vec // 2] * 3)                # a class stride that is no 16-byte multiple
    attempt(4, box_ld=[56] * 3)                           # box_ld < 64
    attempt(4, cls_ld=[72] * 3)                           # cls_ld < classes
    off_box = [box[0].flatten()[1:1 + 2 * 96 * 80].reshape(2, 96, 80)] + box[1:]   # a base one element off
    attempt(4, box_t=off_box, box_ld=[80, 88, 88])
    off_cls = cls[:2] + [cls[2].flatten()[1:1 + 2 * 6 * 88].reshape(2, 6, 88)]
    attempt(4, cls_t=off_cls, cls_ld=[96, 96, 88])
    attempt(3, ws_n=ws_bytes - 256)                       # TRTX_ERR_WORKSPACE
    # and the same tensors with their own strides decode
    out = capi.yolov9_head_decode_nhwc(box, cls, nc, H, W, dfl, mo)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), fused(pl, nc, H, W, mo, dtype, gpu))


def test_planar_kernel_copies_the_mask_coefficients(gpu):
    """is_segmentation: inputs [B, 4 + classes + 32, cells]; floats 6 .. 37 of a record are the cell's 32 coefficients, from the channels
    behind the classes (yolov9/plugin/yololayer.cu:173-175).  Against the oracle's YOLOv8 seg decode, whose record starts with the same
    38 floats.  13 classes on 64 x 96: ragged levels, and no channel offset is a multiple of 8."""
    B, H, W, nc, mo = 2, 64, 96, 13, 127
    pl = planes(B, H, W, nc, torch.float32, seed=11)
    rng = np.random.default_rng(12)
    chw = [np.concatenate([x, rng.normal(0, 1, size=(B, 32, x.shape[2])).astype(np.float32)], 1) for x in chw_of(pl)]
    ref = yp.decode_ex_c(chw, nc, H, W, list(STRIDES), mo, seg=True)
    assert ref[:, 0].min() >= 3
    with time_limit():
        got = capi.yolov9_decode([torch.from_numpy(x).to(gpu) for x in chw], nc, H, W, mo, is_seg=True).cpu().numpy()
    compare(got, ref, "planar, is_segmentation")
    for b in range(B):
        n = int(ref[b, 0])
        G = got[b, 1:1 + n * DET].reshape(n, DET)
        R = ref[b, 1:1 + n * yp.DET_FLOATS].reshape(n, yp.DET_FLOATS)
        assert np.array_equal(G[:, 6:38], R[:, 6:38]) and np.abs(G[:, 6:38]).max() > 0.5


def test_conv1x1_over_24_channels_on_the_mfma_path(gpu):
    """The 24 -> 24 1x1 convolution (the 1x1 branch of RepConvN in YOLOv9t's 24-channel RepNCSP blocks) lowers to the implicit-GEMM kernel
    with a 32-channel k-step whose last 8 channels load zeros; the pixel's own stride stays 24, so a step that read 32 channels would
    read the next pixel.  Against fp64 on the fp16 operands, the bound of tests/test_gpu_yolov5.py's 16-channel case: one fp16 rounding
    of the result, fp32 accumulation of 24 products; with a residual, one more rounding of the sum."""
    rng = np.random.default_rng(24)
    N, H, W, C = 3, 13, 11, 24   # 429 pixels: ragged last tile
    w = rng.normal(0, 0.3, size=(C, C, 1, 1)).astype(np.float32)
    b = rng.normal(0, 0.5, size=C).astype(np.float32)
    x = torch.from_numpy(rng.normal(0, 1, size=(N, H, W, C)).astype(np.float32)).half()
    pk, cp, kp, _ = capi.pack_conv_weights_f16(w, cin_pad=32)
    assert kp == 32
    bias = torch.zeros(cp)
    bias[:C] = torch.from_numpy(b)
    res = torch.from_numpy(rng.normal(0, 1, size=(N, H, W, C)).astype(np.float32)).half()
    for residual in (None, res):
        with time_limit():
            y = capi.conv2d_nhwc_f16(x.to(gpu), torch.from_numpy(pk.view(np.int16)).to(gpu), bias.to(gpu), C, 1, 1, 1, 0, "none",
                                     residual=None if residual is None else residual.to(gpu)).cpu().double()
        w16 = torch.from_numpy(w).half().double()
        xd = x.double().permute(0, 3, 1, 2)
        pre = torch.nn.functional.conv2d(xd, w16, torch.from_numpy(b).double())
        mag = torch.nn.functional.conv2d(xd.abs(), w16.abs(), torch.from_numpy(b).double().abs())
        ref = pre
        bound = 2.0 ** -11 * pre.abs() + 1e-5 * (mag + 1)
        if residual is not None:
            # the epilogue is "bias, act1, rounding, residual, act2" (kernels/igemm_tile.h): the convolution's result is rounded to fp16 as the
            # un-fused graph would store it, then the fp16 residual is added in fp32 and the sum rounded: two fp16 roundings, the first of
            # |pre| (counted above), the second of |pre + residual|
            ref = pre + residual.double().permute(0, 3, 1, 2)
            bound = bound + 2.0 ** -11 * ref.abs()
        ref, bound = ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)
        err = (y - ref).abs()
        print(f"24 -> 24 1x1{' + residual' if residual is not None else ''}: max err {err.max().item():.3g}, max err / bound {(err / bound).max().item():.3g}")
        assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------- NMS
def clustered(B, max_out, n, seed, classes=6):
    """decode rows [B, 1 + max_out * 38] of n corner-box records in clusters: a few centres per class, boxes jittered around them,
    distinct confidences (a tie's order is unspecified in the reference: std::sort)"""
    rng = np.random.default_rng(seed)
    dec = np.zeros((B, 1 + max_out * DET), np.float32)
    for b in range(B):
        c = rng.uniform(60, 580, size=(12, 2))
        k = rng.integers(0, 12, size=n)
        ctr = c[k] + rng.normal(0, 6, size=(n, 2))
        wh = rng.uniform(40, 120, size=(n, 2))
        rec = np.zeros((n, DET), np.float32)
        rec[:, 0:2] = ctr - wh / 2
        rec[:, 2:4] = ctr + wh / 2
        rec[:, 4] = rng.permutation(n).astype(np.float32) / n * 0.9 + 0.05
        rec[:, 5] = k % classes
        rec[:, 6:] = rng.normal(size=(n, 32))
        dec[b, 0] = n
        dec[b, 1:1 + n * DET] = rec.reshape(-1)
    return dec


def check_nms(dec, max_out, gpu, conf=0.5, iou=0.45):
    with time_limit():
        ki, kc, kd = capi.yolov9_nms(torch.from_numpy(dec).to(gpu), max_out, conf, iou)
        torch.cuda.synchronize()
    ri, rc, rd = yp.v5_batch_nms_c(corner_to_centre_f32(dec, max_out), max_out, conf, iou)
    ki, kc, kd = ki.cpu().numpy(), kc.cpu().numpy(), kd.cpu().numpy()
    assert np.array_equal(kc, rc), (kc, rc)
    for b in range(dec.shape[0]):
        assert np.array_equal(ki[b, :rc[b]], ri[b, :rc[b]])
        assert np.array_equal(kd[b, :rc[b]], rd[b, :rc[b]])   # centre-format records, bit-equal
    return rc


def test_nms_matches_the_yolov5_oracle_on_converted_records(gpu):
    dec = clustered(3, 300, 200, seed=1)
    dec[1, 0] = 0                                   # an empty image
    rc = check_nms(dec, 300, gpu)
    assert rc[0] > 5 and rc[1] == 0 and rc[2] > 5 and rc[0] < 100
    full = clustered(2, 128, 128, seed=2)           # a full buffer
    assert check_nms(full, 128, gpu).min() > 5
    edge = clustered(1, 64, 40, seed=3)
    edge[0, 1 + 4:1 + 40 * DET:DET][:10] = np.float32(0.5)   # conf exactly at the threshold: dropped ("conf <= thresh")
    rc = check_nms(edge, 64, gpu, conf=0.5)
    ri, _, _ = yp.v5_batch_nms_c(corner_to_centre_f32(edge, 64), 64, 0.5, 0.45)
    assert rc[0] > 0 and not set(ri[0, :rc[0]].tolist()) & set(range(10))


# ---------------------------------------------------------------------------------------------------------------- engines
def run(plan, x, gpu, batch=None, fill=float("nan")):
    with time_limit(120):
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


def build(name, path, gpu, **kw):
    with time_limit(240):   # on a GPU the build times every convolution's tactics
        return engine.build_plan(name, path, **kw)


def kinds(plan):
    return [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]]


def match_detections(dec, dec_ref, max_out, gpu, skip=None):
    """tests/test_gpu_yolov5.py's matching rule on corner-format records (x1, y1, x2, y2, conf, class): per reference candidate the
    candidate of the same class with the nearest centre, matched when their IoU is above 0.9.  No image may be left out (every count is
    below max_out).  skip: per image a bool per reference record (candidates within 0.02 of the gate), or None."""
    st = dict(ref=0, matched=0, min_iou=1.0, unmatched_by_class={})
    for b in range(dec_ref.shape[0]):
        assert dec_ref[b, 0] < max_out and dec[b, 0] < max_out, (b, dec_ref[b, 0], dec[b, 0], max_out)
        R, G = torch.from_numpy(rows(dec_ref, b)).to(gpu), torch.from_numpy(rows(dec, b)).to(gpu)
        if skip is not None:
            R = R[~torch.from_numpy(skip[b]).to(gpu)]
        st["ref"] += len(R)
        for c in torch.unique(R[:, 5]).tolist():
            r, g = R[R[:, 5] == c], G[G[:, 5] == c]
            if len(g) == 0:
                st["unmatched_by_class"][int(c)] = st["unmatched_by_class"].get(int(c), 0) + len(r)
                continue
            d = ((r[:, None, 0] + r[:, None, 2]) - (g[None, :, 0] + g[None, :, 2])).abs() + ((r[:, None, 1] + r[:, None, 3]) - (g[None, :, 1] + g[None, :, 3])).abs()
            ix = (torch.minimum(r[:, None, 2], g[None, :, 2]) - torch.maximum(r[:, None, 0], g[None, :, 0])).clamp(min=0)
            iy = (torch.minimum(r[:, None, 3], g[None, :, 3]) - torch.maximum(r[:, None, 1], g[None, :, 1])).clamp(min=0)
            area = lambda t: (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])  # noqa: E731
            pair = ix * iy / (area(r)[:, None] + area(g)[None] - ix * iy)
            iou = torch.where(d <= d.min(1, keepdim=True).values, pair, torch.full_like(pair, -1.0)).max(1).values
            ok = iou > 0.9
            st["matched"] += int(ok.sum())
            if not ok.all():
                st["unmatched_by_class"][int(c)] = st["unmatched_by_class"].get(int(c), 0) + int((~ok).sum())
            if ok.any():
                st["min_iou"] = min(st["min_iou"], float(iou[ok].min()))
    return st


def near_gate(heads, counts, margin=0.02):
    """Per image, for the records an engine wrote from `heads` ([B, 84, cells] per level) in canonical (level, cell) order: is the
    largest class probability within `margin` of the 0.1 gate"""
    B = heads[0].shape[0]
    logit = np.concatenate([h[:, 4:].max(1) for h in heads], 1).astype(np.float32)
    p = np.float32(1) / (np.float32(1) + np.exp(-logit))
    out = []
    for b in range(B):
        kept = ~(p[b].astype(np.float64) < 0.1)
        assert kept.sum() == counts[b], (b, kept.sum(), counts[b])   # (a probability within an ulp of the gate would break this: not at these seeds)
        out.append(np.abs(p[b][kept] - 0.1) < margin)
    return out


def twin_check(name, conv, B, S, gpu, decode=False):
    path, sd = yolov9_wts(name, conv)
    mo = cells_of(S, S) + 16
    plan = build(name, path, gpu, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo, converted=conv)
    x = synth.images(B, S, S, seed=5)
    got = run(plan, x, gpu)
    with torch.inference_mode():
        heads, strides = Yolov9(sd, name, bool(conv)).heads(torch.from_numpy(x))
    mine = []
    for i, h in enumerate(heads):
        g = got[f"head{i}"].reshape(h.shape)
        err = (g - h).abs().max().item()
        print(f"{name} converted={conv} head{i}: err {err:.3g}, |head| {h.abs().max().item():.3g}")
        assert err <= 1e-4 * max(1.0, h.abs().max().item()), (i, err)
        mine.append(g.numpy())
    if decode:
        ref = yp.decode_c(mine, 80, S, S, strides, mo)
        assert 0 < ref[:, 0].min() and ref[:, 0].max() < mo
        compare(got["output"].reshape(B, -1).numpy(), ref, "engine output against the oracle decode of its own heads")


def test_yolov9t_fp32_engine_matches_twin_and_oracle_decode(gpu):
    twin_check("yolov9t", 1, 2, 128, gpu, decode=True)


@pytest.mark.parametrize("name", ["yolov9m", "yolov9c"])
def test_yolov9_fp32_engines_with_the_auxiliary_branch_match_twin(name, gpu):
    """unconverted m (odd widths: 240 / 120 / 60 channels) and c (ADown on a 4 x 4 map): CBLinear / CBFuse, DualDDetect on the auxiliary features"""
    twin_check(name, 0, 1, 64, gpu)


@pytest.mark.parametrize("name,B,S", [("yolov9t", 4, 128), ("gelanc", 1, 64)])
def test_yolov9_fp16_engine_tracks_fp32_engine(name, B, S, gpu):
    """fp16 storage, fp32 accumulation, against the fp32 engine: head values within fp16_walk(sites, max |head|) with two sites per
    convolution (packed weights, stored output); detections of the fused head (no marked heads) matched as parity.py asks, candidates
    whose class probability is within 0.02 of the 0.1 gate skipped, no image left out"""
    path, _ = yolov9_wts(name)
    x = synth.images(B, S, S, seed=12)
    mo = cells_of(S, S) + 16
    p16 = build(name, path, gpu, batch=B, h=S, w=S, fp16=1, max_out=mo)
    p16h = build(name, path, gpu, batch=B, h=S, w=S, fp16=1, mark_heads=1, max_out=mo)
    p32h = build(name, path, gpu, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo)
    k = kinds(p16)
    assert k.count("yolo9_head") == 1 and not {"plugin", "to_linear", "softmax", "scatter"} & set(k)
    sites = 2 * len(convs_of(engine.describe_plan(p16, lowered=True)))
    g16, g16h, g32 = run(p16, x, gpu), run(p16h, x, gpu), run(p32h, x, gpu)
    h32 = []
    for i in range(3):
        a, r = g16h[f"head{i}"], g32[f"head{i}"]
        assert torch.isfinite(a).all()
        err, lim = (a - r).abs().max().item(), fp16_walk(sites, r.abs().max().item())
        print(f"{name} B{B} {S}: head{i} err {err:.3g}, bound {lim:.3g} ({sites} sites)")
        assert err <= lim, i
        h32.append(r.reshape(B, 84, -1).numpy())
    ref = g32["output"].reshape(B, -1).numpy()
    st = match_detections(g16["output"].reshape(B, -1).numpy(), ref, mo, gpu, skip=near_gate(h32, ref[:, 0]))
    print(st, "counts", ref[:, 0].min(), "-", ref[:, 0].max())
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_agrees_with_the_plugin_route(gpu, monkeypatch):
    """The fused fp16 plan against the plan the same build makes with TRTX_YOLO9_HEAD=0 (layout passes, the DFL chain, the plugin).  Two
    plans, each with its own tactics: matched as above, not bit-compared - and with no candidate skipped."""
    path, _ = yolov9_wts("yolov9t")
    B, S = 4, 128
    mo = cells_of(S, S) + 16
    x = synth.images(B, S, S, seed=12)
    fused_plan = build("yolov9t", path, gpu, batch=B, h=S, w=S, fp16=1, max_out=mo)
    assert kinds(fused_plan).count("yolo9_head") == 1
    a = run(fused_plan, x, gpu)["output"].reshape(B, -1).numpy()
    monkeypatch.setenv("TRTX_YOLO9_HEAD", "0")
    route = build("yolov9t", path, gpu, batch=B, h=S, w=S, fp16=1, max_out=mo)
    k = kinds(route)
    assert k.count("plugin") == 1 and k.count("yolo9_head") == 0 and k.count("to_linear") == 9
    r = run(route, x, gpu)["output"].reshape(B, -1).numpy()
    st = match_detections(a, r, mo, gpu)
    print(st, "counts fused", a[:, 0], "plugin route", r[:, 0])
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_below_its_maximum_batch(gpu):
    """a max_batch = 8 plan enqueued with batch 3 decodes three images and leaves rows 3..7 of the NaN-filled output untouched"""
    path, _ = yolov9_wts("yolov9t")
    S = 128
    mo = cells_of(S, S) + 16
    plan = build("yolov9t", path, gpu, batch=8, h=S, w=S, fp16=1, max_out=mo)
    assert kinds(plan).count("yolo9_head") == 1
    x = synth.images(8, S, S, seed=12)
    full = run(plan, x, gpu)["output"].reshape(8, -1).numpy()
    part = run(plan, x, gpu, batch=3)["output"].reshape(8, -1).numpy()
    assert np.isnan(part[3:]).all()
    assert (part[:3, 0] > 0).all() and (part[:3, 0] < mo).all()
    for b in range(3):
        assert np.isfinite(rows(part, b)).all()
    st = match_detections(part[:3], full[:3], mo, gpu)
    print(st, "counts", part[:3, 0], full[:, 0])
    assert st["ref"] > 0 and st["matched"] / st["ref"] >= 1 - FP16_MATCH and st["min_iou"] >= 1 - FP16_IOU, st
