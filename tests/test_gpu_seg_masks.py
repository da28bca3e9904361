"""trtx_seg_masks on the GPU, the kernel alone: hand-made decode buffers and keep lists against tests/seg_mask_ref.py in fp64 (the rect
in fp32 exactly as the reference's get_downscale_rect computes it).

The zero pattern is exact: a written pixel is 0.0f if and only if it lies outside the clipped rect.  Values obey
    |m - m64| <= (33 * 2^-24 * sum_j |coef_j * proto_j|) / 4 + 2^-22
the sequential fp32 sum's bound through a function of slope at most 1/4, plus expf and the division.  An fp32 NumPy restatement of the
reference loop reaches 0.06 of this bound (CPU, 64 detections on 40x40, |e| up to 32).  The output buffer is pre-filled with NaN and
framed by guard floats: slots at or beyond the kept count, and the guards, must still hold that NaN bit for bit."""
import functools

import numpy as np
import pytest
import torch

import seg_mask_ref as ref
from tensorrtx_amd import capi

pytestmark = pytest.mark.gpu
NAN_BITS = np.float32(np.nan).view(np.int32)
INF = float("inf")

# (left, top, right, bottom) in network pixels on a 160 x 160 network (40 x 40 planes)
BOXES_160 = [
    (40, 48, 100, 120),                                                            # interior
    (0, 40, 40, 80), (120, 40, 160, 80), (40, 0, 80, 40), (40, 120, 80, 160),      # touching each border
    (-20, 40, 30, 80), (130, 40, 190, 80), (40, -30, 80, 20), (40, 140, 80, 200),  # crossing each border
    (-100, 40, -20, 80), (180, 40, 260, 80), (40, -90, 80, -10), (40, 200, 80, 260),  # wholly outside on each side
    (50, 40, 51, 80), (40, 60, 80, 61.5),                                          # a width / height that rounds and truncates to 0
    (10, 18, 20, 28),       # edges 2.5, 4.5 and sizes 2.5: round() gives 3, 5, 3; truncation 2, 4, 2; half-to-even 2, 4, 2
    (-10, 40, 30, 70),      # left -2.5: round() gives -3, truncation and half-to-even -2; height 7.5 -> 8 / 7
    (6, 6, 20, 12),         # left 1.5 (2 either way of rounding, 1 truncated), width 3.5 -> 4 / 3
    (0, 0, 160, 160),       # the whole image
    (80, 84, 84, 88),       # a 1 x 1 rect
    (-40, -40, 200, 200),   # larger than the image on every side
]


def record(box, box_format, coef, det_floats):
    l, t, r, b = box
    rec = np.zeros(det_floats, np.float32)
    rec[:4] = ((l + r) / 2, (t + b) / 2, r - l, b - t) if box_format == 0 else (l, t, r - l, b - t)
    rec[4], rec[5] = 0.9, 3
    rec[6:38] = coef
    rec[38:] = -7.0   # the keypoint / angle floats of the long record are never read
    return rec


def make_case(boxes_per_image, counts, box_format, det_floats, mask_h, mask_w, max_out, seed, special=None):
    """boxes_per_image: per image a list of boxes; record i of image b goes to slot (37 i + 11 + 5 b) mod max_out (out of slot order, high
    slots first for some) and is kept as detection i.  counts: keep_cnt per image (<= the number of boxes).  special(rec, b, i) may edit a
    record."""
    rng = np.random.default_rng(seed)
    B = len(boxes_per_image)
    dec = rng.normal(0, 1, size=(B, 1 + max_out * det_floats)).astype(np.float32)   # unreferenced slots hold noise
    keep_idx = np.full((B, max_out), -1, np.int32)
    for b, boxes in enumerate(boxes_per_image):
        assert len(boxes) <= max_out and max_out % 2 == 0
        dec[b, 0] = len(boxes)
        for i, box in enumerate(boxes):
            slot = (37 * i + 11 + 5 * b) % max_out
            rec = record(box, box_format, rng.normal(0, rng.choice([0.3, 1.0, 2.0]), size=32), det_floats)
            if special:
                special(rec, b, i)
            dec[b, 1 + slot * det_floats:1 + (slot + 1) * det_floats] = rec
            keep_idx[b, i] = slot
    proto = rng.normal(0, 1, size=(B, 32, mask_h, mask_w)).astype(np.float32)
    return dec, keep_idx, np.asarray(counts, np.int32), proto


def check(gpu, case, box_format, det_floats, net_h, net_w, max_keep, guard=64, what=""):
    dec, keep_idx, keep_cnt, proto = case
    B, _, mh, mw = proto.shape
    n = B * max_keep * mh * mw
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=gpu)
    out = buf[guard:guard + n]
    assert (out.data_ptr() % 16 == 0) == (guard % 4 == 0)
    capi.seg_masks(torch.from_numpy(dec).to(gpu), torch.from_numpy(keep_idx).to(gpu), torch.from_numpy(keep_cnt).to(gpu),
                   torch.from_numpy(proto).to(gpu), net_h, net_w, max_keep, box_format, out=out)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    got = raw[guard:guard + n].reshape(B, max_keep, mh, mw)
    want, inside, mag = ref.seg_masks(dec, det_floats, box_format, keep_idx, keep_cnt, max_keep, proto, net_h, net_w)
    written = np.zeros((B, max_keep), bool)
    for b in range(B):
        written[b, :min(int(keep_cnt[b]), max_keep)] = True
    bits = got.view(np.int32)
    assert (raw[:guard].view(np.int32) == NAN_BITS).all() and (raw[guard + n:].view(np.int32) == NAN_BITS).all(), "guards"
    assert (bits[~written] == NAN_BITS).all(), "slots at or beyond the kept count are not written"
    w_in = inside & written[:, :, None, None]
    w_out = ~inside & written[:, :, None, None]
    assert (bits[w_out] == 0).all(), "outside the rect: +0.0f"
    assert (got[w_in] != 0).all(), "inside the rect: never 0.0f"
    nan_ref = np.isnan(want) & w_in
    assert np.array_equal(np.isnan(got) & w_in, nan_ref), "a NaN coefficient propagates, and nothing else is NaN"
    ok = w_in & ~nan_ref
    err, lim = np.abs(got.astype(np.float64) - want)[ok], ref.bound(mag)[ok]
    ratio = (err / lim).max() if err.size else 0.0
    print(f"{what} fmt {box_format} det {det_floats} {mh}x{mw}: kept {keep_cnt.tolist()} (max_keep {max_keep}), rect pixels {int(ok.sum())}, "
          f"NaN pixels {int(nan_ref.sum())}, max err {err.max() if err.size else 0:.3g}, max err / bound {ratio:.3g}")
    assert (err <= lim).all()
    return got, inside


@functools.lru_cache(maxsize=None)
def boxes_case(box_format, det_floats):
    rng = np.random.default_rng(7)
    img0 = list(BOXES_160) + [(40, 48, 100, 120), (20, 40, 140, 80), (60, 20, 100, 60)]
    nan_i, inf_i, huge_i = len(BOXES_160), len(BOXES_160) + 1, len(BOXES_160) + 2
    img2 = []
    for _ in range(30):
        l, r = np.sort(rng.uniform(-40, 200, size=2))
        img2.append((float(l), float(rng.uniform(-40, 100)), float(r), float(rng.uniform(100, 200))))

    def special(rec, b, i):
        if b == 0 and i == nan_i:
            rec[6 + 5] = np.nan
        if b == 0 and i == inf_i:
            rec[2] = INF      # infinite w: format 0 has -inf / +inf edges (empty); format 1 clamps the right edge to the network
        if b == 0 and i == huge_i:
            rec[3] = 3e38     # a finite height of 3e38: edges far outside the plane, saturating at +-2^29

    boxes = [img0, [(10, 10, 50, 50)] * 4, img2]
    return make_case(boxes, [len(img0), 0, 30], box_format, det_floats, 40, 40, 64, 11 + box_format, special)


@pytest.mark.parametrize("det_floats", [38, 90])
@pytest.mark.parametrize("box_format", [0, 1])
def test_box_cases_on_40x40(gpu, box_format, det_floats):
    """B 3, max_out 64: image 0 keeps every listed box (with a NaN coefficient, an infinite w and an overflowing h among them), image 1
    has keep_cnt = 0, image 2 keeps 30 random boxes with max_keep = 26"""
    case = boxes_case(box_format, det_floats)
    got, inside = check(gpu, case, box_format, det_floats, 160, 160, 26, what="boxes")
    area = inside[0].sum((1, 2))
    # what the list promises, on the reference's rects: interior 15 x 18; the four outside boxes, the two zero-size ones empty
    assert area[0] == 15 * 18 and (area[9:13] == 0).all() and (area[13:15] == 0).all()
    assert area[15] == (3 * 3 if box_format == 0 else 2 * 2)          # round() half away from zero against truncation
    assert area[16] == (7 * 8 if box_format == 0 else 7 * 7)          # format 0: x -3 .. 7 clipped to 0 .. 7, y 10 .. 18; format 1: left clamps to 0
    assert area[18] == 1600 and area[19] == 1 and area[20] == 1600
    assert area[len(BOXES_160) + 1] == (0 if box_format == 0 else 35 * 10)   # the infinite w


@pytest.mark.parametrize("box_format", [0, 1])
def test_rows_longer_than_a_wave_160x160(gpu, box_format):
    """net 640^2, B 1: rects that start and end at x that are no multiple of 4 or 64"""
    boxes = [(61 * 4, 40, 131 * 4, 200), (0, 300, 640, 420), (63 * 4, 100, 64 * 4, 600), (127 * 4, 0, 129 * 4, 640)]
    case = make_case([boxes], [4], box_format, 38, 160, 160, 8, 21)
    _, inside = check(gpu, case, box_format, 38, 640, 640, 5, what="160x160")
    cols = [np.nonzero(inside[0, d].any(0))[0] for d in range(4)]
    assert [(int(c[0]), int(c[-1])) for c in cols] == [(61, 130), (0, 159), (63, 63), (127, 128)]


@pytest.mark.parametrize("box_format", [0, 1])
def test_planes_that_are_not_square_24x40(gpu, box_format):
    boxes = [(20, 10, 150, 90), (-8, -8, 40, 40), (100, 50, 170, 100), (0, 0, 160, 96)]
    case = make_case([boxes, boxes[::-1]], [4, 3], box_format, 90, 24, 40, 16, 31)
    _, inside = check(gpu, case, box_format, 90, 96, 160, 4, what="24x40")
    assert inside[0, 3].all() and inside[1, 0].all()


@pytest.mark.parametrize("mask_w", [40, 42])
def test_element_store_path(gpu, mask_w):
    """a masks base that is only 4-byte aligned (guard of 65 floats), and a plane width that is no multiple of 4"""
    boxes = [(40, 48, 100, 120), (-20, 40, 30, 80), (130, 40, 190, 80), (0, 0, 4 * mask_w, 160), (4 * mask_w - 4, 156, 4 * mask_w, 160)]
    case = make_case([boxes, boxes[::-1]], [5, 2], 0, 38, 40, mask_w, 16, 41)
    check(gpu, case, 0, 38, 160, 4 * mask_w, 6, guard=65 if mask_w == 40 else 64, what="element path")


def test_bad_arguments_leave_the_buffer_untouched(gpu):
    dec, keep_idx, keep_cnt, proto = (torch.from_numpy(a).to(gpu) for a in boxes_case(0, 38))
    out = torch.full((3 * 26 * 40 * 40,), float("nan"), dtype=torch.float32, device=gpu)

    def status(**kw):
        a = dict(decode_out=dec, keep_idx=keep_idx, keep_cnt=keep_cnt, proto=proto, net_h=160, net_w=160, max_keep=26, box_format=0, out=out)
        a.update(kw)
        with pytest.raises(capi.TrtxError) as e:
            capi.seg_masks(**a)
        return e.value.status

    assert status(net_h=120, net_w=120) == 1                          # scale 3
    assert status(net_h=160, net_w=320) == 1                          # 8 across, 4 down
    assert status(net_w=150) == 1                                     # no integer
    assert status(decode_out=torch.cat([dec, dec[:, :128]], 1).contiguous()) == 1   # 1 + 64 * 40 floats per image: det_floats 40
    assert status(max_keep=0) == 1
    assert status(box_format=2) == 1
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.int32) == NAN_BITS).all()
