"""The NMS table: single calls of plugins/yolo_nms.hip through its C entry points, shared by tests/test_nms_cases_cpu.py (the table, its
conditions and its reference, without a GPU) and tests/test_gpu_nms.py (the kernels through the C ABI).

Entry points (ENTRIES): "nms" trtx_yolo_nms (MODE 0, 90-float corner records), "v5" trtx_yolov5_nms (MODE 1, 38-float centre records), "v7"
trtx_yolov7_nms (MODE 1, 6-float centre records), "v9" trtx_yolov9_nms (MODE 3, 38-float corner records the kernel turns into centre format),
"obb" trtx_yolo_nms_obb (MODE 2, 90-float records cx, cy, w, h with the angle in the last float, ProbIoU, ">="), "g" and "gobb" the two
non-greedy kernels behind trtx_yolo_postprocess_gpu{,_obb}.

Geometry of the kernel the families aim at.  The sort is one 1024-key bitonic network per image (wave shuffles below stride 64, LDS from 64 up);
the suppression bits are a lower-triangular matrix of 64 x 64 tiles over the *sorted ranks*, a tile is skipped when the last class of its column
block is below the first class of its row block; the scan takes the 16 blocks in turn and reads the published keep words of the earlier ones.
So "n" is always the number of records that survive the confidence threshold (their ranks are 0 .. n - 1), never the number of slots: records at
or below the threshold are interleaved at every third slot (place()), which keeps slot and rank apart, and the slots behind an image's records
hold a large confident box of the image's first class (POISON) that would suppress whatever a kernel reading past the count let it meet.  Class
ids are not consecutive (79, 3, 0, ...) and descend along the slots: the sort has to reverse them.

Every image is held once, as corner boxes x1, y1, x2, y2 (+ angle); the centre formats are derived from them by the four fp32 operations of the
reference's YOLOv9 nms() (cx = (x1 + x2) / 2, cy = (y1 + y2) / 2, w = x2 - x1, h = y2 - y1; to_centre()), so "v5", "v7" and the converted "v9"
see the same centre boxes.  Outside family 7 the coordinates are small integers: every product and sum of an IoU is exact and only its
division rounds.

Reference.  The project's sequential C restatements: oracle.yolo_post.batch_nms_c ("nms"), v5_batch_nms_c ("v5"; "v7" through the widening to
38 floats; "v9" through to_centre() on the buffer, restated here), batch_nms_obb_c ("obb"), gpu_postprocess_c ("g"), gpu_postprocess_obb_c
("gobb").  Everything is compared bit for bit: selection, order, the copied floats.  The order of records that tie in (class, confidence) - and for
MODE 0 / 2 in bbox[0] - is the ORACLE'S documented canonical order (bbox[0] ascending where the reference's cmp() looks at it, then the decode
slot), which the kernel's header states as well; the reference itself sorts with an unstable std::sort and specifies nothing there.

MODE 2 and "gobb" evaluate ProbIoU through the device's sinf / cosf / expf / log, which need not agree with glibc in the last bit.  So no case
of theirs may hold a same-class pair whose ProbIoU (float64, probiou64) is within OBB_MARGIN = 0.05 of the call's threshold: a condition on the
inputs, orders of magnitude above any libm difference, asserted by the CPU test.  Family 7 does the opposite for the axis-aligned IoUs, whose
operations are IEEE and must agree exactly: pairs found by a seeded search whose fp32 IoU, one operation at a time, *is* the call's threshold
(">" keeps the box), and pairs whose decision flips as soon as any multiply-add of the union is contracted (fma_variants)."""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import yolo_post as yp

F = np.float32
CONF = 0.5
IOU = 0.45
OBB_MARGIN = 0.05
UNSUPPORTED = 4   # TRTX_ERR_UNSUPPORTED (include/trtx_hip.h)
CLASSES = (79.0, 3.0, 0.0)

ENTRIES = {   # det: floats per record; box: what the record's first four floats are; greedy: keep_idx / keep_cnt / keep_det outputs
    "nms": dict(fn="yolo_nms", det=90, box="corner", angle=False, greedy=True, det_out=6),
    "v5": dict(fn="yolov5_nms", det=38, box="centre", angle=False, greedy=True, det_out=6),
    "v7": dict(fn="yolov7_nms", det=6, box="centre", angle=False, greedy=True, det_out=6),
    "v9": dict(fn="yolov9_nms", det=38, box="corner", angle=False, greedy=True, det_out=6),
    "obb": dict(fn="yolo_nms_obb", det=90, box="centre", angle=True, greedy=True, det_out=7),
    "g": dict(fn="yolo_postprocess_gpu", det=90, box="corner", angle=False, greedy=False, det_out=7),
    "gobb": dict(fn="yolo_postprocess_gpu_obb", det=90, box="centre", angle=True, greedy=False, det_out=8),
}
AABB = ("nms", "v5", "v7", "v9")
FAMILIES = {   # family -> the entry points that run it
    "counts": AABB + ("obb", "g", "gobb"),
    "capacity": AABB + ("obb", "g", "gobb"),
    "refusal": AABB + ("obb", "g", "gobb"),
    "class_block": AABB,
    "chains": AABB + ("obb", "g", "gobb"),
    "chains_1024": AABB,
    "ties": AABB + ("obb",),
    "gates": AABB,
    "iou_threshold": AABB + ("g",),
    "batch_workspace": AABB + ("obb", "g", "gobb"),
}
COMBOS = [(ep, fam) for fam, eps in FAMILIES.items() for ep in eps]


def is_obb(ep):
    return ENTRIES[ep]["angle"]


def b0_decides(ep):
    """whether bbox[0] is part of the canonical order (the reference's cmp() of yolov8 looks at it, yolov5's does not)"""
    return ep in ("nms", "obb")


# ------------------------------------------------------------------------------------------------------------------------ images and buffers
@dataclass
class Image:
    """one image's records in slot order, as corner boxes; header: the count written in front (None: the number of records)"""
    box: np.ndarray                 # [m, 4] float32 x1, y1, x2, y2
    conf: np.ndarray                # [m] float32
    cls: np.ndarray                 # [m] float32
    ang: np.ndarray                 # [m] float32
    header: int = None
    patches: list = field(default_factory=list)   # (slot, float index of the record, value) written into the emitted buffer
    marks: dict = field(default_factory=dict)     # name -> slot, for the conditions the CPU test asserts

    @property
    def m(self):
        return len(self.conf)


class Recs:
    def __init__(self):
        self.rows = []

    def add(self, box, conf, cls, ang=0.0):
        self.rows.append((*box, conf, cls, ang))
        return len(self.rows) - 1

    def array(self):
        return np.array(self.rows, dtype=np.float64).reshape(len(self.rows), 7)


def place(recs, total=None, g=False, order=None, header=None, marks=None):
    """recs (a Recs or an [n, 7] array of survivors) in the slot order `order` (a permutation, None: as given), a dropped record at every third
    slot while the image has fewer than `total` slots (None: as many as the pattern gives): a copy of the survivor before it - same box, same
    class - with a confidence at or below the threshold (below it for the g modes, which keep an equal one).  marks: name -> index in recs."""
    a = recs.array() if isinstance(recs, Recs) else np.asarray(recs, dtype=np.float64).reshape(-1, 7)
    n = len(a)
    order = np.arange(n) if order is None else np.asarray(order)
    total = n + n // 2 if total is None else total
    assert n <= total
    rows, where, low = [], {}, (0.3, 0.45) if g else (CONF, 0.3)
    for k, i in enumerate(order):
        if len(rows) % 3 == 2 and len(rows) + (n - k) < total:
            d = a[order[k - 1]].copy()
            d[4] = low[(len(rows) // 3) % 2]
            rows.append(d)
        where[int(i)] = len(rows)
        rows.append(a[i])
    r = np.array(rows, dtype=np.float64).reshape(len(rows), 7)
    img = Image(r[:, :4].astype(F), r[:, 4].astype(F), r[:, 5].astype(F), r[:, 6].astype(F), header)
    img.marks = {k: where[v] for k, v in (marks or {}).items()}
    return img


def to_centre(box):
    """yolov9/src/postprocess.cpp:59-62 on [..., 4] float32 corner boxes: four fp32 operations, one rounding each, the halving exact"""
    box = np.asarray(box, dtype=F)
    x1, y1, x2, y2 = (box[..., k] for k in range(4))
    two = F(2)
    return np.stack([(x1 + x2) / two, (y1 + y2) / two, x2 - x1, y2 - y1], axis=-1).astype(F)


def v9_to_centre_buffer(buf, max_out):
    """the same conversion on a decode buffer [B, 1 + max_out * 38] (every record, counted or not)"""
    buf = np.array(buf, dtype=F, copy=True)
    rec = buf[:, 1:].reshape(buf.shape[0], max_out, 38)
    rec[:, :, :4] = to_centre(rec[:, :, :4].copy())
    return buf


POISON = (-1000.0, -1000.0, 100000.0, 100000.0)


def emit(ep, images, max_out):
    """the decode buffer [B, 1 + max_out * det] of entry point ep; floats a record does not define hold a value that depends on slot and position"""
    e = ENTRIES[ep]
    det = e["det"]
    buf = np.zeros((len(images), 1 + max_out * det), dtype=F)
    for b, im in enumerate(images):
        assert im.m <= max_out, (im.m, max_out)
        rec = buf[b, 1:].reshape(max_out, det)
        rec[:] = (np.arange(max_out, dtype=F)[:, None] * F(0.25) + np.arange(det, dtype=F)[None, :] + F(1000.5))
        box = np.tile(np.array(POISON, dtype=F), (max_out, 1))
        box[:im.m] = im.box
        rec[:, :4] = box if e["box"] == "corner" else to_centre(box)
        rec[:, 4] = F(0.999)
        rec[:im.m, 4] = im.conf
        rec[:, 5] = im.cls[0] if im.m else F(3.0)
        rec[:im.m, 5] = im.cls
        if e["angle"]:
            rec[:, det - 1] = F(0.0)
            rec[:im.m, det - 1] = im.ang
        for slot, col, val in im.patches:
            rec[slot, col] = F(val)
        buf[b, 0] = im.m if im.header is None else im.header
    return buf


@dataclass
class Case:
    """one call: images, capacity and thresholds; expect_status: the status the entry point must return (0: it runs)"""
    name: str
    images: list
    max_out: int = 1000
    conf: float = CONF
    nms: float = IOU
    tie_free: bool = True
    expect_status: int = 0
    same_ws: bool = False      # the call runs on the workspace the call before it (in the family's list) left behind

    def buffer(self, ep):
        return emit(ep, self.images, self.max_out)


def oracle(ep, buf, max_out, conf, nms):
    """greedy entry points: (keep_idx [B, max_out], keep_cnt [B], keep_det [B, max_out, 6 | 7]); g modes: the output buffer [B, 1 + max_out * (7 | 8)]"""
    if ep == "nms":
        return yp.batch_nms_c(buf, max_out, conf, nms)
    if ep == "v5":
        return yp.v5_batch_nms_c(buf, max_out, conf, nms)
    if ep == "v7":   # the widening of tests/test_gpu_yolov7.py: the same six floats in 38-float records
        wide = np.zeros((buf.shape[0], 1 + max_out * 38), dtype=F)
        wide[:, 0] = buf[:, 0]
        wide[:, 1:].reshape(buf.shape[0], max_out, 38)[:, :, :6] = buf[:, 1:].reshape(buf.shape[0], max_out, 6)
        return yp.v5_batch_nms_c(wide, max_out, conf, nms)
    if ep == "v9":
        return yp.v5_batch_nms_c(v9_to_centre_buffer(buf, max_out), max_out, conf, nms)
    if ep == "obb":
        return yp.batch_nms_obb_c(buf, max_out, conf, nms)
    if ep == "g":
        return yp.gpu_postprocess_c(buf, max_out, conf, nms)
    assert ep == "gobb"
    return yp.gpu_postprocess_obb_c(buf, max_out, conf, nms)


def sort_order(ep, buf, max_out, conf=CONF):
    """per image the slots of the surviving records in the oracle's sort order: its emission order when nothing can be suppressed (no IoU
    reaches 2).  The g modes have no order of their own: "g" is ranked like "nms", "gobb" like "obb"."""
    ep = {"g": "nms", "gobb": "obb"}.get(ep, ep)
    idx, cnt, _ = oracle(ep, buf, max_out, conf, 2.0)
    return [idx[b, :cnt[b]].copy() for b in range(buf.shape[0])]


def kept_slots(ep, buf, max_out, conf, nms):
    """per image the set of slots the oracle keeps (g modes: the records whose keep flag is 1)"""
    res = oracle(ep, buf, max_out, conf, nms)
    if ENTRIES[ep]["greedy"]:
        return [set(res[0][b, :res[1][b]].tolist()) for b in range(buf.shape[0])]
    w = ENTRIES[ep]["det_out"]
    return [set(np.flatnonzero(res[b, 1:].reshape(max_out, w)[:, 6] == 1).tolist()) for b in range(buf.shape[0])]


# ------------------------------------------------------------------------------------------------------------------------ ProbIoU in float64
def probiou64(a, b):
    """ProbIoU of records (cx, cy, w, h, angle) [..., 5] in float64 (postprocess.cpp:303-355 without its float roundings)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    eps = 1e-7

    def cov(r):
        p, q = r[..., 2] ** 2 / 12.0, r[..., 3] ** 2 / 12.0
        c, s = np.cos(r[..., 4]), np.sin(r[..., 4])
        return p * c * c + q * s * s, p * s * s + q * c * c, (p - q) * c * s
    a1, b1, c1 = cov(a)
    a2, b2, c2 = cov(b)
    dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
    den = (a1 + a2) * (b1 + b2) - (c1 + c2) ** 2
    t1 = ((a1 + a2) * dy * dy + (b1 + b2) * dx * dx) / (den + eps)
    t2 = ((c1 + c2) * (-dx) * dy) / (den + eps)
    t3 = np.log(den / (4 * np.sqrt(np.maximum(a1 * b1 - c1 * c1, 0)) * np.sqrt(np.maximum(a2 * b2 - c2 * c2, 0)) + eps) + eps)
    bd = np.clip(0.25 * t1 + 0.5 * t2 + 0.5 * t3, eps, 100.0)
    return 1.0 - np.sqrt(1.0 - np.exp(-bd) + eps)


def obb_margin(ep, case):
    """the smallest |ProbIoU - threshold| over the same-class pairs of surviving records of an obb case (float64), inf without a pair"""
    buf = case.buffer(ep)
    worst = np.inf
    for b in range(buf.shape[0]):
        cnt = min(int(buf[b, 0]), case.max_out)
        rec = buf[b, 1:].reshape(case.max_out, 90)[:cnt]
        rec = rec[rec[:, 4] >= F(case.conf)]   # the g mode keeps an equal confidence: the superset
        for c in np.unique(rec[:, 5]):
            r = rec[rec[:, 5] == c][:, [0, 1, 2, 3, 89]].astype(np.float64)
            if len(r) < 2:
                continue
            p = probiou64(r[:, None, :], r[None, :, :])
            i, j = np.triu_indices(len(r), 1)
            worst = min(worst, float(np.abs(p[i, j] - case.nms).min()))
    return worst


# ------------------------------------------------------------------------------------------------------------------------ geometry
OBB_W, OBB_H, OBB_ANG = 120.0, 60.0, 0.3


@functools.lru_cache(None)
def obb_chain_step():
    """the shift along x (a multiple of 1/4) at which two OBB_W x OBB_H boxes at OBB_ANG have ProbIoU 0.6: the neighbour is suppressed with a margin
    of 0.15, the next but one (ProbIoU about 0.29) is not, with the same margin"""
    lo, hi = 0.0, 400.0
    for _ in range(60):
        mid = (lo + hi) / 2
        if probiou64([0, 0, OBB_W, OBB_H, OBB_ANG], [mid, 0, OBB_W, OBB_H, OBB_ANG]) > 0.6:
            lo = mid
        else:
            hi = mid
    return round(lo * 4) / 4


def chain_box(i, obb):
    """link i of a chain: 100 x 100 boxes shifted by 30 (IoU 70 / 130 with the neighbour, 40 / 160 with the next but one, on either side of 0.45);
    for oriented boxes obb_chain_step() apart -> (box, angle)"""
    if obb:
        c = obb_chain_step() * i
        return (c - OBB_W / 2, -OBB_H / 2, c + OBB_W / 2, OBB_H / 2), OBB_ANG
    return (30.0 * i, 0.0, 30.0 * i + 100.0, 100.0), 0.0


def filler_box(k, obb):
    """disjoint boxes far from every chain and from each other"""
    if obb:
        c = 20000.0 + 600.0 * k
        return (c - OBB_W / 2, 5000.0, c + OBB_W / 2, 5000.0 + OBB_H), 0.7
    return (20000.0 + 200.0 * k, 5000.0, 20100.0 + 200.0 * k, 5100.0), 0.0


def confs(rng, n, lo=0.55, step=0.0004):
    """n distinct confidences above the threshold, in random order"""
    return (lo + step * rng.permutation(n)).astype(F)


def clusters(rng, n, classes, obb):
    """n survivors in loose clusters, the classes descending along the slots -> [n, 7].  Axis-aligned: integer boxes of 40 .. 90 around cluster
    centres, sd 12, so that some overlap above 0.45 and some do not.  Oriented: clusters on a grid of 600, members within +-2 of the centre and
    0.01 of its angle (ProbIoU above 0.9), clusters at ProbIoU 0 of each other - nothing near the threshold."""
    a = np.zeros((n, 7))
    k = max(n // 5, 1)
    which = rng.integers(0, k, size=n)
    if obb:
        side = int(np.ceil(np.sqrt(k)))
        cx = 600.0 * (which % side) + rng.integers(-2, 3, size=n)
        cy = 600.0 * (which // side) + rng.integers(-2, 3, size=n)
        w, h = OBB_W + 2 * rng.integers(-1, 2, size=n), OBB_H + 2 * rng.integers(-1, 2, size=n)
        a[:, 6] = (0.1 + 0.37 * which) % 3.0 + 0.01 * rng.integers(-1, 2, size=n)
    else:
        centre = rng.integers(100, 3000, size=(k, 2))
        cx = centre[which, 0] + np.rint(rng.normal(0, 12, size=n))
        cy = centre[which, 1] + np.rint(rng.normal(0, 12, size=n))
        w, h = 2 * rng.integers(20, 46, size=n), 2 * rng.integers(20, 46, size=n)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    a[:, 4] = confs(rng, n)
    a[:, 5] = np.array(classes)[np.minimum(np.arange(n) * len(classes) // max(n, 1), len(classes) - 1)] if n else 0
    return a


# ------------------------------------------------------------------------------------------------------------------------ the families
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024)


def counts_image(n, ep, seed=0):
    g = not ENTRIES[ep]["greedy"]
    max_out = 1024 if n > 1000 else 1000
    rng = np.random.default_rng(1000 * seed + n)
    return place(clusters(rng, n, CLASSES, is_obb(ep)), total=min(n + n // 2, max_out), g=g), max_out


def family_counts(ep):
    out = []
    for n in COUNTS:
        img, max_out = counts_image(n, ep)
        out.append(Case(f"n{n}", [img], max_out))
    return out


CAPACITIES = (1, 7, 64, 100, 1024)


def family_capacity(ep):
    """the buffer holds exactly max_out records, all of them filled; the header says max_out + 7 in image 0 and 5000 in image 1: without the clamp
    image 0 runs into image 1's records and image 1 out of the buffer"""
    g = not ENTRIES[ep]["greedy"]
    out = []
    for mo in CAPACITIES:
        imgs = []
        for k, header in enumerate((mo + 7, 5000)):
            rng = np.random.default_rng(7000 + 10 * mo + k)
            n = mo - mo // 3
            imgs.append(place(clusters(rng, n, CLASSES, is_obb(ep)), total=mo, g=g, header=header))
            assert imgs[-1].m == mo
        out.append(Case(f"max_out{mo}", imgs, mo))
    return out


def family_refusal(ep):
    """max_out = 1025: TRTX_ERR_UNSUPPORTED, nothing is written"""
    img, _ = counts_image(65, ep)
    return [Case("max_out1025", [img], 1025, expect_status=UNSUPPORTED)]


# sorted ranks of the class-against-block image: class -> (first rank, members)
CLASS_BLOCK = {0.0: (0, 64), 3.0: (64, 1), 5.0: (65, 63), 17.0: (128, 64), 79.0: (192, 150)}


def class_block_image(ep):
    """class boundaries between ranks 63|64, 64|65 and 127|128; class 0 and class 17 have 64 members and fill blocks 0 and 2, so tile (1, 2) and
    tile (2, 3) are skipped by the class rule; class 79 has ranks 192 .. 341 over blocks 3, 4 and 5: its 128 most confident members are disjoint
    and every victim in block 5 (ranks 320 .. 341) overlaps one of the first 22 of them, in block 3, by IoU 0.82 - the even ones do, the odd ones
    are disjoint and stay"""
    rng = np.random.default_rng(31)
    parts = []
    for cls in (79.0, 17.0, 5.0, 3.0, 0.0):   # descending along the slots
        first, members = CLASS_BLOCK[cls]
        if cls == 79.0:
            a = np.zeros((members, 7))
            for j in range(members):
                if j < 128:
                    x, y = 200.0 * (j % 16), 200.0 * (j // 16)
                elif j % 2 == 0:
                    s = j - 128
                    x, y = 200.0 * (s % 16) + 10.0, 200.0 * (s // 16)
                else:
                    x, y = 200.0 * (j - 128), 4000.0
                a[j] = (x, y, x + 100.0, y + 100.0, 0.99 - 0.002 * j, cls, 0.0)
            a = a[rng.permutation(members)]
        else:
            a = clusters(rng, members, (cls,), False)
        parts.append(a)
    return place(np.concatenate(parts), total=1000)


def family_class_block(ep):
    rng = np.random.default_rng(32)
    return [Case("five_classes", [class_block_image(ep)], 1000),
            Case("one_class_of_1024", [place(clusters(rng, 1024, (3.0,), False), total=1024)], 1024)]


def chain_images(ep):
    """4 (a) - (d): name -> image, all in class 3; marks name the slots of A, B, C, D"""
    obb, g = is_obb(ep), not ENTRIES[ep]["greedy"]
    rng = np.random.default_rng(41)
    out = {}

    def link(r, i, conf):
        box, ang = chain_box(i, obb)
        return r.add(box, conf, 3.0, ang)

    def fill(r, k0, count, hi, lo):
        for k in range(count):
            box, ang = filler_box(k0 + k, obb)
            r.add(box, hi - (hi - lo) * (k + 1) / (count + 1), 3.0, ang)

    r = Recs()   # (a) A > B > C in one block: B overlaps both, C does not overlap A
    marks = dict(A=link(r, 0, 0.95), B=link(r, 1, 0.90), C=link(r, 2, 0.85))
    fill(r, 0, 4, 0.84, 0.6)
    out["a_in_block"] = place(r, g=g, order=rng.permutation(len(r.rows)), marks=marks)

    r = Recs()   # (b) the same chain at ranks 0, 71 and 136
    marks = dict(A=link(r, 0, 0.95))
    fill(r, 0, 70, 0.94, 0.91)
    marks["B"] = link(r, 1, 0.90)
    fill(r, 70, 64, 0.89, 0.81)
    marks["C"] = link(r, 2, 0.80)
    out["b_three_blocks"] = place(r, g=g, order=rng.permutation(len(r.rows)), marks=marks)

    r = Recs()   # (c) the dead suppressor: A kills B in block 0, B overlaps D in block 1, A does not overlap D
    marks = dict(A=link(r, 0, 0.95), B=link(r, 1, 0.94))
    fill(r, 0, 70, 0.93, 0.81)
    marks["D"] = link(r, 2, 0.80)
    out["c_dead_suppressor"] = place(r, g=g, order=rng.permutation(len(r.rows)), marks=marks)

    r = Recs()   # (d) 200 links, the confidence falling along the chain, the slots scrambled
    marks = {f"L{i}": link(r, i, 0.95 - 0.002 * i) for i in range(200)}
    out["d_chain_of_200"] = place(r, g=g, order=rng.permutation(200), marks=marks)
    return out


def family_chains(ep):
    return [Case(name, [img], 1000) for name, img in chain_images(ep).items()]


def family_chains_1024(ep):
    """4 (e): 1024 identical boxes with distinct confidences (one survivor, every bit of the triangle set); 1024 disjoint boxes (all survive, in
    confidence order)"""
    rng = np.random.default_rng(45)
    same, apart = np.zeros((1024, 7)), np.zeros((1024, 7))
    same[:] = (100.0, 100.0, 200.0, 200.0, 0, 3.0, 0.0)
    same[:, 4] = confs(rng, 1024, 0.5004)
    k = np.arange(1024)
    apart[:, 0], apart[:, 1] = 150.0 * (k % 32), 150.0 * (k // 32)
    apart[:, 2], apart[:, 3] = apart[:, 0] + 100.0, apart[:, 1] + 100.0
    apart[:, 4], apart[:, 5] = confs(rng, 1024, 0.5004), 3.0
    return [Case("identical", [place(same, total=1024)], 1024), Case("disjoint", [place(apart, total=1024)], 1024)]


TIED = 150


def family_ties(ep):
    """equal confidences.  The expected order is the oracle's canonical one (module docstring).  The boxes form chains (60 wide, 17 apart: IoU
    43 / 77 with the neighbour, 26 / 94 with the next), so the order also decides who survives."""
    centre = ENTRIES[ep]["box"] == "centre"
    rng = np.random.default_rng(51)

    step = 20.0 if is_obb(ep) else 17.0   # oriented 60 x 60 boxes: ProbIoU 0.61 at 20, 0.30 at 40

    def at(c, y):   # a 60 x 60 box whose bbox[0] - x1, or cx - is exactly c
        return (c - 30.0, y, c + 30.0, y + 60.0) if centre else (c, y, c + 60.0, y + 60.0)

    def other(r):   # a few records of other classes around the tied ones
        r.add(at(5000.0, 0.0), 0.9, 79.0, 0.2 if is_obb(ep) else 0.0)
        r.add(at(5000.0, 200.0), 0.6, 0.0, 0.2 if is_obb(ep) else 0.0)

    ang = 0.0
    if b0_decides(ep):
        # image 0: bbox[0] ascending decides: distinct values, 20 of them negative, slots scrambled; and three records that tie in bbox[0] as well,
        # +0.0, -0.0 and +0.0 at ascending slots (ord_f32 folds the zeros, the oracle compares them equal): the slot decides among them
        r = Recs()
        other(r)
        ids = [r.add(at(step * (k - 20), 0.0), 0.75, 3.0, ang) for k in range(TIED)]
        z1, z2 = r.add(at(0.0, 1000.0), 0.75, 3.0, ang), r.add(at(0.0, 2000.0), 0.75, 3.0, ang)
        order = rng.permutation(len(r.rows))
        pos = sorted(int(np.flatnonzero(order == i)[0]) for i in (ids[20], z1, z2))
        for p, i in zip(pos, (ids[20], z1, z2)):
            order[p] = i
        img0 = place(r, order=order, marks=dict(zero_a=ids[20], zero_minus=z1, zero_b=z2))
        img0.patches.append((img0.marks["zero_minus"], 0, -0.0))
        # image 1: full ties - equal bbox[0] too, the chain runs along y: the slot decides
        r = Recs()
        other(r)
        for k in range(TIED):
            r.add(at(300.0, step * k), 0.75, 3.0, ang)
        img1 = place(r, order=rng.permutation(len(r.rows)))
        return [Case("bbox0_then_slot", [img0, img1], 1000, tie_free=False)]
    # MODE 1 / 3: cmp() looks at the confidence alone: bbox[0] DESCENDS along the slots, and only the slot may decide
    r = Recs()
    other(r)
    for k in range(TIED):
        r.add(at(step * (TIED - k), 0.0), 0.75, 3.0, ang)
    return [Case("slot_alone", [place(r)], 1000, tie_free=False)]


def family_gates(ep):
    """the confidence gate (equal: dropped, one float step above: kept; NaN: dropped, MODE 0 only), zero-area pairs (0 / 0 is not above a
    threshold) and boxes with x2 < x1"""
    r = Recs()
    marks = dict(
        normal=r.add((100, 100, 200, 200), 0.9, 3.0),
        at_gate=r.add((100, 100, 200, 200), CONF, 3.0),                                   # would be suppressed by `normal` - or suppress, if kept
        above_gate=r.add((1000, 100, 1100, 200), float(np.nextafter(F(CONF), F(1))), 3.0),
        victim=r.add((110, 100, 210, 200), 0.6, 3.0),
        zero_a=r.add((500, 500, 500, 560), 0.8, 3.0), zero_b=r.add((500, 500, 500, 560), 0.7, 3.0),
        point_a=r.add((600, 600, 600, 600), 0.81, 3.0), point_b=r.add((600, 600, 600, 600), 0.71, 3.0),
        inv_a=r.add((760, 700, 700, 760), 0.85, 3.0), inv_b=r.add((760, 700, 700, 760), 0.65, 3.0),
        inv_over=r.add((700, 700, 760, 760), 0.62, 3.0),
        other=r.add((100, 100, 200, 200), 0.7, 79.0))
    if ep == "nms":
        marks["nan"] = r.add((100, 100, 200, 200), float("nan"), 3.0)
    a = r.array()
    order = np.argsort(-a[:, 5], kind="stable")   # classes descending along the slots
    img = place(a, order=order, marks=marks)
    return [Case("gates", [img], 1000)]


# ---- family 7: the axis-aligned IoUs at the threshold
def _iou_parts(kind, l, r):
    """the fp32 pieces of iou_xyxy (kind "xyxy": corner boxes) or iou_cxcywh (kind "cxcywh": centre boxes), one operation at a time, on [N, 4] float32
    arrays -> (overlap?, dx, dy, lw, lh, rw, rh): inter = dx * dy, union = lw * lh + rw * rh - inter"""
    l, r = np.asarray(l, dtype=F), np.asarray(r, dtype=F)
    if kind == "xyxy":
        a0, a1, a2, a3 = l[:, 0], l[:, 2], l[:, 1], l[:, 3]
        b0, b1, b2, b3 = r[:, 0], r[:, 2], r[:, 1], r[:, 3]
        lw, lh, rw, rh = l[:, 2] - l[:, 0], l[:, 3] - l[:, 1], r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    else:
        two = F(2)
        a0, a1, a2, a3 = l[:, 0] - l[:, 2] / two, l[:, 0] + l[:, 2] / two, l[:, 1] - l[:, 3] / two, l[:, 1] + l[:, 3] / two
        b0, b1, b2, b3 = r[:, 0] - r[:, 2] / two, r[:, 0] + r[:, 2] / two, r[:, 1] - r[:, 3] / two, r[:, 1] + r[:, 3] / two
        lw, lh, rw, rh = l[:, 2], l[:, 3], r[:, 2], r[:, 3]
    ib0, ib1, ib2, ib3 = np.maximum(a0, b0), np.minimum(a1, b1), np.maximum(a2, b2), np.minimum(a3, b3)
    return ~((ib2 > ib3) | (ib0 > ib1)), (ib1 - ib0).astype(F), (ib3 - ib2).astype(F), lw.astype(F), lh.astype(F), rw.astype(F), rh.astype(F)


FMA_VARIANTS = {   # name -> (the product fused into the sum of the two areas, whether inter's product is fused into the subtraction)
    "plain": ("", False), "fma_l": ("l", False), "fma_r": ("r", False), "fma_inter": ("", True), "fma_l_inter": ("l", True), "fma_r_inter": ("r", True)}


def fma_variants(kind, l, r):
    """name -> the fp32 IoU [N] with no multiply-add contracted ("plain": what the reference and the kernel compute) and with each contraction a
    compiler may choose in  union = lw * lh + rw * rh - inter:  the left or the right product fused into the sum, inter's product fused into the
    subtraction, and the two pairs that can be fused together.  A fused product is formed in float64, where it is exact."""
    ok, dx, dy, lw, lh, rw, rh = _iou_parts(kind, l, r)
    d = np.float64
    inter = (dx * dy).astype(F)
    pl, pr = (lw * lh).astype(F), (rw * rh).astype(F)
    sums = {"": (pl + pr).astype(F), "l": (lw.astype(d) * lh.astype(d) + pr.astype(d)).astype(F), "r": (pl.astype(d) + rw.astype(d) * rh.astype(d)).astype(F)}
    out = {}
    for name, (side, fused) in FMA_VARIANTS.items():
        s = sums[side]
        uni = (s.astype(d) - dx.astype(d) * dy.astype(d)).astype(F) if fused else (s - inter).astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = np.where(ok, (inter / uni).astype(F), F(0))
    return out


@functools.lru_cache(None)
def threshold_pairs(kind):
    """four pairs (l, r, nms_thresh, direction) of corner boxes for the IoU function `kind` ("xyxy", or "cxcywh" on their to_centre() form), from
    a seeded search over random overlapping boxes with full fp32 mantissas:
      "up":   every contracted variant gives MORE than the plain IoU; the threshold is the plain IoU itself, so the pair sits exactly at the
              threshold - ">" keeps the box - and any contraction suppresses it;
      "down": every contracted variant gives LESS; the threshold is the largest of them, so the plain IoU suppresses the box and any contraction
              keeps it.
    Two of each.  l is the more confident box (the kernel's and the oracle's first argument)."""
    rng = np.random.default_rng(71 if kind == "xyxy" else 72)
    N = 400000
    x1, y1 = rng.uniform(100, 900, N).astype(F), rng.uniform(100, 900, N).astype(F)
    w, h = rng.uniform(40, 160, N).astype(F), rng.uniform(40, 160, N).astype(F)
    l = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(F)
    sh = (rng.uniform(-0.25, 0.25, (N, 4)) * np.stack([w, h, w, h], axis=1)).astype(F)
    r = (l + sh).astype(F)
    a, b = (l, r) if kind == "xyxy" else (to_centre(l), to_centre(r))
    v = fma_variants(kind, a, b)
    plain = v["plain"]
    others = np.stack([v[k] for k in FMA_VARIANTS if k != "plain"])
    mid = (plain > 0.3) & (plain < 0.7)
    up, down = np.flatnonzero(mid & (others > plain).all(0)), np.flatnonzero(mid & (others < plain).all(0))
    assert len(up) >= 2 and len(down) >= 2, (kind, len(up), len(down))
    out = [(l[i], r[i], float(plain[i]), "up") for i in up[:2]] + [(l[i], r[i], float(others[:, i].max()), "down") for i in down[:2]]
    return out


def iou_kind(ep):
    return "xyxy" if ENTRIES[ep]["box"] == "corner" and ep != "v9" else "cxcywh"


def family_iou_threshold(ep):
    """one call per pair: the pair in class 3 (the more confident box first), a dropped record and two disjoint boxes of another class"""
    g = not ENTRIES[ep]["greedy"]
    out = []
    for k, (l, r, thr, direction) in enumerate(threshold_pairs(iou_kind(ep))):
        rr = Recs()
        rr.add((2000, 2000, 2100, 2100), 0.7, 79.0)
        marks = dict(first=rr.add(l.astype(np.float64), 0.9, 3.0), second=rr.add(r.astype(np.float64), 0.8, 3.0))
        rr.add((3000, 2000, 3100, 2100), 0.6, 3.0)
        out.append(Case(f"{direction}{k}", [place(rr, g=g, marks=marks)], 7, nms=thr))
    return out


def family_batch_workspace(ep):
    """a call of three images - n = 1024 (identical boxes for the axis-aligned modes: every bit of all sixteen blocks' triangle set; tight clusters
    for the oriented ones), 0 and 65 - then calls on the workspace it left behind: three small images, and one image alone"""
    g = not ENTRIES[ep]["greedy"]
    if is_obb(ep):
        big = counts_image(1024, ep, seed=8)[0]
    else:
        big = family_chains_1024(ep)[0].images[0]
    small = chain_images(ep)
    first = [big, counts_image(0, ep)[0], counts_image(65, ep, seed=8)[0]]
    second = [small["a_in_block"], counts_image(65, ep, seed=9)[0], counts_image(1, ep, seed=8)[0]]
    return [Case("b3_1024_0_65", first, 1024),
            Case("b3_small_on_used_workspace", second, 1024, same_ws=True),
            Case("b1_small_on_used_workspace", [small["c_dead_suppressor"]], 1024, same_ws=True)]


_BUILD = dict(counts=family_counts, capacity=family_capacity, refusal=family_refusal, class_block=family_class_block, chains=family_chains,
              chains_1024=family_chains_1024, ties=family_ties, gates=family_gates, iou_threshold=family_iou_threshold,
              batch_workspace=family_batch_workspace)


@functools.lru_cache(None)
def cases(ep, family):
    """the calls of one (entry point, family) of COMBOS, in order"""
    assert ep in FAMILIES[family], (ep, family)
    return _BUILD[family](ep)
