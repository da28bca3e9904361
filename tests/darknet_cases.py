"""The Darknet YoloLayer (YOLOv3 / YOLOv3-tiny / YOLOv4) for the tests: a NumPy float32 restatement of the reference's CalDetection
(yolov4/yololayer.cu:154-199, equal in yolov3 and yolov3-tiny) and the case table the decode and fused-head kernels are run on.
Not a test module (no test_ prefix); tests/test_darknet_cpu.py checks that every case reaches the edge it is there for, and
tests/test_gpu_darknet.py runs the kernels on them.

The restatement, per image, level (as passed), cell and anchor k < 3, in that order (the canonical order that replaces the reference's
atomicAdd race):
  Logist(x) = 1./(1. + exp(-x)): a float32 exp, the add and the divide in float64, rounded to float32;
  class scan with strict '>' from (0.0, class 0) - a NaN logit never wins, so max_cls_prob is never NaN;
  dropped if max_cls_prob < 0.1f || box_prob < 0.1f - a NaN box_prob passes;
  bbox[0] = (col + Logist(tx)) * net_w / grid_w, bbox[1] likewise with row, net_h, grid_h: float32, left to right;
  bbox[2] = exp(tw) * anchor_w, bbox[3] = exp(th) * anchor_h;
  record = bbox[4], det_confidence = box_prob, class_id, class_confidence = max_cls_prob: 7 floats, no product.
out[b][0] is the count clamped to max_out; floats behind a row's records keep `fill`.

All case values are fp16-representable, so the planar decode (fp32 planes), the fp32 head and the fp16 head see the same numbers and one
reference serves the three."""
import collections
import functools

import numpy as np

DET = 7
GATE = np.float32(0.1)
LOGIT_GATE = float(np.log(0.1 / 0.9))   # -2.1972: the logit whose Logist is 0.1

Net = collections.namedtuple("Net", "name grids net_w net_h anchors")
V4_ANCHORS = [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]]
TINY_ANCHORS = [[81, 82, 135, 169, 344, 319], [23, 27, 37, 58, 81, 82]]
NETS = {
    # grids are (grid_w, grid_h) per level, in the order the levels are passed
    "A": Net("A", [(5, 3), (3, 2), (1, 1)], 40, 24, V4_ANCHORS),        # 22 cells: level boundaries inside one wave's 16 cells, a one-cell level
    "B": Net("B", [(23, 23), (12, 12), (6, 6)], 184, 184, V4_ANCHORS),  # 709 cells: two 512-cell chunk counters, the chunk edge inside level 0
    "C": Net("C", [(2, 2), (4, 4)], 64, 64, TINY_ANCHORS),              # 20 cells: yolov3-tiny's two levels, coarsest first
}
CLASSES = (1, 3, 80)
BATCHES = (1, 3)


def cells_of(net):
    return sum(gw * gh for gw, gh in net.grids)


def lds_of(classes):
    """pixel strides a case runs with, as (ld, path): the dense 3 * info; where that is a multiple of 8 channels (16 bytes in fp16, 32 in fp32: the
    vector path) also the next odd stride, which takes the element path; and a padded, aligned stride (255 of 256 for 80 classes)"""
    nch = 3 * (5 + classes)
    out = [(nch, "vector" if nch % 8 == 0 else "element")]
    if nch % 8 == 0:
        out.append((nch + 1, "element"))
    out.append(((nch + 8) // 8 * 8, "vector"))
    return out


def fp16_values(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def logist(x):
    with np.errstate(over="ignore"):
        e = np.exp(-np.asarray(x, np.float32))          # float32 in, float32 out
    return (1.0 / (1.0 + e.astype(np.float64))).astype(np.float32)


def probabilities(planes, classes):
    """box_prob, max_cls_prob, class_id of every anchor in canonical order: three arrays [B, cells * 3]"""
    info = 5 + classes
    bp, mp, ci = [], [], []
    for x in planes:
        B, _, cells = x.shape
        v = x.reshape(B, 3, info, cells)
        p = logist(v[:, :, 5:])                                        # [B, 3, classes, cells]
        q = np.where(np.isnan(p), np.float32(-1), p)
        best = q.max(2)
        cls = np.where(best > 0, q.argmax(2), 0)                       # strict '>' from (0.0, class 0): the first maximum, class 0 if none is above 0
        best = np.where(best > 0, best, np.float32(0)).astype(np.float32)
        for src, dst in ((logist(v[:, :, 4]), bp), (best, mp), (cls, ci)):
            dst.append(src.transpose(0, 2, 1).reshape(B, cells * 3))   # (cell, anchor) order
    return np.concatenate(bp, 1), np.concatenate(mp, 1), np.concatenate(ci, 1)


def decode_ref(planes, classes, net, max_out, fill=0.0):
    """planes: [B, 3 * (5 + classes), cells] float32 per level -> [B, 1 + max_out * 7] float32"""
    info = 5 + classes
    B = planes[0].shape[0]
    out = np.full((B, 1 + max_out * DET), fill, np.float32)
    bp, mp, ci = probabilities(planes, classes)
    for b in range(B):
        n, g = 0, 0
        for x, (gw, gh), an in zip(planes, net.grids, net.anchors):
            cells = gw * gh
            v = x[b].reshape(3, info, cells)
            for e in range(cells):
                row, col = divmod(e, gw)
                for k in range(3):
                    box_prob, best = bp[b, g], mp[b, g]
                    g += 1
                    if best < GATE or box_prob < GATE:    # NaN compares false: kept
                        continue
                    if n < max_out:
                        with np.errstate(over="ignore", invalid="ignore"):
                            rec = out[b, 1 + n * DET:1 + (n + 1) * DET]
                            rec[0] = (np.float32(col) + logist(v[k, 0, e])) * np.float32(net.net_w) / np.float32(gw)
                            rec[1] = (np.float32(row) + logist(v[k, 1, e])) * np.float32(net.net_h) / np.float32(gh)
                            rec[2] = np.exp(v[k, 2, e]) * np.float32(an[2 * k])
                            rec[3] = np.exp(v[k, 3, e]) * np.float32(an[2 * k + 1])
                            rec[4] = box_prob
                            rec[5] = np.float32(ci[b, g - 1])
                            rec[6] = best
                    n += 1
        out[b, 0] = min(n, max_out)
    return out


def records(row):
    n = int(row[0])
    return row[1:1 + n * DET].reshape(n, DET)


# ------------------------------------------------------------------------------------------------------------------ the case table
Case = collections.namedtuple("Case", "name net classes batch planes max_out planted nan")
# planted: [(image, global anchor index in canonical order, kept, class id or None, what)]; nan: the case holds NaN logits on purpose


def off_the_gates(x):
    """moves every logit within 0.02 of the gate's logit a quarter up: no probability of a case lies within 1e-4 of 0.1 by accident"""
    return np.where(np.abs(x - LOGIT_GATE) < 0.02, x + 0.25, x)


def random_planes(net, classes, batch, seed):
    """objectness around the gate's logit, class logits shifted so that the class maximum straddles the gate too"""
    rng = np.random.default_rng(seed)
    info = 5 + classes
    shift = {1: 2.2, 3: 3.6, 80: 6.9}[classes]
    planes = []
    for gw, gh in net.grids:
        x = rng.normal(0, 2, size=(batch, 3, info, gw * gh))
        x[:, :, :4] *= 0.5
        x[:, :, 4] -= 1.5
        x[:, :, 5:] -= shift
        planes.append(fp16_values(off_the_gates(x)).reshape(batch, 3 * info, gw * gh))
    return planes


def quiet_planes(net, classes, batch, seed, obj=-9.0, cls=-9.0):
    rng = np.random.default_rng(seed)
    info = 5 + classes
    planes = []
    for gw, gh in net.grids:
        x = rng.normal(0, 0.5, size=(batch, 3, info, gw * gh))
        x[:, :, 4] = obj
        x[:, :, 5:] = cls + 0.25 * rng.normal(0, 1, size=x[:, :, 5:].shape).clip(-2, 2)
        planes.append(x)
    return planes


def anchor_index(net, level, cell, k):
    return 3 * (sum(gw * gh for gw, gh in net.grids[:level]) + cell) + k


def planted_case(net, classes, seed):
    """Image 0: the planted families at chosen (level, cell, anchor) places, among them the last cell of level 0, the first of level 1 and the
    last level's last cell.  Image 1: empty.  Image 2: random."""
    info = 5 + classes
    planes = quiet_planes(net, classes, 3, seed)
    rnd = random_planes(net, classes, 3, seed + 1)
    for x, r in zip(planes, rnd):
        x[2] = r[2].reshape(x[2].shape)
    planted = []
    last = [gw * gh - 1 for gw, gh in net.grids]
    hi_cls = classes - 1

    def plant(level, cell, k, obj, cls_values, kept, cls_id, what, box=None):
        v = planes[level][0, k]
        v[4, cell] = obj
        v[5:, cell] = -9.0
        for c, val in cls_values.items():
            v[5 + c, cell] = val
        if box is not None:
            v[box[0], cell] = box[1]
        planted.append((0, anchor_index(net, level, cell, k), kept, cls_id, what))

    up, dn = LOGIT_GATE + 0.05, LOGIT_GATE - 0.05   # probabilities 0.1045 and 0.0956
    nl = len(net.grids)
    plant(0, 0, 0, up, {0: 3.0}, True, 0, "objectness just above the gate, class well above")
    plant(0, 0, 1, dn, {0: 3.0}, False, None, "objectness just below the gate, class well above")
    plant(0, last[0], 2, 3.0, {hi_cls: up}, True, hi_cls, "class maximum just above the gate, objectness passing")
    plant(0, last[0], 0, 3.0, {hi_cls: dn}, False, None, "class maximum just below the gate, objectness passing")
    plant(1, 0, 1, dn, {0: dn}, False, None, "both below the gate")
    plant(1, 0, 2, 3.0, {0: 2.0, hi_cls: 2.0}, True, 0, "equal class logits: the lowest index")
    if classes == 80:
        plant(1, 1, 0, 3.0, {17: 2.0, 63: 2.0}, True, 17, "equal class logits in different lanes")
        plant(1, 1, 1, 3.0, {40: 2.0, 41: 2.0}, True, 40, "equal class logits inside one lane's chunk")
    plant(1, last[1] - 1, 0, np.nan, {0: 3.0}, True, 0, "NaN objectness: kept")
    plant(nl - 1, last[nl - 1], 0, 3.0, {0: 3.0, hi_cls: np.nan} if classes > 1 else {0: np.nan}, classes > 1, 0 if classes > 1 else None,
          "a NaN class logit" + (" beside a passing one: kept" if classes > 1 else " alone: the maximum stays 0.0, dropped"))
    plant(nl - 1, last[nl - 1], 1, 3.0, {0: 3.0}, True, 0, "tw = 100: an infinite width", box=(2, 100.0))
    plant(nl - 1, last[nl - 1], 2, 3.0, {0: 3.0}, True, 0, "a NaN box value", box=(1, np.nan))
    planes = [fp16_values(x).reshape(3, 3 * info, -1) for x in planes]
    return Case(f"planted-{net.name}-{classes}", net, classes, 3, planes, 3 * cells_of(net) + 5, planted, True)


def full_case(net, classes, max_out, seed):
    """every anchor of every image kept: the count is clamped to max_out and nothing is written behind record max_out - 1"""
    info = 5 + classes
    planes = quiet_planes(net, classes, 2, seed, obj=4.0, cls=-9.0)
    for x in planes:
        x[:, :, 5 + (classes - 1) // 2] = 3.0
    planes = [fp16_values(x).reshape(2, 3 * info, -1) for x in planes]
    return Case(f"full-{net.name}-{classes}-max{max_out}", net, classes, 2, planes, max_out, [], False)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    seed = 100
    for net in NETS.values():
        for classes in CLASSES:
            for batch in BATCHES:
                seed += 1
                out.append(Case(f"random-{net.name}-{classes}-b{batch}", net, classes, batch, random_planes(net, classes, batch, seed),
                                3 * cells_of(net) + 5, [], False))
    for classes in CLASSES:
        out.append(planted_case(NETS["A"], classes, 300 + classes))
    out.append(planted_case(NETS["C"], 3, 320))
    out.append(full_case(NETS["A"], 3, 40, 400))      # 66 anchors, 40 slots
    out.append(full_case(NETS["B"], 1, 1000, 401))    # 2127 anchors, 1000 slots: the cut lies in the first chunk, the count needs both
    out.append(full_case(NETS["C"], 80, 1, 402))      # max_out = 1
    p = planted_case(NETS["A"], 3, 303)
    out.append(p._replace(name="planted-A-3-max1", max_out=1))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, fill):
    """the restatement's output for a case, computed once and shared (callers must not write to it)"""
    c = {c.name: c for c in cases()}[name]
    ref = decode_ref(c.planes, c.classes, c.net, c.max_out, fill)
    ref.setflags(write=False)
    return ref


def to_nhwc(planes, grid, ld, pad=float("nan")):
    """[B, C, gh * gw] planes -> float32 [B, gh, gw, ld] with the channels beyond C holding `pad`"""
    gw, gh = grid
    B, C, _ = planes.shape
    t = np.full((B, gh, gw, ld), pad, np.float32)
    t[..., :C] = planes.reshape(B, C, gh, gw).transpose(0, 2, 3, 1)
    return t
