"""The YOLOv10 decode and top-k tables, with NumPy restatements of the reference's CalDetection (yolov10/plugin/yololayer.cu:157-198) and
get_topk / batch_topk (yolov10/src/postprocess.cpp:35-52).  Shared by tests/test_yolov10_cpu.py (every case reaches the edge it names, on
the restatement's output) and tests/test_gpu_yolov10.py (trtx_yolov10_decode, trtx_yolov10_head_decode_nhwc{,_f32}, trtx_yolov10_topk).

Decode.  Nets of one to three levels: 5 x 7 cells on one level, 3 x 3 + 1 x 1 on two, 126 cells on three with both level boundaries inside
the second wave, and 525 cells (three score workgroups, two 512-cell chunks).  Classes 80 and 8 (every logit in 16-byte pieces), 3 and 1
(the element tail only) - the head reads the first two as the YOLOv8 det head does and the last two as the task head does.  Values are
generated in fp32 and rounded to the storage type; accidental ties for a cell's maximum are broken one storage step up; padding channels
hold NaN and 60000 in turn (tests/yolo_head_cases.py's devices, reused).

The restatement runs the reference's per-cell arithmetic in fp32 (sigmoid as 1 / (1 + expf(-x)), strict '>' from (0.0, class 0), dropped when
the maximum < 0.1, (col + .5 -/+ d) * stride) and hands the slots out in canonical (level, cell) order, the count clamped to max_out: the
two documented deviations of plugins/yolo_decode.hip from the reference's atomicAdd.

What is compared how (nothing fitted):
  exact     counts, class ids, slot order, every float that must stay untouched;
  conf      2e-7: one expf, device against NumPy, and the division (yolo_head_cases.CONF_ATOL - the same arithmetic);
  boxes     planar decode: bit for bit (two fp32 operations of exact inputs, no contraction possible); fused head: the bound
            tests/test_gpu_yolo_head.py uses, yolo_head_cases.bound_of / dfl_terms on this table's bins and weights - the same DFL arithmetic;
  gate      the logits one storage step of fp16 either side of the gate (-2.197265625: p = 0.09999631, dropped; -2.1953125: p = 0.10017, kept),
            which both storage types hold exactly; fp32 tensors add float32(logit(0.1)) -/+ 16 float steps (p about 45 ulps off 0.1), nothing
            closer: a device expf and NumPy's may differ by an ulp, and one fp32 step of the logit moves p by less than that.

Top-k.  The restatement keeps conf > thresh in slot order (topk <= 0, the reference, whose argument is unused) or the topk highest of those
by a stable descending sort; everything is compared bit for bit.  trtx_yolov10_topk takes no workspace, so the issue's "non-zero workspace"
case has nothing to run on; the pre-filled output buffer is the case's other half and is here."""
import functools
from dataclasses import dataclass

import numpy as np

from tests import yolo_head_cases as hc

REC = 6
GATE = 0.1
U = hc.U
GEOMS = {   # name: (net_h, net_w, strides)
    "5x7": (40, 56, (8,)),                 # 35 cells, one level
    "3x3+1x1": (48, 48, (16, 32)),         # 9 + 1 cells
    "126": (64, 96, (8, 16, 32)),          # 96 + 24 + 6: both boundaries inside wave 1
    "525": (160, 160, (8, 16, 32)),        # 400 + 100 + 25: three score workgroups, two chunks
}
GATE16 = ((-2.197265625, False), (-2.1953125, True))
_G32 = np.float32(np.log(0.1 / 0.9))
GATE32 = GATE16 + ((hc._steps(_G32, -16), False), (hc._steps(_G32, 16), True))


def level_cells(geom):
    H, W, strides = GEOMS[geom]
    return [(H // s) * (W // s) for s in strides]


def cells_of(geom):
    return sum(level_cells(geom))


def level_offsets(geom):
    return np.concatenate([[0], np.cumsum(level_cells(geom))]).astype(int)


@dataclass(frozen=True)
class DecodeCase:
    name: str
    geom: str
    family: str
    classes: int
    B: int
    max_out: int
    seed: int = 1

    @property
    def net(self):
        return GEOMS[self.geom]

    @property
    def cells(self):
        return cells_of(self.geom)


FAMILIES = ("seeded", "empty", "full", "overflow", "gate", "ties", "naninf", "dfl")
DECODE_CASES = [
    DecodeCase("seeded_126_nc80_b2", "126", "seeded", 80, 2, 1000),
    DecodeCase("seeded_525_nc80_b3", "525", "seeded", 80, 3, 1000),
    DecodeCase("seeded_5x7_nc3_b3", "5x7", "seeded", 3, 3, 1000),
    DecodeCase("seeded_126_nc8_b1", "126", "seeded", 8, 1, 1000),
    DecodeCase("seeded_3x3+1x1_nc1_b2", "3x3+1x1", "seeded", 1, 2, 7),
    DecodeCase("empty_126_nc80_b2", "126", "empty", 80, 2, 7),
    DecodeCase("empty_5x7_nc1_b1", "5x7", "empty", 1, 1, 1),
    DecodeCase("full_126_nc8_b3", "126", "full", 8, 3, 1000),
    DecodeCase("full_3x3+1x1_nc3_b2", "3x3+1x1", "full", 3, 2, 1000),
    DecodeCase("overflow_126_nc80_b3", "126", "overflow", 80, 3, 7),
    DecodeCase("overflow_525_nc3_b2", "525", "overflow", 3, 2, 1),
    DecodeCase("overflow_5x7_nc8_b1", "5x7", "overflow", 8, 1, 7),
    DecodeCase("gate_126_nc80_b2", "126", "gate", 80, 2, 1000),
    DecodeCase("gate_5x7_nc3_b1", "5x7", "gate", 3, 1, 1000),
    DecodeCase("ties_126_nc80_b2", "126", "ties", 80, 2, 1000),
    DecodeCase("ties_5x7_nc3_b2", "5x7", "ties", 3, 2, 1000),
    DecodeCase("naninf_126_nc80_b3", "126", "naninf", 80, 3, 1000),
    DecodeCase("naninf_5x7_nc3_b2", "5x7", "naninf", 3, 2, 1000),
    DecodeCase("naninf_3x3+1x1_nc1_b1", "3x3+1x1", "naninf", 1, 1, 1000),
    DecodeCase("dfl_126_nc8_b2", "126", "dfl", 8, 2, 1000),
    DecodeCase("dfl_5x7_nc1_b3", "5x7", "dfl", 1, 3, 1000),
]
DECODE_BY_NAME = {c.name: c for c in DECODE_CASES}
DTYPES = hc.DTYPES
MEAN = {1: -4.0, 3: -4.6, 8: -5.4, 80: -6.6}   # mean of the seeded logits (std 1.5): about a tenth of the cells pass


def gates(dtype):
    return GATE16 if dtype == "f16" else GATE32


@dataclass
class Built:
    case: DecodeCase
    bins: np.ndarray      # [B, cells, 4, 16] held values
    logits: np.ndarray    # [B, cells, classes]
    dfl_w: np.ndarray     # [16]
    expect: dict


def _one(logits, b, g, cls, value=3.0, others=-30.0):
    logits[b, g, :] = others
    logits[b, g, cls % logits.shape[-1]] = value


@functools.lru_cache(maxsize=None)
def build(name, dtype):
    c = DECODE_BY_NAME[name]
    n, nc, B = c.cells, c.classes, c.B
    rng = np.random.default_rng(c.seed * 104729 + 13 * nc + n)
    bins = rng.normal(0, 1.5, size=(B, n, 4, 16)).astype(np.float32)
    logits = rng.normal(MEAN[nc], 1.5, size=(B, n, nc)).astype(np.float32)
    delib = np.zeros((B, n), bool)
    expect = {}
    w = rng.uniform(0.0, 17.0, size=16).astype(np.float32)
    fam = c.family
    if fam == "empty":
        logits -= 12.0
        expect["counts"] = [0] * B
    elif fam in ("full", "overflow"):
        for b in range(B):   # every cell passes, the class moving with the cell; the last image of an overflow case keeps its seeded logits
            if fam == "overflow" and b == B - 1 and B > 1:
                continue
            for g in range(n):
                logits[b, g, (5 * g + 3 + b) % nc] = 3.0
        if fam == "full":
            expect["counts"] = [n] * B
    elif fam == "gate":
        off = level_offsets(c.geom)
        spots = sorted({0, n - 1, min(63, n - 1), min(64, n - 1)} | {int(o) - 1 for o in off[1:]} | {int(o) for o in off[:-1]})
        placed = {}
        for b in range(B):
            for j, g in enumerate(spots):
                v, keep = gates(dtype)[(j + b) % len(gates(dtype))]
                _one(logits, b, g, 7 * j + 1, value=v)
                delib[b, g] = True
                placed[(b, g)] = (v, keep)
        expect["gate"] = placed
    elif fam == "ties":
        logits[:] = -5.0
        want = np.zeros((B, n), int)
        pairs = hc.tie_pairs(nc) or [(0, 0)]
        for g in range(n):
            lo, hi = pairs[g % len(pairs)]
            logits[:, g, lo] = 2.0
            logits[:, g, hi] = 2.0
            want[:, g] = lo
        lo, hi = pairs[0]
        logits[B - 1, 0, hi] = 2.5     # the higher index is the strict maximum
        want[B - 1, 0] = hi
        delib[:] = True
        expect["classes"] = want
    elif fam == "naninf":
        drop, nan_beside, inf, neginf = [], [], [], []
        for b, g0 in ((0, 1), (B - 1, n - 5)):
            logits[b, g0, :] = np.nan           # an all-NaN class row: the strict '>' leaves the maximum at 0.0, dropped
            drop.append((b, g0))
            if nc > 1:
                logits[b, g0 + 1, :] = np.nan   # NaN logits beside one that passes: kept with that class
                logits[b, g0 + 1, 2 % nc] = 1.0
                nan_beside.append((b, g0 + 1, 2 % nc))
            else:
                _one(logits, b, g0 + 1, 0)
            _one(logits, b, g0 + 2, 1, value=np.inf)     # +inf: p = 1
            inf.append((b, g0 + 2))
            logits[b, g0 + 3, :] = -np.inf               # -inf everywhere: p = 0, dropped
            neginf.append((b, g0 + 3))
            delib[b, g0:g0 + 4] = True
        expect.update(dropped=drop, nan_beside=nan_beside, inf=inf, neginf=neginf)
    elif fam == "dfl":
        hot = []
        for b, g0 in ((0, 2), (B - 1, n - 3)):
            for k, idx in enumerate((0, 15)):   # one-hot at bin 0 and at bin 15 on every side: the distance is dfl_w[0] / dfl_w[15]
                _one(logits, b, g0 + k, k)
                bins[b, g0 + k] = -60000.0
                bins[b, g0 + k, :, idx] = 60000.0
                hot.append((b, g0 + k, idx))
                delib[b, g0 + k] = True
        expect["onehot"] = hot
    bins, logits = hc.to_grid(bins, dtype), hc.to_grid(logits, dtype)
    hc.break_ties(logits, ~delib, dtype)
    for a in (bins, logits):
        a.setflags(write=False)
    return Built(c, bins, logits, w, expect)


# ---- the restatement of CalDetection ----------------------------------------------------------------------------------------------------
def decode_ref(levels, classes, net_h, net_w, strides, max_out):
    """levels: per level fp32 [B, 4 + classes, cells_l] -> fp32 [B, 1 + max_out * 6], zeros behind the records"""
    B = levels[0].shape[0]
    out = np.zeros((B, 1 + max_out * REC), np.float32)
    one, half = np.float32(1.0), np.float32(0.5)
    for b in range(B):
        recs = []
        for x, s in zip(levels, strides):
            gw = net_w // s
            x = np.asarray(x[b], np.float32)
            with np.errstate(all="ignore"):
                p = one / (one + np.exp(-x[4:4 + classes], dtype=np.float32))
            q = np.where(np.isnan(p), np.float32(-1.0), p)          # a NaN fails 'p > max'
            cls = np.argmax(q, 0)                                    # the first of equal maxima: strict '>'
            best = q[cls, np.arange(q.shape[1])]
            cls = np.where(best > 0, cls, 0)                         # nothing above the initial 0.0: class 0
            best = np.where(best > 0, best, np.float32(0.0)).astype(np.float32)
            keep = ~(best.astype(np.float64) < GATE)
            e = np.nonzero(keep)[0]
            row, col = (e // gw).astype(np.float32), (e % gw).astype(np.float32)
            st = np.float32(s)
            with np.errstate(all="ignore"):
                r = np.stack([((col + half) - x[0, e]) * st, ((row + half) - x[1, e]) * st, ((col + half) + x[2, e]) * st,
                              ((row + half) + x[3, e]) * st, best[e], cls[e].astype(np.float32)], 1).astype(np.float32)
            recs.append(r)
        r = np.concatenate(recs, 0)[:max_out]
        out[b, 0] = len(r)
        out[b, 1:1 + r.size] = r.ravel()
    return out


def records(dec, b):
    n = int(dec[b, 0])
    return dec[b, 1:1 + n * REC].reshape(n, REC)


def split_levels(a, geom):
    off = level_offsets(geom)
    return [np.ascontiguousarray(a[:, off[i]:off[i + 1]].transpose(0, 2, 1)) for i in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def dfl64(name, dtype):
    bt = build(name, dtype)
    return hc.dfl_terms(bt.bins, bt.dfl_w)


@functools.lru_cache(maxsize=None)
def planar(name, dtype):
    """the plugin's inputs: per level fp32 [B, 4 + classes, cells_l], the DFL done in float64 and rounded to fp32"""
    bt = build(name, dtype)
    with np.errstate(all="ignore"):
        d = dfl64(name, dtype)[0].astype(np.float32)
    return split_levels(np.concatenate([d, bt.logits], -1), bt.case.geom)


@functools.lru_cache(maxsize=None)
def reference(name, dtype, max_out=None):
    c = DECODE_BY_NAME[name]
    H, W, strides = c.net
    out = decode_ref(planar(name, dtype), c.classes, H, W, strides, c.max_out if max_out is None else max_out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kept_cells(name, dtype):
    """per image the canonical cells that pass, from the logits alone in float64"""
    bt = build(name, dtype)
    with np.errstate(all="ignore"):
        m = np.nan_to_num(bt.logits.astype(np.float64), nan=-np.inf).max(-1)
        p = 1.0 / (1.0 + np.exp(-m))
    return [np.nonzero(p[b] >= GATE)[0] for b in range(bt.case.B)]


def cell_strides(geom):
    H, W, strides = GEOMS[geom]
    return np.concatenate([np.full((H // s) * (W // s), s) for s in strides])


def box_bound(name, dtype, b, cells, ref_rows):
    """tests/yolo_head_cases.box_bound for this table's data (its non-obb form, term for term): stride (bound_d + u |d|) + 2 u |coord|"""
    bt = build(name, dtype)
    d, S, A = dfl64(name, dtype)
    bd = hc.bound_of(d, S, A, bt.dfl_w)[b][cells] + U * np.abs(d[b][cells])
    stride = cell_strides(bt.case.geom)[cells][:, None].astype(np.float64)
    return stride * bd + 2 * U * np.abs(ref_rows[:, :4].astype(np.float64))


def head_lds(case, dtype):
    """every pixel stride the class count allows on a small budget: the smallest 16-byte multiple, one vector more, three vectors more"""
    vec = hc.VEC[dtype]
    base = hc.round_up(64 + case.classes, vec)
    return (base, base + vec, base + 3 * vec)


def head_tensors(name, dtype, ld):
    """per level CPU tensors [B, cells_l, ld] of the storage type, NaN / 60000 in the padding channels"""
    bt = build(name, dtype)
    c, off = bt.case, level_offsets(bt.case.geom)
    x = np.concatenate([bt.bins.reshape(c.B, c.cells, 64), bt.logits], -1)
    return [hc.nhwc(x[:, off[i]:off[i + 1]], ld, dtype) for i in range(len(off) - 1)]


# ---- top-k ------------------------------------------------------------------------------------------------------------------------------
CAP = 1024   # the capacity of trtx_yolov7_nms, and of trtx_yolov10_topk


def topk_ref(dec, max_out, conf_thresh, topk):
    """get_topk on every row of dec [B, 1 + max_out * 6] -> the same shape, zeros behind the records.  topk <= 0: the reference."""
    out = np.zeros_like(dec)
    th = np.float32(conf_thresh)
    for b in range(dec.shape[0]):
        with np.errstate(all="ignore"):
            h = dec[b, 0]
            n = 0 if np.isnan(h) else int(min(max(h, 0), max_out))   # a header above max_out is clamped
        r = dec[b, 1:1 + n * REC].reshape(n, REC)
        with np.errstate(all="ignore"):
            r = r[r[:, 4] > th]                                      # NaN fails the '>'
        if topk > 0:
            order = np.argsort(-(r[:, 4] + np.float32(0.0)), kind="stable")   # descending conf, ties in slot order (-0.0 ties with 0.0)
            r = r[order[:topk]]
        out[b, 0] = len(r)
        out[b, 1:1 + r.size] = r.ravel()
    return out


@dataclass(frozen=True)
class TopkCase:
    name: str
    counts: tuple        # header per image
    max_out: int
    thresh: float
    topk: int
    kind: str = "seeded"   # "seeded" | "at_thresh" | "ties" | "nan"


def _tk(name, counts, max_out, thresh=0.5, topk=0, kind="seeded"):
    return TopkCase(name, tuple(counts), max_out, thresh, topk, kind)


TOPK_CASES = [
    _tk("counts_0_1", (0, 1), 7),
    _tk("counts_63_64_65", (63, 64, 65), 100),
    _tk("counts_63_64_65_top10", (63, 64, 65), 100, topk=10),
    _tk("count_1000", (1000, 999), 1000),
    _tk("count_1000_top300", (1000, 3), 1000, topk=300),
    _tk("capacity_1024", (1024, 1023), CAP),
    _tk("capacity_1024_top1", (1024, 1024), CAP, topk=1),
    _tk("header_above_max_out", (1030, 9, 8), 8, thresh=-1.0),
    _tk("header_above_max_out_top5", (5000, 8), 8, thresh=-1.0, topk=5),
    _tk("at_thresh", (40, 40), 64, kind="at_thresh"),
    _tk("at_thresh_top3", (40, 40), 64, topk=3, kind="at_thresh"),
    _tk("ties_across_the_cut", (50, 50), 64, thresh=0.2, topk=7, kind="ties"),
    _tk("topk_equals_survivors", (30,), 64, thresh=-1.0, topk=30),
    _tk("topk_one_below_survivors", (30,), 64, thresh=-1.0, topk=29),
    _tk("topk_above_survivors", (30,), 64, thresh=-1.0, topk=31),
    _tk("topk_negative", (30,), 64, topk=-3),
    _tk("nan_conf", (20, 20), 32, kind="nan"),
    _tk("nan_conf_top4", (20, 20), 32, topk=4, kind="nan"),
    _tk("max_out_1", (1, 0, 7), 1, thresh=-1.0, topk=1),
]
TOPK_BY_NAME = {c.name: c for c in TOPK_CASES}


@functools.lru_cache(maxsize=None)
def topk_input(name):
    """[B, 1 + max_out * 6]: seeded records in every slot of the buffer (so a header above the count of real ones still reads numbers)"""
    c = TOPK_BY_NAME[name]
    B = len(c.counts)
    rng = np.random.default_rng(sum(map(ord, name)))
    dec = np.zeros((B, 1 + c.max_out * REC), np.float32)
    for b in range(B):
        r = rng.uniform(0, 640, size=(c.max_out, REC)).astype(np.float32)
        r[:, 4] = rng.uniform(0.05, 0.99, size=c.max_out).astype(np.float32)
        r[:, 5] = rng.integers(0, 80, size=c.max_out).astype(np.float32)
        n = min(c.counts[b], c.max_out)
        th = np.float32(c.thresh)
        if c.kind == "at_thresh" and n >= 6:
            r[1, 4] = th                                   # exactly at the threshold: dropped
            r[3, 4] = np.nextafter(th, np.float32(1))      # one ulp above: kept
            r[5, 4] = np.nextafter(th, np.float32(0))      # one ulp below: dropped
        if c.kind == "ties" and n >= 20:
            r[:n, 4] = np.float32(0.3)                     # everything ties ...
            r[2:n:5, 4] = np.float32(0.9)                  # ... but every fifth, which ties among itself: the cut falls inside a tie
            r[4, 4] = np.float32(0.1)                      # below the threshold
        if c.kind == "nan" and n >= 8:
            r[0, 4] = np.nan
            r[7, 4] = np.nan
            r[n - 1, 4] = np.nan
            r[3, 4] = np.float32(-0.0)
        dec[b, 0] = c.counts[b]
        dec[b, 1:] = r.ravel()
    dec.setflags(write=False)
    return dec
