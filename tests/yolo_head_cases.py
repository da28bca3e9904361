"""The fused YOLOv8 / YOLO11 head table: single calls of plugins/yolo_decode.hip's head_score<T, TAIL> and its two emit passes through
trtx_yolo_head_decode_nhwc{,_f32} (det head, classes % 8 == 0) and trtx_yolo_task_head_decode_nhwc{,_f32} (task head, any class count, one
of seg / pose / obb), shared by tests/test_yolo_head_cases_cpu.py (the table and its reference, without a GPU) and
tests/test_gpu_yolo_head.py (the kernels through the C ABI).

Geometry.  The score kernel runs 256 cells per workgroup, 64 per wave; a wave reads the logits of its 64 cells in consecutive 16-byte pieces
through cell_ptr(g0 + c), so a level boundary inside a wave changes the base pointer, the cell count and the stride in the middle of one
load instruction.  Two score workgroups feed one 512-cell counter; the emit pass runs 512 cells per workgroup.  GEOMS holds the smallest
nets that reach each of those: 126 cells (one workgroup, a partly filled second wave, both boundaries inside a wave), 525 (three score
workgroups, two counters, the chunk boundary inside level 2), 340 (four levels, level 0 fills workgroup 0), 85 (a one-cell level behind a
2 x 2 one), 41 (odd counts, two levels, not square).

Data.  Everything is generated in fp32, rounded to the storage type of the engine (the values the tensors hold), and then the largest logit
of every cell that was not built on purpose is moved one storage step up where it ties with another: no pair of logits ties by accident.
Padding channels hold NaN and 60000 in turn (PAD): read by an argmax or a maximum they would win.  The DFL weights are seeded, in [-2, 17]
with one negative; one case keeps arange(16).

Reference.  The four box channels are softmax(bins) . dfl_w in torch float64 from the held values, rounded to fp32, and go with the logits
and the branch channels through the project's C restatement of CalDetection (oracle.yolo_post.decode_c / decode_ex_c).

Error model (nothing fitted; u = 2^-24, the relative error of one fp32 rounding).
  exact:  out[b][0], the slot order, class ids, seg coefficients, the -1 pattern of keypoints, every float the head does not own.
  conf:   |p - p_ref| <= 2e-7 - one expf, device against glibc, and the division; about 3 ulps below 1 (the suite's figure for it).
  a DFL distance d = sum_i e_i w_i / sum_i e_i, e_i = expf(t_i), t_i = x_i - max, p_i = e_i / sum e:
    * t_i is one fp32 subtraction of fp32 values: relative u, so the logarithm of e_i moves by u |t_i|;
    * expf: 1 ulp = 2u relative (EXP_ULP; "HIP math API", single precision floating-point functions, the table's maximum ulp error for
      expf - the same figure OpenCL's OCML backs it with); to first order d moves by sum_i p_i eta_i (w_i - d), |eta_i| <= u (|t_i| + 2 EXP_ULP):
          A = sum_i p_i (|t_i| + 2 EXP_ULP) (|w_i| + |d|)
    * the sequential fp32 sum of 16 terms: 15 roundings, each relative to a partial sum <= the total: 15 u |d|;
    * the fmaf chain over dfl_w: 16 roundings of partial sums bounded by S = sum_i p_i |w_i|: 16 u S;
    * the fp16 path divides once (u |d| <= u S); the fp32 path takes a reciprocal and multiplies every e_i by it (2 u S): 2 u S covers both;
    * e_i below the smallest normal fp32 (t_i < -87.3) may be flushed: 16 * 2^-126 * max|w|, absolute (ABS_FLUSH);
    * second order terms: the whole is raised by 1e-3 of itself.
          bound_d = u (A + 18 S + 15 |d|) (1 + 1e-3) + ABS_FLUSH
    The reference's own d is the float64 value rounded to fp32: u |d| more.
  a box coordinate (col + 0.5 -+ d) * stride: col + 0.5 is exact, the sum is rounded once in the kernel and once in the oracle, and every
    stride of the table is a power of two, so the product is exact (the table asserts it):
          bound = stride (bound_d + u |d|) + 2 u |coord|
  obb: w = (d0 + d2) * stride has two such distances and one rounding each side: stride (b0 + b2 + u (|d0| + |d2|)) + 2 u |w| (h alike);
    the centre rotates xf = (d2 - d0) / 2, yf = (d3 - d1) / 2 by the angle in double and rounds once: with e_x = (b0 + b2) / 2 + u |d0| + u |d2|
    (e_y alike) and the angle's own error da = pi * 2e-7 (its sigmoid is a conf):
          stride (e_x + e_y + da (|xf| + |yf|)) + 2 u |centre|
  keypoints and the angle keep the tolerances of tests/test_gpu_yolo11_tasks.py: rtol 1e-6 / atol 1e-4 (x and y are one double expression
    of exact inputs rounded once - they come out bit-equal; the confidence is a sigmoid) and rtol 1e-6 / atol 1e-7."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from oracle import yolo_post as yp

U = 2.0 ** -24
EXP_ULP = 1.0
CONF_ATOL = 2e-7
GATE = 0.1
PAD = (float("nan"), 60000.0)
DET = yp.DET_FLOATS
KPT_CONF = 0.5

GEOMS = {   # name: (net_h, net_w, strides)
    "64x96": (64, 96, (8, 16, 32)),
    "160x160": (160, 160, (8, 16, 32)),
    "128x128": (128, 128, (8, 16, 32, 64)),
    "64x64": (64, 64, (8, 16, 32, 64)),
    "40x56": (40, 56, (8, 16)),
}
CELLS = {"64x96": 126, "160x160": 525, "128x128": 340, "64x64": 85, "40x56": 41}
FAMILIES = ("seeded", "overflow", "full", "threshold", "ties", "naninf", "dfl")
EXTRA = {"seg": lambda nk: 32, "pose": lambda nk: 3 * nk, "obb": lambda nk: 1}
# mean of the seeded class logits (std 1.5): a few per cent of the cells pass the gate; on the nets below 130 cells about a tenth, where a
# few per cent would be fewer than the three records per image the seeded family asks for
MEAN = {1: -5.0, 8: -6.0, 13: -6.2, 15: -6.5, 80: -7.2}
SMALL_NET_SHIFT = 0.6

# (c) the two-phase pre-filter of head_score: 'm > -2.3f' flags a cell, the exact sigmoid scan settles it.  (value, flagged, kept)
THRESH16 = (
    (-2.302734375, False, False),
    (-2.30078125, False, False),
    (-2.298828125, True, False),
    (-2.19921875, True, False),
    (-2.197265625, True, False),      # p = 0.09999631
    (-2.1953125, True, True),         # p = 0.10017
)
LOGIT_GATE32 = np.float32(np.log(0.1 / 0.9))


def _steps(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return float(x)


# fp32 only: 16 float steps either side of float32(logit(0.1)): p about 45 ulps of 0.1 below / above the gate - nothing closer, a device
# expf and glibc's may differ by an ulp
THRESH32 = THRESH16 + ((_steps(LOGIT_GATE32, -16), True, False), (_steps(LOGIT_GATE32, 16), True, True))


def thresholds(dtype):
    return THRESH16 if dtype == "f16" else THRESH32


@dataclass(frozen=True)
class HeadCase:
    name: str
    geom: str
    head: str            # "det" | "task"
    family: str
    classes: int
    B: int
    task: str = ""       # "" | "seg" | "pose" | "obb"
    nk: int = 17
    seed: int = 0
    max_out: int = 0     # 0: cells + 1
    dfl: str = "seeded"  # "seeded" | "arange"
    layouts: tuple = (("pad", "pad"),)   # (head stride, branch stride): "pad" | "exact", "pad" | "exact" | "odd"

    @property
    def net(self):
        return GEOMS[self.geom]

    @property
    def cells(self):
        return CELLS[self.geom]

    @property
    def mo(self):
        return self.max_out or self.cells + 1

    @property
    def extra(self):
        return EXTRA[self.task](self.nk) if self.task else 0

    @property
    def flags(self):
        return {self.task: True} if self.task else {}

    @property
    def kpt_conf(self):
        return KPT_CONF if self.task == "pose" else 0.0


def level_cells(geom):
    H, W, strides = GEOMS[geom]
    return [(H // s) * (W // s) for s in strides]


def level_offsets(geom):
    return np.concatenate([[0], np.cumsum(level_cells(geom))]).astype(int)


def positions(geom):
    """The cells where a wave-cooperative read or a compaction can go wrong, by kind: first and last lane of a wave (the last cell of the net
    where no wave is full), the last cell of a level, the first cell of the next"""
    off, n = level_offsets(geom), CELLS[geom]
    return {
        "lane0": [g for g in range(0, n, 64)],
        "lane63": [g for g in range(63, n, 64)] or [n - 1],
        "level_last": [int(o) - 1 for o in off[1:-1]],
        "level_first": [int(o) for o in off[1:-1]],
    }


KINDS = ("lane0", "lane63", "level_last", "level_first")


def tie_pairs(classes):
    """(lower, higher) class pairs that tie for the maximum: the first and the last class, two neighbours inside one 16-byte piece, two
    different pieces; with an element tail (classes % 8) also the last full piece against the tail, and two inside the tail"""
    if classes < 2:
        return []
    full = classes & ~7
    pairs = [(0, classes - 1)]
    a = min((classes // 2) & ~7, classes - 2)
    pairs.append((a + 1, a + 2) if a + 2 < min(classes, (a & ~7) + 8) else (a, a + 1))
    if classes > 8:
        pairs.append((17 if classes >= 32 else 1, ((classes - 1) & ~7) + ((classes - 1) % 8) // 2))
    if classes % 8 and full:
        pairs.append((full - 1, full))
        if classes - full >= 2:
            pairs.append((full, classes - 1))
    return pairs


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
CASES = []


def add(**kw):
    c = HeadCase(**kw)
    assert all(o.name != c.name for o in CASES), c.name
    CASES.append(c)


_DET_CLASSES = (80, 8)
_TASKS = (("seg", 13, 17), ("pose", 1, 17), ("obb", 15, 17), ("seg", 80, 17), ("pose", 8, 5), ("obb", 80, 17), ("pose", 13, 5))
_SEEDED_LAYOUTS = (("pad", "pad"), ("exact", "exact"), ("pad", "odd"))
# seeds: fixed here so that the reference meets the conditions tests/test_yolo_head_cases_cpu.py asserts (counts, distances from the gate,
# from the box edges and from kpt_conf); a case that misses one gets another seed, never a looser condition
SEEDS = {"pose_64x96_seeded_nc1_nk17": 3,   # seeds 1 and 2: a keypoint 0.007 / 0.004 px from an edge of its box
         "obb_40x56_seeded_nc15": 3}        # seeds 1 and 2: two records on image 1

for gi, geom in enumerate(GEOMS):
    for fi, fam in enumerate(FAMILIES):
        B = 3 if fam in ("overflow", "full", "threshold") else 2
        mo = {"64x96": 40}.get(geom, CELLS[geom] // 3) if fam == "overflow" else 0
        nc = _DET_CLASSES[(gi + fi) % 2]
        name = f"det_{geom}_{fam}_nc{nc}"
        add(name=name, geom=geom, head="det", family=fam, classes=nc, B=B, seed=SEEDS.get(name, 1), max_out=mo,
            layouts=_SEEDED_LAYOUTS[:2] if fam == "seeded" else (("pad", "pad"),))
        task, tc, nk = _TASKS[(gi + 2 * fi) % len(_TASKS)]
        if fam == "ties" and tc == 1:
            task, tc, nk = "seg", 13, 17
        name = f"{task}_{geom}_{fam}_nc{tc}" + (f"_nk{nk}" if task == "pose" else "")
        add(name=name, geom=geom, head="task", family=fam, classes=tc, B=B, task=task, nk=nk, seed=SEEDS.get(name, 1), max_out=mo,
            layouts=_SEEDED_LAYOUTS if fam == "seeded" else (("pad", "pad"),))
# (g) every task branch on the small nets, seeded: seg through the vector and the element path, pose with 17 and 5 keypoints, obb; 13 classes
# put five logits into the element tail; and the det head with both class counts on the two nets the planar plugin kernel also runs on
for geom, task, tc, nk in (("64x96", "seg", 13, 17), ("64x96", "pose", 1, 17), ("64x96", "pose", 8, 5), ("64x96", "obb", 15, 17), ("64x96", "seg", 80, 17),
                           ("160x160", "seg", 80, 17), ("160x160", "pose", 1, 5), ("160x160", "obb", 15, 17), ("160x160", "pose", 13, 17),
                           ("40x56", "seg", 13, 17), ("40x56", "pose", 1, 17), ("40x56", "obb", 15, 17), ("64x64", "obb", 80, 17), ("128x128", "pose", 13, 17)):
    name = f"{task}_{geom}_seeded_nc{tc}" + (f"_nk{nk}" if task == "pose" else "")
    if all(o.name != name for o in CASES):
        add(name=name, geom=geom, head="task", family="seeded", classes=tc, B=2, task=task, nk=nk, seed=SEEDS.get(name, 1), layouts=_SEEDED_LAYOUTS)
for geom in ("64x96", "160x160"):
    for nc in _DET_CLASSES:
        name = f"det_{geom}_seeded_nc{nc}"
        if all(o.name != name for o in CASES):
            add(name=name, geom=geom, head="det", family="seeded", classes=nc, B=2, seed=SEEDS.get(name, 1), layouts=_SEEDED_LAYOUTS[:2])
add(name="det_64x96_seeded_nc80_arange", geom="64x96", head="det", family="seeded", classes=80, B=2, seed=1, dfl="arange")

BY_NAME = {c.name: c for c in CASES}
DTYPES = ("f16", "f32")
TORCH = {"f16": torch.float16, "f32": torch.float32}
VEC = {"f16": 8, "f32": 4}


# ---- data --------------------------------------------------------------------------------------------------------------------------------------
def to_grid(a, dtype):
    """the values a tensor of the engine's storage type holds"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH[dtype]).float().numpy()


def step_up(v, dtype):
    if dtype == "f32":
        return np.nextafter(v.astype(np.float32), np.float32(np.inf), dtype=np.float32)
    h = v.astype(np.float16)
    return np.nextafter(h, np.float16(np.inf)).astype(np.float32)


def break_ties(logits, free, dtype):
    """logits [B, cells, classes]; where the maximum of a `free` cell is held twice, the first holder moves one storage step up (again, if
    that made a new tie - it cannot, the maximum was the largest value)"""
    mx = np.where(np.isnan(logits), -np.inf, logits).max(-1, keepdims=True)
    tied = ((logits == mx).sum(-1) > 1) & free
    for b, g in zip(*np.nonzero(tied)):
        c = int(np.argmax(logits[b, g]))
        logits[b, g, c] = step_up(logits[b, g, c:c + 1], dtype)[0]
    return int(tied.sum())


@dataclass
class Built:
    case: HeadCase
    dtype: str
    bins: np.ndarray      # [B, cells, 4, 16] the held values, all levels in canonical cell order
    logits: np.ndarray    # [B, cells, classes]
    branch: np.ndarray    # [B, cells, extra] or None
    dfl_w: np.ndarray     # [16] fp32
    delib: np.ndarray     # [B, cells] bool: cells built on purpose (ties, values at the gate, NaN)
    expect: dict          # what the family promises, by name


def _dfl_weights(case):
    if case.dfl == "arange":
        return np.arange(16, dtype=np.float32)
    rng = np.random.default_rng(1000 + case.seed + 7 * case.classes + CELLS[case.geom])
    w = rng.uniform(-2.0, 17.0, size=16)
    k = int(rng.integers(0, 16))
    w[w < 0] *= -1
    w[k] = -abs(rng.uniform(0.5, 2.0))
    return w.astype(np.float32)


def _pass_cell(logits, b, g, cls, value=3.0, others=-30.0):
    logits[b, g, :] = others
    logits[b, g, cls % logits.shape[-1]] = value


@functools.lru_cache(maxsize=None)
def build(name, dtype):
    case = BY_NAME[name]
    n, nc, B = case.cells, case.classes, case.B
    rng = np.random.default_rng(case.seed * 7919 + 17 * nc + n + (31 if case.task else 0))
    mean = MEAN[nc] + (SMALL_NET_SHIFT if n < 130 else 0.0)
    bins = rng.normal(0, 1.5, size=(B, n, 4, 16)).astype(np.float32)
    logits = rng.normal(mean, 1.5, size=(B, n, nc)).astype(np.float32)
    branch = None
    if case.task == "seg":
        branch = rng.normal(0, 1.0, size=(B, n, 32))
    elif case.task == "pose":
        branch = rng.normal(0, 1.5, size=(B, n, 3 * case.nk))
        branch[..., 2::3] = rng.normal(0.5, 2.0, size=(B, n, case.nk))
    elif case.task == "obb":
        branch = rng.normal(0, 2.0, size=(B, n, 1))
    delib = np.zeros((B, n), bool)
    expect = {}
    fam = case.family
    if fam in ("overflow", "full"):
        # image 0 seeded, image 1 nothing passes, image 2 every cell passes (one class per cell at 3.0, the class moving with the cell)
        logits[1] -= 8.0
        for g in range(n):
            logits[2, g, (5 * g + 3) % nc] = 3.0
        expect["counts"] = {1: 0, 2: min(n, case.mo)}
    elif fam == "threshold":
        pos, th = positions(case.geom), thresholds(dtype)
        gi = list(GEOMS).index(case.geom)
        placed = {}
        for b in range(B):
            for j, (v, _, kept) in enumerate(th):
                lst = pos[KINDS[(j + b + gi) % 4]]
                free = [g for t in range(len(lst)) for g in [lst[(j + t) % len(lst)]] if (b, g) not in placed]
                if free:   # a small net has fewer such cells than values: the other images and nets take them (the CPU test counts)
                    placed[(b, free[0])] = j
        for (b, g), j in placed.items():
            _pass_cell(logits, b, g, 7 * j + 3, value=th[j][0])
            delib[b, g] = True
        expect["gate"] = {k: th[j] for k, j in placed.items()}
    elif fam == "ties":
        pairs = tie_pairs(nc)
        logits[:] = -5.0
        want = np.zeros((B, n), int)
        for g in range(n):
            lo, hi = pairs[g % len(pairs)]
            logits[:, g, lo] = 2.0
            logits[:, g, hi] = 2.0
            want[:, g] = lo
        lo, hi = pairs[0]
        logits[1, 0, hi] = 2.5     # image 1, cell 0: the higher index is the strict maximum
        want[1, 0] = hi
        delib[:] = True
        expect["classes"] = want
        expect["counts"] = {b: n for b in range(B)}
    elif fam == "naninf":
        drop, nanbox, inf = [], [], []
        for b, g0 in ((0, 5), (B - 1, n - 5)):
            logits[b, g0, :] = np.nan           # NaN logits around one that passes
            logits[b, g0, 33 % nc] = 1.0
            logits[b, g0 + 1, :] = np.nan       # NaN only: dropped
            drop.append((b, g0 + 1))
            _pass_cell(logits, b, g0 + 2, 2, value=np.inf)
            inf.append((b, g0 + 2))
            _pass_cell(logits, b, g0 + 3, 70)   # a NaN DFL bin in a passing cell: the record is emitted, that side is NaN
            bins[b, g0 + 3, 1, 4] = np.nan
            nanbox.append((b, g0 + 3))
            delib[b, g0:g0 + 4] = True
        expect.update(dropped=drop, nanbox=nanbox, inf=inf)
    elif fam == "dfl":
        eq, hot, wide = [], [], []
        for b, g0 in ((0, 7), (B - 1, n - 4)):
            _pass_cell(logits, b, g0, 2)
            bins[b, g0] = 0.25                        # all-equal bins: mean(dfl_w) on every side
            eq.append((b, g0))
            _pass_cell(logits, b, g0 + 1, 70)
            bins[b, g0 + 1] = -60000.0
            for s, i in enumerate((3, 15, 0, 9)):     # one-hot: dfl_w[i]
                bins[b, g0 + 1, s, i] = 60000.0
            hot.append((b, g0 + 1))
            _pass_cell(logits, b, g0 + 2, 5)
            bins[b, g0 + 2, 0] = -7.0 * np.arange(16)         # spans 105 > 88: expf underflows on the far bins
            bins[b, g0 + 2, 1] = -7.0 * np.arange(16)[::-1]
            bins[b, g0 + 2, 2] = np.where(np.arange(16) % 2, -100.0, 0.5)
            bins[b, g0 + 2, 3] = np.where(np.arange(16) < 2, 40.0, -60.0)
            wide.append((b, g0 + 2))
            delib[b, g0:g0 + 3] = True
        expect.update(equal=eq, onehot=hot, onehot_bins=(3, 15, 0, 9), wide=wide)
    bins, logits = to_grid(bins, dtype), to_grid(logits, dtype)
    if branch is not None:
        branch = to_grid(branch, dtype)
    expect["ties_broken"] = break_ties(logits, ~delib, dtype)
    for a in (bins, logits, branch, delib):
        if a is not None:
            a.setflags(write=False)
    return Built(case, dtype, bins, logits, branch, _dfl_weights(case), delib, expect)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
def dfl_terms(bins, w):
    """bins [..., 16] (held values), w [16] -> (d, S, A) float64: the distance, sum p |w| and the first-order expf term of the error model"""
    x = torch.from_numpy(np.asarray(bins, dtype=np.float64))
    w = torch.from_numpy(np.asarray(w, dtype=np.float64))
    p = x.softmax(-1)
    d = (p * w).sum(-1)
    t = (x - x.max(-1, keepdim=True).values).abs()
    S = (p * w.abs()).sum(-1)
    # p_i |t_i|: a bin that underflowed to 0 in float64 too has p = 0 and |t| finite
    A = (p * (t + 2 * EXP_ULP) * (w.abs() + d.abs()[..., None])).sum(-1)
    return d.numpy(), S.numpy(), A.numpy()


def bound_of(d, S, A, w):
    return U * (A + 18 * S + 15 * np.abs(d)) * (1 + 1e-3) + 16 * 2.0 ** -126 * float(np.abs(w).max())


@functools.lru_cache(maxsize=None)
def dfl64(name, dtype):
    """dfl_terms of a case: float64 [B, cells, 4] each"""
    bt = build(name, dtype)
    return dfl_terms(bt.bins, bt.dfl_w)


def bound_d(name, dtype):
    return bound_of(*dfl64(name, dtype), build(name, dtype).dfl_w)


def coord_bound(bd, d, stride, coord):
    """a corner coordinate's bound from its distance's: bd, d, stride, coord broadcast"""
    return stride * (bd + U * np.abs(d)) + 2 * U * np.abs(coord)


def split_levels(a, geom):
    """[B, cells, C] in canonical order -> per level [B, C, cells_l] (the plugin's planar layout)"""
    off = level_offsets(geom)
    return [np.ascontiguousarray(a[:, off[i]:off[i + 1]].transpose(0, 2, 1)) for i in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def planar(name, dtype):
    """the oracle's / the planar plugin kernel's inputs: [B, 4 + classes + extra, cells_l] per level, the DFL done in float64"""
    bt = build(name, dtype)
    d = dfl64(name, dtype)[0].astype(np.float32)
    parts = [d, bt.logits] + ([bt.branch] if bt.branch is not None else [])
    return split_levels(np.concatenate(parts, -1), bt.case.geom)


@functools.lru_cache(maxsize=None)
def reference(name, dtype, max_out=None):
    c = BY_NAME[name]
    H, W, strides = c.net
    mo = c.mo if max_out is None else max_out
    with np.errstate(all="ignore"):
        if c.task:
            out = yp.decode_ex_c(planar(name, dtype), c.classes, H, W, list(strides), mo, nk=c.nk, kpt_conf=c.kpt_conf, **c.flags)
        else:
            out = yp.decode_c(planar(name, dtype), c.classes, H, W, list(strides), mo)
    out.setflags(write=False)
    return out


def records(dec, b):
    n = int(dec[b, 0])
    return dec[b, 1:1 + n * DET].reshape(n, DET)


@functools.lru_cache(maxsize=None)
def kept_cells(name, dtype):
    """per image the canonical cells that pass the gate, from the logits alone (fp64 sigmoid of the largest logit; the CPU test holds every
    probability off the gate by more than expf's error, and asserts that this agrees with the oracle's counts)"""
    bt = build(name, dtype)
    with np.errstate(all="ignore"):
        m = np.nan_to_num(bt.logits.astype(np.float64), nan=-np.inf).max(-1)
        p = 1.0 / (1.0 + np.exp(-m))
    return [np.nonzero(p[b] >= GATE)[0] for b in range(bt.case.B)]


def cell_geometry(geom):
    """(row, col, stride) of every canonical cell"""
    H, W, strides = GEOMS[geom]
    row, col, st = [], [], []
    for s in strides:
        gh, gw = H // s, W // s
        e = np.arange(gh * gw)
        row.append(e // gw)
        col.append(e % gw)
        st.append(np.full(gh * gw, s))
    return np.concatenate(row), np.concatenate(col), np.concatenate(st)


def box_bound(name, dtype, b, cells, ref_rows):
    """[len(cells), 4] bound of floats 0..3 of image b's records at canonical `cells`, next to the reference's rows (|coord| terms)"""
    c = BY_NAME[name]
    d, _, _ = dfl64(name, dtype)
    d = d[b][cells]
    bd = bound_d(name, dtype)[b][cells] + U * np.abs(d)     # the reference's fp32 rounding of d
    stride = cell_geometry(c.geom)[2][cells][:, None].astype(np.float64)
    R = np.abs(ref_rows[:, :4].astype(np.float64))
    if c.task != "obb":
        return stride * bd + 2 * U * R
    ex = (bd[:, 0] + bd[:, 2]) / 2
    ey = (bd[:, 1] + bd[:, 3]) / 2
    xf, yf = np.abs(d[:, 2] - d[:, 0]) / 2, np.abs(d[:, 3] - d[:, 1]) / 2
    da = np.pi * CONF_ATOL
    ctr = stride[:, 0] * (ex + ey + da * (xf + yf))
    out = np.empty((len(cells), 4))
    out[:, 0] = ctr + 2 * U * R[:, 0]
    out[:, 1] = ctr + 2 * U * R[:, 1]
    out[:, 2] = stride[:, 0] * (bd[:, 0] + bd[:, 2]) + 2 * U * R[:, 2]
    out[:, 3] = stride[:, 0] * (bd[:, 1] + bd[:, 3]) + 2 * U * R[:, 3]
    return out


def owned(case):
    """which of a record's 90 floats the head writes"""
    m = np.zeros(DET, bool)
    m[:6] = True
    if case.task == "seg":
        m[6:38] = True
    elif case.task == "pose":
        m[38:38 + 3 * case.nk] = True
    elif case.task == "obb":
        m[DET - 1] = True
    return m


# ---- fp32 restatements of the kernel's two DFL orders (NumPy; fmaf as an exact float64 product and sum rounded once to fp32) --------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def dfl_restated(bins, w, order):
    """bins [..., 16] fp32, w [16] fp32 -> fp32 distances; order "div": acc / sum (fp16 engines), "inv": fmaf(ex * (1 / sum), w, acc) (fp32)"""
    x = bins.astype(np.float32)
    with np.errstate(all="ignore"):
        mx = np.fmax.reduce(x, -1, keepdims=True)
        ex = np.exp((x - mx).astype(np.float32), dtype=np.float32)
        s = np.zeros(x.shape[:-1], np.float32)
        acc = np.zeros(x.shape[:-1], np.float32)
        if order == "div":
            for i in range(16):
                s = (s + ex[..., i]).astype(np.float32)
                acc = _fma(ex[..., i], np.broadcast_to(w[i], s.shape), acc)
            return (acc / s).astype(np.float32)
        for i in range(16):
            s = (s + ex[..., i]).astype(np.float32)
        inv = (np.float32(1.0) / s).astype(np.float32)
        for i in range(16):
            acc = _fma((ex[..., i] * inv).astype(np.float32), np.broadcast_to(w[i], s.shape), acc)
        return acc


# ---- device layout ------------------------------------------------------------------------------------------------------------------------------
def round_up(n, m):
    return -(-n // m) * m


def head_ld(case, dtype, mode):
    vec = VEC[dtype]
    return round_up(64 + case.classes, vec) + (vec if mode == "pad" else 0)


def branch_ld(case, dtype, mode):
    vec, e = VEC[dtype], case.extra
    if mode == "odd":
        return e + (1 if e % 2 == 0 else 2)
    return round_up(e, vec) + (vec if mode == "pad" else 0)


def nhwc(a, ld, dtype):
    """[B, cells_l, C] -> a torch tensor [B, cells_l, ld] of the storage type whose channels beyond C hold PAD in turn"""
    B, n, C = a.shape
    t = np.empty((B, n, ld), np.float32)
    for c in range(C, ld):
        t[..., c] = PAD[(c - C) % len(PAD)]
    t[..., :C] = a
    return torch.from_numpy(t).to(TORCH[dtype])


def tensors(name, dtype, layout=("pad", "pad")):
    """(heads, branches): per level CPU tensors [B, cells_l, ld]; branches is None for the det head"""
    bt = build(name, dtype)
    c, off = bt.case, level_offsets(bt.case.geom)
    x = np.concatenate([bt.bins.reshape(c.B, c.cells, 64), bt.logits], -1)
    heads = [nhwc(x[:, off[i]:off[i + 1]], head_ld(c, dtype, layout[0]), dtype) for i in range(len(off) - 1)]
    branches = None
    if c.task:
        branches = [nhwc(bt.branch[:, off[i]:off[i + 1]], branch_ld(c, dtype, layout[1]), dtype) for i in range(len(off) - 1)]
    return heads, branches
