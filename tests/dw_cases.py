"""The depthwise table: single launches of kernels/conv_dw.hip (groups == C, k 3 / 5 / 7 with pad k / 2, stride 1 / 2, fp16 and fp32), shared by
tests/test_attention_dw_cases_cpu.py (coverage, conditioning of the reference, the mutations the table must catch) and
tests/test_gpu_depthwise_op.py (the kernel through the C ABI entry trtx_op_conv2d_dw_nhwc, in aligned and misaligned channel slices).

The kernel has twelve instantiations (k x stride x type) times two paths: whole 16-byte channel vectors (8 halves / 4 floats; C, every channel
stride and every base pointer allow them) or one channel per lane.  fp16 takes the vector path for C % 8 == 0, fp32 for C % 4 == 0; every C of this
table is a multiple of 4, so the fp32 element-wise path, and the fp16 one for C 8 / 64, is reached through the layout of the slice
(tests/test_gpu_depthwise_op.py runs every case in both).  One lane computes a strip of four neighbouring output columns, and the grid is
capped at 2048 blocks of 256 lanes: 524,288 work items (N * Ho * ceil(Wo / 4) * C / V) per trip of the grid-stride loop.

Every case is a few thousand outputs - the two that make the loop take a second trip excepted.  Data is seeded by the case name (zlib.crc32).
Operands are generated on the grid the kernel reads: x and the shortcut rounded to fp16 for an fp16 launch, fp32 otherwise; the filter
(fp32 [C][k][k] here, [k * k][C] on the device) and the bias are fp32 in both.  The reference is torch fp64 on those operands, so it has no
storage site of its own.

The bound, per element, with the sites counted from the kernel text:
    |err| <= fp32_bound(n, mag, amp) + fp16_walk(1, mag)          (the second term for fp16 launches only)
  * n = k * k + 2 fp32 terms: the bias, k * k fused multiply-adds (row by row), the shortcut;
  * the kernel adds the shortcut in fp32 and rounds once at the store: ONE fp16 site with or without a shortcut, none in fp32.  (The plan-level
    test tests/test_gpu_yolo11.py::test_depthwise_op_matches_torch counts 3 sites because its reference starts from the unrounded fp32 x and
    shortcut: their two storage roundings are sites there and operands here);
  * mag: the same convolution on absolute values plus |bias|, pushed through each activation's own growth - Lipschitz constant 1 for none / relu /
    leaky / tanh (each also has |f(v)| <= |v|), 1.1 for SiLU (slope <= 1.0998) and mish (<= 1.0885) - plus |shortcut|;
  * sigmoid is bounded by 1, not by |v|, so its magnitude is its own value and the error of its argument enters as an absolute term through its
    slope (<= 1 / 4): amp * mag = 0.25 * (1e-5 + n * 2^-24) * mag(argument), the `amp` of tests/layer_cases.py's Out.
Nothing here is fitted to a kernel's output."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from tests.layer_cases import U32, Out, fp32_bound
from tests.parity import fp16_walk

GRID_CAP = 2048 * 256     # conv_dw.hip grid_for: blocks x lanes, one work item per lane per trip
STRIP = 4                 # output columns per work item
ALPHA = 0.1               # the leaky slope every case uses
VEC = {"f16": 8, "f32": 4}


@dataclass(frozen=True)
class DwCase:
    name: str
    N: int
    H: int
    W: int
    C: int
    k: int
    s: int
    act1: str = "none"
    res: bool = False
    act2: str = "none"
    bias: bool = True
    engines: tuple = ("f16", "f32")
    big: bool = False     # a two-trip case: only the aligned and the fully misaligned layout run on the device

    @property
    def out_hw(self):
        p = self.k // 2
        return (self.H + 2 * p - self.k) // self.s + 1, (self.W + 2 * p - self.k) // self.s + 1

    @property
    def outputs(self):
        return self.N * self.out_hw[0] * self.out_hw[1] * self.C

    def work_items(self, v):
        """lanes' worth of work of a launch that moves v channels per lane"""
        Ho, Wo = self.out_hw
        return self.N * Ho * ((Wo + STRIP - 1) // STRIP) * (self.C // v)

    def paths(self, engine):
        """the kernel paths the device test reaches: the slice's layout forces the element-wise one; C decides whether the vector one exists"""
        return {"vector", "scalar"} if self.C % VEC[engine] == 0 else {"scalar"}


CASES = []


def add(name, N, H, W, C, k, s, act1="none", res=False, act2="none", bias=True, engines=("f16", "f32"), big=False):
    assert all(o.name != name for o in CASES), name
    CASES.append(DwCase(name, N, H, W, C, k, s, act1, res, act2, bias, tuple(engines), big))


# ---- k x stride x C x map x epilogue, crossed: every (k, stride) with a C that is whole vectors in both types and one that is not in fp16 -----------------
add("k3s1_c8_13x17_silu", 2, 13, 17, 8, 3, 1, "silu")                                  # exactly one fp16 vector
add("k3s1_c4_15x18_tanh", 2, 15, 18, 4, 3, 1, "tanh")                                  # exactly one fp32 vector
add("k3s2_c12_13x17_relu", 2, 13, 17, 12, 3, 2, "relu")                                # C 12: vectors in fp32, element-wise in fp16; odd x odd under stride 2
add("k3s2_c64_16x16_silu_res_silu", 2, 16, 16, 64, 3, 2, "silu", True, "silu")         # even x even; shortcut under stride 2 with a second activation
add("k5s1_c20_16x16_leaky", 2, 16, 16, 20, 5, 1, "leaky")
add("k5s1_c64_13x17_res_relu", 1, 13, 17, 64, 5, 1, "none", True, "relu")
add("k5s2_c64_16x16_silu_res", 2, 16, 16, 64, 5, 2, "silu", True)                      # shortcut under stride 2, no second activation
add("k5s2_c8_15x18_res_nobias", 2, 15, 18, 8, 5, 2, "none", True, bias=False)          # odd x even; a null bias with a shortcut
add("k7s1_c36_15x18_mish", 1, 15, 18, 36, 7, 1, "mish")
add("k7s1_c8_16x16_sigmoid_nobias", 2, 16, 16, 8, 7, 1, "sigmoid", bias=False)
add("k7s2_c4_15x18", 2, 15, 18, 4, 7, 2)
add("k7s2_c64_13x17_tanh_res_relu", 1, 13, 17, 64, 7, 2, "tanh", True, "relu")
add("k7s2_c20_16x16_sigmoid_res", 2, 16, 16, 20, 7, 2, "sigmoid", True)                 # a bounded activation in front of a shortcut
add("k3s1_c36_13x17_mish_res", 1, 13, 17, 36, 3, 1, "mish", True)
add("k5s2_c12_13x17_leaky", 2, 13, 17, 12, 5, 2, "leaky")
# ---- the last strip: Wo % 4 in 1, 2, 3 under stride 2 with even and odd W, and under stride 1 ---------------------------------------------------------------
add("wo1_k3s2_w2_c20", 2, 9, 2, 20, 3, 2, "silu")
add("wo1_k5s2_w1_c8", 2, 8, 1, 8, 5, 2, "relu")
add("wo2_k5s2_w3_c8", 2, 8, 3, 8, 5, 2, "silu", True)
add("wo2_k3s2_w4_c36", 2, 9, 4, 36, 3, 2, "none")
add("wo3_k3s2_w5_c64", 2, 8, 5, 64, 3, 2, "silu")
add("wo3_k7s2_w6_c12", 2, 9, 6, 12, 7, 2, "relu", True, "relu")
add("wo5_k5s2_w10_c4", 2, 9, 10, 4, 5, 2, "leaky")
add("wo5_k3s1_w5_c8", 2, 11, 5, 8, 3, 1, "silu", True)
add("wo5_k7s2_w9_c64", 1, 9, 9, 64, 7, 2, "silu")
add("wo7_k3s2_w13_c20", 2, 9, 13, 20, 3, 2, "silu")
add("wo7_k7s1_w7_c64", 1, 8, 7, 64, 7, 1, "none", True)
add("wo7_k5s2_w14_c36", 2, 9, 14, 36, 5, 2, "tanh")
# ---- maps smaller than the filter --------------------------------------------------------------------------------------------------------------------------
add("small_1x1_k7s1_c64", 5, 1, 1, 64, 7, 1, "silu")
add("small_1x1_k7s2_c12", 5, 1, 1, 12, 7, 2, "none", True)
add("small_1x9_k7s2_c8", 3, 1, 9, 8, 7, 2, "silu")
add("small_9x1_k7s1_c12", 3, 9, 1, 12, 7, 1, "relu")
add("small_2x5_k7s2_c20", 3, 2, 5, 20, 7, 2, "leaky")
add("small_2x5_k7s1_c64_res", 3, 2, 5, 64, 7, 1, "silu", True, "relu")
add("small_2x5_k5s1_c4", 3, 2, 5, 4, 5, 1, "sigmoid")
# ---- the grid-stride loop's second trip.  Work items per trip: 524,288 -------------------------------------------------------------------------------------
# element-wise path, fp16, C 36 (never whole vectors): 1 x 122 x 480 -> 122 rows x 120 strips x 36 channels = 527,040 items (121 x 480 would be 522,720)
add("trip2_scalar_f16_c36_122x480_k3s1", 1, 122, 480, 36, 3, 1, "silu", engines=("f16",), big=True)
# vector path, fp32, C 256 (64 vectors), Wo 5 (two strips, the second with one live column): 1 x 4097 x 5 -> 4097 rows x 2 strips x 64 = 524,416 items
# (4096 rows are exactly one trip).  A narrow map keeps the tensor at 5.2 M outputs; a square one would need four times as many.
add("trip2_vector_f32_c256_4097x5_k3s1", 1, 4097, 5, 256, 3, 1, "relu", True, engines=("f32",), big=True)

BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

# the axis values the table must show (tests/test_attention_dw_cases_cpu.py)
AXES = {
    "k": [3, 5, 7],
    "s": [1, 2],
    "C": [4, 8, 12, 20, 36, 64],
    "s2_maps": [(13, 17), (16, 16), (15, 18)],
    "Wo": [1, 2, 3, 5, 7],
    "small_k7": [(1, 1), (1, 9), (9, 1), (2, 5)],
    "act1": ["none", "relu", "silu", "leaky", "sigmoid", "tanh", "mish"],
}


def _mish(t):
    return t * torch.tanh(F.softplus(t))


ACT = {"none": lambda t: t, "relu": torch.relu, "silu": F.silu, "leaky": lambda t: F.leaky_relu(t, ALPHA), "sigmoid": torch.sigmoid, "tanh": torch.tanh,
       "mish": _mish}
LIPSCHITZ = {"none": 1.0, "relu": 1.0, "leaky": 1.0, "tanh": 1.0, "silu": 1.1, "mish": 1.1, "sigmoid": 0.25}


def _rng(case, what):
    return np.random.default_rng(zlib.crc32((case.name + "/" + what).encode()))


@functools.lru_cache(maxsize=None)
def gen_inputs(name):
    """{x [N, H, W, C], w [C, k, k], bias [C], res [N, Ho, Wo, C]}: fp32 torch, not yet on any engine's grid"""
    c = BY_NAME[name]
    Ho, Wo = c.out_hw
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return dict(x=t(_rng(c, "x").standard_normal((c.N, c.H, c.W, c.C))),
                w=t(_rng(c, "w").standard_normal((c.C, c.k, c.k)) / c.k),
                bias=t(_rng(c, "bias").standard_normal(c.C) * 0.5),
                res=t(_rng(c, "res").standard_normal((c.N, Ho, Wo, c.C))))


def stored(case, engine):
    """(x, res or None) NHWC as the launch reads them: on the fp16 grid for an fp16 launch (torch.float16), fp32 otherwise"""
    d = gen_inputs(case.name)
    cast = (lambda t: t.half()) if engine == "f16" else (lambda t: t)
    return cast(d["x"]), cast(d["res"]) if case.res else None


def taps_c(case):
    """the filter as the device reads it: fp32 numpy [k * k][C], tap-major"""
    w = gen_inputs(case.name)["w"].numpy()
    return np.ascontiguousarray(w.reshape(case.C, case.k * case.k).T)


def _conv(case, x, w, b):
    return F.conv2d(x, w[:, None], b, case.s, case.k // 2, 1, case.C)


@dataclass
class Ref:
    y: torch.Tensor        # [N, Ho, Wo, C] fp64
    mag: torch.Tensor
    bound: torch.Tensor
    n: int
    sites: int


def _through(act, v, mag, extra, e_rel):
    """one activation: (value, magnitude, absolute extra) behind it"""
    if act == "sigmoid":
        r = torch.sigmoid(v)
        return r, r, LIPSCHITZ[act] * (extra + e_rel * mag)
    return ACT[act](v), LIPSCHITZ[act] * mag, LIPSCHITZ[act] * extra


@functools.lru_cache(maxsize=None)
def reference(name, engine):
    case = BY_NAME[name]
    d = gen_inputs(name)
    x, res = stored(case, engine)
    x = x.double().permute(0, 3, 1, 2)
    res = None if res is None else res.double().permute(0, 3, 1, 2)
    w = d["w"].double()
    b = d["bias"].double() if case.bias else None
    n = case.k * case.k + 2
    e_rel = 1e-5 + n * U32
    pre = _conv(case, x, w, b)
    mag = _conv(case, x.abs(), w.abs(), None if b is None else b.abs())
    y, mag, extra = _through(case.act1, pre, mag, torch.zeros_like(mag), e_rel)
    if res is not None:
        y, mag = y + res, mag + res.abs()
    y, mag, extra = _through(case.act2, y, mag, extra, e_rel)
    sites = 1 if engine == "f16" else 0
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    y, mag, extra = nhwc(y), nhwc(mag), nhwc(extra)
    bound = fp32_bound(Out(None, mag, n=n, amp=extra / mag.clamp_min(1e-30))) + (fp16_walk(sites, mag) if sites else 0.0)
    return Ref(y, mag, bound, n, sites)


def restate(name, engine, mutate=None):
    """The kernel's arithmetic in torch fp32, rounded where the kernel rounds: the accumulator starts at the bias and takes the taps row by row
    (a tap outside the image is skipped: adding its exact zero product is the same), act1, + shortcut, act2 in fp32, one rounding at an fp16 store.
    mutate = "clamp": a border tap reads the nearest pixel instead of being skipped; "strip": the live outputs of a ragged last strip all carry
    the sum of the strip's fourth column (wo0 + 3, beyond the map).  -> [N, Ho, Wo, C] in the launch's type"""
    case = BY_NAME[name]
    d = gen_inputs(name)
    x, res = stored(case, engine)
    k, s, p = case.k, case.s, case.k // 2
    Ho, Wo = case.out_hw
    strips = (Wo + STRIP - 1) // STRIP
    Wo_full = strips * STRIP if mutate == "strip" else Wo     # columns the strips compute
    x = x.float().permute(0, 3, 1, 2)
    right = max(0, (Wo_full - 1) * s + k - (case.W + 2 * p))
    if mutate == "clamp":
        xp = F.pad(F.pad(x, (p, p, p, p), mode="replicate"), (0, right, 0, 0))
    else:
        xp = F.pad(x, (p, p + right, p, p))
    w = d["w"]
    acc = (d["bias"] if case.bias else torch.zeros(case.C))[None, :, None, None].expand(case.N, case.C, Ho, Wo_full).clone()
    for r in range(k):
        for q in range(k):
            acc += xp[:, :, r:r + (Ho - 1) * s + 1:s, q:q + (Wo_full - 1) * s + 1:s] * w[:, r, q][None, :, None, None]
    if mutate == "strip" and Wo % STRIP:
        acc[..., (strips - 1) * STRIP:Wo] = acc[..., Wo_full - 1:Wo_full]
    acc = acc[..., :Wo]
    y = ACT[case.act1](acc)
    if res is not None:
        y = y + res.float().permute(0, 3, 1, 2)
    y = ACT[case.act2](y).permute(0, 2, 3, 1).contiguous()
    return y.half() if engine == "f16" else y
