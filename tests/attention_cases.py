"""The attention table: single launches of kernels/attention.hip (YOLO11's PSA attention: kd 32, hd 64, every pixel a key) and
kernels/attention_mfma.hip (YOLOv12's area attention on MFMA: kd 32, hd 32, the image split into `area` ranges of Na = N / area pixels),
shared by tests/test_attention_dw_cases_cpu.py (coverage, conditioning, the mutations the table must catch) and
tests/test_gpu_attention_op.py (the kernels through the C ABI, in aligned and misaligned channel slices).

Both kernels walk the keys in chunks of 64 with an online softmax; the area kernel updates its running max per 32-key group, each of the four
16-lane groups of a wave holding 8 keys of it, rounds P to fp16 for the second MFMA, zero-fills the LDS rows of a partial chunk and masks their
scores.  The sizes are the edges of that: Na / N in 1, 2, 8, 31, 32, 33, 40, 63, 64, 65, 97, 128, 129, 200 (a remainder of 1..8 keys leaves three of the
four lane groups with masked keys only; 65 and 129 leave a query tile with one live lane).  Besides Gaussian data:
  * rising / falling: key m's score grows / shrinks monotonically with m over four chunks - every key (PSA) and every group (area) raises the running
    max and rescales what was accumulated, or the first one holds it;
  * large: |score| > 40 and at least 30 % of the rows dominated by one key (the conditions tests/test_gpu_yolo11.py asserts; the host test asserts them here);
  * tied: every key of a (image, head) has the same k row, so all scores of a row are equal and O is the mean of v;
  * leak: one target area holds Gaussian data; in every other area and image v is offset by +-200 (exact in fp16, the sign alternating from area to
    area) and the k rows are scaled by 8.  A single key of a neighbour read at the edge of a partial chunk moves a target output by up to 200.

qkv is generated on the fp16 grid (the kernels read fp16), so the fp64 reference has no storage site of its own.  Per element, sites from the kernel text:
    PSA :  |err| <= fp16_walk(1, |O|) + 1e-4 * max|v| + E_exp                       (P and O stay fp32; one rounding at the store)
    area:  |err| <= 2 u16 * (softmax @ |v|) + fp16_walk(1, |O|) + 1e-4 * max|v| + E_exp     (P rounded to fp16: relative u16 per weight, numerator only)
  * 1e-4 * max|v| is the floor the plan-level tests use for the fp32 arithmetic in between, the maximum taken here over the v rows a query may see (its
    image, head and area: never more than the whole tensor's); the "one-ulp disagreement of q / k" term of those tests is dropped: there qkv is the
    rounded output of a convolution, here it is given;
  * E_exp, the exponential's argument.  A weight is exp(s_m - max) built from exp(s_m - running max) times the later rescales exp(old max - new max); the
    running max only rises, so the arguments of one key's factors have one sign and sum to s_m - max.  Each factor's argument is rounded to fp32 (2^-24
    relative), and the fast __expf multiplies it by a rounded log2(e) (2^-24 again, the constant's own error 2^-25 more): 3 * 2^-24 * |s_m - max| =: d_m on the
    logarithm of weight m.  To first order dO = sum_m w_m d_m (v_m - O), so  E_exp = (w * d) @ |v| + (sum_m w_m d_m) * |O|.  With scores of +-60 this
    reaches 1e-5 * |v| on a row with two comparable keys far below the max of their partial chunk - an order of magnitude under the floor, but it grows with
    the scores where the floor does not;
  * the V image is a copy: bit-equal to the v slice of qkv."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from tests.layer_cases import U32
from tests.parity import EPS16, fp16_walk

KD = 32
HD = {"psa": 64, "area": 32}
SCALE = KD ** -0.5
CHUNK, GROUP = 64, 32
FLOOR = 1e-4
LEAK_OFFSET, LEAK_GAIN = 200.0, 8.0


@dataclass(frozen=True)
class AttnCase:
    name: str
    kind: str            # "psa" | "area"
    B: int
    heads: int
    N: int
    area: int = 1
    data: str = "gauss"  # gauss | rising | falling | large | tied | leak

    @property
    def hd(self):
        return HD[self.kind]

    @property
    def Na(self):
        return self.N // self.area

    @property
    def width(self):
        return self.heads * (2 * KD + self.hd)

    @property
    def target(self):
        """(image, area) of the leak case's Gaussian block: a middle one, so that pixels of a neighbour follow it wherever there is a neighbour"""
        return (self.B - 1) // 2, (self.area - 1) // 2


CASES = []


def add(name, kind, B, heads, N, area=1, data="gauss"):
    assert all(o.name != name for o in CASES), name
    assert N % area == 0
    CASES.append(AttnCase(name, kind, B, heads, N, area, data))


# ---- PSA: heads 1..3 x B 1..2 x N ---------------------------------------------------------------------------------------------------------------------------
add("psa_n1_h2_b2", "psa", 2, 2, 1)
add("psa_n2_h1_b1", "psa", 1, 1, 2)
add("psa_n63_h3_b1", "psa", 1, 3, 63)
add("psa_n64_h1_b2", "psa", 2, 1, 64)
add("psa_n65_h2_b1", "psa", 1, 2, 65)          # the second query tile has one live lane; the second key chunk one key
add("psa_n129_h1_b2", "psa", 2, 1, 129)
add("psa_n200_h3_b2", "psa", 2, 3, 200)
add("psa_rising_n200_h1_b1", "psa", 1, 1, 200, data="rising")
add("psa_falling_n200_h2_b1", "psa", 1, 2, 200, data="falling")
add("psa_large_n65_h2_b2", "psa", 2, 2, 65, data="large")
add("psa_large_n129_h1_b1", "psa", 1, 1, 129, data="large")
add("psa_tied_n129_h1_b1", "psa", 1, 1, 129, data="tied")
add("psa_leak_n65_h1_b2", "psa", 2, 1, 65, data="leak")   # the next image's keys behind a one-key chunk
# ---- area: heads in 1, 2, 5 x B in 1, 3 x area in 1, 2, 4 x Na ------------------------------------------------------------------------------------------------
add("area_na1_a4_h2_b3", "area", 3, 2, 4, 4)
add("area_na8_a1_h1_b1", "area", 1, 1, 8, 1)
add("area_na31_a2_h5_b1", "area", 1, 5, 62, 2)
add("area_na32_a1_h2_b3", "area", 3, 2, 32, 1)
add("area_na33_a4_h1_b1", "area", 1, 1, 132, 4)
add("area_na40_a2_h2_b3", "area", 3, 2, 80, 2)
add("area_na63_a1_h5_b1", "area", 1, 5, 63, 1)
add("area_na64_a2_h1_b3", "area", 3, 1, 128, 2)
add("area_na65_a4_h2_b1", "area", 1, 2, 260, 4)
add("area_na97_a1_h1_b3", "area", 3, 1, 97, 1)
add("area_na128_a2_h2_b1", "area", 1, 2, 256, 2)
add("area_na129_a1_h5_b1", "area", 1, 5, 129, 1)
add("area_rising_na200_a2_h2_b1", "area", 1, 2, 400, 2, "rising")
add("area_falling_na200_a1_h1_b3", "area", 3, 1, 200, 1, "falling")
add("area_large_na97_a2_h2_b1", "area", 1, 2, 194, 2, "large")
add("area_large_na40_a4_h1_b3", "area", 3, 1, 160, 4, "large")
add("area_tied_na129_a2_h1_b1", "area", 1, 1, 258, 2, "tied")
add("area_leak_na40_a4_h2_b3", "area", 3, 2, 160, 4, "leak")      # 40 keys: the group 32..63 holds 8 live keys, then the next area's
add("area_leak_na97_a1_h1_b3", "area", 3, 1, 97, 1, "leak")       # area 1: the neighbours are the other images
add("area_leak_na33_a2_h5_b1", "area", 1, 5, 66, 2, "leak")       # one key in the last group

BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
PSA = [c for c in CASES if c.kind == "psa"]
AREA = [c for c in CASES if c.kind == "area"]

AXES = {
    "psa": {"heads": [1, 2, 3], "B": [1, 2], "N": [1, 2, 63, 64, 65, 129, 200]},
    "area": {"heads": [1, 2, 5], "B": [1, 3], "area": [1, 2, 4], "Na": [1, 8, 31, 32, 33, 40, 63, 64, 65, 97, 128, 129]},
    "data": ["gauss", "rising", "falling", "large", "tied", "leak"],
}


def _rng(case, what):
    return np.random.default_rng(zlib.crc32((case.name + "/" + what).encode()))


def split(case, qkv):
    """[B, N, width] -> q [B, heads, N, KD], k likewise, v [B, heads, N, hd] (views)"""
    t = qkv.reshape(case.B, case.N, case.heads, 2 * KD + case.hd).permute(0, 2, 1, 3)
    return t[..., :KD], t[..., KD:2 * KD], t[..., 2 * KD:]


@functools.lru_cache(maxsize=None)
def gen_inputs(name):
    """qkv [B, N, heads * (2 KD + hd)] torch.float16: head h's channels are q (KD), k (KD), v (hd)"""
    c = BY_NAME[name]
    B, H, N, hd = c.B, c.heads, c.N, c.hd
    q = _rng(c, "q").standard_normal((B, H, N, KD))
    k = _rng(c, "k").standard_normal((B, H, N, KD))
    v = _rng(c, "v").standard_normal((B, H, N, hd))
    if c.data in ("rising", "falling"):
        # q_n = a_n on four channels, k_m = m / 16 on the same four (exact in fp16 up to m = 2047): score = SCALE * a_n * m / 4, a step of
        # 0.044 .. 0.088 per key - every key is a new maximum (a_n > 0) or the first one stays it (a_n < 0), and some twenty keys carry weight
        a = _rng(c, "a").integers(2, 5, (B, H, N, 1)) * (0.5 if c.data == "rising" else -0.5)
        m = np.arange(N, dtype=np.float64)[None, None, :, None]
        q = np.zeros_like(q)
        k = np.zeros_like(k)
        q[..., :4] = a
        k[..., :4] = m / 16.0
    elif c.data == "large":
        q, k = q * 6.0, k * 6.0
    elif c.data == "tied":
        k = np.broadcast_to(k[:, :, :1], k.shape).copy()
    elif c.data == "leak":
        tb, ta = c.target
        for b in range(B):
            for a in range(c.area):
                if (b, a) == (tb, ta):
                    continue
                sl = slice(a * c.Na, (a + 1) * c.Na)
                k[b, :, sl] *= LEAK_GAIN
                v[b, :, sl] += LEAK_OFFSET * (1.0 if (b + a) % 2 else -1.0)
    qkv = np.concatenate([q, k, v], axis=-1).transpose(0, 2, 1, 3).reshape(B, N, c.width)
    return torch.from_numpy(np.ascontiguousarray(qkv, dtype=np.float32)).half()


def _blocks(case, t):
    """[B, heads, N, d] -> [B, heads, area, Na, d]"""
    return t.reshape(case.B, case.heads, case.area, case.Na, t.shape[-1])


@dataclass
class Ref:
    o: torch.Tensor        # [B, N, heads * hd] fp64
    v: torch.Tensor        # [B, N, heads * hd] torch.float16: what the V image must equal bit for bit
    bound: torch.Tensor
    scores: torch.Tensor   # [B, heads, area, Na, Na] fp64, scaled
    e_exp: torch.Tensor


def _image(case, t):
    """[B, heads, area, Na, hd] -> [B, N, heads * hd]"""
    return t.reshape(case.B, case.heads, case.N, case.hd).permute(0, 2, 1, 3).reshape(case.B, case.N, case.heads * case.hd).contiguous()


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    qkv = gen_inputs(name)
    q, k, v = (_blocks(c, t.double()) for t in split(c, qkv))
    s = (q @ k.transpose(-2, -1)) * SCALE
    w = s.softmax(-1)
    o = w @ v
    pv = w @ v.abs()
    d = 3 * U32 * (s - s.max(-1, keepdim=True).values).abs()
    e_exp = (w * d) @ v.abs() + (w * d).sum(-1, keepdim=True) * o.abs()
    bound = fp16_walk(1, o.abs()) + FLOOR * v.abs().amax((-2, -1), keepdim=True) + e_exp
    if c.kind == "area":
        bound = bound + 2 * EPS16 * pv
    vimg = split(c, qkv)[2].permute(0, 2, 1, 3).reshape(c.B, c.N, c.heads * c.hd).contiguous()
    return Ref(_image(c, o), vimg, _image(c, bound), s, _image(c, e_exp))


def restate(name, mutate=None):
    """The kernels' arithmetic in torch fp32, rounded where they round: scores in fp32 (exact fp16 products), online softmax over 64-key chunks - the
    area kernel in 32-key groups, P rounded to fp16 for the product with V and unrounded in the denominator; the PSA kernel a chunk at a time, P in fp32 -,
    the accumulator rescaled by exp(old max - new max), one fp16 rounding of O.  Keys beyond the area are masked (score -inf, weight 0).
    mutate = "nomask": the keys a partial chunk (PSA) / group (area) has room for beyond the area are read from the pixels that follow (the next area, the next
    image, zeros behind the last) and take part;  "norescale": the accumulator keeps its old scale when the max rises (the denominator is rescaled);
    "lanegroup" (area): O is divided by the share of the denominator one 16-lane group holds - keys 0..7 of every 32-key group - instead of the whole.
    -> O [B, N, heads * hd] torch.float16"""
    c = BY_NAME[name]
    qkv = gen_inputs(name)
    q, k, v = (t.float() for t in split(c, qkv))           # [B, heads, N, d]
    step = GROUP if c.kind == "area" else CHUNK
    Na, hd = c.Na, c.hd
    # the keys as one pixel sequence over the batch, zeros behind it: what an unmasked read beyond an area finds
    kflat = torch.cat([k.permute(1, 0, 2, 3).reshape(c.heads, c.B * c.N, KD), torch.zeros(c.heads, step, KD)], 1)
    vflat = torch.cat([v.permute(1, 0, 2, 3).reshape(c.heads, c.B * c.N, hd), torch.zeros(c.heads, step, hd)], 1)
    out = torch.empty(c.B, c.heads, c.N, hd)
    for b in range(c.B):
        for a in range(c.area):
            p0 = b * c.N + a * Na
            qa = q[b, :, a * Na:(a + 1) * Na]                                   # [heads, Na, KD]
            acc = torch.zeros(c.heads, Na, hd)
            mx = torch.full((c.heads, Na, 1), -float("inf"))
            den = torch.zeros(c.heads, Na, 1)
            share = torch.zeros(c.heads, Na, 1)
            for m0 in range(0, Na, step):
                kk, vv = kflat[:, p0 + m0:p0 + m0 + step], vflat[:, p0 + m0:p0 + m0 + step]
                s = (qa @ kk.transpose(-2, -1)) * SCALE                          # [heads, Na, step]
                live = torch.arange(m0, m0 + step) < Na
                if mutate != "nomask":
                    s = s.masked_fill(~live[None, None, :], -float("inf"))
                mnew = torch.maximum(mx, s.max(-1, keepdim=True).values)
                alpha = torch.exp(mx - mnew)
                p = torch.exp(s - mnew)
                den = den * alpha + p.sum(-1, keepdim=True)
                share = share * alpha + p[..., :8].sum(-1, keepdim=True)
                if mutate != "norescale":
                    acc = acc * alpha
                pm = p.half().float() if c.kind == "area" else p
                acc = acc + pm @ vv
                mx = mnew
            out[b, :, a * Na:(a + 1) * Na] = acc / (share if mutate == "lanegroup" else den)
    return out.permute(0, 2, 1, 3).reshape(c.B, c.N, c.heads * hd).half()
