"""The fused stem pair (tensorrtx_amd/csrc/kernels/conv_stem_pair.hip) on the CPU.

1. Its index arithmetic (kernels/stem_pair_index.h, compiled with g++ as it stands - the kernel calls the same functions) replayed lane by lane:
   fp32 input patch -> 36 stem groups of 16 region pixels -> LDS image of the intermediate (zeros outside the intermediate image) -> the
   second convolution's fragments, two taps per 32-wide k-step -> v_mfma_f32_16x16x32_f16 semantics -> 8 consecutive channels per lane,
   against a NumPy direct convolution of both layers.  What this file mirrors by hand are the few lines of the kernel that are not index
   functions: the patch fill (bounds -> zero), the stem's tap table (stem_setup) and the out-of-image test.
2. The plan pass (plan_passes.cpp mark_stem_pair): which plans carry the mark."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tensorrtx_amd import engine
from util import synth_wts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "tensorrtx_amd", "csrc", "kernels")

SHIM = r"""
#include "stem_pair_index.h"
using namespace trtx::pairidx;
extern "C" {
void c_consts(int* o) { o[0] = kTH; o[1] = kTW; o[2] = kRH; o[3] = kRW; o[4] = kGroups; o[5] = kPR; o[6] = kPCA; o[7] = kImageBytes; o[8] = kSteps; o[9] = kTaps; }
void c_tile_of(int tile, int tiles_x, int tiles_y, int* o) { Tile t = tile_of(tile, tiles_x, tiles_y); o[0] = t.n; o[1] = t.y0; o[2] = t.x0; }
int c_region_start(int o0) { return region_start(o0); }
int c_patch_start(int o0) { return patch_start(o0); }
int c_patch_aligned_start(int wi) { return patch_aligned_start(wi); }
void c_region_pixel(int group, int lane, int* o) { RegionPixel r = region_pixel(group, lane); o[0] = r.ry; o[1] = r.rx; o[2] = r.live; }
int c_patch_offset(int ry, int rx, int shift) { return patch_offset(ry, rx, shift); }
int c_image_offset(int ry, int rx, int ch) { return image_offset(ry, rx, ch); }
int c_step_tap(int kt, int lane) { return step_tap(kt, lane); }
int c_step_chunk(int lane) { return step_chunk(lane); }
int c_frag_offset(int oy, int ox, int tap, int chunk) { return frag_offset(oy, ox, tap, chunk); }
int c_weight_row_channel(int j, int a) { return weight_row_channel(j, a); }
}
"""

# the GPU test's shapes (tests/test_gpu_stem_pair.py): one partial tile; exact tiles; odd intermediate height with ragged tiles in x and y;
# odd height and a width one past a 16-pixel fragment
SHAPES = [(1, 20, 24), (2, 64, 64), (3, 70, 132), (2, 38, 68)]


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "shim.cpp")
        open(src, "w").write(SHIM)
        so = os.path.join(tmp, "shim.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{HDR}", src, "-o", so])
        yield ctypes.CDLL(so)


def _silu(v):
    return v / (1.0 + np.exp(-v))


def _conv_s2(x, w, b):
    """x [N,H,W,C], w [Co,C,3,3], b [Co], float64: 3x3 stride 2 pad 1, SiLU"""
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.zeros((N, Ho, Wo, w.shape[0])) + b
    for r in range(3):
        for q in range(3):
            out += np.einsum("nhwc,oc->nhwo", xp[:, r:r + 2 * Ho:2, q:q + 2 * Wo:2], w[:, :, r, q].astype(np.float64))
    return _silu(out)


def test_index_functions_cover_their_ranges(shim):
    L = shim
    c = (ctypes.c_int * 10)()
    L.c_consts(c)
    TH, TW, RH, RW, G, PR, PCA, IMG, STEPS, TAPS = list(c)
    assert (RH, RW, PR) == (2 * TH + 1, 2 * TW + 1, 2 * RH + 1) and G * 16 >= RH * RW > (G - 1) * 16 and G % 4 == 0
    o = (ctypes.c_int * 3)()
    seen = set()
    for g in range(G):
        for ln in range(64):
            L.c_region_pixel(g, ln, o)
            ry, rx, live = list(o)
            assert 0 <= ry < RH and 0 <= rx < RW
            if live and ln < 16:
                seen.add((ry, rx))
            # every tap of every lane (clamped tail lanes included) stays inside one channel plane of the patch: 2 rows / 2 columns below the corner
            assert L.c_patch_offset(ry, rx, 3) + 2 * PCA + 2 < PR * PCA and 2 * rx + 3 + 2 < PCA
    assert len(seen) == RH * RW                                    # every region pixel is computed by exactly one lane column
    # the image: 8-byte pieces of all region pixels tile it without overlap, inside kImageBytes
    offs = sorted(L.c_image_offset(ry, rx, ch) for ry in range(RH) for rx in range(RW) for ch in (0, 4, 8, 12))
    assert len(set(offs)) == len(offs) and offs[0] == 0 and offs[-1] + 8 <= IMG and all(v % 8 == 0 for v in offs)
    # a fragment's 16 pixels x 2 chunks of one tap are one contiguous 512-byte run: ds_read_b128 without bank conflicts
    for oy in range(TH):
        for tap in range(TAPS):
            run = sorted(L.c_frag_offset(oy, ox, tap, ch) for ox in range(TW) for ch in (0, 1))
            assert run == list(range(run[0], run[0] + 512, 16))
    # k-step placement: k = 32 kt + 8 (lane >> 4) + e is tap k // 16, channel k % 16
    for kt in range(STEPS):
        for ln in range(64):
            k0 = 32 * kt + 8 * (ln >> 4)
            assert L.c_step_tap(kt, ln) == k0 // 16 and L.c_step_chunk(ln) * 8 == k0 % 16
    # a lane's accumulator rows 4g + e of fragments 0 and 1 are channels 8g .. 8g + 7
    for g in range(4):
        assert [L.c_weight_row_channel(j, 4 * g + e) for j in (0, 1) for e in range(4)] == list(range(8 * g, 8 * g + 8))
    assert sorted(L.c_weight_row_channel(j, a) for j in (0, 1) for a in range(16)) == list(range(32))
    for wi in range(-7, 9):
        a = L.c_patch_aligned_start(wi)
        assert a % 4 == 0 and a <= wi < a + 4


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_lane_level_replay_of_the_pair_kernel_is_the_two_convolutions(shim, N, H, W):
    L = shim
    c = (ctypes.c_int * 10)()
    L.c_consts(c)
    TH, TW, RH, RW, G, PR, PCA, IMG, STEPS, TAPS = list(c)
    rng = np.random.default_rng(N * 1000 + H)
    Cin = 3
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float16).astype(np.float32)        # fp16-representable: the kernel converts its taps to fp16
    w0 = (rng.standard_normal((16, Cin, 3, 3)) * (2.0 / 27) ** 0.5).astype(np.float16)
    b0 = rng.standard_normal(16).astype(np.float32) * 0.5
    w1 = (rng.standard_normal((32, 16, 3, 3)) * (2.0 / 144) ** 0.5).astype(np.float16)
    b1 = rng.standard_normal(32).astype(np.float32) * 0.5
    Hi, Wi = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    # reference: both layers in float64, the intermediate rounded to fp16 as the stem stores it
    mid_ref = _conv_s2(x.transpose(0, 2, 3, 1).astype(np.float64), w0, b0.astype(np.float64)).astype(np.float16)
    ref = _conv_s2(mid_ref.astype(np.float64), w1, b1.astype(np.float64))
    # operands as the kernel holds them
    stem_w = w0.reshape(16, 27).astype(np.float32)                 # [cout][k = (c*3 + r)*3 + q]
    l_off = np.array([((k // 9) * PR + (k % 9) // 3) * PCA + k % 3 for k in range(27)])   # stem_setup's tap table
    packed = np.zeros((32, 160), np.float16)                       # [Cout_pad][Kpad], k = tap * 16 + c
    for r in range(3):
        for q in range(3):
            packed[:, (r * 3 + q) * 16:(r * 3 + q) * 16 + 16] = w1[:, :, r, q]
    o3 = (ctypes.c_int * 3)()
    lanes = np.arange(64)
    rp = np.zeros((G, 64, 3), np.int64)
    for g in range(G):
        for ln in range(64):
            L.c_region_pixel(g, ln, o3)
            rp[g, ln] = list(o3)
    img_off = np.array([[[L.c_image_offset(int(rp[g, ln, 0]), int(rp[g, ln, 1]), 4 * (ln >> 4)) for ln in range(64)] for g in range(G)]])[0]
    wrow = np.array([[L.c_weight_row_channel(j, a) for a in range(16)] for j in (0, 1)])
    tiles_x, tiles_y = (Wo + TW - 1) // TW, (Ho + TH - 1) // TH
    out = np.full((N, Ho, Wo, 32), np.nan, np.float32)
    for tile in range(N * tiles_x * tiles_y):
        L.c_tile_of(tile, tiles_x, tiles_y, o3)
        n, y0, x0 = list(o3)
        hi_start, wi_start = L.c_patch_start(y0), L.c_patch_start(x0)
        al_start = L.c_patch_aligned_start(wi_start)
        shift = wi_start - al_start
        assert 0 <= shift < 4
        # stage 1 (mirrored): element (c, pr, pc) of the patch = input (hi_start + pr, al_start + pc), zero outside the image
        patch = np.zeros((Cin, PR, PCA), np.float32)
        for pr in range(PR):
            hi = hi_start + pr
            if 0 <= hi < H:
                lo, hi_c = max(0, -al_start), min(PCA, W - al_start)
                if hi_c > lo:
                    patch[:, pr, lo:hi_c] = x[n, :, hi, al_start + lo:al_start + hi_c]
        patch = patch.ravel()
        # stage 2: wave w computes groups w, w + 4, ...; a lane's 4 channels (8 bytes) go to image_offset
        img = np.full(IMG // 2, np.float16(np.nan))
        iy0, ix0 = L.c_region_start(y0), L.c_region_start(x0)
        for g in range(G):
            src = np.array([L.c_patch_offset(int(rp[g, ln, 0]), int(rp[g, ln, 1]), shift) for ln in range(16)])
            X = patch[src[:, None] + l_off[None, :]].astype(np.float16).astype(np.float32)      # [pixel][k]: the B operand
            acc = stem_w @ X.T                                                                   # [channel][pixel]
            val = _silu((acc + b0[:, None]).astype(np.float64)).astype(np.float16)
            for ln in lanes:
                ry, rx, live = (int(v) for v in rp[g, ln])
                iy, ix = iy0 + ry, ix0 + rx
                v4 = val[4 * (ln >> 4):4 * (ln >> 4) + 4, ln & 15]
                if not (0 <= iy < Hi and 0 <= ix < Wi):
                    v4 = np.zeros(4, np.float16)                    # the second convolution's padding, not a stem value
                if live:
                    o = int(img_off[g, ln]) // 2
                    img[o:o + 4] = v4
        # the image is what the stem computes inside the intermediate and zero outside (1 fp16 ulp: fp32 sums here, float64 in the reference)
        for ry in range(RH):
            for rx in range(RW):
                o = L.c_image_offset(ry, rx, 0) // 2
                iy, ix = iy0 + ry, ix0 + rx
                got = img[o:o + 16].astype(np.float32)
                if 0 <= iy < Hi and 0 <= ix < Wi:
                    want = mid_ref[n, iy, ix].astype(np.float32)
                    assert np.all(np.abs(got - want) <= 2.0 ** -10 * np.maximum(np.abs(want), 2.0 ** -14)), (tile, ry, rx)
                else:
                    assert np.all(got == 0), (tile, ry, rx)
        # stage 3: wave w owns tile rows 2w, 2w + 1
        for wv in range(4):
            for i in range(2):
                oy = 2 * wv + i
                acc = np.zeros((2, 16, 16), np.float32)             # [fragment][weight row][pixel]
                for kt in range(STEPS):
                    B = np.zeros((16, 32), np.float32)              # [pixel][k of this step]
                    for ln in lanes:
                        tap, chunk = L.c_step_tap(kt, int(ln)), L.c_step_chunk(int(ln))
                        if tap < TAPS:
                            o = L.c_frag_offset(oy, int(ln & 15), tap, chunk) // 2
                            B[ln & 15, 8 * (ln >> 4):8 * (ln >> 4) + 8] = img[o:o + 8]
                    for j in (0, 1):
                        A = packed[wrow[j], kt * 32:kt * 32 + 32].astype(np.float32)
                        acc[j] += A @ B.T
                y = y0 + oy
                for pxl in range(16):
                    xx = x0 + pxl
                    if y < Ho and xx < Wo:
                        for g4 in range(4):   # lane group g4 of this pixel: rows 4 g4 + e of fragments 0 and 1 = channels 8 g4 .. 8 g4 + 7
                            v8 = np.concatenate([acc[0, 4 * g4:4 * g4 + 4, pxl], acc[1, 4 * g4:4 * g4 + 4, pxl]])
                            assert not np.isnan(v8).any(), "a fragment read of a byte nobody wrote"
                            out[n, y, xx, 8 * g4:8 * g4 + 8] = _silu((v8 + b1[8 * g4:8 * g4 + 8]).astype(np.float64))
    assert not np.isnan(out).any(), "an output pixel no tile wrote"
    # 144 products of fp16 operands summed in fp32 (here) / float64 (reference), and an intermediate that may differ by 1 fp16 ulp per element
    err = np.abs(out - ref).max()
    assert err < 2e-3 * max(1.0, np.abs(ref).max()), err


# ---------------------------------------------------------------------------------------------------- the plan pass
def _ops(plan):
    return engine.describe_plan(plan, lowered=True)["ops"]


def _marked(ops):
    return [k for k, o in enumerate(ops) if o.get("stem_pair")]


def test_yolov8n_at_benchmark_size_has_one_marked_op_and_the_switch_removes_it(monkeypatch):
    path, _ = synth_wts("yolov8n")
    plan = engine.build_plan("yolov8n", path, batch=32, h=640, w=640, fp16=1)
    on = _ops(plan)
    assert _marked(on) == [1] and on[0]["stem"] and on[1]["kind"] == "conv" and (on[1]["cin"], on[1]["cout"], on[1]["k"][0]) == (16, 32, 3)
    monkeypatch.setenv("TRTX_STEM_PAIR", "0")
    off = _ops(plan)
    assert _marked(off) == []
    # the mark is all that differs: op count, kinds, names
    assert len(on) == len(off) == 53 and [o["kind"] for o in on] == [o["kind"] for o in off] and [o.get("name") for o in on] == [o.get("name") for o in off]


def test_other_stems_and_other_precisions_are_not_marked():
    path, _ = synth_wts("resnet50")
    assert _marked(_ops(engine.build_plan("resnet50", path, batch=2, fp16=1, h=64, w=64))) == []      # 7x7 stem
    path, _ = synth_wts("yolov8n")
    assert _marked(_ops(engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=0))) == []     # fp32 build
    assert _marked(_ops(engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=1))) == [1]


def _toy(second_reader=False, int8=False):
    """stem 3 -> 16 3x3/2, conv 16 -> 32 3x3/2, conv 32 -> 32 3x3, each with ReLU; optionally a second reader of the stem's output"""
    from tensorrtx_amd import builder, calibrator
    rng = np.random.default_rng(5)
    net = builder.Network(max_batch=2, fp16=True, int8=int8)
    x = net.input("data", (3, 32, 48))

    def conv(t, cin, cout, stride, k=3):
        w = rng.normal(0, 0.1, (cout, cin, k, k)).astype(np.float32)
        return net.out(net.activation(net.out(net.conv(t, w, bias=np.zeros(cout, np.float32), stride=stride, padding=k // 2)), "relu"))
    s = conv(x, 3, 16, 2)
    y = conv(conv(s, 16, 32, 2), 32, 32, 1)
    net.mark_output(y, "y")
    if second_reader:
        net.mark_output(conv(s, 16, 32, 1), "z")
    if int8:
        import struct
        fp16_net = _toy(second_reader)
        names = [t["name"] or f"(Unnamed Tensor* {t['id']})" for t in engine.describe_plan(fp16_net)["tensors"]]
        cache = b"TRT-8601-EntropyCalibration2\n" + b"".join(f"{nm}: {struct.unpack('<I', struct.pack('<f', 0.05))[0]:08x}\n".encode() for nm in names)
        net.set_int8_calibrator(calibrator.Calibrator(cache=cache))
    plan = net.build()
    net.close()
    return plan


def test_toy_networks_second_reader_and_int8_are_not_marked():
    assert _marked(_ops(_toy())) == [1]
    assert _marked(_ops(_toy(second_reader=True))) == []
    low8 = _ops(_toy(int8=True))
    assert _marked(low8) == [] and any(o.get("i8", [0])[0] for o in low8 if o["kind"] == "conv"), "the int8 toy must really run a convolution in int8"
