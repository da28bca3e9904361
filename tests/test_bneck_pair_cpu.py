"""The fused bottleneck pair (tensorrtx_amd/csrc/kernels/conv_bneck_pair.hip) on the CPU.

1. Its index arithmetic (kernels/bneck_pair_index.h, compiled with g++ as it stands - the kernel calls the same functions) replayed lane by lane for every
   shape of the GPU test: patch fill (two buffers, a workgroup's run of tiles) -> 13 first-convolution groups of 16 region elements -> LDS image of the
   intermediate (zeros outside the image) -> the second convolution's fragments -> v_mfma_f32_16x16x32_f16 semantics -> the half-wave swap -> shortcut from
   the patch -> 8 consecutive channels per lane, against a NumPy direct convolution of both layers.  What this file mirrors by hand are the few lines of
   the kernel that are not index functions: the bounds tests (outside -> zero), the lane exchange of v_permlane32_swap and the order of the epilogue.
   Along the way: every LDS byte a fragment reads was written (NaN sentinel), every output pixel is written exactly once, and every ds_read_b128 is
   conflict-free under the lane groups the LDS serves it in.
2. The plan pass (plan_passes.cpp mark_bneck_pair): which plans carry the mark."""
import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tensorrtx_amd import engine
from util import synth_wts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "tensorrtx_amd", "csrc", "kernels")

SHIM = r"""
#include "bneck_pair_index.h"
using namespace trtx::bneckidx;
extern "C" {
void c_consts(int* o) { o[0] = kTH; o[1] = kTW; o[2] = kRH; o[3] = kRW; o[4] = kPH; o[5] = kPW; o[6] = kGroups; o[7] = kPatchChunks; o[8] = kFetch;
                        o[9] = kPatchBytes; o[10] = kImageBytes; o[11] = kLdsBytes; o[12] = kSteps; o[13] = kTaps; o[14] = kRegionLin; }
void c_tile_of(int tile, int tiles_x, int tiles_y, int* o) { Tile t = tile_of(tile, tiles_x, tiles_y); o[0] = t.n; o[1] = t.y0; o[2] = t.x0; }
int c_run_length(int total, int grid) { return run_length(total, grid); }
int c_run_first(int wg, int total, int grid) { return run_first(wg, total, grid); }
void c_patch_chunk(int c, int* o) { PatchChunk p = patch_chunk(c); o[0] = p.py; o[1] = p.px; o[2] = p.plane; }
int c_patch_offset(int py, int px, int plane) { return patch_offset(py, px, plane); }
int c_image_offset(int ry, int rx, int ch) { return image_offset(ry, rx, ch); }
void c_region_pixel(int group, int lane, int* o) { RegionPixel r = region_pixel(group, lane); o[0] = r.ry; o[1] = r.rx; o[2] = r.live; }
int c_step_tap(int kt, int lane) { return step_tap(kt, lane); }
int c_step_chunk(int lane) { return step_chunk(lane); }
int c_frag1_offset(int ry, int rx, int tap, int chunk) { return frag1_offset(ry, rx, tap, chunk); }
int c_frag2_offset(int oy, int ox, int tap, int chunk) { return frag2_offset(oy, ox, tap, chunk); }
int c_lane_channel(int g) { return lane_channel(g); }
int c_weight_row_channel(int a) { return weight_row_channel(a); }
int c_store_row(int wave, int lane) { return store_row(wave, lane); }
int c_store_channel(int lane) { return store_channel(lane); }
int c_shortcut_offset(int wave, int lane) { return shortcut_offset(wave, lane); }
}
"""

# the GPU test's shapes (tests/test_gpu_bneck_pair.py), tile 8 x 16: one partial tile; exact tiles; ragged in both directions; one row and one column past a tile
SHAPES = [(1, 5, 6), (2, 16, 32), (3, 19, 35), (2, 9, 17)]
# ds_read_b128: the four lane groups the LDS serves one cycle each; bank of byte address a = (a / 4) mod 64
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)), list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


class Tables:
    """every index function over its whole domain, once"""

    def __init__(self, L):
        c = (ctypes.c_int * 15)()
        L.c_consts(c)
        (self.TH, self.TW, self.RH, self.RW, self.PH, self.PW, self.G, self.CHUNKS, self.FETCH, self.PATCH, self.IMG, self.LDS, self.STEPS, self.TAPS,
         self.RLIN) = list(c)
        o = (ctypes.c_int * 3)()
        self.chunk = np.zeros((self.CHUNKS, 3), np.int64)
        for i in range(self.CHUNKS):
            L.c_patch_chunk(i, o)
            self.chunk[i] = list(o)
        self.chunk_off = np.array([L.c_patch_offset(int(py), int(px), int(pl)) for py, px, pl in self.chunk])
        self.rp = np.zeros((self.G, 64, 3), np.int64)
        for g in range(self.G):
            for ln in range(64):
                L.c_region_pixel(g, ln, o)
                self.rp[g, ln] = list(o)
        self.tap = np.array([[L.c_step_tap(kt, ln) for ln in range(64)] for kt in range(self.STEPS)])
        self.chk = np.array([L.c_step_chunk(ln) for ln in range(64)])
        self.lane_ch = np.array([L.c_lane_channel(ln >> 4) for ln in range(64)])
        # byte offsets of the fragment reads, -1 where the tap does not exist (no read is issued: the operand is zero)
        self.f1 = np.full((self.G, self.STEPS, 64), -1, np.int64)
        for g in range(self.G):
            for kt in range(self.STEPS):
                for ln in range(64):
                    if self.tap[kt, ln] < self.TAPS:
                        self.f1[g, kt, ln] = L.c_frag1_offset(int(self.rp[g, ln, 0]), int(self.rp[g, ln, 1]), int(self.tap[kt, ln]), int(self.chk[ln]))
        self.f2 = np.full((4, 2, self.STEPS, 64), -1, np.int64)
        for wv in range(4):
            for i in range(2):
                for kt in range(self.STEPS):
                    for ln in range(64):
                        if self.tap[kt, ln] < self.TAPS:
                            self.f2[wv, i, kt, ln] = L.c_frag2_offset(2 * wv + i, ln & 15, int(self.tap[kt, ln]), int(self.chk[ln]))
        self.img_off = np.array([[L.c_image_offset(int(self.rp[g, ln, 0]), int(self.rp[g, ln, 1]), int(self.lane_ch[ln])) for ln in range(64)] for g in range(self.G)])
        self.wrow = np.array([L.c_weight_row_channel(a) for a in range(16)])
        self.store_row = np.array([[L.c_store_row(wv, ln) for ln in range(64)] for wv in range(4)])
        self.store_ch = np.array([L.c_store_channel(ln) for ln in range(64)])
        self.short_off = np.array([[L.c_shortcut_offset(wv, ln) for ln in range(64)] for wv in range(4)])


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "shim.cpp")
        open(src, "w").write(SHIM)
        so = os.path.join(tmp, "shim.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{HDR}", src, "-o", so])
        yield ctypes.CDLL(so)


@pytest.fixture(scope="module")
def tables(shim):
    return Tables(shim)


def _silu(v):
    return v / (1.0 + np.exp(-v))


def _conv_s1(x, w, b):
    """x [N,H,W,C], w [Co,C,3,3], b [Co], float64: 3x3 stride 1 pad 1, SiLU"""
    N, H, W, C = x.shape
    xp = np.zeros((N, H + 2, W + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.zeros((N, H, W, w.shape[0])) + b
    for r in range(3):
        for q in range(3):
            out += np.einsum("nhwc,oc->nhwo", xp[:, r:r + H, q:q + W], w[:, :, r, q].astype(np.float64))
    return _silu(out)


def _conflict_free(offsets):
    """offsets: the 64 lanes' byte addresses of one ds_read_b128 (-1: lane not reading).  Within a lane group two DIFFERENT addresses may not share a bank."""
    for grp in B128_GROUPS:
        owner = {}
        for a in {int(offsets[ln]) for ln in grp if offsets[ln] >= 0}:
            assert a % 16 == 0
            for j in range(4):
                bank = (a // 4 + j) % 64
                if owner.setdefault(bank, a) != a:
                    return False
    return True


def test_index_functions_cover_their_ranges(shim, tables):
    L, T = shim, tables
    assert (T.TH, T.TW) in ((8, 16), (16, 16)) and (T.RH, T.RW, T.PH, T.PW) == (T.TH + 2, T.TW + 2, T.TH + 4, T.TW + 4)
    assert T.G * 16 >= T.RLIN > (T.G - 1) * 16 and T.FETCH * 256 >= T.CHUNKS and T.LDS == 2 * T.PATCH + T.IMG and T.LDS <= 32 * 1024
    # the patch: the chunks tile both planes of every patch pixel exactly once, 16-byte aligned, inside a buffer
    assert sorted(map(tuple, T.chunk)) == sorted((py, px, pl) for py in range(T.PH) for px in range(T.PW) for pl in (0, 1))
    assert len(set(T.chunk_off)) == T.CHUNKS and T.chunk_off.min() == 0 and T.chunk_off.max() + 16 <= T.PATCH and not (T.chunk_off % 16).any()
    # 8 consecutive lanes of the fill write 128 consecutive bytes (one ds_write_b128 lane group)
    for c0 in range(0, T.CHUNKS, 8):
        assert list(T.chunk_off[c0:c0 + 8]) == list(range(T.chunk_off[c0], T.chunk_off[c0] + 128, 16))
    # the region: every region pixel is computed by exactly one live lane column; dead lanes stay inside the region rows
    live = [(int(ry), int(rx)) for g in range(T.G) for ry, rx, lv in T.rp[g, :16] if lv]
    assert sorted(live) == [(ry, rx) for ry in range(T.RH) for rx in range(T.RW)]
    assert T.rp[..., 0].max() < T.RH and T.rp[..., 1].max() < T.PW and (T.rp[:, :16] == T.rp[:, 16:32]).all() and (T.rp[:, :16] == T.rp[:, 48:]).all()
    # the image: the 8-byte pieces of all region pixels tile it without overlap, inside kImageBytes
    offs = sorted(L.c_image_offset(ry, rx, ch) for ry in range(T.RH) for rx in range(T.RW) for ch in (0, 4, 8, 12))
    assert len(set(offs)) == len(offs) and offs[0] == 0 and offs[-1] + 8 <= T.IMG and all(v % 8 == 0 for v in offs)
    # every fragment read stays inside its buffer
    assert T.f1.max() + 16 <= T.PATCH and T.f2.max() + 16 <= T.IMG and T.short_off.max() + 16 <= T.PATCH
    # k-step placement: k = 32 kt + 8 (lane >> 4) + e is tap k // 16, channel k % 16
    for kt in range(T.STEPS):
        for ln in range(64):
            k0 = 32 * kt + 8 * (ln >> 4)
            assert T.tap[kt, ln] == k0 // 16 and T.chk[ln] * 8 == k0 % 16
    # a lane's accumulator rows 4g + e are channels lane_channel(g) + e; the weight rows are a permutation of the 16 channels
    assert sorted(T.wrow) == list(range(16))
    for g in range(4):
        assert [T.wrow[4 * g + e] for e in range(4)] == [L.c_lane_channel(g) + e for e in range(4)]
    # after the swap: a lower-half lane joins its own 4 channels with those of the lane 32 above, an upper-half lane those of the lane 32 below with its own
    for ln in range(32):
        assert T.lane_ch[ln] == T.store_ch[ln] and T.lane_ch[ln + 32] == T.store_ch[ln] + 4 and T.store_ch[ln + 32] == T.store_ch[ln]
    # runs: contiguous, covering, nothing twice
    for total, grid in ((1, 1), (7, 3), (27, 4), (6400, 1600), (6400, 2048), (10, 10)):
        per = L.c_run_length(total, grid)
        got = [t for wg in range(grid) for t in range(L.c_run_first(wg, total, grid), min(total, L.c_run_first(wg, total, grid) + per))]
        assert got == list(range(total))


def test_fragment_reads_are_conflict_free(tables):
    T = tables
    for g in range(T.G):
        for kt in range(T.STEPS):
            assert _conflict_free(T.f1[g, kt]), ("first convolution", g, kt)
    for wv in range(4):
        for i in range(2):
            for kt in range(T.STEPS):
                assert _conflict_free(T.f2[wv, i, kt]), ("second convolution", wv, i, kt)
        assert _conflict_free(T.short_off[wv]), ("shortcut", wv)
    # (the checker does see a conflict: two pixels 256 bytes apart in one lane group)
    bad = np.full(64, -1)
    bad[0], bad[1] = 0, 256
    assert not _conflict_free(bad)


@pytest.mark.parametrize("shortcut", [True, False])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_lane_level_replay_of_the_pair_kernel_is_the_two_convolutions(shim, tables, N, H, W, shortcut):
    L, T = shim, tables
    rng = np.random.default_rng(N * 1000 + H)
    LD, COFF = 48, 16                                               # the real plan's aliasing: channels 16 .. 31 of a 48-wide buffer
    buf = rng.standard_normal((N, H, W, LD)).astype(np.float16)
    x = buf[..., COFF:COFF + 16]
    w0 = (rng.standard_normal((16, 16, 3, 3)) * (2.0 / 144) ** 0.5).astype(np.float16)
    b0 = rng.standard_normal(16).astype(np.float32) * 0.5
    w1 = (rng.standard_normal((16, 16, 3, 3)) * (2.0 / 144) ** 0.5).astype(np.float16)
    b1 = rng.standard_normal(16).astype(np.float32) * 0.5
    # reference: both layers in float64, the intermediate and the second layer's activation rounded to fp16 as the two launches store them
    mid_ref = _conv_s1(x.astype(np.float64), w0, b0.astype(np.float64)).astype(np.float16)
    ref = _conv_s1(mid_ref.astype(np.float64), w1, b1.astype(np.float64)).astype(np.float16).astype(np.float64)
    if shortcut:
        ref = ref + x.astype(np.float64)

    def pack(w):                                                   # [Cout_pad 16][Kpad 160], k = tap * 16 + c
        p = np.zeros((16, 160), np.float16)
        for r in range(3):
            for q in range(3):
                p[:, (r * 3 + q) * 16:(r * 3 + q) * 16 + 16] = w[:, :, r, q]
        return p.astype(np.float32)
    A0, A1 = pack(w0)[T.wrow], pack(w1)[T.wrow]                    # fragment row a holds channel wrow[a]
    lanes = np.arange(64)
    grp, col = lanes >> 4, lanes & 15
    tiles_x, tiles_y = (W + T.TW - 1) // T.TW, (H + T.TH - 1) // T.TH
    total = N * tiles_x * tiles_y
    grid = min(total, 3)                                           # runs of several tiles, crossing rows and images
    per = L.c_run_length(total, grid)
    out = np.full((N, H, W, 16), np.nan, np.float32)
    writes = np.zeros((N, H, W, 16), np.int64)
    o3 = (ctypes.c_int * 3)()
    NANH = np.float16(np.nan)

    def read8(mem, offs):                                          # [64 lanes][8 halfs] at byte offsets; lanes with offset -1 read nothing: zeros
        idx = np.where(offs >= 0, offs, 0)[:, None] // 2 + np.arange(8)[None, :]
        v = mem[idx].astype(np.float32)
        v[offs < 0] = 0.0
        return v

    def mfma(A, Bl, acc):                                          # A [16 rows][32 k]; Bl [64 lanes][8]: lane (g, col) holds k = 8 g + [0, 8) of pixel col
        B = np.zeros((16, 32), np.float32)
        for g in range(4):
            B[:, 8 * g:8 * g + 8] = Bl[16 * g:16 * g + 16]
        return acc + A @ B.T                                       # [row][pixel]

    for wg in range(grid):
        lds = np.full(T.LDS // 2, NANH)
        first = L.c_run_first(wg, total, grid)
        for it, tile in enumerate(range(first, min(total, first + per))):
            L.c_tile_of(tile, tiles_x, tiles_y, o3)
            n, y0, x0 = list(o3)
            p0 = (it & 1) * T.PATCH // 2                            # this tile's patch buffer (half index)
            patch = lds[p0:p0 + T.PATCH // 2]
            img = lds[T.PATCH:T.PATCH + T.IMG // 2]
            patch[:] = NANH                                         # whatever an earlier tile left there must not be read
            img[:] = NANH
            # fetch + land (mirrored): chunk (py, px, plane) = input pixel (y0 - 2 + py, x0 - 2 + px), zeros outside the image
            for (py, px, pl), off in zip(T.chunk, T.chunk_off):
                y, xx = y0 - 2 + py, x0 - 2 + px
                v = x[n, y, xx, 8 * pl:8 * pl + 8] if 0 <= y < H and 0 <= xx < W else np.zeros(8, np.float16)
                patch[off // 2:off // 2 + 8] = v
            # first convolution: group g, lanes (grp, col); rows 4 grp + e of the accumulator are this lane's channels lane_ch + e
            for g in range(T.G):
                acc = np.zeros((16, 16), np.float32)
                for kt in range(T.STEPS):
                    Bl = read8(patch, T.f1[g, kt])
                    assert not np.isnan(Bl).any(), "the first convolution read a patch byte nobody wrote"
                    acc = mfma(A0[:, 32 * kt:32 * kt + 32], Bl, acc)
                for ln in lanes:
                    ry, rx, lv = (int(v) for v in T.rp[g, ln])
                    ch = int(T.lane_ch[ln])
                    v4 = _silu((acc[4 * grp[ln]:4 * grp[ln] + 4, col[ln]] + b0[ch:ch + 4]).astype(np.float64)).astype(np.float16)
                    iy, ix = y0 - 1 + ry, x0 - 1 + rx
                    if not (0 <= iy < H and 0 <= ix < W):
                        v4 = np.zeros(4, np.float16)                # the second convolution's padding, not a value of the first
                    if lv:
                        o = int(T.img_off[g, ln]) // 2
                        assert np.isnan(img[o:o + 4]).all(), "two lanes wrote one image slot"
                        img[o:o + 4] = v4
            # the image is the first layer inside the image and zero outside (1 fp16 ulp: fp32 sums here, float64 in the reference)
            for ry in range(T.RH):
                for rx in range(T.RW):
                    got = np.concatenate([img[L.c_image_offset(ry, rx, c8) // 2:][:8] for c8 in (0, 8)]).astype(np.float32)
                    iy, ix = y0 - 1 + ry, x0 - 1 + rx
                    if 0 <= iy < H and 0 <= ix < W:
                        want = mid_ref[n, iy, ix].astype(np.float32)
                        assert np.all(np.abs(got - want) <= 2.0 ** -10 * np.maximum(np.abs(want), 2.0 ** -14)), (tile, ry, rx)
                    else:
                        assert np.all(got == 0), (tile, ry, rx)
            # second convolution and epilogue: wave wv owns tile rows 2 wv, 2 wv + 1
            for wv in range(4):
                h = np.zeros((2, 64, 4), np.float16)
                for i in range(2):
                    acc = np.zeros((16, 16), np.float32)
                    for kt in range(T.STEPS):
                        Bl = read8(img, T.f2[wv, i, kt])
                        assert not np.isnan(Bl).any(), "the second convolution read an image byte nobody wrote"
                        acc = mfma(A1[:, 32 * kt:32 * kt + 32], Bl, acc)
                    for ln in lanes:
                        ch = int(T.lane_ch[ln])
                        h[i, ln] = _silu((acc[4 * grp[ln]:4 * grp[ln] + 4, col[ln]] + b1[ch:ch + 4]).astype(np.float64)).astype(np.float16)
                # v_permlane32_swap(row 2 wv, row 2 wv + 1): lanes 32-63 of the first operand <-> lanes 0-31 of the second
                v8 = np.zeros((64, 8), np.float16)
                v8[:32, :4], v8[:32, 4:] = h[0, :32], h[0, 32:]
                v8[32:, :4], v8[32:, 4:] = h[1, :32], h[1, 32:]
                if shortcut:
                    rv = read8(patch, T.short_off[wv])
                    assert not np.isnan(rv).any()
                    v8 = (v8.astype(np.float32) + rv).astype(np.float16)
                for ln in lanes:
                    y, xx, c0 = y0 + int(T.store_row[wv, ln]), x0 + int(col[ln]), int(T.store_ch[ln])
                    if y < H and xx < W:
                        out[n, y, xx, c0:c0 + 8] = v8[ln]
                        writes[n, y, xx, c0:c0 + 8] += 1
    assert (writes == 1).all(), "every output element is written exactly once"
    assert not np.isnan(out).any()
    if shortcut:                                                    # the shortcut the lanes read is the input at their own pixel and channels
        plain = _conv_s1(mid_ref.astype(np.float64), w1, b1.astype(np.float64))
        assert np.abs((out - x.astype(np.float32)) - plain).max() < 4e-3 * max(1.0, np.abs(ref).max())
    # 144 products of fp16 operands summed in fp32 (here) / float64 (reference), and an intermediate that may differ by 1 fp16 ulp per element
    err = np.abs(out - ref).max()
    assert err < 2e-3 * max(1.0, np.abs(ref).max()), err


# ---------------------------------------------------------------------------------------------------- the plan pass
def _ops(plan):
    return engine.describe_plan(plan, lowered=True)["ops"]


def _marked(ops):
    return [k for k, o in enumerate(ops) if o.get("bneck_pair")]


def test_yolov8n_at_benchmark_size_has_one_marked_op_and_the_switch_removes_it(monkeypatch):
    path, _ = synth_wts("yolov8n")
    plan = engine.build_plan("yolov8n", path, batch=32, h=640, w=640, fp16=1)
    on = _ops(plan)
    assert _marked(on) == [4]
    for k in (3, 4):
        assert on[k]["kind"] == "conv" and (on[k]["cin"], on[k]["cout"], on[k]["k"], on[k]["stride"], on[k]["hw_in"]) == (16, 16, [3, 3], [1, 1], [160, 160])
    assert not on[3]["residual"] and on[4]["residual"] and on[3]["ld_in"] == 48 and on[4]["ld_out"] == 48 and on[4]["in"][1] == on[3]["in"][0]
    assert [k for k, o in enumerate(on) if o.get("stem_pair")] == [1]
    monkeypatch.setenv("TRTX_BNECK_PAIR", "0")
    off = _ops(plan)
    assert _marked(off) == []
    # the mark is all that differs: op count, kinds, names
    assert len(on) == len(off) == 53 and [o["kind"] for o in on] == [o["kind"] for o in off] and [o.get("name") for o in on] == [o.get("name") for o in off]
    assert [{k: v for k, v in o.items() if k != "bneck_pair"} for o in on] == off


def test_other_precisions_are_not_marked():
    from tensorrtx_amd import calibrator
    path, _ = synth_wts("yolov8n")
    assert _marked(_ops(engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=0))) == []     # fp32 build
    plan16 = engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=1)
    assert _marked(_ops(plan16)) == [4]
    names = [t["name"] or f"(Unnamed Tensor* {t['id']})" for t in engine.describe_plan(plan16)["tensors"]]
    cache = b"TRT-8601-EntropyCalibration2\n" + b"".join(f"{n}: {struct.unpack('<I', struct.pack('<f', 0.05))[0]:08x}\n".encode() for n in names)
    with calibrator.Calibrator(cache=cache).installed():
        plan8 = engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=1, int8=1)
    assert engine.describe_plan(plan8)["int8"] is True and _marked(_ops(plan8)) == []


def _toy(ch=16, second_reader=False, mid_output=False, other_shortcut=False, shortcut=True, pointwise=False, hw=(32, 48)):
    """stem 3 -> ch 3x3/2, then the bottleneck: conv ch -> ch, conv ch -> ch (+ the bottleneck's input), then one more convolution; each with ReLU.
    pointwise: a 1x1 ch -> ch in front of the bottleneck, so that the pair's input is a tensor only the pair reads"""
    from tensorrtx_amd import builder
    rng = np.random.default_rng(5)
    net = builder.Network(max_batch=2, fp16=True)
    x = net.input("data", (3,) + tuple(hw))

    def conv(t, cin, cout, stride, k=3):
        w = rng.normal(0, 0.1, (cout, cin, k, k)).astype(np.float32)
        return net.out(net.activation(net.out(net.conv(t, w, bias=np.zeros(cout, np.float32), stride=stride, padding=k // 2)), "relu"))
    s = conv(x, 3, ch, 2)
    s = conv(s, ch, ch, 2)                       # (not the stem pair's 16 -> 32)
    if pointwise:
        s = conv(s, ch, ch, 1, k=1)
    mid = conv(s, ch, ch, 1)
    y = conv(mid, ch, ch, 1)
    if shortcut:
        y = net.out(net.elementwise(y, conv(x, 3, ch, 4, k=5) if other_shortcut else s))
    net.mark_output(conv(y, ch, 32, 1), "y")
    if second_reader:
        net.mark_output(conv(mid, ch, 32, 1), "z")
    if mid_output:
        net.mark_output(mid, "m")
    plan = net.build()
    net.close()
    return plan


def test_toy_networks():
    ops = _ops(_toy())
    m = _marked(ops)
    assert len(m) == 1 and ops[m[0]]["residual"] and ops[m[0]]["in"][0] == ops[m[0] - 1]["out"][0] and ops[m[0]]["in"][1] == ops[m[0] - 1]["in"][0]
    ops = _ops(_toy(shortcut=False))
    m = _marked(ops)
    assert len(m) == 1 and not ops[m[0]]["residual"]
    assert _marked(_ops(_toy(second_reader=True))) == []          # the tensor between the two has another reader
    assert _marked(_ops(_toy(mid_output=True))) == []             # ... or is an output of the network
    assert _marked(_ops(_toy(other_shortcut=True))) == []         # the shortcut comes from another tensor
    assert _marked(_ops(_toy(ch=32))) == []                       # a 32-channel pair


def test_a_marked_pair_never_gets_its_output_placed_on_its_input(monkeypatch):
    """Without a shortcut the first convolution is the only reader of the pair's input.  For two launches the arena may then put the second convolution's
    output on that input (the input is dead once the first launch is done); the fused launch reads the input while it writes the output, so for a marked
    pair the two blocks must be apart - and with the switch off the arena is free to share them again."""
    def blocks(plan):
        low = engine.describe_plan(plan, lowered=True)
        ops = low["ops"]
        m = _marked(ops)
        k = m[0] if m else next(j for j in range(1, len(ops)) if ops[j]["kind"] == "conv" and ops[j - 1]["kind"] == "conv" and
                                (ops[j]["cin"], ops[j]["cout"], ops[j]["k"]) == (16, 16, [3, 3]) == (ops[j - 1]["cin"], ops[j - 1]["cout"], ops[j - 1]["k"]))
        st = lambda t: low["storages"][low["tensors"][t]["storage"]]
        a, b = st(ops[k - 1]["in"][0]), st(ops[k]["out"][0])
        return m, a, b, a["offset"] < b["offset"] + b["bytes"] and b["offset"] < a["offset"] + a["bytes"]
    plan = _toy(shortcut=False, pointwise=True, hw=(96, 160))
    m, a, b, overlap = blocks(plan)
    assert len(m) == 1 and not overlap, (a, b)
    monkeypatch.setenv("TRTX_BNECK_PAIR", "0")
    m, a, b, overlap = blocks(plan)
    assert m == [] and overlap, "the two-launch form of this network is expected to run the pair in place: otherwise this test shows nothing"
