// Index arithmetic of the fused bottleneck pair kernel (conv_bneck_pair.hip): which tile a workgroup works on, which 16-byte chunk of the input patch a
// thread stages, which pixel of the intermediate a lane of a 16-pixel MFMA group computes, where its operands lie in the LDS patch, where its four
// channels land in the LDS image of the intermediate, where a fragment lane of the second convolution reads its 16 bytes, which output channel a
// weight-fragment row holds and which pixel / channels a lane stores after the half-wave swap.  Plain integer functions, usable from host code:
// tests/test_bneck_pair_cpu.py compiles this header with g++ and replays the kernel's data path lane by lane (patch -> first-convolution groups -> LDS
// image -> fragments -> v_mfma_f32_16x16x32_f16 semantics -> epilogue) against a direct convolution of both layers.  The kernel calls exactly these.
//
// Geometry.  Both layers are 3x3, stride 1, pad 1 over 16 channels.  An output tile is kTH x kTW = 8 x 16 pixels of one image: wave w owns tile rows
// 2w and 2w + 1, one 16-pixel fragment each.  The intermediate REGION the tile reads is kRH x kRW = 10 x 18 pixels starting at (y0 - 1, x0 - 1); the
// input PATCH under it is kPH x kPW = 12 x 20 pixels starting at (y0 - 2, x0 - 2).
// LDS layouts.  Patch and image alike: one PLANE per 8-channel chunk, 16 bytes per pixel, rows of kPW = 20 pixels, plane stride a multiple of 256
// bytes.  The first convolution walks the region as a LINEAR list over rows of 20 (two dead columns per row, kept so that the 16 pixels of a group
// are 16 CONSECUTIVE 16-byte slots for every tap); the second convolution's 16 pixels are a tile row.  A ds_read_b128 lane group (two half-rows of
// 8 lanes, one per chunk of one tap) then covers 8 + 8 different slots of one 256-byte window: conflict-free without an XOR key.
#pragma once

#if defined(__HIPCC__)
#define TRTX_HD __host__ __device__ __forceinline__
#else
#define TRTX_HD inline
#endif

namespace trtx {
namespace bneckidx {

constexpr int kTH = 8, kTW = 16;                        // output tile
constexpr int kRH = kTH + 2, kRW = kTW + 2;             // intermediate region: 10 x 18
constexpr int kPH = kTH + 4, kPW = kTW + 4;             // input patch: 12 x 20 pixels
constexpr int kRegionLin = (kRH - 1) * kPW + kRW;       // linear region elements over rows of kPW: 198
constexpr int kGroups = (kRegionLin + 15) / 16;         // 13 MFMA groups of 16 region elements
constexpr int kPatchPixels = kPH * kPW;                 // 240
constexpr int kPatchChunks = 2 * kPatchPixels;          // 16-byte chunks of a patch: 480
constexpr int kFetch = (kPatchChunks + 255) / 256;      // chunks a thread stages: 2
constexpr int kPatchPlane = (kPatchPixels * 16 + 255) / 256 * 256;    // 3840
constexpr int kPatchBytes = 2 * kPatchPlane;                          // 7680, double-buffered by the kernel
constexpr int kImagePlane = (kRH * kPW * 16 + 255) / 256 * 256;       // 3328
constexpr int kImageBytes = 2 * kImagePlane;                          // 6656
constexpr int kLdsBytes = 2 * kPatchBytes + kImageBytes;              // 22 016
constexpr int kTaps = 9, kSteps = 5;                    // k = tap * 16 + c, five 32-wide k-steps, tap 9 is zero
static_assert(kPatchPixels % 8 == 0, "patch chunks are staged in runs of 8 pixels per plane");

// tiles along x, then y, then images
struct Tile {
    int n, y0, x0;
};
TRTX_HD Tile tile_of(int tile, int tiles_x, int tiles_y) {
    Tile t;
    const int tx = tile % tiles_x;
    const int rest = tile / tiles_x;
    t.x0 = tx * kTW;
    t.y0 = (rest % tiles_y) * kTH;
    t.n = rest / tiles_y;
    return t;
}
// workgroup `wg` of `grid` walks the contiguous run [first, first + count) of `total` tiles
TRTX_HD int run_length(int total, int grid) { return (total + grid - 1) / grid; }
TRTX_HD int run_first(int wg, int total, int grid) { return wg * run_length(total, grid); }

// Patch fill.  Chunk c (< kPatchChunks; thread t stages chunks t, t + 256, ...) is the 8 channels `plane` of patch pixel (py, px): 16 chunks = 8
// consecutive pixels x 2 planes, so that 8 consecutive lanes write 128 consecutive LDS bytes and 16 lanes read 8 whole pixels (32 bytes each).
struct PatchChunk {
    int py, px, plane;
};
TRTX_HD PatchChunk patch_chunk(int c) {
    const int j = c & 15;
    const int pix = (c >> 4) * 8 + (j & 7);
    PatchChunk p;
    p.plane = j >> 3;
    p.py = pix / kPW;
    p.px = pix - p.py * kPW;
    return p;
}
// byte offset inside a patch buffer of the 8-channel chunk `plane` of patch pixel (py, px)
TRTX_HD int patch_offset(int py, int px, int plane) { return plane * kPatchPlane + (py * kPW + px) * 16; }
// byte offset inside the image of channel `ch` of region pixel (ry, rx)
TRTX_HD int image_offset(int ry, int rx, int ch) { return (ch >> 3) * kImagePlane + (ry * kPW + rx) * 16 + (ch & 7) * 2; }

// First convolution.  Lane `lane` of group `group` computes region element e = 16 group + (lane & 15) of the linear list: row e / 20, column
// e % 20.  Columns 18 and 19 and e >= kRegionLin compute (the tail on the element 16 before it) and store nothing.
struct RegionPixel {
    int ry, rx;
    bool live;
};
TRTX_HD RegionPixel region_pixel(int group, int lane) {
    const int e = group * 16 + (lane & 15);
    const int ee = e < kRegionLin ? e : e - 16;   // (the element one group back: the same 16-byte slot of the 256-byte window, so the tail adds no bank conflict)
    RegionPixel r;
    r.ry = ee / kPW;
    r.rx = ee - r.ry * kPW;
    r.live = e < kRegionLin && r.rx < kRW;
    return r;
}
// In k-step `kt`, lane group g = lane >> 4 supplies k = 32 kt + 8 g + [0, 8): filter tap 2 kt + (g >> 1), channels 8 (g & 1) + [0, 8) -
// conv_igemm_tile's two-taps-per-step placement (CinK == 16).  Tap 9 does not exist: the operand is zero.
TRTX_HD int step_tap(int kt, int lane) { return 2 * kt + ((lane >> 4) >> 1); }
TRTX_HD int step_chunk(int lane) { return (lane >> 4) & 1; }
// 16 bytes of region pixel (ry, rx) of the first convolution for tap `tap` (< 9), chunk `chunk`: inside a patch buffer
TRTX_HD int frag1_offset(int ry, int rx, int tap, int chunk) {
    const int r = tap / 3, q = tap - r * 3;
    return patch_offset(ry + r, rx + q, chunk);
}
// ... and of tile pixel (oy, ox) of the second convolution: inside the image
TRTX_HD int frag2_offset(int oy, int ox, int tap, int chunk) {
    const int r = tap / 3, q = tap - r * 3;
    return image_offset(oy + r, ox + q, chunk * 8);
}
// Row `a` (= lane & 15 on the weight side) of the weight fragment holds this output channel: the accumulator rows 4 g + [0, 4) of lane group g are
// then channels lane_channel(g) + [0, 4) = {0, 8, 4, 12}[g] + [0, 4), so that exchanging the upper half-wave of tile row 2w with the lower half-wave of
// tile row 2w + 1 (v_permlane32_swap) leaves every lane with 8 consecutive channels of one pixel = one 16-byte store
TRTX_HD int lane_channel(int g) { return 8 * (g & 1) + 4 * (g >> 1); }
TRTX_HD int weight_row_channel(int a) { return lane_channel(a >> 2) + (a & 3); }
// after the swap lane `lane` of wave `wave` stores channels store_channel + [0, 8) of tile pixel (store_row, lane & 15); the same 16 bytes of the input
// patch, two pixels down and right, are its shortcut
TRTX_HD int store_row(int wave, int lane) { return 2 * wave + (lane >> 5); }
TRTX_HD int store_channel(int lane) { return 8 * ((lane >> 4) & 1); }
TRTX_HD int shortcut_offset(int wave, int lane) { return patch_offset(store_row(wave, lane) + 2, (lane & 15) + 2, (lane >> 4) & 1); }

}  // namespace bneckidx
}  // namespace trtx
