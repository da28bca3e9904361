// Index arithmetic of the fused stem pair kernel (conv_stem_pair.hip): which stem pixel a lane of a 16-pixel MFMA group computes, where its
// taps lie in the fp32 input patch, where its four channels land in the LDS image of the intermediate, where a fragment lane of the second
// convolution reads its 16 bytes, which output channel a weight-fragment row holds.  Plain integer functions, usable from host code:
// tests/test_stem_pair_cpu.py compiles this header with g++ and replays the kernel's data path lane by lane (patch -> stem groups -> LDS image ->
// fragments -> v_mfma_f32_16x16x32_f16 semantics) against a direct convolution of both layers.  The kernel calls exactly these functions.
//
// Geometry.  Both layers are 3x3, stride 2, pad 1.  An output tile of the second layer is kTH x kTW = 8 x 16 pixels of one image: wave w owns
// tile rows 2w and 2w + 1, one 16-pixel fragment each.  The intermediate REGION the tile reads is kRH x kRW = 17 x 33 stem pixels starting at
// (2 y0 - 1, 2 x0 - 1); the fp32 input patch under that region is 35 rows x 67 columns per channel starting at (4 y0 - 3, 4 x0 - 3), staged
// with the column start floored to a multiple of 4 floats (16-byte DMA chunks) and a row pitch of kPCA = 72 floats.
// LDS image of the region: 32 bytes per pixel (16 fp16 channels), even and odd region columns in separate half-rows of kHalf = 17 pixels - a
// fragment lane of tap column q reads region column 2 ox + q, so the 16 pixels of a fragment are CONSECUTIVE 32-byte slots and the four lane
// groups of a ds_read_b128 (two taps x two 8-channel chunks) cover whole 512-byte runs: conflict-free without an XOR key.
#pragma once

#if defined(__HIPCC__)
#define TRTX_HD __host__ __device__ __forceinline__
#else
#define TRTX_HD inline
#endif

namespace trtx {
namespace pairidx {

constexpr int kTH = 8, kTW = 16;                       // output tile of the second convolution
constexpr int kRH = 2 * kTH + 1, kRW = 2 * kTW + 1;    // intermediate region: 17 x 33 stem pixels
constexpr int kRegion = kRH * kRW;                     // 561
constexpr int kGroups = (kRegion + 15) / 16;           // 36 MFMA groups of 16 stem pixels = 9 per wave
constexpr int kPR = 2 * kRH + 1;                       // input patch rows per channel: 35
constexpr int kPC = 2 * kRW + 1;                       // input patch columns the taps touch: 67
constexpr int kPCA = (kPC + 3 + 3) / 4 * 4;            // staged row pitch in floats, with up to 3 floats of alignment slack: 72
constexpr int kHalf = (kRW + 1) / 2;                   // pixels per parity half-row of the LDS image: 17
constexpr int kPixelBytes = 32;                        // 16 fp16 channels
constexpr int kImageBytes = kRH * 2 * kHalf * kPixelBytes;   // 18 496
constexpr int kTaps = 9, kSteps = 5;                   // k = tap * 16 + c, five 32-wide k-steps, tap 9 is zero

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
// first region pixel (intermediate coordinates) and first patch pixel (input coordinates) of a tile; both may be negative
TRTX_HD int region_start(int o0) { return 2 * o0 - 1; }
TRTX_HD int patch_start(int o0) { return 4 * o0 - 3; }
TRTX_HD int patch_aligned_start(int wi_start) { return (wi_start >= 0 ? wi_start : wi_start - 3) / 4 * 4; }   // floor to a multiple of 4

// Stem side.  Lane `lane` of group `group` computes region pixel e = 16 group + (lane & 15), row-major over the region; e >= kRegion (the
// last group's tail) computes a clamped pixel and stores nothing.
struct RegionPixel {
    int ry, rx;
    bool live;
};
TRTX_HD RegionPixel region_pixel(int group, int lane) {
    const int e = group * 16 + (lane & 15);
    RegionPixel r;
    r.live = e < kRegion;
    const int ee = r.live ? e : kRegion - 1;
    r.ry = ee / kRW;
    r.rx = ee - r.ry * kRW;
    return r;
}
// float index inside a channel plane of the patch of the top-left tap of region pixel (ry, rx); `shift` = wi_start - aligned start
TRTX_HD int patch_offset(int ry, int rx, int shift) { return 2 * ry * kPCA + 2 * rx + shift; }
// byte offset in the LDS image of channel `ch` of region pixel (ry, rx)
TRTX_HD int image_offset(int ry, int rx, int ch) { return ((ry * 2 + (rx & 1)) * kHalf + (rx >> 1)) * kPixelBytes + ch * 2; }

// Second convolution.  In k-step `kt`, lane group g = lane >> 4 supplies k = 32 kt + 8 g + [0, 8): filter tap 2 kt + (g >> 1), channels
// 8 (g & 1) + [0, 8) - conv_igemm_tile's two-taps-per-step placement (CinK == 16).  Tap 9 does not exist: the operand is zero.
TRTX_HD int step_tap(int kt, int lane) { return 2 * kt + ((lane >> 4) >> 1); }
TRTX_HD int step_chunk(int lane) { return (lane >> 4) & 1; }
// 16 bytes of tile pixel (oy, ox) for tap `tap` (< 9), 8-channel chunk `chunk`
TRTX_HD int frag_offset(int oy, int ox, int tap, int chunk) {
    const int r = tap / 3, q = tap - r * 3;
    return image_offset(2 * oy + r, 2 * ox + q, chunk * 8);
}
// Row `a` (= lane & 15 on the weight side) of weight fragment j (0, 1) holds this output channel: the accumulator rows 4 g + [0, 4) of a
// lane are then channels 8 g + 4 j + [0, 4), so the two fragments of a lane are 8 consecutive channels = one 16-byte store
TRTX_HD int weight_row_channel(int j, int a) { return 8 * (a >> 2) + 4 * j + (a & 3); }

}  // namespace pairidx
}  // namespace trtx
