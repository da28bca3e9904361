// Grouped 3x3 convolution with MANY NARROW groups on the matrix pipe for gfx950 (MI355X): the sixteen 3x3 layers of ResNeXt-50 32x4d
// (resnet/resnext50_32x4d.cpp:111-154: setNbGroups(32) over 128, 256, 512 and 1024 channels = 4, 8, 16 and 32 channels per group, the first block
// of stages 2 - 4 at stride 2).  conv_grouped.hip keeps a whole layer's filter in one workgroup's registers (2 - 8 wide groups, Cout <= 128); here a
// layer has up to 590 KB of filter and groups that fill a quarter of an MFMA row, and it is bound by bandwidth (18 real FLOP per byte at 4 per group).
//
// Scope (conv_slab_supported): fp16 NHWC in / out / residual; Cin == Cout == C, C / groups in {4, 8, 16, 32}, C a multiple of 16; 3x3, pad 1, no
// dilation, stride 1 or 2 (both axes); channel strides multiples of 8 halves, pointers 16-byte aligned; no cap on C or on the group count.
//
// Slabs.  A slab is S = max(16, C / groups) consecutive channels: 16 / cg whole groups (cg <= 16) or one group (cg = 32); its S outputs read exactly
// its S inputs.  The packed filter is block-diagonal inside a slab: fp16 rows [C][Kpad], k = tap * S + c_local, Kpad = 9 S rounded up to 32 (160 / 288),
// zero wherever c_local lies outside the row's own group, BN scale folded before the one rounding (runtime/pack.cpp; for cg = 16 and 32 these are
// conv_grouped.hip's rows byte for byte).  K steps are v_mfma_f32_16x16x32_f16: two taps per step at S = 16 (the ninth tap's partner is zeros in the
// filter and in the A operand), one tap per step at S = 32.
//   DEVIATION: the block-diagonal zeros are multiplied, not skipped.  A non-finite input channel therefore makes the other outputs of its 16-channel
//   slab NaN (0 * inf), where the direct kernel confines the damage to the channel's own group.  Only cg = 4 and 8 have such zeros.
//
// Work split.  A workgroup of 4 waves owns a CHUNK of 64 channels (the last chunk of a layer: 16, 32 or 48; its idle waves skip the MFMAs, not the
// barriers) and walks tiles of 4 x 16 output pixels persistently: grid = walkers x chunks.  Wave w owns output unit w (16 channels) of the chunk and
// keeps that unit's filter rows in registers for the workgroup's lifetime (5 half8 per lane at S = 16, 9 at S = 32): weights are read once per
// workgroup, and a tile's channels are read by exactly one workgroup.
//
// A operand.  The chunk's halo patch (stride 1: 6 x 18 pixels, stride 2: 9 x 33) goes global -> VGPR -> LDS in 16-byte pieces, planes of 16 channels
// at 32 bytes per pixel: conv_grouped.hip's layout, in which each 16-lane group of a ds_read_b128 ({0-3, 12-15, 20-27} ...: every pixel index li once,
// the 16-byte half alternating with lane >> 4) reads slots 2 li + half of the 256-byte bank row, 16 distinct ones, for any run of 16 CONSECUTIVE pixel
// slots.  At stride 2 the 16 lanes of a fragment read every second column, which in that layout is slots 4 li + 2 q + half: a conflict.  So a stride-2
// patch row keeps its 17 even columns first and its 16 odd columns behind them (pixel slot = (px & 1) * 17 + (px >> 1)): tap column q of output
// column li is input column 2 li + q, of parity q & 1 at index li + (q >> 1), and the 16 lanes again read 16 consecutive slots of one half-row - the
// stride-1 argument holds unchanged.  The plane pitch is 64 mod 256 bytes, so that the eight pieces of a pixel (4 planes x 2 halves) and those of its
// neighbour start in 16 distinct slots when they are written.  Pixels outside the image are written as zeros and never loaded.
//   Pipeline: the next tile's pieces are loaded into registers before this tile's k-loop.  Stride 1 has two patch buffers and two staging tiles and ONE
//   barrier per tile (the pieces go to the other buffer behind the k-loop).  Stride 2 keeps ONE patch buffer and two barriers per tile: a second 9 x 33
//   buffer would make 85 KB of LDS and leave a workgroup alone on its CU; with one, both strides take 47 KB, three workgroups per CU.
//
// Output.  fp32 accumulation; bias -> act1 -> (+ residual) -> act2 in registers (act.h), ONE fp16 rounding, then an LDS staging tile (pitch 144 bytes:
// 16 consecutive rows start in distinct slots) so that the stores are row-major 16-byte chunks of the chunk's 128 bytes per pixel.  Ragged tiles and
// ragged chunks write nothing outside their view.  The summation order of an output (k-steps ascending, inside the MFMA) depends on neither the grid
// nor the tile: a layer returns the same bits at every batch and grid size.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../common.h"
#include "act.h"
#include "kernels.h"
#include "launch.h"

namespace trtx {
namespace {

constexpr int kRows = 4;              // 16-pixel fragments per tile = output rows of a tile
constexpr int kTilePx = kRows * 16;
constexpr int kChunk = 64;            // channels of a workgroup
constexpr int kStagePitch = kChunk * 2 + 16;
constexpr int kStageBytes = kTilePx * kStagePitch;
constexpr int kMaxGrid = 256 * 3;     // persistent workgroups: three per CU (LDS)

struct SlabGeom {
    int tiles_x, tiles_y, total_tiles;
    int chunks;
};

constexpr int slab_ph(int stride) { return (kRows - 1) * stride + 3; }
constexpr int slab_pw(int stride) { return 15 * stride + 3; }
// bytes of a 16-channel plane of the patch, padded to 64 mod 256
constexpr int slab_plane(int stride) { return (slab_ph(stride) * slab_pw(stride) * 32 + 191) / 256 * 256 + 64; }
constexpr int slab_lds_bytes(int stride) { return stride == 1 ? 2 * (4 * slab_plane(1) + kStageBytes) : 4 * slab_plane(2) + kStageBytes; }

// S: slab width (16 or 32); STRIDE: 1 or 2
template <int S, int STRIDE>
__global__ __launch_bounds__(256) void conv_slab_f16_kernel(const ConvArgs p, const SlabGeom g) {
    constexpr int KS = S == 16 ? 5 : 9, KPAD = KS * 32;
    constexpr int PH = slab_ph(STRIDE), PW = slab_pw(STRIDE), PLANE = slab_plane(STRIDE);
    constexpr int NBUF = STRIDE == 1 ? 2 : 1;
    constexpr int PIECES = PH * PW * 8, NPF = (PIECES + 255) / 256;   // 16-byte pieces of a 64-channel patch; per thread
    constexpr int ODD0 = (PW + 1) / 2;                                // stride 2: the first slot of a row's odd columns
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lj = lane >> 4;
    const int c0 = blockIdx.y * kChunk;                       // first channel of the chunk
    const int cc = min(kChunk, p.Cout - c0);                  // its channels: 16, 32, 48 or 64
    const int cpc = cc >> 3;                                  // 16-byte pieces of one of its pixels
    const bool live_wave = wave * 16 < cc;                    // wave-uniform
    char* patch = smem;
    char* stage = smem + NBUF * 4 * PLANE;

    const _Float16* __restrict__ in = static_cast<const _Float16*>(p.in) + c0;
    const _Float16* __restrict__ res = p.residual ? static_cast<const _Float16*>(p.residual) + c0 : nullptr;
    _Float16* __restrict__ out = static_cast<_Float16*>(p.out) + c0;

    // ---- the unit's filter rows -> registers, once: row (lane & 15), chunk (lane >> 4) of every k-step
    half8 breg[KS];
    const int u16 = live_wave ? wave * 16 : 0;
    {
        const _Float16* wr = static_cast<const _Float16*>(p.wgt) + (size_t)(c0 + u16 + li) * KPAD + lj * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) breg[ks] = *reinterpret_cast<const half8*>(wr + ks * 32);
    }
    const float4 bias4 = p.bias ? *reinterpret_cast<const float4*>(p.bias + c0 + u16 + lj * 4) : make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- per-lane A offsets inside the patch (tile independent), fragment 0: S = 16: step ks holds taps 2 ks and 2 ks + 1, the lane's chunk is channels
    // (lj & 1) * 8 .. of tap 2 ks + (lj >> 1) in plane `wave`; S = 32: step ks is tap ks, the lane's chunk is channels lj * 8 .. of the slab's two planes
    unsigned a_off[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        int tap = S == 16 ? 2 * ks + (lj >> 1) : ks;
        if (tap > 8) tap = 0;   // (the ninth tap's partner: read as zeros below)
        const int plane = S == 16 ? (u16 >> 4) : (u16 >> 5) * 2 + (lj >> 1);
        const int r = tap / 3, q = tap - 3 * r;
        const int slot = STRIDE == 1 ? r * PW + q + li : r * PW + (q & 1) * ODD0 + (q >> 1) + li;
        a_off[ks] = (unsigned)(plane * PLANE + slot * 32 + (lj & 1) * 16);
    }
    const bool tail_live = S == 32 || lj < 2;

    const bool second = res || p.act2 != ACT_NONE;
    const int tpi = g.tiles_x * g.tiles_y;
    half8 pf[NPF];   // the next tile's pieces

    // piece it = tid + 256 i of a patch: pixel it >> 3 (row-major in the PH x PW patch), 16-byte piece it & 7 of the chunk's channels
    auto fetch = [&](int tile) {
        const int n = tile / tpi, rem = tile - n * tpi, ty = rem / g.tiles_x;
        const int hi0 = ty * kRows * STRIDE - 1, wi0 = (rem - ty * g.tiles_x) * 16 * STRIDE - 1;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int it = tid + 256 * i, pp = it >> 3, c8 = it & 7;
            const int py = pp / PW, px = pp - py * PW;
            const int hi = hi0 + py, wi = wi0 + px;
            half8 v = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (it < PIECES && c8 < cpc && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
                v = *reinterpret_cast<const half8*>(in + (((long)n * p.H + hi) * p.W + wi) * p.ld_in + c8 * 8);
            pf[i] = v;
        }
    };
    auto put = [&](char* buf) {
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int it = tid + 256 * i, pp = it >> 3, c8 = it & 7;
            const int py = pp / PW, px = pp - py * PW;
            const int slot = STRIDE == 1 ? pp : py * PW + (px & 1) * ODD0 + (px >> 1);
            if (it < PIECES) *reinterpret_cast<half8*>(buf + (c8 >> 1) * PLANE + slot * 32 + (c8 & 1) * 16) = pf[i];
        }
    };

    int tile = blockIdx.x;
    if (tile >= g.total_tiles) return;   // (workgroup-uniform; the launcher starts no such workgroup)
    fetch(tile);
    put(patch);
    __syncthreads();
    int cur = 0;

    for (; tile < g.total_tiles; tile += gridDim.x) {
        const int n = tile / tpi, rem = tile - n * tpi, ty = rem / g.tiles_x;
        const int ho0 = ty * kRows, wo0 = (rem - ty * g.tiles_x) * 16;
        const bool has_next = tile + (int)gridDim.x < g.total_tiles;   // workgroup-uniform
        if (has_next) fetch(tile + gridDim.x);
        char* st = stage + (NBUF == 2 ? cur * kStageBytes : 0);

        if (live_wave) {
            const char* ab = patch + (NBUF == 2 ? cur * 4 * PLANE : 0);
            floatx4 acc[kRows];
#pragma unroll
            for (int f = 0; f < kRows; ++f) acc[f] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int f = 0; f < kRows; ++f) {
                    half8 a = *reinterpret_cast<const half8*>(ab + a_off[ks] + f * (STRIDE * PW * 32));
                    if constexpr (S == 16) {
                        if (ks == KS - 1 && !tail_live) a = half8{0, 0, 0, 0, 0, 0, 0, 0};
                    }
                    acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(breg[ks], a, acc[f], 0, 0, 0);
                }
            }
            // ---- epilogue: the lane holds channels ch .. ch + 3 (of the chunk) of pixel (lane & 15) of fragment f
            const int ch = u16 + lj * 4;
            const float b4[4] = {bias4.x, bias4.y, bias4.z, bias4.w};
#pragma unroll
            for (int f = 0; f < kRows; ++f) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = act_fast(acc[f][e] + b4[e], p.act1, p.alpha1);
                if (second) {
                    float r4[4] = {0.f, 0.f, 0.f, 0.f};
                    const int ho = ho0 + f, wo = wo0 + li;
                    if (res && ho < p.Ho && wo < p.Wo) {
                        const half4 rv = *reinterpret_cast<const half4*>(res + (((long)n * p.Ho + ho) * p.Wo + wo) * p.ld_res + ch);
#pragma unroll
                        for (int e = 0; e < 4; ++e) r4[e] = (float)rv[e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_fast(v[e] + r4[e], p.act2, p.alpha2);
                }
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = round_to_half(v[e]);
                *reinterpret_cast<half4*>(st + (f * 16 + li) * kStagePitch + ch * 2) = o;
            }
        }
        if constexpr (NBUF == 2) {
            // the other buffer's last reader was the previous tile's k-loop, which every wave left before the previous barrier
            if (has_next) put(patch + (cur ^ 1) * 4 * PLANE);
            __syncthreads();
        } else {
            __syncthreads();   // every wave has left the k-loop: the one buffer may be overwritten
            if (has_next) put(patch);
        }

        // ---- staging -> global, row-major: eight consecutive lanes store the 16-byte chunks of a pixel's channels
#pragma unroll
        for (int i = 0; i < kTilePx * 8 / 256; ++i) {
            const int it = tid + 256 * i, row = it >> 3, c8 = it & 7;
            const int ho = ho0 + (row >> 4), wo = wo0 + (row & 15);
            if (c8 < cpc && ho < p.Ho && wo < p.Wo)
                *reinterpret_cast<half8*>(out + (((long)n * p.Ho + ho) * p.Wo + wo) * p.ld_out + c8 * 8) = *reinterpret_cast<const half8*>(st + row * kStagePitch + c8 * 16);
        }
        if constexpr (NBUF == 2) {
            cur ^= 1;   // (this staging tile is written again two tiles on, behind the next tile's barrier, which follows the reads above)
        } else {
            __syncthreads();   // the patch is complete, and the staging tile has been read
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int S, int STRIDE>
int32_t launch_slab(const ConvArgs& a, const SlabGeom& g, hipStream_t s) {
    const int walkers = std::min(g.total_tiles, std::max(1, kMaxGrid / g.chunks));
    TRTX_LAUNCH((conv_slab_f16_kernel<S, STRIDE>), dim3(walkers, g.chunks), dim3(256), slab_lds_bytes(STRIDE), s, a, g);
    return check_launch("conv_slab_f16");
}

}  // namespace

int conv_slab_width(const ConvArgs& a) { return std::max(16, a.Cin / std::max(a.groups, 1)); }
int conv_slab_kpad(const ConvArgs& a) { return (9 * conv_slab_width(a) + 31) / 32 * 32; }

bool conv_slab_supported(const ConvArgs& a) {
    if (a.in_i8 || a.out_i8 || a.res_i8 || a.f32 || a.up_C != 0) return false;
    if (a.groups < 2 || a.Cin <= 0 || a.Cin != a.Cout || a.Cin % a.groups || a.Cin % 16) return false;
    const int cg = a.Cin / a.groups;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return false;
    if (a.kh != 3 || a.kw != 3 || a.pad_h != 1 || a.pad_w != 1 || a.dil_h != 1 || a.dil_w != 1) return false;
    const int st = a.stride_h;
    if ((st != 1 && st != 2) || a.stride_w != st || a.H < 1 || a.W < 1 || a.Ho != (a.H - 1) / st + 1 || a.Wo != (a.W - 1) / st + 1) return false;
    if (a.ld_in % 8 || a.ld_out % 8 || a.ld_in < a.Cin || a.ld_out < a.Cout) return false;
    if ((a.residual || a.ld_res) && (a.ld_res % 8 || a.ld_res < a.Cout)) return false;
    if ((a.Cout + kChunk - 1) / kChunk > 65535) return false;   // chunks are the grid's second axis
    // tile counts and pixel indices are ints
    return (long)a.N * a.H * a.W < (1L << 30);
}

int32_t launch_conv_slab_f16(const ConvArgs& a, hipStream_t s) {
    if (!conv_slab_supported(a) || a.Kpad != conv_slab_kpad(a)) return TRTX_ERR_UNSUPPORTED;
    if (!a.in || !a.out || !a.wgt || !aligned16(a.in) || !aligned16(a.out) || !aligned16(a.wgt) || (a.residual && !aligned16(a.residual)) ||
        (a.bias && !aligned16(a.bias)))
        return TRTX_ERR_INVALID;
    if (a.N <= 0) return TRTX_OK;
    SlabGeom g{};
    g.tiles_x = (a.Wo + 15) / 16;
    g.tiles_y = (a.Ho + kRows - 1) / kRows;
    g.total_tiles = a.N * g.tiles_x * g.tiles_y;
    g.chunks = (a.Cout + kChunk - 1) / kChunk;
    const int S = conv_slab_width(a);
    if (S == 16) return a.stride_h == 1 ? launch_slab<16, 1>(a, g, s) : launch_slab<16, 2>(a, g, s);
    return a.stride_h == 1 ? launch_slab<32, 1>(a, g, s) : launch_slab<32, 2>(a, g, s);
}

}  // namespace trtx
