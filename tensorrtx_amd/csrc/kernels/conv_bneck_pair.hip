// The two 3x3 convolutions of a 16-channel C2f bottleneck in ONE launch for gfx950: NHWC fp16 in (a channel slice of the concat buffer), the second
// convolution's output - plus the input as shortcut - out (another slice of it).  (YOLOv8n model.2.m.0: Conv 16 -> 16 3x3, Conv 16 -> 16 3x3, add;
// yolov8/src/block.cpp bottleneck().)
//
// Why.  On the 160 x 160 map at batch 32 the two launches move 131 MB - the 26 MB tensor between them written and read back, the input read twice -
// against 52 MB that the pair needs, and K = 144 puts both far below the MFMA ridge.  Fused, the intermediate lives in LDS only and the shortcut
// comes from the input patch that is there already.
//
// A persistent workgroup (4 waves) keeps BOTH weight sets (2 x 5 half8 A fragments) and both biases in registers and walks a contiguous run of output
// tiles of 8 x 16 pixels:
//   fetch    the 12 x 20 x 16-channel input patch of a tile, global -> registers (two 16-byte chunks per thread), issued one tile ahead right after
//            the first convolution so that it travels under the second convolution and the stores, then registers -> the other patch buffer;
//   conv 1   over the 10 x 18 region as a linear list of 13 MFMA groups of 16 pixels, B fragments straight from the patch; bias, activation and
//            rounding as conv_epilogue_fast computes them; a lane's 4 channels (8 bytes) go into the LDS image of the region.  Region pixels
//            outside the image are stored as ZEROS: they are the second convolution's padding, not values of the first;
//   conv 2   from that image, wave w owns tile rows 2w and 2w + 1; bias, act1, rounding; one v_permlane32_swap per packed dword leaves every lane
//            with 8 consecutive channels of one pixel; then (float)v + (float)shortcut from the centre of the patch, act2, rounding, 16-byte stores.
// K order of both convolutions: k = tap * 16 + c, five 32-wide k-steps accumulated from zero, tap 9 zero - conv_igemm_tile's CinK == 16 form, so
// every output element is, bit for bit, what two launches of the implicit-GEMM kernel's main K order produce.
// Index arithmetic: bneck_pair_index.h (host-compilable, replayed on the CPU by tests/test_bneck_pair_cpu.py).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "act.h"
#include "bneck_pair_index.h"
#include "kernels.h"
#include "launch.h"

namespace trtx {
namespace {

namespace bx = bneckidx;

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx2 __attribute__((ext_vector_type(2)));

static_assert(bx::kLdsBytes <= 32 * 1024, "at least four workgroups per CU beside other contexts' workgroups");

__device__ __forceinline__ unsigned bneck_pack_h2(_Float16 lo, _Float16 hi) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, half2v{lo, hi});
}

// round_to_half(act1(x)) for the three activations conv_epilogue_fast has a fast path for
__device__ __forceinline__ _Float16 bneck_act1(float x, int act) {
    if (act == ACT_SILU) return round_to_half(x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)));
    if (act == ACT_RELU) return round_to_half(x > 0.f ? x : 0.f);
    return round_to_half(x);
}

__global__ __launch_bounds__(256) void conv_bneck_pair_kernel(const ConvArgs pa, const ConvArgs pb, int tiles_x, int tiles_y, int total_tiles) {
    extern __shared__ __attribute__((aligned(256))) char s_lds[];
    char* const s_img = s_lds + 2 * bx::kPatchBytes;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 4, col = lane & 15;

    // ---- resident operands: both weight sets as A fragments (k-step kt: k = 32 kt + 8 grp + [0, 8) of row weight_row_channel(col)), both biases
    half8 wa[bx::kSteps], wb[bx::kSteps];
    {
        const _Float16* __restrict__ w0 = static_cast<const _Float16*>(pa.wgt);   // [Cout_pad = 16][Kpad = 160]
        const _Float16* __restrict__ w1 = static_cast<const _Float16*>(pb.wgt);
        const int row = bx::weight_row_channel(col);
#pragma unroll
        for (int kt = 0; kt < bx::kSteps; ++kt) {
            wa[kt] = *reinterpret_cast<const half8*>(w0 + (size_t)row * pa.Kpad + kt * 32 + grp * 8);
            wb[kt] = *reinterpret_cast<const half8*>(w1 + (size_t)row * pb.Kpad + kt * 32 + grp * 8);
        }
    }
    const int ch4 = bx::lane_channel(grp);   // this lane's accumulator rows are channels ch4 + [0, 4)
    float4 ba = make_float4(0.f, 0.f, 0.f, 0.f), bb = ba;
    if (pa.bias) ba = *reinterpret_cast<const float4*>(pa.bias + ch4);
    if (pb.bias) bb = *reinterpret_cast<const float4*>(pb.bias + ch4);
    const _Float16* __restrict__ in = static_cast<const _Float16*>(pa.in);
    _Float16* __restrict__ out = static_cast<_Float16*>(pb.out);
    const bool shortcut = pb.residual != nullptr, relu2 = pb.act2 != ACT_NONE;

    uintx4 stage[bx::kFetch];
    auto fetch = [&](int tile) {   // global -> registers; pixels outside the image are zeros
        const bx::Tile t = bx::tile_of(tile, tiles_x, tiles_y);
#pragma unroll
        for (int f = 0; f < bx::kFetch; ++f) {
            const int c = tid + f * 256;
            stage[f] = uintx4{0u, 0u, 0u, 0u};
            if (c < bx::kPatchChunks) {
                const bx::PatchChunk pc = bx::patch_chunk(c);
                const int y = t.y0 - 2 + pc.py, x = t.x0 - 2 + pc.px;
                if ((unsigned)y < (unsigned)pa.H && (unsigned)x < (unsigned)pa.W)
                    stage[f] = *reinterpret_cast<const uintx4*>(in + (((size_t)t.n * pa.H + y) * pa.W + x) * pa.ld_in + pc.plane * 8);
            }
        }
    };
    auto land = [&](char* patch) {   // registers -> LDS
#pragma unroll
        for (int f = 0; f < bx::kFetch; ++f) {
            const int c = tid + f * 256;
            if (c < bx::kPatchChunks) {
                const bx::PatchChunk pc = bx::patch_chunk(c);
                *reinterpret_cast<uintx4*>(patch + bx::patch_offset(pc.py, pc.px, pc.plane)) = stage[f];
            }
        }
    };

    const int per = bx::run_length(total_tiles, (int)gridDim.x);
    const int first = bx::run_first((int)blockIdx.x, total_tiles, (int)gridDim.x);
    const int last = first + per < total_tiles ? first + per : total_tiles;
    if (first < last) fetch(first);
    int buf = 0;
    for (int tile = first; tile < last; ++tile, buf ^= 1) {
        const bx::Tile t = bx::tile_of(tile, tiles_x, tiles_y);
        char* const s_patch = s_lds + buf * bx::kPatchBytes;
        // ---- this tile's patch was fetched under the previous tile's second convolution (or above); the other buffer is still being read
        land(s_patch);
        __syncthreads();   // the patch is complete; every wave is done reading the previous tile's image
        // ---- first convolution over the region, into the LDS image
#pragma nounroll
        for (int gi = wave; gi < bx::kGroups; gi += 4) {
            const bx::RegionPixel rp = bx::region_pixel(gi, lane);
            floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kt = 0; kt < bx::kSteps; ++kt) {
                const int tap = bx::step_tap(kt, lane);
                half8 xf = half8{0, 0, 0, 0, 0, 0, 0, 0};
                if (tap < bx::kTaps) xf = *reinterpret_cast<const half8*>(s_patch + bx::frag1_offset(rp.ry, rp.rx, tap, bx::step_chunk(lane)));
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[kt], xf, acc, 0, 0, 0);
            }
            float x[4] = {acc[0], acc[1], acc[2], acc[3]};
            if (pa.bias) {
                x[0] += ba.x; x[1] += ba.y; x[2] += ba.z; x[3] += ba.w;
            }
            half4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = bneck_act1(x[e], pa.act1);
            const int iy = t.y0 - 1 + rp.ry, ix = t.x0 - 1 + rp.rx;
            if ((unsigned)iy >= (unsigned)pa.Ho || (unsigned)ix >= (unsigned)pa.Wo) o = half4{0, 0, 0, 0};   // the second convolution's padding
            if (rp.live) *reinterpret_cast<half4*>(s_img + bx::image_offset(rp.ry, rp.rx, ch4)) = o;
        }
        __syncthreads();   // the image is complete
        if (tile + 1 < last) fetch(tile + 1);
        // ---- second convolution: wave w owns tile rows 2w and 2w + 1
        floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kt = 0; kt < bx::kSteps; ++kt) {
            const int tap = bx::step_tap(kt, lane);
            half8 xf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                xf[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
                if (tap < bx::kTaps) xf[i] = *reinterpret_cast<const half8*>(s_img + bx::frag2_offset(2 * wave + i, col, tap, bx::step_chunk(lane)));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[kt], xf[i], acc[i], 0, 0, 0);
        }
        // ---- epilogue: bias, act1, rounding; the half-wave swap; shortcut, act2, rounding; one 16-byte store per lane
        unsigned pk[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float x[4] = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
            if (pb.bias) {
                x[0] += bb.x; x[1] += bb.y; x[2] += bb.z; x[3] += bb.w;
            }
            _Float16 h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = bneck_act1(x[e], pb.act1);
            pk[i][0] = bneck_pack_h2(h[0], h[1]);
            pk[i][1] = bneck_pack_h2(h[2], h[3]);
        }
        // lanes 32-63 of tile row 2w <-> lanes 0-31 of tile row 2w + 1: afterwards (s0[0], s1[0], s0[1], s1[1]) are channels store_channel + [0, 8) of
        // pixel (store_row, col) in every lane
        const uintx2 s0 = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false);
        const uintx2 s1 = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false);
        const uintx4 q = {s0[0], s1[0], s0[1], s1[1]};
        half8 v = __builtin_bit_cast(half8, q);
        if (shortcut || relu2) {
            half8 rv = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (shortcut) rv = *reinterpret_cast<const half8*>(s_patch + bx::shortcut_offset(wave, lane));
            if (!relu2) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = round_to_half((float)v[e] + (float)rv[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float s = (float)v[e] + (float)rv[e];
                    v[e] = round_to_half(s > 0.f ? s : 0.f);
                }
            }
        }
        const int ho = t.y0 + bx::store_row(wave, lane), wo = t.x0 + col;
        if (ho < pb.Ho && wo < pb.Wo) {
            const size_t m = ((size_t)t.n * pb.Ho + ho) * pb.Wo + wo;
            *reinterpret_cast<half8*>(out + m * pb.ld_out + bx::store_channel(lane)) = v;
        }
    }
}

bool bneck_layer_ok(const ConvArgs& c) {
    const bool fast_act = c.act1 == ACT_SILU || c.act1 == ACT_RELU || c.act1 == ACT_NONE;
    return !c.f32 && !c.in_i8 && !c.out_i8 && !c.res_i8 && !c.up_C && fast_act && !c.scalar_out && c.groups == 1 && c.dil_h == 1 && c.dil_w == 1 && c.Cin == 16 &&
           c.CinK == 16 && c.bk == 32 && c.Kpad == 160 && c.Cout == 16 && c.Cout_pad == 16 && c.kh == 3 && c.kw == 3 && c.stride_h == 1 && c.stride_w == 1 &&
           c.pad_h == 1 && c.pad_w == 1 && c.N >= 1 && c.H >= 1 && c.W >= 1 && c.Ho == c.H && c.Wo == c.W && (reinterpret_cast<uintptr_t>(c.wgt) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(c.bias) & 15) == 0;
}

}  // namespace

// plan time: pointers may be null (geometry only); launch time: the alignment of the pointers counts too, and a shortcut must be the first layer's input
bool conv_bneck_pair_possible(const ConvArgs& a, const ConvArgs& b) {
    const bool first_ok = bneck_layer_ok(a) && !a.residual && a.act2 == ACT_NONE && a.ld_in % 8 == 0 && a.ld_in >= 16 &&
                          (reinterpret_cast<uintptr_t>(a.in) & 15) == 0;
    const bool second_ok = bneck_layer_ok(b) && (b.act2 == ACT_NONE || (b.act2 == ACT_RELU && b.residual)) && b.ld_out % 8 == 0 && b.ld_out >= 16 &&
                           (reinterpret_cast<uintptr_t>(b.out) & 15) == 0;
    const bool chained = b.N == a.N && b.H == a.Ho && b.W == a.Wo;
    // the shortcut is read from the input patch: the same tensor (at launch time, where both pointers are set: the same address and stride)
    const bool shortcut_ok = !b.residual || !a.in || reinterpret_cast<uintptr_t>(b.residual) < 4096 || (b.residual == a.in && b.ld_res == a.ld_in);
    // The output may not lie on the input: a workgroup stores its tile while others - and its own fetch of the next tile - still read those pixels as patch or
    // halo (two launches may run in place, this one may not).  At launch time, where both pointers are set: the two byte ranges are apart, or they are
    // different 16-channel slices of one buffer (the same channel stride, the pointers less than one pixel apart)
    bool apart = true;
    if (a.in && b.out && first_ok && second_ok && chained) {
        const intptr_t pin = reinterpret_cast<intptr_t>(a.in), pout = reinterpret_cast<intptr_t>(b.out);
        const intptr_t pixels = (intptr_t)a.N * a.H * a.W;
        const intptr_t in_bytes = ((pixels - 1) * a.ld_in + 16) * 2, out_bytes = ((pixels - 1) * b.ld_out + 16) * 2;
        const intptr_t d = pout > pin ? pout - pin : pin - pout;   // bytes
        const bool disjoint = pin + in_bytes <= pout || pout + out_bytes <= pin;
        const bool slices = a.ld_in == b.ld_out && d >= 32 && d + 32 <= (intptr_t)a.ld_in * 2;
        apart = disjoint || slices;
    }
    return first_ok && second_ok && chained && shortcut_ok && apart;
}

// The pair where the fused kernel takes it, the two launches of the implicit-GEMM kernel where it does not (a.out, the tensor between the two, is then
// written and b.in must be it): what the executor issues at a marked op, so that the first convolution can never be left out
int32_t conv_bneck_pair_or_two_f16(const ConvArgs& a, const ConvArgs& b, hipStream_t stream) {
    if (conv_bneck_pair_possible(a, b) && a.in && a.wgt && b.wgt && b.out) return conv_bneck_pair_f16(a, b, stream);
    if (!a.out || b.in != a.out) return TRTX_ERR_INVALID;
    const int32_t st = conv_igemm_f16(a, stream);
    return st != TRTX_OK ? st : conv_igemm_f16(b, stream);
}

// a: the first convolution as conv_igemm_f16 takes it (a.out unused); b: the second (b.in unused; b.residual, if set, is a.in)
int32_t conv_bneck_pair_f16(const ConvArgs& a, const ConvArgs& b, hipStream_t stream) {
    if (!conv_bneck_pair_possible(a, b) || !a.in || !a.wgt || !b.wgt || !b.out || (b.residual && b.residual != a.in)) return TRTX_ERR_UNSUPPORTED;
    namespace bx = bneckidx;
    const int tiles_x = (b.Wo + bx::kTW - 1) / bx::kTW, tiles_y = (b.Ho + bx::kTH - 1) / bx::kTH;
    const long total_l = (long)b.N * tiles_x * tiles_y;
    if (total_l > 0x7fffffffL - 65536) return TRTX_ERR_UNSUPPORTED;
    const int total = (int)total_l;
    // as many workgroups as are resident at once (cached per thread and device, as the stem pair does), each walking a contiguous run of tiles
    static thread_local int resident[2] = {-1, 0};   // [0]: device, [1]: workgroups on the chip
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (resident[0] != dev || resident[1] <= 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv_bneck_pair_kernel, 256, bx::kLdsBytes) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        (void)hipGetLastError();
        resident[0] = dev;
        resident[1] = per_cu * cus;
    }
    const int most = total < resident[1] ? total : resident[1];
    const int grid = (total + bx::run_length(total, most) - 1) / bx::run_length(total, most);   // equal runs: no workgroup without tiles
    TRTX_LAUNCH(conv_bneck_pair_kernel, dim3((unsigned)grid), dim3(256), bx::kLdsBytes, stream, a, b, tiles_x, tiles_y, total);
    return check_launch("conv_bneck_pair_f16");
}

}  // namespace trtx
