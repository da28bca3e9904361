// The YOLO stem and the stride-2 3x3 convolution behind it in ONE launch for gfx950: fp32 NCHW network input in, the second convolution's NHWC
// fp16 output out.  (YOLOv8 model.0 3->16 3x3/2 and model.1 16->32 3x3/2, yolov8/src/model.cpp:115-116.)
//
// Why.  Run one after the other the two layers move 420 MB per 640 x 640 batch-32 step, half of it the stem's output written and read back - the
// largest intermediate tensor of the network - and both are far below the MFMA ridge (K = 27 and 144).  Both strides are 2, so the halo of the
// intermediate is small: a 17 x 33 stem region serves an 8 x 16 output tile (1.10x recompute).  Fused, the intermediate lives in LDS only.
//
// A persistent workgroup (4 waves) keeps both weight sets in registers and walks output tiles of the second convolution:
//   stage 1  the fp32 input patch of the tile (3 x 35 x 72 floats) HBM -> LDS, stem_tile.h's LDS-DMA fetch (the stem kernel's own stage 1);
//   stage 2  the stem over the 17 x 33 region as a linear list of 36 MFMA groups of 16 pixels, stem_tile.h's registers and arithmetic; a lane's 4
//            channels (8 bytes) go into the LDS image of the region.  Region pixels outside the intermediate image are stored as ZEROS: they are
//            the second convolution's padding, not stem values;
//   stage 3  the second convolution from that image, two taps per 32-wide k-step exactly as conv_igemm_tile's CinK == 16 form places them (k = tap * 16
//            + c, five k-steps from zero, tap 9 zero), then bias, activation and rounding as conv_epilogue_fast computes them, 16-byte NHWC stores
//            straight from the registers.
// The next tile's patch fetch is issued as soon as stage 2 has released the patch, so it travels under stage 3 and the stores.
// Every output element is, bit for bit, what conv_stem_nchw_f32 followed by the implicit-GEMM kernel's main K order produces.
// Index arithmetic: stem_pair_index.h (host-compilable, replayed on the CPU by tests/test_stem_pair_cpu.py).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "act.h"
#include "kernels.h"
#include "launch.h"
#include "stem_pair_index.h"
#include "stem_tile.h"

namespace trtx {
namespace {

namespace px = pairidx;

constexpr int kPairPatchBytesMax = (4 * px::kPR * px::kPCA / 4 + 255) / 256 * 256 * 16;   // Cin = 4: 40 960
static_assert(kPairPatchBytesMax + px::kImageBytes <= 80 * 1024, "two workgroups per CU and room for other contexts");

__device__ __forceinline__ size_t pair_patch_bytes(int cin) { return (size_t)((cin * px::kPR * px::kPCA / 4 + 255) / 256 * 256) * 16; }

__global__ __launch_bounds__(256) void conv_stem_pair_kernel(const ConvArgs ps, const ConvArgs p1, const StemGeom g, unsigned in_bytes, int total_tiles) {
    extern __shared__ __attribute__((aligned(16))) float s_patch[];
    char* const s_img = reinterpret_cast<char*>(s_patch) + pair_patch_bytes(ps.Cin);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 4, col = lane & 15;

    // ---- resident operands
    StemRegs<1, 1> R;
    stem_setup<1, 1>(ps, g, R);
    half8 w1[2][px::kSteps];   // the second convolution's weights as A fragments: fragment j, k-step kt, k = 32 kt + 8 grp + [0, 8)
    {
        const _Float16* __restrict__ w = static_cast<const _Float16*>(p1.wgt);   // [Cout_pad = 32][Kpad = 160]
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kt = 0; kt < px::kSteps; ++kt)
                w1[j][kt] = *reinterpret_cast<const half8*>(w + (size_t)px::weight_row_channel(j, col) * p1.Kpad + kt * 32 + grp * 8);
    }
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;   // bias of channels 8 grp + [0, 8)
    if (p1.bias) {
        b0 = *reinterpret_cast<const float4*>(p1.bias + grp * 8);
        b1 = *reinterpret_cast<const float4*>(p1.bias + grp * 8 + 4);
    }
    _Float16* __restrict__ out = static_cast<_Float16*>(p1.out);

    auto fetch = [&](int tile) {
        const px::Tile t = px::tile_of(tile, g.tiles_x, g.tiles_y);
        stem_patch_fetch(ps, g, in_bytes, s_patch, t.n, px::patch_start(t.y0), px::patch_aligned_start(px::patch_start(t.x0)));
    };
    if ((int)blockIdx.x < total_tiles) fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const px::Tile t = px::tile_of(tile, g.tiles_x, g.tiles_y);
        const int hi_start = px::patch_start(t.y0), wi_start = px::patch_start(t.x0);
        const int al_start = px::patch_aligned_start(wi_start);
        const int shift = wi_start - al_start;
        // ---- stage 1: this tile's patch was issued before the previous tile's stage 3 (or above)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // the patch has landed; every wave is done reading the previous tile's image
        stem_patch_tail(ps, g, s_patch, t.n, hi_start, al_start);
        // ---- stage 2: the stem over the region, into the LDS image
        const int iy0 = px::region_start(t.y0), ix0 = px::region_start(t.x0);
#pragma nounroll
        for (int gi = wave; gi < px::kGroups; gi += 4) {
            const px::RegionPixel rp = px::region_pixel(gi, lane);
            floatx4 acc[1];
            stem_group_mfma<1, 1>(R, s_patch + px::patch_offset(rp.ry, rp.rx, shift), acc);
            half4 o = stem_finish4(ps, acc[0], R.bias4[0]);
            const int iy = iy0 + rp.ry, ix = ix0 + rp.rx;
            if ((unsigned)iy >= (unsigned)p1.H || (unsigned)ix >= (unsigned)p1.W) o = half4{0, 0, 0, 0};   // the second convolution's padding
            if (rp.live) *reinterpret_cast<half4*>(s_img + px::image_offset(rp.ry, rp.rx, grp * 4)) = o;
        }
        __syncthreads();   // the image is complete; every wave is done with the patch
        const int next = tile + (int)gridDim.x;
        if (next < total_tiles) fetch(next);
        // ---- stage 3: the second convolution, wave w owns tile rows 2w and 2w + 1
        floatx4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < px::kSteps; ++kt) {
            const int tap = px::step_tap(kt, lane);
            half8 xf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                xf[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
                if (tap < px::kTaps) xf[i] = *reinterpret_cast<const half8*>(s_img + px::frag_offset(2 * wave + i, col, tap, px::step_chunk(lane)));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[j][kt], xf[i], acc[i][j], 0, 0, 0);
        }
        // ---- epilogue: a lane holds channels 8 grp + [0, 8) of pixel (2 wave + i, col)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ho = t.y0 + 2 * wave + i, wo = t.x0 + col;
            if (ho >= p1.Ho || wo >= p1.Wo) continue;
            float x[8] = {acc[i][0][0], acc[i][0][1], acc[i][0][2], acc[i][0][3], acc[i][1][0], acc[i][1][1], acc[i][1][2], acc[i][1][3]};
            if (p1.bias) {
                x[0] += b0.x; x[1] += b0.y; x[2] += b0.z; x[3] += b0.w;
                x[4] += b1.x; x[5] += b1.y; x[6] += b1.z; x[7] += b1.w;
            }
            half8 v;
            if (p1.act1 == ACT_SILU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = round_to_half(x[e] * __builtin_amdgcn_rcpf(1.0f + __expf(-x[e])));
            } else if (p1.act1 == ACT_RELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = round_to_half(x[e] > 0.f ? x[e] : 0.f);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = round_to_half(x[e]);
            }
            const size_t m = ((size_t)t.n * p1.Ho + ho) * p1.Wo + wo;
            *reinterpret_cast<half8*>(out + m * p1.ld_out + grp * 8) = v;
        }
    }
}

}  // namespace

// plan time: pointers may be null (geometry only); launch time: the alignment of the pointers counts too
bool conv_stem_pair_possible(const ConvArgs& s, const ConvArgs& c) {
    const bool stem_ok = conv_stem_supported(s) && !s.f32 && s.Cin <= 4 && s.Cout == 16 && s.kh == 3 && s.kw == 3 && s.stride_h == 2 && s.stride_w == 2 &&
                         s.pad_h == 1 && s.pad_w == 1 && s.N >= 1 && (size_t)s.N * s.Cin * s.H * s.W * 4 < 2000000000u &&
                         s.Ho == (s.H - 1) / 2 + 1 && s.Wo == (s.W - 1) / 2 + 1;
    const bool fast_act = c.act1 == ACT_SILU || c.act1 == ACT_RELU || c.act1 == ACT_NONE;
    const bool conv_ok = !c.f32 && !c.in_i8 && !c.out_i8 && !c.res_i8 && !c.residual && !c.up_C && c.act2 == ACT_NONE && fast_act && !c.scalar_out &&
                         c.groups == 1 && c.dil_h == 1 && c.dil_w == 1 && c.Cin == 16 && c.CinK == 16 && c.bk == 32 && c.Kpad == 160 && c.Cout == 32 &&
                         c.Cout_pad == 32 && c.kh == 3 && c.kw == 3 && c.stride_h == 2 && c.stride_w == 2 && c.pad_h == 1 && c.pad_w == 1 &&
                         c.ld_out % 8 == 0 && c.ld_out >= 32;
    const bool chained = c.N == s.N && c.H == s.Ho && c.W == s.Wo && c.Ho == (c.H - 1) / 2 + 1 && c.Wo == (c.W - 1) / 2 + 1;
    const bool aligned = (reinterpret_cast<uintptr_t>(s.in) & 15) == 0 && (reinterpret_cast<uintptr_t>(c.out) & 15) == 0 &&
                         (reinterpret_cast<uintptr_t>(c.wgt) & 15) == 0 && (reinterpret_cast<uintptr_t>(c.bias) & 15) == 0;
    return stem_ok && conv_ok && chained && aligned;
}

// s: the stem as conv_stem_nchw_f32 takes it (s.out unused); c: the second convolution as conv_igemm_f16 takes it (c.in unused)
int32_t conv_stem_pair_f16(const ConvArgs& s, const ConvArgs& c, hipStream_t stream) {
    if (!conv_stem_pair_possible(s, c) || !s.in || !s.wgt || !c.wgt || !c.out) return TRTX_ERR_UNSUPPORTED;
    namespace px = pairidx;
    StemGeom g;
    g.PR = px::kPR;
    g.PCA = px::kPCA;
    g.tiles_x = (c.Wo + px::kTW - 1) / px::kTW;
    g.tiles_y = (c.Ho + px::kTH - 1) / px::kTH;
    g.chunks = s.Cin * g.PR * g.PCA / 4;
    const size_t lds = (size_t)((g.chunks + 255) / 256 * 256) * 16 + px::kImageBytes;   // the patch in whole 1 KiB DMA rows, then the image
    const unsigned in_bytes = (unsigned)((size_t)s.N * s.Cin * s.H * s.W * 4);
    const long total_l = (long)s.N * g.tiles_x * g.tiles_y;
    if (total_l > 0x7fffffffL - 65536) return TRTX_ERR_UNSUPPORTED;
    const int total = (int)total_l;
    // as many workgroups as are resident at once, each walking total / grid tiles (cached per thread, device and LDS size, as the stem kernel does)
    static thread_local int resident[3] = {-1, 0, 0};   // [0]: device, [1]: LDS bytes the figure was computed for, [2]: workgroups on the chip
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (resident[0] != dev || resident[1] != (int)lds || resident[2] <= 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv_stem_pair_kernel, 256, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        (void)hipGetLastError();
        resident[0] = dev;
        resident[1] = (int)lds;
        resident[2] = per_cu * cus;
    }
    const int grid = total < resident[2] ? total : resident[2];
    TRTX_LAUNCH(conv_stem_pair_kernel, dim3((unsigned)grid), dim3(256), lds, stream, s, c, g, in_bytes, total);
    return check_launch("conv_stem_pair_f16");
}

}  // namespace trtx
