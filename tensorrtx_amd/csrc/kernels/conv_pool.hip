// YOLOv9's downsamplers (yolov9/src/block.cpp:256-290) with the pools inside the convolution's launch, for gfx950: NHWC fp16 in and out, fp32 accumulation.
//   AVG_C3    (AConv, ADown's first half):   out = act(conv3x3 s2 p1 (avgpool2x2 s1 p0 (x)) + bias)
//   AVGMAX_C1 (ADown's second half):         out = act(conv1x1 (maxpool3x3 s2 p1 (avgpool2x2 s1 p0 (x))) + bias)
// Output pixel (i, j) reads the pooled positions (2i - 1 + r, 2j - 1 + q), r, q = 0 .. 2; pooled (u, v) = ((x[u][v] + x[u][v+1]) + x[u+1][v]) + x[u+1][v+1], times 1/4,
// in fp32 and rounded ONCE to fp16 - nhwc_pool's order and rounding, so the operand is bit for bit the tensor the two-op route stores - for 0 <= u <= H - 2 and
// 0 <= v <= W - 2.  Outside that range a pooled position is the convolution's zero padding (AVG_C3) or is left out of the maximum (AVGMAX_C1): it is never
// built from the input's border.  Ho = H / 2, Wo = W / 2.
//
// Why.  As separate ops the average pool reads and writes the whole full-resolution map for readers that want a quarter of it, and the max-pool reads half of that
// again; here neither pooled tensor exists outside LDS.  The implicit-GEMM family cannot do this: it fetches its A operand by LDS-DMA straight from global memory.
//
// Work unit: a workgroup of 4 waves owns 8 x 16 output pixels of one image (M = 128) by BN = 64 or 128 output channels, and walks Cin in chunks of 32 channels.
// Per chunk:
//   1. the raw halo patch, 18 x 34 pixels x 32 channels (39 KB), goes global -> registers -> LDS in 16-byte pieces: up to ten per thread, fetched while the
//      PREVIOUS chunk's taps issue (positions outside the image and channels beyond Cin arrive as zeros, and are never part of a valid pooled value);
//   2. one pooling pass writes the 17 x 33 pooled patch next to it.  Validity is decided here, not by the loads: an invalid position is stored as 0 (AVG_C3) or
//      -inf (AVGMAX_C1).  A pooled pixel is 32 halfs at a pitch of 40 (16 bytes more than 64), and a row holds its even columns first and its odd columns behind
//      them: the 16 lanes that read one k-slice of a tap read 16 NEIGHBOURING slots, 80 bytes apart - sixteen different 16-byte bank groups;
//   2b. AVGMAX_C1: a second pass takes the 3 x 3 maximum into an 8 x 16 x 32 tile (same pitch) that lies on the raw patch, which is dead by then;
//   3. v_mfma_f32_16x16x32_f16, tap by tap: the packed filter rows are the A fragments (16 output channels x 32 k, 16 bytes per lane from global / L2), the
//      pooled pixels of one tile row the B fragments.  A wave owns BN / 64 column blocks for all 8 tile rows: 8 or 16 accumulator fragments.
// Weights: the implicit-GEMM family's fp16 [Cout_pad][Kpad] with k = (r kw + q) CinK + c, CinK = Cin rounded up to 32 (conv_layout_view): zero beyond Cin.
// Epilogue in registers, as conv_dw_pw's: a lane holds 4 consecutive channels of one pixel: + bias, act (act.h's act_fast), one rounding, one 8-byte store.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../common.h"
#include "act.h"
#include "kernels.h"
#include "launch.h"

namespace trtx {
namespace {

constexpr int kThreads = 256;
constexpr int kTH = 8, kTW = 16;                  // output pixels per tile
constexpr int kRH = 2 * kTH + 2, kRW = 2 * kTW + 2;   // raw halo patch: 18 x 34
constexpr int kPH = kRH - 1, kPW = kRW - 1;       // pooled patch: 17 x 33
constexpr int kChunk = 32;                        // channels per k-loop step
constexpr int kPitch = kChunk + 8;                // halfs per pooled pixel in LDS
constexpr int kRawItems = kRH * kRW * (kChunk / 8);
constexpr int kRawPerThread = (kRawItems + kThreads - 1) / kThreads;
constexpr int kRawBytes = kRH * kRW * kChunk * 2;
constexpr int kLdsBytes = kRawBytes + kPH * kPW * kPitch * 2;
static_assert(kTH * kTW * kPitch * 2 <= kRawBytes, "the max-pooled tile lies on the raw patch");

// slot of pooled column pc within its row: the even columns, then the odd ones
__device__ __forceinline__ int pooled_slot(int pc) { return (pc & 1) ? (kPW + 1) / 2 + (pc >> 1) : (pc >> 1); }

template <int MODE, int NF>
__global__ __launch_bounds__(kThreads) void conv_pool_kernel(const ConvArgs p, int tiles_x, int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) char s_lds[];
    _Float16* const s_raw = reinterpret_cast<_Float16*>(s_lds);
    _Float16* const s_pool = reinterpret_cast<_Float16*>(s_lds + kRawBytes);
    _Float16* const s_max = s_raw;   // AVGMAX_C1: the A tile
    constexpr int TAPS = MODE == CONV_POOL_AVG_C3 ? 9 : 1;
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int x0 = (b % tiles_x) * kTW;
    b /= tiles_x;
    const int y0 = (b % tiles_y) * kTH;
    const long n = b / tiles_y;
    const int cb0 = blockIdx.y * 4 * NF;   // this workgroup's first 16-channel column block
    const int u0 = 2 * y0 - 1, v0 = 2 * x0 - 1;   // pooled (and raw) position of patch element (0, 0)
    const _Float16* __restrict__ in = static_cast<const _Float16*>(p.in) + n * p.H * p.W * (long)p.ld_in;
    const int chunks = (p.Cin + kChunk - 1) / kChunk;

    half8 pre[kRawPerThread];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int k = 0; k < kRawPerThread; ++k) {
            const int i = tid + k * kThreads;
            const int cv = i & 3, pix = i >> 2;
            const int row = u0 + pix / kRW, col = v0 + pix % kRW, c = chunk * kChunk + cv * 8;
            pre[k] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (i < kRawItems && (unsigned)row < (unsigned)p.H && (unsigned)col < (unsigned)p.W && c < p.Cin)
                pre[k] = *reinterpret_cast<const half8*>(in + ((long)row * p.W + col) * p.ld_in + c);
        }
    };

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 4, col = lane & 15;
    const _Float16* __restrict__ wgt = static_cast<const _Float16*>(p.wgt);
    const int nblk = (p.Cout + 15) / 16;
    const int cbw = cb0 + wave * NF;   // this wave's first column block
    floatx4 acc[kTH][NF];
#pragma unroll
    for (int rf = 0; rf < kTH; ++rf)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[rf][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
#pragma nounroll
    for (int chunk = 0; chunk < chunks; ++chunk) {
        // ---- 1. the raw patch of this chunk, fetched during the previous chunk's taps
#pragma unroll
        for (int k = 0; k < kRawPerThread; ++k) {
            const int i = tid + k * kThreads;
            if (i < kRawItems) *reinterpret_cast<half8*>(s_raw + i * 8) = pre[k];
        }
        __syncthreads();
        // ---- 2. the 2 x 2 average, nhwc_pool's sum order, one rounding; positions outside the pooled map are padding
        for (int i = tid; i < kPH * kPW * (kChunk / 8); i += kThreads) {
            const int cv = i & 3, pp = i >> 2;
            const int pr = pp / kPW, pc = pp % kPW;
            const _Float16 pad = MODE == CONV_POOL_AVG_C3 ? (_Float16)0.f : (_Float16)(-INFINITY);
            half8 o = half8{pad, pad, pad, pad, pad, pad, pad, pad};
            if ((unsigned)(u0 + pr) < (unsigned)(p.H - 1) && (unsigned)(v0 + pc) < (unsigned)(p.W - 1)) {
                const _Float16* r0 = s_raw + (pr * kRW + pc) * kChunk + cv * 8;
                const half8 a = *reinterpret_cast<const half8*>(r0), bq = *reinterpret_cast<const half8*>(r0 + kChunk);
                const half8 c = *reinterpret_cast<const half8*>(r0 + kRW * kChunk), d = *reinterpret_cast<const half8*>(r0 + (kRW + 1) * kChunk);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = round_to_half(((((float)a[e] + (float)bq[e]) + (float)c[e]) + (float)d[e]) * 0.25f);
            }
            *reinterpret_cast<half8*>(s_pool + (pr * kPW + pooled_slot(pc)) * kPitch + cv * 8) = o;
        }
        __syncthreads();
        if (MODE == CONV_POOL_AVGMAX_C1) {
            // ---- 2b. the 3 x 3 stride-2 maximum over the pooled values that exist (a ragged tile's pixels outside the map have none: zeros, never stored)
            for (int i = tid; i < kTH * kTW * (kChunk / 8); i += kThreads) {
                const int cv = i & 3, op = i >> 2;
                const int rf = op / kTW, j = op % kTW;
                const _Float16 ninf = (_Float16)(-INFINITY);
                half8 m = half8{ninf, ninf, ninf, ninf, ninf, ninf, ninf, ninf};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const half8 v = *reinterpret_cast<const half8*>(s_pool + ((2 * rf + r) * kPW + pooled_slot(2 * j + q)) * kPitch + cv * 8);
#pragma unroll
                        for (int e = 0; e < 8; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
                    }
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = m[e] == ninf ? (_Float16)0.f : m[e];
                *reinterpret_cast<half8*>(s_max + op * kPitch + cv * 8) = m;
            }
            __syncthreads();
        }
        // ---- 3. the next chunk's raw patch into registers, then this chunk's taps
        if (chunk + 1 < chunks) fetch(chunk + 1);
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const int r = tap / 3, q = tap % 3;
            half8 wf[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                wf[j] = half8{0, 0, 0, 0, 0, 0, 0, 0};
                if (cbw + j < nblk) wf[j] = *reinterpret_cast<const half8*>(wgt + (size_t)((cbw + j) * 16 + col) * p.Kpad + (size_t)tap * p.CinK + chunk * kChunk + grp * 8);
            }
#pragma unroll
            for (int rf = 0; rf < kTH; ++rf) {
                const _Float16* src = MODE == CONV_POOL_AVG_C3 ? s_pool + ((2 * rf + r) * kPW + pooled_slot(2 * col + q)) * kPitch : s_max + (rf * kTW + col) * kPitch;
                const half8 xf = *reinterpret_cast<const half8*>(src + grp * 8);
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[rf][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf, acc[rf][j], 0, 0, 0);
            }
        }
        __syncthreads();   // every wave is done with this chunk's operands before the next chunk's overwrite them
    }

    // ---- epilogue: this lane's accumulator rows are channels 16 cb + 4 grp + [0, 4) of pixel (y0 + rf, x0 + col)
    _Float16* __restrict__ out = static_cast<_Float16*>(p.out);
    const int wo = x0 + col;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int c = (cbw + j) * 16 + grp * 4;
        if (c >= p.Cout || wo >= p.Wo) continue;   // (Cout % 8 == 0: all four channels or none)
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.bias) bv = *reinterpret_cast<const float4*>(p.bias + c);
#pragma unroll
        for (int rf = 0; rf < kTH; ++rf) {
            const int ho = y0 + rf;
            if (ho >= p.Ho) continue;
            const size_t m = ((size_t)n * p.Ho + ho) * p.Wo + wo;
            const float v[4] = {acc[rf][j][0] + bv.x, acc[rf][j][1] + bv.y, acc[rf][j][2] + bv.z, acc[rf][j][3] + bv.w};
            half4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = round_to_half(act_fast(v[e], p.act1, p.alpha1));
            *reinterpret_cast<half4*>(out + m * p.ld_out + c) = o;
        }
    }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// The output may not lie on the input's pixels: a workgroup stores its tile while others still read those pixels as halo.  Where both pointers are set: the
// two byte ranges are apart.  (Unlike DSConv's the two maps differ in size, so a slice of the input's own buffer is always on pixels that are read.)
bool output_on_input(const ConvArgs& a) {
    if (!a.in || !a.out) return false;
    const intptr_t pin = reinterpret_cast<intptr_t>(a.in), pout = reinterpret_cast<intptr_t>(a.out);
    const intptr_t in_bytes = (((intptr_t)a.N * a.H * a.W - 1) * a.ld_in + a.Cin) * 2;
    const intptr_t out_bytes = (((intptr_t)a.N * a.Ho * a.Wo - 1) * a.ld_out + a.Cout) * 2;
    return !(pin + in_bytes <= pout || pout + out_bytes <= pin);
}

template <int MODE, int NF>
int32_t launch(const ConvArgs& a, hipStream_t s) {
    const int tiles_x = (a.Wo + kTW - 1) / kTW, tiles_y = (a.Ho + kTH - 1) / kTH;
    const long total = (long)a.N * tiles_x * tiles_y;
    const int col_tiles = (a.Cout + 64 * NF - 1) / (64 * NF);
    if (total > 0x7fffffffL || col_tiles > 65535) return TRTX_ERR_UNSUPPORTED;
    static bool asked[64] = {};   // per instantiation and device: more than 64 KB of dynamic LDS has to be asked for
    int dev = 0;
    TRTX_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return TRTX_ERR_HIP;
    if (!asked[dev]) {
        TRTX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_pool_kernel<MODE, NF>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        asked[dev] = true;
    }
    TRTX_LAUNCH((conv_pool_kernel<MODE, NF>), dim3((unsigned)total, (unsigned)col_tiles), dim3(kThreads), kLdsBytes, s, a, tiles_x, tiles_y);
    return check_launch("conv_pool_f16");
}

}  // namespace

// plan time: pointers may be null (geometry only); launch time: the alignment of whatever pointers are set counts too
bool conv_pool_supported(int mode, const ConvArgs& a) {
    const int k = mode == CONV_POOL_AVG_C3 ? 3 : 1;
    const bool geometry = (mode == CONV_POOL_AVG_C3 || mode == CONV_POOL_AVGMAX_C1) && a.kh == k && a.kw == k && a.groups == 1 && a.dil_h == 1 && a.dil_w == 1 &&
                          a.N >= 1 && a.H >= 2 && a.W >= 2 && a.Ho == a.H / 2 && a.Wo == a.W / 2;
    const bool plain = !a.f32 && !a.in_i8 && !a.out_i8 && !a.res_i8 && !a.up_C && !a.residual && a.act2 == ACT_NONE && a.act1 >= ACT_NONE && a.act1 <= ACT_GELU_TANH;
    const bool channels = a.Cin >= 8 && a.Cin % 8 == 0 && a.Cout >= 8 && a.Cout % 8 == 0 && a.ld_in % 8 == 0 && a.ld_in >= a.Cin && a.ld_out % 8 == 0 && a.ld_out >= a.Cout;
    const bool packed = a.CinK == (a.Cin + kChunk - 1) / kChunk * kChunk && a.Kpad == k * k * a.CinK && a.Cout_pad >= (a.Cout + 15) / 16 * 16;
    // (an image below 2 GB on either side: the kernel's offsets within an image are computed in 64 bits, the limit is the family's)
    const bool sizes = (long)a.H * a.W * a.ld_in < (1L << 30) && (long)a.Ho * a.Wo * a.ld_out < (1L << 30);
    return geometry && plain && channels && packed && sizes && aligned16(a.in) && aligned16(a.wgt) && aligned16(a.bias) && aligned16(a.out);
}

// Where the lowering fuses (match_pool_conv).  Measured (tools/pool_conv_time.py, profiles/pool_conv_time.jsonl; fp16, batch 32, 640 x 640, one context, five alternating
// pairs, ms per step, pool_conv | pool ops): yolov9c (ADown, 128 -> 128 at 160 x 160, 256 -> 256 at 80 x 80 and 40 x 40) 12.25 | 11.86, spread 0.06; yolov9t (AConv, 32 -> 64
// .. 96 -> 128) 3.347 | 3.328, spread 0.011.  The one launch lost every pair of both models, and every profiled op pair: 84 KB of LDS leave one workgroup of four waves
// on a CU, whose staging, pooling and MFMA phases then run one after the other (128 -> 128 at 160 x 160: 0.30 ms where the tile's MFMAs need about 0.06).  Admitted is
// what measured faster: nothing yet.  The kernel stays reachable through trtx_op_conv_pool_f16 and TRTX_POOL_CONV=2 until a faster work split changes that.
bool conv_pool_worthwhile(int mode, int cin, int cout) {
    (void)mode; (void)cin; (void)cout;
    return false;
}

int32_t conv_pool_f16(int mode, const ConvArgs& a, hipStream_t s) {
    if (!conv_pool_supported(mode, a) || !a.in || !a.wgt || !a.out) return TRTX_ERR_UNSUPPORTED;
    if (output_on_input(a)) return TRTX_ERR_INVALID;
    const bool wide = a.Cout > 64;
    if (mode == CONV_POOL_AVG_C3) return wide ? launch<CONV_POOL_AVG_C3, 2>(a, s) : launch<CONV_POOL_AVG_C3, 1>(a, s);
    return wide ? launch<CONV_POOL_AVGMAX_C1, 2>(a, s) : launch<CONV_POOL_AVGMAX_C1, 1>(a, s);
}

}  // namespace trtx
