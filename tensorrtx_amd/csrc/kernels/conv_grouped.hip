// Grouped convolution (2 <= groups <= 8, not depthwise) on the matrix pipe for gfx950 (MI355X): the layers that fell to the scalar
// direct kernel because the implicit-GEMM family is written for groups == 1.  YOLOv9's detect head has two per pyramid level
// (yolov9/src/block.cpp:355-366: a 3x3 and a 1x1 convolution 64 -> 64 with g = 4, 16 -> 16 per group).
//
// Scope (conv_grouped_supported): fp16 NHWC in / out / residual; Cin / groups and Cout / groups multiples of 16 up to 64; 1x1 without
// padding or 3x3 with padding 1, stride 1, no dilation; channel strides multiples of 8; at most kMaxUnits 16-channel output fragments
// (Cout <= 128) and at most kLdsBudget bytes of LDS.
//
// Mapping (DESIGN.md "Grouped convolution"):
//   * a workgroup of 4 waves walks tiles of 4 x 16 output pixels (3x3; 1x1: 64 consecutive pixels of the N*H*W row) of ALL groups:
//     each input pixel's whole channel row crosses HBM / L2 -> LDS once per tile with 16-byte loads (the 3x3 halo: 6 x 18 pixels),
//     each output pixel's whole channel row leaves with 16-byte stores;
//   * the layer's whole filter lives in REGISTERS for the workgroup's lifetime: a "unit" is 16 output channels of one group, wave w owns
//     units w, w + 4 (UPW <= 2 per wave), each KS MFMA B operands, loaded once;
//   * K order is tap-major, then channel: k = tap * Cin_g + c, cut into 32-wide steps of v_mfma_f32_16x16x32_f16.  A lane's 8-half chunk
//     never straddles a tap (Cin_g % 8 == 0); with Cin_g = 16 a step covers two taps, and the chunks beyond the last tap (the ninth
//     tap's partner) are zeros in the packed filter and zeros in the A operand;
//   * LDS patch: one plane per 16 input channels, 32 bytes per pixel.  The 16-lane groups of ds_read_b128 then read 16 distinct
//     16-byte slots of the 256-byte bank row for any run of 16 consecutive pixels (MI355X_MICROARCH.md, LDS): conflict free;
//   * fp32 accumulation; epilogue bias -> act1 -> (+ residual) -> act2 in registers, ONE fp16 rounding, then through an LDS staging tile
//     so that the stores are row-major 16-byte chunks (the same reason as in conv_ws.hip).
// Packed weights: fp16 [group][Cout_g][Kpad] = rows [Cout][Kpad], Kpad = K rounded up to 32, BN scale folded (runtime/pack.cpp).
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

constexpr int kRows = 4;          // 16-pixel fragments per tile (3x3: tile rows)
constexpr int kTilePx = kRows * 16;
constexpr int kMaxUnits = 8;      // 16-channel output fragments of a layer: two per wave
constexpr int kLdsBudget = 64 * 1024;
constexpr int kMaxGrid = 256 * 4; // persistent workgroups: four per CU

struct GrGeom {
    int tiles_x, tiles_y, total_tiles;
    int M;   // N * Ho * Wo
};

constexpr int gr_ks(int taps, int cing) { return (taps * cing * 16 + 31) / 32; }
// registers a wave keeps live: stationary weights, A offsets, accumulators of the four fragments, A operands in flight, bookkeeping
constexpr int gr_regs(int taps, int cing, int upw) { return upw * gr_ks(taps, cing) * 4 + gr_ks(taps, cing) + 16 + 16 + 36; }
constexpr int gr_min_waves(int regs) { return regs <= 128 ? 4 : (regs <= 200 ? 2 : 1); }

// TAPS: 1 (1x1) or 9 (3x3); CING: Cin per group / 16; UPW: units per wave (1 or 2)
template <int TAPS, int CING, int UPW>
__global__ __launch_bounds__(256, gr_min_waves(gr_regs(TAPS, CING, UPW))) void conv_grouped_f16_kernel(const ConvArgs p, const GrGeom g) {
    constexpr int CG = CING * 16, K = TAPS * CG, KS = gr_ks(TAPS, CING), KPAD = KS * 32;
    constexpr int PH = TAPS == 9 ? kRows + 2 : kRows, PW = TAPS == 9 ? 18 : 16, PLANE = PH * PW * 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lj = lane >> 4;
    const int planes = p.Cin >> 4, units = p.Cout >> 4, nt = (p.Cout / p.groups) >> 4;
    const int cpp = p.Cin >> 3, cpo = p.Cout >> 3;   // 16-byte chunks of an input / output pixel
    const int sp = p.Cout * 2 + 16;                  // staging row pitch (bytes): 16 consecutive rows start in distinct 16-byte slots
    char* patch = smem;
    char* stage = smem + planes * PLANE;

    const _Float16* __restrict__ in = static_cast<const _Float16*>(p.in);
    const _Float16* __restrict__ res = static_cast<const _Float16*>(p.residual);
    _Float16* __restrict__ out = static_cast<_Float16*>(p.out);

    // ---- the filter -> registers, once: unit u = wave + 4 i, row (lane & 15) of it, chunk (lane >> 4) of every k-step
    half8 breg[UPW][KS];
    float4 bias4[UPW];
    int gbase[UPW];
#pragma unroll
    for (int i = 0; i < UPW; ++i) {
        const int u = wave + 4 * i;
        const int uu = u < units ? u : 0;
        const _Float16* wr = static_cast<const _Float16*>(p.wgt) + (size_t)(uu * 16 + li) * KPAD + lj * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) breg[i][ks] = *reinterpret_cast<const half8*>(wr + ks * 32);
        bias4[i] = p.bias ? *reinterpret_cast<const float4*>(p.bias + uu * 16 + lj * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        gbase[i] = (uu / nt) * CING * PLANE;
    }

    // ---- per-lane A offsets inside the patch (tile independent): chunk k0 = ks * 32 + (lane >> 4) * 8 of the K axis is channels
    // c .. c + 7 of tap k0 / CG, read at pixel (lane & 15) of the fragment shifted by the tap
    unsigned a_off[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int k0 = ks * 32 + lj * 8;
        const int kk = k0 < K ? k0 : 0;
        const int tap = kk / CG, c = kk - tap * CG;
        const int r = TAPS == 9 ? tap / 3 : 0, q = TAPS == 9 ? tap - 3 * r : 0;
        a_off[ks] = (unsigned)((c >> 4) * PLANE + (r * PW + q + li) * 32 + ((c >> 3) & 1) * 16);
    }
    const bool tail_live = (KS - 1) * 32 + lj * 8 < K;   // only the last step can reach beyond K

    const bool second = res || p.act2 != ACT_NONE;
    const int tpi = g.tiles_x * g.tiles_y;

    for (int tile = blockIdx.x; tile < g.total_tiles; tile += gridDim.x) {
        int n = 0, ho0 = 0, wo0 = 0;
        const long m0 = (long)tile * kTilePx;   // 1x1: first pixel of the tile
        if (TAPS == 9) {
            n = tile / tpi;
            const int rem = tile - n * tpi;
            const int ty = rem / g.tiles_x;
            ho0 = ty * kRows;
            wo0 = (rem - ty * g.tiles_x) * 16;
        }
        // ---- patch -> LDS: consecutive lanes take consecutive 16-byte chunks of a pixel's channel row; outside the image: zeros
        for (int it = tid; it < PH * PW * cpp; it += 256) {
            const int pp = it / cpp, c8 = it - pp * cpp;
            half8 v = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (TAPS == 9) {
                const int py = pp / PW, px = pp - py * PW;
                const int hi = ho0 - 1 + py, wi = wo0 - 1 + px;
                if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
                    v = *reinterpret_cast<const half8*>(in + (((long)n * p.H + hi) * p.W + wi) * p.ld_in + c8 * 8);
            } else {
                const long m = m0 + pp;
                if (m < g.M) v = *reinterpret_cast<const half8*>(in + m * p.ld_in + c8 * 8);
            }
            *reinterpret_cast<half8*>(patch + (c8 >> 1) * PLANE + pp * 32 + (c8 & 1) * 16) = v;
        }
        __syncthreads();

#pragma unroll
        for (int i = 0; i < UPW; ++i) {
            const int u = wave + 4 * i;
            if (u >= units) continue;   // wave-uniform
            const char* ab = patch + gbase[i];
            floatx4 acc[kRows];
#pragma unroll
            for (int f = 0; f < kRows; ++f) acc[f] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int f = 0; f < kRows; ++f) {
                    half8 a = *reinterpret_cast<const half8*>(ab + a_off[ks] + f * (PW * 32));
                    if (ks == KS - 1 && K % 32 != 0 && !tail_live) a = half8{0, 0, 0, 0, 0, 0, 0, 0};
                    acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(breg[i][ks], a, acc[f], 0, 0, 0);
                }
            }
            // ---- epilogue: the lane holds channels c0 .. c0 + 3 of pixel (lane & 15) of fragment f
            const int c0 = u * 16 + lj * 4;
            const float b4[4] = {bias4[i].x, bias4[i].y, bias4[i].z, bias4[i].w};
#pragma unroll
            for (int f = 0; f < kRows; ++f) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = act_fast(acc[f][e] + b4[e], p.act1, p.alpha1);
                if (second) {
                    float r4[4] = {0.f, 0.f, 0.f, 0.f};
                    if (res) {
                        long m;
                        bool live;
                        if (TAPS == 9) {
                            const int ho = ho0 + f, wo = wo0 + li;
                            live = ho < p.Ho && wo < p.Wo;
                            m = ((long)n * p.Ho + ho) * p.Wo + wo;
                        } else {
                            m = m0 + f * 16 + li;
                            live = m < g.M;
                        }
                        if (live) {
                            const half4 rv = *reinterpret_cast<const half4*>(res + m * p.ld_res + c0);
#pragma unroll
                            for (int e = 0; e < 4; ++e) r4[e] = (float)rv[e];
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_fast(v[e] + r4[e], p.act2, p.alpha2);
                }
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = round_to_half(v[e]);
                *reinterpret_cast<half4*>(stage + (f * 16 + li) * sp + c0 * 2) = o;
            }
        }
        __syncthreads();

        // ---- staging -> global, row-major: consecutive lanes store consecutive 16-byte chunks of a pixel's channel row
        for (int it = tid; it < kTilePx * cpo; it += 256) {
            const int row = it / cpo, cc = it - row * cpo;
            long m;
            bool live;
            if (TAPS == 9) {
                const int ho = ho0 + (row >> 4), wo = wo0 + (row & 15);
                live = ho < p.Ho && wo < p.Wo;
                m = ((long)n * p.Ho + ho) * p.Wo + wo;
            } else {
                m = m0 + row;
                live = m < g.M;
            }
            if (live) *reinterpret_cast<half8*>(out + m * p.ld_out + cc * 8) = *reinterpret_cast<const half8*>(stage + row * sp + cc * 16);
        }
        // (no third barrier: the next tile's patch writes follow this tile's last patch read by a barrier, and its staging writes follow
        // its own first barrier, which every lane reaches after its staging reads above have returned)
    }
}

size_t gr_lds_bytes(const ConvArgs& a) {
    const int taps = a.kh * a.kw;
    const int ph = taps == 9 ? kRows + 2 : kRows, pw = taps == 9 ? 18 : 16;
    return (size_t)(a.Cin / 16) * ph * pw * 32 + (size_t)kTilePx * (a.Cout * 2 + 16);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int TAPS, int CING, int UPW>
int32_t launch_grouped(const ConvArgs& a, const GrGeom& g, hipStream_t s) {
    const int grid = std::min(g.total_tiles, kMaxGrid);
    TRTX_LAUNCH((conv_grouped_f16_kernel<TAPS, CING, UPW>), dim3(grid), dim3(256), gr_lds_bytes(a), s, a, g);
    return check_launch("conv_grouped_f16");
}

}  // namespace

int conv_grouped_kpad(const ConvArgs& a) { return (a.kh * a.kw * (a.Cin / std::max(a.groups, 1)) + 31) / 32 * 32; }

bool conv_grouped_supported(const ConvArgs& a) {
    if (a.in_i8 || a.out_i8 || a.res_i8 || a.f32 || a.up_C != 0) return false;
    if (a.groups < 2 || a.groups > 8 || a.Cin <= 0 || a.Cout <= 0 || a.Cin % a.groups || a.Cout % a.groups) return false;
    const int cg = a.Cin / a.groups, og = a.Cout / a.groups;
    if (cg % 16 || og % 16 || cg > 64 || og > 64) return false;
    const bool k1 = a.kh == 1 && a.kw == 1 && a.pad_h == 0 && a.pad_w == 0;
    const bool k3 = a.kh == 3 && a.kw == 3 && a.pad_h == 1 && a.pad_w == 1;
    if (!k1 && !k3) return false;
    if (a.stride_h != 1 || a.stride_w != 1 || a.dil_h != 1 || a.dil_w != 1 || a.Ho != a.H || a.Wo != a.W) return false;
    if (a.ld_in % 8 || a.ld_out % 8 || a.ld_in < a.Cin || a.ld_out < a.Cout || (a.residual && (a.ld_res % 8 || a.ld_res < a.Cout))) return false;
    if (a.Cout / 16 > kMaxUnits || gr_lds_bytes(a) > (size_t)kLdsBudget) return false;
    // tile counts and pixel indices are ints
    return (long)a.N * a.Ho * a.Wo < (1L << 30);
}

int32_t conv_grouped(const ConvArgs& a, hipStream_t s) {
    if (!conv_grouped_supported(a) || a.Kpad != conv_grouped_kpad(a)) return TRTX_ERR_UNSUPPORTED;
    if (!a.in || !a.out || !a.wgt || !aligned16(a.in) || !aligned16(a.out) || !aligned16(a.wgt) || (a.residual && !aligned16(a.residual)) ||
        (a.bias && !aligned16(a.bias)))
        return TRTX_ERR_INVALID;
    GrGeom g{};
    g.M = a.N * a.Ho * a.Wo;
    if (g.M <= 0) return TRTX_OK;
    if (a.kh == 3) {
        g.tiles_x = (a.Wo + 15) / 16;
        g.tiles_y = (a.Ho + kRows - 1) / kRows;
        g.total_tiles = a.N * g.tiles_x * g.tiles_y;
    } else {
        g.tiles_x = (g.M + kTilePx - 1) / kTilePx;
        g.tiles_y = 1;
        g.total_tiles = g.tiles_x;
    }
    const int cing = a.Cin / a.groups / 16, upw = (a.Cout / 16 + 3) / 4;
#define GR_CASE(T, C, U) \
    if (a.kh * a.kw == T && cing == C && upw == U) return launch_grouped<T, C, U>(a, g, s);
    GR_CASE(9, 1, 1) GR_CASE(9, 1, 2) GR_CASE(9, 2, 1) GR_CASE(9, 2, 2) GR_CASE(9, 3, 1) GR_CASE(9, 3, 2) GR_CASE(9, 4, 1) GR_CASE(9, 4, 2)
    GR_CASE(1, 1, 1) GR_CASE(1, 1, 2) GR_CASE(1, 2, 1) GR_CASE(1, 2, 2) GR_CASE(1, 3, 1) GR_CASE(1, 3, 2) GR_CASE(1, 4, 1) GR_CASE(1, 4, 2)
#undef GR_CASE
    return TRTX_ERR_UNSUPPORTED;
}

}  // namespace trtx
