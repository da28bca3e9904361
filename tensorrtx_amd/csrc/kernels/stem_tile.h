// Device code the stem kernels share (conv_stem.hip: conv_stem_lds_kernel / conv_stem_frames_kernel; conv_stem_pair.hip: the stem fused into the
// convolution behind it): the fp32 input patch of a tile global -> LDS, the per-lane registers (weights as MFMA A fragments, tap offsets, bias) and
// the arithmetic that turns an accumulator fragment into four fp16 channels.  One definition each: the kernels must produce the same bits.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "act.h"
#include "kernels.h"

namespace trtx {
namespace {

typedef __attribute__((address_space(3))) void* stem_lds_ptr_t;

struct StemGeom {
    int PR, PCA;            // input patch rows / 4-float-aligned columns staged in LDS per channel
    int tiles_x, tiles_y;
    int chunks;             // 16-byte chunks of the patch (Cin * PR * PCA / 4)
};

// Stage 1 of a tile, first half: the fp32 input patch (Cin x PR x PCA floats, top-left input pixel (hi_start, al_start), al_start a multiple of 4)
// of image n goes HBM -> LDS with 16-byte LDS-DMA loads; rows and columns outside the image are range-checked to zero by the buffer descriptor.
// The caller waits for the loads (s_waitcnt vmcnt(0)) and passes a barrier before stem_patch_tail.
__device__ __forceinline__ void stem_patch_fetch(const ConvArgs& p, const StemGeom& g, unsigned in_bytes, float* s_patch, int n, int hi_start, int al_start) {
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.in), 0, in_bytes, 0x00020000);
    const int cpr = g.PCA / 4;                  // chunks per patch row
    const float inv_cpr = 1.0f / (float)cpr, inv_pr = 1.0f / (float)g.PR;
    for (int base = 0; base < g.chunks; base += 256) {
        const int ci = base + tid;
        int row = (int)((float)ci * inv_cpr);   // (c * PR + pr); estimate within +-1, fixed up exactly
        int cq = ci - row * cpr;
        if (cq < 0) { --row; cq += cpr; }
        if (cq >= cpr) { ++row; cq -= cpr; }
        int c = (int)((float)row * inv_pr);
        int pr = row - c * g.PR;
        if (pr < 0) { --c; pr += g.PR; }
        if (pr >= g.PR) { ++c; pr -= g.PR; }
        const int hi = hi_start + pr, wi = al_start + cq * 4;
        const bool ok = ci < g.chunks && (unsigned)hi < (unsigned)p.H && wi >= 0 && wi + 3 < p.W;
        const unsigned off = ok ? (unsigned)(((((long)n * p.Cin + c) * p.H + hi) * p.W + wi) * 4) : 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (stem_lds_ptr_t)(s_patch + (size_t)(base + wave * 64) * 4), 16, off, 0, 0, 0);
    }
}

// ... second half, after the loads have landed and a barrier: the `W & 3` tail, followed by a barrier of its own where it runs.
__device__ __forceinline__ void stem_patch_tail(const ConvArgs& p, const StemGeom& g, float* s_patch, int n, int hi_start, int al_start) {
    const int tid = threadIdx.x;
    if (p.W & 3) {
        // Ragged width (Faster R-CNN's 1333): the 16-byte chunk that straddles the end of an image row was range-checked away whole
        // above; its 1..3 real pixels are fetched here, one patch row per thread (right-edge tiles only have any)
        const int cpr = g.PCA / 4, rows = p.Cin * g.PR, wtail = p.W & ~3;
        const int cq = (wtail - al_start) >> 2;
        if (cq >= 0 && cq < cpr && wtail >= al_start) {
            const float* __restrict__ src = static_cast<const float*>(p.in);
            for (int rrow = tid; rrow < rows; rrow += 256) {
                const int c = rrow / g.PR, pr = rrow - c * g.PR, hi = hi_start + pr;
                if ((unsigned)hi >= (unsigned)p.H) continue;
                const size_t base = (((size_t)n * p.Cin + c) * p.H + hi) * p.W;
                for (int e = 0; e < 4; ++e)
                    if (wtail + e < p.W) s_patch[((size_t)rrow * cpr + cq) * 4 + e] = src[base + wtail + e];
            }
        }
        __syncthreads();
    }
}

// what a workgroup keeps in registers for all of its tiles: the weights as MFMA A fragments, the patch offsets of its taps, its bias
template <int NFRAG, int KS>
struct StemRegs {
    half8 wf[NFRAG][KS];
    int l_off[KS][8];   // float index inside the patch of tap (c, r, q) relative to the pixel's top-left corner
    float bias4[NFRAG][4];
};

// weights, tap tables and bias of a lane.  EVERY load is issued unconditionally from a clamped index and masked afterwards: written as
// `cond ? w[i] : 0` the compiler put each of the 160 loads of the 7x7 stem (176 with the bias) into its own exec-masked branch with an
// s_waitcnt vmcnt(0) behind it - 176 dependent round trips of ~700 cycles per workgroup, which is where conv_stem_lds_kernel<4, 5> spent its
// 148 us on ResNet-50's 224 x 224 batch 32 (12x its byte floor; profiles/r04_kernel_stats_c2_1ctx_lanes1.txt) and 888 us on RetinaFace's 1280 x 1280.
template <int NFRAG, int KS>
__device__ __forceinline__ void stem_setup(const ConvArgs& p, const StemGeom& g, StemRegs<NFRAG, KS>& R) {
    const int lane = threadIdx.x & 63;
    const int khw = p.kh * p.kw;
    const int K = khw * p.Cin;
    const float* __restrict__ w = static_cast<const float*>(p.wgt);  // [tap = (c*kh + r)*kw + q][Cout]
    const int kq = (lane >> 4) * 8;
    auto& wf = R.wf;
    auto& l_off = R.l_off;
    auto& bias4 = R.bias4;
    const float inv_khw = 1.0f / (float)khw, inv_kw = 1.0f / (float)p.kw;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = ks * 32 + kq + e;
            // k < 160, khw <= 49: (k + 0.5) / d is never within rounding distance of an integer, the floor is exact
            const int c = (int)(((float)k + 0.5f) * inv_khw), rem = k - c * khw;
            const int r = (int)(((float)rem + 0.5f) * inv_kw), q = rem - r * p.kw;
            l_off[ks][e] = k < K ? (c * g.PR + r) * g.PCA + q : 0;  // padded taps: zero weights, any valid address
#pragma unroll
            for (int j = 0; j < NFRAG; ++j) {
                const int co = j * 16 + (lane & 15);
                const float wv = w[(size_t)(k < K ? k : K - 1) * p.Cout + (co < p.Cout ? co : p.Cout - 1)];
                wf[j][ks][e] = (k < K && co < p.Cout) ? (_Float16)wv : (_Float16)0.f;
            }
        }
    const int ch4 = (lane >> 4) * 4;
    const float* __restrict__ bsrc = p.bias ? p.bias : w;   // (wave-uniform; without a bias the loaded values are masked away)
#pragma unroll
    for (int j = 0; j < NFRAG; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = j * 16 + ch4 + e;
            const float bv = bsrc[co < p.Cout ? co : p.Cout - 1];
            bias4[j][e] = (p.bias && co < p.Cout) ? bv : 0.f;
        }
}

// one 16-pixel group: every lane gathers the 8 taps of its (pixel, k-chunk) from the patch at `src` (its pixel's top-left tap), converts to fp16
// and feeds the B operand of v_mfma_f32_16x16x32_f16; the weights are the A fragments
template <int NFRAG, int KS>
__device__ __forceinline__ void stem_group_mfma(const StemRegs<NFRAG, KS>& R, const float* src, floatx4 (&acc)[NFRAG]) {
#pragma unroll
    for (int j = 0; j < NFRAG; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        half8 xf;
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[e] = (_Float16)src[R.l_off[ks][e]];
#pragma unroll
        for (int j = 0; j < NFRAG; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(R.wf[j][ks], xf, acc[j], 0, 0, 0);
    }
}

// a lane's four channels of one pixel: round_to_half(act(acc + bias))
__device__ __forceinline__ half4 stem_finish4(const ConvArgs& p, const floatx4& acc, const float (&bias4)[4]) {
    half4 o;
    if (p.act1 == ACT_SILU) {  // wave-uniform: pick the activation once, not per element
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = acc[e] + bias4[e];
            o[e] = round_to_half(x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)));
        }
    } else if (p.act1 == ACT_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = acc[e] + bias4[e];
            o[e] = (_Float16)(x > 0.f ? x : 0.f);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = round_to_half(act_stem(acc[e] + bias4[e], p.act1, p.alpha1));
    }
    return o;
}

}  // namespace
}  // namespace trtx
