// Depthwise convolution (groups == Cin == Cout, odd k of 3 / 5 / 7 with 'same' padding k/2, stride 1 or 2, no dilation) on NHWC
// fp16 / fp32 tensors with any channel stride (views into concat buffers).  YOLO11's DWConv (yolo11/src/block.cpp:417-437) and the
// PSA attention's positional conv `pe` (block.cpp:329-331, g = dim) are this layer; the generic direct kernel (nhwc_ops.hip) runs it
// one scalar output per thread with an inner loop of length 1.
//
// The layer is HBM-bound (k*k MACs per element read).  One lane owns V channels (16 bytes: 8 halfs / 4 floats) of OW horizontally
// neighbouring output pixels: per filter row it walks the (OW-1)*S + k input pixels those outputs need once, each a 16-byte load,
// and adds every one into all the outputs whose window covers it - k*k*OW loads become k*((OW-1)*S + k).  Lanes of a wave take
// consecutive channel vectors of a pixel first, so a wave's loads are contiguous runs of the pixel's channels.  fp32 accumulation,
// summed in the direct kernel's order (bias first, then taps row by row); the direct kernel's epilogue: act1, + residual, act2.
//
// Weights: fp32 [kh*kw][C] (tap-major, the folded BN scale applied; runtime/pack.cpp pack_weights), bias fp32 [C].
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../common.h"
#include "act.h"
#include "kernels.h"

namespace trtx {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;
constexpr int kOW = 4;   // output pixels per lane

inline int grid_for(long work) {
    long b = (work + kThreads - 1) / kThreads;
    if (b < 1) b = 1;
    return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

template <typename T, int V>
__device__ __forceinline__ void load_vec(const T* p, float (&x)[V]) {
    const Pack<T, V> v = *reinterpret_cast<const Pack<T, V>*>(p);
#pragma unroll
    for (int e = 0; e < V; ++e) x[e] = (float)v.v[e];
}

template <typename T, int V, int K, int S>
__global__ __launch_bounds__(kThreads) void conv_dw_kernel(const ConvArgs p) {
    constexpr int NW = (kOW - 1) * S + K;   // input columns the lane's outputs read per filter row
    const T* __restrict__ in = static_cast<const T*>(p.in);
    const float* __restrict__ w = static_cast<const float*>(p.wgt);
    const T* __restrict__ res = static_cast<const T*>(p.residual);
    T* __restrict__ out = static_cast<T*>(p.out);
    const int C = p.Cout;
    const int CV = C / V;
    const int strips = (p.Wo + kOW - 1) / kOW;
    const long total = (long)p.N * p.Ho * strips * CV;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cv = (int)(i % CV);
        long t = i / CV;
        const int s = (int)(t % strips);
        t /= strips;
        const int ho = (int)(t % p.Ho);
        const long n = t / p.Ho;
        const int c0 = cv * V;
        const int wo0 = s * kOW;
        const int wi0 = wo0 * S - p.pad_w;
        float acc[kOW][V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float b = p.bias ? p.bias[c0 + e] : 0.f;
#pragma unroll
            for (int o = 0; o < kOW; ++o) acc[o][e] = b;
        }
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int hi = ho * S - p.pad_h + r;
            if ((unsigned)hi >= (unsigned)p.H) continue;
            float wr[K][V];
#pragma unroll
            for (int q = 0; q < K; ++q)
#pragma unroll
                for (int e = 0; e < V; ++e) wr[q][e] = w[(size_t)(r * K + q) * C + c0 + e];
            const T* row = in + ((n * p.H + hi) * p.W) * (long)p.ld_in + c0;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int wi = wi0 + j;
                if ((unsigned)wi >= (unsigned)p.W) continue;
                float x[V];
                load_vec<T, V>(row + (long)wi * p.ld_in, x);
#pragma unroll
                for (int o = 0; o < kOW; ++o) {
                    const int q = j - o * S;   // compile-time after unrolling
                    if (q < 0 || q >= K) continue;
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[o][e] = fmaf(x[e], wr[q][e], acc[o][e]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < kOW; ++o) {
            const int wo = wo0 + o;
            if (wo >= p.Wo) break;
            const long m = (n * p.Ho + ho) * p.Wo + wo;
            float r[V];
            if (res) load_vec<T, V>(res + m * p.ld_res + c0, r);
            Pack<T, V> v;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float y = act_exact(acc[o][e], p.act1, p.alpha1);
                if (res) y += r[e];
                y = act_exact(y, p.act2, p.alpha2);
                v.v[e] = (T)y;
            }
            *reinterpret_cast<Pack<T, V>*>(out + m * p.ld_out + c0) = v;
        }
    }
}

template <typename T, int V>
int32_t launch_v(const ConvArgs& a, hipStream_t s) {
    const long total = (long)a.N * a.Ho * ((a.Wo + kOW - 1) / kOW) * (a.Cout / V);
    if (total == 0) return TRTX_OK;
    const dim3 g(grid_for(total)), b(kThreads);
#define DW_CASE(K, S) \
    if (a.kh == K && a.stride_h == S) { hipLaunchKernelGGL((conv_dw_kernel<T, V, K, S>), g, b, 0, s, a); return check_launch("conv_dw"); }
    DW_CASE(3, 1) DW_CASE(3, 2) DW_CASE(5, 1) DW_CASE(5, 2) DW_CASE(7, 1) DW_CASE(7, 2)
#undef DW_CASE
    return TRTX_ERR_UNSUPPORTED;
}

bool aligned(const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

bool conv_dw_supported(const ConvArgs& a) {
    return a.groups == a.Cin && a.Cin == a.Cout && a.Cout > 0 && a.kh == a.kw && (a.kh == 3 || a.kh == 5 || a.kh == 7) && a.pad_h == a.kh / 2 &&
           a.pad_w == a.kw / 2 && a.stride_h == a.stride_w && (a.stride_h == 1 || a.stride_h == 2) && a.dil_h == 1 && a.dil_w == 1 &&
           a.Ho == (a.H + 2 * a.pad_h - a.kh) / a.stride_h + 1 && a.Wo == (a.W + 2 * a.pad_w - a.kw) / a.stride_w + 1 && !a.in_i8 && !a.out_i8 &&
           !a.res_i8 && a.up_C == 0;
}

int32_t conv_dw(const ConvArgs& a, int dtype, hipStream_t s) {
    if (!conv_dw_supported(a)) return TRTX_ERR_UNSUPPORTED;
    const int v = dtype == DT_F16 ? 8 : 4;
    const bool vec = a.Cout % v == 0 && a.ld_in % v == 0 && a.ld_out % v == 0 && (!a.residual || a.ld_res % v == 0) && aligned(a.in) &&
                     aligned(a.out) && aligned(a.residual);
    if (dtype == DT_F16) return vec ? launch_v<_Float16, 8>(a, s) : launch_v<_Float16, 1>(a, s);
    return vec ? launch_v<float, 4>(a, s) : launch_v<float, 1>(a, s);
}

}  // namespace trtx
