// The epilogue activations of the convolution and layer kernels, one definition per NUMERIC FAMILY, and the vector types the kernels share.
// Which family a kernel uses is part of its contract: the parity bounds of the tests rest on it, and kernels that must return the same bits
// (the exchangeable tactics of one layer) must use the same one.  A new activation kind is added here, once per family.
// ACT_GELU_TANH (gelu_tanh_ref, common.h: the reference's constants, the accurate tanhf) is the same expression in every family.
#pragma once
#include <hip/hip_runtime.h>

#include "../common.h"
#include "kernels.h"

namespace trtx {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef int intx4 __attribute__((ext_vector_type(4)));

// ---- fast: the fp16 MFMA kernels (igemm_tile.h and its wave-split-K / resident-patch forms, conv_gemm256.hip, conv_ws.hip, conv_grouped.hip).
// SiLU / sigmoid on the hardware's v_exp_f32 / v_rcp_f32 (1 ulp each, far below the fp16 rounding of the result that follows); the epilogues are
// VALU-issue bound and an IEEE division is ~10 instructions per element.  These kernels are exchangeable tactics of one layer: one expression,
// the same bits.  The rare kinds are out of line: one copy in the kernel instead of one per call site (code size is a cost there).
__device__ __attribute__((noinline)) float act_fast_rare(float v, int act, float alpha) {
    switch (act) {
        case ACT_SIGMOID: return __builtin_amdgcn_rcpf(1.0f + __expf(-v));
        case ACT_LEAKY: return v > 0.f ? v : v * alpha;
        case ACT_TANH: return tanhf(v);
        case ACT_MISH: return mish_ref(v);
        case ACT_GELU_TANH: return gelu_tanh_ref(v);
        default: return v;
    }
}
__device__ __forceinline__ float act_fast(float v, int act, float alpha) {
    if (act == ACT_NONE) return v;
    if (act == ACT_SILU) return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
    if (act == ACT_RELU) return v > 0.f ? v : 0.f;
    return act_fast_rare(v, act, alpha);
}

// ---- fp32 engine: conv_epilogue_f32 (igemm_tile.h: the fp32 implicit-GEMM, resident-patch and resident-operand kernels) and conv_stem_f32.hip.
// SiLU / sigmoid are v * rcp(1 + exp2(-v log2 e)) on v_exp_f32 / v_rcp_f32 (1 ulp each): 5 instructions per element where expf + an IEEE division
// are ~30.  Measured on the first build (round 5): with the accurate forms a 128 x 80 tile's epilogue was ~7k cycles of VALU issue per wave - 12 %
// of a 45-step 3x3 and MORE than the whole k-loop of a 4-step 1x1 - for an error 60x below what 63 layers of fp32 summation leave on a logit
// (7e-5 at 640 x 640, against BASELINE's 1e-4).
__device__ __attribute__((noinline)) float act_f32_rare(float v, int act, float alpha) {
    switch (act) {
        case ACT_LEAKY: return v > 0.f ? v : v * alpha;
        case ACT_TANH: return tanhf(v);
        case ACT_MISH: return mish_ref(v);
        case ACT_GELU_TANH: return gelu_tanh_ref(v);
        default: return v;
    }
}
__device__ __forceinline__ float act_f32(float v, int act, float alpha) {
    if (act == ACT_NONE) return v;
    if (act == ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == ACT_SILU || act == ACT_SIGMOID) {
        const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896341f));
        return act == ACT_SILU ? v * sg : sg;
    }
    return act_f32_rare(v, act, alpha);
}

// ---- exact: the generic kernels (nhwc_ops.hip, linear_ops.hip, conv_dw.hip), fp32 and fp16 alike: the accurate expf and an IEEE division.
// They are memory-bound, so the ~30 instructions per element are free, and they are what the layer tests pin on fp64 references.
__device__ __forceinline__ float act_exact(float v, int act, float alpha) {
    switch (act) {
        case ACT_RELU: return v > 0.f ? v : 0.f;
        case ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
        case ACT_SILU: return v / (1.0f + expf(-v));
        case ACT_LEAKY: return v > 0.f ? v : v * alpha;
        case ACT_TANH: return tanhf(v);
        case ACT_MISH: return mish_ref(v);
        case ACT_GELU_TANH: return gelu_tanh_ref(v);
        case ACT_EXP: return expf(v);   // IUnaryLayer kEXP: the accurate expf in fp32, rounded once by the caller's store
        default: return v;
    }
}

// ---- stem: conv_stem.hip (the fp16 engines' first layer): the hardware exponential, but an IEEE division.  The kernel is bound by HBM, the division
// costs nothing there, and its outputs are what every later layer of the engine was measured on.
__device__ __forceinline__ float act_stem(float v, int act, float alpha) {
    switch (act) {
        case ACT_RELU: return v > 0.f ? v : 0.f;
        case ACT_SIGMOID: return 1.0f / (1.0f + __expf(-v));
        case ACT_SILU: return v / (1.0f + __expf(-v));
        case ACT_LEAKY: return v > 0.f ? v : v * alpha;
        case ACT_TANH: return tanhf(v);
        case ACT_MISH: return mish_ref(v);
        case ACT_GELU_TANH: return gelu_tanh_ref(v);
        default: return v;
    }
}

}  // namespace
}  // namespace trtx
