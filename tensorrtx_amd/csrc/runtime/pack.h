// Host-side weight re-layout used at engine-build time (and by the single-op test entry points).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace trtx {

// TensorRT conv weights are KCRS fp32 ([Cout][Cin][kh][kw]).  The implicit-GEMM kernel wants
// fp16 [Cout_pad][Kpad = kh*kw*cin_pad rounded up to bk] with k = (r*kw + q)*cin_pad + c (cin_pad = CinK, the per-tap stride), zero padded; an optional per-output-channel
// scale (folded BatchNorm, yolov8/src/block.cpp:45-77) is multiplied in before rounding to fp16.
void pack_conv_weights_f16(const float* w_kcrs, int cout, int cin, int kh, int kw, int cin_pad, int bk,
                           const float* ch_scale, uint16_t* packed);

// fp32 [Cout][kh][kw][Cin/groups] for the generic direct kernel (KCRS source, Cin here = per group)
void pack_conv_weights_f32(const float* w_kcrs, int cout, int cin_g, int kh, int kw, const float* ch_scale,
                           float* packed);

// fp16 [group][Cout_g][kpad] = rows [Cout][kpad] for the grouped MFMA kernel (kernels/conv_grouped.hip): k = (r*kw + q)*cin_g + c, kpad = K rounded
// up to 32, zero padded; the per-output-channel scale is multiplied in before rounding to fp16, as in pack_conv_weights_f16
void pack_conv_weights_grouped_f16(const float* w_kcrs, int cout, int cin_g, int kh, int kw, int kpad, const float* ch_scale, uint16_t* packed);

// TensorRT deconvolution weights are CKRS ([Cin][Cout/groups][kh][kw]); gather form for
// deconv_direct is [Cout][kh][kw][Cin/groups].
void pack_deconv_weights_f32(const float* w_ckrs, int cin, int cout, int groups, int kh, int kw, float* packed);

// ReOrg (four stride-2 slices + concat) in front of a kh x kw stride-1 convolution over 4 cin channels, as one 2kh x 2kw stride-2
// convolution over cin channels (runtime/lower_match.cpp, match_reorg_fold): out [cout][cin][2kh][2kw] from KCRS w [cout][4 cin][kh][kw]
void reorg_fold_weights(const float* w, int cout, int cin, int kh, int kw, float* out);
// RepVGGDW's two depthwise branches as one 7x7 filter [channels][7][7] and one shift per channel (pack.cpp)
void repvggdw_fold_weights(const float* w7, const float* scale7, const float* shift7, const float* bias7, const float* w3, const float* scale3,
                           const float* shift3, const float* bias3, int channels, float* w_out, float* shift_out);

uint16_t f32_to_f16_bits(float f);
float f16_bits_to_f32(uint16_t h);

}  // namespace trtx
