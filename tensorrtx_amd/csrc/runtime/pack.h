// Host-side weight re-layout used at engine-build time (and by the single-op test entry points).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace trtx {

struct ConvArgs;
enum ConvRoute : int;

// Each family's packed layout, stated once: the packed-geometry fields of a ConvArgs (bn, bk, CinK, K, Kpad, Cout_pad) from its logical geometry (Cin, Cout,
// kh, kw, groups).  The lowering, the single-op entry points and the packers below all take the layout from here; a kernel's _supported() checks it.
//  - fp16 implicit GEMM: the caller chooses the k-step bk (conv_igemm_pick_bk, or 32 where the plan's batch says so); Cin is already a multiple of 8
void conv_layout_igemm_f16(ConvArgs* a, int bk);
//  - int8 implicit GEMM: 64-channel k-steps.  Takes Cin and ld_in in channels and leaves them, like CinK / K / Kpad, in 2-byte units (ConvArgs::in_i8, which it sets)
void conv_layout_igemm_i8(ConvArgs* a);
//  - fp32 implicit GEMM (ConvArgs::f32, which it sets): 16-channel k-steps, the tile shape left to the launcher (bn = bm = 0)
void conv_layout_igemm_f32(ConvArgs* a);
//  - channel views (kernels/conv_view.hip): the fp16 implicit-GEMM rows with CinK = Cin rounded up to 32
void conv_layout_view(ConvArgs* a);
//  - grouped (kernels/conv_grouped.hip): K per group, rows of conv_grouped_kpad()
void conv_layout_grouped(ConvArgs* a);
//  - fp32 engines' grouped / channel-view kernel (kernels/conv_patch_f32.hip; sets ConvArgs::f32): groups == 1 the fp32 implicit-GEMM rows exactly, grouped the
//    rows of conv_layout_grouped.  No layout of its own: the kernel reads what those two families pack, in fp32
void conv_layout_patch_f32(ConvArgs* a);
//  - many narrow groups (kernels/conv_slab.hip): conv_layout_slab, declared with the kernel in kernels/kernels.h: rows of conv_slab_kpad(); for 16 and 32
//    channels per group these are conv_layout_grouped's rows
//  - direct, depthwise, stem, deconvolution: nothing is padded
void conv_layout_unpadded(ConvArgs* a);
// Bytes of the packed filter of a convolution on `route` (what pack_weights reserves, and the weight term of POp::bytes)
size_t conv_packed_weight_bytes(ConvRoute route, const ConvArgs& a);

// TensorRT conv weights are KCRS fp32 ([Cout][Cin][kh][kw]).  The implicit-GEMM kernel wants
// fp16 [cout_pad][kpad] with k = (r*kw + q)*cink + c (cink = CinK, the per-tap stride), zero padded (conv_layout_igemm_f16 / conv_layout_view); an optional
// per-output-channel scale (folded BatchNorm, yolov8/src/block.cpp:45-77) is multiplied in before rounding to fp16.
void pack_conv_weights_f16(const float* w_kcrs, int cout, int cin, int kh, int kw, int cink, int kpad, int cout_pad,
                           const float* ch_scale, uint16_t* packed);

// fp32 [Cout][kh][kw][Cin/groups] for the generic direct kernel (KCRS source, Cin here = per group)
void pack_conv_weights_f32(const float* w_kcrs, int cout, int cin_g, int kh, int kw, const float* ch_scale,
                           float* packed);

// fp16 [group][Cout_g][kpad] = rows [Cout][kpad] for the grouped MFMA kernel (kernels/conv_grouped.hip): k = (r*kw + q)*cin_g + c, kpad = K rounded
// up to 32, zero padded; the per-output-channel scale is multiplied in before rounding to fp16, as in pack_conv_weights_f16.
// slab > cin_g (kernels/conv_slab.hip, Cout_g == Cin_g below 16): the rows are block-diagonal inside slabs of `slab` channels, k = (r*kw + q)*slab + c_local
// with c_local = the row's group's first channel inside its slab + c, zero outside the group (conv_layout_slab); slab <= cin_g: the rows above exactly
void pack_conv_weights_grouped_f16(const float* w_kcrs, int cout, int cin_g, int kh, int kw, int kpad, const float* ch_scale, uint16_t* packed, int slab = 0);

// ... and the same rows in fp32 (kernels/conv_patch_f32.hip, grouped layers)
void pack_conv_weights_grouped_f32(const float* w_kcrs, int cout, int cin_g, int kh, int kw, int kpad, const float* ch_scale, float* packed);

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
