// Internal kernel-launcher interface (C++), used by the runtime executor and by the thin
// extern "C" test/bench entry points in ops_capi.cpp.  Everything here runs on a HIP stream;
// nothing falls back to the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace trtx {

enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2, ACT_SILU = 3, ACT_LEAKY = 4, ACT_TANH = 5,
                 ACT_MISH = 6 /* x * tanh(softplus(x)), the reference's Mish_TRT plugin (yolov4/mish.cu:113-135) */,
                 ACT_GELU_TANH = 7 /* 0.5 x (1 + tanh(0.797885 (x + 0.044715 x^3))), the reference's eleven-layer GELU() (yolov13/src/block.cpp:702-744) */,
                 ACT_EXP = 8 /* e^x, IUnaryLayer kEXP (yolov13/src/block.cpp:389); an op of its own in the generic kernels (act_exact), never a convolution's epilogue */ };
enum DType : int { DT_F32 = 0, DT_F16 = 1, DT_I8 = 2 };
inline size_t dtype_size(int dt) { return dt == DT_F16 ? 2 : (dt == DT_I8 ? 1 : 4); }
enum EwOp : int { EW_SUM = 0, EW_PROD = 1, EW_MAX = 2, EW_MIN = 3, EW_SUB = 4, EW_DIV = 5, EW_POW = 6 };
enum PoolOp : int { POOL_MAX = 0, POOL_AVG = 1 };

// Values of ConvArgs::t_ws / ConvTactic::ws: which kernel of the implicit-GEMM family runs the layer.  The numbers are stored in plans and tactic caches and
// cross the C ABI (trtx_op_conv2d_tactics), so they stay what they are; the fields stay int.
enum Ws : int {
    WS_AUTO = 0,       // the weight-stationary kernel (conv_ws.hip) where it is supported, else the implicit-GEMM kernel
    WS_OFF = 1,        // never the weight-stationary kernel
    WS_ON = 2,         // the weight-stationary kernel asked for (still only where supported)
    WS_PATCH = 3,      // the resident-patch 3x3 kernel (patch_tile.h)
    WS_F32_REGS = 5,   // (fp32 launches) operands through registers
    WS_F32_ROLES = 6,  // (fp32 launches) fetching + multiplying wave roles
    WS_RES3 = 7,       // the resident-operand 3x3 kernel (conv_res.hip)
    WS_RES1 = 8,       // ... and its 1x1 sibling
};
// Values of ConvArgs::t_wsk / ConvTactic::wsk: the wave-split-K variant (conv_igemm_wsk_f16_kernel)
enum Wsk : int {
    WSK_RULE = 0,  // by the static rule (few tiles, a long k-chain)
    WSK_OFF = 1,   // never
    WSK_ON = 2,    // wherever it exists
};

// One fused convolution launch.  Activations are NHWC; `in`/`out`/`residual` already point at the
// first channel of the slice they address and ld_* is the channel stride of the underlying buffer.
struct ConvArgs {
    const void* in;
    const void* wgt;    // igemm: fp16 [Cout_pad][Kpad], k = (r*kw+q)*CinK + c.  direct: fp32 [Cout][kh*kw*Cin/groups]
    const float* bias;  // [Cout_pad] (folded BN shift / conv bias) or nullptr
    void* out;
    const void* residual;  // same geometry as out, or nullptr
    int N, H, W, Cin, ld_in;
    int Ho, Wo, Cout, Cout_pad, ld_out, ld_res;
    int kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups;
    int K, Kpad, M;
    int act1, act2;
    float alpha1, alpha2;
    int bn;  // igemm column-tile width (16/32/64/80/128)
    int scalar_out;  // igemm: element-wise epilogue stores (Cout, channel stride or offset not a multiple of 8)
    int CinK;        // igemm: per-tap stride of the packed K axis: Cin rounded up to bk, or 16 (two taps per step);
                     // Kpad = kh*kw*CinK rounded up to bk
    int bk;          // igemm: k-step width in halfs (32, or 64 when CinK % 64 == 0)
    // INT8 (kINT8 engines, conv_igemm only).  in_i8: activations and weights are int8, accumulated by v_mfma_i32_16x16x64_i8;
    // the input-side fields Cin, ld_in, CinK, K, Kpad are then counted in PAIRS of int8 channels (= 2-byte units), so that
    // every byte offset the kernel derives is the one the fp16 kernel would derive; Cout / ld_out / ld_res stay in channels.
    // out = act(acc * cscale[c] + bias[c]) with cscale[c] = input_scale * weight_scale[c]; out_i8: quantised with out_inv_scale
    // (round to nearest even, clamp +-127); res_i8: the residual is int8 with scale res_scale.
    int in_i8, out_i8, res_i8;
    const float* cscale;   // [Cout_pad]
    float out_inv_scale, res_scale;
    // Tactic (see ConvTactic): 0 everywhere = the untuned dispatch.
    int bm;     // igemm rows per tile: 0 / 128, 64 or 256
    int t_wsk;  // a Wsk value
    int t_ws;   // a Ws value
    int t_rs;   // implicit-GEMM operands through registers (global -> VGPR -> ds_write) instead of LDS-DMA: 0 = no, 1 = yes (same bits)
    // Folded nearest 2x upsample (conv_igemm main kernel, 1x1 stride-1 convolutions only): input channels [0, up_C) are not read from
    // `in` but from `up_in`, an NHWC fp16 tensor of HALF the resolution ([N][up_H][up_W][up_ld], H = 2 up_H, W = 2 up_W), at pixel
    // (h >> 1, w >> 1); channels >= up_C come from `in` as usual.  This is Upsample -> Concat -> Conv1x1 (YOLOv8 head, model.cpp:130-160)
    // without the upsampled tensor ever existing.  up_C = 0: off.
    const void* up_in;
    int up_C, up_ld, up_H, up_W;
    // fp32 engines (builds without kFP16; conv_igemm_f32.hip): activations, residual and packed weights are fp32, the k-step is 16 channels
    // (bk == 16; CinK = Cin rounded up to 16, or 8 for Cin <= 8: two filter taps per step), Kpad = K rounded up to 16.  All fields in channels.
    int f32;
    // The layer's summation order is pinned to the main kernel's (lowering: members of a grouped launch, and the would-be members under TRTX_GROUP_CONVS=0):
    // conv_tactics() lists no wave-split-K / weight-stationary candidate for it - the tuner cannot hand it another K order.  Part of the tactic signature.
    int k_pinned;
};

// One launch configuration of an implicit-GEMM layer.  All tactics of a layer share its packed weights (Cout_pad, CinK, Kpad), so
// the executor may exchange them at run time: runtime/tune.cpp times them in place and keeps the fastest (TensorRT's builder does
// the same with its tactics; here it happens at deserializeCudaEngine because plans store the network, not kernels).
struct ConvTactic {
    int bn, bk, bm;  // column-tile width, k-step width, rows per tile
    int wsk, ws;     // values of ConvArgs::t_wsk / t_ws (Wsk / Ws)
};

// Launch probe (IProfiler-style per-layer timing): while one is set for the calling thread, the first MFMA / stem convolution
// launch records the DISPATCH's own begin and end timestamps into its events (hipExtLaunchKernelGGL) - the kernel's duration as
// rocprofv3 sees it, without the hand-over between two stream events that bracketing a launch with hipEventRecord includes.
struct LaunchProbe {
    hipEvent_t start = nullptr, stop = nullptr;
    int launches = 0;
};
void conv_set_launch_probe(LaunchProbe* p);  // nullptr: off
LaunchProbe* conv_launch_probe();

// --- conv -------------------------------------------------------------------------------------------
// fused implicit-GEMM conv on MFMA (conv_igemm.hip): LDS-DMA operands, range-checked gather, 3-stage pipeline
int conv_igemm_pick_bn(int cout);   // column-tile width for a Cout
int conv_igemm_pick_bk(int cin, int taps);  // k-step width for a (padded-to-8) Cin and kh*kw filter taps
int conv_igemm_pick_cink(int cin, int bk);  // per-tap stride of the packed K axis
bool conv_igemm_supported(const ConvArgs& a);
// int8 weight packing: per-output-channel symmetric scales (max |w| / 127 after the BN scale is folded in), same [Cout_pad][Kpad]
// row layout as the fp16 packing with CinK = Cin rounded up to 64 channels; wscale_out[Cout_pad]
void conv_pack_weights_i8(const float* w_kcrs, int cout, int cin, int kh, int kw, int cink, const float* ch_scale, int cout_pad, int kpad,
                          int8_t* packed, float* wscale_out);
int32_t conv_igemm_f16(const ConvArgs& a, hipStream_t s);
// the tactics applicable to a layer (a.N / a.M at the batch it will run with); out[0] is the untuned default. Returns the count.
// work_efficient_only: leave out the configurations that buy latency with extra traffic (narrower column tiles re-read the
// activations, 64-row tiles re-read the weights) - what an engine whose contexts run side by side should choose from.
int conv_tactics(const ConvArgs& a, ConvTactic* out, int max_out, bool work_efficient_only = false);
void conv_apply_tactic(ConvArgs* a, const ConvTactic& t);
// Several independent fp16 implicit-GEMM convolutions in ONE launch (conv_igemm.hip conv_igemm_group_f16_kernel): the members share a
// kernel instantiation - 128-row tiles, one column-tile width (64 or 80), 32-wide k-steps, the same operand path (t_rs) and all or none of
// them plain 1x1 GEMMs - and each is computed exactly as its own launch would compute it (same tiles, same K order: the same bits).
constexpr int kMaxConvGroup = 4;
bool conv_igemm_group_supported(const ConvArgs* a, int n);
int32_t conv_igemm_group_f16(const ConvArgs* a, int n, hipStream_t s);
// Two such groups that read the SAME tensors in one launch (conv_igemm.hip conv_igemm_dual_group_f16_kernel; the detect head's cv2.x.0 and cv3.x.0): member k
// of a0 (-> 64 channels) and member k of a1 (-> 80) share their input pointer, geometry, filter, Kpad and k-step, and run as one 144-column tile whose A operand is
// fetched once; each output element is computed exactly as its own launch computes it (same K order, same epilogue: the same bits).  1 <= n <= kMaxDualGroup.
// _possible(): fp16 without a shortcut or folded upsample, CinK != 16, the main kernel's 128-row / 32-wide-step form on both sides (no wave-split-K,
// WS_PATCH or WS_RES* member; t_rs only chooses an operand path of the same bits - the dual tile always takes LDS-DMA), a per-problem input slice below 2 GB and - for whatever pointers are set - no output that overlaps an input or another output
// (channel slices side by side in one buffer do not overlap).  conv_dual_group_f16: TRTX_ERR_INVALID for such an overlap, TRTX_ERR_UNSUPPORTED otherwise refused.
constexpr int kMaxDualGroup = 3;
bool conv_dual_group_possible(const ConvArgs* a0, const ConvArgs* a1, int n);
int32_t conv_dual_group_f16(const ConvArgs* a0, const ConvArgs* a1, int n, hipStream_t s);
// ... where _possible() holds, otherwise exactly the two launches of each group on its own (n == 1: of each convolution).  What the executor issues at a marked op.
int32_t conv_dual_group_or_two_f16(const ConvArgs* a0, const ConvArgs* a1, int n, hipStream_t s);
// Large plain-GEMM convolutions on the 256 x 256 x 64 role-alternating tile (conv_gemm256.hip): the tactic ConvArgs::bn == 256 of the
// implicit-GEMM family (same packed weights, same bits); conv_igemm_f16 dispatches to it
bool conv_gemm256_possible(const ConvArgs& a);     // may run (any batch up to the build batch)
bool conv_gemm256_worthwhile(const ConvArgs& a);   // is a candidate of the tactic timing at this batch
int32_t conv_gemm256_f16(const ConvArgs& a, hipStream_t s);
// fp32 engines: the same skeleton on v_mfma_f32_16x16x4_f32 (conv_igemm_f32.hip).  ConvArgs::f32 = 1, bn / bm = 0: the launcher's own tile choice
int conv_igemm_f32_pick_cink(int cin);
bool conv_igemm_f32_supported(const ConvArgs& a);
int32_t conv_igemm_f32(const ConvArgs& a, hipStream_t s);
int conv_tactics_f32(const ConvArgs& a, ConvTactic* out, int max_out);   // (bn, bm) pairs; out[0] = the untuned choice; every pair returns the same bits
void conv_pack_weights_igemm_f32(const float* w_kcrs, int cout, int cin, int kh, int kw, int cink, int kpad, int cout_pad, const float* ch_scale, float* packed);
// Resident-operand 3x3 stride-1 kernel (conv_res.hip, round 6; tactic WS_RES3): persistent workgroups keep the layer's whole weight slab in LDS, two
// role-alternating halves of 4 waves (k-loop | register epilogue + next patch fetch); same packed weights, same K order, same bits as the main kernel.
// a[0..n): 1..kMaxConvGroup independent layers of one instantiation in one launch (a workgroup is bound to one of them).
bool conv_res_possible(const ConvArgs& a);
bool conv_res_group_possible(const ConvArgs* a, int n);
int32_t conv_res_f16(const ConvArgs* a, int n, hipStream_t s);
// ... and its 1x1 stride-1 sibling (tactic WS_RES1): the column tile's weights resident in LDS, 16 independent waves per workgroup, the A operand global -> VGPR
bool conv_res1_possible(const ConvArgs& a);
int32_t conv_res1_f16(const ConvArgs& a, hipStream_t s);
// weight-stationary persistent kernel for small-channel 3x3 (stride 1, pad 1) and 1x1 layers (conv_ws.hip): weights in
// registers, input patch staged once in LDS; same packed weights / ConvArgs as the implicit-GEMM kernel, which dispatches to it
bool conv_ws_supported(const ConvArgs& a);
int32_t conv_ws_f16(const ConvArgs& a, hipStream_t s);
int32_t poison_lds(unsigned* device_word, hipStream_t s);  // test support (test_support.hip): NaN patterns into every CU's LDS
// first layer: fp32 NCHW input (1..4 channels) -> NHWC fp16, weights fp32 [kh*kw*Cin (c,r,q)][Cout]
bool conv_stem_supported(const ConvArgs& a);
int32_t conv_stem_nchw_f32(const ConvArgs& a, hipStream_t s);
// ... and of an fp32 engine (conv_stem_f32.hip): the same input and weight layout, NHWC fp32 out, Cout a multiple of 16
bool conv_stem_f32_supported(const ConvArgs& a);
int32_t conv_stem_nchw_f32_out_f32(const ConvArgs& a, hipStream_t s);
// The stem fed by camera frames instead of the fp32 network input: image n of the batch is the letterbox (yolov8/src/preprocess.cu) of
// frames[n] - a device-resident uint8 HWC BGR image of w x h pixels with d2s = the inverse affine map trtx_letterbox_matrix computes
// for (w, h) -> (a.W, a.H) - sampled inside the kernel's patch fill.  a.in is ignored.  3-channel stems on the LDS / MFMA path only
// (TRTX_ERR_UNSUPPORTED otherwise: the caller then runs the letterbox kernel and the ordinary stem).
constexpr int kStemMaxFrames = 64;
struct StemFrame {
    const void* src;
    int w, h;
    float d2s[6];
};
int32_t conv_stem_frames_f32(const ConvArgs& a, const StemFrame* frames, hipStream_t s);
// The stem and the stride-2 3x3 convolution behind it in one launch (conv_stem_pair.hip): stem Cin <= 4 -> 16, then 16 -> 32, both 3x3 / 2 pad 1, fp16.
// `stem` as conv_stem_nchw_f32 takes it (its `out` is not written), `conv` as conv_igemm_f16 takes it (its `in` is not read): the same packed weights,
// the same bits as the stem followed by the implicit-GEMM kernel's main K order.  _possible(): geometry, and the alignment of whatever pointers are set.
bool conv_stem_pair_possible(const ConvArgs& stem, const ConvArgs& conv);
int32_t conv_stem_pair_f16(const ConvArgs& stem, const ConvArgs& conv, hipStream_t s);
// The two 3x3 convolutions of a 16-channel bottleneck in one launch (conv_bneck_pair.hip): 16 -> 16 -> 16, both 3x3 / 1 pad 1, fp16, the second with or
// without the first one's input as shortcut.  `first` and `second` as conv_igemm_f16 takes them (first.out is not written, second.in is not read;
// second.residual, if set, is first.in with ld_res == ld_in): the same packed weights, the same bits as two launches of the implicit-GEMM kernel's main
// K order.  _possible(): geometry, and the alignment / identity of whatever pointers are set (a residual below 4096 only says "there is one").
bool conv_bneck_pair_possible(const ConvArgs& first, const ConvArgs& second);
int32_t conv_bneck_pair_f16(const ConvArgs& first, const ConvArgs& second, hipStream_t s);
// ... where _possible() holds (it refuses an output that lies on the input other than as a different channel slice of one buffer: the fused kernel cannot run
// in place), otherwise the two launches: first.out, the tensor between them, is then written and second.in must be it.  What the executor issues at a marked op.
int32_t conv_bneck_pair_or_two_f16(const ConvArgs& first, const ConvArgs& second, hipStream_t s);
// generic direct convolution (any groups / dilation / channel count), T = activation dtype, fp32 weights
int32_t conv_direct(const ConvArgs& a, int dtype, hipStream_t s);
// depthwise convolution (conv_dw.hip): groups == Cin == Cout, k 3 / 5 / 7 with pad k/2, stride 1 / 2, no dilation; weights fp32 [kh*kw][C]
bool conv_dw_supported(const ConvArgs& a);
// fused PSA attention (attention.hip): NHWC fp16 qkv [B][N][ld_qkv] (head h: q at h*(2kd+hd), k next, v next) -> O [B][N][ld_out] and the
// gathered V image [B][N][ld_v], channel h*hd + d; kd == 32, hd == 64
bool psa_attention_supported(int kd, int hd);
int32_t psa_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int kd, int hd,
                          float scale, hipStream_t s);
// area attention on the matrix pipe (attention_mfma.hip; YOLOv12's AAttn): the same tensors as psa_attention_f16, the N pixels of an image
// split into `area` contiguous ranges of N / area pixels that attend within themselves (area = 1: the whole image); kd == hd == 32.
// A base pointer or channel stride that rules out 16-byte accesses takes element-wise loads / stores, not an error.
bool area_attention_supported(int kd, int hd);
int32_t area_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int area, int kd,
                           int hd, float scale, hipStream_t s);
// the same kernel body on separate operands (YOLOv13's AAttn, yolov13/src/block.cpp:303-423: q | k from one convolution, v from another): q, k, v
// are NHWC fp16 [B][N][ld], head h reads q and k channels h*kd .. and v channels h*hd ..; O as above, no V image (v is a tensor already).  Given the
// same values O is bit-equal to area_attention_f16's.  16-byte loads / 8-byte stores per operand where its base and stride allow, element-wise otherwise.
bool area_attention_split_supported(int kd, int hd);
int32_t area_attention_split_f16(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, void* out, int ld_out, int B, int heads, int N,
                                 int area, int kd, int hd, float scale, hipStream_t s);
int32_t conv_dw(const ConvArgs& a, int dtype, hipStream_t s);
// YOLOv13's adaptive hypergraph convolution (hgconv.hip; AdaHyperedgeGen + AdaHGConv, yolov13/src/block.cpp:607-790): NHWC fp16 x [B][N][ld_x] (D channels)
// -> out [B][N][ld_out] = GELU((A He') W_node^T + b_node) + x with A the softmax over the N nodes of an image.  D % 16 == 0, D <= 384, 1 <= E <= 16; x and out
// 16-byte aligned with pixel strides that are multiples of 8 (TRTX_ERR_UNSUPPORTED otherwise).  The weights are the layers' own fp32 arrays; `workspace`
// holds at least hgconv_workspace_bytes(B, N, D, E) bytes (a pure function of its arguments; 0 = unsupported), 16-byte aligned.
struct HgconvWeights {
    const float* w_ctx;    // context_net.weight [E D][2 D]
    const float* b_ctx;    // context_net.bias [E D]
    const float* proto;    // prototype_base [E][D]
    const float* w_pre;    // pre_head_proj.weight [D][D]
    const float* b_pre;    // pre_head_proj.bias [D]: constant over the nodes, cancels in the node softmax (never read; may be null)
    const float* w_edge;   // edge_proj.0.weight [D][D]
    const float* b_edge;   // edge_proj.0.bias [D]
    const float* w_node;   // node_proj.0.weight [D][D]
    const float* b_node;   // node_proj.0.bias [D]
};
bool hgconv_supported(int D, int E);
size_t hgconv_workspace_bytes(int B, int N, int D, int E);
int hgconv_geometry(int32_t* tiles, int max_tiles);   // the node-tile sizes of the launcher (ascending); returns how many there are
int32_t hgconv_f16(const void* x, int ld_x, void* out, int ld_out, int B, int N, int D, int E, float logit_scale, const HgconvWeights& w, void* workspace,
                   size_t workspace_bytes, hipStream_t s);
// grouped convolution on the matrix pipe (conv_grouped.hip): fp16, 2 <= groups <= 8, Cin / groups and Cout / groups multiples of 16 up to 64,
// Cout <= 128, 1x1 pad 0 or 3x3 pad 1, stride 1, no dilation, channel strides multiples of 8.  Weights fp16 [group][Cout_g][Kpad],
// k = tap * Cin_g + c, Kpad = conv_grouped_kpad() = K rounded up to 32 (ConvArgs::Kpad must say so); bias fp32 [Cout]
bool conv_grouped_supported(const ConvArgs& a);
int conv_grouped_kpad(const ConvArgs& a);
int32_t conv_grouped(const ConvArgs& a, hipStream_t s);
// generic transposed convolution, fp32 weights laid out [Cin][kh][kw][Cout/groups]
int32_t deconv_direct(const ConvArgs& a, int dtype, hipStream_t s);

// --- layout / dtype conversion ----------------------------------------------------------------------
// LINEAR fp32 [N][C][H][W] -> NHWC dtype, channels [C, Cpad) zero-filled
int32_t nchw_f32_to_nhwc(const float* in, void* out, int dtype, int N, int C, int H, int W, int Cpad, int ld_out,
                         hipStream_t s);
// NHWC dtype -> LINEAR fp32 [N][C][H][W]
int32_t nhwc_to_nchw_f32(const void* in, int dtype, float* out, int N, int C, int H, int W, int ld_in, hipStream_t s);

// --- NHWC element ops (dtype = DT_F16 / DT_F32), strided channel slices ---------------------------------
// SPPF: three chained k x k stride-1 'same' max-pools (fp16, C % 8 == 0, H*W*32 B <= 60 KB of LDS)
// (f32: fp32 NHWC tensors, 4-channel chunks - the fp32 engines' SPPF)
int32_t nhwc_maxpool_chain3_f16(const void* in, void* o1, void* o2, void* o3, int N, int H, int W, int C, int ld_in, int ld1,
                                int ld2, int ld3, int k, hipStream_t s, int f32 = 0);
// [N,H,W,(r,q,c)] -> [N,H*bh,W*bw,c], fp16, C % 8 == 0
int32_t nhwc_depth_to_space_f16(const void* in, void* out, int N, int H, int W, int C, int bh, int bw, int ld_in, int ld_out,
                                hipStream_t s);
int32_t nhwc_pool(const void* in, void* out, int dtype, int op, int N, int H, int W, int C, int ld_in, int Ho, int Wo,
                  int ld_out, int kh, int kw, int sh, int sw, int ph, int pw, int avg_exclusive, hipStream_t s);
int32_t nhwc_resize_nearest(const void* in, void* out, int dtype, int N, int H, int W, int C, int ld_in, int Ho,
                            int Wo, int ld_out, hipStream_t s);
// IPaddingLayer: the H x W image at (top, left) of a Ho x Wo image of zeros; Ho >= H + top, Wo >= W + left
int32_t nhwc_zero_pad(const void* in, void* out, int dtype, int N, int H, int W, int C, int ld_in, int Ho, int Wo, int ld_out, int top,
                      int left, hipStream_t s);
int32_t nhwc_elementwise(const void* a, const void* b, void* out, int dtype, int op, long pixels, int C, int ld_a,
                         int ld_b, int ld_out, hipStream_t s);
int32_t nhwc_activation(const void* in, void* out, int dtype, int act, float alpha, long pixels, int C, int ld_in,
                        int ld_out, hipStream_t s);
// out = a + gate (.) b, gate = C fp32 values (a one-element gate repeated); fp32 arithmetic, one rounding to `dtype` (DT_F16 / DT_F32)
int32_t nhwc_gated_add(const void* a, const void* b, const float* gate, void* out, int dtype, long pixels, int C, int ld_a, int ld_b, int ld_out,
                       hipStream_t s);
int32_t nhwc_scale(const void* in, void* out, int dtype, const float* scale, const float* shift, long pixels, int C,
                   int ld_in, int ld_out, hipStream_t s);
int32_t nhwc_copy(const void* in, void* out, int dtype, long pixels, int C, int ld_in, int ld_out, hipStream_t s);
// mean over H*W: NHWC [N][H][W][C] -> NHWC [N][1][1][C]
int32_t nhwc_reduce_hw_avg(const void* in, void* out, int dtype, int N, int HW, int C, int ld_in, int ld_out,
                           hipStream_t s);

// --- INT8 support (quant_ops.hip): calibration statistics over NHWC fp16 tensors, int8 resize with requantisation
int32_t nhwc_absmax_f16(const void* x, long pixels, int C, int ld, unsigned* out_float_bits, hipStream_t s);  // atomicMax of the float bits
// hist[bin] += 1 with bin = |x| / range * 8192 (runtime/int8.h kCalibBins; values beyond the range go to the last bin)
int32_t nhwc_hist_f16(const void* x, long pixels, int C, int ld, float range, unsigned long long* hist8192, hipStream_t s);
int32_t nhwc_resize_nearest_i8(const void* in, void* out, int N, int H, int W, int C, int ld_in, int Ho, int Wo, int ld_out, float ratio,
                               hipStream_t s);

// --- LINEAR fp32 ops (rank <= 6, row-major, batch outermost) -----------------------------------------------
struct StridedView {
    int rank;
    long shape[6];
    long stride_in[6];   // element strides into the source (0 = broadcast)
    long stride_in2[6];  // second operand (elementwise only)
};
// out (dense row-major `shape`) = in[gather by stride_in]   (permute / slice / broadcast copy)
int32_t lin_gather(const float* in, float* out, const StridedView& v, hipStream_t s);
// dense source -> strided destination (concat placement): out[stride_in-indexed] = in
int32_t lin_scatter(const float* in, float* out, const StridedView& v, hipStream_t s);
int32_t lin_elementwise(const float* a, const float* b, float* out, int op, const StridedView& v, hipStream_t s);
int32_t lin_activation(const float* in, float* out, int act, float alpha, long n, hipStream_t s);
int32_t lin_softmax(const float* in, float* out, long outer, long axis, long inner, hipStream_t s);
// C[b][m][n] = sum_k A(b,m,k) * B(b,k,n); ta/tb: operand stored transposed; batch stride 0 = broadcast.
// The batch index splits into (b / binner, b % binner), strided by (bsA, bsA2) / (bsB, bsB2): two broadcast patterns
int32_t lin_matmul(const float* A, const float* B, float* C, int batch, int M, int N, int K, int ta, int tb,
                   long bsA, long bsB, hipStream_t s, int binner = 1, long bsA2 = 0, long bsB2 = 0);
int32_t lin_reduce(const float* in, float* out, int op /*0 sum,1 avg,2 max*/, long outer, long axis, long inner,
                   hipStream_t s);
int32_t lin_scale(const float* in, float* out, const float* scale, const float* shift, const float* power, int mode,
                  long outer, long C, long inner, hipStream_t s);

}  // namespace trtx
