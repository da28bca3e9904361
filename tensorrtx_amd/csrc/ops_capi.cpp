// extern "C" entry points that expose single kernels (for parity tests, micro-benchmarks and
// reference-style plugin classes) plus the library-level queries.  See include/trtx_hip.h.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "options.h"
#include "kernels/kernels.h"
#include "runtime/pack.h"

using namespace trtx;

extern "C" const char* trtx_status_string(int32_t s) {
    switch (s) {
        case TRTX_OK: return "ok";
        case TRTX_ERR_INVALID: return "invalid argument";
        case TRTX_ERR_HIP: return "HIP error";
        case TRTX_ERR_WORKSPACE: return "workspace too small";
        case TRTX_ERR_UNSUPPORTED: return "unsupported configuration";
        case TRTX_ERR_NO_DEVICE: return "no HIP device";
        case TRTX_ERR_IO: return "I/O or parse error";
        case TRTX_ERR_STATE: return "invalid call order";
        default: return "unknown status";
    }
}

extern "C" int32_t trtx_abi_version(void) {
    return TRTX_ABI_VERSION;
}

extern "C" int32_t trtx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int32_t trtx_conv_packed_dims(int cout, int cin_pad, int kh, int kw, int32_t* cout_pad, int32_t* kpad,
                                         int32_t* bn) {
    if (cout < 1 || cin_pad < 1 || kh < 1 || kw < 1) return TRTX_ERR_INVALID;
    const int b = conv_igemm_pick_bn(cout);
    if (bn) *bn = b;
    if (cout_pad) *cout_pad = (cout + b - 1) / b * b;
    if (kpad) {
        const int bk = conv_igemm_pick_bk(cin_pad, kh * kw);
        *kpad = (kh * kw * conv_igemm_pick_cink(cin_pad, bk) + bk - 1) / bk * bk;
    }
    return TRTX_OK;
}

extern "C" int32_t trtx_conv_pack_weights_f16(const float* w_kcrs, int cout, int cin, int kh, int kw, int cin_pad,
                                              const float* ch_scale, uint16_t* packed) {
    if (!w_kcrs || !packed || cin_pad < cin) return TRTX_ERR_INVALID;
    const int bk = conv_igemm_pick_bk(cin_pad, kh * kw);
    pack_conv_weights_f16(w_kcrs, cout, cin, kh, kw, conv_igemm_pick_cink(cin_pad, bk), bk, ch_scale, packed);
    return TRTX_OK;
}

// geometry of the launch trtx_op_conv2d_nhwc_f16 performs (pointers left null)
static ConvArgs op_conv_args(int N, int H, int W, int Cin, int ld_in, int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph, int pw,
                             int act1, int has_res, int ld_res, int act2) {
    ConvArgs a{};
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ld_in = ld_in;
    a.Ho = (H + 2 * ph - kh) / sh + 1;
    a.Wo = (W + 2 * pw - kw) / sw + 1;
    a.Cout = Cout;
    a.bn = conv_igemm_pick_bn(Cout);
    a.Cout_pad = (Cout + a.bn - 1) / a.bn * a.bn;
    a.ld_out = ld_out; a.ld_res = ld_res;
    a.kh = kh; a.kw = kw; a.stride_h = sh; a.stride_w = sw; a.pad_h = ph; a.pad_w = pw; a.dil_h = 1; a.dil_w = 1;
    a.groups = 1;
    a.bk = conv_igemm_pick_bk(Cin, kh * kw);
    a.CinK = conv_igemm_pick_cink(Cin, a.bk);
    a.K = kh * kw * a.CinK;
    a.Kpad = (a.K + a.bk - 1) / a.bk * a.bk;
    a.M = N * a.Ho * a.Wo;
    a.act1 = act1; a.act2 = act2; a.alpha1 = 0.1f; a.alpha2 = 0.1f;
    a.scalar_out = (Cout % 8 || ld_out % 8 || (has_res && ld_res % 8)) ? 1 : 0;
    return a;
}

static bool g_force_tactic = false;
static ConvTactic g_forced{};

extern "C" int32_t trtx_op_conv_force_tactic(const int32_t* t) {
    if (t && t[5] != 0) return TRTX_ERR_UNSUPPORTED;   // the sixth word (the row-reuse kernel's, which left the library) is always 0
    g_force_tactic = t != nullptr;
    if (t) g_forced = ConvTactic{t[0], t[1], t[2], t[3], t[4]};
    return TRTX_OK;
}

extern "C" int32_t trtx_op_conv2d_tactics(int N, int H, int W, int Cin, int ld_in, int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph,
                                          int pw, int has_residual, int ld_res, int32_t* out6, int32_t max_out) {
    if (!out6 || max_out < 1 || N < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1) return 0;
    ConvArgs a = op_conv_args(N, H, W, Cin, ld_in, Cout, ld_out, kh, kw, sh, sw, ph, pw, 0, has_residual, ld_res, 0);
    a.residual = has_residual ? reinterpret_cast<const void*>(1) : nullptr;
    std::vector<ConvTactic> t(max_out);
    const int n = conv_tactics(a, t.data(), max_out);
    for (int i = 0; i < n; ++i) {
        out6[6 * i + 0] = t[i].bn; out6[6 * i + 1] = t[i].bk; out6[6 * i + 2] = t[i].bm; out6[6 * i + 3] = t[i].wsk; out6[6 * i + 4] = t[i].ws;
        out6[6 * i + 5] = 0;   // kept by the ABI
    }
    return n;
}

extern "C" int32_t trtx_op_conv2d_nhwc_f16(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked,
                                           const float* bias, void* out, int Cout, int ld_out, int kh, int kw, int sh,
                                           int sw, int ph, int pw, int act1, const void* residual, int ld_res,
                                           int act2, trtx_stream_t stream) {
    ConvArgs a = op_conv_args(N, H, W, Cin, ld_in, Cout, ld_out, kh, kw, sh, sw, ph, pw, act1, residual != nullptr, ld_res, act2);
    a.in = in;
    a.wgt = wpacked;
    a.bias = bias;
    a.out = out;
    a.residual = residual;
    if (reinterpret_cast<uintptr_t>(out) & 15) a.scalar_out = 1;
    if (g_force_tactic) conv_apply_tactic(&a, g_forced);
    // TRTX_OP_REPS=n (timing tools only): n back-to-back launches per call, so that the device — not the Python caller — sets the pace
    const int reps = options().op_reps;
    int32_t st = TRTX_OK;
    for (int r = 0; r < reps && st == TRTX_OK; ++r) st = conv_igemm_f16(a, stream);
    return st;
}

// --- the first layer (kernels/conv_stem.hip) and the stem pair in one launch (kernels/conv_stem_pair.hip), test / tool entry points
static ConvArgs op_stem_args(const float* in, int N, int C, int H, int W, const float* w_taps_cout, const float* bias, int Cout, int k, int stride, int pad, int act) {
    ConvArgs a{};
    a.in = in; a.wgt = w_taps_cout; a.bias = bias;
    a.N = N; a.H = H; a.W = W; a.Cin = C; a.ld_in = C;
    a.Ho = (H + 2 * pad - k) / stride + 1;
    a.Wo = (W + 2 * pad - k) / stride + 1;
    a.Cout = Cout; a.Cout_pad = Cout;
    a.kh = k; a.kw = k; a.stride_h = stride; a.stride_w = stride; a.pad_h = pad; a.pad_w = pad; a.dil_h = 1; a.dil_w = 1;
    a.groups = 1;
    a.K = k * k * C; a.Kpad = a.K;
    a.M = N * a.Ho * a.Wo;
    a.act1 = act; a.alpha1 = 0.1f; a.alpha2 = 0.1f;
    return a;
}

extern "C" int32_t trtx_op_conv_stem_nchw_f16(const float* in, int N, int C, int H, int W, const float* w_taps_cout, const float* bias, void* out, int Cout,
                                              int ld_out, int k, int stride, int pad, int act, trtx_stream_t stream) {
    if (!in || !w_taps_cout || !out || N < 1 || C < 1 || H < 1 || W < 1 || k < 1 || stride < 1 || pad < 0 || H + 2 * pad < k || W + 2 * pad < k) return TRTX_ERR_INVALID;
    ConvArgs a = op_stem_args(in, N, C, H, W, w_taps_cout, bias, Cout, k, stride, pad, act);
    a.out = out;
    a.ld_out = ld_out;
    return conv_stem_nchw_f32(a, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trtx_op_conv_stem_pair_f16(const float* in, int N, int C, int H, int W, const float* stem_w_taps_cout, const float* stem_bias, int stem_act,
                                              const void* conv_wpacked, const float* conv_bias, int conv_act, void* out, int ld_out, trtx_stream_t stream) {
    if (!in || !stem_w_taps_cout || !conv_wpacked || !out || N < 1 || C < 1 || H < 1 || W < 1) return TRTX_ERR_INVALID;
    const ConvArgs s = op_stem_args(in, N, C, H, W, stem_w_taps_cout, stem_bias, 16, 3, 2, 1, stem_act);
    ConvArgs c = op_conv_args(N, s.Ho, s.Wo, 16, 16, 32, ld_out, 3, 3, 2, 2, 1, 1, conv_act, 0, 0, 0);
    c.wgt = conv_wpacked;
    c.bias = conv_bias;
    c.out = out;
    return conv_stem_pair_f16(s, c, static_cast<hipStream_t>(stream));
}

// --- the two 3x3 convolutions of a 16-channel bottleneck in one launch (kernels/conv_bneck_pair.hip), test / tool entry points
static int32_t op_bneck_pair(const void* in, int N, int H, int W, int ld_in, int in_coff, const void* w1_packed, const float* bias1, int act1, const void* w2_packed,
                             const float* bias2, int act2, int shortcut, int act_after, void* mid, void* out, int ld_out, bool or_two, trtx_stream_t stream) {
    if (!in || !w1_packed || !w2_packed || !out || N < 1 || H < 1 || W < 1 || ld_in < 16 || ld_in % 8 || in_coff < 0 || in_coff % 8 || in_coff + 16 > ld_in ||
        ld_out < 16 || ld_out % 8 || (or_two && !mid))
        return TRTX_ERR_INVALID;
    ConvArgs a = op_conv_args(N, H, W, 16, ld_in, 16, 16, 3, 3, 1, 1, 1, 1, act1, 0, 0, 0);
    ConvArgs b = op_conv_args(N, H, W, 16, 16, 16, ld_out, 3, 3, 1, 1, 1, 1, act2, shortcut ? 1 : 0, shortcut ? ld_in : 0, act_after);
    a.in = static_cast<const uint16_t*>(in) + in_coff;
    a.wgt = w1_packed;
    a.bias = bias1;
    a.out = mid;
    b.in = mid;
    b.wgt = w2_packed;
    b.bias = bias2;
    b.out = out;
    b.residual = shortcut ? a.in : nullptr;
    if (or_two) return conv_bneck_pair_or_two_f16(a, b, static_cast<hipStream_t>(stream));
    if (!conv_bneck_pair_possible(a, b)) return TRTX_ERR_INVALID;   // (an output that lies on the input channels among the reasons)
    return conv_bneck_pair_f16(a, b, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trtx_op_conv_bneck_pair_f16(const void* in, int N, int H, int W, int ld_in, int in_coff, const void* w1_packed, const float* bias1, int act1,
                                               const void* w2_packed, const float* bias2, int act2, int shortcut, int act_after, void* out, int ld_out,
                                               trtx_stream_t stream) {
    return op_bneck_pair(in, N, H, W, ld_in, in_coff, w1_packed, bias1, act1, w2_packed, bias2, act2, shortcut, act_after, nullptr, out, ld_out, false, stream);
}

extern "C" int32_t trtx_op_conv_bneck_pair_or_two_f16(const void* in, int N, int H, int W, int ld_in, int in_coff, const void* w1_packed, const float* bias1, int act1,
                                                      const void* w2_packed, const float* bias2, int act2, int shortcut, int act_after, void* mid, void* out,
                                                      int ld_out, trtx_stream_t stream) {
    return op_bneck_pair(in, N, H, W, ld_in, in_coff, w1_packed, bias1, act1, w2_packed, bias2, act2, shortcut, act_after, mid, out, ld_out, true, stream);
}

// --- two sibling groups over the same inputs in one launch (the dual tile of kernels/igemm_tile.h), test / tool entry points
static int32_t op_dual_group(int n, const void* const* in, const int32_t* geom, int k, int stride, int pad, const void* const* w0, const float* const* bias0,
                             void* const* out0, const int32_t* side0, const void* const* w1, const float* const* bias1, void* const* out1, const int32_t* side1,
                             const void* const* res1, int ld_res1, int i8_1, bool or_two, trtx_stream_t stream) {
    if (n < 1 || n > kMaxDualGroup || !in || !geom || !w0 || !out0 || !side0 || !w1 || !out1 || !side1 || k < 1 || stride < 1 || pad < 0) return TRTX_ERR_INVALID;
    ConvArgs a0[kMaxDualGroup], a1[kMaxDualGroup];
    for (int j = 0; j < n; ++j) {
        const int32_t *g = geom + 5 * j, *s0 = side0 + 3 * j, *s1 = side1 + 3 * j;
        if (!in[j] || !w0[j] || !out0[j] || !w1[j] || !out1[j] || g[0] < 1 || g[1] + 2 * pad < k || g[2] + 2 * pad < k || g[3] < 1) return TRTX_ERR_INVALID;
        const void* r1 = res1 ? res1[j] : nullptr;
        a0[j] = op_conv_args(g[0], g[1], g[2], g[3], g[4], s0[0], s0[1], k, k, stride, stride, pad, pad, s0[2], 0, 0, 0);
        a1[j] = op_conv_args(g[0], g[1], g[2], g[3], g[4], s1[0], s1[1], k, k, stride, stride, pad, pad, s1[2], r1 != nullptr, ld_res1, 0);
        a0[j].in = a1[j].in = in[j];
        a0[j].wgt = w0[j]; a0[j].bias = bias0 ? bias0[j] : nullptr; a0[j].out = out0[j];
        a1[j].wgt = w1[j]; a1[j].bias = bias1 ? bias1[j] : nullptr; a1[j].out = out1[j];
        a1[j].residual = r1;
        a1[j].in_i8 = i8_1 ? 1 : 0;
        a0[j].t_wsk = a1[j].t_wsk = WSK_OFF;   // as the members of a grouped launch: the main kernel's K order
        a0[j].t_ws = a1[j].t_ws = WS_OFF;
        a0[j].k_pinned = a1[j].k_pinned = 1;
    }
    return or_two ? conv_dual_group_or_two_f16(a0, a1, n, static_cast<hipStream_t>(stream)) : conv_dual_group_f16(a0, a1, n, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trtx_op_conv_dual_group_f16(int n, const void* const* in, const int32_t* geom, int k, int stride, int pad, const void* const* w0,
                                               const float* const* bias0, void* const* out0, const int32_t* side0, const void* const* w1, const float* const* bias1,
                                               void* const* out1, const int32_t* side1, const void* const* res1, int ld_res1, int i8_1, trtx_stream_t stream) {
    return op_dual_group(n, in, geom, k, stride, pad, w0, bias0, out0, side0, w1, bias1, out1, side1, res1, ld_res1, i8_1, false, stream);
}

extern "C" int32_t trtx_op_conv_dual_group_or_two_f16(int n, const void* const* in, const int32_t* geom, int k, int stride, int pad, const void* const* w0,
                                                      const float* const* bias0, void* const* out0, const int32_t* side0, const void* const* w1,
                                                      const float* const* bias1, void* const* out1, const int32_t* side1, const void* const* res1, int ld_res1, int i8_1,
                                                      trtx_stream_t stream) {
    return op_dual_group(n, in, geom, k, stride, pad, w0, bias0, out0, side0, w1, bias1, out1, side1, res1, ld_res1, i8_1, true, stream);
}

// --- grouped convolution on the matrix pipe (kernels/conv_grouped.hip), test / tool entry points
extern "C" int32_t trtx_conv_pack_weights_grouped_f16(const float* w_kcrs, int cout, int cin_g, int kh, int kw, const float* ch_scale, uint16_t* packed,
                                                      int32_t* kpad_out) {
    if (!w_kcrs || cout < 1 || cin_g < 1 || kh < 1 || kw < 1) return TRTX_ERR_INVALID;
    const int kpad = (kh * kw * cin_g + 31) / 32 * 32;
    if (kpad_out) *kpad_out = kpad;
    if (packed) pack_conv_weights_grouped_f16(w_kcrs, cout, cin_g, kh, kw, kpad, ch_scale, packed);
    return TRTX_OK;
}

extern "C" int32_t trtx_op_conv2d_grouped_nhwc_f16(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked, const float* bias, void* out,
                                                   int Cout, int ld_out, int groups, int k, int pad, int act1, const void* residual, int ld_res, int act2,
                                                   trtx_stream_t stream) {
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || groups < 1 || k < 1 || pad < 0 || H + 2 * pad < k || W + 2 * pad < k) return TRTX_ERR_INVALID;
    ConvArgs a{};
    a.in = in; a.wgt = wpacked; a.bias = bias; a.out = out; a.residual = residual;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ld_in = ld_in;
    a.Ho = H + 2 * pad - k + 1;
    a.Wo = W + 2 * pad - k + 1;
    a.Cout = Cout; a.Cout_pad = Cout; a.ld_out = ld_out; a.ld_res = ld_res;
    a.kh = k; a.kw = k; a.stride_h = 1; a.stride_w = 1; a.pad_h = pad; a.pad_w = pad; a.dil_h = 1; a.dil_w = 1;
    a.groups = groups;
    a.K = k * k * (Cin / groups);
    a.Kpad = conv_grouped_kpad(a);
    a.M = N * a.Ho * a.Wo;
    a.act1 = act1; a.act2 = act2; a.alpha1 = 0.1f; a.alpha2 = 0.1f;
    const int reps = options().op_reps;   // timing tools only
    int32_t st = TRTX_OK;
    for (int r = 0; r < reps && st == TRTX_OK; ++r) st = conv_grouped(a, static_cast<hipStream_t>(stream));
    return st;
}

// --- depthwise convolution (kernels/conv_dw.hip) and the two attention kernels (kernels/attention.hip, kernels/attention_mfma.hip), test / tool entry points
extern "C" int32_t trtx_op_conv2d_dw_nhwc(const void* in, int dtype, int N, int H, int W, int C, int ld_in, const float* w_taps_c, const float* bias, void* out,
                                          int ld_out, const void* residual, int ld_res, int k, int stride, int pad, int dilation, int act1, float alpha1,
                                          int act2, float alpha2, trtx_stream_t stream) {
    if (!in || !w_taps_c || !out || N < 1 || H < 1 || W < 1 || C < 1 || k < 1 || stride < 1 || pad < 0 || dilation < 1) return TRTX_ERR_INVALID;
    if (dtype != DT_F16 && dtype != DT_F32) return TRTX_ERR_UNSUPPORTED;
    if (H + 2 * pad < dilation * (k - 1) + 1 || W + 2 * pad < dilation * (k - 1) + 1) return TRTX_ERR_INVALID;
    ConvArgs a{};
    a.in = in; a.wgt = w_taps_c; a.bias = bias; a.out = out; a.residual = residual;
    a.N = N; a.H = H; a.W = W; a.Cin = C; a.ld_in = ld_in;
    a.Ho = (H + 2 * pad - dilation * (k - 1) - 1) / stride + 1;
    a.Wo = (W + 2 * pad - dilation * (k - 1) - 1) / stride + 1;
    a.Cout = C; a.Cout_pad = C; a.ld_out = ld_out; a.ld_res = ld_res;
    a.kh = k; a.kw = k; a.stride_h = stride; a.stride_w = stride; a.pad_h = pad; a.pad_w = pad; a.dil_h = dilation; a.dil_w = dilation;
    a.groups = C;
    a.K = k * k;
    a.Kpad = a.K;
    a.M = N * a.Ho * a.Wo;
    a.act1 = act1; a.act2 = act2; a.alpha1 = alpha1; a.alpha2 = alpha2;
    a.f32 = dtype == DT_F32;
    return conv_dw(a, dtype, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trtx_op_psa_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int kd, int hd,
                                             float scale, trtx_stream_t stream) {
    if (!qkv || !out || !vimg) return TRTX_ERR_INVALID;
    return psa_attention_f16(qkv, ld_qkv, out, ld_out, vimg, ld_v, B, heads, N, kd, hd, scale, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trtx_op_area_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int area,
                                              int kd, int hd, float scale, trtx_stream_t stream) {
    if (!qkv || !out || !vimg) return TRTX_ERR_INVALID;
    return area_attention_f16(qkv, ld_qkv, out, ld_out, vimg, ld_v, B, heads, N, area, kd, hd, scale, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trtx_op_area_attention_split_f16(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, void* out, int ld_out, int B,
                                                    int heads, int N, int area, int kd, int hd, float scale, trtx_stream_t stream) {
    if (!q || !k || !v || !out) return TRTX_ERR_INVALID;
    return area_attention_split_f16(q, ld_q, k, ld_k, v, ld_v, out, ld_out, B, heads, N, area, kd, hd, scale, static_cast<hipStream_t>(stream));
}

// --- YOLOv13's hypergraph convolution (kernels/hgconv.hip), test / tool entry points
extern "C" size_t trtx_op_hgconv_workspace_bytes(int B, int N, int D, int E) { return hgconv_workspace_bytes(B, N, D, E); }

extern "C" int32_t trtx_op_hgconv_geometry(int32_t* tiles, int max_tiles, int32_t* n_tiles) {
    if (!tiles || !n_tiles || max_tiles < 1) return TRTX_ERR_INVALID;
    *n_tiles = hgconv_geometry(tiles, max_tiles);
    return TRTX_OK;
}

extern "C" int32_t trtx_op_hgconv_f16(const void* x, int ld_x, void* out, int ld_out, int B, int N, int D, int E, float logit_scale, const float* w_ctx,
                                      const float* b_ctx, const float* proto, const float* w_pre, const float* b_pre, const float* w_edge, const float* b_edge,
                                      const float* w_node, const float* b_node, void* workspace, size_t workspace_bytes, trtx_stream_t stream) {
    if (!x || !out || !w_ctx || !b_ctx || !proto || !w_pre || !b_pre || !w_edge || !b_edge || !w_node || !b_node || !workspace) return TRTX_ERR_INVALID;
    const HgconvWeights w{w_ctx, b_ctx, proto, w_pre, b_pre, w_edge, b_edge, w_node, b_node};
    return hgconv_f16(x, ld_x, out, ld_out, B, N, D, E, logit_scale, w, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

// --- fp32 engines: the implicit-GEMM convolution on the fp32 MFMA (kernels/conv_igemm_f32.hip), test / tool entry points
static ConvArgs op_conv_args_f32(int N, int H, int W, int Cin, int ld_in, int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph, int pw,
                                 int act1, int has_res, int ld_res, int act2) {
    ConvArgs a{};
    a.f32 = 1;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ld_in = ld_in;
    a.Ho = (H + 2 * ph - kh) / sh + 1;
    a.Wo = (W + 2 * pw - kw) / sw + 1;
    a.Cout = Cout;
    a.Cout_pad = (Cout + 15) / 16 * 16;
    a.ld_out = ld_out; a.ld_res = ld_res;
    a.kh = kh; a.kw = kw; a.stride_h = sh; a.stride_w = sw; a.pad_h = ph; a.pad_w = pw; a.dil_h = 1; a.dil_w = 1;
    a.groups = 1;
    a.bk = 16;
    a.CinK = conv_igemm_f32_pick_cink(Cin);
    a.K = kh * kw * a.CinK;
    a.Kpad = (a.K + 15) / 16 * 16;
    a.M = N * a.Ho * a.Wo;
    a.act1 = act1; a.act2 = act2; a.alpha1 = 0.1f; a.alpha2 = 0.1f;
    a.scalar_out = (Cout % 4 || ld_out % 4 || (has_res && ld_res % 4)) ? 1 : 0;
    return a;
}

extern "C" int32_t trtx_conv_packed_dims_f32(int cout, int cin_pad, int kh, int kw, int32_t* cout_pad, int32_t* kpad, int32_t* cink) {
    if (cout < 1 || cin_pad < 1 || kh < 1 || kw < 1) return TRTX_ERR_INVALID;
    const int ck = conv_igemm_f32_pick_cink(cin_pad);
    if (cout_pad) *cout_pad = (cout + 15) / 16 * 16;
    if (kpad) *kpad = (kh * kw * ck + 15) / 16 * 16;
    if (cink) *cink = ck;
    return TRTX_OK;
}

extern "C" int32_t trtx_conv_pack_weights_f32(const float* w_kcrs, int cout, int cin, int kh, int kw, int cin_pad, const float* ch_scale, float* packed) {
    if (!w_kcrs || !packed || cin_pad < cin) return TRTX_ERR_INVALID;
    const int ck = conv_igemm_f32_pick_cink(cin_pad);
    conv_pack_weights_igemm_f32(w_kcrs, cout, cin, kh, kw, ck, (kh * kw * ck + 15) / 16 * 16, (cout + 15) / 16 * 16, ch_scale, packed);
    return TRTX_OK;
}

extern "C" int32_t trtx_op_conv2d_tactics_f32(int N, int H, int W, int Cin, int ld_in, int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph,
                                              int pw, int has_residual, int ld_res, int32_t* out2, int32_t max_out) {   // (4 ints per entry)
    if (!out2 || max_out < 1 || N < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1) return 0;
    ConvArgs a = op_conv_args_f32(N, H, W, Cin, ld_in, Cout, ld_out, kh, kw, sh, sw, ph, pw, 0, has_residual, ld_res, 0);
    a.residual = has_residual ? reinterpret_cast<const void*>(1) : nullptr;
    std::vector<ConvTactic> t(max_out);
    const int n = conv_tactics_f32(a, t.data(), max_out);
    for (int i = 0; i < n; ++i) {
        out2[4 * i + 0] = t[i].bn;
        out2[4 * i + 1] = t[i].bm;
        out2[4 * i + 2] = t[i].ws;
        out2[4 * i + 3] = t[i].bk;
    }
    return n;
}

extern "C" int32_t trtx_op_conv2d_nhwc_f32(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked, const float* bias, void* out,
                                           int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph, int pw, int act1, const void* residual,
                                           int ld_res, int act2, const int32_t* tile2, trtx_stream_t stream) {
    ConvArgs a = op_conv_args_f32(N, H, W, Cin, ld_in, Cout, ld_out, kh, kw, sh, sw, ph, pw, act1, residual != nullptr, ld_res, act2);
    a.in = in;
    a.wgt = wpacked;
    a.bias = bias;
    a.out = out;
    a.residual = residual;
    if ((reinterpret_cast<uintptr_t>(out) & 15) || (residual && (reinterpret_cast<uintptr_t>(residual) & 15))) a.scalar_out = 1;
    if (tile2) {
        a.bn = tile2[0];
        a.bm = tile2[1];
        a.t_ws = tile2[2];
        a.bk = tile2[3];
    }
    const int reps = options().op_reps;   // timing tools only
    int32_t st = TRTX_OK;
    for (int r = 0; r < reps && st == TRTX_OK; ++r) st = conv_igemm_f32(a, stream);
    return st;
}

// --- kINT8 conv, test / tool entry points.  Packed dims: cink = Cin rounded up to 64 channels, kpad = kh*kw*cink (bytes per row).
extern "C" int32_t trtx_conv_pack_weights_i8(const float* w_kcrs, int cout, int cin, int kh, int kw, const float* ch_scale, int8_t* packed,
                                             float* wscale_out, int32_t* cout_pad_out, int32_t* kpad_out) {
    if (!w_kcrs || cout < 1 || cin < 1) return TRTX_ERR_INVALID;
    const int bn = conv_igemm_pick_bn(cout);
    const int cout_pad = (cout + bn - 1) / bn * bn, cink = (cin + 63) / 64 * 64, kpad = kh * kw * cink;
    if (cout_pad_out) *cout_pad_out = cout_pad;
    if (kpad_out) *kpad_out = kpad;
    if (packed && wscale_out) conv_pack_weights_i8(w_kcrs, cout, cin, kh, kw, cink, ch_scale, cout_pad, kpad, packed, wscale_out);
    return TRTX_OK;
}

// in: int8 NHWC [N,H,W,ld_in]; out: int8 (out_inv_scale > 0) or fp16 NHWC; cscale[Cout_pad] = input scale * weight scale
extern "C" int32_t trtx_op_conv2d_nhwc_i8(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked, const float* cscale,
                                          const float* bias, void* out, int out_is_i8, float out_inv_scale, int Cout, int ld_out, int kh,
                                          int kw, int sh, int sw, int ph, int pw, int act1, const void* residual, int res_is_i8,
                                          float res_scale, int ld_res, int act2, trtx_stream_t stream) {
    if (Cin % 16 || ld_in % 16) return TRTX_ERR_INVALID;
    ConvArgs a{};
    a.in = in; a.wgt = wpacked; a.bias = bias; a.out = out; a.residual = residual;
    a.N = N; a.H = H; a.W = W;
    a.Ho = (H + 2 * ph - kh) / sh + 1;
    a.Wo = (W + 2 * pw - kw) / sw + 1;
    a.Cout = Cout;
    a.bn = conv_igemm_pick_bn(Cout);
    a.Cout_pad = (Cout + a.bn - 1) / a.bn * a.bn;
    a.ld_out = ld_out; a.ld_res = ld_res;
    a.kh = kh; a.kw = kw; a.stride_h = sh; a.stride_w = sw; a.pad_h = ph; a.pad_w = pw; a.dil_h = 1; a.dil_w = 1; a.groups = 1;
    a.bk = 32;
    const int cink = (Cin + 63) / 64 * 64;
    a.in_i8 = 1; a.out_i8 = out_is_i8; a.res_i8 = res_is_i8;
    a.cscale = cscale; a.out_inv_scale = out_inv_scale; a.res_scale = res_scale;
    // input-side geometry in 2-byte units (pairs of int8 channels)
    a.Cin = Cin / 2; a.ld_in = ld_in / 2; a.CinK = cink / 2;
    a.K = kh * kw * a.CinK;
    a.Kpad = a.K;
    a.M = N * a.Ho * a.Wo;
    a.act1 = act1; a.act2 = act2; a.alpha1 = 0.1f; a.alpha2 = 0.1f;
    a.scalar_out = 0;
    if (Cout % 8 || ld_out % 8 || (residual && ld_res % 8)) return TRTX_ERR_UNSUPPORTED;
    return conv_igemm_f16(a, stream);
}

extern "C" int32_t trtx_op_nchw_f32_to_nhwc_f16(const float* in, void* out, int N, int C, int H, int W, int Cpad,
                                                int ld_out, trtx_stream_t stream) {
    return nchw_f32_to_nhwc(in, out, DT_F16, N, C, H, W, Cpad, ld_out, stream);
}

extern "C" int32_t trtx_op_nhwc_f16_to_nchw_f32(const void* in, float* out, int N, int C, int H, int W, int ld_in,
                                                trtx_stream_t stream) {
    return nhwc_to_nchw_f32(in, DT_F16, out, N, C, H, W, ld_in, stream);
}

// test support: fill the LDS of every CU with fp16 NaN patterns (LDS survives kernel boundaries; tests/test_gpu_multi_context.py)
extern "C" int32_t trtx_op_poison_lds(void* device_word, trtx_stream_t stream) {
    if (!device_word) return TRTX_ERR_INVALID;
    return poison_lds(static_cast<unsigned*>(device_word), static_cast<hipStream_t>(stream));
}


extern "C" int32_t trtx_repvggdw_fold_weights(const float* w7, const float* scale7, const float* shift7, const float* w3, const float* scale3,
                                              const float* shift3, int channels, float* w_out, float* shift_out) {
    if (!w7 || !scale7 || !shift7 || !w3 || !scale3 || !shift3 || !w_out || !shift_out || channels < 1) return TRTX_ERR_INVALID;
    const std::vector<float> zero(channels, 0.f);   // the reference's depthwise convolutions carry no bias of their own
    repvggdw_fold_weights(w7, scale7, shift7, zero.data(), w3, scale3, shift3, zero.data(), channels, w_out, shift_out);
    return TRTX_OK;
}

extern "C" int32_t trtx_reorg_fold_weights(const float* w_kcrs, int cout, int cin, int kh, int kw, float* folded) {
    if (!w_kcrs || !folded || cout < 1 || cin < 1 || kh < 1 || kw < 1) return TRTX_ERR_INVALID;
    reorg_fold_weights(w_kcrs, cout, cin, kh, kw, folded);
    return TRTX_OK;
}
