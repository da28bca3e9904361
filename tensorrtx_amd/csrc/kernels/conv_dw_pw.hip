// YOLOv13's DSConv (yolov13/src/block.cpp:491-534) in ONE launch for gfx950: a depthwise k x k convolution (k 3 / 5 / 7, pad k/2, stride 1 / 2; no bias, no
// BatchNorm, no activation) and the 1x1 convolution behind it (+ folded BatchNorm, act1, + residual, act2), NHWC fp16 in and out, fp32 accumulation.
//
// Why.  As two launches the depthwise result - as large as the block's input over stride^2 - goes to HBM as fp16 and comes straight back for its one reader;
// conv_dw is HBM-bound and the 1x1 behind it reads nothing else.  Here that tensor lives in LDS only, as the A operand of the 1x1 on the matrix pipe.
//
// Work unit: ONE tile per workgroup (4 waves), TH rows x 16 columns of output pixels of one image - never two images.  Not a persistent grid: stage 1 is
// bound by global loads and stage 2 by the matrix pipe, and two to four workgroups resident on a CU (below) overlap the one's stage 1 with the other's stage
// 2 without a double-buffered A tile, which at the widest Cin would not fit beside the first anyway; the weights are too large for registers (Cout x Cin), so
// a persistent workgroup would have nothing to keep between tiles.
//   TH = 16 (256 pixels) for Cin <= 128 on maps of more than 4 rows: (128 + 8) x 256 x 2 B = 68 KB, two workgroups per CU, and enough stage-1 items for the
//           256 threads at 16 channels (256 pixels / 4 x 2 channel vectors = 128);
//   TH = 4  (64 pixels) otherwise: (Cin' + 8) x 64 x 2 B - 33 KB at Cin 256 (four per CU), 78 KB at Cin 608 (two), 99 KB at Cin 768 (one: there the two stages
//           of a CU no longer overlap), Cin <= 1024.  Cin' = Cin rounded up to the 32-wide k-step.
// Stage 1, depthwise into LDS: a thread owns the 16-byte channel vector of 4 horizontally neighbouring output pixels and walks the input rows once with
//   16-byte global loads, k ((4 - 1) S + k) of them instead of 4 k^2 - conv_dw_kernel's scheme, and its summation: taps row by row, fmaf in fp32 from 0,
//   out-of-image taps skipped, ONE rounding to fp16.  The result is stored as [pixel][Cin' + 8] halfs: the same values the two-launch route's intermediate
//   tensor holds, so the fused route differs from it only in the 1x1's summation order (and in rounding once, not twice, around the residual).  Channels
//   Cin .. Cin' and the pixels of a ragged tile that lie outside the image are stored as zeros.  The pitch of Cin' + 8 halfs is 16 bytes more than a multiple
//   of 64 bytes: the 16 pixels a quarter-wave reads as one k-slice start in different 16-byte bank groups - no conflicts on the fragment reads.
// One __syncthreads.
// Stage 2, the 1x1 on v_mfma_f32_16x16x32_f16: the weights are the A fragments (16 output channels x 32 k, 16 bytes per lane straight from the packed
//   [Cout_pad][Kpad] fp16 array trtx_conv_pack_weights_f16 produces for a 1x1: k = channel, BatchNorm scale folded, zero beyond Cin), the tile row's 16 pixels the
//   B fragments from LDS.  A wave owns 16 / TH neighbouring 16-channel column blocks for all TH tile rows (16 accumulator fragments = 64 VGPRs), the four
//   waves take neighbouring runs, and Cout beyond 4 x 16 / TH blocks is further passes over the same resident tile: stage 1 runs once however wide Cout is.
// Epilogue in registers: a lane holds 4 consecutive channels of one pixel: + bias, act1 (act.h's act_fast), + residual, act2, one rounding, one 8-byte store
//   into out + m ld_out, for pixels inside the image only.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "act.h"
#include "kernels.h"
#include "launch.h"

namespace trtx {
namespace {

constexpr int kThreads = 256;
constexpr int kTW = 16;       // tile columns: the 16 pixel columns of one MFMA
constexpr int kOW = 4;        // output pixels per thread in stage 1 (conv_dw's)
constexpr int kPitchPad = 8;  // halfs added to Cin' per pixel of the A tile
constexpr int kMaxCin = 1024;
constexpr int kWideTileCin = 128;   // up to here (and on maps of more than 4 rows) the 16-row tile

__host__ __device__ inline int kstep_pad(int cin) { return (cin + 31) / 32 * 32; }

template <int K, int S, int TH>
__global__ __launch_bounds__(kThreads) void conv_dw_pw_kernel(const ConvArgs dw, const ConvArgs pw, int tiles_x, int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) char s_lds[];
    _Float16* const s_a = reinterpret_cast<_Float16*>(s_lds);
    constexpr int NB = 16 / TH;              // column blocks per wave and pass
    constexpr int NW = (kOW - 1) * S + K;    // input columns a thread's outputs read per filter row
    const int tid = threadIdx.x;
    const int C = dw.Cin, KP = kstep_pad(C), pitch = KP + kPitchPad;
    int b = blockIdx.x;
    const int x0 = (b % tiles_x) * kTW;
    b /= tiles_x;
    const int y0 = (b % tiles_y) * TH;
    const long n = b / tiles_y;

    // ---- stage 1: the depthwise convolution of the tile, rounded to fp16, into LDS as [pixel][KP + 8]
    {
        const _Float16* __restrict__ in = static_cast<const _Float16*>(dw.in);
        const float* __restrict__ w = static_cast<const float*>(dw.wgt);
        const int CVP = KP / 8;
        const int items = TH * (kTW / kOW) * CVP;
        for (int i = tid; i < items; i += kThreads) {
            const int cv = i % CVP;
            const int t = i / CVP;
            const int r = t / (kTW / kOW), s = t % (kTW / kOW);
            const int c0 = cv * 8;
            const int ho = y0 + r, wo0 = x0 + s * kOW;
            half8 hv[kOW];
#pragma unroll
            for (int o = 0; o < kOW; ++o) hv[o] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (c0 < C && ho < dw.Ho && wo0 < dw.Wo) {
                const int wi0 = wo0 * S - dw.pad_w;
                float acc[kOW][8];
#pragma unroll
                for (int o = 0; o < kOW; ++o)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[o][e] = 0.f;
#pragma unroll
                for (int fr = 0; fr < K; ++fr) {
                    const int hi = ho * S - dw.pad_h + fr;
                    if ((unsigned)hi >= (unsigned)dw.H) continue;
                    float wr[K][8];
#pragma unroll
                    for (int q = 0; q < K; ++q) {
                        const float4 lo = *reinterpret_cast<const float4*>(w + (size_t)(fr * K + q) * C + c0);
                        const float4 hi4 = *reinterpret_cast<const float4*>(w + (size_t)(fr * K + q) * C + c0 + 4);
                        wr[q][0] = lo.x; wr[q][1] = lo.y; wr[q][2] = lo.z; wr[q][3] = lo.w;
                        wr[q][4] = hi4.x; wr[q][5] = hi4.y; wr[q][6] = hi4.z; wr[q][7] = hi4.w;
                    }
                    const _Float16* row = in + ((n * dw.H + hi) * dw.W) * (long)dw.ld_in + c0;
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        const int wi = wi0 + j;
                        if ((unsigned)wi >= (unsigned)dw.W) continue;
                        const half8 xv = *reinterpret_cast<const half8*>(row + (long)wi * dw.ld_in);
#pragma unroll
                        for (int o = 0; o < kOW; ++o) {
                            const int q = j - o * S;   // compile-time after unrolling
                            if (q < 0 || q >= K) continue;
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[o][e] = fmaf((float)xv[e], wr[q][e], acc[o][e]);
                        }
                    }
                }
#pragma unroll
                for (int o = 0; o < kOW; ++o)
                    if (wo0 + o < dw.Wo) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) hv[o][e] = round_to_half(acc[o][e]);
                    }
            }
            _Float16* dst = s_a + (r * kTW + s * kOW) * pitch + c0;
#pragma unroll
            for (int o = 0; o < kOW; ++o) *reinterpret_cast<half8*>(dst + o * pitch) = hv[o];
        }
    }
    __syncthreads();   // the A tile is complete

    // ---- stage 2: out[pixel][channel] = sum_k A[pixel][k] W[channel][k]; weights as the MFMA's A operand, pixels as its B operand
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 4, col = lane & 15;
    const _Float16* __restrict__ wgt = static_cast<const _Float16*>(pw.wgt);
    const _Float16* __restrict__ res = static_cast<const _Float16*>(pw.residual);
    _Float16* __restrict__ out = static_cast<_Float16*>(pw.out);
    const int nblk = (pw.Cout + 15) / 16;
    const int ksteps = KP / 32;
    const _Float16* const a_lane = s_a + col * pitch + grp * 8;
    // (Below four runs of column blocks some waves have nothing to multiply.  Splitting the tile's rows among them instead was tried and measured slower - 16 ch at
    // 160 x 160 0.292 ms per plan against 0.259, 64 ch at 80 x 80 0.231 against 0.223: 236 VGPRs instead of 154 - where stage 2 is a few MFMAs behind a load-bound stage 1.)
    for (int cb0 = wave * NB; cb0 < nblk; cb0 += 4 * NB) {   // one pass; wave-uniform
        floatx4 acc[TH][NB];
#pragma unroll
        for (int rf = 0; rf < TH; ++rf)
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[rf][j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma nounroll
        for (int kt = 0; kt < ksteps; ++kt) {
            half8 wf[NB], xf[TH];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                wf[j] = half8{0, 0, 0, 0, 0, 0, 0, 0};
                if (cb0 + j < nblk) wf[j] = *reinterpret_cast<const half8*>(wgt + (size_t)((cb0 + j) * 16 + col) * pw.Kpad + kt * 32 + grp * 8);
            }
#pragma unroll
            for (int rf = 0; rf < TH; ++rf) xf[rf] = *reinterpret_cast<const half8*>(a_lane + rf * kTW * pitch + kt * 32);
#pragma unroll
            for (int rf = 0; rf < TH; ++rf)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[rf][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[rf], acc[rf][j], 0, 0, 0);
        }
        // ---- epilogue: this lane's accumulator rows are channels 16 cb + 4 grp + [0, 4) of pixel (y0 + rf, x0 + col)
        const int wo = x0 + col;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int c = (cb0 + j) * 16 + grp * 4;
            if (c >= pw.Cout || wo >= pw.Wo) continue;   // (Cout % 8 == 0: all four channels or none)
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pw.bias) bv = *reinterpret_cast<const float4*>(pw.bias + c);
#pragma unroll
            for (int rf = 0; rf < TH; ++rf) {
                const int ho = y0 + rf;
                if (ho >= pw.Ho) continue;
                const size_t m = ((size_t)n * pw.Ho + ho) * pw.Wo + wo;
                float v[4] = {acc[rf][j][0] + bv.x, acc[rf][j][1] + bv.y, acc[rf][j][2] + bv.z, acc[rf][j][3] + bv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = act_fast(v[e], pw.act1, pw.alpha1);
                if (res) {
                    const half4 rv = *reinterpret_cast<const half4*>(res + m * pw.ld_res + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
                }
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = round_to_half(act_fast(v[e], pw.act2, pw.alpha2));
                *reinterpret_cast<half4*>(out + m * pw.ld_out + c) = o;
            }
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool epilogue_act(int a) { return a == ACT_NONE || a == ACT_RELU || a == ACT_SILU; }

// The output may not lie on the input: a workgroup stores its tile while others still read those pixels as halo (two launches may run in place, this one
// may not).  Where both pointers are set: the two byte ranges are apart, or they are different channel slices of one buffer (the same map, the same
// channel stride, the pointers less than one pixel apart)
bool output_on_input(const ConvArgs& dw, const ConvArgs& pw) {
    if (!dw.in || !pw.out) return false;
    const intptr_t pin = reinterpret_cast<intptr_t>(dw.in), pout = reinterpret_cast<intptr_t>(pw.out);
    const intptr_t in_bytes = (((intptr_t)dw.N * dw.H * dw.W - 1) * dw.ld_in + dw.Cin) * 2;
    const intptr_t out_bytes = (((intptr_t)pw.N * pw.Ho * pw.Wo - 1) * pw.ld_out + pw.Cout) * 2;
    if (pin + in_bytes <= pout || pout + out_bytes <= pin) return false;
    const intptr_t ld = (intptr_t)dw.ld_in * 2;
    const bool same_map = dw.H == pw.Ho && dw.W == pw.Wo && dw.ld_in == pw.ld_out;
    const bool out_behind = pout >= pin + (intptr_t)dw.Cin * 2 && pout - pin + (intptr_t)pw.Cout * 2 <= ld;
    const bool out_before = pin >= pout + (intptr_t)pw.Cout * 2 && pin - pout + (intptr_t)dw.Cin * 2 <= ld;
    return !(same_map && (out_behind || out_before));
}

template <int K, int S>
int32_t launch_ks(const ConvArgs& dw, const ConvArgs& pw, hipStream_t s) {
    const bool wide = dw.Cin <= kWideTileCin && pw.Ho > 4;
    const int th = wide ? 16 : 4;
    const int tiles_x = (pw.Wo + kTW - 1) / kTW, tiles_y = (pw.Ho + th - 1) / th;
    const long total = (long)pw.N * tiles_x * tiles_y;
    if (total > 0x7fffffffL) return TRTX_ERR_UNSUPPORTED;
    const size_t lds = (size_t)th * kTW * (kstep_pad(dw.Cin) + kPitchPad) * 2;
    const void* kern = wide ? reinterpret_cast<const void*>(&conv_dw_pw_kernel<K, S, 16>) : reinterpret_cast<const void*>(&conv_dw_pw_kernel<K, S, 4>);
    static bool asked[2][64] = {};   // per instantiation and device: more than 64 KB of dynamic LDS has to be asked for
    int dev = 0;
    TRTX_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return TRTX_ERR_HIP;
    if (!asked[wide][dev]) {
        TRTX_HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * (kMaxCin + kPitchPad) * 2));
        asked[wide][dev] = true;
    }
    if (wide)
        TRTX_LAUNCH((conv_dw_pw_kernel<K, S, 16>), dim3((unsigned)total), dim3(kThreads), lds, s, dw, pw, tiles_x, tiles_y);
    else
        TRTX_LAUNCH((conv_dw_pw_kernel<K, S, 4>), dim3((unsigned)total), dim3(kThreads), lds, s, dw, pw, tiles_x, tiles_y);
    return check_launch("conv_dw_pw_f16");
}

}  // namespace

// plan time: pointers may be null (geometry only); launch time: the alignment of whatever pointers are set counts too
bool conv_dw_pw_supported(const ConvArgs& dw, const ConvArgs& pw) {
    const int C = dw.Cin;
    const bool dw_ok = conv_dw_supported(dw) && !dw.f32 && !dw.bias && dw.act1 == ACT_NONE && dw.act2 == ACT_NONE && !dw.residual && C >= 8 && C % 8 == 0 &&
                       C <= kMaxCin && dw.N >= 1 && dw.H >= 1 && dw.W >= 1 && dw.ld_in % 8 == 0 && dw.ld_in >= C && aligned16(dw.in) && aligned16(dw.wgt);
    const bool pw_ok = !pw.f32 && !pw.in_i8 && !pw.out_i8 && !pw.res_i8 && !pw.up_C && pw.kh == 1 && pw.kw == 1 && pw.stride_h == 1 && pw.stride_w == 1 &&
                       pw.pad_h == 0 && pw.pad_w == 0 && pw.dil_h == 1 && pw.dil_w == 1 && pw.groups == 1 && pw.Cout >= 8 && pw.Cout % 8 == 0 &&
                       pw.ld_out % 8 == 0 && pw.ld_out >= pw.Cout && (!pw.residual || (pw.ld_res % 8 == 0 && pw.ld_res >= pw.Cout)) && epilogue_act(pw.act1) &&
                       epilogue_act(pw.act2) && pw.Kpad % 8 == 0 && pw.Kpad >= kstep_pad(C) && pw.Cout_pad >= (pw.Cout + 15) / 16 * 16 && aligned16(pw.wgt) &&
                       aligned16(pw.bias) && aligned16(pw.out) && aligned16(pw.residual);
    const bool chained = pw.Cin == C && pw.N == dw.N && pw.H == dw.Ho && pw.W == dw.Wo && pw.Ho == pw.H && pw.Wo == pw.W;
    return dw_ok && pw_ok && chained;
}

// Where the lowering fuses (match_dsconv).  Every workgroup streams the whole Cout x Cin weight matrix from L2 for its 64 .. 256 pixels, so the 1x1 half falls
// behind the implicit-GEMM kernel's 128-row tiles as the matrix grows.  Measured (tools/dsconv_time.py, profiles/dsconv_time.jsonl; fp16, batch 32, 640 x 640, ms
// per plan, one launch | two): 16 -> 16 at 160 x 160 0.259 | 0.263, 64 -> 64 at 80 x 80 0.223 | 0.229, 128 -> 128 / 2 at 80 x 80 0.107 | 0.085, 768 -> 768 / 2 at
// 40 x 40 0.338 | 0.168.  Admitted is what the two winning measurements span, nothing beyond them: Cin and Cout both from 16 to 64.
bool conv_dw_pw_worthwhile(int cin, int cout) { return cin >= 16 && cin <= 64 && cout >= 16 && cout <= 64; }

// dw: the depthwise convolution as conv_dw takes it (dw.out is not written); pw: the 1x1 as conv_igemm_f16 takes it (pw.in is not read)
int32_t conv_dw_pw_f16(const ConvArgs& dw, const ConvArgs& pw, hipStream_t s) {
    if (!conv_dw_pw_supported(dw, pw) || !dw.in || !dw.wgt || !pw.wgt || !pw.out) return TRTX_ERR_UNSUPPORTED;
    if (output_on_input(dw, pw)) return TRTX_ERR_INVALID;
#define DWPW_CASE(K, S) \
    if (dw.kh == K && dw.stride_h == S) return launch_ks<K, S>(dw, pw, s);
    DWPW_CASE(3, 1) DWPW_CASE(3, 2) DWPW_CASE(5, 1) DWPW_CASE(5, 2) DWPW_CASE(7, 1) DWPW_CASE(7, 2)
#undef DWPW_CASE
    return TRTX_ERR_UNSUPPORTED;
}

// The fused launch where it is admitted - supported, worthwhile and not on its own input -, otherwise conv_dw into `mid` (NHWC fp16 [N][Ho][Wo][Cin], dense, written only then) and the 1x1 on the
// implicit-GEMM kernel's default tactic from it: what the executor issues, so that the depthwise half can never be left out
int32_t conv_dw_pw_or_two_f16(const ConvArgs& dw, const ConvArgs& pw, void* mid, hipStream_t s) {
    if (conv_dw_pw_supported(dw, pw) && conv_dw_pw_worthwhile(dw.Cin, pw.Cout) && dw.in && dw.wgt && pw.wgt && pw.out && !output_on_input(dw, pw))
        return conv_dw_pw_f16(dw, pw, s);
    if (!mid || !dw.in || !pw.out) return TRTX_ERR_INVALID;
    ConvArgs a = dw, b = pw;
    a.out = mid;
    a.ld_out = dw.Cout;
    b.in = mid;
    b.ld_in = dw.Cout;
    const int32_t st = conv_dw(a, DT_F16, s);
    return st != TRTX_OK ? st : conv_igemm_f16(b, s);
}

}  // namespace trtx
