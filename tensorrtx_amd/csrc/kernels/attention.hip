// Fused PSA attention of YOLO11's C2PSA (yolo11/src/block.cpp:287-339) and YOLOv10's PSA (yolov10/src/block.cpp:297-386): per image b and
// head h, with q, k (kd = 32 channels; 36 in yolov10m) and v (hd = 64 channels; 72 in yolov10m) read straight from the NHWC fp16 qkv tensor (head h's channels start at h * (2 kd + hd): q, then k, then v),
//     O[b, n, h*hd + d] = sum_m v[d, m] * softmax_m(scale * sum_j q[j, n] k[j, m])
// written NHWC fp16 with the consumer's channel stride, plus the gathered V image Vimg[b, n, h*hd + d] = v[d, n] that the positional
// conv `pe` reads (its epilogue adds O as the residual).  Replaces the qkv view -> slices -> transpose -> matmul -> scale -> softmax ->
// transpose -> matmul -> reshape chain (fp32 NCHW, two layout passes) of the generic lowering.
//
// One lane per query pixel, a workgroup per 64 queries of one (b, h); key / value tiles of 64 pixels staged in LDS (fp32).  Softmax is
// online over the key tiles in fp32 (running max and sum, the scale applied to the score before the max), P and O stay fp32; only the
// store rounds.  Keys beyond N are never read (the tile loop stops at N); queries beyond N are neither computed into nor stored.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../common.h"
#include "kernels.h"

namespace trtx {
namespace {

constexpr int QB = 64, KB = 64;

// KD / HD = key / value channels per head: 32 / 64 (YOLO11's C2PSA and YOLOv10's PSA with 64-channel heads) or 36 / 72 (yolov10m: its
// 288-channel PSA half has 288 / 64 = 4 heads of 72, yolov10/src/block.cpp:297-303, 360-371)
template <int KD, int HD>
__global__ __launch_bounds__(QB) void psa_attention_kernel(const _Float16* __restrict__ qkv, int ld_qkv, _Float16* __restrict__ out,
                                                           int ld_out, _Float16* __restrict__ vimg, int ld_v, int N, int heads, float scale) {
    __shared__ float Ks[KB][KD + 1];
    __shared__ float Vs[KB][HD + 1];
    const int b = blockIdx.z, h = blockIdx.y;
    const int n = blockIdx.x * QB + threadIdx.x;
    const bool live = n < N;
    const long img = (long)b * N;
    const int cq = h * (2 * KD + HD), ck = cq + KD, cv = cq + 2 * KD;
    float q[KD];
#pragma unroll
    for (int j = 0; j < KD; ++j) q[j] = live ? (float)qkv[(img + n) * ld_qkv + cq + j] * scale : 0.f;
    if (live)
#pragma unroll 8
        for (int d = 0; d < HD; ++d) vimg[(img + n) * ld_v + h * HD + d] = qkv[(img + n) * ld_qkv + cv + d];
    float acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
    float mx = -INFINITY, sum = 0.f;
    for (int m0 = 0; m0 < N; m0 += KB) {
        const int cnt = min(KB, N - m0);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * KD; i += QB) {
            const int m = i / KD, j = i - m * KD;
            Ks[m][j] = (float)qkv[(img + m0 + m) * ld_qkv + ck + j];
        }
        for (int i = threadIdx.x; i < cnt * HD; i += QB) {
            const int m = i / HD, d = i - m * HD;
            Vs[m][d] = (float)qkv[(img + m0 + m) * ld_qkv + cv + d];
        }
        __syncthreads();
        for (int m = 0; m < cnt; ++m) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KD; ++j) s = fmaf(q[j], Ks[m][j], s);
            if (s > mx) {   // new running max: rescale what was accumulated
                const float c = expf(mx - s);
                sum *= c;
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] *= c;
                mx = s;
            }
            const float p = expf(s - mx);
            sum += p;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = fmaf(p, Vs[m][d], acc[d]);
        }
    }
    if (!live) return;
    const float inv = 1.0f / sum;
#pragma unroll 8
    for (int d = 0; d < HD; ++d) out[(img + n) * ld_out + h * HD + d] = (_Float16)(acc[d] * inv);
}

}  // namespace

bool psa_attention_supported(int kd, int hd) { return (kd == 32 && hd == 64) || (kd == 36 && hd == 72); }

int32_t psa_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int kd, int hd,
                          float scale, hipStream_t s) {
    if (!psa_attention_supported(kd, hd) || B < 1 || heads < 1 || N < 1 || B > 65535 || heads > 65535 || ld_qkv < heads * (2 * kd + hd) ||
        ld_out < heads * hd || ld_v < heads * hd)
        return TRTX_ERR_UNSUPPORTED;
    const dim3 grid((N + QB - 1) / QB, heads, B);
    if (kd == 36)
        hipLaunchKernelGGL((psa_attention_kernel<36, 72>), grid, dim3(QB), 0, s, static_cast<const _Float16*>(qkv), ld_qkv,
                           static_cast<_Float16*>(out), ld_out, static_cast<_Float16*>(vimg), ld_v, N, heads, scale);
    else
        hipLaunchKernelGGL((psa_attention_kernel<32, 64>), grid, dim3(QB), 0, s, static_cast<const _Float16*>(qkv), ld_qkv,
                           static_cast<_Float16*>(out), ld_out, static_cast<_Float16*>(vimg), ld_v, N, heads, scale);
    return check_launch("psa_attention");
}

}  // namespace trtx
