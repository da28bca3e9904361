// Area attention of YOLOv12's AAttn (yolov12/src/block.cpp:522-625) on the matrix pipe: flash-style attention with both products on
// v_mfma_f32_16x16x32_f16.  Per image b, area a (the contiguous pixel range [a Na, (a + 1) Na) of the image, Na = N / area) and head h,
// with q, k (KD = 32 channels) and v (HD channels) read straight from the NHWC fp16 qkv tensor (head h's channels start at
// h * (2 KD + HD): q, then k, then v),
//     O[b, n, h*HD + d] = sum_{m in area(n)} v[m, d] * softmax_m(scale * sum_j q[n, j] k[m, j])
// written NHWC fp16 with the consumer's channel stride, plus the V image Vimg[b, n, h*HD + d] = v[n, d] that the positional conv `pe`
// reads (its epilogue adds O as the residual).  area = 1 is plain multi-head attention over the image.
//
// Mapping (the transposed one).  A workgroup is 4 waves and serves 64 queries of one (b, a, h), 16 per wave; the keys of the area pass
// through LDS in chunks of 64, shared by the four waves, the next chunk's global loads in flight (registers) while the current one is
// multiplied.  Per 32 keys a wave computes S^T = K Q^T as two 16x16x32 MFMAs (keys on the MFMA rows, the wave's 16 queries on the columns,
// KD = 32 is the one k-step).  With the accumulator map col = lane & 15, row = 4 (lane >> 4) + reg, a lane then holds 8 scores of ONE
// query, so the running max and sum are per-lane work plus one exchange over lane >> 4.  The K rows are read in the order
// row i of tile t = key 8 (i >> 2) + 4 t + (i & 3), which makes those 8 scores the keys 8 (lane >> 4) + 0..7 in order: exactly the
// B-operand fragment (k = 8 (lane >> 4) + j, col = lane & 15) of O^T = V^T P^T, no lane movement, and V^T is read from an LDS image that
// was stored transposed ([d][key]), 16 bytes per lane.  O^T has the query on the lane too, so the rescale by exp(m_old - m_new) is per lane.
//
// Numerics: scores are fp32 MFMA sums of exact fp16 products; the scale multiplies the fp32 score before the max; max, exponentials, the
// denominator (sum of the unrounded fp32 p) and O are fp32; p is rounded to fp16 only as the MFMA operand; O is rounded once at the store.
// Keys beyond the area are never read: their LDS rows are zero-filled and their scores set to -inf (a 32-key group with no key in range
// is skipped, so every processed group has a finite max).  Queries beyond the area read nothing and store nothing.
// HD is a template parameter (HD / 16 accumulator tiles); 32 is the instantiation AAttn needs.
//
// YOLOv13's AAttn (yolov13/src/block.cpp:303-423) takes q | k from one 1x1 convolution and v from another.  SPLIT is that form of the same body: three
// operands with their own base, pixel stride and vector flag, head h's q and k at channel h * KD and its v at h * HD, and no V image (v is a tensor that
// `pe` reads as it is).  Only the addresses differ, so on equal values O is bit-equal between the two instantiations.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../common.h"
#include "kernels.h"

namespace trtx {
namespace {

using h8 = __attribute__((ext_vector_type(8))) _Float16;
using h4 = __attribute__((ext_vector_type(4))) _Float16;
using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int KD = 32;        // q / k channels per head: one MFMA k-step
constexpr int QW = 16;        // queries per wave
constexpr int WAVES = 4;
constexpr int QB = QW * WAVES;   // queries per workgroup
constexpr int THREADS = 64 * WAVES;
constexpr int KC = 64;        // keys per LDS chunk
constexpr int KS_LD = KD + 8;   // halves per K row: 80 bytes, 16-byte rows 5 slots apart -> the b128 fragment reads spread over the banks
constexpr int VT_LD = KC + 8;   // halves per V^T row: 144 bytes, rows 9 slots apart

// 8 consecutive halves: one 16-byte load where the address allows it
__device__ inline h8 load8(const _Float16* p, bool vec) {
    if (vec) return *reinterpret_cast<const h8*>(p);
    h8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = p[i];
    return r;
}
__device__ inline void store8(_Float16* p, h8 v, bool vec) {
    if (vec) {
        *reinterpret_cast<h8*>(p) = v;
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = v[i];
}

// Where a head's q, k and v rows are.  Packed: one qkv tensor, head h's channels at h * (2 KD + HD) as q, k, v, and the V image is written.
// Split: three operands, each with its own base, pixel stride and vector flag; head h's q and k at h * KD, its v at h * HD; no V image.
template <int HD, bool SPLIT>
__global__ __launch_bounds__(THREADS) void area_attention_mfma_kernel(const _Float16* __restrict__ q, int ld_q, const _Float16* __restrict__ k, int ld_k,
                                                                         const _Float16* __restrict__ v, int ld_vin, _Float16* __restrict__ out, int ld_out,
                                                                         _Float16* __restrict__ vimg, int ld_v, int N, int Na, int heads, float scale,
                                                                         int vec_q, int vec_k, int vec_vin, int vec_o, int vec_v) {
    constexpr int T = THREADS;
    constexpr int VG = HD / 8;       // 8-channel groups of a V row
    constexpr int VL = KC * VG / T;  // V groups a thread stages per chunk
    constexpr int OT = HD / 16;      // accumulator tiles of O^T
    static_assert(KC * KD / 8 == T && VL >= 1, "staging assumes one K group and VL V groups per thread");
    __shared__ __attribute__((aligned(16))) _Float16 Ks[KC][KS_LD];
    __shared__ __attribute__((aligned(16))) _Float16 Vt[HD][VT_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int a = blockIdx.y / heads, h = blockIdx.y - a * heads, b = blockIdx.z;
    const long pix0 = (long)b * N + (long)a * Na;   // first pixel of the area
    const _Float16 *qh, *kh, *vh;   // the head's first q, k and v channel of pixel 0
    if constexpr (SPLIT) {
        qh = q + h * KD;
        kh = k + h * KD;
        vh = v + h * HD;
    } else {
        qh = q + h * (2 * KD + HD);
        kh = qh + KD;
        vh = qh + 2 * KD;
        ld_k = ld_vin = ld_q;
        vec_k = vec_vin = vec_q;
    }
    const int q0 = blockIdx.x * QB;
    const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    if constexpr (!SPLIT) {   // the V image of this workgroup's own 64 query pixels
        for (int i = t; i < QB * VG; i += T) {
            const int n = q0 + i / VG, dg = i % VG;
            if (n < Na) store8(vimg + (pix0 + n) * ld_v + h * HD + 8 * dg, load8(vh + (pix0 + n) * ld_vin + 8 * dg, vec_vin), vec_v);
        }
    }
    // Q^T fragment: query i16 of the wave, channels 8 g .. 8 g + 7
    const int qn = q0 + wave * QW + i16;
    const h8 qf = qn < Na ? load8(qh + (pix0 + qn) * ld_q + 8 * g, vec_q) : zero8;

    h8 kreg, vreg[VL];
    auto fetch = [&](int c0) {   // global -> registers; rows beyond the area become zeros without a read
        const int key = c0 + (t >> 2);
        kreg = key < Na ? load8(kh + (pix0 + key) * ld_k + 8 * (t & 3), vec_k) : zero8;
#pragma unroll
        for (int u = 0; u < VL; ++u) {
            const int idx = t + u * T, kv = c0 + idx / VG;
            vreg[u] = kv < Na ? load8(vh + (pix0 + kv) * ld_vin + 8 * (idx % VG), vec_vin) : zero8;
        }
    };
    auto stage = [&]() {         // registers -> LDS: K rows as they are, V transposed
        *reinterpret_cast<h8*>(&Ks[t >> 2][8 * (t & 3)]) = kreg;
#pragma unroll
        for (int u = 0; u < VL; ++u) {
            const int idx = t + u * T, kv = idx / VG, d0 = 8 * (idx % VG);
#pragma unroll
            for (int j = 0; j < 8; ++j) Vt[d0 + j][kv] = vreg[u][j];
        }
    };

    f4 acc[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) acc[o] = f4{0.f, 0.f, 0.f, 0.f};
    float mx = -INFINITY, lsum = 0.f;   // running max of the query; this lane's share of the denominator (its 8 keys of every group)

    fetch(0);
    for (int c0 = 0; c0 < Na; c0 += KC) {
        __syncthreads();   // the previous chunk's fragment reads are done (every wave waited for its LDS reads before this barrier)
        stage();
        __syncthreads();
        if (c0 + KC < Na) fetch(c0 + KC);   // in flight while this chunk is multiplied
        const int cnt = min(KC, Na - c0);
#pragma unroll
        for (int sub = 0; sub < KC / 32; ++sub) {
            if (32 * sub >= cnt) break;   // uniform: no key of this group is in range
            const int krow = 32 * sub + 8 * (i16 >> 2) + (i16 & 3);
            const h8 k0 = *reinterpret_cast<const h8*>(&Ks[krow][8 * g]);
            const h8 k1 = *reinterpret_cast<const h8*>(&Ks[krow + 4][8 * g]);
            h8 vf[OT];
#pragma unroll
            for (int o = 0; o < OT; ++o) vf[o] = *reinterpret_cast<const h8*>(&Vt[16 * o + i16][32 * sub + 8 * g]);
            const f4 z = {0.f, 0.f, 0.f, 0.f};
            const f4 s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0, qf, z, 0, 0, 0);
            const f4 s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1, qf, z, 0, 0, 0);
            float s[8];
            const int key0 = 32 * sub + 8 * g;   // this lane's keys of the group: key0 .. key0 + 7
            float tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[j] = key0 + j < cnt ? (j < 4 ? s0[j] : s1[j - 4]) * scale : -INFINITY;
                tmax = fmaxf(tmax, s[j]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float mnew = fmaxf(mx, tmax);   // finite: the group has a key in range
            const float alpha = __expf(mx - mnew);
            mx = mnew;
            float psum = 0.f;
            h8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = __expf(s[j] - mnew);
                psum += p;
                pf[j] = (_Float16)p;
            }
            lsum = lsum * alpha + psum;
#pragma unroll
            for (int o = 0; o < OT; ++o) {
                acc[o] *= alpha;
                acc[o] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[o], pf, acc[o], 0, 0, 0);
            }
        }
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (qn >= Na) return;
    const float inv = 1.0f / lsum;
    _Float16* op = out + (pix0 + qn) * ld_out + h * HD + 4 * g;   // O^T tile o, rows 4 g + r: channels 16 o + 4 g + r of the query
#pragma unroll
    for (int o = 0; o < OT; ++o) {
        h4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (_Float16)(acc[o][j] * inv);
        if (vec_o) {
            *reinterpret_cast<h4*>(op + 16 * o) = r;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) op[16 * o + j] = r[j];
        }
    }
}

bool aligned(const void* p, int ld, int bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0 && ((size_t)ld * 2) % bytes == 0; }

}  // namespace

bool area_attention_supported(int kd, int hd) { return kd == KD && hd == 32; }

int32_t area_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int area, int kd,
                           int hd, float scale, hipStream_t s) {
    if (!area_attention_supported(kd, hd) || B < 1 || heads < 1 || N < 1 || area < 1 || N % area != 0 || B > 65535 || (long)heads * area > 65535 ||
        ld_qkv < heads * (2 * kd + hd) || ld_out < heads * hd || ld_v < heads * hd)
        return TRTX_ERR_UNSUPPORTED;
    const int Na = N / area;
    // 16-byte loads of qkv and stores of the V image, 8-byte stores of O where base and channel stride allow; element-wise otherwise
    const _Float16* in = static_cast<const _Float16*>(qkv);
    const int vec_in = aligned(qkv, ld_qkv, 16);
    hipLaunchKernelGGL((area_attention_mfma_kernel<32, false>), dim3((Na + QB - 1) / QB, heads * area, B), dim3(THREADS), 0, s, in, ld_qkv, in, ld_qkv, in,
                       ld_qkv, static_cast<_Float16*>(out), ld_out, static_cast<_Float16*>(vimg), ld_v, N, Na, heads, scale, vec_in, vec_in, vec_in,
                       (int)aligned(out, ld_out, 8), (int)aligned(vimg, ld_v, 16));
    return check_launch("area_attention");
}

bool area_attention_split_supported(int kd, int hd) { return area_attention_supported(kd, hd); }

int32_t area_attention_split_f16(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, void* out, int ld_out, int B, int heads, int N,
                                 int area, int kd, int hd, float scale, hipStream_t s) {
    if (!area_attention_split_supported(kd, hd) || B < 1 || heads < 1 || N < 1 || area < 1 || N % area != 0 || B > 65535 || (long)heads * area > 65535 ||
        ld_q < heads * kd || ld_k < heads * kd || ld_v < heads * hd || ld_out < heads * hd)
        return TRTX_ERR_UNSUPPORTED;
    const int Na = N / area;
    // per operand: 16-byte loads of q, k and v, 8-byte stores of O where its base and channel stride allow; element-wise otherwise
    hipLaunchKernelGGL((area_attention_mfma_kernel<32, true>), dim3((Na + QB - 1) / QB, heads * area, B), dim3(THREADS), 0, s, static_cast<const _Float16*>(q),
                       ld_q, static_cast<const _Float16*>(k), ld_k, static_cast<const _Float16*>(v), ld_v, static_cast<_Float16*>(out), ld_out,
                       static_cast<_Float16*>(nullptr), 0, N, Na, heads, scale, (int)aligned(q, ld_q, 16), (int)aligned(k, ld_k, 16), (int)aligned(v, ld_v, 16),
                       (int)aligned(out, ld_out, 8), 0);
    return check_launch("area_attention_split");
}

}  // namespace trtx
