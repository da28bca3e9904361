// Attention of fp32 engines (the tolerance build) on the fp32 matrix instruction: flash-style attention on the NHWC fp32 packed qkv tensor with both
// products on v_mfma_f32_16x16x4_f32.  The tensors and arguments are those of area_attention_f16 and psa_attention_mfma_f16 (kernels/attention_mfma.hip):
// per image b, area a (the contiguous pixel range [a Na, (a + 1) Na) of the image, Na = N / area; area = 1 is plain multi-head attention, which is PSA)
// and head h, with q, k (KD channels) and v (HD channels) read straight from qkv (head h's channels start at h * (2 KD + HD): q, then k, then v),
//     O[b, n, h*HD + d] = sum_{m in area(n)} v[m, d] * softmax_m(scale * sum_j q[n, j] k[m, j])
// written NHWC fp32 with the consumer's channel stride, plus the V image Vimg[b, n, h*HD + d] = v[n, d].  (KD, HD) = (32, 32) is YOLOv12's AAttn,
// (32, 64) YOLO11's C2PSA / YOLOv10's PSA, (36, 72) yolov10m.
//
// The instruction.  D (16x16) += A (16x4) B (4x16); a lane gives ONE float of each operand, A[row = lane & 15][k = lane >> 4] and
// B[k = lane >> 4][col = lane & 15], and holds D[row = 4 (lane >> 4) + reg][col = lane & 15] in four registers.  Below i16 = lane & 15, g = lane >> 4.
//
// Mapping (the transposed one: queries on the MFMA columns - the lane -, keys on the rows).  A workgroup is 4 waves and serves 64 queries of one
// (b, a, h), 16 per wave; the keys of the area pass through LDS in chunks of 64, shared by the four waves, the next chunk's global loads in flight
// (registers) while the current one is multiplied.
//   * Scores.  S^T = K Q^T of a 16-key tile is a chain of KD / 4 k-steps on one accumulator: 8 for KD 32, 9 for KD 36 - the reduction has no padding.
//     The k index of an MFMA is only a name for "which product": both operands give the same channel at the same (step, g), any assignment that visits
//     every channel once is the same sum.  Step s < 8 takes channel 8 g + s, step 8 (KD 36) channel 32 + g: a lane's q fragment and its K fragment are
//     then 8 consecutive floats (two 16-byte accesses) plus one.
//   * The K rows of a tile are read in the order "row 4 g' + r = key 4 r + g'" (lane i16 reads key 4 (i16 & 3) + (i16 >> 2)).  Register r of lane group g
//     of the score tile is then key 4 r + g of the tile: exactly the B operand (k = g, col = i16) of k-step r of O^T = V^T P^T.  P never leaves its lane
//     and is never rounded; the running max is per-lane work over the lane's 16 scores of a chunk plus one exchange over g, the denominator a per-lane
//     share summed over g at the end, the rescale by exp(old max - new max) per lane.
//   * V^T comes from an LDS image stored [d][key position], the keys of a tile permuted so that what a lane needs is contiguous: key 4 r + g of tile t
//     sits at position 16 t + 4 g + r.  The A operands of the four k-steps of (tile t, row tile o) are then ONE 16-byte read Vt[16 o + i16][16 t + 4 g .. + 3].
//   * O^T has ceil(HD / 16) row tiles.  HD 72 makes the fifth half live: rows 72 .. 79 are register zeros that are never loaded (V^T has HD rows), and only
//     the lane groups 0 and 1 (channels 64 .. 71) store it.
//
// LDS and its banks (64 banks of 4 bytes; a 16-byte access covers 4 consecutive banks, so there are 16 "slots", and 16 lanes with distinct slots are
// one conflict-free pass - four passes per wave-wide 16-byte read is the floor).
//   * K rows: KS_LD = 36 floats = 9 slots, for both KD (36 channels fill the row, 32 leave 4 floats of padding).  A 16-lane group (one g) reads the 16 rows of
//     a tile at the same offset: slots 9 row + const mod 16, 9 is odd, 16 consecutive rows -> 16 distinct slots.  The tail float Ks[row][32 + g]: bank
//     36 row + 32 + g mod 64; 36 row mod 64 over 16 consecutive rows is 16 distinct multiples of 4, plus g in 0 .. 3 -> a wave's 64 reads on 64 distinct banks.
//   * V^T rows: VT_LD = 68 floats = 17 slots.  A 16-lane group reads rows 16 o + i16 at the same position: slots 17 i16 + const mod 16 = i16 + const ->
//     16 distinct slots.  (One float per lane per step instead would be bank 68 i16 + g = 4 i16 + g mod 64: distinct too, at four times the instructions.)
//     The transposing store writes 4 floats of one key down a column: a wave stores (64 / VG) keys x VG channel groups, bank 16 dg + position mod 64:
//     two lanes per bank at worst.
//   * 9216 B of K plus 8704 / 17408 / 19584 B of V^T (HD 32 / 64 / 72).  No scratch, no workspace.
//
// Numerics: scores are fp32 MFMA sums of fp32 products; the scale multiplies the fp32 score before the max; max, exponentials (__expf), the denominator,
// P and O are fp32, nothing is rounded to fp16 anywhere; the V image holds the input's bits.  Keys beyond the area are never read: their LDS rows are
// zero-filled and their scores set to -inf; a 16-key tile with no key in range is skipped (neither product is issued), and every chunk has a key in
// range, so the running max is finite from the first chunk on.  Queries beyond the area load nothing and store nothing.
// Accesses are 16 bytes (4 floats) where base pointer and channel stride allow - a head's q, k, v and O channels then start on such boundaries for all
// three head shapes - and element-wise otherwise; which one is taken changes no bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../common.h"
#include "kernels.h"

namespace trtx {
namespace {

using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int QW = 16;        // queries per wave
constexpr int WAVES = 4;
constexpr int QB = QW * WAVES;   // queries per workgroup
constexpr int THREADS = 64 * WAVES;
constexpr int KC = 64;        // keys per LDS chunk
constexpr int KT = KC / 16;   // 16-key tiles of a chunk
constexpr int KS_LD = 36;     // floats per K row
constexpr int VT_LD = KC + 4; // floats per V^T row

__device__ inline f4 load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const f4*>(p);
    f4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = p[i];
    return r;
}
__device__ inline void store4(float* p, f4 v, bool vec) {
    if (vec) {
        *reinterpret_cast<f4*>(p) = v;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = v[i];
}

template <int PKD, int HD>
__global__ __launch_bounds__(THREADS) void attention_f32_kernel(const float* __restrict__ qkv, int ld_qkv, float* __restrict__ out, int ld_out,
                                                                   float* __restrict__ vimg, int ld_v, int N, int Na, int heads, float scale, int vec_in,
                                                                   int vec_o, int vec_v) {
    constexpr int T = THREADS;
    constexpr int KS = PKD / 4;                   // k-steps of the score product
    constexpr int KG = PKD / 4;                   // 4-channel pieces of a K row
    constexpr int KL = (KC * KG + T - 1) / T;     // K pieces a thread stages per chunk (the last round partly idle when PKD = 36)
    constexpr int VG = HD / 4;                    // 4-channel pieces of a V row
    constexpr int VL = (KC * VG + T - 1) / T;
    constexpr int OT = (HD + 15) / 16;            // accumulator tiles of O^T
    static_assert((PKD == 32 || PKD == 36) && PKD <= KS_LD && HD % 4 == 0, "eight k-steps of 8 g + s, at most one of 32 + g; whole 4-channel V pieces");
    __shared__ __attribute__((aligned(16))) float Ks[KC][KS_LD];
    __shared__ __attribute__((aligned(16))) float Vt[HD][VT_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int a = blockIdx.y / heads, h = blockIdx.y - a * heads;
    const long pix0 = (long)blockIdx.z * N + (long)a * Na;   // first pixel of the area
    const float* qh = qkv + h * (2 * PKD + HD);
    const float* kh = qh + PKD;
    const float* vh = qh + 2 * PKD;
    const int q0 = blockIdx.x * QB;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    for (int i = t; i < QB * VG; i += T) {   // the V image of this workgroup's own 64 query pixels
        const int n = q0 + i / VG, dg = i % VG;
        if (n < Na) store4(vimg + (pix0 + n) * ld_v + h * HD + 4 * dg, load4(vh + (pix0 + n) * ld_qkv + 4 * dg, vec_in), vec_v);
    }
    // Q^T fragments: query i16 of the wave; step s < 8 is channel 8 g + s, step 8 channel 32 + g
    const int qn = q0 + wave * QW + i16;
    float qf[KS];
    {
        const float* qp = qh + (pix0 + qn) * ld_qkv;
        const f4 lo = qn < Na ? load4(qp + 8 * g, vec_in) : zero4, hi = qn < Na ? load4(qp + 8 * g + 4, vec_in) : zero4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qf[j] = lo[j];
            qf[4 + j] = hi[j];
        }
        if constexpr (KS > 8) qf[8] = qn < Na ? qp[32 + g] : 0.f;
    }

    f4 kreg[KL], vreg[VL];
    auto fetch = [&](int c0) {   // global -> registers; rows beyond the area become zeros without a read
#pragma unroll
        for (int u = 0; u < KL; ++u) {
            const int idx = t + u * T, key = c0 + idx / KG;
            kreg[u] = idx < KC * KG && key < Na ? load4(kh + (pix0 + key) * ld_qkv + 4 * (idx % KG), vec_in) : zero4;
        }
#pragma unroll
        for (int u = 0; u < VL; ++u) {
            const int idx = t + u * T, kv = c0 + idx / VG;
            vreg[u] = idx < KC * VG && kv < Na ? load4(vh + (pix0 + kv) * ld_qkv + 4 * (idx % VG), vec_in) : zero4;
        }
    };
    auto stage = [&]() {         // registers -> LDS: K rows as they are, V transposed with key 4 r + g' of a tile at position 4 g' + r
#pragma unroll
        for (int u = 0; u < KL; ++u) {
            const int idx = t + u * T;
            if (idx < KC * KG) *reinterpret_cast<f4*>(&Ks[idx / KG][4 * (idx % KG)]) = kreg[u];
        }
#pragma unroll
        for (int u = 0; u < VL; ++u) {
            const int idx = t + u * T, kv = idx / VG, d0 = 4 * (idx % VG);
            const int pos = (kv & ~15) + 4 * (kv & 3) + ((kv >> 2) & 3);
            if (idx < KC * VG) {
#pragma unroll
                for (int j = 0; j < 4; ++j) Vt[d0 + j][pos] = vreg[u][j];
            }
        }
    };

    f4 acc[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) acc[o] = zero4;
    float mx = -INFINITY, lsum = 0.f;   // running max of the query; this lane's share of the denominator (its 16 keys of every chunk)
    const int krow = 4 * (i16 & 3) + (i16 >> 2);   // the key of a tile whose K row this lane gives as MFMA row i16

    fetch(0);
    for (int c0 = 0; c0 < Na; c0 += KC) {
        __syncthreads();   // the previous chunk's fragment reads are done
        stage();
        __syncthreads();
        if (c0 + KC < Na) fetch(c0 + KC);   // in flight while this chunk is multiplied
        const int cnt = min(KC, Na - c0);   // >= 1
        f4 s[KT];
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            s[kt] = f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (16 * kt >= cnt) continue;   // uniform: no key of this tile is in range
            const float* kp = &Ks[16 * kt + krow][0];
            const f4 lo = *reinterpret_cast<const f4*>(kp + 8 * g), hi = *reinterpret_cast<const f4*>(kp + 8 * g + 4);
            f4 d = zero4;
#pragma unroll
            for (int j = 0; j < 4; ++j) d = __builtin_amdgcn_mfma_f32_16x16x4f32(lo[j], qf[j], d, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) d = __builtin_amdgcn_mfma_f32_16x16x4f32(hi[j], qf[4 + j], d, 0, 0, 0);
            if constexpr (KS > 8) d = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[32 + g], qf[8], d, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // register r is key 4 r + g of the tile
                s[kt][r] = 16 * kt + 4 * r + g < cnt ? d[r] * scale : -INFINITY;
                tmax = fmaxf(tmax, s[kt][r]);
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew = fmaxf(mx, tmax);   // finite: key c0 is in range
        const float alpha = __expf(mx - mnew);
        mx = mnew;
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] = __expf(s[kt][r] - mnew);   // P, in place: exp(-inf) = 0 for the keys beyond the area
                psum += s[kt][r];
            }
        }
        lsum = lsum * alpha + psum;
#pragma unroll
        for (int o = 0; o < OT; ++o) acc[o] *= alpha;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            if (16 * kt >= cnt) continue;
            f4 vf[OT];
#pragma unroll
            for (int o = 0; o < OT; ++o)   // the rows of the last tile beyond HD are zeros
                vf[o] = 16 * o + i16 < HD ? *reinterpret_cast<const f4*>(&Vt[min(16 * o + i16, HD - 1)][16 * kt + 4 * g]) : zero4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 0; o < OT; ++o) acc[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[o][r], s[kt][r], acc[o], 0, 0, 0);
            }
        }
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (qn >= Na) return;
    const float inv = 1.0f / lsum;
    float* op = out + (pix0 + qn) * ld_out + h * HD + 4 * g;   // O^T tile o, rows 4 g + r: channels 16 o + 4 g + r of the query
#pragma unroll
    for (int o = 0; o < OT; ++o) {
        if (16 * o + 4 * g >= HD) continue;   // the padding rows of the last tile (HD is a multiple of 4: a lane's four rows are live or padding together)
        store4(op + 16 * o, acc[o] * inv, vec_o);
    }
}

bool aligned16(const void* p, int ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0; }

template <int PKD, int HD>
void launch(const float* qkv, int ld_qkv, float* out, int ld_out, float* vimg, int ld_v, int B, int heads, int N, int area, float scale, hipStream_t s) {
    const int Na = N / area;
    hipLaunchKernelGGL((attention_f32_kernel<PKD, HD>), dim3((Na + QB - 1) / QB, heads * area, B), dim3(THREADS), 0, s, qkv, ld_qkv, out, ld_out, vimg, ld_v, N,
                       Na, heads, scale, (int)aligned16(qkv, ld_qkv), (int)aligned16(out, ld_out), (int)aligned16(vimg, ld_v));
}

}  // namespace

bool attention_f32_supported(int kd, int hd) { return (kd == 32 && (hd == 32 || hd == 64)) || (kd == 36 && hd == 72); }

int32_t attention_f32(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int area, int kd, int hd,
                      float scale, hipStream_t s) {
    if (!attention_f32_supported(kd, hd) || B < 0 || heads < 0 || N < 0 || area < 1 || N % area != 0 || B > 65535 || (long)heads * area > 65535 ||
        ld_qkv < heads * (2 * kd + hd) || ld_out < heads * hd || ld_v < heads * hd)
        return TRTX_ERR_UNSUPPORTED;
    if (B == 0 || heads == 0 || N == 0) return TRTX_OK;   // empty tensors: nothing to launch
    const float* in = static_cast<const float*>(qkv);
    float *o = static_cast<float*>(out), *v = static_cast<float*>(vimg);
    if (hd == 32)
        launch<32, 32>(in, ld_qkv, o, ld_out, v, ld_v, B, heads, N, area, scale, s);
    else if (hd == 64)
        launch<32, 64>(in, ld_qkv, o, ld_out, v, ld_v, B, heads, N, area, scale, s);
    else
        launch<36, 72>(in, ld_qkv, o, ld_out, v, ld_v, B, heads, N, area, scale, s);
    return check_launch("attention_f32");
}

}  // namespace trtx
