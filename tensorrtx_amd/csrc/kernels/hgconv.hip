// YOLOv13's adaptive hypergraph convolution (AdaHyperedgeGen + AdaHGConv, yolov13/src/block.cpp:607-790) as one op on the NHWC fp16 tensor
// of C3AH.cv1.  Per image, with X the N = H W tokens of D channels, E hyperedges, heads = D / 16 contiguous channel groups:
//     ctx    = [mean_n X, max_n X]                                        (2 D values)
//     P      = prototype_base + reshape(W_ctx ctx + b_ctx, E x D)
//     logits = mean_h(X_proj_h . P_h) / sqrt(head_dim),  X_proj = X W_pre^T + b_pre
//     A      = softmax of the logits OVER THE NODE AXIS n (block.cpp:696-697: setAxes(1 << 1) on {B, N, E})
//     He     = A^T X,   He' = GELU(He W_edge^T + b_edge)
//     out    = GELU((A He') W_node^T + b_node) + X                        (GELU = the reference's tanh chain, block.cpp:702-744)
//
// The fold.  The heads partition D, so the mean over heads of the per-head dot products is the full dot product over D divided by heads:
//     logits[n, e] = s X[n] . Q[e] + const_e,   Q = P W_pre (E x D),   s = 1 / (heads sqrt(head_dim)),   const_e = s b_pre . P[e]
// and const_e does not depend on n, so it cancels in the softmax over n (b_pre is never read).  On the way out
//     (A He') W_node^T = A G,   G = He' W_node^T (E x D).
// Neither N x D x D product is left: an image costs three passes over X with an inner dimension of E <= 16 plus E-row products with the
// D x D matrices.
//
// The launch chain (eight ordinary launches on one stream; `ws` = the caller's workspace, laid out by hg_layout):
//   1 hg_colstat   grid (D / 64, B)      ctx: every column's mean and max over the N rows of the image
//   2 hg_proto     grid (E D / 8)        P for every image: a wave per row of W_ctx, the row in registers, the images' ctx through LDS
//   3 hg_rows<T>   grid (D / 64, B)      Q = P W_pre
//   4 hg_logits    grid (N / 128, B)     logits of a 128-node tile in sub-tiles of 32, and the tile's online-softmax partial per hyperedge:
//                                        m_e = max, s_e = sum exp(l - m_e), H_e = sum exp(l - m_e) X[n]
//   5 hg_merge     grid (E, B)           M_e, S_e and He = sum_t H_t exp(m_t - M) / S over the tiles t in ascending order
//   6 hg_rows<N>   grid (D / 64, B)      He' = GELU(He W_edge^T + b_edge)
//   7 hg_rows<N>   grid (D / 64, B)      G = He' W_node^T
//   8 hg_node      grid (N / 128, B)     out[n] = GELU(sum_e exp(l[n, e] - M_e) / S_e G[e] + b_node) + X[n], rounded to fp16 once
// A launch reads only what an earlier launch of the chain wrote: no workgroup waits for another one, there is no cooperative launch, no
// arrival counter and no atomic.  Every sum has one fixed order and the node tiles depend on N alone, so an image's result is the same
// bits at any batch size, at any position in the batch and in every process.
//
// Numerics: X is fp16, everything else (weights, scores, max, exponentials, sums, P, Q, He, G) is fp32 with the accurate expf / tanhf.
// Rows beyond N are never read: they enter neither the column max, nor a softmax max or sum, and their output rows are not stored.
// X and out are read and written 16 bytes per lane; a base pointer or a pixel stride that rules that out is refused (TRTX_ERR_UNSUPPORTED),
// as is D % 16 != 0, D > 384, E < 1 or E > 16 (hgconv_supported).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../common.h"
#include "act.h"
#include "kernels.h"

namespace trtx {
namespace {

constexpr int HG_MAX_D = 384;
constexpr int HG_MAX_E = 16;
constexpr int HG_TILE = 128;     // nodes per workgroup of hg_logits and hg_node: the partition of the softmax partials
constexpr int HG_SUB = 32;       // nodes per online-softmax step inside a tile
constexpr int HG_THREADS = 256;
constexpr int HG_PROTO_ROWS = 2; // rows of W_ctx per wave
constexpr int HG_PROTO_IMGS = 8; // images whose ctx is in LDS at a time

// ---- 1: ctx[b] = [mean over n, max over n] of every column.  8 lanes read 64 channels of a row (16 bytes each), 32 rows at a time; a lane's
// rows n = rg, rg + 32, ... are summed in that order, then the 32 row groups in ascending order.
__global__ __launch_bounds__(HG_THREADS) void hg_colstat_kernel(const _Float16* __restrict__ x, int ld_x, float* __restrict__ ctx, int N, int D) {
    __shared__ float ssum[32][65], smax[32][65];
    const int b = blockIdx.y, tid = threadIdx.x, sub = tid & 7, rg = tid >> 3;
    const int c = blockIdx.x * 64 + sub * 8;
    float sum[8], mx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { sum[i] = 0.f; mx[i] = -INFINITY; }
    if (c < D) {
        const _Float16* col = x + (size_t)b * N * ld_x + c;
        for (int n = rg; n < N; n += 32) {
            const half8 v = *reinterpret_cast<const half8*>(col + (size_t)n * ld_x);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float f = (float)v[i];
                sum[i] += f;
                mx[i] = fmaxf(mx[i], f);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) { ssum[rg][sub * 8 + i] = sum[i]; smax[rg][sub * 8 + i] = mx[i]; }
    __syncthreads();
    if (tid < 64 && blockIdx.x * 64 + tid < D) {
        float s = 0.f, m = -INFINITY;
        for (int r = 0; r < 32; ++r) { s += ssum[r][tid]; m = fmaxf(m, smax[r][tid]); }
        float* o = ctx + (size_t)b * 2 * D;
        o[blockIdx.x * 64 + tid] = s / (float)N;
        o[D + blockIdx.x * 64 + tid] = m;
    }
}

// ---- 2: P[b][r] = proto[r] + (W_ctx[r] . ctx[b] + b_ctx[r]) for the E D rows r.  A wave owns HG_PROTO_ROWS rows; a row's 2 D <= 768 weights sit in
// 12 registers per lane and meet the ctx of HG_PROTO_IMGS images at a time in LDS, so W_ctx (14 MB at D = 384, E = 12) is read B / 8 times, not B.
// An image's dot product is summed per lane over k, then over the lanes by the xor butterfly: the same order for every image and batch size.
__global__ __launch_bounds__(HG_THREADS) void hg_proto_kernel(const float* __restrict__ ctx, const float* __restrict__ w_ctx, const float* __restrict__ b_ctx,
                                                              const float* __restrict__ proto, float* __restrict__ P, int B, int D, int E) {
    __shared__ float sctx[HG_PROTO_IMGS][2 * HG_MAX_D];
    const int K2 = 2 * D, rows = E * D, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = (blockIdx.x * (HG_THREADS / 64) + wave) * HG_PROTO_ROWS;
    for (int b0 = 0; b0 < B; b0 += HG_PROTO_IMGS) {
        const int nb = min(HG_PROTO_IMGS, B - b0);
        __syncthreads();
        for (int i = tid; i < nb * K2; i += HG_THREADS) sctx[i / K2][i % K2] = ctx[(size_t)b0 * K2 + i];
        __syncthreads();
        for (int rr = 0; rr < HG_PROTO_ROWS; ++rr) {
            const int r = row0 + rr;
            if (r >= rows) break;   // (wave-uniform)
            float w[2 * HG_MAX_D / 64];
#pragma unroll
            for (int k = 0; k < 2 * HG_MAX_D / 64; ++k) w[k] = lane + 64 * k < K2 ? w_ctx[(size_t)r * K2 + lane + 64 * k] : 0.f;
            const float base = proto[r], bias = b_ctx[r];
            for (int bi = 0; bi < nb; ++bi) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 2 * HG_MAX_D / 64; ++k)
                    if (lane + 64 * k < K2) acc += w[k] * sctx[bi][lane + 64 * k];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
                if (lane == 0) P[(size_t)(b0 + bi) * rows + r] = base + (acc + bias);
            }
        }
    }
}

// ---- 3, 6, 7: out[b][e][j] = act(sum_d V[b][e][d] W(j, d) + bias[j]) for the E rows of an image and 64 columns j per workgroup (one wave).
// WT: W is stored [d][j] (Q = P W_pre: lane j reads row d coalesced).  Otherwise W is [j][d] (a Linear's weight): 64 x 64 tiles pass through LDS,
// read coalesced along d and used transposed.  d ascends in both forms.
template <bool WT>
__global__ __launch_bounds__(64) void hg_rows_kernel(const float* __restrict__ V, const float* __restrict__ W, const float* __restrict__ bias,
                                                     float* __restrict__ out, int D, int E, int act) {
    __shared__ float sv[HG_MAX_E * HG_MAX_D];
    __shared__ float sw[WT ? 1 : 64][65];
    const int b = blockIdx.y, tid = threadIdx.x, j0 = blockIdx.x * 64, j = j0 + tid;
    for (int i = tid; i < E * D; i += 64) sv[i] = V[(size_t)b * E * D + i];
    float acc[HG_MAX_E];
#pragma unroll
    for (int e = 0; e < HG_MAX_E; ++e) acc[e] = 0.f;
    __syncthreads();
    if (WT) {
        for (int d = 0; d < D; ++d) {
            const float w = j < D ? W[(size_t)d * D + j] : 0.f;
#pragma unroll
            for (int e = 0; e < HG_MAX_E; ++e)
                if (e < E) acc[e] += sv[e * D + d] * w;
        }
    } else {
        for (int d0 = 0; d0 < D; d0 += 64) {
            __syncthreads();
            for (int i = tid; i < 64 * 64; i += 64) {
                const int jj = i >> 6, dd = i & 63;
                sw[jj][dd] = (j0 + jj < D && d0 + dd < D) ? W[(size_t)(j0 + jj) * D + d0 + dd] : 0.f;
            }
            __syncthreads();
            const int nd = min(64, D - d0);
            for (int dd = 0; dd < nd; ++dd) {
                const float w = sw[tid][dd];
#pragma unroll
                for (int e = 0; e < HG_MAX_E; ++e)
                    if (e < E) acc[e] += sv[e * D + d0 + dd] * w;
            }
        }
    }
    if (j < D) {
        const float bj = bias ? bias[j] : 0.f;
#pragma unroll
        for (int e = 0; e < HG_MAX_E; ++e)
            if (e < E) out[((size_t)b * E + e) * D + j] = act_exact(acc[e] + bj, act, 0.f);
    }
}

// ---- 4: the logits of one 128-node tile and its softmax partial.  Per sub-tile of 32 nodes:
//   a  8 lanes per node: each reads its 8-channel pieces of the row (16 bytes), keeps them in LDS and sums its share of the E dot products with Q
//      (LDS, broadcast over the nodes); the 8 lanes add up by the xor butterfly; logits = scale * sum, to the workspace and to LDS
//   b  thread e: the sub-tile's max, the new running max, the factor exp(m_old - m_new) for what has been summed so far
//   c  every thread: a[n][e] = exp(l - m_new)
//   d  thread e: s_e = s_e f + sum_n a (ascending n); thread c2 (two channels): H[e][c] = H[e][c] f + sum_n a[n][e] X[n][c]
// Only the nv <= 32 rows inside the image are read, scored or summed.  The loops over e run to EB without a guard: rows [E, EB) of Q are zero in
// LDS, so those hyperedges have logits 0 everywhere (finite, harmless) and nothing of them is stored.
template <int EB>   // E rounded up to 4 / 8 / 12 / 16: the register count follows the hyperedges
__global__ __launch_bounds__(HG_THREADS) void hg_logits_kernel(const _Float16* __restrict__ x, int ld_x, const float* __restrict__ Q, float* __restrict__ logits,
                                                               float* __restrict__ pm, float* __restrict__ ps, float* __restrict__ pH, int N, int D, int E,
                                                               float scale) {
    __shared__ __attribute__((aligned(16))) float sq[HG_MAX_E * HG_MAX_D];
    __shared__ __attribute__((aligned(16))) _Float16 sx[HG_SUB * (HG_MAX_D + 8)];
    __shared__ float sl[HG_SUB][HG_MAX_E + 1], sa[HG_SUB][HG_MAX_E + 1];
    __shared__ float srun_m[HG_MAX_E], srun_s[HG_MAX_E], snew_m[HG_MAX_E], sf[HG_MAX_E];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, nt = gridDim.x;
    const int ldx_s = D + 8;   // halves per LDS row: 16-byte rows an odd number of 16-byte slots apart
    const int n0 = t * HG_TILE, n1 = min(n0 + HG_TILE, N);
    for (int i = tid; i < EB * D; i += HG_THREADS) sq[i] = i < E * D ? Q[(size_t)b * E * D + i] : 0.f;   // rows [E, EB): zero, their logits are 0 and never stored
    if (tid < HG_MAX_E) { srun_m[tid] = -INFINITY; srun_s[tid] = 0.f; }
    float acc[EB][2];
#pragma unroll
    for (int e = 0; e < EB; ++e) acc[e][0] = acc[e][1] = 0.f;
    const int n = tid >> 3, sub = tid & 7;
    for (int s0 = n0; s0 < n1; s0 += HG_SUB) {
        const int nv = min(HG_SUB, n1 - s0);
        __syncthreads();   // the previous step's readers of sx / sa are done (and, the first time, sq and the running values are written)
        float l[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) l[e] = 0.f;
        if (n < nv) {
            const _Float16* row = x + ((size_t)b * N + s0 + n) * ld_x;
            for (int c = sub * 8; c < D; c += 64) {
                const half8 v = *reinterpret_cast<const half8*>(row + c);
                *reinterpret_cast<half8*>(sx + n * ldx_s + c) = v;
#pragma unroll
                for (int e = 0; e < EB; ++e) {
                        const floatx4 q0 = *reinterpret_cast<const floatx4*>(sq + e * D + c), q1 = *reinterpret_cast<const floatx4*>(sq + e * D + c + 4);
                        l[e] += (float)v[0] * q0[0] + (float)v[1] * q0[1] + (float)v[2] * q0[2] + (float)v[3] * q0[3] + (float)v[4] * q1[0] +
                                (float)v[5] * q1[1] + (float)v[6] * q1[2] + (float)v[7] * q1[3];
                    }
            }
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) {
                l[e] += __shfl_xor(l[e], 1, 64);
                l[e] += __shfl_xor(l[e], 2, 64);
                l[e] += __shfl_xor(l[e], 4, 64);
            }
        if (sub == 0 && n < nv) {
#pragma unroll
            for (int e = 0; e < EB; ++e) {
                const float v = l[e] * scale;
                sl[n][e] = v;
                if (e < E) logits[((size_t)b * N + s0 + n) * E + e] = v;
            }
        }
        __syncthreads();
        if (tid < EB) {
            float mt = sl[0][tid];
            for (int k = 1; k < nv; ++k) mt = fmaxf(mt, sl[k][tid]);
            const float mo = srun_m[tid], mn = fmaxf(mo, mt);
            snew_m[tid] = mn;
            sf[tid] = expf(mo - mn);   // 0 on the first step (mo = -inf, mn finite)
            srun_m[tid] = mn;
        }
        __syncthreads();
        for (int i = tid; i < nv * EB; i += HG_THREADS) {
            const int k = i / EB, e = i - k * EB;
            sa[k][e] = expf(sl[k][e] - snew_m[e]);
        }
        __syncthreads();
        if (tid < EB) {
            float s = 0.f;
            for (int k = 0; k < nv; ++k) s += sa[k][tid];
            srun_s[tid] = srun_s[tid] * sf[tid] + s;
        }
        if (2 * tid < D) {
#pragma unroll
            for (int e = 0; e < EB; ++e) { acc[e][0] *= sf[e]; acc[e][1] *= sf[e]; }
            for (int k = 0; k < nv; ++k) {
                const _Float16* p = sx + k * ldx_s + 2 * tid;
                const float x0 = (float)p[0], x1 = (float)p[1];
#pragma unroll
                for (int e = 0; e < EB; ++e) {
                        const float a = sa[k][e];
                        acc[e][0] += a * x0;
                        acc[e][1] += a * x1;
                    }
            }
        }
    }
    __syncthreads();
    const size_t part = (size_t)b * nt + t;
    if (tid < E) {
        pm[part * E + tid] = srun_m[tid];
        ps[part * E + tid] = srun_s[tid];
    }
    if (2 * tid < D) {
#pragma unroll
        for (int e = 0; e < EB; ++e)
            if (e < E) {
                float* o = pH + (part * E + e) * D + 2 * tid;
                o[0] = acc[e][0];
                o[1] = acc[e][1];
            }
    }
}

// ---- 5: one hyperedge of one image: M = max_t m_t, S = sum_t s_t exp(m_t - M), He[c] = (sum_t H_t[c] exp(m_t - M)) / S, t ascending
__global__ __launch_bounds__(128) void hg_merge_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pH,
                                                       float* __restrict__ stat, float* __restrict__ He, int nt, int D, int E) {
    const int e = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t p0 = (size_t)b * nt;
    float M = -INFINITY;
    for (int t = 0; t < nt; ++t) M = fmaxf(M, pm[(p0 + t) * E + e]);
    float S = 0.f;
    for (int t = 0; t < nt; ++t) S += ps[(p0 + t) * E + e] * expf(pm[(p0 + t) * E + e] - M);
    if (tid == 0) {
        stat[((size_t)b * E + e) * 2] = M;
        stat[((size_t)b * E + e) * 2 + 1] = S;
    }
    for (int c = tid; c < D; c += 128) {
        float h = 0.f;
        for (int t = 0; t < nt; ++t) h += pH[((p0 + t) * E + e) * D + c] * expf(pm[(p0 + t) * E + e] - M);
        He[((size_t)b * E + e) * D + c] = h / S;
    }
}

// ---- 8: out[n][c] = GELU(sum_e A[n][e] G[e][c] + b_node[c]) + X[n][c] for a 128-node tile, A[n][e] = exp(l[n][e] - M_e) / S_e; G, b_node and the
// tile's A in LDS, a lane takes 8 channels of a node (16 bytes in, 16 bytes out).  Rows beyond N are neither read nor stored.
__global__ __launch_bounds__(HG_THREADS) void hg_node_kernel(const _Float16* __restrict__ x, int ld_x, _Float16* __restrict__ out, int ld_out,
                                                             const float* __restrict__ logits, const float* __restrict__ stat, const float* __restrict__ G,
                                                             const float* __restrict__ b_node, int N, int D, int E) {
    __shared__ __attribute__((aligned(16))) float sg[HG_MAX_E * HG_MAX_D];
    __shared__ __attribute__((aligned(16))) float sb[HG_MAX_D];
    __shared__ float sa[HG_TILE][HG_MAX_E + 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n0 = blockIdx.x * HG_TILE, nv = min(HG_TILE, N - n0);
    for (int i = tid; i < E * D; i += HG_THREADS) sg[i] = G[(size_t)b * E * D + i];
    for (int i = tid; i < D; i += HG_THREADS) sb[i] = b_node[i];
    for (int i = tid; i < nv * E; i += HG_THREADS) {
        const int k = i / E, e = i - k * E;
        const float M = stat[((size_t)b * E + e) * 2], S = stat[((size_t)b * E + e) * 2 + 1];
        sa[k][e] = expf(logits[((size_t)b * N + n0) * E + i] - M) / S;
    }
    __syncthreads();
    const int chunks = D / 8;
    for (int i = tid; i < nv * chunks; i += HG_THREADS) {
        const int k = i / chunks, c = (i - k * chunks) * 8;
        const size_t node = (size_t)b * N + n0 + k;
        const half8 v = *reinterpret_cast<const half8*>(x + node * ld_x + c);
        float o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = 0.f;
#pragma unroll
        for (int e = 0; e < HG_MAX_E; ++e)
            if (e < E) {
                const float a = sa[k][e];
                const floatx4 g0 = *reinterpret_cast<const floatx4*>(sg + e * D + c), g1 = *reinterpret_cast<const floatx4*>(sg + e * D + c + 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) { o[q] += a * g0[q]; o[4 + q] += a * g1[q]; }
            }
        half8 r;
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] = round_to_half(gelu_tanh_ref(o[q] + sb[c + q]) + (float)v[q]);
        *reinterpret_cast<half8*>(out + node * ld_out + c) = r;
    }
}

struct HgLayout {   // float offsets into the workspace; every block starts on 256 bytes
    size_t ctx, P, Q, logits, pm, ps, pH, stat, He, He2, G, total;
    int nt;
};
HgLayout hg_layout(int B, int N, int D, int E) {
    HgLayout L{};
    L.nt = (N + HG_TILE - 1) / HG_TILE;
    size_t at = 0;
    auto take = [&](size_t floats) {
        const size_t o = at;
        at += (floats + 63) / 64 * 64;
        return o;
    };
    const size_t b = (size_t)B, ed = (size_t)E * D;
    L.ctx = take(b * 2 * D);
    L.P = take(b * ed);
    L.Q = take(b * ed);
    L.logits = take(b * N * E);
    L.pm = take(b * L.nt * E);
    L.ps = take(b * L.nt * E);
    L.pH = take(b * L.nt * ed);
    L.stat = take(b * E * 2);
    L.He = take(b * ed);
    L.He2 = take(b * ed);
    L.G = take(b * ed);
    L.total = at;
    return L;
}

}  // namespace

bool hgconv_supported(int D, int E) { return D >= 16 && D % 16 == 0 && D <= HG_MAX_D && E >= 1 && E <= HG_MAX_E; }

size_t hgconv_workspace_bytes(int B, int N, int D, int E) {
    if (!hgconv_supported(D, E) || B < 1 || N < 1) return 0;
    return hg_layout(B, N, D, E).total * sizeof(float);
}

int hgconv_geometry(int32_t* tiles, int max_tiles) {
    const int32_t t[2] = {HG_SUB, HG_TILE};
    for (int i = 0; i < 2 && i < max_tiles; ++i) tiles[i] = t[i];
    return 2;
}

int32_t hgconv_f16(const void* x, int ld_x, void* out, int ld_out, int B, int N, int D, int E, float logit_scale, const HgconvWeights& w, void* workspace,
                   size_t workspace_bytes, hipStream_t s) {
    if (!x || !out || !workspace || !w.w_ctx || !w.b_ctx || !w.proto || !w.w_pre || !w.w_edge || !w.b_edge || !w.w_node || !w.b_node || B < 1 || N < 1 ||
        D < 1 || E < 1 || ld_x < D || ld_out < D)
        return TRTX_ERR_INVALID;
    if (!hgconv_supported(D, E) || B > 65535 || (long)B * N > INT32_MAX) return TRTX_ERR_UNSUPPORTED;
    auto vec16 = [](const void* p, int ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 8 == 0; };
    if (!vec16(x, ld_x) || !vec16(out, ld_out) || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return TRTX_ERR_UNSUPPORTED;
    const HgLayout L = hg_layout(B, N, D, E);
    if (workspace_bytes < L.total * sizeof(float)) return TRTX_ERR_INVALID;
    float* ws = static_cast<float*>(workspace);
    const _Float16* xh = static_cast<const _Float16*>(x);
    const dim3 cols((D + 63) / 64, B), tiles(L.nt, B);
    hipLaunchKernelGGL(hg_colstat_kernel, cols, dim3(HG_THREADS), 0, s, xh, ld_x, ws + L.ctx, N, D);
    const int rows_per_block = HG_THREADS / 64 * HG_PROTO_ROWS;
    hipLaunchKernelGGL(hg_proto_kernel, dim3((E * D + rows_per_block - 1) / rows_per_block), dim3(HG_THREADS), 0, s, ws + L.ctx, w.w_ctx, w.b_ctx, w.proto,
                       ws + L.P, B, D, E);
    hipLaunchKernelGGL(hg_rows_kernel<true>, cols, dim3(64), 0, s, ws + L.P, w.w_pre, static_cast<const float*>(nullptr), ws + L.Q, D, E, (int)ACT_NONE);
    const auto logits_kernel = E <= 4 ? hg_logits_kernel<4> : (E <= 8 ? hg_logits_kernel<8> : (E <= 12 ? hg_logits_kernel<12> : hg_logits_kernel<16>));
    hipLaunchKernelGGL(logits_kernel, tiles, dim3(HG_THREADS), 0, s, xh, ld_x, ws + L.Q, ws + L.logits, ws + L.pm, ws + L.ps, ws + L.pH, N, D, E, logit_scale);
    hipLaunchKernelGGL(hg_merge_kernel, dim3(E, B), dim3(128), 0, s, ws + L.pm, ws + L.ps, ws + L.pH, ws + L.stat, ws + L.He, L.nt, D, E);
    hipLaunchKernelGGL(hg_rows_kernel<false>, cols, dim3(64), 0, s, ws + L.He, w.w_edge, w.b_edge, ws + L.He2, D, E, (int)ACT_GELU_TANH);
    hipLaunchKernelGGL(hg_rows_kernel<false>, cols, dim3(64), 0, s, ws + L.He2, w.w_node, static_cast<const float*>(nullptr), ws + L.G, D, E, (int)ACT_NONE);
    hipLaunchKernelGGL(hg_node_kernel, tiles, dim3(HG_THREADS), 0, s, xh, ld_x, static_cast<_Float16*>(out), ld_out, ws + L.logits, ws + L.stat, ws + L.G,
                       w.b_node, N, D, E);
    return check_launch("hgconv");
}

}  // namespace trtx
