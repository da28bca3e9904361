// Anchor-based YoloLayer decode (YOLOv5 / v7 / v3-v4 family) for gfx950 (MI355X) — deterministic two-pass compaction.
//
// Replaces YoloLayerPlugin::forwardGpu + CalDetection of the reference (yolov5/plugin/yololayer.cu:161-227,
// yolov7/plugin/yololayer.cu:152-207: the same arithmetic).  Per grid cell and per anchor k of a level (input
// [batch][3 * (5 + classes (+32))][cells], channel-major):
//   box_prob = sigmoid(obj); dropped if box_prob < kIgnoreThresh (0.1f, yolov5/src/config.h:38);
//   class scan: p = sigmoid(logit_c), strict '>' from (0.0, class 0);
//   bbox = [(col - 0.5 + 2 sigma(x)) * netW / gridW, (row - 0.5 + 2 sigma(y)) * netH / gridH,
//           (2 sigma(w))^2 * anchor_w, (2 sigma(h))^2 * anchor_h]           (centre format)
//   conf = box_prob * max class prob; class_id; 32 mask coefficients copied when is_segmentation (YOLOv5 only).
// What differs between the families is the record, a Detection struct of kDet floats: 38 for YOLOv5 (bbox[4], conf, class_id, mask[32],
// yolov5/src/types.h:11-16) and 6 for YOLOv7 (bbox[4], conf, class_id, yolov7/include/types.h; no mask branch).
// As in yolo_decode.hip the reference's atomicAdd slot race is replaced by a canonical order — (level, cell, anchor)
// ascending, handed out by a prefix scan — and out[b][0] is clamped to max_out.  Nothing of a row is written behind its records.
//
// The Darknet form (YOLOv3 / YOLOv3-tiny / YOLOv4, yolov4/yololayer.cu:154-199, equal in the other two) is a third record, kDet = 7:
// bbox[4], det_confidence, class_id, class_confidence (yolov4/yololayer.h:41-47), and other arithmetic in front of the same compaction:
//   Logist(x) = 1./(1. + exp(-x)): a float exp, the add and the divide in double, rounded to float;
//   dropped if max_cls_prob < 0.1f || box_prob < 0.1f (two gates; a NaN objectness passes, max_cls_prob is never NaN);
//   bbox = [(col + Logist(x)) * netW / gridW, (row + Logist(y)) * netH / gridH, exp(w) * anchor_w, exp(h) * anchor_h];
//   det_confidence = box_prob, class_confidence = max_cls_prob: no product.
// The reference scans the classes of every anchor and tests both gates after; here the objectness gate comes first and spares the scan,
// which keeps the same anchors.  Pass 1 leaves max_cls_prob (>= 0.1 where kept) in the score plane; pass 2 takes box_prob from the input again.
//
// Both passes are templates on kDet.  The 38-float kernels take two more int arguments than the 6-float ones, info_len and
// is_segmentation, each at the place it has always had in the argument list; the pack Seg (one int, or empty) spells that, and with it
// both instantiations keep the instruction streams of the kernels they replace (profiles/anchor_units_isa.txt).
//
// HBM-bound: pass 1 reads the objectness plane of every anchor (12 B per cell) and the class planes of the few cells that pass;
// pass 2 touches only survivors.  One thread per cell in both passes (coalesced along the cell axis), three anchors each.  A record
// starts at float 1 + kDet * slot: 4-byte aligned only, so it is written with float stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "decode_common.h"

namespace {

using trtx::logist;
using trtx::logist_darknet;

constexpr int kMaxLevels = 8;
constexpr int kAnchors = 3;   // kNumAnchor, yolov5/src/config.h:35 and yolov7/include/config.h
constexpr int kChunk = 512;   // cells per workgroup

struct LevelTable {
    const float* in[kMaxLevels];
    int cell_off[kMaxLevels + 1];
    int grid_w[kMaxLevels], grid_h[kMaxLevels];
    float anchors[kMaxLevels][kAnchors * 2];
    int n_levels;
};

// Pass 1: conf / class of every (cell, anchor); -1 marks a dropped candidate.  score / cls: [batch][cells][3].
// seg_len: info_len where the record has the mask coefficients (5 + classes, + 32 in a segmentation head), nothing where it has not.
template <int kDet, typename... Seg>
__global__ __launch_bounds__(kChunk) void anchor_score_kernel(LevelTable t, int classes, Seg... seg_len, int total_cells,
                                                              float* __restrict__ score, int* __restrict__ cls_out,
                                                              int* __restrict__ chunk_cnt, int n_chunks) {
    static_assert(sizeof...(Seg) == (kDet == 38 ? 1 : 0) && (kDet == 38 || kDet == 6 || kDet == 7));
    const int info_len = sizeof...(Seg) ? (0 + ... + seg_len) : 5 + classes;
    const int b = blockIdx.y;
    const int g = blockIdx.x * kChunk + threadIdx.x;
    int nkeep = 0;
    if (g < total_cells) {
        const int l = trtx::find_level(t.cell_off, t.n_levels, g);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const int e = g - t.cell_off[l];
        const float* cur = t.in[l] + (size_t)b * info_len * cells * kAnchors + e;
#pragma unroll
        for (int k = 0; k < kAnchors; ++k) {
            const float* a = cur + (size_t)k * info_len * cells;
            float conf = -1.0f;
            int best_c = 0;
            if constexpr (kDet == 7) {
                const float box_prob = logist_darknet(a[(size_t)4 * cells]);
                if (!(box_prob < 0.1f)) {  // "|| box_prob < IGNORE_THRESH": NaN is kept, as there
                    float best = 0.0f;
                    for (int c = 0; c < classes; ++c) {
                        const float p = logist_darknet(a[(size_t)(5 + c) * cells]);
                        if (p > best) {
                            best = p;
                            best_c = c;
                        }
                    }
                    if (!(best < 0.1f)) {  // "max_cls_prob < IGNORE_THRESH ||": best is in [0.1, 1] here, never NaN
                        conf = best;
                        ++nkeep;
                    }
                }
            } else if (const float box_prob = logist(a[(size_t)4 * cells]); !(box_prob < 0.1f)) {  // "if (box_prob < kIgnoreThresh) continue;": NaN is kept, as there
                float best = 0.0f;
                for (int c = 0; c < classes; ++c) {
                    const float p = logist(a[(size_t)(5 + c) * cells]);
                    if (p > best) {
                        best = p;
                        best_c = c;
                    }
                }
                conf = box_prob * best;
                // conf >= 0 marks "kept" below; a NaN product (NaN logits) must stay a kept record as in the reference
                if (!(conf >= 0.0f)) conf = __builtin_nanf("");
                ++nkeep;
            }
            const size_t o = ((size_t)b * total_cells + g) * kAnchors + k;
            score[o] = conf;
            cls_out[o] = best_c;
        }
    }
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int w = trtx::wave_sum(nkeep);
    trtx::workgroup_count(&s_cnt, (threadIdx.x & 63) == 0 ? w : 0);
    if (threadIdx.x == 0) chunk_cnt[b * n_chunks + blockIdx.x] = s_cnt;
}

// Pass 2: ordered compaction, one thread per cell (0..3 records each).  is_seg: as seg_len, is_segmentation or nothing.
template <int kDet, typename... Seg>
__global__ __launch_bounds__(kChunk) void anchor_emit_kernel(LevelTable t, int classes, Seg... seg_len, int total_cells, int net_w, int net_h,
                                                             Seg... is_seg, const float* __restrict__ score, const int* __restrict__ cls_in,
                                                             const int* __restrict__ chunk_cnt, int n_chunks, int max_out, int out_elem,
                                                             float* __restrict__ output) {
    static_assert(sizeof...(Seg) == (kDet == 38 ? 1 : 0) && (kDet == 38 || kDet == 6 || kDet == 7));
    const int info_len = sizeof...(Seg) ? (0 + ... + seg_len) : 5 + classes;
    const int b = blockIdx.y;
    const int chunk = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int kWaves = kChunk / 64;
    __shared__ int s_wave[kWaves];
    __shared__ int s_base;
    if (wave == 0) {
        int acc = 0;
        for (int j = lane; j < chunk; j += 64) acc += chunk_cnt[b * n_chunks + j];
        acc = trtx::wave_sum(acc);
        if (lane == 0) s_base = acc;
    }
    const int g = chunk * kChunk + threadIdx.x;
    float sc[kAnchors] = {-1.0f, -1.0f, -1.0f};
    int mine = 0;
    if (g < total_cells) {
#pragma unroll
        for (int k = 0; k < kAnchors; ++k) {
            sc[k] = score[((size_t)b * total_cells + g) * kAnchors + k];
            mine += (sc[k] >= 0.0f || sc[k] != sc[k]) ? 1 : 0;  // kept: conf >= 0 or NaN
        }
    }
    // exclusive prefix of `mine` (records, not floats) inside the wave
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int slot = s_base + incl - mine;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv)
        if (wv < wave) slot += s_wave[wv];
    float* out = output + (size_t)b * out_elem;
    if (mine) {
        const int l = trtx::find_level(t.cell_off, t.n_levels, g);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const int e = g - t.cell_off[l];
        const int gw = t.grid_w[l], gh = t.grid_h[l];
        const int row = e / gw, col = e - row * gw;
        const float* cur = t.in[l] + (size_t)b * info_len * cells * kAnchors + e;
#pragma unroll
        for (int k = 0; k < kAnchors; ++k) {
            if (!(sc[k] >= 0.0f || sc[k] != sc[k])) continue;
            if (slot < max_out) {
                const float* a = cur + (size_t)k * info_len * cells;
                float* det = out + 1 + (size_t)slot * kDet;
                if constexpr (kDet == 7) {
                    // yolov4 yololayer.cu:187-197, operation for operation
                    det[0] = (col + logist_darknet(a[0])) * net_w / gw;
                    det[1] = (row + logist_darknet(a[(size_t)cells])) * net_h / gh;
                    det[2] = expf(a[(size_t)2 * cells]) * t.anchors[l][2 * k];
                    det[3] = expf(a[(size_t)3 * cells]) * t.anchors[l][2 * k + 1];
                    det[4] = logist_darknet(a[(size_t)4 * cells]);
                    det[5] = (float)cls_in[((size_t)b * total_cells + g) * kAnchors + k];
                    det[6] = sc[k];
                } else {
                    // yolov5 yololayer.cu:199-206, yolov7 yololayer.cu:196-203, operation for operation
                    det[0] = (col - 0.5f + 2.0f * logist(a[0])) * net_w / gw;
                    det[1] = (row - 0.5f + 2.0f * logist(a[(size_t)cells])) * net_h / gh;
                    float bw = 2.0f * logist(a[(size_t)2 * cells]);
                    bw = bw * bw * t.anchors[l][2 * k];
                    float bh = 2.0f * logist(a[(size_t)3 * cells]);
                    bh = bh * bh * t.anchors[l][2 * k + 1];
                    det[2] = bw;
                    det[3] = bh;
                    det[4] = sc[k];
                    det[5] = (float)cls_in[((size_t)b * total_cells + g) * kAnchors + k];
                    if constexpr (kDet == 6 + 32) {   // only a record with room for them takes the mask coefficients
                        if ((0 + ... + is_seg))
                            for (int i = 0; i < 32; ++i) det[6 + i] = a[(size_t)(5 + classes + i) * cells];
                    }
                }
            }
            ++slot;
        }
    }
    if (chunk == n_chunks - 1 && threadIdx.x == kChunk - 1) {
        int total = s_base;
        for (int wv = 0; wv < kWaves; ++wv) total += s_wave[wv];
        out[0] = (float)(total < max_out ? total : max_out);
    }
}

// score / class planes [batch][cells][3] and one candidate count per 512 cells; 0 for arguments the decode refuses
size_t anchor_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    if (batch < 1 || !grid_w || !grid_h || n_levels < 1 || n_levels > kMaxLevels) return 0;
    size_t cells = 0;
    for (int i = 0; i < n_levels; ++i) cells += (size_t)grid_w[i] * grid_h[i];
    const size_t n_chunks = (cells + kChunk - 1) / kChunk;
    return 2 * trtx::align_up((size_t)batch * cells * kAnchors * 4, 256) + trtx::align_up((size_t)batch * n_chunks * sizeof(int), 256);
}

// kDet 38 with is_segmentation as passed, or kDet 6 or 7 with is_segmentation 0
template <int kDet>
int32_t anchor_decode(const char* entry, const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                      const int* grid_w, const int* grid_h, const float* anchors, int max_out, int is_segmentation, float* output,
                      void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (n_levels < 1 || n_levels > kMaxLevels || batch < 1 || classes < 1 || max_out < 1 || !inputs || !grid_w || !grid_h || !anchors ||
        !output || !workspace)
        return TRTX_ERR_INVALID;
    // every refusal comes before the first write to the workspace
    for (int i = 0; i < n_levels; ++i)
        if (grid_w[i] < 1 || grid_h[i] < 1 || !inputs[i]) return TRTX_ERR_INVALID;
    if (workspace_bytes < anchor_workspace(batch, grid_w, grid_h, n_levels)) return TRTX_ERR_WORKSPACE;
    LevelTable t{};
    t.n_levels = n_levels;
    int off = 0;
    for (int i = 0; i < n_levels; ++i) {
        t.in[i] = inputs[i];
        t.cell_off[i] = off;
        t.grid_w[i] = grid_w[i];
        t.grid_h[i] = grid_h[i];
        for (int k = 0; k < kAnchors * 2; ++k) t.anchors[i][k] = anchors[i * kAnchors * 2 + k];
        off += grid_w[i] * grid_h[i];
    }
    for (int i = n_levels; i <= kMaxLevels; ++i) t.cell_off[i] = off;
    const int total_cells = off;
    const int n_chunks = (total_cells + kChunk - 1) / kChunk;
    char* ws = static_cast<char*>(workspace);
    const size_t plane = trtx::align_up((size_t)batch * total_cells * kAnchors * 4, 256);
    float* score = reinterpret_cast<float*>(ws);
    int* cls = reinterpret_cast<int*>(ws + plane);
    int* chunk_cnt = reinterpret_cast<int*>(ws + 2 * plane);
    const int out_elem = 1 + max_out * kDet;
    const dim3 grid(n_chunks, batch);
    if constexpr (kDet == 38) {
        const int info_len = 5 + classes + (is_segmentation ? 32 : 0);
        hipLaunchKernelGGL((anchor_score_kernel<38, int>), grid, dim3(kChunk), 0, stream, t, classes, info_len, total_cells, score, cls, chunk_cnt,
                           n_chunks);
        hipLaunchKernelGGL((anchor_emit_kernel<38, int>), grid, dim3(kChunk), 0, stream, t, classes, info_len, total_cells, net_w, net_h, is_segmentation,
                           score, cls, chunk_cnt, n_chunks, max_out, out_elem, output);
    } else {
        hipLaunchKernelGGL(anchor_score_kernel<kDet>, grid, dim3(kChunk), 0, stream, t, classes, total_cells, score, cls, chunk_cnt, n_chunks);
        hipLaunchKernelGGL(anchor_emit_kernel<kDet>, grid, dim3(kChunk), 0, stream, t, classes, total_cells, net_w, net_h, score, cls, chunk_cnt,
                           n_chunks, max_out, out_elem, output);
    }
    return trtx::check_launch(entry);
}

}  // namespace

extern "C" size_t trtx_yolov5_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    return anchor_workspace(batch, grid_w, grid_h, n_levels);
}

extern "C" size_t trtx_yolov7_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    return anchor_workspace(batch, grid_w, grid_h, n_levels);
}

extern "C" size_t trtx_darknet_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    return anchor_workspace(batch, grid_w, grid_h, n_levels);
}

extern "C" int32_t trtx_yolov5_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                                      const int* grid_w, const int* grid_h, const float* anchors, int max_out, int is_segmentation,
                                      float* output, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return anchor_decode<38>("trtx_yolov5_decode", inputs, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out,
                             is_segmentation, output, workspace, workspace_bytes, stream);
}

extern "C" int32_t trtx_yolov7_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                                      const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                      void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return anchor_decode<6>("trtx_yolov7_decode", inputs, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, 0, output,
                            workspace, workspace_bytes, stream);
}

extern "C" int32_t trtx_darknet_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                                       const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                       void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return anchor_decode<7>("trtx_darknet_decode", inputs, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, 0, output,
                            workspace, workspace_bytes, stream);
}
