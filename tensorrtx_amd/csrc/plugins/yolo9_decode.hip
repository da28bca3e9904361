// YOLOv9 YoloLayer decode for gfx950 (MI355X) - deterministic two-pass compaction, 38-float records.
//
// Replaces YoloLayerPlugin::forwardGpu + CalDetection of the reference (yolov9/plugin/yololayer.cu:133-197).  The layer has three inputs
// on the strides 8 / 16 / 32, each [batch][4 + classes (+ 32 if is_segmentation)][cells], channel-major, fp32.  Per cell, CalDetection's
// arithmetic:
//   p_c = 1 / (1 + expf(-logit_c)); argmax with strict '>' from (0.0, class 0); dropped if (double)p < 0.1;
//   bbox = [(col + .5 - l) * s, (row + .5 - t) * s, (col + .5 + r) * s, (row + .5 + b) * s]; conf = p; class_id = argmax;
//   with is_segmentation the 32 mask coefficients are copied behind them.
// Records are the Detection of yolov9/include/types.h: bbox[4], conf, class_id, mask[32] = 38 floats (the YOLOv8 layer's are 90).
// As in yolo_decode.hip the reference's atomicAdd slot race is replaced by the canonical (level, cell) order handed out by a prefix
// scan, and out[b][0] is clamped to max_out.  This planar route is what runs behind marked heads, TRTX_YOLO9_HEAD=0 and a user's graph;
// engines use the fused head of yolo9_head.hip.
//
// HBM-bound: pass 1 reads classes x cells x 4 B per image once, one thread per cell, so a wave's load instruction reads 256 consecutive
// bytes of one class plane; pass 2 touches 8 B of scratch per cell and the box planes of the surviving cells.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "decode_common.h"

namespace {

using trtx::find_level;
using trtx::logist;

constexpr int kLevels = 3;
constexpr int kChunk = 512;   // cells per workgroup in both passes
constexpr int kDet9 = 38;     // sizeof(Detection) / 4 (yolov9/include/types.h)

struct Level9Table {
    const float* in[kLevels];
    int cell_off[kLevels + 1];
    int grid_w[kLevels];
    int stride[kLevels];
};

// Pass 1: best class / probability per cell; -1 marks a dropped cell.
__global__ __launch_bounds__(kChunk) void yolo9_score_kernel(Level9Table t, int classes, int info_len, int total_cells, float* __restrict__ score,
                                                             int* __restrict__ cls_out, int* __restrict__ chunk_cnt, int n_chunks) {
    const int b = blockIdx.y;
    const int g = blockIdx.x * kChunk + threadIdx.x;
    int keep = 0;
    if (g < total_cells) {
        const int l = find_level(t.cell_off, kLevels, g);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const float* cur = t.in[l] + (size_t)b * cells * info_len + (g - t.cell_off[l]);
        float best = 0.0f;
        int bcls = 0;
#pragma unroll 4
        for (int c = 0; c < classes; ++c) {
            const float pr = logist(cur[(size_t)(4 + c) * cells]);
            if (pr > best) {
                best = pr;
                bcls = c;
            }
        }
        keep = !((double)best < 0.1) ? 1 : 0;   // "if (max_cls_prob < 0.1) return;", yololayer.cu:156
        score[(size_t)b * total_cells + g] = keep ? best : -1.0f;
        cls_out[(size_t)b * total_cells + g] = bcls;
    }
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int w = trtx::wave_sum(keep);
    trtx::workgroup_count(&s_cnt, (threadIdx.x & 63) == 0 ? w : 0);
    if (threadIdx.x == 0) chunk_cnt[b * n_chunks + blockIdx.x] = s_cnt;
}

// Pass 2: ordered compaction, one thread per cell.
__global__ __launch_bounds__(kChunk) void yolo9_emit_kernel(Level9Table t, int classes, int info_len, int total_cells, int is_seg,
                                                            const float* __restrict__ score, const int* __restrict__ cls_in,
                                                            const int* __restrict__ chunk_cnt, int n_chunks, int max_out, int out_elem,
                                                            float* __restrict__ output) {
    const int b = blockIdx.y;
    const int chunk = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int kWaves = kChunk / 64;
    __shared__ int s_wave[kWaves];
    __shared__ int s_base;
    if (wave == 0) {   // slots used by earlier chunks of this image
        int acc = 0;
        for (int j = lane; j < chunk; j += 64) acc += chunk_cnt[b * n_chunks + j];
        acc = trtx::wave_sum(acc);
        if (lane == 0) s_base = acc;
    }
    const int g = chunk * kChunk + threadIdx.x;
    float sc = -1.0f;
    if (g < total_cells) sc = score[(size_t)b * total_cells + g];
    const bool keep = sc >= 0.0f;
    const unsigned long long m = __ballot(keep);
    const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = s_base;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv)
        if (wv < wave) before += s_wave[wv];
    const int slot = before + in_wave;
    float* out = output + (size_t)b * out_elem;
    if (keep && slot < max_out) {
        const int l = find_level(t.cell_off, kLevels, g);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const int e = g - t.cell_off[l];
        const int gw = t.grid_w[l];
        const int stride = t.stride[l];
        const float* cur = t.in[l] + (size_t)b * cells * info_len + e;
        const int row = e / gw, col = e - row * gw;
        float* det = out + 1 + (size_t)slot * kDet9;
        // yololayer.cu:166-175, operation for operation
        det[0] = (col + 0.5f - cur[0]) * stride;
        det[1] = (row + 0.5f - cur[(size_t)cells]) * stride;
        det[2] = (col + 0.5f + cur[(size_t)2 * cells]) * stride;
        det[3] = (row + 0.5f + cur[(size_t)3 * cells]) * stride;
        det[4] = sc;
        det[5] = (float)cls_in[(size_t)b * total_cells + g];
        if (is_seg)
            for (int k = 0; k < 32; ++k) det[6 + k] = cur[(size_t)(4 + classes + k) * cells];
    }
    if (chunk == n_chunks - 1 && threadIdx.x == kChunk - 1) {   // the last thread of the last chunk sees the full count
        const int total = before + in_wave + (keep ? 1 : 0);
        out[0] = (float)(total < max_out ? total : max_out);
    }
}

size_t cells_of(int net_h, int net_w) {
    size_t c = 0;
    for (int l = 0; l < kLevels; ++l) c += (size_t)(net_h / (8 << l)) * (net_w / (8 << l));   // yololayer.cu:185-186
    return c;
}

}  // namespace

// score and class planes [batch][cells] and one candidate count per 512 cells, each aligned to 256 bytes
extern "C" size_t trtx_yolov9_decode_workspace(int batch, int net_h, int net_w) {
    const size_t cells = cells_of(net_h, net_w);
    const size_t n_chunks = (cells + kChunk - 1) / kChunk;
    return 2 * trtx::align_up((size_t)batch * cells * 4, 256) + trtx::align_up((size_t)batch * n_chunks * sizeof(int), 256);
}

extern "C" int32_t trtx_yolov9_decode(const float* const* inputs, int batch, int classes, int net_h, int net_w, int max_out, int is_segmentation,
                                      float* output, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (batch < 1 || classes < 1 || max_out < 1 || net_h < 32 || net_w < 32 || !inputs || !output || !workspace) return TRTX_ERR_INVALID;
    if (workspace_bytes < trtx_yolov9_decode_workspace(batch, net_h, net_w)) return TRTX_ERR_WORKSPACE;
    Level9Table t{};
    int off = 0;
    for (int l = 0; l < kLevels; ++l) {
        if (!inputs[l]) return TRTX_ERR_INVALID;
        t.in[l] = inputs[l];
        t.cell_off[l] = off;
        t.grid_w[l] = net_w / (8 << l);
        t.stride[l] = 8 << l;
        off += (net_h / (8 << l)) * (net_w / (8 << l));
    }
    t.cell_off[kLevels] = off;
    const int total_cells = off;
    const int n_chunks = (total_cells + kChunk - 1) / kChunk;
    const int info_len = 4 + classes + (is_segmentation ? 32 : 0);
    char* ws = static_cast<char*>(workspace);
    const size_t plane = trtx::align_up((size_t)batch * total_cells * 4, 256);
    float* score = reinterpret_cast<float*>(ws);
    int* cls = reinterpret_cast<int*>(ws + plane);
    int* chunk_cnt = reinterpret_cast<int*>(ws + 2 * plane);
    const int out_elem = 1 + max_out * kDet9;
    const dim3 grid(n_chunks, batch);
    hipLaunchKernelGGL(yolo9_score_kernel, grid, dim3(kChunk), 0, stream, t, classes, info_len, total_cells, score, cls, chunk_cnt, n_chunks);
    hipLaunchKernelGGL(yolo9_emit_kernel, grid, dim3(kChunk), 0, stream, t, classes, info_len, total_cells, is_segmentation ? 1 : 0, score, cls,
                       chunk_cnt, n_chunks, max_out, out_elem, output);
    return trtx::check_launch("trtx_yolov9_decode");
}
