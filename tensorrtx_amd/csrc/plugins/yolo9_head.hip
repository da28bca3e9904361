// Fused DDetect / DualDDetect head (YOLOv9, GELAN) for gfx950 (MI355X): DFL + the YOLOv9 YoloLayer decode on the two NHWC tensors the
// head's last convolutions write - what the engine runs instead of, per level, two NHWC -> fp32 LINEAR conversions, the DFL shuffle /
// softmax / 1x1 convolution / shuffle, the class reshape and the concat scatters (yolov9/src/block.cpp:380-399, 441-453), followed by the
// plugin's two passes (yolov9/plugin/yololayer.cu:133-197; plugins/yolo9_decode.hip).
//
// box[l]: [batch][cells_l][box_ld], channels [0, 64) = 4 sides x 16 DFL bins: the output of the grouped 1x1 convolution cv2.l.2.
// cls[l]: [batch][cells_l][cls_ld], channels [0, classes) = class logits: the output of cv3.l.2.
// T = _Float16 (fp16 engines) or float (fp32 engines).  Channels beyond those are padding that holds whatever the convolutions wrote:
// the 16-byte pieces cover [0, classes & ~7) only and the last classes % 8 logits are read one element at a time, so no padding value
// reaches a maximum, a sigmoid or a load past the tensor's last pixel.
//
// Per cell: DFL = softmax over the 16 bins with the maximum subtracted, then the expectation with dfl_weights, in fp32 - head_score's
// arithmetic of yolo_decode.hip for fp16 engines and its to-the-bit form of the un-fused chain (softmax_kernel, then the fmaf chain of
// the direct 1x1 convolution) for fp32 engines; then CalDetection's class scan: sigmoid, strict '>' argmax from (0.0, class 0), dropped
// when (double)p < 0.1, corner box from the four sides.  Records (38 floats), canonical (level, cell) order and the clamped count are
// those of trtx_yolov9_decode.
//
// Mapping, and what a wave reads per instruction.  The kernel's time is the class logits: 160 B per cell for 80 fp16 classes, against
// 128 B of box bins that only survivors need.  A cell's class row is contiguous, so the logits are read by the WAVE, not by the cell's
// own thread: the 64 cells of a wave are classes / 8 16-byte pieces each, and consecutive lanes take consecutive pieces, so one load
// instruction reads 1 KiB that lies in 64 * 16 / (2 cls_ld) consecutive rows - 1 KiB contiguous when cls_ld = classes, ~7 rows of 160 B
// for 80 classes - instead of 64 rows 160 B apart (one 16-byte piece of each of 64 cache lines, the one-thread-per-cell mapping).
// That pass only takes the packed maximum of the raw logits: a cell can survive only if some sigmoid(logit) >= 0.1, i.e. some logit
// >= -2.1972, so `max > -2.3` (no exp) settles every cell that cannot pass: most cells where a model keeps few candidates (an expectation
// for trained weights, not a measurement; the synthetic ones keep 4 - 36 %).  The possible survivors are compacted into an LDS
// list and the exact pass - 16-byte loads of the cell's own class row and of its 64 box bins - runs on dense lanes.  The box row is
// read for those cells only.  Pass 2 is the one-thread-per-cell ordered compaction of the plugin kernels on 8 B of scratch per cell.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "decode_common.h"

namespace {

using trtx::find_level;
using trtx::logist;

constexpr int kLevels = 3;
constexpr int kChunk = 512;   // cells per chunk counter and per emit workgroup
constexpr int kBlock = 256;   // cells per score workgroup: divides kChunk, so a workgroup feeds one chunk counter
constexpr int kDet9 = 38;     // sizeof(Detection) / 4 (yolov9/include/types.h): bbox[4], conf, class_id, mask[32]

struct Head9Table {
    const void* box[kLevels];
    const void* cls[kLevels];
    int box_ld[kLevels], cls_ld[kLevels];
    int cell_off[kLevels + 1];
    int grid_w[kLevels];
    int stride[kLevels];
};

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

// eight consecutive channels of a cell as floats: one 16-byte load of an fp16 engine's tensor, two of an fp32 engine's
template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&x)[8]) {
    if constexpr (sizeof(T) == 2) {
        const half8_t v = *reinterpret_cast<const half8_t*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (float)v[i];
    } else {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
        x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    }
}

// Pass 1: best class / probability and the four DFL distances of every cell that can survive; -1 marks a dropped cell.
template <typename T>
__global__ __launch_bounds__(kBlock) void yolo9_head_score_kernel(Head9Table t, int classes, int total_cells, const float* __restrict__ dfl_w,
                                                                  float* __restrict__ score, int* __restrict__ cls_out, float4* __restrict__ boxes,
                                                                  int* __restrict__ chunk_cnt, int n_chunks) {
    __shared__ int s_list[kBlock];
    __shared__ int s_n, s_keep;
    const int b = blockIdx.y;
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (threadIdx.x == 0) {
        s_n = 0;
        s_keep = 0;
    }
    s_list[threadIdx.x] = 0;   // phase 1 borrows the list as the per-cell flags (same-value races only)
    __syncthreads();
    const int full = classes & ~7;   // classes read eight at a time; [full, classes) one at a time
    auto cls_ptr = [&](int gg) {
        const int l = find_level(t.cell_off, kLevels, gg);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        return static_cast<const T*>(t.cls[l]) + ((size_t)b * cells + (gg - t.cell_off[l])) * t.cls_ld[l];
    };
    // ---- phase 1, every cell: the packed maximum of the raw logits, read in 16-byte pieces by the wave (file header).  A piece whose
    // maximum passes raises its cell's flag; NaN logits do not (fmaxf drops them), exactly like NaN fails 'pr > best' in the scan.
    {
        const int wave0 = threadIdx.x & ~63, lane = threadIdx.x & 63;
        const int pieces = (classes + 7) >> 3;
        const int g0 = blockIdx.x * kBlock + wave0;
        int cells_here = total_cells - g0;
        cells_here = cells_here > 64 ? 64 : cells_here;
        const int n = cells_here * pieces;   // <= 0 for a wave behind the last cell
        for (int j = lane; j < n; j += 64) {
            const int c = j / pieces, q = j - c * pieces;
            const T* p = cls_ptr(g0 + c) + q * 8;
            float m = -INFINITY;
            if (q * 8 < full) {
                float v[8];
                load8(p, v);
                m = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
            } else {
                for (int i = 0; i < classes - full; ++i) m = fmaxf(m, (float)p[i]);
            }
            if (m > -2.3f) s_list[wave0 + c] = 1;
        }
    }
    __syncthreads();
    bool maybe = false;
    if (g < total_cells) {
        maybe = s_list[threadIdx.x] != 0;
        if (!maybe) {
            const size_t o = (size_t)b * total_cells + g;
            score[o] = -1.0f;
            cls_out[o] = 0;
        }
    }
    __syncthreads();   // the flags are read; the list proper is written next
    {
        const unsigned long long m = __ballot(maybe);
        int base = 0;
        if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(&s_n, __popcll(m));
        base = __shfl(base, 0);
        if (maybe) s_list[base + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull))] = threadIdx.x;
    }
    __syncthreads();
    // ---- phase 2, possible survivors only: the reference arithmetic, so kept candidates are bit-identical to evaluating every cell.
    // The order of the list (waves race for its segments) decides only which thread takes which cell.
    int kept = 0;
    for (int k = threadIdx.x; k < s_n; k += kBlock) {
        const int gg = blockIdx.x * kBlock + s_list[k];
        const int l = find_level(t.cell_off, kLevels, gg);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const size_t pix = (size_t)b * cells + (gg - t.cell_off[l]);
        const T* bx = static_cast<const T*>(t.box[l]) + pix * t.box_ld[l];
        const T* cl = static_cast<const T*>(t.cls[l]) + pix * t.cls_ld[l];
        float best = 0.0f;
        int bcls = 0;
        for (int c0 = 0; c0 < full; c0 += 8) {
            float v[8];
            load8(cl + c0, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float pr = logist(v[i]);
                if (pr > best) {
                    best = pr;
                    bcls = c0 + i;
                }
            }
        }
        for (int c = full; c < classes; ++c) {
            const float pr = logist((float)cl[c]);
            if (pr > best) {
                best = pr;
                bcls = c;
            }
        }
        const bool keep = !((double)best < 0.1);   // "if (max_cls_prob < 0.1) return;", yololayer.cu:156
        const size_t o = (size_t)b * total_cells + gg;
        score[o] = keep ? best : -1.0f;
        cls_out[o] = bcls;
        if (!keep) continue;   // the box row is read for survivors only
        ++kept;
        float w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = dfl_w[i];
        float side[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float lo[8], hi[8], x[16];
            load8(bx + s * 16, lo);
            load8(bx + s * 16 + 8, hi);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                x[i] = lo[i];
                x[8 + i] = hi[i];
            }
            float mx = x[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, x[i]);
            float sum = 0.f, acc = 0.f;
            if constexpr (sizeof(T) == 4) {
                // fp32 engines: the un-fused chain to the bit - softmax_kernel (p_i = expf(x_i - max) * (1 / sum)), then the direct 1x1
                // convolution's fmaf chain over the 16 bins from 0 (yolo_decode.hip, head_score)
                float ex[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    ex[i] = expf(x[i] - mx);
                    sum += ex[i];
                }
                const float inv = 1.0f / sum;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc = fmaf(ex[i] * inv, w[i], acc);
                side[s] = acc;
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float ex = expf(x[i] - mx);
                    sum += ex;
                    acc = fmaf(ex, w[i], acc);
                }
                side[s] = acc / sum;
            }
        }
        boxes[o] = make_float4(side[0], side[1], side[2], side[3]);
    }
    // per-kChunk candidate counts (two workgroups feed one chunk counter)
    trtx::workgroup_count(&s_keep, kept);
    if (threadIdx.x == 0 && s_keep) atomicAdd(&chunk_cnt[b * n_chunks + (blockIdx.x * kBlock) / kChunk], s_keep);
}

// Pass 2: ordered compaction, one thread per cell; the distances come from pass 1.
__global__ __launch_bounds__(kChunk) void yolo9_head_emit_kernel(Head9Table t, int total_cells, const float* __restrict__ score,
                                                                 const int* __restrict__ cls_in, const float4* __restrict__ boxes,
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
        const int e = g - t.cell_off[l];
        const int gw = t.grid_w[l];
        const int stride = t.stride[l];
        const float4 d = boxes[(size_t)b * total_cells + g];
        const int row = e / gw, col = e - row * gw;
        float* det = out + 1 + (size_t)slot * kDet9;
        // yololayer.cu:166-171, operation for operation
        det[0] = (col + 0.5f - d.x) * stride;
        det[1] = (row + 0.5f - d.y) * stride;
        det[2] = (col + 0.5f + d.z) * stride;
        det[3] = (row + 0.5f + d.w) * stride;
        det[4] = sc;
        det[5] = (float)cls_in[(size_t)b * total_cells + g];
    }
    if (chunk == n_chunks - 1 && threadIdx.x == kChunk - 1) {   // the last thread of the last chunk sees the full count
        const int total = before + in_wave + (keep ? 1 : 0);
        out[0] = (float)(total < max_out ? total : max_out);
    }
}

// score | cls | boxes | chunk_cnt, each aligned to 256 bytes; a null base gives the size
struct Workspace9 {
    float* score;
    int* cls;
    float4* boxes;
    int* chunk_cnt;
    int n_chunks;
    size_t bytes;
};

Workspace9 carve(void* base, int batch, size_t cells) {
    Workspace9 w{};
    w.n_chunks = (int)((cells + kChunk - 1) / kChunk);
    const auto take = [&](size_t bytes) {
        void* p = base ? static_cast<char*>(base) + w.bytes : nullptr;
        w.bytes += trtx::align_up(bytes, 256);
        return p;
    };
    w.score = static_cast<float*>(take((size_t)batch * cells * sizeof(float)));
    w.cls = static_cast<int*>(take((size_t)batch * cells * sizeof(int)));
    w.boxes = static_cast<float4*>(take((size_t)batch * cells * sizeof(float4)));
    w.chunk_cnt = static_cast<int*>(take((size_t)batch * w.n_chunks * sizeof(int)));
    return w;
}

size_t cells_of(int net_h, int net_w) {
    size_t c = 0;
    for (int l = 0; l < kLevels; ++l) c += (size_t)(net_h / (8 << l)) * (net_w / (8 << l));   // yololayer.cu:185-186
    return c;
}

int32_t head9_decode(const void* const* box, const int* box_ld, const void* const* cls, const int* cls_ld, int elem_bytes, int batch, int classes,
                     int net_h, int net_w, const float* dfl_weights, int max_out, float* output, void* workspace, size_t workspace_bytes,
                     hipStream_t stream) {
    if (batch < 1 || classes < 1 || max_out < 1 || net_h < 32 || net_w < 32 || !box || !box_ld || !cls || !cls_ld || !dfl_weights || !output ||
        !workspace)
        return TRTX_ERR_INVALID;
    for (int l = 0; l < kLevels; ++l)
        if (!box[l] || !cls[l]) return TRTX_ERR_INVALID;
    const int vec = 16 / elem_bytes;
    for (int l = 0; l < kLevels; ++l)
        if (box_ld[l] < 64 || cls_ld[l] < classes || box_ld[l] % vec || cls_ld[l] % vec || (reinterpret_cast<uintptr_t>(box[l]) & 15) ||
            (reinterpret_cast<uintptr_t>(cls[l]) & 15))
            return TRTX_ERR_UNSUPPORTED;
    if (workspace_bytes < trtx_yolov9_head_decode_workspace(batch, net_h, net_w)) return TRTX_ERR_WORKSPACE;
    Head9Table t{};
    int off = 0;
    for (int l = 0; l < kLevels; ++l) {
        t.box[l] = box[l];
        t.cls[l] = cls[l];
        t.box_ld[l] = box_ld[l];
        t.cls_ld[l] = cls_ld[l];
        t.cell_off[l] = off;
        t.grid_w[l] = net_w / (8 << l);
        t.stride[l] = 8 << l;
        off += (net_h / (8 << l)) * (net_w / (8 << l));
    }
    t.cell_off[kLevels] = off;
    const int total_cells = off;
    const Workspace9 w = carve(workspace, batch, total_cells);
    if (hipMemsetAsync(w.chunk_cnt, 0, (size_t)batch * w.n_chunks * sizeof(int), stream) != hipSuccess) return TRTX_ERR_HIP;
    const int out_elem = 1 + max_out * kDet9;
    const dim3 sgrid((total_cells + kBlock - 1) / kBlock, batch), egrid(w.n_chunks, batch);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(yolo9_head_score_kernel<_Float16>, sgrid, dim3(kBlock), 0, stream, t, classes, total_cells, dfl_weights, w.score, w.cls,
                           w.boxes, w.chunk_cnt, w.n_chunks);
    else
        hipLaunchKernelGGL(yolo9_head_score_kernel<float>, sgrid, dim3(kBlock), 0, stream, t, classes, total_cells, dfl_weights, w.score, w.cls,
                           w.boxes, w.chunk_cnt, w.n_chunks);
    hipLaunchKernelGGL(yolo9_head_emit_kernel, egrid, dim3(kChunk), 0, stream, t, total_cells, w.score, w.cls, (const float4*)w.boxes, w.chunk_cnt,
                       w.n_chunks, max_out, out_elem, output);
    return trtx::check_launch("trtx_yolov9_head_decode_nhwc");
}

}  // namespace

extern "C" size_t trtx_yolov9_head_decode_workspace(int batch, int net_h, int net_w) {
    return carve(nullptr, batch, cells_of(net_h, net_w)).bytes;
}

extern "C" int32_t trtx_yolov9_head_decode_nhwc(const void* const* box, const int* box_ld, const void* const* cls, const int* cls_ld, int batch,
                                                int classes, int net_h, int net_w, const float* dfl_weights, int max_out, float* output,
                                                void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head9_decode(box, box_ld, cls, cls_ld, 2, batch, classes, net_h, net_w, dfl_weights, max_out, output, workspace, workspace_bytes, stream);
}

extern "C" int32_t trtx_yolov9_head_decode_nhwc_f32(const void* const* box, const int* box_ld, const void* const* cls, const int* cls_ld, int batch,
                                                    int classes, int net_h, int net_w, const float* dfl_weights, int max_out, float* output,
                                                    void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head9_decode(box, box_ld, cls, cls_ld, 4, batch, classes, net_h, net_w, dfl_weights, max_out, output, workspace, workspace_bytes, stream);
}
