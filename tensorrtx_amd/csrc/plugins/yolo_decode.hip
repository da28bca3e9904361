// YOLOv8 anchor-free decode for gfx950 (MI355X) — deterministic two-pass compaction.
//
// Replaces YoloLayerPlugin::forwardGpu + CalDetection of the reference
// (yolov8/plugin/yololayer.cu:178-220, 282-316).  Same arithmetic per cell:
//   p_c = 1/(1+expf(-logit_c)); argmax with strict '>' from (0.0, class 0); drop if p < 0.1;
//   bbox = [(col+.5-l)*s, (row+.5-t)*s, (col+.5+r)*s, (row+.5+b)*s]; conf = p; class_id = argmax.
// Differences (both documented in DESIGN.md):
//   * slots are handed out in canonical (level, cell) order by a prefix scan instead of atomicAdd,
//     so the output is bit-reproducible (the reference's slot order is a race);
//   * out[b][0] is clamped to max_out (the reference lets the counter run past the buffer).
//
// HBM-bound: reads (4+classes) x cells x 4 B per image once (pass 1, 16 B per lane, coalesced along
// the cell axis), then 8 B/cell of scratch + the 4 box channels of the surviving cells (pass 2).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "decode_common.h"

namespace {

using trtx::find_level;
using trtx::logist;

constexpr int kMaxLevels = 8;
constexpr int kChunk = 512;  // cells per workgroup in both passes

// which optional branches of the YOLOv8 Detection record are decoded (yololayer.cu:222-279)
struct YoloBranches {
    int seg, pose, obb, nk;
    float kpt_conf;
};

struct LevelTable {
    const float* in[kMaxLevels];  // device pointers, [batch][4+classes][cells]
    int cell_off[kMaxLevels + 1];  // cumulative cell offsets
    int grid_w[kMaxLevels];
    int stride[kMaxLevels];
    int n_levels;
};

// Pass 1: per cell best class/prob.  VEC cells per thread (VEC = 4 -> 16-byte loads).
template <int VEC>
__global__ __launch_bounds__(kChunk / VEC) void yolo_score_kernel(LevelTable t, int classes, int info_len, int total_cells,
                                                                  float* __restrict__ score,
                                                                  int* __restrict__ cls_out,
                                                                  int* __restrict__ chunk_cnt, int n_chunks) {
    const int b = blockIdx.y;
    const int chunk = blockIdx.x;
    const int g0 = chunk * kChunk + threadIdx.x * VEC;
    int nflag = 0;
    if (g0 < total_cells) {
        const int l = find_level(t.cell_off, t.n_levels, g0);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const int e0 = g0 - t.cell_off[l];
        const float* cur = t.in[l] + (size_t)b * cells * info_len + e0;
        float best[VEC];
        int bcls[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            best[v] = 0.0f;
            bcls[v] = 0;
        }
#pragma unroll 4
        for (int c = 0; c < classes; ++c) {
            float x[VEC];
            const float* p = cur + (size_t)(4 + c) * cells;
            if constexpr (VEC == 4) {
                const float4 q = *reinterpret_cast<const float4*>(p);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) x[v] = p[v];
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float pr = logist(x[v]);
                if (pr > best[v]) {
                    best[v] = pr;
                    bcls[v] = c;
                }
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int g = g0 + v;
            if (g < total_cells) {
                const bool keep = !((double)best[v] < 0.1);  // same comparison as yololayer.cu:203
                score[(size_t)b * total_cells + g] = keep ? best[v] : -1.0f;
                cls_out[(size_t)b * total_cells + g] = bcls[v];
                nflag += keep ? 1 : 0;
            }
        }
    }
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int w = trtx::wave_sum(nflag);
    trtx::workgroup_count(&s_cnt, (threadIdx.x & 63) == 0 ? w : 0);
    if (threadIdx.x == 0) chunk_cnt[b * n_chunks + chunk] = s_cnt;
}

// Pass 2: ordered compaction.  One thread per cell, kChunk threads per workgroup.
// `boxes` != nullptr: ltrb distances were already produced by the fused DFL pass ([batch][cells][4]).
// REC = floats per Detection record: kYoloDetFloats (YOLOv8 / YOLO11, with the task branches) or 6 (YOLOv10, yolov10/plugin/yololayer.cu:
// 157-198: {x1, y1, x2, y2, conf, class_id} and no branches; the box, conf and class arithmetic is the same, operation for operation).
template <int REC>
__global__ __launch_bounds__(kChunk) void yolo_emit_kernel(LevelTable t, int classes, int total_cells,
                                                           const float* __restrict__ score,
                                                           const int* __restrict__ cls_in,
                                                           const int* __restrict__ chunk_cnt, int n_chunks,
                                                           int max_out, int out_elem, float* __restrict__ output,
                                                           const float4* __restrict__ boxes, YoloBranches br) {
    const int b = blockIdx.y;
    const int chunk = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int kWaves = kChunk / 64;
    __shared__ int s_wave[kWaves];
    __shared__ int s_base;

    // slots used by earlier chunks of this image
    if (wave == 0) {
        int acc = 0;
        for (int j = lane; j < chunk; j += 64) acc += chunk_cnt[b * n_chunks + j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
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
        const int l = find_level(t.cell_off, t.n_levels, g);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const int e = g - t.cell_off[l];
        const int gw = t.grid_w[l];
        const float stride = (float)t.stride[l];
        float4 d;
        const int info_len = 4 + classes + (br.seg ? 32 : 0) + (br.pose ? br.nk * 3 : 0) + (br.obb ? 1 : 0);
        const float* cur = boxes ? nullptr : t.in[l] + (size_t)b * cells * info_len + e;
        if (boxes) {
            d = boxes[(size_t)b * total_cells + g];
        } else {
            d = make_float4(cur[0], cur[(size_t)cells], cur[(size_t)2 * cells], cur[(size_t)3 * cells]);
        }
        const int row = e / gw, col = e - row * gw;
        float* det = out + 1 + (size_t)slot * REC;
        det[0] = (col + 0.5f - d.x) * stride;
        det[1] = (row + 0.5f - d.y) * stride;
        det[2] = (col + 0.5f + d.z) * stride;
        det[3] = (row + 0.5f + d.w) * stride;
        det[4] = sc;
        det[5] = (float)cls_in[(size_t)b * total_cells + g];
        if constexpr (REC == trtx::kYoloDetFloats) {
        // ---- the seg / pose / obb branches of CalDetection (yololayer.cu:222-279); plugin-ABI form only
        if (cur && br.seg) {
            const float* m = cur + (size_t)(4 + classes + (br.pose ? br.nk * 3 : 0) + (br.obb ? 1 : 0)) * cells;
            for (int k = 0; k < 32; ++k) det[6 + k] = m[(size_t)k * cells];
        }
        if (cur && br.pose) {
            const int istride = t.stride[l];
            const float* kp = cur + (size_t)(4 + classes + (br.seg ? 32 : 0) + (br.obb ? 1 : 0)) * cells;
            for (int k = 0; k < br.nk; ++k) {
                const float kconf = 1.0f / (1.0f + expf(-kp[(size_t)(k * 3 + 2) * cells]));
                // "(in * 2.0 + col) * stride": double arithmetic, rounded once to float (yololayer.cu:236-237)
                const float kx = (float)((kp[(size_t)(k * 3) * cells] * 2.0 + col) * istride);
                const float ky = (float)((kp[(size_t)(k * 3 + 1) * cells] * 2.0 + row) * istride);
                const bool inside = kx >= det[0] && kx <= det[2] && ky >= det[1] && ky <= det[3];
                float* o = det + 38 + k * 3;
                if (kconf < br.kpt_conf || !inside) {
                    o[0] = -1;
                    o[1] = -1;
                    o[2] = -1;
                } else {
                    o[0] = kx;
                    o[1] = ky;
                    o[2] = kconf;
                }
            }
        }
        if (cur && br.obb) {
            const int istride = t.stride[l];
            const double pi = 3.14159265358979323846;  // M_PI
            const float ain = cur[(size_t)(4 + classes + (br.seg ? 32 : 0) + (br.pose ? br.nk * 3 : 0)) * cells];
            const double angle = ((1.0f / (1.0f + expf(-ain))) - 0.25f) * pi;  // float difference times double pi (:259)
            const double cos1 = cos(angle), sin1 = sin(angle);
            const float xf = (d.z - d.x) / 2, yf = (d.w - d.y) / 2;
            const double x = xf * cos1 - yf * sin1;
            const double y = xf * sin1 + yf * cos1;
            det[0] = (float)((col + 0.5f + x) * istride);
            det[1] = (float)((row + 0.5f + y) * istride);
            det[2] = (d.x + d.z) * istride;
            det[3] = (d.y + d.w) * istride;
            det[trtx::kYoloDetFloats - 1] = (float)angle;
        }
        }   // REC == kYoloDetFloats
    }
    if (chunk == n_chunks - 1 && threadIdx.x == kChunk - 1) {
        int total = before + in_wave + (keep ? 1 : 0);  // last thread of the last chunk sees the full count
        out[0] = (float)(total < max_out ? total : max_out);
    }
}

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


// ---------------------------------------------------------------------------------------------------------
// Fused detect-head tail: reads the NHWC fp16 output of the head convolutions directly
// (channels [0,64) = 4 sides x 16 DFL bins, [64, 64+classes) = class logits) and performs, per cell,
//   DFL: softmax over the 16 bins of each side, expectation with the 1x1 "dfl.conv" weights
//        (yolov8/src/block.cpp:239-257 — shuffle/softmax/conv/shuffle collapsed into registers, fp32), and
//   the CalDetection class scan (sigmoid, strict-'>' argmax, 0.1 threshold; yololayer.cu:195-204).
// It replaces ~10 layout/shuffle/slice/softmax/concat launches per level of the un-fused graph.

struct HeadTable {
    const void* in[kMaxLevels];
    int ld[kMaxLevels];
    int cell_off[kMaxLevels + 1];
    int n_levels;
};

struct BranchTable {
    const void* in[kMaxLevels];  // device pointers, [batch][cells_l][ld[l]]: channels [0, extra) of the cell's branch
    int ld[kMaxLevels];
    int vec;                      // every ld and base allows 16-byte loads
};

// Pass 1 of the fused heads.  T = element type of the NHWC head tensors: _Float16 (kFP16 engines) or float (fp32 engines, round 5:
// the build that meets BASELINE's tolerance had run the un-fused graph, ~30 layout / shuffle / softmax launches).
// TAIL = false (det head): classes % 8 == 0, every logit is read in 16-byte pieces.  TAIL = true (task head): any classes >= 1; the
// last (classes % 8) logits are read one by one, so the NHWC padding channels behind them never reach the argmax (nor a load past
// the tensor's last pixel).  With classes % 8 == 0 both are the same arithmetic, operation for operation.
// The det and the task kernel used to be two copies, the det one pinned by being left untouched.  Now both are this body, and what pins
// it is: the tail is `if constexpr`, so the det instantiations hold none of it (their ISA equals the pre-merge kernels' up to the operand
// order of commutative packed adds and multiplies); the det plans' hashes (tests/golden/yolo11_det_plan_sha256.json); and the bit-for-bit tests against
// the oracle and the reference's own plugin (tests/test_gpu_yolo11_tasks.py, test_gpu_yolo_plugins.py, test_ref_pinning.py).
template <typename T, bool TAIL>
__device__ __forceinline__ void head_score(const HeadTable& t, int classes, int total_cells, const float* __restrict__ dfl_w,
                                           float* __restrict__ score, int* __restrict__ cls_out, float4* __restrict__ boxes,
                                           int* __restrict__ chunk_cnt, int n_chunks) {
    __shared__ int s_list[256];
    __shared__ int s_n, s_keep;
    const int b = blockIdx.y;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) {
        s_n = 0;
        s_keep = 0;
    }
    __syncthreads();
    const int full = TAIL ? classes & ~7 : classes;  // classes read eight at a time; [full, classes) one at a time
    auto cell_ptr = [&](int gg) {
        const int l = find_level(t.cell_off, t.n_levels, gg);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        return static_cast<const T*>(t.in[l]) + ((size_t)b * cells + (gg - t.cell_off[l])) * t.ld[l];
    };
    // ---- phase 1, every cell: the cell can only survive if some sigmoid(logit) >= 0.1, i.e. some logit >= -2.1972.  The
    // maximum of the raw fp16 logits (exact, packed max, no exp) settles that; possible survivors are compacted into a
    // list so that the expensive exact pass below runs on dense lanes instead of a few lanes of every wave.
    // The class logits are read by the WAVE, not by the cell's own thread: consecutive lanes take consecutive 16-byte pieces of
    // the 64 cells of the wave (a cell's logits are classes/8 pieces in a row), so one load instruction touches ~15 cache lines
    // instead of 64 (one per lane, 288 bytes apart) - this pass is what the kernel's time is.  A piece whose packed maximum
    // passes the test raises its cell's flag in LDS; NaN pieces do not, exactly like NaN fails 'pr > best' in the scan.
    s_list[threadIdx.x] = 0;   // phase 1 borrows the list as the per-cell flags (same-value races only)
    __syncthreads();
    {
        const int wave0 = threadIdx.x & ~63, lane = threadIdx.x & 63;
        const int pieces = TAIL ? (classes + 7) >> 3 : classes >> 3;
        const int g0 = blockIdx.x * 256 + wave0;
        int cells_here = total_cells - g0;
        cells_here = cells_here > 64 ? 64 : cells_here;
        const int n = cells_here * pieces;
        for (int j = lane; j < n; j += 64) {
            const int c = j / pieces, q = j - c * pieces;
            const T* p = cell_ptr(g0 + c) + 64 + q * 8;
            bool tail_piece = false;
            if constexpr (TAIL) tail_piece = q * 8 >= full;
            float m = -INFINITY;
            if (!tail_piece) {
                float v[8];
                load8(p, v);
                m = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
            } else if constexpr (TAIL) {
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
    // ---- phase 2, possible survivors only: the reference arithmetic (DFL softmax . w per side, sigmoid of every class, strict
    // '>' argmax), so kept candidates are bit-identical to evaluating every cell
    int kept = 0;
    for (int k = threadIdx.x; k < s_n; k += 256) {
        const int gg = blockIdx.x * 256 + s_list[k];
        const T* cell = cell_ptr(gg);
        float w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = dfl_w[i];
        float side[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float lo[8], hi[8], x[16];
            load8(cell + s * 16, lo);
            load8(cell + s * 16 + 8, hi);
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
                // fp32 engines: the arithmetic of the un-fused chain to the bit - softmax_kernel (linear_ops.hip: p_i = expf(x_i - max) * (1 / sum)) followed by the
                // DFL 1x1 convolution (conv_direct_kernel: an fmaf chain over the 16 bins from 0) - so that a user YoloLayer plugin behind the un-fused graph and
                // the built-in fused tail return the same boxes (tests/test_ref_pinning.py::test_reference_yololayer_plugin_runs_inside_a_full_engine)
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
        float best = 0.0f;
        int bcls = 0;
        const T* cl = cell + 64;
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
        if constexpr (TAIL) {
            for (int c = full; c < classes; ++c) {
                const float pr = logist((float)cl[c]);
                if (pr > best) {
                    best = pr;
                    bcls = c;
                }
            }
        }
        const bool keep = !((double)best < 0.1);
        const size_t o = (size_t)b * total_cells + gg;
        score[o] = keep ? best : -1.0f;
        cls_out[o] = bcls;
        boxes[o] = make_float4(side[0], side[1], side[2], side[3]);
        kept += keep ? 1 : 0;
    }
    // per-kChunk candidate counts (two 256-thread workgroups feed one chunk counter)
    trtx::workgroup_count(&s_keep, kept);
    if (threadIdx.x == 0 && s_keep) atomicAdd(&chunk_cnt[b * n_chunks + (blockIdx.x * 256) / kChunk], s_keep);
}

template <typename T>
__global__ __launch_bounds__(256) void yolo_head_score_kernel(HeadTable t, int classes, int total_cells,
                                                              const float* __restrict__ dfl_w,
                                                              float* __restrict__ score, int* __restrict__ cls_out,
                                                              float4* __restrict__ boxes,
                                                              int* __restrict__ chunk_cnt, int n_chunks) {
    head_score<T, false>(t, classes, total_cells, dfl_w, score, cls_out, boxes, chunk_cnt, n_chunks);
}

template <typename T>
__global__ __launch_bounds__(256) void yolo_task_score_kernel(HeadTable t, int classes, int total_cells,
                                                              const float* __restrict__ dfl_w,
                                                              float* __restrict__ score, int* __restrict__ cls_out,
                                                              float4* __restrict__ boxes,
                                                              int* __restrict__ chunk_cnt, int n_chunks) {
    head_score<T, true>(t, classes, total_cells, dfl_w, score, cls_out, boxes, chunk_cnt, n_chunks);
}

// The seg / pose / obb fields of one Detection record (yololayer.cu:222-279) from the cell's branch channels `br` (contiguous; `vec`:
// 16-byte aligned).  The arithmetic is the plugin's (yolo_emit_kernel above): keypoints as (v * 2.0 + col) * stride in double rounded
// once, a sigmoid confidence and the -1 triple below kpt_conf or outside the box; obb rotates the centre by (sigmoid(a) - 0.25) * pi.
template <typename T>
__device__ __forceinline__ void task_branch(float* det, const T* br, bool vec, const YoloBranches& b, float4 d, int row, int col, int istride) {
    if (b.seg) {
        if (vec) {
#pragma unroll
            for (int k = 0; k < 32; k += 8) {
                float v[8];
                load8(br + k, v);
#pragma unroll
                for (int i = 0; i < 8; ++i) det[6 + k + i] = v[i];
            }
        } else {
            for (int k = 0; k < 32; ++k) det[6 + k] = (float)br[k];
        }
    }
    if (b.pose) {
        for (int k = 0; k < b.nk; ++k) {
            const float kconf = 1.0f / (1.0f + expf(-(float)br[k * 3 + 2]));
            const float kx = (float)(((float)br[k * 3] * 2.0 + col) * istride);
            const float ky = (float)(((float)br[k * 3 + 1] * 2.0 + row) * istride);
            const bool inside = kx >= det[0] && kx <= det[2] && ky >= det[1] && ky <= det[3];
            float* o = det + 38 + k * 3;
            if (kconf < b.kpt_conf || !inside) {
                o[0] = -1;
                o[1] = -1;
                o[2] = -1;
            } else {
                o[0] = kx;
                o[1] = ky;
                o[2] = kconf;
            }
        }
    }
    if (b.obb) {
        const double pi = 3.14159265358979323846;
        const float ain = (float)br[0];
        const double angle = ((1.0f / (1.0f + expf(-ain))) - 0.25f) * pi;
        const double cos1 = cos(angle), sin1 = sin(angle);
        const float xf = (d.z - d.x) / 2, yf = (d.w - d.y) / 2;
        const double x = xf * cos1 - yf * sin1;
        const double y = xf * sin1 + yf * cos1;
        det[0] = (float)((col + 0.5f + x) * istride);
        det[1] = (float)((row + 0.5f + y) * istride);
        det[2] = (d.x + d.z) * istride;
        det[3] = (d.y + d.w) * istride;
        det[trtx::kYoloDetFloats - 1] = (float)angle;
    }
}

// Pass 2 of the task head: yolo_emit_kernel's ordered compaction and box / conf / class record, then the branch of the cell.
template <typename T>
__global__ __launch_bounds__(kChunk) void yolo_task_emit_kernel(LevelTable t, BranchTable bt, int total_cells,
                                                                const float* __restrict__ score,
                                                                const int* __restrict__ cls_in,
                                                                const int* __restrict__ chunk_cnt, int n_chunks,
                                                                int max_out, int out_elem, float* __restrict__ output,
                                                                const float4* __restrict__ boxes, YoloBranches br) {
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
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
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
        const int l = find_level(t.cell_off, t.n_levels, g);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const int e = g - t.cell_off[l];
        const int gw = t.grid_w[l];
        const float stride = (float)t.stride[l];
        const float4 d = boxes[(size_t)b * total_cells + g];
        const int row = e / gw, col = e - row * gw;
        float* det = out + 1 + (size_t)slot * trtx::kYoloDetFloats;
        det[0] = (col + 0.5f - d.x) * stride;
        det[1] = (row + 0.5f - d.y) * stride;
        det[2] = (col + 0.5f + d.z) * stride;
        det[3] = (row + 0.5f + d.w) * stride;
        det[4] = sc;
        det[5] = (float)cls_in[(size_t)b * total_cells + g];
        const T* bp = static_cast<const T*>(bt.in[l]) + ((size_t)b * cells + e) * bt.ld[l];
        task_branch(det, bp, bt.vec != 0, br, d, row, col, t.stride[l]);
    }
    if (chunk == n_chunks - 1 && threadIdx.x == kChunk - 1) {
        int total = before + in_wave + (keep ? 1 : 0);
        out[0] = (float)(total < max_out ? total : max_out);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// Host side.  The three entry paths (plugin, det head, task head) share the level geometry and the workspace layout.

// geometry of the levels, for however many of them fit the table; `in` is left to the caller (the plugin's planar inputs)
static LevelTable make_levels(int n_levels, int net_h, int net_w, const int* strides) {
    LevelTable t{};
    t.n_levels = n_levels;
    int off = 0;
    for (int i = 0; i < n_levels && i < kMaxLevels; ++i) {
        t.cell_off[i] = off;
        t.grid_w[i] = net_w / strides[i];
        t.stride[i] = strides[i];
        off += (net_h / strides[i]) * t.grid_w[i];
    }
    for (int i = n_levels < 0 ? 0 : n_levels; i <= kMaxLevels; ++i) t.cell_off[i] = off;
    return t;
}

// the level geometry every entry path divides by: a null table, a stride below 1 or an empty net would be a host division by zero or a
// launch over no cells
static bool bad_geometry(int n_levels, int net_h, int net_w, const int* strides) {
    if (n_levels < 1 || n_levels > kMaxLevels || !strides || net_h < 1 || net_w < 1) return true;
    for (int i = 0; i < n_levels; ++i)
        if (strides[i] < 1) return true;
    return false;
}

// 0 for a geometry no entry path accepts (bad_geometry, or no level holds a cell)
static size_t count_cells(int net_h, int net_w, const int* strides, int n_levels) {
    if (bad_geometry(n_levels, net_h, net_w, strides)) return 0;
    size_t cells = 0;
    for (int i = 0; i < n_levels; ++i) cells += (size_t)(net_h / strides[i]) * (net_w / strides[i]);
    return cells;
}

// the NHWC head tensors over the same levels
static HeadTable make_head(const LevelTable& t, const void* const* heads, const int* ld) {
    HeadTable h{};
    h.n_levels = t.n_levels;
    for (int i = 0; i < t.n_levels; ++i) {
        h.in[i] = heads[i];
        h.ld[i] = ld[i];
    }
    for (int i = 0; i <= kMaxLevels; ++i) h.cell_off[i] = t.cell_off[i];
    return h;
}

// score | cls | boxes (fused heads only) | chunk_cnt, each aligned to 256 bytes.  The *_workspace functions carve a null base, so the
// size they report is the end of the same layout.
struct Workspace {
    float* score;
    int* cls;
    float4* boxes;
    int* chunk_cnt;
    int n_chunks;
    size_t bytes;
};

static Workspace carve(void* base, int batch, size_t cells, bool with_boxes) {
    Workspace w{};
    w.n_chunks = (int)((cells + kChunk - 1) / kChunk);
    const auto take = [&](size_t bytes) {
        void* p = base ? static_cast<char*>(base) + w.bytes : nullptr;
        w.bytes += trtx::align_up(bytes, 256);
        return p;
    };
    w.score = static_cast<float*>(take((size_t)batch * cells * sizeof(float)));
    w.cls = static_cast<int*>(take((size_t)batch * cells * sizeof(int)));
    if (with_boxes) w.boxes = static_cast<float4*>(take((size_t)batch * cells * sizeof(float4)));
    w.chunk_cnt = static_cast<int*>(take((size_t)batch * w.n_chunks * sizeof(int)));
    return w;
}

extern "C" size_t trtx_yolo_decode_workspace(int batch, int net_h, int net_w, const int* strides, int n_levels) {
    return carve(nullptr, batch, count_cells(net_h, net_w, strides, n_levels), false).bytes;
}

extern "C" size_t trtx_yolo_head_decode_workspace(int batch, int net_h, int net_w, const int* strides, int n_levels) {
    return carve(nullptr, batch, count_cells(net_h, net_w, strides, n_levels), true).bytes;
}

// the plugin route of both record lengths: the score pass, then the emit pass of `rec` floats per record
static int32_t decode_planar(int rec, const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w, const int* strides,
                             int max_out, const YoloBranches& br, float* output, void* workspace, size_t workspace_bytes, hipStream_t stream,
                             const char* what) {
    if (n_levels < 1 || n_levels > kMaxLevels || batch < 1 || classes < 1 || max_out < 1 || !inputs || !output ||
        !workspace || br.nk < 0 || br.nk > 17 || count_cells(net_h, net_w, strides, n_levels) == 0)
        return TRTX_ERR_INVALID;
    for (int i = 0; rec == 6 && i < n_levels; ++i)
        if (!inputs[i]) return TRTX_ERR_INVALID;
    if (workspace_bytes < trtx_yolo_decode_workspace(batch, net_h, net_w, strides, n_levels)) return TRTX_ERR_WORKSPACE;
    const int info_len = 4 + classes + (br.seg ? 32 : 0) + (br.pose ? br.nk * 3 : 0) + (br.obb ? 1 : 0);
    LevelTable t = make_levels(n_levels, net_h, net_w, strides);
    bool vec4 = true;
    for (int i = 0; i < n_levels; ++i) {
        t.in[i] = inputs[i];
        if ((t.cell_off[i + 1] - t.cell_off[i]) % 4 != 0 || (reinterpret_cast<uintptr_t>(inputs[i]) & 15) != 0) vec4 = false;
    }
    const int total_cells = t.cell_off[n_levels];
    const Workspace w = carve(workspace, batch, total_cells, false);
    const int out_elem = 1 + max_out * rec;
    dim3 grid(w.n_chunks, batch);
    if (vec4)
        hipLaunchKernelGGL(yolo_score_kernel<4>, grid, dim3(kChunk / 4), 0, stream, t, classes, info_len, total_cells, w.score,
                           w.cls, w.chunk_cnt, w.n_chunks);
    else
        hipLaunchKernelGGL(yolo_score_kernel<1>, grid, dim3(kChunk), 0, stream, t, classes, info_len, total_cells, w.score, w.cls,
                           w.chunk_cnt, w.n_chunks);
    if (rec == 6)
        hipLaunchKernelGGL(yolo_emit_kernel<6>, grid, dim3(kChunk), 0, stream, t, classes, total_cells, w.score, w.cls,
                           w.chunk_cnt, w.n_chunks, max_out, out_elem, output, (const float4*)nullptr, br);
    else
        hipLaunchKernelGGL(yolo_emit_kernel<trtx::kYoloDetFloats>, grid, dim3(kChunk), 0, stream, t, classes, total_cells, w.score, w.cls,
                           w.chunk_cnt, w.n_chunks, max_out, out_elem, output, (const float4*)nullptr, br);
    return trtx::check_launch(what);
}

extern "C" int32_t trtx_yolo_decode_ex(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                                       const int* strides, int max_out, int n_kpt, float kpt_conf, int is_seg, int is_pose, int is_obb,
                                       float* output, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const YoloBranches br{is_seg ? 1 : 0, is_pose ? 1 : 0, is_obb ? 1 : 0, n_kpt, kpt_conf};
    return decode_planar(trtx::kYoloDetFloats, inputs, n_levels, batch, classes, net_h, net_w, strides, max_out, br, output, workspace,
                         workspace_bytes, stream, "trtx_yolo_decode");
}

// YOLOv10's YoloLayerPlugin::forwardGpu + CalDetection (yolov10/plugin/yololayer.cu:157-240): the YOLOv8 score pass and 6-float records
extern "C" int32_t trtx_yolov10_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                                       const int* strides, int max_out, float* output, void* workspace, size_t workspace_bytes,
                                       hipStream_t stream) {
    return decode_planar(6, inputs, n_levels, batch, classes, net_h, net_w, strides, max_out, YoloBranches{0, 0, 0, 0, 0.f}, output, workspace,
                         workspace_bytes, stream, "trtx_yolov10_decode");
}

extern "C" int32_t trtx_yolo_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h,
                                    int net_w, const int* strides, int max_out, float* output, void* workspace,
                                    size_t workspace_bytes, hipStream_t stream) {
    return trtx_yolo_decode_ex(inputs, n_levels, batch, classes, net_h, net_w, strides, max_out, 0, 0.f, 0, 0, 0, output, workspace,
                               workspace_bytes, stream);
}

// The fused heads after their argument checks: `bt` = nullptr is the det head (yolo_head_score_kernel, then the plugin's emit pass on
// the DFL boxes), otherwise the task head with the masked class tail and the branch tensors of `bt`.
static int32_t launch_head(const LevelTable& t, const HeadTable& h, const BranchTable* bt, int elem_bytes, int batch, int classes,
                           const float* dfl_weights, int max_out, const YoloBranches& br, float* output, void* workspace, hipStream_t stream,
                           const char* what, int rec = trtx::kYoloDetFloats) {
    const int total_cells = t.cell_off[t.n_levels];
    const Workspace w = carve(workspace, batch, total_cells, true);
    if (hipMemsetAsync(w.chunk_cnt, 0, (size_t)batch * w.n_chunks * sizeof(int), stream) != hipSuccess) return TRTX_ERR_HIP;
    const int out_elem = 1 + max_out * rec;
    const dim3 sgrid((total_cells + 255) / 256, batch), egrid(w.n_chunks, batch);
    const auto score = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, sgrid, dim3(256), 0, stream, h, classes, total_cells, dfl_weights, w.score, w.cls, w.boxes, w.chunk_cnt,
                           w.n_chunks);
    };
    const auto task_emit = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, egrid, dim3(kChunk), 0, stream, t, *bt, total_cells, w.score, w.cls, w.chunk_cnt, w.n_chunks, max_out,
                           out_elem, output, (const float4*)w.boxes, br);
    };
    if (!bt && rec == 6) {
        // the YOLOv10 head: the det score pass (classes % 8 == 0) or the task head's masked class tail (any class count), 6-float records
        const bool tail = classes % 8 != 0;
        if (elem_bytes == 2)
            tail ? score(yolo_task_score_kernel<_Float16>) : score(yolo_head_score_kernel<_Float16>);
        else
            tail ? score(yolo_task_score_kernel<float>) : score(yolo_head_score_kernel<float>);
        hipLaunchKernelGGL(yolo_emit_kernel<6>, egrid, dim3(kChunk), 0, stream, t, classes, total_cells, w.score, w.cls, w.chunk_cnt,
                           w.n_chunks, max_out, out_elem, output, (const float4*)w.boxes, br);
    } else if (!bt) {
        if (elem_bytes == 2)
            score(yolo_head_score_kernel<_Float16>);
        else
            score(yolo_head_score_kernel<float>);
        hipLaunchKernelGGL(yolo_emit_kernel<trtx::kYoloDetFloats>, egrid, dim3(kChunk), 0, stream, t, classes, total_cells, w.score, w.cls, w.chunk_cnt,
                           w.n_chunks, max_out, out_elem, output, (const float4*)w.boxes, br);
    } else if (elem_bytes == 2) {
        score(yolo_task_score_kernel<_Float16>);
        task_emit(yolo_task_emit_kernel<_Float16>);
    } else {
        score(yolo_task_score_kernel<float>);
        task_emit(yolo_task_emit_kernel<float>);
    }
    return trtx::check_launch(what);
}

static int32_t head_decode(const void* const* heads, const int* ld, int elem_bytes, int n_levels, int batch, int classes, int net_h, int net_w, const int* strides,
                           const float* dfl_weights, int max_out, float* output, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (n_levels < 1 || n_levels > kMaxLevels || batch < 1 || classes < 8 || classes % 8 || max_out < 1 || !heads ||
        !ld || !dfl_weights || !output || !workspace || count_cells(net_h, net_w, strides, n_levels) == 0)
        return TRTX_ERR_INVALID;
    if (workspace_bytes < trtx_yolo_head_decode_workspace(batch, net_h, net_w, strides, n_levels)) return TRTX_ERR_WORKSPACE;
    for (int i = 0; i < n_levels; ++i)
        // the 16-byte loads read channels [0, 64 + classes) of every pixel: a shorter stride would read the next pixel's (and, at the
        // tensor's last pixel, past it)
        if (ld[i] % (16 / elem_bytes) || ld[i] < 64 + classes || (reinterpret_cast<uintptr_t>(heads[i]) & 15)) return TRTX_ERR_UNSUPPORTED;
    const LevelTable t = make_levels(n_levels, net_h, net_w, strides);
    return launch_head(t, make_head(t, heads, ld), nullptr, elem_bytes, batch, classes, dfl_weights, max_out, YoloBranches{0, 0, 0, 0, 0.f},
                       output, workspace, stream, "trtx_yolo_head_decode_nhwc");
}

extern "C" int32_t trtx_yolo_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch,
                                              int classes, int net_h, int net_w, const int* strides,
                                              const float* dfl_weights, int max_out, float* output, void* workspace,
                                              size_t workspace_bytes, hipStream_t stream) {
    return head_decode(heads, ld, 2, n_levels, batch, classes, net_h, net_w, strides, dfl_weights, max_out, output, workspace, workspace_bytes, stream);
}

extern "C" int32_t trtx_yolo_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                  const int* strides, const float* dfl_weights, int max_out, float* output, void* workspace,
                                                  size_t workspace_bytes, hipStream_t stream) {
    return head_decode(heads, ld, 4, n_levels, batch, classes, net_h, net_w, strides, dfl_weights, max_out, output, workspace, workspace_bytes, stream);
}

// Fused YOLOv10 head: the det head above for the 6-float plugin (yolov10/plugin/yololayer.cu:157-198 behind the DFL chain of
// yolov10/src/block.cpp:214-233), any class count >= 1.  The head tensors are read as the det head reads them (classes % 8 == 0) or as
// the task head does (the last classes % 8 logits one by one); the workspace is the det head's.
extern "C" size_t trtx_yolov10_head_decode_workspace(int batch, int net_h, int net_w, const int* strides, int n_levels) {
    return trtx_yolo_head_decode_workspace(batch, net_h, net_w, strides, n_levels);
}

static int32_t head10_decode(const void* const* heads, const int* ld, int elem_bytes, int n_levels, int batch, int classes, int net_h, int net_w,
                             const int* strides, const float* dfl_weights, int max_out, float* output, void* workspace, size_t workspace_bytes,
                             hipStream_t stream) {
    if (n_levels < 1 || n_levels > kMaxLevels || batch < 1 || classes < 1 || max_out < 1 || !heads || !ld || !dfl_weights || !output ||
        !workspace || count_cells(net_h, net_w, strides, n_levels) == 0)
        return TRTX_ERR_INVALID;
    for (int i = 0; i < n_levels; ++i)
        if (!heads[i]) return TRTX_ERR_INVALID;
    if (workspace_bytes < trtx_yolo_head_decode_workspace(batch, net_h, net_w, strides, n_levels)) return TRTX_ERR_WORKSPACE;
    for (int i = 0; i < n_levels; ++i)
        // the 16-byte loads read channels [0, 64 + (classes & ~7)) of every pixel, the scalar ones up to 64 + classes
        if (ld[i] % (16 / elem_bytes) || ld[i] < 64 + classes || (reinterpret_cast<uintptr_t>(heads[i]) & 15)) return TRTX_ERR_UNSUPPORTED;
    const LevelTable t = make_levels(n_levels, net_h, net_w, strides);
    return launch_head(t, make_head(t, heads, ld), nullptr, elem_bytes, batch, classes, dfl_weights, max_out, YoloBranches{0, 0, 0, 0, 0.f},
                       output, workspace, stream, "trtx_yolov10_head_decode_nhwc", 6);
}

extern "C" int32_t trtx_yolov10_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                 const int* strides, const float* dfl_weights, int max_out, float* output, void* workspace,
                                                 size_t workspace_bytes, hipStream_t stream) {
    return head10_decode(heads, ld, 2, n_levels, batch, classes, net_h, net_w, strides, dfl_weights, max_out, output, workspace, workspace_bytes, stream);
}

extern "C" int32_t trtx_yolov10_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                     const int* strides, const float* dfl_weights, int max_out, float* output, void* workspace,
                                                     size_t workspace_bytes, hipStream_t stream) {
    return head10_decode(heads, ld, 4, n_levels, batch, classes, net_h, net_w, strides, dfl_weights, max_out, output, workspace, workspace_bytes, stream);
}

// Fused task head (YOLO11 seg / pose / obb, explicit batch): reads, besides the det head's tensors, the cell's task branch from its own
// NHWC tensor - the output of the cv4 1x1 convolution (yolo11/src/model.cpp:474-507).  It replaces, per level, the (64 + classes)-channel
// head converted to fp32 LINEAR, the slices, the DFL chain, the branch's own conversion, the concat scatters and then the plugin's two
// passes (yololayer.cu:178-279).
static int32_t task_head_decode(const void* const* heads, const int* ld, const void* const* branches, const int* branch_ld, int elem_bytes,
                                int n_levels, int batch, int classes, int net_h, int net_w, const int* strides, const float* dfl_weights,
                                int max_out, int is_seg, int is_pose, int is_obb, int n_kpt, float kpt_conf, float* output, void* workspace,
                                size_t workspace_bytes, hipStream_t stream) {
    if (n_levels < 1 || n_levels > kMaxLevels || batch < 1 || classes < 1 || max_out < 1 || !heads || !ld || !branches || !branch_ld ||
        !dfl_weights || !output || !workspace || (is_seg != 0) + (is_pose != 0) + (is_obb != 0) != 1 || (is_pose && (n_kpt < 1 || n_kpt > 17)) ||
        count_cells(net_h, net_w, strides, n_levels) == 0)
        return TRTX_ERR_INVALID;
    if (workspace_bytes < trtx_yolo_head_decode_workspace(batch, net_h, net_w, strides, n_levels)) return TRTX_ERR_WORKSPACE;
    const int extra = is_seg ? 32 : (is_pose ? 3 * n_kpt : 1);
    const int vec_elems = 16 / elem_bytes;
    BranchTable bt{};
    bt.vec = 1;
    for (int i = 0; i < n_levels; ++i) {
        // the head's 16-byte loads read channels up to 64 + (classes & ~7): a stride of at least 64 + classes, a multiple of 16 bytes
        if (ld[i] % vec_elems || ld[i] < 64 + classes || (reinterpret_cast<uintptr_t>(heads[i]) & 15)) return TRTX_ERR_UNSUPPORTED;
        if (!branches[i] || branch_ld[i] < extra) return TRTX_ERR_INVALID;
        if (branch_ld[i] % vec_elems || (reinterpret_cast<uintptr_t>(branches[i]) & 15)) bt.vec = 0;
        bt.in[i] = branches[i];
        bt.ld[i] = branch_ld[i];
    }
    const LevelTable t = make_levels(n_levels, net_h, net_w, strides);
    const YoloBranches br{is_seg ? 1 : 0, is_pose ? 1 : 0, is_obb ? 1 : 0, is_pose ? n_kpt : 0, kpt_conf};
    return launch_head(t, make_head(t, heads, ld), &bt, elem_bytes, batch, classes, dfl_weights, max_out, br, output, workspace, stream,
                       "trtx_yolo_task_head_decode_nhwc");
}

extern "C" int32_t trtx_yolo_task_head_decode_nhwc(const void* const* heads, const int* ld, const void* const* branches, const int* branch_ld,
                                                   int n_levels, int batch, int classes, int net_h, int net_w, const int* strides,
                                                   const float* dfl_weights, int max_out, int is_seg, int is_pose, int is_obb, int n_kpt,
                                                   float kpt_conf, float* output, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return task_head_decode(heads, ld, branches, branch_ld, 2, n_levels, batch, classes, net_h, net_w, strides, dfl_weights, max_out, is_seg,
                            is_pose, is_obb, n_kpt, kpt_conf, output, workspace, workspace_bytes, stream);
}

extern "C" int32_t trtx_yolo_task_head_decode_nhwc_f32(const void* const* heads, const int* ld, const void* const* branches, const int* branch_ld,
                                                       int n_levels, int batch, int classes, int net_h, int net_w, const int* strides,
                                                       const float* dfl_weights, int max_out, int is_seg, int is_pose, int is_obb, int n_kpt,
                                                       float kpt_conf, float* output, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return task_head_decode(heads, ld, branches, branch_ld, 4, n_levels, batch, classes, net_h, net_w, strides, dfl_weights, max_out, is_seg,
                            is_pose, is_obb, n_kpt, kpt_conf, output, workspace, workspace_bytes, stream);
}
