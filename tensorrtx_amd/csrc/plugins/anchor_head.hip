// Fused anchor head (YOLOv5 and YOLOv7 families) for gfx950 (MI355X): the two passes of anchor_decode.hip reading the detect
// convolutions' own NHWC output - what the engine uses instead of one layout pass per level to fp32 planes followed by the plugin.
//
// heads[l]: [batch][cells_l][ld_l], T = _Float16 (fp16 engines) or float (fp32 engines).  Channel k * info + j of a pixel is value j of
// anchor k (info = 5 + classes): x, y, w, h, objectness, class logits.  Channels [3 * info, ld) are padding and hold whatever the
// convolution wrote: no lane reads one into a result.  The arithmetic is that of anchor_decode.hip's two kernels, operation for
// operation (yolov5/plugin/yololayer.cu:161-227, yolov7/plugin/yololayer.cu:152-207); the records, their canonical (level, cell, anchor)
// order and the clamped count are those of trtx_yolov5_decode and trtx_yolov7_decode.  The families differ in the record alone: kDet
// floats, 38 for YOLOv5 (bbox[4], conf, class_id, mask[32]) and 6 for YOLOv7 (no mask).  Pass 1 never sees a record, so the two share its
// kernels; pass 2 is one template on kDet.
//
// The Darknet form (YOLOv3 / YOLOv3-tiny / YOLOv4; kDet = 7: bbox[4], det_confidence, class_id, class_confidence) runs the same mapping
// with anchor_decode.hip's Darknet arithmetic (yolov4/yololayer.cu:154-199): the double-divide Logist, a second gate on the class maximum
// after the scan (so pass 1 counts what passed both, not the ballot), the class maximum alone in the score plane, and in pass 2
// (col + Logist(x)), exp(w) * anchor and the objectness taken from the row again.  The double divide runs for anchors past the objectness
// gate only.
//
// Mapping.  A pixel is one contiguous row (510 B of 512 for 80 classes in fp16), so lanes run along the CHANNEL axis:
//   step 1  a wave takes 16 consecutive cells; lane 3 p + k loads the objectness of anchor k of cell p (48 loads in one instruction,
//           one 64-B sector each) and the ballot of `!(box_prob < 0.1f)` is the wave's candidate mask.  A cell without a candidate is
//           done here: its class logits are neither loaded nor put through expf.  That is the common case by far (the gate drops
//           > 99 % of the anchors of a trained model), so the kernel reads three sectors of most rows, not the rows.
//   step 2  cells with a candidate are taken two at a time, one per half-wave.  32 lanes cover a 256-channel fp16 row with one 16-byte
//           load each (two for fp32); a lane scans its 8 (4) channels in ascending order into one (best, class) pair per anchor, for
//           the anchors that passed only, and a 5-step xor butterfly over the half-wave joins the pairs.  The join keeps the lower
//           class index on equal probability, which is what the reference's strict-'>' scan from (0.0, class 0) returns.
//           Rows whose base or stride is not 16-byte aligned take element loads (lane s reads channels s, s + 32, ...).
// One thread per cell (the channel-major kernel's mapping) would read 2-byte elements 512 B apart here.
// Pass 2 counts records, one per kept (cell, anchor); a record starts at float 1 + kDet * slot of its row - 4-byte aligned only - and its
// six floats are written with six float stores.  Floats 6 .. 37 of a YOLOv5 record (the mask coefficients of the segmentation plugin
// route) are not written here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "decode_common.h"

namespace {

using trtx::logist;
using trtx::logist_darknet;

constexpr int kMaxLevels = 8;
constexpr int kAnchors = 3;     // kNumAnchor, yolov5/src/config.h:35 and yolov7/include/config.h
constexpr int kChunk = 512;     // cells per chunk counter and per emit workgroup (as anchor_decode.hip)
constexpr int kWaveCells = 16;  // cells per wave in the score pass: 48 objectness loads in one instruction
constexpr int kScoreBlock = 256;
constexpr int kBlockCells = kWaveCells * kScoreBlock / 64;   // 64: divides kChunk, so a workgroup feeds one chunk counter

struct HeadTable {
    const void* in[kMaxLevels];
    int ld[kMaxLevels];
    int vec[kMaxLevels];   // base and ld are multiples of 16 bytes
    int cell_off[kMaxLevels + 1];
    int grid_w[kMaxLevels], grid_h[kMaxLevels];
    float anchors[kMaxLevels][kAnchors * 2];
    int n_levels;
};

template <typename T>
struct Vec16;
template <>
struct Vec16<_Float16> {
    static constexpr int N = 8;
    typedef _Float16 type __attribute__((ext_vector_type(8)));
};
template <>
struct Vec16<float> {
    static constexpr int N = 4;
    typedef float type __attribute__((ext_vector_type(4)));
};

// One channel of the row into the per-anchor running maxima: the reference's `if (p > best)` in ascending class order.
template <bool kDarknet>
__device__ __forceinline__ void scan_channel(float v, int ch, int info, int nch, int abits, float (&best)[kAnchors], int (&bcls)[kAnchors]) {
    if (ch >= nch) return;   // padding
    const int k = ch >= 2 * info ? 2 : (ch >= info ? 1 : 0);
    const int j = ch - k * info;
    if (j < 5 || !((abits >> k) & 1)) return;
    const float p = kDarknet ? logist_darknet(v) : logist(v);
#pragma unroll
    for (int kk = 0; kk < kAnchors; ++kk)
        if (kk == k && p > best[kk]) {
            best[kk] = p;
            bcls[kk] = j - 5;
        }
}

// Pass 1: conf / class of every (cell, anchor); -1 marks a dropped candidate.  score / cls: [batch][cells][3].
// kDarknet: the Darknet Logist, the second gate, and the class maximum as the score.
template <typename T, bool kDarknet = false>
__global__ __launch_bounds__(kScoreBlock) void anchor_head_score_kernel(HeadTable t, int info, int total_cells, float* __restrict__ score,
                                                                       int* __restrict__ cls_out, int* __restrict__ chunk_cnt, int n_chunks) {
    using V = typename Vec16<T>::type;
    constexpr int VN = Vec16<T>::N;
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int g0 = blockIdx.x * kBlockCells + (threadIdx.x >> 6) * kWaveCells;
    const int nch = kAnchors * info;

    // ---- step 1: objectness of 16 cells x 3 anchors
    const int p = lane / kAnchors, k = lane - p * kAnchors;
    const int g = g0 + p;
    const bool mine = lane < kWaveCells * kAnchors && g < total_cells;
    float box_prob = 0.0f;
    bool pass = false;
    if (mine) {
        const int l = trtx::find_level(t.cell_off, t.n_levels, g);
        const int cells = t.cell_off[l + 1] - t.cell_off[l];
        const T* row = static_cast<const T*>(t.in[l]) + ((size_t)b * cells + (g - t.cell_off[l])) * t.ld[l];
        box_prob = kDarknet ? logist_darknet((float)row[k * info + 4]) : logist((float)row[k * info + 4]);
        pass = !(box_prob < 0.1f);  // "if (box_prob < kIgnoreThresh) continue;": NaN is kept, as there
        if (!pass) {
            const size_t o = ((size_t)b * total_cells + g) * kAnchors + k;
            score[o] = -1.0f;
            cls_out[o] = 0;
        }
    }
    const unsigned long long mask = __ballot(pass);   // bit 3 p + k, the same in every lane

    // ---- step 2: the class scan of the cells that hold a candidate, two per iteration (one per half-wave)
    const int half = lane >> 5, sub = lane & 31;
    int nkept = 0;     // kDarknet: anchors of this wave past both gates
    unsigned pm = 0;   // cells with a candidate
    for (int q = 0; q < kWaveCells; ++q)
        if ((mask >> (kAnchors * q)) & 7ull) pm |= 1u << q;
    while (pm) {
        const int p0 = __builtin_ctz(pm);
        pm &= pm - 1;
        const int p1 = pm ? __builtin_ctz(pm) : -1;
        pm &= pm - 1;   // (0 stays 0)
        const int px = half ? p1 : p0;
        const int abits = px >= 0 ? (int)((mask >> (kAnchors * px)) & 7ull) : 0;
        float best[kAnchors] = {0.0f, 0.0f, 0.0f};
        int bcls[kAnchors] = {0, 0, 0};
        if (px >= 0) {
            // g0 + px < total_cells: a bit of `mask` is set only for a cell that step 1 loaded
            const int gg = g0 + px;
            const int l = trtx::find_level(t.cell_off, t.n_levels, gg);
            const int cells = t.cell_off[l + 1] - t.cell_off[l];
            const T* row = static_cast<const T*>(t.in[l]) + ((size_t)b * cells + (gg - t.cell_off[l])) * t.ld[l];
            if (t.vec[l]) {
                // chunk c0 .. c0 + VN - 1 lies inside the row: c0 < 3 info <= ld and ld is a multiple of VN
                for (int c0 = sub * VN; c0 < nch; c0 += 32 * VN) {
                    const V v = *reinterpret_cast<const V*>(row + c0);
#pragma unroll
                    for (int i = 0; i < VN; ++i) scan_channel<kDarknet>((float)v[i], c0 + i, info, nch, abits, best, bcls);
                }
            } else {
                for (int ch = sub; ch < nch; ch += 32) scan_channel<kDarknet>((float)row[ch], ch, info, nch, abits, best, bcls);
            }
        }
        // join over the half-wave; every lane of the wave is here (p0, p1 and the masks are wave-uniform)
        const int any = (int)(((mask >> (kAnchors * p0)) | (p1 >= 0 ? (mask >> (kAnchors * p1)) : 0ull)) & 7ull);
#pragma unroll
        for (int kk = 0; kk < kAnchors; ++kk) {
            if (!((any >> kk) & 1)) continue;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best[kk], o);
                const int oc = __shfl_xor(bcls[kk], o);
                if (ob > best[kk] || (ob == best[kk] && oc < bcls[kk])) {   // equal probability: the lower class index, as the sequential scan
                    best[kk] = ob;
                    bcls[kk] = oc;
                }
            }
        }
        // lane kk of each half writes anchor kk of its cell
        const bool scanned = px >= 0 && sub < kAnchors && ((abits >> sub) & 1);
        if constexpr (kDarknet) {
            // "if (max_cls_prob < IGNORE_THRESH || box_prob < IGNORE_THRESH) continue;": the second half was the ballot
            const float bst = sub == 0 ? best[0] : (sub == 1 ? best[1] : best[2]);
            const int bc = sub == 0 ? bcls[0] : (sub == 1 ? bcls[1] : bcls[2]);
            const bool keep = scanned && !(bst < 0.1f);
            if (scanned) {
                const size_t o = ((size_t)b * total_cells + g0 + px) * kAnchors + sub;
                score[o] = keep ? bst : -1.0f;   // bst is in [0.1, 1] where kept, never NaN
                cls_out[o] = bc;
            }
            nkept += __popcll(__ballot(keep));   // every lane of the wave is here
        } else {
            // box_prob sits in lane 3 px + kk; every lane of the wave takes part in the shuffle
            const float bp = __shfl(box_prob, px >= 0 && sub < kAnchors ? kAnchors * px + sub : 0);
            if (scanned) {
                const float bst = sub == 0 ? best[0] : (sub == 1 ? best[1] : best[2]);
                const int bc = sub == 0 ? bcls[0] : (sub == 1 ? bcls[1] : bcls[2]);
                float conf = bp * bst;
                // conf >= 0 marks "kept" in pass 2; a NaN product (NaN logits) must stay a kept record as in the reference
                if (!(conf >= 0.0f)) conf = __builtin_nanf("");
                const size_t o = ((size_t)b * total_cells + g0 + px) * kAnchors + sub;
                score[o] = conf;
                cls_out[o] = bc;
            }
        }
    }

    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    trtx::workgroup_count(&s_cnt, lane == 0 ? (kDarknet ? nkept : __popcll(mask)) : 0);
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&chunk_cnt[b * n_chunks + (blockIdx.x * kBlockCells) / kChunk], s_cnt);
}

// Pass 2: anchor_emit_kernel's ordered compaction, one thread per cell (0..3 records each); the box values come from the cell's row.
// kDet: floats per record, 38 (YOLOv5) or 6 (YOLOv7), of which floats 0 .. 5 are written, or 7 (Darknet), all written.
template <typename T, int kDet>
__global__ __launch_bounds__(kChunk) void anchor_head_emit_kernel(HeadTable t, int info, int total_cells, int net_w, int net_h,
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
        const T* cur = static_cast<const T*>(t.in[l]) + ((size_t)b * cells + e) * t.ld[l];
#pragma unroll
        for (int k = 0; k < kAnchors; ++k) {
            if (!(sc[k] >= 0.0f || sc[k] != sc[k])) continue;
            if (slot < max_out) {
                const T* a = cur + k * info;
                float* det = out + 1 + (size_t)slot * kDet;
                if constexpr (kDet == 7) {
                    // yolov4 yololayer.cu:187-197, operation for operation
                    det[0] = (col + logist_darknet((float)a[0])) * net_w / gw;
                    det[1] = (row + logist_darknet((float)a[1])) * net_h / gh;
                    det[2] = expf((float)a[2]) * t.anchors[l][2 * k];
                    det[3] = expf((float)a[3]) * t.anchors[l][2 * k + 1];
                    det[4] = logist_darknet((float)a[4]);
                    det[5] = (float)cls_in[((size_t)b * total_cells + g) * kAnchors + k];
                    det[6] = sc[k];
                } else {
                    // yolov5 yololayer.cu:199-206, yolov7 yololayer.cu:196-203, operation for operation
                    det[0] = (col - 0.5f + 2.0f * logist((float)a[0])) * net_w / gw;
                    det[1] = (row - 0.5f + 2.0f * logist((float)a[1])) * net_h / gh;
                    float bw = 2.0f * logist((float)a[2]);
                    bw = bw * bw * t.anchors[l][2 * k];
                    float bh = 2.0f * logist((float)a[3]);
                    bh = bh * bh * t.anchors[l][2 * k + 1];
                    det[2] = bw;
                    det[3] = bh;
                    det[4] = sc[k];
                    det[5] = (float)cls_in[((size_t)b * total_cells + g) * kAnchors + k];
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

// the planar plugin's planes: the same for both families
size_t head_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    return trtx_yolov5_decode_workspace(batch, grid_w, grid_h, n_levels);
}

template <int kDet>
int32_t head_decode(const char* entry, const void* const* heads, const int* ld, int elem_bytes, int n_levels, int batch, int classes, int net_h,
                    int net_w, const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output, void* workspace,
                    size_t workspace_bytes, hipStream_t stream) {
    if (n_levels < 1 || n_levels > kMaxLevels || batch < 1 || classes < 1 || max_out < 1 || !heads || !ld || !grid_w || !grid_h || !anchors ||
        !output || !workspace)
        return TRTX_ERR_INVALID;
    const int info = 5 + classes;
    // every refusal comes before the first write to the workspace
    for (int i = 0; i < n_levels; ++i)
        if (grid_w[i] < 1 || grid_h[i] < 1 || !heads[i] || ld[i] < kAnchors * info) return TRTX_ERR_INVALID;
    if (workspace_bytes < head_workspace(batch, grid_w, grid_h, n_levels)) return TRTX_ERR_WORKSPACE;
    HeadTable t{};
    t.n_levels = n_levels;
    int off = 0;
    for (int i = 0; i < n_levels; ++i) {
        t.in[i] = heads[i];
        t.ld[i] = ld[i];
        t.vec[i] = ld[i] % (16 / elem_bytes) == 0 && (reinterpret_cast<uintptr_t>(heads[i]) & 15) == 0;
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
    if (hipMemsetAsync(chunk_cnt, 0, (size_t)batch * n_chunks * sizeof(int), stream) != hipSuccess) return TRTX_ERR_HIP;
    const int out_elem = 1 + max_out * kDet;
    const dim3 sgrid((total_cells + kBlockCells - 1) / kBlockCells, batch), egrid(n_chunks, batch);
    if (elem_bytes == 2) {
        hipLaunchKernelGGL((anchor_head_score_kernel<_Float16, kDet == 7>), sgrid, dim3(kScoreBlock), 0, stream, t, info, total_cells, score, cls, chunk_cnt, n_chunks);
        hipLaunchKernelGGL((anchor_head_emit_kernel<_Float16, kDet>), egrid, dim3(kChunk), 0, stream, t, info, total_cells, net_w, net_h, score, cls, chunk_cnt,
                           n_chunks, max_out, out_elem, output);
    } else {
        hipLaunchKernelGGL((anchor_head_score_kernel<float, kDet == 7>), sgrid, dim3(kScoreBlock), 0, stream, t, info, total_cells, score, cls, chunk_cnt, n_chunks);
        hipLaunchKernelGGL((anchor_head_emit_kernel<float, kDet>), egrid, dim3(kChunk), 0, stream, t, info, total_cells, net_w, net_h, score, cls, chunk_cnt,
                           n_chunks, max_out, out_elem, output);
    }
    return trtx::check_launch(entry);
}

}  // namespace

// score / class planes [batch][cells][3] and one candidate count per 512 cells: the plugin's workspace
extern "C" size_t trtx_yolov5_head_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    return head_workspace(batch, grid_w, grid_h, n_levels);
}

extern "C" size_t trtx_yolov7_head_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    return head_workspace(batch, grid_w, grid_h, n_levels);
}

extern "C" size_t trtx_darknet_head_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels) {
    return head_workspace(batch, grid_w, grid_h, n_levels);
}

extern "C" int32_t trtx_yolov5_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                                void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head_decode<38>("trtx_yolov5_head_decode_nhwc", heads, ld, 2, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, output, workspace,
                            workspace_bytes, stream);
}

extern "C" int32_t trtx_yolov5_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                    const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                                    void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head_decode<38>("trtx_yolov5_head_decode_nhwc", heads, ld, 4, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, output, workspace,
                            workspace_bytes, stream);
}

extern "C" int32_t trtx_yolov7_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                                void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head_decode<6>("trtx_yolov7_head_decode_nhwc", heads, ld, 2, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, output, workspace,
                            workspace_bytes, stream);
}

extern "C" int32_t trtx_yolov7_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                    const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                                    void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head_decode<6>("trtx_yolov7_head_decode_nhwc", heads, ld, 4, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, output, workspace,
                            workspace_bytes, stream);
}

extern "C" int32_t trtx_darknet_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                 const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                                 void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head_decode<7>("trtx_darknet_head_decode_nhwc", heads, ld, 2, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, output, workspace,
                           workspace_bytes, stream);
}

extern "C" int32_t trtx_darknet_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                                     const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                                     void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return head_decode<7>("trtx_darknet_head_decode_nhwc", heads, ld, 4, n_levels, batch, classes, net_h, net_w, grid_w, grid_h, anchors, max_out, output, workspace,
                           workspace_bytes, stream);
}
