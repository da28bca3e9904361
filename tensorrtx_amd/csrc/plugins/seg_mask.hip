// Mask assembly of the seg programs for gfx950 (MI355X): kept detections x prototypes -> masks at prototype resolution.
//
// Replaces the coefficient loop of the reference's host process_mask (yolov5/src/postprocess.cpp:94-120, yolov8/yolov8_seg.cpp:17-53,
// yolo11/yolo11_seg.cpp:17-53: the same loop), which runs on a proto tensor copied to the host.  Per kept detection, in NMS emission
// order:
//   r = get_downscale_rect(bbox, scale)                     in fp32 as written there; box_format 0: centre boxes and round() (yolov5),
//                                                           1: corner boxes clamped to the network size and int() (yolov8 / yolo11)
//   inside r:  e = sum_j mask[j] * proto[j][y][x], j = 0 .. 31 ascending, fp32, no FMA;  value = 1 / (1 + expf(-e))
//   the rest of the plane is 0.0f (cv::Mat::zeros), written by the same kernel.
// cv::resize, scale_mask and drawing stay with the caller.
// Two stated departures: the reference writes through cv::Mat::at without a bounds check (undefined for a rect outside the matrix):
// here the rect is intersected with the plane; and a rect with a non-finite edge (the int conversion of which is undefined) is empty.
// Edges beyond +-2^29 saturate there before x + width is formed, so the int sum cannot overflow.
//
// Mapping: lanes run along x, a wave takes one (detection, row) at a time and a workgroup of four waves kRows rows.  Every plane load
// is one coalesced row segment, the 32 coefficients and the box are wave-uniform loads.  With mask_w % 4 == 0 and 16-byte aligned
// bases a lane owns four pixels (16-byte loads and stores), else one.  Waves of slots at or beyond the kept count exit.  No
// workspace, no atomics, no host synchronisation: the launch can be captured in a graph.
// The traffic is a plane written once (mask_h * mask_w * 4 bytes per detection) and 128 bytes of proto per rect pixel, re-read per
// detection out of L2 / Infinity Cache.  The one measurement taken (a sparse keep list: 370 of 20480 workgroups had a
// detection) found the launch 25x off those bytes, bound by dispatching workgroups that exit at once; a dense keep list was not measured.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.h"
#include "decode_common.h"

namespace {

constexpr int kCoef = 32;    // Detection::mask[32]
constexpr int kCoefOff = 6;  // bbox[4], conf, class_id precede the coefficients in the 38-float (yolov5) and the 90-float (yolov8) record
constexpr int kWaves = 4;
constexpr int kRows = 16;    // rows per workgroup: four per wave

struct Rect {
    int x0, y0, x1, y1;   // [x0, x1) x [y0, y1), already intersected with the plane; empty when x0 >= x1 or y0 >= y1
};

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN

__device__ __forceinline__ int to_int_sat(float v) {   // v is finite or +-inf here
    return (int)fminf(fmaxf(v, -536870912.0f), 536870912.0f);
}

// the two get_downscale_rect bodies, operation for operation in fp32 (this unit is compiled with -ffp-contract=off)
__device__ __forceinline__ Rect downscale_rect(const float* bbox, int box_format, float scale, int net_w, int net_h, int mask_w, int mask_h) {
    float left, top, right, bottom;
    if (box_format == 0) {
        left = bbox[0] - bbox[2] / 2;
        top = bbox[1] - bbox[3] / 2;
        right = bbox[0] + bbox[2] / 2;
        bottom = bbox[1] + bbox[3] / 2;
    } else {
        left = bbox[0];
        top = bbox[1];
        right = bbox[0] + bbox[2];
        bottom = bbox[1] + bbox[3];
        left = left < 0 ? 0 : left;
        top = top < 0 ? 0 : top;
        right = right > net_w ? net_w : right;
        bottom = bottom > net_h ? net_h : bottom;
    }
    left /= scale;
    top /= scale;
    right /= scale;
    bottom /= scale;
    Rect r{0, 0, 0, 0};
    if (!(is_finite(left) && is_finite(top) && is_finite(right) && is_finite(bottom))) return r;
    int x, y, w, h;
    if (box_format == 0) {
        x = to_int_sat(roundf(left));
        y = to_int_sat(roundf(top));
        w = to_int_sat(roundf(right - left));
        h = to_int_sat(roundf(bottom - top));
    } else {
        x = to_int_sat(truncf(left));
        y = to_int_sat(truncf(top));
        w = to_int_sat(truncf(right - left));
        h = to_int_sat(truncf(bottom - top));
    }
    r.x0 = max(x, 0);
    r.y0 = max(y, 0);
    r.x1 = min(x + w, mask_w);
    r.y1 = min(y + h, mask_h);
    return r;
}

// V pixels per lane: 4 (16-byte loads and stores; mask_w % 4 == 0, aligned bases) or 1
template <int V>
__global__ __launch_bounds__(kWaves * 64) void seg_mask_kernel(const float* __restrict__ decode_out, int det_floats, int box_format,
                                                               const int32_t* __restrict__ keep_idx, const int32_t* __restrict__ keep_cnt,
                                                               int max_out, int max_keep, const float* __restrict__ proto, int mask_h,
                                                               int mask_w, int net_h, int net_w, float scale, float* __restrict__ masks) {
    const int b = blockIdx.z, d = blockIdx.y;
    const int kept = min(keep_cnt[b], min(max_keep, max_out));
    if (d >= kept) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = keep_idx[(size_t)b * max_out + d];
    Rect r{0, 0, 0, 0};
    const float* det = nullptr;
    if (idx >= 0 && idx < max_out) {   // a slot outside the record array gives an empty plane, never a read
        det = decode_out + (size_t)b * (1 + (size_t)max_out * det_floats) + 1 + (size_t)idx * det_floats;
        r = downscale_rect(det, box_format, scale, net_w, net_h, mask_w, mask_h);
    }
    const size_t plane = (size_t)mask_h * mask_w;
    const float* pr = proto + (size_t)b * kCoef * plane;
    float* out = masks + ((size_t)b * max_keep + d) * plane;
    const int y_end = min((int)(blockIdx.x + 1) * kRows, mask_h);
    for (int y = blockIdx.x * kRows + wave; y < y_end; y += kWaves) {
        const bool row_in = y >= r.y0 && y < r.y1 && r.x0 < r.x1;
        for (int x = lane * V; x < mask_w; x += 64 * V) {
            float e[V];
#pragma unroll
            for (int v = 0; v < V; ++v) e[v] = 0.0f;
            if (row_in && x < r.x1 && x + V > r.x0) {
                const float* p = pr + (size_t)y * mask_w + x;
#pragma unroll 8
                for (int j = 0; j < kCoef; ++j) {
                    const float c = det[kCoefOff + j];
                    if constexpr (V == 4) {
                        const float4 q = *reinterpret_cast<const float4*>(p + (size_t)j * plane);
                        e[0] += c * q.x;
                        e[1] += c * q.y;
                        e[2] += c * q.z;
                        e[3] += c * q.w;
                    } else {
                        e[0] += c * p[(size_t)j * plane];
                    }
                }
#pragma unroll
                for (int v = 0; v < V; ++v) e[v] = (x + v >= r.x0 && x + v < r.x1) ? trtx::logist(e[v]) : 0.0f;
            }
            float* o = out + (size_t)y * mask_w + x;
            if constexpr (V == 4)
                *reinterpret_cast<float4*>(o) = make_float4(e[0], e[1], e[2], e[3]);
            else
                o[0] = e[0];
        }
    }
}

}  // namespace

extern "C" int32_t trtx_seg_masks(const float* decode_out, int det_floats, int box_format, const int32_t* keep_idx, const int32_t* keep_cnt,
                                  int batch, int max_out, int max_keep, const float* proto, int mask_h, int mask_w, int net_h, int net_w,
                                  float* masks, hipStream_t stream) {
    if (!decode_out || !keep_idx || !keep_cnt || !proto || !masks) return TRTX_ERR_INVALID;
    if (det_floats != 38 && det_floats != trtx::kYoloDetFloats) return TRTX_ERR_INVALID;
    if (box_format != 0 && box_format != 1) return TRTX_ERR_INVALID;
    if (batch < 1 || batch > 65535 || max_out < 1 || max_keep < 1 || max_keep > 65535 || mask_h < 1 || mask_w < 1 || net_h < 1 || net_w < 1)
        return TRTX_ERR_INVALID;
    // process_mask's scale is the literal 4 in all three programs: prototypes at a quarter of the network size, nothing else
    if (net_w % mask_w || net_h % mask_h || net_w / mask_w != net_h / mask_h || net_w / mask_w != 4) return TRTX_ERR_INVALID;
    if ((size_t)mask_h * mask_w > (size_t)1 << 30) return TRTX_ERR_INVALID;
    const float scale = (float)(net_w / mask_w);
    const dim3 grid((mask_h + kRows - 1) / kRows, max_keep, batch);
    const bool vec = mask_w % 4 == 0 && (reinterpret_cast<uintptr_t>(masks) | reinterpret_cast<uintptr_t>(proto)) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(seg_mask_kernel<4>, grid, dim3(kWaves * 64), 0, stream, decode_out, det_floats, box_format, keep_idx, keep_cnt, max_out,
                           max_keep, proto, mask_h, mask_w, net_h, net_w, scale, masks);
    else
        hipLaunchKernelGGL(seg_mask_kernel<1>, grid, dim3(kWaves * 64), 0, stream, decode_out, det_floats, box_format, keep_idx, keep_cnt, max_out,
                           max_keep, proto, mask_h, mask_w, net_h, net_w, scale, masks);
    return trtx::check_launch("trtx_seg_masks");
}
