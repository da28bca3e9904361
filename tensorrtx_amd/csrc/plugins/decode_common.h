// Device pieces shared by the decode plugins (yolo_decode.hip, anchor_decode.hip, anchor_head.hip, yolo9_decode.hip, yolo9_head.hip, the
// RetinaFace decode of det_plugins.hip): the sigmoid and the level lookup every one of them needs, and pass 1 of their deterministic
// two-pass compaction, in which every workgroup leaves its candidate count in chunk_cnt[image][chunk].  Pass 2 (slot = candidates of
// earlier chunks + earlier waves + earlier lanes) stays written out in each emit kernel: every form of it shared as a helper across
// DIFFERENT kernels that was tried moved those kernels' instruction streams, and they are kept instruction for instruction.  One kernel
// as a template on its record length is another matter: anchor_decode.hip and anchor_head.hip serve YOLOv5 (38 floats) and YOLOv7 (6)
// from one source each, and the instantiations kept the streams of the copies they replaced (profiles/anchor_units_isa.txt).  All
// kernels here are wave64.
#pragma once
#include <hip/hip_runtime.h>

namespace trtx {

__device__ __forceinline__ float logist(float x) {
    return 1.0f / (1.0f + expf(-x));
}

// The Darknet plugins' Logist (yolov4/yololayer.cu:154, equal in yolov3 and yolov3-tiny): "1./(1. + exp(-data))" on a float is a float
// exp, then the add and the divide in double, rounded to float on return.
__device__ __forceinline__ float logist_darknet(float x) {
    return (float)(1.0 / (1.0 + (double)expf(-x)));
}

// level of global cell g; cell_off holds the cumulative cell offsets of the levels (cell_off[n_levels] = all cells)
template <int N>
__device__ __forceinline__ int find_level(const int (&cell_off)[N], int n_levels, int g) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < N - 1; ++i)
        if (i < n_levels && g >= cell_off[i]) l = i;
    return l;
}

// sum over the wave, valid in lane 0
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// Pass 1: adds `mine` to the workgroup's LDS counter, which was zeroed before an earlier barrier; when it returns, *s_cnt is the
// workgroup's total.  Callers with a count in every thread pass lane 0 the wave_sum and the other lanes 0.
__device__ __forceinline__ void workgroup_count(int* s_cnt, int mine) {
    if (mine) atomicAdd(s_cnt, mine);
    __syncthreads();
}

}  // namespace trtx
