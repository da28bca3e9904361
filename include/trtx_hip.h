/*
 * trtx_hip.h — C ABI of libtrtx_hip.so, the MI355X (gfx950) runtime behind the tensorrtx
 * network-definition / plugin surface.
 *
 * Plain C: opaque handles, plain pointers and sizes, int32_t status returns.  No C++ or torch types.
 * Device pointers are ordinary hipMalloc'd addresses owned by the caller; `stream` is a hipStream_t.
 *
 * Section 1 (this part): the detection plugin operators — each entry point replaces the `enqueue`
 * body of one reference plugin (file:line cited per function) and is what a cgo/JNI/ctypes binding
 * or a reference-style IPluginV2::enqueue override would call.
 * Section 2: network-definition builder / engine / execution-context API (mirrors the nvinfer1
 * objects the reference host code uses; see include/NvInfer.h for the C++ shim on top of it).
 */
#ifndef TRTX_HIP_H_
#define TRTX_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t without dragging the HIP headers into pure-C callers. */
#ifndef TRTX_NO_HIP_TYPES
struct ihipStream_t;
typedef struct ihipStream_t* trtx_stream_t;
#endif

/* ---- status codes ---------------------------------------------------------------------------- */
#define TRTX_ABI_VERSION 1
#define TRTX_OK 0
#define TRTX_ERR_INVALID 1     /* bad argument */
#define TRTX_ERR_HIP 2         /* a HIP call or kernel launch failed (message on stderr) */
#define TRTX_ERR_WORKSPACE 3   /* workspace too small */
#define TRTX_ERR_UNSUPPORTED 4 /* configuration outside what the kernels implement */
#define TRTX_ERR_NO_DEVICE 5   /* no gfx950 device visible: the runtime never falls back to the CPU */
#define TRTX_ERR_IO 6          /* file / parse error (.wts, plan) */
#define TRTX_ERR_STATE 7       /* call order violated (e.g. enqueue before build) */

const char* trtx_status_string(int32_t status);
/* ABI version of this header; bumped on any incompatible change. */
int32_t trtx_abi_version(void);
/* Number of visible HIP devices (0 when none; never an error). */
int32_t trtx_device_count(void);

/* ============================== Section 1: plugin operators ================================== */

/*
 * YOLOv8 anchor-free decode.  Replaces YoloLayerPlugin::enqueue -> forwardGpu -> CalDetection
 * (reference yolov8/plugin/yololayer.cu:167-172, 178-220, 282-316).
 *   inputs[l]  device, fp32 [batch][4+classes][ (net_h/strides[l]) * (net_w/strides[l]) ]  (CHW linear)
 *   output     device, fp32 [batch][1 + max_out*90]; output[b][0] = candidate count (clamped to
 *              max_out), then Detection records of 90 floats (yolov8/include/types.h:4-12) of which
 *              bbox[4] (xyxy), conf, class_id are written.  Candidates appear in (level, cell) order.
 *   `inputs` and `strides` are HOST arrays (as in IPluginV2::enqueue's `inputs`).
 */
size_t trtx_yolo_decode_workspace(int batch, int net_h, int net_w, const int* strides, int n_levels);
int32_t trtx_yolo_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                         const int* strides, int max_out, float* output, void* workspace, size_t workspace_bytes,
                         trtx_stream_t stream);

/* trtx_yolo_decode with the optional branches of CalDetection (yololayer.cu:222-279): inputs [batch][4 + classes (+32 seg)
 * (+3*n_kpt pose) (+1 obb)][cells]; seg copies the 32 mask coefficients into Detection::mask, pose decodes n_kpt keypoints
 * ((2*v + col|row) * stride, sigmoid confidence, -1 triple when below kpt_conf or outside the box), obb rotates the box
 * centre by (sigmoid(a) - 0.25) * pi and stores cx, cy, w, h + Detection::angle. */
int32_t trtx_yolo_decode_ex(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                            const int* strides, int max_out, int n_kpt, float kpt_conf, int is_seg, int is_pose, int is_obb,
                            float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * Fused DFL + YOLOv8 decode on the detect head's own NHWC fp16 output (what the engine uses instead of the
 * shuffle/slice/softmax/conv/concat chain of yolov8/src/block.cpp:239-257 + model.cpp:263-303 followed by
 * YoloLayerPlugin::enqueue).  heads[l]: device fp16 [batch][cells_l][ld[l]], channels [0,64) = 4x16 DFL
 * bins, [64, 64+classes) = class logits; dfl_weights: device fp32[16] (model.22.dfl.conv.weight).
 * Output format and candidate order are those of trtx_yolo_decode.  classes % 8 == 0.
 * Refused with nothing written: TRTX_ERR_INVALID for a null pointer, n_levels outside 1..8, batch / max_out / net_h / net_w < 1, a
 * stride < 1 or a class count that is no positive multiple of 8; TRTX_ERR_WORKSPACE; TRTX_ERR_UNSUPPORTED for a base or an ld[l] that
 * is no 16-byte multiple, or ld[l] < 64 + classes.  The workspace size of a geometry refused here is 0.
 */
size_t trtx_yolo_head_decode_workspace(int batch, int net_h, int net_w, const int* strides, int n_levels);
int32_t trtx_yolo_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes,
                                   int net_h, int net_w, const int* strides, const float* dfl_weights, int max_out,
                                   float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* The same on the NHWC fp32 head tensors of an fp32 engine (a build without BuilderFlag::kFP16, yolov8/src/model.cpp:314-324): ld in floats. */
int32_t trtx_yolo_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes,
                                   int net_h, int net_w, const int* strides, const float* dfl_weights, int max_out,
                                   float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * Fused DFL + YOLO11 seg / pose / obb decode on the NHWC fp16 head and branch tensors of an explicit-batch engine: what the engine
 * uses instead of the flatten / slice / DFL chain, the cv4 branch's reshape and the [dfl, classes, branch] concat of
 * yolo11/src/model.cpp:595-756 (seg), 960-1060 (pose), 1265-1358 (obb) followed by YoloLayerPlugin::enqueue (yololayer.cu:178-279).
 * heads[l]: [batch][cells_l][ld[l]] as for trtx_yolo_head_decode_nhwc, any classes >= 1 (ld[l] >= 64 + classes);
 * branches[l]: [batch][cells_l][branch_ld[l]], channels [0, extra) = the cv4 convolution's output (32 mask coefficients,
 * 3 * n_kpt keypoint values or 1 angle logit).  Exactly one of is_seg / is_pose / is_obb.  Output format, candidate order and
 * branch arithmetic are those of trtx_yolo_decode_ex; workspace: trtx_yolo_head_decode_workspace.
 */
int32_t trtx_yolo_task_head_decode_nhwc(const void* const* heads, const int* ld, const void* const* branches, const int* branch_ld,
                                        int n_levels, int batch, int classes, int net_h, int net_w, const int* strides,
                                        const float* dfl_weights, int max_out, int is_seg, int is_pose, int is_obb, int n_kpt,
                                        float kpt_conf, float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* The same on the NHWC fp32 head and branch tensors of an fp32 engine (yolo11/src/model.cpp:785-796 without kFP16): ld in floats. */
int32_t trtx_yolo_task_head_decode_nhwc_f32(const void* const* heads, const int* ld, const void* const* branches, const int* branch_ld,
                                            int n_levels, int batch, int classes, int net_h, int net_w, const int* strides,
                                            const float* dfl_weights, int max_out, int is_seg, int is_pose, int is_obb, int n_kpt,
                                            float kpt_conf, float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);

/*
 * YOLOv10 YoloLayer.  Replaces YoloLayerPlugin::forwardGpu + CalDetection of yolov10/plugin/yololayer.cu:157-240.  The per-cell
 * arithmetic is trtx_yolo_decode's (sigmoid, strict-'>' argmax from (0.0, class 0), dropped below 0.1, (col + .5 -/+ d) * stride); the
 * record is Detection = bbox[4] (xyxy), conf, class_id (yolov10/include/types.h), 6 floats.
 *   inputs[l]  device, fp32 [batch][4 + classes][(net_h / strides[l]) * (net_w / strides[l])]
 *   output     device, fp32 [batch][1 + max_out * 6]: count (clamped to max_out), then the records in canonical (level, cell) order.
 *              Nothing of a row is written behind its records.
 * Workspace: trtx_yolo_decode_workspace.  TRTX_ERR_INVALID, before the device is touched, for a null pointer (a level's too),
 * n_levels outside 1..8, batch / classes / max_out / net_h / net_w < 1 or a stride < 1; TRTX_ERR_WORKSPACE.
 */
int32_t trtx_yolov10_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w, const int* strides,
                            int max_out, float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * Fused YOLOv10 head: the DFL chain (yolov10/src/block.cpp:214-233, model.cpp:202-252) and trtx_yolov10_decode on the detect head's own
 * NHWC output, read exactly as trtx_yolo_head_decode_nhwc reads it (classes % 8 == 0) or as trtx_yolo_task_head_decode_nhwc does (any
 * other class count >= 1: the last classes % 8 logits one by one, so the padding channels never reach the argmax).
 *   heads[l]   device fp16 [batch][cells_l][ld[l]]: channels [0, 64) DFL bins, [64, 64 + classes) logits; ld[l] >= 64 + classes and,
 *              like the base, a 16-byte multiple (else TRTX_ERR_UNSUPPORTED).  Output and order: trtx_yolov10_decode.
 */
size_t trtx_yolov10_head_decode_workspace(int batch, int net_h, int net_w, const int* strides, int n_levels);
int32_t trtx_yolov10_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                      const int* strides, const float* dfl_weights, int max_out, float* output, void* workspace,
                                      size_t workspace_bytes, trtx_stream_t stream);
/* The same on the NHWC fp32 head tensors of an fp32 engine: ld in floats. */
int32_t trtx_yolov10_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                          const int* strides, const float* dfl_weights, int max_out, float* output, void* workspace,
                                          size_t workspace_bytes, trtx_stream_t stream);
/*
 * The device side of YOLOv10's get_topk / batch_topk (yolov10/src/postprocess.cpp:35-52), which is all the post-processing the
 * NMS-free head has.  decode_out and out: device, fp32 [batch][1 + max_out * 6], two different buffers.
 *   topk <= 0  the reference (its `topk` argument is unused): the records with conf > conf_thresh, in slot order
 *   topk > 0   of those, the topk highest confidences, by descending conf, ties in slot order (a stable rank)
 * out[b][0] = records written; nothing is written behind them.  A NaN conf fails the '>'; a header above max_out is clamped.
 * max_out <= 1024, beyond it TRTX_ERR_UNSUPPORTED like trtx_yolov7_nms; TRTX_ERR_INVALID for a null pointer, out == decode_out,
 * batch < 1 or max_out < 1.  No workspace.
 */
int32_t trtx_yolov10_topk(const float* decode_out, int batch, int max_out, float conf_thresh, int topk, float* out, trtx_stream_t stream);

/*
 * Class-aware greedy NMS over the decode buffer.  Replaces host batch_nms()/nms()
 * (reference yolov8/src/postprocess.cpp:71-129; call site yolov8/yolov8_det.cpp:240).
 *   decode_out device, fp32 [batch][1 + max_out*90]  (output of trtx_yolo_decode)
 *   keep_idx   device, int32 [batch][max_out]  decode slot of every kept detection, in the reference's
 *              emission order (class ascending, conf descending, bbox[0] ascending)
 *   keep_cnt   device, int32 [batch]
 *   keep_det   device, fp32 [batch][max_out][6] = x1,y1,x2,y2,conf,class of the kept boxes; may be NULL
 *   workspace  device, >= trtx_yolo_nms_workspace(batch) bytes, 16-byte aligned (sorted records + the 1024x1024-bit
 *              suppression matrix per image)
 * max_out <= 1024.
 */
size_t trtx_yolo_nms_workspace(int batch);
int32_t trtx_yolo_nms(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh,
                      int32_t* keep_idx, int32_t* keep_cnt, float* keep_det, void* workspace, size_t workspace_bytes,
                      trtx_stream_t stream);


/*
 * Anchor-based YoloLayer (YOLOv5 / v3 / v4 family; YOLOv7's 6-float records: trtx_yolov7_decode below) - the reference's
 * yolov5/plugin/yololayer.cu:161-227.
 *   inputs     n_levels device pointers, fp32 [batch][3 * (5 + classes (+ 32 if is_segmentation))][grid_h * grid_w]
 *   grid_w/h   per level (YoloKernel::width / height, yolov5/src/types.h:5-9); anchors: n_levels x 6 floats (w0,h0,w1,h1,w2,h2)
 *   output     device, fp32 [batch][1 + max_out * 38]: count (clamped to max_out), then Detection records of 38 floats
 *              (yolov5/src/types.h:11-16): cx, cy, w, h, conf = obj * cls, class_id, mask[32]
 * Candidates with sigmoid(obj) >= 0.1 (kIgnoreThresh) in canonical (level, cell, anchor) order (the reference: atomicAdd race).
 */
size_t trtx_yolov5_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels);
int32_t trtx_yolov5_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                           const int* grid_w, const int* grid_h, const float* anchors, int max_out, int is_segmentation,
                           float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * Fused anchor head: trtx_yolov5_decode (detection, no mask coefficients) on the detect convolutions' own NHWC output, what the engine
 * uses instead of one layout pass per level followed by YoloLayerPlugin::enqueue (yolov5/src/model.cpp:331-343, yololayer.cu:161-227).
 *   heads[l]   device fp16 [batch][grid_h[l] * grid_w[l]][ld[l]]; channel k * (5 + classes) + j of a pixel = value j of anchor k
 *              (x, y, w, h, objectness, class logits); ld[l] >= 3 * (5 + classes), channels beyond that are padding and never read
 *              into a result.  Rows whose base and ld are multiples of 16 bytes are read with 16-byte loads, others element-wise.
 *   `heads`, `ld`, `grid_w`, `grid_h` and `anchors` are HOST arrays.  Output, candidate order and arithmetic: trtx_yolov5_decode.
 */
size_t trtx_yolov5_head_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels);
int32_t trtx_yolov5_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                     const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                     void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* The same on the NHWC fp32 head tensors of an fp32 engine: ld in floats. */
int32_t trtx_yolov5_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                         const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                         void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * YOLOv7 YoloLayer - the reference's yolov7/plugin/yololayer.cu:152-207 (CalDetection + forwardGpu).  The arithmetic is the YOLOv5
 * plugin's; the record is not: Detection is bbox[4], conf, class_id (yolov7/include/types.h), 6 floats, and there is no mask branch.
 *   inputs     n_levels (1..8) device pointers, fp32 [batch][3 * (5 + classes)][grid_h * grid_w]
 *   grid_w/h   per level (YoloKernel::width / height); anchors: n_levels x 6 floats (w0,h0,w1,h1,w2,h2)
 *   output     device, fp32 [batch][1 + max_out * 6]: count (clamped to max_out), then records cx, cy, w, h, conf = obj * cls,
 *              class_id at float 1 + 6 * slot.  Nothing of a row is written behind its records.
 * Candidates with !(sigmoid(obj) < 0.1) in canonical (level, cell, anchor) order (the reference: atomicAdd race).
 */
size_t trtx_yolov7_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels);
int32_t trtx_yolov7_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                           const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output, void* workspace,
                           size_t workspace_bytes, trtx_stream_t stream);
/*
 * Fused YOLOv7 head: trtx_yolov7_decode on the detect convolutions' own NHWC output, what the engine uses instead of one layout pass
 * per level followed by YoloLayerPlugin::enqueue (yolov7/src/block.cpp:220-255, yololayer.cu:152-207).
 *   heads[l]   device fp16 [batch][grid_h[l] * grid_w[l]][ld[l]]; channel k * (5 + classes) + j of a pixel = value j of anchor k
 *              (x, y, w, h, objectness, class logits); ld[l] >= 3 * (5 + classes), channels beyond that are padding and never read
 *              into a result.  Rows whose base and ld are multiples of 16 bytes are read with 16-byte loads, others element-wise.
 *   `heads`, `ld`, `grid_w`, `grid_h` and `anchors` are HOST arrays.  Output, candidate order and arithmetic: trtx_yolov7_decode.
 *   A refused call (TRTX_ERR_INVALID, TRTX_ERR_WORKSPACE) writes neither the output nor the workspace.
 */
size_t trtx_yolov7_head_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels);
int32_t trtx_yolov7_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                     const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                     void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* The same on the NHWC fp32 head tensors of an fp32 engine: ld in floats. */
int32_t trtx_yolov7_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                         const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                         void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * Darknet YoloLayer (YOLOv3 / YOLOv3-tiny / YOLOv4) - the reference's yolov4/yololayer.cu:154-219 (Logist + CalDetection + forwardGpu; equal
 * in yolov3 and yolov3-tiny).
 *   inputs     n_levels (1..8) device pointers, fp32 [batch][3 * (5 + classes)][grid_h * grid_w]
 *   grid_w/h   per level; anchors: n_levels x 6 floats (w0,h0,w1,h1,w2,h2)
 *   output     device, fp32 [batch][1 + max_out * 7]: count (clamped to max_out), then Detection records (yolov4/yololayer.h:41-47)
 *              cx, cy, w, h, det_confidence, class_id, class_confidence at float 1 + 7 * slot.  Nothing of a row is written behind its records.
 * Logist(x) = 1./(1. + exp(-x)) with a float exp and a double add and divide; an anchor is dropped if max class prob < 0.1f or
 * Logist(obj) < 0.1f; cx = (col + Logist(x)) * net_w / grid_w, w = exp(tw) * anchor_w; the two probabilities are stored apart.
 * Canonical (level as passed, cell, anchor) order (the reference: atomicAdd race).
 */
size_t trtx_darknet_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels);
int32_t trtx_darknet_decode(const float* const* inputs, int n_levels, int batch, int classes, int net_h, int net_w,
                            const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output, void* workspace,
                            size_t workspace_bytes, trtx_stream_t stream);
/*
 * Fused Darknet head: trtx_darknet_decode on the detect convolutions' own NHWC output (heads, ld and refusals as
 * trtx_yolov7_head_decode_nhwc); the same records in the same order.
 */
size_t trtx_darknet_head_decode_workspace(int batch, const int* grid_w, const int* grid_h, int n_levels);
int32_t trtx_darknet_head_decode_nhwc(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                      const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                      void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* The same on the NHWC fp32 head tensors of an fp32 engine: ld in floats. */
int32_t trtx_darknet_head_decode_nhwc_f32(const void* const* heads, const int* ld, int n_levels, int batch, int classes, int net_h, int net_w,
                                          const int* grid_w, const int* grid_h, const float* anchors, int max_out, float* output,
                                          void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * YOLOv9 YoloLayer - the reference's yolov9/plugin/yololayer.cu:133-197 (CalDetection + forwardGpu).
 *   inputs     3 device pointers (strides 8 / 16 / 32), fp32 [batch][4 + classes (+ 32 if is_segmentation)][(net_h / s) * (net_w / s)]
 *   output     device, fp32 [batch][1 + max_out * 38]: count (clamped to max_out), then Detection records of 38 floats
 *              (yolov9/include/types.h): x1, y1, x2, y2, conf, class_id, mask[32]
 * Candidates with max sigmoid(class) >= 0.1 in canonical (level, cell) order (the reference: atomicAdd race).
 */
size_t trtx_yolov9_decode_workspace(int batch, int net_h, int net_w);
int32_t trtx_yolov9_decode(const float* const* inputs, int batch, int classes, int net_h, int net_w, int max_out, int is_segmentation,
                           float* output, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * Fused DDetect / DualDDetect head: DFL + trtx_yolov9_decode (detection) on the NHWC outputs of the head's last convolutions, what the
 * engine uses instead of the shuffle / softmax / conv / shuffle chain, the class reshape and the concat of yolov9/src/block.cpp:380-399,
 * 441-453 followed by YoloLayerPlugin::enqueue (yolov9/plugin/yololayer.cu:124-197).
 *   box[l]     device fp16 [batch][cells_l][box_ld[l]], channels [0, 64) = 4 sides x 16 DFL bins (the grouped 1x1 cv2.l.2)
 *   cls[l]     device fp16 [batch][cells_l][cls_ld[l]], channels [0, classes) = class logits (cv3.l.2); any classes >= 1
 *   Channels beyond those are padding and never reach a result.  dfl_weights: device fp32[16] (<detect>.dfl.conv.weight).
 *   `box`, `box_ld`, `cls`, `cls_ld` are HOST arrays of 3.  Bases and strides that are no multiples of 16 bytes, box_ld < 64 and
 *   cls_ld < classes: TRTX_ERR_UNSUPPORTED, nothing is written.  Output, candidate order and decode arithmetic: trtx_yolov9_decode.
 */
size_t trtx_yolov9_head_decode_workspace(int batch, int net_h, int net_w);
int32_t trtx_yolov9_head_decode_nhwc(const void* const* box, const int* box_ld, const void* const* cls, const int* cls_ld, int batch, int classes,
                                     int net_h, int net_w, const float* dfl_weights, int max_out, float* output, void* workspace,
                                     size_t workspace_bytes, trtx_stream_t stream);
/* The same on the NHWC fp32 tensors of an fp32 engine: ld in floats; the DFL is the un-fused chain's arithmetic to the bit. */
int32_t trtx_yolov9_head_decode_nhwc_f32(const void* const* box, const int* box_ld, const void* const* cls, const int* cls_ld, int batch, int classes,
                                         int net_h, int net_w, const float* dfl_weights, int max_out, float* output, void* workspace,
                                         size_t workspace_bytes, trtx_stream_t stream);
/* Oriented boxes (yolov8 obb): host nms_obb() on the GPU (yolov8/src/postprocess.cpp:303-393, ProbIoU, "conf <= thresh" dropped,
 * erased when probiou >= nms_thresh); keep_det is [batch][max_out][7] = cx, cy, w, h, conf, class, angle.  And the reference's
 * GPU mode for oriented boxes, cuda_decode_obb + cuda_nms_obb (yolov8/src/postprocess.cu:7-40, 113-166): out [batch][1 + max_out*8]. */
int32_t trtx_yolo_nms_obb(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh, int32_t* keep_idx,
                          int32_t* keep_cnt, float* keep_det, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
int32_t trtx_yolo_postprocess_gpu_obb(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh, float* out,
                                      trtx_stream_t stream);
/* YOLOv5 host nms() / batch_nms() on the GPU (yolov5/src/postprocess.cpp:30-80): centre-format IoU, conf <= thresh dropped,
 * class-wise greedy suppression in conf-descending order.  Same outputs / workspace as trtx_yolo_nms; records are 38 floats. */
int32_t trtx_yolov5_nms(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh, int32_t* keep_idx,
                        int32_t* keep_cnt, float* keep_det, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* YOLOv9 host nms() / batch_nms() on the GPU (yolov9/src/postprocess.cpp:48-83): records of 38 floats with corner boxes; conf <= thresh
 * dropped, each box turned into centre format by the reference's four fp32 operations (:59-62), then the YOLOv5 iou and conf-descending
 * class-wise suppression.  Same outputs / workspace as trtx_yolov5_nms; keep_det holds the centre-format boxes, as the reference's res. */
int32_t trtx_yolov9_nms(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh, int32_t* keep_idx,
                        int32_t* keep_cnt, float* keep_det, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* YOLOv7 host nms() / batch_nms() on the GPU (yolov7/src/postprocess.cpp:48-89): trtx_yolov5_nms on records of 6 floats
 * ([batch][1 + max_out * 6], the YOLOv7 engines' "prob").  Same outputs / workspace: keep_idx, keep_cnt, keep_det[batch][max_out][6]. */
int32_t trtx_yolov7_nms(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh, int32_t* keep_idx,
                        int32_t* keep_cnt, float* keep_det, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/* Darknet host nms() on the GPU (yolov4/yolov4.cpp:81-124, equal in yolov3 and yolov3-tiny): trtx_yolov5_nms on records of 7 floats
 * (det_confidence at float 4 is what is thresholded and sorted by, class_id at float 5).  keep_det[batch][max_out][6]: floats 0-5.
 * The reference's thresholds are 0.5 / 0.4 (yolov3, yolov4) and 0.4 / 0.5 (yolov3-tiny). */
int32_t trtx_darknet_nms(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh, int32_t* keep_idx,
                         int32_t* keep_cnt, float* keep_det, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
/*
 * Mask assembly of the seg programs: the coefficient x prototype loop of the host process_mask with its get_downscale_rect
 * (yolov5/src/postprocess.cpp:94-120; yolov8/yolov8_seg.cpp:17-53 and yolo11/yolo11_seg.cpp:17-53, one body), on the engine's
 * device buffers.  cv::resize, scale_mask and drawing stay with the caller.
 *   decode_out  device fp32 [batch][1 + max_out * det_floats], the engine's decode binding; det_floats 38 (yolov5) or 90 (yolov8 /
 *               yolo11): bbox is floats 0-3 and the 32 coefficients floats 6-37 of a record in both
 *   keep_idx    device [batch][max_out], keep_cnt device [batch]: the outputs of trtx_yolov5_nms / trtx_yolo_nms
 *   proto       device fp32 [batch][32][mask_h][mask_w], the engine's proto binding; net_w / mask_w must be an integer equal to
 *               net_h / mask_h and to the reference's 4, anything else is TRTX_ERR_INVALID
 *   box_format  0: centre boxes, Rect(round(left), round(top), round(right - left), round(bottom - top)) (yolov5);
 *               1: corner boxes clamped to [0, net], the same with int() truncation (yolov8 / yolo11); fp32 as written there
 *   masks       device fp32 [batch][max_keep][mask_h][mask_w]: slot d of image b is kept detection d in NMS emission order for
 *               d < min(keep_cnt[b], max_keep), 1 / (1 + expf(-sum_j coef[j] * proto[j][y][x])) (j ascending, fp32) inside the rect
 *               and 0.0f elsewhere; later slots are not written.
 * Unlike the reference (cv::Mat::at, unchecked) the rect is intersected with the plane, and a rect with a non-finite edge is empty.
 * One launch, no workspace, no synchronisation.
 */
int32_t trtx_seg_masks(const float* decode_out, int det_floats, int box_format, const int32_t* keep_idx, const int32_t* keep_cnt, int batch,
                       int max_out, int max_keep, const float* proto, int mask_h, int mask_w, int net_h, int net_w, float* masks,
                       trtx_stream_t stream);

/*
 * Letterbox pre-processing (the reference's cuda_preprocess / cuda_batch_preprocess, yolov8/src/preprocess.cu:7-127):
 * uint8 HWC BGR image -> fp32 CHW RGB / 255, bilinear warp-affine about the image centres, border 128.
 *   trtx_letterbox_batch   sources already on the device: src[i] device pointer, tightly packed src_w[i] x src_h[i] x 3;
 *                          dst device fp32 [batch][3][dst_h][dst_w]; ONE launch for the batch, nothing synchronises.
 *   trtx_preprocess_init / _destroy / trtx_batch_preprocess   host images (cuda_preprocess_init(max_image_size), :129-139):
 *                          pinned ring + device ring + copy stream; batch <= ring_depth.
 *   trtx_letterbox_matrix  the dst->src map the kernel uses (s2d about the centres, inverted as cv::invertAffineTransform does).
 */
void trtx_letterbox_matrix(int src_w, int src_h, int dst_w, int dst_h, float* d2s_out /* 6 floats */);
int32_t trtx_letterbox_batch(const void* const* src, const int* src_w, const int* src_h, int batch, float* dst, int dst_w, int dst_h,
                             trtx_stream_t stream);
int32_t trtx_preprocess_init(int max_image_size, int ring_depth);
void trtx_preprocess_destroy(void);
int32_t trtx_batch_preprocess(const void* const* src_host, const int* src_w, const int* src_h, int batch, float* dst, int dst_w, int dst_h,
                              trtx_stream_t stream);

/*
 * The reference's optional GPU post-processing mode "g": cuda_decode + cuda_nms (yolov8/src/postprocess.cu:42-111, call
 * site yolov8/yolov8_det.cpp:105-112; batch 1 only there, any batch here).  NOT the same result as trtx_yolo_nms: the
 * suppression is non-greedy (a box is dropped if any same-class box with higher confidence overlaps it).
 *   out  device, fp32 [batch][1 + max_out*7]: out[0] = input count, then records x1,y1,x2,y2,conf,class,keep (1/0) in input
 *        slot order; records of positions with conf < conf_thresh are all-zero.  max_out <= 1024.
 */
int32_t trtx_yolo_postprocess_gpu(const float* decode_out, int batch, int max_out, float conf_thresh, float nms_thresh,
                                  float* out, trtx_stream_t stream);

/* ---- Mish (yolov4, scaled-yolov4 and the early yolov5 samples) ------------------------------------ */
/* mish_kernel of MishPlugin::forwardGpu (reference yolov4/mish.cu:113-141): out[i] = in[i] * tanh(softplus(in[i])) over n device fp32
 * values, softplus with the reference's threshold of 20 (x > 20 -> x, x < -20 -> exp(x)), tanh spelled 2 / (1 + exp(-2y)) - 1. */
int32_t trtx_mish(const float* in, float* out, size_t n, trtx_stream_t stream);

/* ---- RetinaFace ------------------------------------------------------------------------------- */
/*
 * DecodePlugin::enqueue (reference retinaface/decode.cu:110-191).  inputs[l] (l = stride 8/16/32): device fp32
 * [batch][32][h_l*w_l] = bbox(2x4) | cls(2x2) | landmark(2x10) planes (retina_r50.cpp:197-202).
 * output: [batch][1 + anchors*15]: count, then Detection{bbox[4] xyxy px, conf, landmark[10]} (decode.h:11-15)
 * for every anchor with softmax conf > 0.02, in (level, cell, k) order.  The reference fixes INPUT_H/W at
 * compile time (decode.h:16-17); here they are arguments.
 */
size_t trtx_retina_decode_output_floats(int net_h, int net_w);
size_t trtx_retina_decode_workspace(int batch, int net_h, int net_w);
int32_t trtx_retina_decode(const float* const* inputs, int batch, int net_h, int net_w, float* output, void* workspace,
                           size_t workspace_bytes, trtx_stream_t stream);
/*
 * Host nms() of the reference (retinaface/common.hpp:91-130) on the device: conf > conf_thresh (0.1, compared in
 * double), sort by conf descending, greedy suppression with iou(+1e-6) > nms_thresh.  keep_idx [batch][max_keep]
 * = decode slots in emission order, keep_det (nullable) [batch][max_keep][15] the kept records.
 */
size_t trtx_retina_nms_workspace(int batch, int net_h, int net_w);
int32_t trtx_retina_nms(const float* decode_out, int batch, int net_h, int net_w, double conf_thresh, float nms_thresh,
                        int max_keep, int32_t* keep_idx, int32_t* keep_cnt, float* keep_det, void* workspace,
                        size_t workspace_bytes, trtx_stream_t stream);

/* ---- R-CNN (detectron2-style) plugin chain ------------------------------------------------------ */
/* rpnDecode (rcnn/RpnDecode.cu:27-143): stable descending sort of the A*h*w logits, top_n, anchor delta decode
 * + clip; empty boxes get score -FLT_MAX.  scores [batch][A*h*w], deltas [batch][A*4*h*w] (CHW planes),
 * anchors_host: host fp32 [A*4] (GenerateAnchors, rcnn.cpp:62-77). */
size_t trtx_rpn_decode_workspace(int batch, int num_anchors, int height, int width);
int32_t trtx_rpn_decode(int batch, const float* scores, const float* deltas, int height, int width, int image_height,
                        int image_width, float stride, const float* anchors_host, int num_anchors, int top_n,
                        float* out_scores, float* out_boxes, void* workspace, size_t workspace_bytes,
                        trtx_stream_t stream);
/* rpnNms (rcnn/RpnNms.cu:59-121): sort, exact greedy NMS (the reference kernel races across blocks), stable
 * re-sort, first post_nms_topk boxes.  scores [batch][pre], boxes [batch][pre][4] -> out_boxes [batch][post][4] */
size_t trtx_sorted_nms_workspace(int batch, int n);
int32_t trtx_rpn_nms(int batch, const float* scores, const float* boxes, int pre_nms_topk, int post_nms_topk,
                     float nms_thresh, float* out_boxes, void* workspace, size_t workspace_bytes,
                     trtx_stream_t stream);
/* roiAlign (rcnn/RoiAlign.cu:83-182): detectron2 ROIAlign(aligned=True), adaptive sampling when ratio == 0.
 * boxes [batch][P][4], features [batch][C][fh][fw] -> out [batch][P][C][res][res] */
int32_t trtx_roi_align(int batch, const float* boxes, const float* features, int pooler_resolution, float spatial_scale,
                       int sampling_ratio, int num_proposals, int channels, int feature_h, int feature_w, float* out,
                       trtx_stream_t stream);
/* The same operator on the engine's native layout: features NHWC fp16 [batch][fh][fw][ld_in] (channels % 8 == 0), out NHWC fp16
 * [batch * P][res][res][ld_out] - what the RoI head's convolutions consume.  Used by the fp16 engine in place of the fp32
 * plugin edge + two layout passes. */
int32_t trtx_roi_align_nhwc_f16(int batch, const float* boxes, const void* features, int ld_in, int pooler_resolution,
                                float spatial_scale, int sampling_ratio, int num_proposals, int channels, int feature_h,
                                int feature_w, void* out, int ld_out, trtx_stream_t stream);
/* ... computing only every bin_step-th bin per axis: out [batch * P][ores][ores][ld_out], ores = (res - 1) / bin_step + 1, bin (oh, ow) of
 * the output = bin (oh * bin_step, ow * bin_step) of the res x res grid, same arithmetic.  bin_step 2 is what res5.0's two 1x1 STRIDE-2
 * convolutions read of the 14 x 14 RoI features (rcnn/backbone.hpp:9,110-117 STRIDE_IN_1X1; rcnn/rcnn.cpp:147-163): the engine emits
 * the 7 x 7 grid and runs those convolutions at stride 1 - three quarters of the RoIAlign samples and writes are gone. */
int32_t trtx_roi_align_nhwc_f16_strided(int batch, const float* boxes, const void* features, int ld_in, int pooler_resolution,
                                        float spatial_scale, int sampling_ratio, int num_proposals, int channels, int feature_h,
                                        int feature_w, void* out, int ld_out, int bin_step, trtx_stream_t stream);
/* predictorDecode (rcnn/PredictorDecode.cu:24-110): sort N*C scores, top N (n, cls) pairs, weighted delta decode.
 * The reference clips y2 with image_width (line 99); kept for parity. */
size_t trtx_predictor_decode_workspace(int batch, int num_boxes, int num_classes);
int32_t trtx_predictor_decode(int batch, const float* scores, const float* deltas, const float* proposals, int num_boxes,
                              int num_classes, int image_height, int image_width, const float* bbox_reg_weights_host,
                              float* out_scores, float* out_boxes, float* out_classes, void* workspace,
                              size_t workspace_bytes, trtx_stream_t stream);
/* batchedNms (rcnn/BatchedNms.cu:28-162): class-aware; method 0 hard, 1 soft-NMS linear (reference default,
 * rcnn.cpp:59), 2 soft-NMS gaussian; workspace: trtx_sorted_nms_workspace(batch, count) */
int32_t trtx_batched_nms(int nms_method, int batch, const float* scores, const float* boxes, const float* classes,
                         int count, int detections_per_im, float nms_thresh, float* out_scores, float* out_boxes,
                         float* out_classes, void* workspace, size_t workspace_bytes, trtx_stream_t stream);

/* maskRcnnInference (rcnn/MaskRcnnInference.cu:8-62): sigmoid of the mask plane of each detection's predicted class.
 * labels [batch][D] (class ids as floats), masks [batch][D][C][S][S] -> out_masks [batch][D][1][S][S]; class ids outside
 * [0, C) give a zero plane (the reference leaves it unwritten). */
int32_t trtx_mask_rcnn_inference(int batch, const float* labels, const float* masks, int detections_per_im, int output_size,
                                 int num_classes, float* out_masks, trtx_stream_t stream);

/* ---- single-kernel entry points (parity tests / micro-benchmarks) ----------------------------- */
/* activation codes for the fused conv epilogue */
#define TRTX_ACT_NONE 0
#define TRTX_ACT_RELU 1
#define TRTX_ACT_SIGMOID 2
#define TRTX_ACT_SILU 3
#define TRTX_ACT_LEAKY 4
#define TRTX_ACT_TANH 5
/* dims of the packed fp16 weight image [cout_pad][kpad] the implicit-GEMM kernel reads */
int32_t trtx_conv_packed_dims(int cout, int cin_pad, int kh, int kw, int32_t* cout_pad, int32_t* kpad, int32_t* bn);
/* host: KCRS fp32 -> packed fp16 (optional per-output-channel scale = folded BatchNorm) */
int32_t trtx_conv_pack_weights_f16(const float* w_kcrs, int cout, int cin, int kh, int kw, int cin_pad,
                                   const float* ch_scale, uint16_t* packed);
/* one fused convolution launch: NHWC fp16 in/out (channel strides ld_*), y = act2(act1(conv+bias) + residual) */
int32_t trtx_op_conv2d_nhwc_f16(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked,
                                const float* bias, void* out, int Cout, int ld_out, int kh, int kw, int sh, int sw,
                                int ph, int pw, int act1, const void* residual, int ld_res, int act2,
                                trtx_stream_t stream);
/* Tactics of that launch (tests / tools): the exchangeable launch configurations of the layer trtx_op_conv2d_nhwc_f16 would
 * run, 6 ints each {column-tile width, k-step width, rows per tile, wave-split-K (1 off / 2 on), weight-stationary (1 off / 2 on),
 * 3x3 row-reuse kernel (0 no / 1 three LDS stages / 2 two)}; entry 0 is the default.  Returns the count (<= max_out).  trtx_op_conv_force_tactic pins the configuration used by the following
 * trtx_op_conv2d_nhwc_f16 calls of this process (NULL: back to the default). */
int32_t trtx_op_conv2d_tactics(int N, int H, int W, int Cin, int ld_in, int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph, int pw,
                               int has_residual, int ld_res, int32_t* out6, int32_t max_out);
int32_t trtx_op_conv_force_tactic(const int32_t* tactic6);
/* The first layer of an fp16 engine (kernels/conv_stem.hip): fp32 NCHW input with 1..4 channels -> NHWC fp16, k x k filter, fp32 weights laid out
 * [tap = (c*k + r)*k + q][Cout] (folded BatchNorm scale included), bias [Cout] or NULL; Cout 8 / 16 / 32 / 64, ld_out a multiple of 8, out 16-byte aligned. */
int32_t trtx_op_conv_stem_nchw_f16(const float* in, int N, int C, int H, int W, const float* w_taps_cout, const float* bias, void* out, int Cout,
                                   int ld_out, int k, int stride, int pad, int act, trtx_stream_t stream);
/* That layer (C <= 4 -> 16, 3x3 stride 2 pad 1) and the 16 -> 32 3x3 stride 2 pad 1 convolution behind it in ONE launch (kernels/conv_stem_pair.hip): the
 * stem's weights and bias as above, the second convolution's as trtx_conv_pack_weights_f16 packs them ([32][160] fp16, cin_pad 16) with bias [32] or NULL,
 * out NHWC fp16 [N][Ho][Wo] with channel stride ld_out (a multiple of 8; a concat slice works as a destination).  The intermediate tensor is never written.
 * Same bits as trtx_op_conv_stem_nchw_f16 followed by trtx_op_conv2d_nhwc_f16 on its default tactic.  conv_act: none, ReLU or SiLU. */
int32_t trtx_op_conv_stem_pair_f16(const float* in, int N, int C, int H, int W, const float* stem_w_taps_cout, const float* stem_bias, int stem_act,
                                   const void* conv_wpacked, const float* conv_bias, int conv_act, void* out, int ld_out, trtx_stream_t stream);
/* The two 3x3 stride-1 pad-1 convolutions of a 16-channel bottleneck in ONE launch (kernels/conv_bneck_pair.hip): in NHWC fp16 [N][H][W] with channel stride
 * ld_in, the 16 input channels starting at channel in_coff (a concat slice works as a source: ld_in and in_coff multiples of 8, in 16-byte aligned); both
 * weight sets as trtx_conv_pack_weights_f16 packs them ([16][160] fp16, cin_pad 16) with biases [16] or NULL; act1 / act2: none, ReLU or SiLU; shortcut != 0
 * adds the input to the second convolution's result, act_after (none, or ReLU with a shortcut) follows; out NHWC fp16 with channel stride ld_out (a multiple
 * of 8).  The output may be another 16-channel slice of the input's buffer (same channel stride) or memory apart from it; an output that lies on the input
 * channels is TRTX_ERR_INVALID: the kernel cannot run in place.  The tensor between the two is never written.  Same bits as two trtx_op_conv2d_nhwc_f16
 * launches on the default tactic, the second with the input as residual. */
int32_t trtx_op_conv_bneck_pair_f16(const void* in, int N, int H, int W, int ld_in, int in_coff, const void* w1_packed, const float* bias1, int act1,
                                    const void* w2_packed, const float* bias2, int act2, int shortcut, int act_after, void* out, int ld_out,
                                    trtx_stream_t stream);
/* What the executor issues for such a pair: that launch where it is possible, otherwise the two implicit-GEMM launches through `mid` (NHWC fp16 [N][H][W][16],
 * 16-byte aligned, written only then) - an output that lies on the input included, which two launches compute correctly. */
int32_t trtx_op_conv_bneck_pair_or_two_f16(const void* in, int N, int H, int W, int ld_in, int in_coff, const void* w1_packed, const float* bias1, int act1,
                                           const void* w2_packed, const float* bias2, int act2, int shortcut, int act_after, void* mid, void* out,
                                           int ld_out, trtx_stream_t stream);
/* 1 <= n <= 3 pairs of convolutions that read the same input, in ONE launch (the dual tile of kernels/igemm_tile.h; the detect head's cv2.x.0 -> 64 and
 * cv3.x.0 -> 80 over three pyramid levels): problem j reads in[j], NHWC fp16 with geom[5 j ..] = {N, H, W, Cin, ld_in}, through one k x k filter geometry
 * (stride, pad) and writes out0[j] (side0[3 j ..] = {Cout, ld_out, act}: 57 .. 64 channels in steps of 8) and out1[j] (side1 likewise: 65 .. 80 channels); weights as
 * trtx_conv_pack_weights_f16 packs them, biases [Cout_pad] or NULL arrays, act none / ReLU / SiLU.  Every output element has the bits of its own
 * trtx_op_conv2d_nhwc_f16 launch on the tactic {bn, 32, 128, 1, 1}.  TRTX_ERR_INVALID: an output that overlaps an input or another output (channel slices side by
 * side in one buffer do not overlap) - nothing is launched.  TRTX_ERR_UNSUPPORTED: what the dual tile does not take - Cin <= 16 (two taps per k-step), a shortcut
 * (res1: per problem the second side's residual with channel stride ld_res1, or NULL), int8 operands (i8_1 != 0 declares the second side's so), other widths. */
int32_t trtx_op_conv_dual_group_f16(int n, const void* const* in, const int32_t* geom, int k, int stride, int pad, const void* const* w0, const float* const* bias0,
                                    void* const* out0, const int32_t* side0, const void* const* w1, const float* const* bias1, void* const* out1,
                                    const int32_t* side1, const void* const* res1, int ld_res1, int i8_1, trtx_stream_t stream);
/* What the executor issues for such a pair of groups: that launch where it is possible, otherwise the launches of each side on its own (same bits). */
int32_t trtx_op_conv_dual_group_or_two_f16(int n, const void* const* in, const int32_t* geom, int k, int stride, int pad, const void* const* w0,
                                           const float* const* bias0, void* const* out0, const int32_t* side0, const void* const* w1, const float* const* bias1,
                                           void* const* out1, const int32_t* side1, const void* const* res1, int ld_res1, int i8_1, trtx_stream_t stream);
/* The same launch in an fp32 engine (builds without BuilderFlag::kFP16: yolov8/include/config.h:1-3 USE_FP32, yolov8/src/model.cpp:314-324):
 * NHWC fp32 in / out / residual, fp32 weights packed [cout_pad][kpad] (k = tap * cink + c, cink = Cin rounded up to the 16-channel k-step, or 8 for
 * Cin <= 8; Cin itself a multiple of 4), fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products and sums).  trtx_op_conv2d_tactics_f32 lists the tile
 * configurations of the layer, 4 ints each {column-tile width, rows per tile, operand path: 1 = LDS-DMA, 3 = resident patch, 5 = through registers, 6 = wave roles,
 * 7 / 8 = the resident-operand 3x3 / 1x1 kernels of conv_res.hip, channels per k-step: 16 / 32} - entry 0 the launcher's own choice, every entry the same bits -;
 * tile4 pins one for this call (NULL: the launcher's choice).  `bias` (may be NULL) holds cout_pad floats (trtx_conv_packed_dims_f32; Cout rounded up to 16), 16-byte
 * aligned: the tile starts its accumulators with 16-byte loads of it up to the padded width - a [Cout] array with Cout % 16 != 0 would be read past its end. */
/* The filter of a convolution that absorbed the ReOrg in front of it (yolov7/src/block.cpp:106-114: four stride-2 slices of x
 * concatenated, then a kh x kw stride-1 padding-p convolution): w_kcrs [cout][4 cin][kh][kw] -> folded [cout][cin][2kh][2kw], the filter
 * of the equal stride-2 padding-2p convolution of x, folded[o][c][2i + dy][2j + dx] = w[o][q cin + c][i][j], q = 2 dx + dy.  Host arrays. */
int32_t trtx_reorg_fold_weights(const float* w_kcrs, int cout, int cin, int kh, int kw, float* folded);
/* The filter and shift the lowering packs for RepVGGDW (yolov10/src/block.cpp:388-403: SiLU(dw7x7 + BN + dw3x3 + BN) on one tensor) as ONE
 * depthwise 7x7 convolution: w_out[c] = scale7[c] * w7[c] with scale3[c] * w3[c] added into its centre, shift_out[c] = shift7[c] + shift3[c];
 * double arithmetic, rounded once to fp32.  Host arrays: w7 [channels][7][7], w3 [channels][3][3], the rest [channels]. */
int32_t trtx_repvggdw_fold_weights(const float* w7, const float* scale7, const float* shift7, const float* w3, const float* scale3,
                                   const float* shift3, int channels, float* w_out, float* shift_out);
int32_t trtx_conv_packed_dims_f32(int cout, int cin_pad, int kh, int kw, int32_t* cout_pad, int32_t* kpad, int32_t* cink);
int32_t trtx_conv_pack_weights_f32(const float* w_kcrs, int cout, int cin, int kh, int kw, int cin_pad, const float* ch_scale, float* packed);
int32_t trtx_op_conv2d_nhwc_f32(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked, const float* bias, void* out, int Cout,
                                int ld_out, int kh, int kw, int sh, int sw, int ph, int pw, int act1, const void* residual, int ld_res, int act2,
                                const int32_t* tile4, trtx_stream_t stream);
int32_t trtx_op_conv2d_tactics_f32(int N, int H, int W, int Cin, int ld_in, int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph, int pw,
                                   int has_residual, int ld_res, int32_t* out4, int32_t max_out);
/* kINT8 convolution, single-kernel entries for the parity tests (what TensorRT runs for a layer of a USE_INT8 build, yolov8/include/config.h:1-3): KCRS fp32 weights ->
 * int8 [cout_pad][kpad bytes] with per-output-channel symmetric scales (cink = Cin rounded up to 64 channels, kpad = kh*kw*cink; packed / wscale_out NULL: sizes only);
 * the int8 MFMA convolution on NHWC int8 input: out int8 (out_is_i8, quantised with out_inv_scale) or fp16, cscale[cout_pad] = input scale x weight scale, optional
 * int8 / fp16 shortcut. */
int32_t trtx_conv_pack_weights_i8(const float* w_kcrs, int cout, int cin, int kh, int kw, const float* ch_scale, int8_t* packed, float* wscale_out,
                                  int32_t* cout_pad_out, int32_t* kpad_out);
int32_t trtx_op_conv2d_nhwc_i8(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked, const float* cscale, const float* bias, void* out,
                               int out_is_i8, float out_inv_scale, int Cout, int ld_out, int kh, int kw, int sh, int sw, int ph, int pw, int act1,
                               const void* residual, int res_is_i8, float res_scale, int ld_res, int act2, trtx_stream_t stream);
/* Grouped convolution on the matrix pipe (tests / tools): 2 <= groups <= 8, Cin / groups and Cout / groups multiples of 16 up to 64, Cout <= 128,
 * k = 1 with pad 0 or k = 3 with pad 1, stride 1; NHWC fp16 in / out / residual with channel strides that are multiples of 8 and 16-byte aligned
 * pointers (TRTX_ERR_UNSUPPORTED / TRTX_ERR_INVALID otherwise).  The packed filter is fp16 [Cout][kpad], k = tap * Cin_g + c, kpad = K rounded up to
 * 32 (packed == NULL: only *kpad_out); bias: Cout floats.  This is the layer the reference hands to cuDNN through
 * addConvolutionNd + setNbGroups (yolov9/src/block.cpp:355-366, DetectBbox_Conv). */
int32_t trtx_conv_pack_weights_grouped_f16(const float* w_kcrs, int cout, int cin_g, int kh, int kw, const float* ch_scale, uint16_t* packed,
                                           int32_t* kpad_out);
int32_t trtx_op_conv2d_grouped_nhwc_f16(const void* in, int N, int H, int W, int Cin, int ld_in, const void* wpacked, const float* bias, void* out,
                                        int Cout, int ld_out, int groups, int k, int pad, int act1, const void* residual, int ld_res, int act2,
                                        trtx_stream_t stream);
/* Depthwise convolution (tests / tools; kernels/conv_dw.hip: YOLO11's DWConv and the attention's positional conv): groups == C, square k of 3 / 5 / 7 with
 * pad == k / 2, stride 1 or 2, dilation 1 (anything else: TRTX_ERR_UNSUPPORTED, nothing is launched).  dtype: TRTX_DTYPE_FLOAT or TRTX_DTYPE_HALF, the type of
 * in / out / residual, each an NHWC channel slice with its own pixel stride ld_*; the filter is fp32 [k * k][C] (tap-major), bias C floats or NULL, residual
 * (out's geometry) or NULL.  out = act2(act1(conv + bias) + residual), the activation kinds as in trtx_op_conv2d_nhwc_f16, alpha the leaky slope.  Whole
 * 16-byte vectors of channels where C, every ld and every base pointer allow them, element-wise otherwise: the same sums in the same order. */
int32_t trtx_op_conv2d_dw_nhwc(const void* in, int dtype, int N, int H, int W, int C, int ld_in, const float* w_taps_c, const float* bias, void* out, int ld_out,
                               const void* residual, int ld_res, int k, int stride, int pad, int dilation, int act1, float alpha1, int act2, float alpha2,
                               trtx_stream_t stream);
/* The fused attention kernels (tests / tools).  qkv: NHWC fp16 [B][N][ld_qkv], head h's channels start at h * (2 kd + hd): q (kd), k (kd), v (hd).
 * out[b][n][h * hd + d] = sum_m softmax_m(scale * q_n . k_m) v[m][d] and vimg[b][n][h * hd + d] = v[n][d], fp16 with pixel strides ld_out / ld_v.
 * psa: kd 32, hd 64 (or kd 36, hd 72: yolov10m), every pixel of the image is a key (kernels/attention.hip).  area: kd 32, hd 32, the N pixels split into `area` contiguous ranges of
 * N / area that attend within themselves (kernels/attention_mfma.hip); pointers or strides that rule out 16-byte loads / 8-byte stores take element-wise ones.
 * TRTX_ERR_UNSUPPORTED, nothing launched: another kd / hd, N % area != 0, ld_qkv < heads * (2 kd + hd), ld_out or ld_v < heads * hd. */
int32_t trtx_op_psa_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int kd, int hd, float scale,
                                  trtx_stream_t stream);
int32_t trtx_op_area_attention_f16(const void* qkv, int ld_qkv, void* out, int ld_out, void* vimg, int ld_v, int B, int heads, int N, int area, int kd, int hd,
                                   float scale, trtx_stream_t stream);
/* The area attention on separate operands (tests / tools; kernels/attention_mfma.hip), as YOLOv13's AAttn has them (yolov13/src/block.cpp:303-423: q | k
 * come from one 1x1 convolution, v from another).  q, k, v: NHWC fp16 [B][N][ld_q / ld_k / ld_v]; head h reads q channels h * kd .., k channels h * kd ..
 * and v channels h * hd ..; out[b][n][h * hd + d] as trtx_op_area_attention_f16 and, given the same values, bit-equal to it.  No V image is written.
 * For YOLOv13 k = q + heads * kd halves and ld_k = ld_q; the entry point does not assume that.  Each operand takes 16-byte loads (O: 8-byte stores) where its
 * base pointer and stride allow them and element-wise accesses otherwise.  TRTX_ERR_UNSUPPORTED, nothing launched: kd != 32 or hd != 32, a count < 1,
 * N % area != 0, B > 65535, heads * area > 65535, ld_q or ld_k < heads * kd, ld_v or ld_out < heads * hd. */
int32_t trtx_op_area_attention_split_f16(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, void* out, int ld_out, int B, int heads,
                                         int N, int area, int kd, int hd, float scale, trtx_stream_t stream);
/* YOLOv13's adaptive hypergraph convolution (tests / tools; kernels/hgconv.hip): AdaHyperedgeGen (yolov13/src/block.cpp:607-700) and AdaHGConv
 * (block.cpp:746-790) with the eleven-layer tanh GELU (block.cpp:702-744), per image on x: NHWC fp16 [B][N][ld_x], D channels = the token image of
 * AdaHGComputation (block.cpp:792-812), E hyperedges:
 *   P = prototype_base + context_net([mean_n x, max_n x]);  A = softmax over the N NODES of logit_scale * (x W_pre^T + b_pre) . P;
 *   out[b][n] = GELU((A GELU(A^T x W_edge^T + b_edge)) W_node^T + b_node) + x[b][n], fp16 with pixel stride ld_out.
 * logit_scale = 1 / (heads * scaling) (the mean over the heads and the division by sqrt(head_dim)).  The weights are the layers' own fp32 device arrays:
 * w_ctx [E D][2 D], b_ctx [E D], proto [E][D], w_pre / w_edge / w_node [D][D], b_pre / b_edge / b_node [D] (b_pre cancels in the node softmax: never read).
 * workspace: at least trtx_op_hgconv_workspace_bytes(B, N, D, E) bytes of device memory, 16-byte aligned (a pure function of its four arguments; 0 for
 * what the op does not implement).  TRTX_ERR_INVALID, nothing launched: a null pointer, ld_x or ld_out < D, a short workspace, a count < 1.
 * TRTX_ERR_UNSUPPORTED, nothing launched: D % 16 != 0, D > 384, E > 16, x or out not 16-byte aligned or a pixel stride that is no multiple of 8.
 * trtx_op_hgconv_geometry: the launcher's node-tile sizes, ascending, into tiles[0 .. max_tiles) and their count into *n_tiles (an image's result depends on N
 * through these alone, never on B). */
size_t trtx_op_hgconv_workspace_bytes(int B, int N, int D, int E);
int32_t trtx_op_hgconv_geometry(int32_t* tiles, int max_tiles, int32_t* n_tiles);
int32_t trtx_op_hgconv_f16(const void* x, int ld_x, void* out, int ld_out, int B, int N, int D, int E, float logit_scale, const float* w_ctx, const float* b_ctx,
                           const float* proto, const float* w_pre, const float* b_pre, const float* w_edge, const float* b_edge, const float* w_node,
                           const float* b_node, void* workspace, size_t workspace_bytes, trtx_stream_t stream);
int32_t trtx_op_poison_lds(void* device_word, trtx_stream_t stream); /* test support: NaN patterns into every CU's LDS */
int32_t trtx_op_nchw_f32_to_nhwc_f16(const float* in, void* out, int N, int C, int H, int W, int Cpad, int ld_out,
                                     trtx_stream_t stream);
int32_t trtx_op_nhwc_f16_to_nchw_f32(const void* in, float* out, int N, int C, int H, int W, int ld_in,
                                     trtx_stream_t stream);

/* ================= Section 2: network definition / engine / execution context =================== */
/*
 * Mirrors, object for object, the nvinfer1 API subset the reference builders use (SURVEY.md §2.3,
 * §8b): IBuilder / IBuilderConfig / INetworkDefinition / ITensor / ILayer / IHostMemory / IRuntime /
 * ICudaEngine / IExecutionContext / IPluginV2 / IPluginCreator / getPluginRegistry().
 * include/NvInfer.h is the header-only C++ shim that gives these the nvinfer1 spelling.
 *
 * Ownership: layers and tensors are owned by their network (never freed by the caller); weights are
 * COPIED when a layer is added, so the caller may free its host blobs after build (the reference frees
 * them after buildSerializedNetwork, yolov8/src/model.cpp:332-334).
 */
typedef struct trtx_builder trtx_builder;
typedef struct trtx_network trtx_network;
typedef struct trtx_hostmem trtx_hostmem;
typedef struct trtx_engine trtx_engine;
typedef struct trtx_context trtx_context;
typedef struct trtx_plugin trtx_plugin; /* runtime-side handle of one plugin instance */

#define TRTX_MAX_DIMS 8
typedef struct trtx_dims {
    int32_t nb;
    int64_t d[TRTX_MAX_DIMS];
} trtx_dims;

/* nvinfer1::DataType */
#define TRTX_DTYPE_FLOAT 0
#define TRTX_DTYPE_HALF 1
#define TRTX_DTYPE_INT8 2
#define TRTX_DTYPE_INT32 3
/* nvinfer1::ActivationType */
#define TRTX_ACTIVATION_RELU 0
#define TRTX_ACTIVATION_SIGMOID 1
#define TRTX_ACTIVATION_TANH 2
#define TRTX_ACTIVATION_LEAKY_RELU 3
/* nvinfer1::PoolingType */
#define TRTX_POOLING_MAX 0
#define TRTX_POOLING_AVERAGE 1
/* nvinfer1::ElementWiseOperation */
#define TRTX_ELEMENTWISE_SUM 0
#define TRTX_ELEMENTWISE_PROD 1
#define TRTX_ELEMENTWISE_MAX 2
#define TRTX_ELEMENTWISE_MIN 3
#define TRTX_ELEMENTWISE_SUB 4
#define TRTX_ELEMENTWISE_DIV 5
#define TRTX_ELEMENTWISE_POW 6
/* nvinfer1::ScaleMode */
#define TRTX_SCALE_UNIFORM 0
#define TRTX_SCALE_CHANNEL 1
#define TRTX_SCALE_ELEMENTWISE 2
/* nvinfer1::ReduceOperation */
#define TRTX_REDUCE_SUM 0
#define TRTX_REDUCE_PROD 1
#define TRTX_REDUCE_MAX 2
#define TRTX_REDUCE_MIN 3
#define TRTX_REDUCE_AVG 4
/* nvinfer1::MatrixOperation */
#define TRTX_MATMUL_NONE 0
#define TRTX_MATMUL_TRANSPOSE 1
#define TRTX_MATMUL_VECTOR 2
/* nvinfer1::UnaryOperation: kEXP .. kISINF are 0 .. 23; only kEXP has a kernel, a network with another one is refused when it is built */
#define TRTX_UNARY_EXP 0
#define TRTX_UNARY_LAST 23
/* nvinfer1::ResizeMode */
#define TRTX_RESIZE_NEAREST 0
#define TRTX_RESIZE_LINEAR 1
/* nvinfer1::BuilderFlag */
#define TRTX_FLAG_FP16 0
#define TRTX_FLAG_INT8 1
/* layer parameter ids for trtx_layer_set_ints / _floats / _dims */
#define TRTX_P_STRIDE 1
#define TRTX_P_PADDING 2
#define TRTX_P_DILATION 3
#define TRTX_P_GROUPS 4
#define TRTX_P_ALPHA 5
#define TRTX_P_BETA 6
#define TRTX_P_AXIS 7          /* concat axis; softmax / reduce axes bitmask */
#define TRTX_P_RESHAPE 8       /* IShuffleLayer::setReshapeDimensions */
#define TRTX_P_FIRST_TRANSPOSE 9
#define TRTX_P_SECOND_TRANSPOSE 10
#define TRTX_P_RESIZE_MODE 11
#define TRTX_P_RESIZE_SCALES 12
#define TRTX_P_RESIZE_OUT_DIMS 13
#define TRTX_P_AVG_EXCLUSIVE 14
#define TRTX_P_KERNEL 15
#define TRTX_P_NB_OUT 16

/* --- plugins: C v-table an IPluginV2-style object is driven through --------------------------- */
/* Every callback receives `self`.  Semantics and call order follow IPluginV2Ext/IOExt as the reference
 * uses them (yolov8/plugin/yololayer.h:7-81; rcnn/RpnDecodePlugin.h:29-187; SURVEY.md §8b lifecycle):
 * clone at addPluginV2 -> configure -> workspace_size -> initialize -> serialize at plan write;
 * on load: creator.deserialize -> configure -> initialize -> enqueue xN -> terminate -> destroy.
 * Tensors at the plugin edge are fp32 LINEAR (NCHW), as supportsFormatCombination demands in the
 * reference (yololayer.h:32-35). */
typedef struct trtx_plugin_vtbl {
    void* self;
    int32_t (*get_nb_outputs)(void* self);
    int32_t (*get_output_dims)(void* self, int32_t index, const trtx_dims* inputs, int32_t nb_inputs, trtx_dims* out);
    int32_t (*configure)(void* self, const trtx_dims* in, int32_t nb_in, const trtx_dims* out, int32_t nb_out,
                         int32_t max_batch);
    int32_t (*initialize)(void* self);
    void (*terminate)(void* self);
    size_t (*workspace_size)(void* self, int32_t max_batch);
    int32_t (*enqueue)(void* self, int32_t batch, const void* const* inputs, void* const* outputs, void* workspace,
                       trtx_stream_t stream); /* 0 = OK, as IPluginV2::enqueue */
    size_t (*serialization_size)(void* self);
    void (*serialize)(void* self, void* buffer);
    const char* (*plugin_type)(void* self);
    const char* (*plugin_version)(void* self);
    /* fills *out with a v-table for an independent copy; returns 0 on success */
    int32_t (*clone)(void* self, struct trtx_plugin_vtbl* out);
    void (*destroy)(void* self);
} trtx_plugin_vtbl;

typedef struct trtx_plugin_field {
    const char* name;
    const void* data;
    int32_t type; /* nvinfer1::PluginFieldType: 0 f16, 1 f32, 2 f64, 3 i8, 4 i16, 5 i32, 6 char */
    int32_t length;
} trtx_plugin_field;

typedef struct trtx_creator_vtbl {
    void* self;
    const char* (*plugin_name)(void* self);
    const char* (*plugin_version)(void* self);
    int32_t (*create)(void* self, const char* name, const trtx_plugin_field* fields, int32_t nb_fields,
                      trtx_plugin_vtbl* out);
    int32_t (*deserialize)(void* self, const char* name, const void* data, size_t length, trtx_plugin_vtbl* out);
} trtx_creator_vtbl;

/* getPluginRegistry()->registerCreator / getPluginCreator (REGISTER_TENSORRT_PLUGIN, yololayer.h:109).
 * Built-in HIP plugins are pre-registered: "YoloLayer_TRT"/"1", "Decode_TRT"/"1" (retinaface). */
int32_t trtx_registry_register(const trtx_creator_vtbl* creator);
int32_t trtx_registry_get(const char* name, const char* version, trtx_creator_vtbl* out);

/* --- .wts weight files (loadWeights, lenet/utils.h:49-80; yolov8/src/block.cpp:13-43) ----------- */
typedef struct trtx_wts trtx_wts;
int32_t trtx_wts_load(const char* path, trtx_wts** out);
int32_t trtx_wts_count(const trtx_wts* w);
/* i-th entry in file order; values are the host fp32 array owned by `w` */
int32_t trtx_wts_entry(const trtx_wts* w, int32_t i, const char** name, const float** values, int64_t* count);
int32_t trtx_wts_find(const trtx_wts* w, const char* name, const float** values, int64_t* count);
void trtx_wts_free(trtx_wts* w);

/* --- builder / config (createInferBuilder, IBuilderConfig) --------------------------------------- */
int32_t trtx_builder_create(trtx_builder** out);
void trtx_builder_destroy(trtx_builder* b);
int32_t trtx_builder_set_max_batch(trtx_builder* b, int32_t n);        /* IBuilder::setMaxBatchSize */
int32_t trtx_builder_set_flag(trtx_builder* b, int32_t flag, int32_t on); /* IBuilderConfig::setFlag */
int32_t trtx_builder_set_workspace(trtx_builder* b, size_t bytes);     /* setMaxWorkspaceSize / setMemoryPoolLimit */
/* IBuilderConfig::setInt8Calibrator (yolov8/src/model.cpp:317-324): the calibrator as a C v-table, IInt8EntropyCalibrator2's
 * methods (yolov8/include/calibrator.h:14-36).  With BuilderFlag::kINT8, trtx_build_serialized first asks read_cache; if that
 * yields a cache the scales come from it (no GPU needed), otherwise get_batch is called until it returns 0, every batch runs
 * through an fp16 engine of the network on the GPU, per-tensor |x| histograms are reduced to thresholds by entropy minimisation
 * and the resulting cache text is handed to write_cache. */
typedef struct trtx_calibrator_vtbl {
    void* self;
    int32_t (*get_batch_size)(void* self);
    /* fills bindings[i] with the DEVICE pointer of input names[i] for one batch; returns 1, or 0 when the data is exhausted */
    int32_t (*get_batch)(void* self, void** bindings, const char* const* names, int32_t nb_bindings);
    const void* (*read_cache)(void* self, size_t* length); /* NULL / length 0: no cache */
    void (*write_cache)(void* self, const void* cache, size_t length);
    /* IInt8Calibrator::getAlgorithm (nvinfer1::CalibrationAlgoType): NULL or 1 / 2 = entropy calibration (the reference's
     * IInt8EntropyCalibrator2: the threshold that minimises the KL divergence, clipping rare large values); 3 = kMINMAX_CALIBRATION
     * (IInt8MinMaxCalibrator: the largest |x| seen, nothing clipped). */
    int32_t (*get_algorithm)(void* self);
} trtx_calibrator_vtbl;
/* IBuilderConfig::setMaxAuxStreams (TensorRT >= 8.6): how many streams besides the caller's an execution context may use to run
 * independent branches of the plan concurrently.  -1 (default) = the runtime's choice (3); 0 = strictly the caller's stream, the
 * right setting when several execution contexts are kept in flight on their own streams (bench.py --contexts). */
int32_t trtx_builder_set_max_aux_streams(trtx_builder* b, int32_t n);
int32_t trtx_builder_set_int8_calibrator(trtx_builder* b, const trtx_calibrator_vtbl* calibrator);
/* the threshold search of the entropy calibration on a caller-supplied histogram of |x| over [0, range] (tests, tools) */
float trtx_int8_entropy_threshold(const double* hist, int32_t bins, float range);
/* the clip limit the calibration applies on top of it (round 6; TRTX_INT8_CLIP_LIMIT, default 1e-4): the lowest bin edge >= thr beyond which at most `limit` of the
 * histogram's mass lies; limit <= 0 returns thr.  TensorRT's entropy calibrator is closed: both searches are this library's own. */
float trtx_int8_clip_limited_threshold(const double* hist, int32_t bins, float range, float thr, double limit);
/* createNetworkV2(flags): bit 0 = kEXPLICIT_BATCH */
int32_t trtx_network_create(trtx_builder* b, uint32_t flags, trtx_network** out);
void trtx_network_destroy(trtx_network* n);
const char* trtx_network_last_error(const trtx_network* n);

/* --- INetworkDefinition::add*: return a layer index (>= 0) or -1; outputs via trtx_layer_output ---- */
int32_t trtx_add_input(trtx_network* n, const char* name, int32_t dtype, const trtx_dims* dims); /* tensor id */
int32_t trtx_add_convolution(trtx_network* n, int32_t input, int32_t nb_out, int32_t kh, int32_t kw,
                             const float* kernel, int64_t kernel_count, const float* bias, int64_t bias_count);
int32_t trtx_add_deconvolution(trtx_network* n, int32_t input, int32_t nb_out, int32_t kh, int32_t kw,
                               const float* kernel, int64_t kernel_count, const float* bias, int64_t bias_count);
int32_t trtx_add_fully_connected(trtx_network* n, int32_t input, int32_t nb_out, const float* kernel,
                                 int64_t kernel_count, const float* bias, int64_t bias_count);
int32_t trtx_add_activation(trtx_network* n, int32_t input, int32_t type);
int32_t trtx_add_pooling(trtx_network* n, int32_t input, int32_t type, int32_t kh, int32_t kw);
int32_t trtx_add_scale(trtx_network* n, int32_t input, int32_t mode, const float* shift, int64_t shift_count,
                       const float* scale, int64_t scale_count, const float* power, int64_t power_count);
int32_t trtx_add_elementwise(trtx_network* n, int32_t a, int32_t b, int32_t op);
int32_t trtx_add_concatenation(trtx_network* n, const int32_t* inputs, int32_t nb_inputs);
int32_t trtx_add_slice(trtx_network* n, int32_t input, const trtx_dims* start, const trtx_dims* size,
                       const trtx_dims* stride);
int32_t trtx_add_shuffle(trtx_network* n, int32_t input);
int32_t trtx_add_resize(trtx_network* n, int32_t input);
int32_t trtx_add_softmax(trtx_network* n, int32_t input);
int32_t trtx_add_matrix_multiply(trtx_network* n, int32_t a, int32_t op_a, int32_t b, int32_t op_b);
int32_t trtx_add_constant(trtx_network* n, const trtx_dims* dims, const float* values, int64_t count);
int32_t trtx_add_reduce(trtx_network* n, int32_t input, int32_t op, uint32_t axes, int32_t keep_dims);
int32_t trtx_add_identity(trtx_network* n, int32_t input);
/* addPaddingNd (yolov3-tiny/yolov3-tiny.cpp:248: Pad(0,0;1,1) in front of the stride-1 max-pool): pre and post are DimsHW, the fill is zero.
 * A negative (cropping) value is refused when the network is built, with the reason in the build's error. */
int32_t trtx_add_padding(trtx_network* n, int32_t input, const trtx_dims* pre, const trtx_dims* post);
/* addUnary (yolov13/src/block.cpp:389: the exp of AAttn's spelled-out softmax); op: a TRTX_UNARY_* / nvinfer1::UnaryOperation value */
int32_t trtx_network_add_unary(trtx_network* n, int32_t input, int32_t op);
/* addPluginV2: the runtime clones the plugin through vtbl->clone (as TensorRT does) */
int32_t trtx_add_plugin_v2(trtx_network* n, const int32_t* inputs, int32_t nb_inputs, const trtx_plugin_vtbl* plugin);

/* ILayer / ITensor accessors */
int32_t trtx_layer_nb_outputs(const trtx_network* n, int32_t layer);
int32_t trtx_layer_output(const trtx_network* n, int32_t layer, int32_t index); /* tensor id */
int32_t trtx_layer_set_name(trtx_network* n, int32_t layer, const char* name);
int32_t trtx_layer_set_ints(trtx_network* n, int32_t layer, int32_t param, const int32_t* v, int32_t count);
int32_t trtx_layer_set_floats(trtx_network* n, int32_t layer, int32_t param, const float* v, int32_t count);
int32_t trtx_layer_set_dims(trtx_network* n, int32_t layer, int32_t param, const trtx_dims* d);
int32_t trtx_tensor_get_dims(const trtx_network* n, int32_t tensor, trtx_dims* out);
int32_t trtx_tensor_set_name(trtx_network* n, int32_t tensor, const char* name);
const char* trtx_tensor_get_name(const trtx_network* n, int32_t tensor);
int32_t trtx_mark_output(trtx_network* n, int32_t tensor);

/* IBuilder::buildSerializedNetwork -> IHostMemory.  Works without a GPU (pure host work). */
int32_t trtx_build_serialized(trtx_builder* b, trtx_network* n, trtx_hostmem** out);
const void* trtx_hostmem_data(const trtx_hostmem* m);
size_t trtx_hostmem_size(const trtx_hostmem* m);
void trtx_hostmem_destroy(trtx_hostmem* m);
/* a host-memory object holding a copy of `size` bytes (the shim's ICudaEngine::serialize on a machine where engines are only built) */
int32_t trtx_hostmem_create(const void* data, size_t size, trtx_hostmem** out);
/* JSON description of a serialized plan: network definition with weight offsets into the plan
 * (used by the test oracle's graph interpreter) and, with lowered != 0, the fused kernel schedule,
 * buffer plan and FLOP/byte counts the engine would execute.  Caller frees with trtx_string_free. */
int32_t trtx_plan_describe(const void* plan, size_t size, int32_t lowered, char** json_out);
void trtx_string_free(char* s);

/* --- IRuntime / ICudaEngine / IExecutionContext ---------------------------------------------------- */
/* deserializeCudaEngine: needs a gfx950 device (TRTX_ERR_NO_DEVICE otherwise — no CPU fallback) */
int32_t trtx_engine_deserialize(const void* plan, size_t size, trtx_engine** out);
int32_t trtx_engine_serialize(const trtx_engine* e, trtx_hostmem** out);
void trtx_engine_destroy(trtx_engine* e);
int32_t trtx_engine_nb_bindings(const trtx_engine* e);
int32_t trtx_engine_binding_index(const trtx_engine* e, const char* name);
const char* trtx_engine_binding_name(const trtx_engine* e, int32_t index);
int32_t trtx_engine_binding_is_input(const trtx_engine* e, int32_t index);
int32_t trtx_engine_binding_dims(const trtx_engine* e, int32_t index, trtx_dims* out);
int32_t trtx_engine_binding_dtype(const trtx_engine* e, int32_t index);
int32_t trtx_engine_max_batch(const trtx_engine* e);
size_t trtx_engine_device_memory(const trtx_engine* e);
/* Tactic selection (TensorRT's builder times several kernels per layer and keeps the fastest; buildSerializedNetwork,
 * yolov8/src/model.cpp:327).  Here it runs inside trtx_engine_deserialize: every MFMA convolution's exchangeable launch
 * configurations are timed in place, behind their real producers, and a layer leaves its default for one that is >= 3 % faster
 * (TRTX_TUNE=0 in the environment at deserialize: every layer keeps its static default and this returns []; TRTX_TACTIC_CACHE=<file>: choices are read from / appended to that file, the ITimingCache
 * analogue, so a later process does not time again).  Returns JSON [{op, name, tactic, default, us, default_us, candidates}, ...]; free with
 * trtx_string_free. */
int32_t trtx_engine_tactics(const trtx_engine* e, char** json_out);
/* Multi-GPU in one process (reference: tutorials/multi_GPU_processing.md:13-30, one `Plan` per device after cudaSetDevice(i)):
 * an engine is bound to the HIP device that was current at trtx_engine_deserialize; this returns its ordinal (-1 for NULL).
 * trtx_context_create / enqueue / enqueue_v3 / profile return TRTX_ERR_STATE when another device is current. */
int32_t trtx_engine_device(const trtx_engine* e);
int32_t trtx_context_create(trtx_engine* e, trtx_context** out);
void trtx_context_destroy(trtx_context* c);
/* IExecutionContext::enqueue(batch, bindings, stream, nullptr) — implicit batch */
int32_t trtx_context_enqueue(trtx_context* c, int32_t batch, void* const* bindings, trtx_stream_t stream);
/* cuda_batch_preprocess + enqueue in one call (yolov8/yolov8_det.cpp:146-160 -> preprocess.cu:119-127): frames[i] is a DEVICE pointer to a
 * tightly packed uint8 HWC BGR image of frame_w[i] x frame_h[i]; the engine's first layer samples the letterboxed frame itself, the fp32
 * network input is never materialised (the input binding's pointer is ignored and may be NULL).  Same output bits as
 * trtx_letterbox_batch followed by trtx_context_enqueue.  Engines whose first layer is a 3-channel stem convolution on the MFMA path
 * (every YOLO / RetinaFace / ResNet builder of the reference); TRTX_ERR_UNSUPPORTED otherwise - then use the two calls. */
int32_t trtx_context_enqueue_frames(trtx_context* c, int32_t batch, const void* const* frames, const int32_t* frame_w, const int32_t* frame_h,
                                    void* const* bindings, trtx_stream_t stream);
/* setTensorAddress + enqueueV3 — explicit batch */
int32_t trtx_context_set_tensor_address(trtx_context* c, const char* name, void* ptr);
int32_t trtx_context_enqueue_v3(trtx_context* c, trtx_stream_t stream);
/* per-kernel timing of the last profiled enqueue (IProfiler::reportLayerTime analogue):
 * runs one enqueue with hipEvents around every launch and returns JSON [{name, kind, ms}, ...] */
int32_t trtx_context_profile(trtx_context* c, int32_t batch, void* const* bindings, trtx_stream_t stream,
                             char** json_out);

#ifdef __cplusplus
}
#endif
#endif /* TRTX_HIP_H_ */
