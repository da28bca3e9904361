// Model builders written against the nvinfer1-shaped API (include/NvInfer.h), mirroring the reference's
// per-model builder functions.  Compile-time constants of the reference (kInputH/W, kBatchSize, kNumClass,
// USE_FP16 ... yolov8/include/config.h:1-31) are run-time arguments here so one binary serves batch 32,
// 1280x1280, etc. (SURVEY.md §5 "Config / flags").
#pragma once
#include <string>
#include <vector>

#include "NvInfer.h"

namespace trtx_host {

// lenet/lenet.cpp:36-155
nvinfer1::IHostMemory* buildLenet(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                  int32_t N);
// resnet/resnet50.cpp:155-229
nvinfer1::IHostMemory* buildResnet50(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                     int maxBatch, bool fp16, int H = 224, int W = 224);

// retinaface/retina_r50.cpp:100-242
nvinfer1::IHostMemory* buildRetinaFaceR50(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                          int maxBatch, bool fp16, int H = 480, int W = 640);

// What every YOLO family's configuration holds: the reference's compile-time constants (include/config.h of each directory) as run-time
// arguments.  The batch has two spellings, one per kind of network: `batch` where the reference builds explicit batch (the batch is part
// of the input dims, so a plan serves exactly that many images per enqueue) and `max_batch` where it builds implicit batch
// (setMaxBatchSize: a plan serves any batch up to it).  They are one field.
struct YoloConfig {
    int input_h = 640, input_w = 640;   // kInputH / kInputW
    int num_class = 80;                 // kNumClass
    union {
        int batch = 1;                  // kBatchSize
        int max_batch;
    };
    int max_out_bbox = 1000;            // kMaxNumOutputBbox
    bool fp16 = true;                   // USE_FP16
    bool mark_heads = false;            // debugging: also expose the plugin's inputs as outputs "head0..N-1"
};

struct Yolov8Config : YoloConfig {
    float gd = 0.33f, gw = 0.25f;       // 'n' scale (yolov8_det.cpp:130-133)
    int max_channels = 1024;
    // 0 det (buildEngineYolov8Det), 1 seg (..Seg, model.cpp:1057-1308: + 32 mask coefficients per cell and the "proto" output),
    // 2 pose (..Pose, :1310-1563: + kNumberOfPoints * 3 keypoint values), 3 obb (..Obb, :2499-2740: + 1 angle logit)
    int task = 0;
    int num_points = 17;                // kNumberOfPoints (include/config.h:28)
    float kpt_conf = 0.5f;              // kConfThreshKeypoints (include/config.h:14); the plugin field carries (int)kpt_conf like the reference
};
// yolov8/src/model.cpp:98-336 (det), 1057-1308 (seg), 1310-1563 (pose), 2499-2740 (obb): one graph, the task adds the cv4 branch
nvinfer1::IHostMemory* buildEngineYolov8Det(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config,
                                            const std::string& wts, const Yolov8Config& cfg);

// yolo11/include/config.h constants as run-time configuration.  Explicit batch like the reference (model.cpp:143-149): the batch is
// part of the input dims, so a plan serves exactly `batch` images per enqueue.
struct Yolo11Scale {                    // shared with YOLOv12: the two programs carry the same table (yolo11_det.cpp / yolo12_det.cpp:120-150)
    float gd = 0.50f, gw = 0.25f;       // 'n' scale
    int max_channels = 1024;
    bool c3k = false;                   // C3k blocks inside C3K2 (m / l / x; model.cpp:160-163, yolov12 model.cpp:60-63)
};
struct Yolo11Config : YoloConfig, Yolo11Scale {
    // 0 det, 1 seg (buildEngineYolo11Seg, model.cpp:509-799: + 32 mask coefficients per cell and the "proto" output), 2 pose
    // (..Pose, :801-1090: + 3 * num_points keypoint values), 3 obb (..Obb, :1092-1389: + 1 angle logit), 4 cls (..Cls, :33-136: logits)
    int task = 0;
    int num_points = 17;                // kNumberOfPoints
    float kpt_conf = 0.5f;              // kConfThreshKeypoints (truncated into the plugin field like the reference)
};
// the n / s / m / l / x scale: gd, gw, max_channels and the c3k flag; false for an unknown letter
bool yolo11_scale(char type, Yolo11Scale* cfg);
// yolo11/src/model.cpp:138-400 (det), 509-799 (seg), 801-1090 (pose), 1092-1389 (obb) with yolo11/src/block.cpp: one graph, the task adds the
// cv4 branch (and Proto for seg); task 4 builds the classifier (model.cpp:33-136) instead
nvinfer1::IHostMemory* buildEngineYolo11Det(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config,
                                            const std::string& wts, const Yolo11Config& cfg);

// yolov12/include/config.h constants as run-time configuration; explicit batch like YOLO11.  Detection only (the reference has no other
// YOLOv12 program).
struct Yolo12Config : YoloConfig, Yolo11Scale {};   // the scale is YOLO11's table: yolo11_scale
// yolov12/src/model.cpp:33-302 with yolov12/src/block.cpp (A2C2f / ABlock / AAttn: area attention in the backbone).  Returns null when
// the stride-16 grid's H * W is not divisible by the attention's area count (4).
nvinfer1::IHostMemory* buildEngineYolo12Det(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config,
                                            const std::string& wts, const Yolo12Config& cfg);

// yolov5/src/config.h constants as run-time configuration.  Implicit batch like the reference (createNetworkV2(0U), Dims3{3, H, W},
// setMaxBatchSize): a plan serves any batch up to max_batch.  Detection, segmentation and classification: `task`.
struct Yolov5Config : YoloConfig {
    float gd = 0.33f, gw = 0.25f;       // 'n' scale (yolov5_det.cpp:22-41; yolov5_scale)
    bool p6 = false;                    // the P6 models (n6 ... x6): four detect levels, strides 8 .. 64
    // 0 det (build_det_engine / build_det_p6_engine), 1 seg (build_seg_engine, model.cpp:539-628: + 32 mask coefficients per anchor, the
    // plugin's is_segmentation flag and the "proto" output), 4 cls (build_cls_engine, :479-537: logits; num_class is kClsNumClass, input_h /
    // input_w kClsInputH / kClsInputW).  The numbers are Yolo11Config's.  P5 only: the reference has no P6 seg / cls builder.
    int task = 0;
};
// the n / s / m / l / x scale: gd and gw; false for an unknown letter
bool yolov5_scale(char type, Yolov5Config* cfg);
// what the builder accepts: task 0 on any model, 1 and 4 on the P5 models (the one statement of that rule: trtx_host_build answers
// TRTX_ERR_INVALID where it is false)
inline bool yolov5_task_valid(int task, bool p6) { return task == 0 || ((task == 1 || task == 4) && !p6); }
// yolov5/src/model.cpp:286-373 (P5), 375-476 (P6), 539-628 (seg) and 479-537 (cls).  Input "data", output "prob" (det / seg:
// 1 + max_out * 38 floats; cls: num_class logits), seg also "proto" (32, H / 4, W / 4).  Returns null where yolov5_task_valid is false
// and when the weight map's anchor_grid / strides do not describe one level per detect convolution.
nvinfer1::IHostMemory* buildEngineYolov5(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                         const Yolov5Config& cfg);
// the name the builder had while it built detection only
inline nvinfer1::IHostMemory* buildEngineYolov5Det(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                                   const Yolov5Config& cfg) {
    return buildEngineYolov5(builder, config, wts, cfg);
}

// yolov9/include/config.h constants as run-time configuration.  Implicit batch like the reference (createNetworkV2(0U), Dims3{3, H, W},
// setMaxBatchSize).  Detection only.
struct Yolov9Config : YoloConfig {
    std::string model = "yolov9t";      // "yolov9t" / "yolov9s" / "yolov9m" / "yolov9c" / "gelanc": the build_engine_* function (yolov9/src/model.cpp)
    bool converted = false;             // isConvert (t / s / m): the re-parameterised checkpoint without the auxiliary branch: its "model.N"
                                        // numbering and DDetect instead of DualDDetect
};
// what the builder accepts: the five names, `converted` on t / s / m only (trtx_host_build answers TRTX_ERR_INVALID where it is false)
bool yolov9_model_valid(const std::string& name, bool converted);
// yolov9/src/model.cpp:25-176 (t), 178-320 (s), 321-555 (m), 557-740 (c), 1160-1286 (gelan-c) with yolov9/src/block.cpp.  Input "images",
// output "output": 1 + max_out * 38 floats.  Layers the reference creates and never connects to the output are not created
// (host/yolov9.cpp).  Returns null where yolov9_model_valid is false.
nvinfer1::IHostMemory* buildEngineYolov9(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                         const Yolov9Config& cfg);

// yolov7/include/config.h constants as run-time configuration.  Implicit batch like the reference (createNetworkV2(0U), Dims3{3, H, W},
// setMaxBatchSize).  Detection, which is all the reference's yolov7 builds.
struct Yolov7Config : YoloConfig {
    std::string model = "yolov7";       // "yolov7tiny" / "yolov7" / "yolov7x" / "yolov7w6" / "yolov7e6": the build_engine_* function (yolov7/src/model.cpp)
};
// the five names the builder accepts (yolov7d6 and yolov7e6e are not built), and which of them have four levels (strides 8 .. 64)
bool yolov7_model_valid(const std::string& name);
bool yolov7_model_p6(const std::string& name);
// yolov7/src/model.cpp:1775-2100 (tiny), 1567-1773 (v7), 1284-1565 (x), 1046-1282 (w6), 775-1044 (e6) with yolov7/src/block.cpp.  Input
// "data", output "prob": 1 + max_out * 6 floats (Detection is bbox[4], conf, class_id).  Returns null for another name and when
// <detect>.anchor_grid does not describe one level per detect convolution.
nvinfer1::IHostMemory* buildEngineYolov7(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                         const Yolov7Config& cfg);

// yolov10/include/config.h constants as run-time configuration.  Explicit batch like the reference (model.cpp:38-44): a plan serves exactly
// max_batch images per enqueue.  Detection, which is all the reference's yolov10 builds.
struct Yolov10Config : YoloConfig {
    std::string model = "yolov10n";     // "yolov10n" / "s" / "m" / "b" / "l" / "x": gd, gw, max_channels (yolov10_det.cpp:111-141) and the stage table
};
// the six names the builder accepts
bool yolov10_model_valid(const std::string& name);
// yolov10/src/model.cpp:33-283 (N), 285-535 (S), 537-787 (M), 789-1039 (B and L), 1041-1291 (X) with yolov10/src/block.cpp: one graph and a
// per-model stage table (host/yolov10.cpp).  Input "images", output "output": 1 + max_out * 6 floats per image (Detection is bbox[4],
// conf, class_id).  Returns null for another name.
nvinfer1::IHostMemory* buildEngineYolov10(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                          const Yolov10Config& cfg);

// yolov3/yololayer.h, yolov3-tiny/yololayer.h and yolov4/yololayer.h constants (INPUT_H / INPUT_W 608, CLASS_NUM 80) as run-time configuration.
// Implicit batch like the reference (createNetworkV2(0U), Dims3{3, H, W}, setMaxBatchSize).  MAX_OUTPUT_BBOX_COUNT (1000) and the anchors are
// compiled into the reference's plugin and stay what they are there.
struct DarknetConfig : YoloConfig {
    DarknetConfig() { input_h = input_w = 608; }   // INPUT_H / INPUT_W: multiples of 32, not necessarily equal.  max_out_bbox is not read.
    std::string model = "yolov4";       // "yolov3" / "yolov3-tiny" / "yolov4": the createEngine of that directory
};
bool darknet_model_valid(const std::string& name);
// the model's module table as JSON rows [module, kind, channels, k, s, p, [from ...]] (host/darknet.cpp); "" for another name
std::string darknet_rows_json(const std::string& name);
// yolov3/yolov3.cpp:190-340, yolov3-tiny/yolov3-tiny.cpp:222-296, yolov4/yolov4.cpp:232-490.  Input "data", output "prob": 1 + 1000 * 7 floats
// (Detection is bbox[4], det_confidence, class_id, class_confidence).  Returns null for another name.
nvinfer1::IHostMemory* buildEngineDarknet(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                          const DarknetConfig& cfg);

// The reference's file-scope constants (rcnn/rcnn.cpp:16-60) as run-time configuration.
struct RcnnConfig {
    int input_h = 800, input_w = 1067;      // INPUT_H / INPUT_W: 480x640 resized by calculateSize() (rcnn.cpp:349-366)
    int max_batch = 1;                      // BATCH_SIZE
    bool fp16 = true;
    float pixel_mean[3] = {103.53f, 116.28f, 123.675f};
    float pixel_std[3] = {1.0f, 1.0f, 1.0f};
    int num_classes = 80;
    int res2_out_channels = 256;            // R50
    std::vector<float> anchor_sizes = {32, 64, 128, 256, 512};
    std::vector<float> aspect_ratios = {0.5f, 1.0f, 2.0f};
    int pre_nms_topk = 6000;                // PRE_NMS_TOP_K_TEST
    float rpn_nms_thresh = 0.7f;
    int post_nms_topk = 1000;
    int stride = 16;                        // STRIDES
    int sampling_ratio = 0;
    int pooler_resolution = 14;
    float nms_thresh_test = 0.5f;
    int detections_per_image = 100;
    float bbox_reg_weights[4] = {10.0f, 10.0f, 5.0f, 5.0f};
    int nms_method = 1;                     // 0 hard, 1 soft-NMS linear (reference default), 2 soft-NMS gaussian
    bool mask_on = false;                   // MASK_ON: Mask R-CNN head (rcnn.cpp:202-232), extra output "masks"
    bool mark_stages = false;               // debugging: also expose "features" and "proposals"
};
// rcnn/rcnn.cpp:79-278 (box head, and the mask head when mask_on)
nvinfer1::IHostMemory* buildRcnnR50C4(nvinfer1::IBuilder* builder, nvinfer1::IBuilderConfig* config, const std::string& wts,
                                      const RcnnConfig& cfg);

}  // namespace trtx_host
