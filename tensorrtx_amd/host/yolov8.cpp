// YOLOv8 detection network (BASELINE config 3) through the network-definition API.
// Mirrors the reference blocks and builder:
//   convBnSiLU / bottleneck / C2F / SPPF / DFL / addYoLoLayer     yolov8/src/block.cpp:79-309 (yolo_blocks.h, on implicit-batch tensors)
//   get_width / get_depth / buildEngineYolov8Det                  yolov8/src/model.cpp:13-25, 98-336
// Graph, weight keys ("model.<n>...") and layer order are those of the reference; the code is organised
// around small tables (backbone stages, the three detect levels) instead of one long listing.
#include <cmath>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

// Proto (model.cpp:36-52): 3x3 convBnSiLU -> ConvTranspose 2x2 stride 2 (bias) -> 3x3 -> 1x1 to 32 mask prototypes
ITensor* proto(Ctx& c, ITensor& in, const Yolov8Config& cfg) {
    const int mid = get_width_v8(256, cfg.gw, cfg.max_channels);
    ITensor* a = convBnSiLU(c, in, mid, 3, 1, "model.22.proto.cv1");
    auto* up = c.net->addDeconvolutionNd(*a, mid, DimsHW{2, 2}, need(c.wm, "model.22.proto.upsample.weight"),
                                         need(c.wm, "model.22.proto.upsample.bias"));
    assert(up);
    up->setStrideNd(DimsHW{2, 2});
    ITensor* b = convBnSiLU(c, *up->getOutput(0), mid, 3, 1, "model.22.proto.cv2");
    return convBnSiLU(c, *b, 32, 1, 1, "model.22.proto.cv3");
}

}  // namespace

IHostMemory* buildEngineYolov8Det(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolov8Config& cfg) {
    Session s(builder, wts);
    Ctx& c = s.c;
    const float gd = cfg.gd, gw = cfg.gw;
    auto W = [&](int x) { return get_width_v8(x, gw, cfg.max_channels); };

    ITensor* data = s.input("images", cfg.input_h, cfg.input_w);
    // ---- backbone (model.cpp:115-140)
    ITensor* p1 = convBnSiLU(c, *data, W(64), 3, 2, "model.0");
    ITensor* p2 = convBnSiLU(c, *p1, W(128), 3, 2, "model.1");
    ITensor* c2 = C2F(c, *p2, W(128), get_depth(3, gd), true, 0.5f, "model.2");
    ITensor* p3 = convBnSiLU(c, *c2, W(256), 3, 2, "model.3");
    ITensor* c4 = C2F(c, *p3, W(256), get_depth(6, gd), true, 0.5f, "model.4");
    ITensor* p4 = convBnSiLU(c, *c4, W(512), 3, 2, "model.5");
    ITensor* c6 = C2F(c, *p4, W(512), get_depth(6, gd), true, 0.5f, "model.6");
    ITensor* p5 = convBnSiLU(c, *c6, W(1024), 3, 2, "model.7");
    ITensor* c8 = C2F(c, *p5, W(1024), get_depth(3, gd), true, 0.5f, "model.8");
    ITensor* c9 = SPPF(c, *c8, W(1024), W(1024), 5, "model.9");
    // ---- neck (model.cpp:145-182)
    ITensor* c12 = C2F(c, *cat2(c, upsample2x(c, *c9), c6), W(512), get_depth(3, gd), false, 0.5f, "model.12");
    ITensor* c15 = C2F(c, *cat2(c, upsample2x(c, *c12), c4), W(256), get_depth(3, gd), false, 0.5f, "model.15");
    ITensor* c16 = convBnSiLU(c, *c15, W(256), 3, 2, "model.16");
    ITensor* c18 = C2F(c, *cat2(c, c16, c12), W(512), get_depth(3, gd), false, 0.5f, "model.18");
    ITensor* c19 = convBnSiLU(c, *c18, W(512), 3, 2, "model.19");
    ITensor* c21 = C2F(c, *cat2(c, c19, c9), W(1024), get_depth(3, gd), false, 0.5f, "model.21");

    // ---- detect head and tail (model.cpp:188-303), layers in the reference's own order: the plan this builder serializes is byte for
    // byte the plan the reference's buildEngineYolov8Det produces through the same shim on the same .wts (tests/test_ref_builders.py)
    DetectV8 h{"model.22.", "model.22.dfl.conv.weight", false, (gw == 1.25f) ? 80 : 64,
               (gw == 0.25f) ? std::max(64, std::min(cfg.num_class, 100)) : W(256), cfg.num_class, 0, cfg.input_h, cfg.input_w, cfg.task};
    if (cfg.task == 1) {  // seg: the reference's width table (model.cpp:61-70)
        h.cv4_mid = gw <= 0.5f ? 32 : (gw == 0.75f ? 48 : (gw == 1.0f ? 64 : 80));
        h.cv4_out = 32;
    } else if (cfg.task) {  // pose / obb: the width stored in the weights (:74-82)
        h.cv4_mid = (int)need(s.wm, "model.22.cv4.0.0.bn.weight").count;
        h.cv4_out = cfg.task == 2 ? cfg.num_points * 3 : 1;
    }
    const std::vector<int> strides = strides_from(cfg.input_h, {p3, p4, p5});
    const std::vector<ITensor*> dets = detect_v8(c, h, {c15, c18, c21}, strides);
    if (cfg.mark_heads) s.mark_heads(dets);
    // block.cpp:259-309; :278: the float keypoint threshold is truncated
    IPluginV2Layer* yolo = addYoLoLayer(c, dets, strides, {cfg.num_class, cfg.num_points, (int)cfg.kpt_conf, cfg.input_w, cfg.input_h, cfg.max_out_bbox,
                                                          cfg.task == 1, cfg.task == 2, cfg.task == 3});
    assert(yolo);
    s.output(yolo->getOutput(0), "output");
    if (cfg.task == 1) s.output(proto(c, *c15, cfg), "proto");  // model.cpp:1280-1282
    return s.finish(builder, config, cfg.max_batch, cfg.fp16);
}

}  // namespace trtx_host
