// YOLOv10 detection network through the network-definition API, explicit batch like the reference.
// Mirrors the reference blocks and builders:
//   convBnSiLU / convBn / bottleneck / C2F / SPPF / DFL / addYoLoLayer / SCDown / Attention / PSA / RepVGGDW / CIB / C2fCIB
//                                                              yolov10/src/block.cpp:73-461 (all in yolo_blocks.h; this file holds the
//                                                              stage table and the graph)
//   get_width / get_depth / calculateStrides                   yolov10/src/model.cpp:9-31
//   buildEngineYolov10Det{N,S,M,BL,X}                          yolov10/src/model.cpp:33-283, 285-535, 537-787, 789-1039, 1041-1291
// The five reference functions are one graph.  They differ in which of the stages 6, 8, 13, 19 and 22 are C2F and which C2fCIB, and in
// C2fCIB's `lk` argument (RepVGGDW in place of the middle depthwise convolution); everything else - the SCDown stages 5, 7 and 20, SPPF 9,
// PSA 10, C2F's shortcut (true in the backbone, false in the neck), C2fCIB's shortcut (always true) and the head's channel formulae
// (model.cpp:113-117, the same five times) - is the same text in all five.  kStages below is that difference.
// Graph, weight keys ("model.<n>...") and layer order are those of the reference.
#include <cmath>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

enum Stage : int { F = 0 /* C2F */, C = 1 /* C2fCIB, lk = false */, L = 2 /* C2fCIB, lk = true */ };
struct StageRow {
    char letter;
    float gd, gw;
    int max_channels;      // yolov10_det.cpp:111-141
    Stage s6, s8, s13, s19, s22;
};
const StageRow kStages[] = {
        {'n', 0.33f, 0.25f, 1024, F, F, F, F, L},   // model.cpp:63, 67, 84, 101, 107
        {'s', 0.33f, 0.50f, 1024, F, L, F, F, L},   // model.cpp:315, 319, 336, 353, 359
        {'m', 0.67f, 0.75f, 768, F, C, F, C, C},    // model.cpp:567, 571, 588, 605, 611
        {'b', 0.67f, 1.00f, 512, F, C, C, C, C},    // model.cpp:819, 823, 840, 857, 863 (BL)
        {'l', 1.00f, 1.00f, 512, F, C, C, C, C},    // the same function with the 'l' scale
        {'x', 1.00f, 1.25f, 512, C, C, C, C, C},    // model.cpp:1071, 1075, 1092, 1109, 1115
};

const StageRow* stage_row(const std::string& name) {
    if (name.size() != 8 || name.compare(0, 7, "yolov10") != 0) return nullptr;
    for (const StageRow& r : kStages)
        if (r.letter == name[7]) return &r;
    return nullptr;
}

// one of the five variable stages: C2F with the caller's shortcut, or C2fCIB (shortcut true) with or without the large kernel
ITensor* stage(Ctx& c, ITensor& in, Stage kind, int c2, int n, bool c2f_shortcut, const std::string& lname) {
    if (kind == F) return C2F(c, in, c2, n, c2f_shortcut, 0.5f, lname);
    return C2fCIB(c, in, c2, n, true, kind == L, 0.5f, lname);
}

}  // namespace

bool yolov10_model_valid(const std::string& name) { return stage_row(name) != nullptr; }

IHostMemory* buildEngineYolov10(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolov10Config& cfg) {
    const StageRow* row = stage_row(cfg.model);
    if (!row) return nullptr;
    Session s(builder, wts, cfg.max_batch);
    Ctx& c = s.c;
    const float gd = row->gd;
    const int nc = cfg.num_class;
    auto W = [&](int x) { return get_width(x, row->gw, row->max_channels); };

    ITensor* data = s.input("images", cfg.input_h, cfg.input_w);
    // ---- backbone (model.cpp:50-71)
    ITensor* conv0 = convBnSiLU(c, *data, W(64), 3, 2, "model.0");
    ITensor* conv1 = convBnSiLU(c, *conv0, W(128), 3, 2, "model.1");
    ITensor* conv2 = C2F(c, *conv1, W(128), get_depth(3, gd), true, 0.5f, "model.2");
    ITensor* conv3 = convBnSiLU(c, *conv2, W(256), 3, 2, "model.3");
    ITensor* conv4 = C2F(c, *conv3, W(256), get_depth(6, gd), true, 0.5f, "model.4");
    ITensor* conv5 = SCDown(c, *conv4, W(512), 3, 2, "model.5");
    ITensor* conv6 = stage(c, *conv5, row->s6, W(512), get_depth(6, gd), true, "model.6");
    ITensor* conv7 = SCDown(c, *conv6, W(1024), 3, 2, "model.7");
    ITensor* conv8 = stage(c, *conv7, row->s8, W(1024), get_depth(3, gd), true, "model.8");
    ITensor* conv9 = SPPF(c, *conv8, W(1024), W(1024), 5, "model.9");
    ITensor* conv10 = PSA(c, *conv9, W(1024), "model.10");
    // ---- neck (model.cpp:75-108)
    ITensor* conv13 = stage(c, *cat2(c, upsample2x(c, *conv10), conv6), row->s13, W(512), get_depth(3, gd), false, "model.13");
    ITensor* conv16 = C2F(c, *cat2(c, upsample2x(c, *conv13), conv4), W(256), get_depth(3, gd), false, 0.5f, "model.16");
    ITensor* conv17 = convBnSiLU(c, *conv16, W(256), 3, 2, "model.17");
    ITensor* conv19 = stage(c, *cat2(c, conv17, conv13), row->s19, W(512), get_depth(3, gd), false, "model.19");
    ITensor* conv20 = SCDown(c, *conv19, W(512), 3, 2, "model.20");
    ITensor* conv22 = stage(c, *cat2(c, conv20, conv10), row->s22, W(1024), get_depth(3, gd), false, "model.22");

    // ---- one-to-one detect head (model.cpp:113-191) and tail (:197-252)
    const int ch0 = channels_of(*conv16);
    const DetectV8 h{"model.23.one2one_", "model.23.dfl.conv.weight", true, std::max(16, std::max(ch0 / 4, 16 * 4)), std::max(ch0, std::min(nc, 100)),
                     nc, cfg.max_batch, cfg.input_h, cfg.input_w};
    const std::vector<int> strides = strides_from(cfg.input_h, {conv3, conv5, conv7});
    const std::vector<ITensor*> dets = detect_v8(c, h, {conv16, conv19, conv22}, strides);
    if (cfg.mark_heads) s.mark_heads(dets);
    // addYoLoLayer (block.cpp:235-277): "combinedInfo" = {classes, W, H, maxOut, strides...}, the 6-float form of YoloLayer_TRT
    IPluginV2Layer* yolo = addYoLoLayer(c, dets, strides, {nc, cfg.input_w, cfg.input_h, cfg.max_out_bbox});
    assert(yolo);
    s.output(yolo->getOutput(0), "output");
    return s.finish(builder, config, cfg.max_batch, cfg.fp16);
}

}  // namespace trtx_host
