// YOLOv5 detection, segmentation and classification (the v6 / v7 graphs: 6x6 stem, C3, SPPF; P5, and P6 for detection) through the
// network-definition API, implicit batch like the reference.  Mirrors the reference blocks and builders:
//   convBlock / bottleneck / C3 / SPPF / Proto / getAnchors / addYoLoLayer   yolov5/src/model.cpp:99-232, 234-284
//   get_width / get_depth / build_det_engine / build_det_p6_engine          yolov5/src/model.cpp:53-64, 286-476
//   build_cls_engine / build_seg_engine                                     yolov5/src/model.cpp:479-537, 539-628
// Graph, weight keys ("model.<n>...") and layer order are those of the reference.  Not built: P6 seg / cls (the reference has none),
// the v1 - v5 era blocks (focus, bottleneckCSP, SPP), INT8.
#include <cmath>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

constexpr int kNumAnchor = 3;   // yolov5/src/config.h:35

// Conv (no bias, padding k / 3: 6 -> 2, 3 -> 1, 1 -> 0) + BN (eps 1e-3) + SiLU   (model.cpp:99-116)
ITensor* convBlock(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname) { return silu(c, conv_p(c, in, ch, k, s, k / 3, lname)); }

ITensor* bottleneck13(Ctx& c, ITensor& in, int c1, int c2, bool shortcut, float e, const std::string& lname) {  // model.cpp:129-137: 1x1 then 3x3 (blocks::bottleneck is 3x3, 3x3)
    ITensor* a = convBlock(c, in, (int)((float)c2 * e), 1, 1, lname + ".cv1");
    ITensor* b = convBlock(c, *a, c2, 3, 1, lname + ".cv2");
    return shortcut && c1 == c2 ? sum(c, in, *b) : b;
}

ITensor* C3(Ctx& c, ITensor& in, int c2, int n, bool shortcut, const std::string& lname) {  // model.cpp:162-177, e = 0.5
    const int c_ = (int)((float)c2 * 0.5f);
    ITensor* y = convBlock(c, in, c_, 1, 1, lname + ".cv1");
    ITensor* b = convBlock(c, in, c_, 1, 1, lname + ".cv2");
    for (int i = 0; i < n; ++i) y = bottleneck13(c, *y, c_, c_, shortcut, 1.0f, lname + ".m." + std::to_string(i));
    return convBlock(c, *cat2(c, y, b), c2, 1, 1, lname + ".cv3");
}

// nearest upsample to the lateral tensor's dimensions, joined with it (model.cpp:310-316)
ITensor* upcat(Ctx& c, ITensor& in, ITensor* lateral) {
    auto* r = c.net->addResize(in);
    assert(r);
    r->setResizeMode(ResizeMode::kNEAREST);
    r->setOutputDimensions(lateral->getDimensions());
    return cat2(c, r->getOutput(0), lateral);
}

// the biased 1x1 detect convolutions (model.cpp:331; seg, model.cpp:582: 32 mask coefficients more per anchor)
ITensor* detect(Ctx& c, ITensor& in, int info, const std::string& lname) {
    auto* det = c.net->addConvolutionNd(in, kNumAnchor * info, DimsHW{1, 1}, need(c.wm, lname + ".weight"), need(c.wm, lname + ".bias"));
    assert(det);
    return det->getOutput(0);
}

// model.cpp:234-284: the strides are <detect>.strides (floats, truncated), "netinfo" five ints, [4] is_segmentation.  The registry's
// YoloLayer_TRT / 1 creator resolves this field set to the anchor plugin.  Null when the weight map does not describe one level per
// detect convolution.
IPluginV2Layer* addYoLoLayer(Ctx& c, const std::string& lname, const std::vector<ITensor*>& dets, const Yolov5Config& cfg) {
    const Weights& st = need(c.wm, lname + ".strides");
    if ((size_t)st.count < dets.size()) return nullptr;
    std::vector<int> scales;
    for (size_t i = 0; i < dets.size(); ++i) scales.push_back((int)static_cast<const float*>(st.values)[i]);
    return addAnchorYoLoLayer(c, lname, dets, {cfg.num_class, cfg.input_w, cfg.input_h, cfg.max_out_bbox, cfg.task == 1}, scales);
}

// Proto (model.cpp:219-232): 3x3 convBlock, nearest resize by the scales {1, 2, 2}, 3x3 convBlock, 1x1 convBlock to c2 channels
ITensor* Proto(Ctx& c, ITensor& in, int c_, int c2, const std::string& lname) {
    ITensor* cv1 = convBlock(c, in, c_, 3, 1, lname + ".cv1");
    auto* up = c.net->addResize(*cv1);
    assert(up);
    up->setResizeMode(ResizeMode::kNEAREST);
    const float scales[] = {1, 2, 2};
    up->setScales(scales, 3);
    ITensor* cv2 = convBlock(c, *up->getOutput(0), c_, 3, 1, lname + ".cv2");
    return convBlock(c, *cv2, c2, 1, 1, lname + ".cv3");
}

// the part of the backbone every model shares (model.cpp:295-302, 385-391, 488-496): the 6x6 stride-2 stem with padding 2, then C3
// stages to model.6; c4 and c6 are the laterals
ITensor* backbone(Ctx& c, ITensor* data, const Yolov5Config& cfg, ITensor** c4, ITensor** c6) {
    auto W = [&](int x) { return get_width_v5(x, cfg.gw); };
    auto D = [&](int x) { return get_depth(x, cfg.gd); };
    ITensor* x = convBlock(c, *data, W(64), 6, 2, "model.0");
    x = convBlock(c, *x, W(128), 3, 2, "model.1");
    x = C3(c, *x, W(128), D(3), true, "model.2");
    x = convBlock(c, *x, W(256), 3, 2, "model.3");
    *c4 = C3(c, *x, W(256), D(6), true, "model.4");
    x = convBlock(c, **c4, W(512), 3, 2, "model.5");
    return *c6 = C3(c, *x, W(512), D(9), true, "model.6");
}

// build_cls_engine (model.cpp:479-537): the backbone to model.8, convBlock to 1280 channels, average pool over the whole map, fully
// connected layer.  The reference pools DimsHW{k, k} with k = kClsInputH / 32, the square case of (h / 32, w / 32).
IHostMemory* buildCls(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolov5Config& cfg) {
    Session s(builder, wts);
    Ctx& c = s.c;
    ITensor *c4, *c6;
    ITensor* x = backbone(c, s.input("data", cfg.input_h, cfg.input_w), cfg, &c4, &c6);
    x = convBlock(c, *c6, get_width_v5(1024, cfg.gw), 3, 2, "model.7");
    x = C3(c, *x, get_width_v5(1024, cfg.gw), get_depth(3, cfg.gd), true, "model.8");
    ITensor* conv_class = convBlock(c, *x, 1280, 1, 1, "model.9.conv");
    auto* pool = s.net->addPoolingNd(*conv_class, PoolingType::kAVERAGE, DimsHW{cfg.input_h / 32, cfg.input_w / 32});
    assert(pool);
    auto* fc = s.net->addFullyConnected(*pool->getOutput(0), cfg.num_class, need(s.wm, "model.9.linear.weight"), need(s.wm, "model.9.linear.bias"));
    assert(fc);
    s.output(fc->getOutput(0), "prob");
    return s.finish(builder, config, cfg.max_batch, cfg.fp16);
}

}  // namespace

bool yolov5_scale(char type, Yolov5Config* cfg) {  // yolov5_det.cpp:22-41
    switch (type) {
        case 'n': cfg->gd = 0.33f; cfg->gw = 0.25f; break;
        case 's': cfg->gd = 0.33f; cfg->gw = 0.50f; break;
        case 'm': cfg->gd = 0.67f; cfg->gw = 0.75f; break;
        case 'l': cfg->gd = 1.00f; cfg->gw = 1.00f; break;
        case 'x': cfg->gd = 1.33f; cfg->gw = 1.25f; break;
        default: return false;
    }
    return true;
}

IHostMemory* buildEngineYolov5(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolov5Config& cfg) {
    if (!yolov5_task_valid(cfg.task, cfg.p6)) return nullptr;
    if (cfg.task == 4) return buildCls(builder, config, wts, cfg);
    Session s(builder, wts);
    Ctx& c = s.c;
    const int nc = cfg.num_class + 5 + (cfg.task == 1 ? 32 : 0);   // values per anchor of a detect convolution
    auto W = [&](int x) { return get_width_v5(x, cfg.gw); };
    auto D = [&](int x) { return get_depth(x, cfg.gd); };

    std::vector<ITensor*> dets;
    std::string detect_name;
    ITensor* proto_in = nullptr;   // seg: Proto reads model.17's output
    ITensor *c4, *c6;
    ITensor* x = backbone(c, s.input("data", cfg.input_h, cfg.input_w), cfg, &c4, &c6);
    if (!cfg.p6) {
        x = convBlock(c, *c6, W(1024), 3, 2, "model.7");
        x = C3(c, *x, W(1024), D(3), true, "model.8");
        x = SPPF(c, *x, W(1024), W(1024), 5, "model.9");
        // ---- head (model.cpp:308-341): the detect convolutions sit where the reference adds them
        ITensor* c10 = convBlock(c, *x, W(512), 1, 1, "model.10");
        ITensor* c13 = C3(c, *upcat(c, *c10, c6), W(512), D(3), false, "model.13");
        ITensor* c14 = convBlock(c, *c13, W(256), 1, 1, "model.14");
        ITensor* c17 = C3(c, *upcat(c, *c14, c4), W(256), D(3), false, "model.17");
        dets.push_back(detect(c, *c17, nc, "model.24.m.0"));
        proto_in = c17;
        ITensor* c18 = convBlock(c, *c17, W(256), 3, 2, "model.18");
        ITensor* c20 = C3(c, *cat2(c, c18, c14), W(512), D(3), false, "model.20");
        dets.push_back(detect(c, *c20, nc, "model.24.m.1"));
        ITensor* c21 = convBlock(c, *c20, W(512), 3, 2, "model.21");
        ITensor* c23 = C3(c, *cat2(c, c21, c10), W(1024), D(3), false, "model.23");
        dets.push_back(detect(c, *c23, nc, "model.24.m.2"));
        detect_name = "model.24";
    } else {
        // ---- P6 backbone tail and head (model.cpp:392-445): four levels, strides 8 .. 64
        x = convBlock(c, *c6, W(768), 3, 2, "model.7");
        ITensor* c8 = C3(c, *x, W(768), D(3), true, "model.8");
        x = convBlock(c, *c8, W(1024), 3, 2, "model.9");
        x = C3(c, *x, W(1024), D(3), true, "model.10");
        x = SPPF(c, *x, W(1024), W(1024), 5, "model.11");
        ITensor* c12 = convBlock(c, *x, W(768), 1, 1, "model.12");
        ITensor* c15 = C3(c, *upcat(c, *c12, c8), W(768), D(3), false, "model.15");
        ITensor* c16 = convBlock(c, *c15, W(512), 1, 1, "model.16");
        ITensor* c19 = C3(c, *upcat(c, *c16, c6), W(512), D(3), false, "model.19");
        ITensor* c20 = convBlock(c, *c19, W(256), 1, 1, "model.20");
        ITensor* c23 = C3(c, *upcat(c, *c20, c4), W(256), D(3), false, "model.23");
        ITensor* c24 = convBlock(c, *c23, W(256), 3, 2, "model.24");
        ITensor* c26 = C3(c, *cat2(c, c24, c20), W(512), D(3), false, "model.26");
        ITensor* c27 = convBlock(c, *c26, W(512), 3, 2, "model.27");
        ITensor* c29 = C3(c, *cat2(c, c27, c16), W(768), D(3), false, "model.29");
        ITensor* c30 = convBlock(c, *c29, W(768), 3, 2, "model.30");
        ITensor* c32 = C3(c, *cat2(c, c30, c12), W(1024), D(3), false, "model.32");
        ITensor* feats[4] = {c23, c26, c29, c32};
        for (int lv = 0; lv < 4; ++lv) dets.push_back(detect(c, *feats[lv], nc, "model.33.m." + std::to_string(lv)));
        detect_name = "model.33";
    }
    if (cfg.mark_heads) s.mark_heads(dets);
    IPluginV2Layer* yolo = addYoLoLayer(c, detect_name, dets, cfg);
    if (!yolo) return nullptr;
    s.output(yolo->getOutput(0), "prob");
    // model.cpp:598-600: after the plugin, so the bindings are data, prob, proto
    if (cfg.task == 1) s.output(Proto(c, *proto_in, W(256), 32, detect_name + ".proto"), "proto");
    return s.finish(builder, config, cfg.max_batch, cfg.fp16);
}

}  // namespace trtx_host
