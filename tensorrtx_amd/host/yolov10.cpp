// YOLOv10 detection network through the network-definition API, explicit batch like the reference.
// Mirrors the reference blocks and builders:
//   convBnSiLU / convBn / bottleneck / C2F / SPPF / DFL / addYoLoLayer / SCDown / Attention / PSA / RepVGGDW / CIB / C2fCIB
//                                                              yolov10/src/block.cpp:73-461 (yolo_blocks.h)
//   get_width / get_depth / calculateStrides                   yolov10/src/model.cpp:9-31
//   buildEngineYolov10Det{N,S,M,BL,X}                          yolov10/src/model.cpp:33-283, 285-535, 537-787, 789-1039, 1041-1291
// The five reference functions are one graph.  They differ in which of the stages 6, 8, 13, 19 and 22 are C2F and which C2fCIB, and in
// C2fCIB's `lk` argument (RepVGGDW in place of the middle depthwise convolution); everything else - the SCDown stages 5, 7 and 20, SPPF 9,
// PSA 10, C2F's shortcut (true in the backbone, false in the neck), C2fCIB's shortcut (always true) and the head's channel formulae
// (model.cpp:113-117, the same five times) - is the same text in all five.  kStages below is that difference.
// Graph, weight keys ("model.<n>...") and layer order are those of the reference.
#include <cmath>
#include <vector>

#include "common.h"
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
    WeightMap wm = loadWeights(wts);
    INetworkDefinition* net = builder->createNetworkV2(1U << static_cast<uint32_t>(NetworkDefinitionCreationFlag::kEXPLICIT_BATCH));
    IHostMemory* plan = nullptr;
    {
        Ctx c{net, wm, {}};
        const float gd = row->gd, gw = row->gw;
        const int mc = row->max_channels, B = cfg.max_batch, nc = cfg.num_class;
        auto W = [&](int x) { return get_width(x, gw, mc); };

        ITensor* data = net->addInput("images", DataType::kFLOAT, Dims4{B, 3, cfg.input_h, cfg.input_w});
        assert(data);
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

        // ---- one-to-one detect head (model.cpp:113-191): per level a 64-channel box branch and a depthwise / 1x1 class branch
        const int ch0 = (int)conv16->getDimensions().d[1];
        const int c2 = std::max(16, std::max(ch0 / 4, 16 * 4));
        const int c3 = std::max(ch0, std::min(nc, 100));
        ITensor* feats[3] = {conv16, conv19, conv22};
        const int feat_w[3] = {W(256), W(512), W(1024)};
        std::vector<ITensor*> cats;
        for (int lv = 0; lv < 3; ++lv) {
            const std::string s = "model.23.one2one_cv2." + std::to_string(lv), t = "model.23.one2one_cv3." + std::to_string(lv);
            ITensor* b = convBnSiLU(c, *feats[lv], c2, 3, 1, s + ".0");
            b = convBnSiLU(c, *b, c2, 3, 1, s + ".1");
            auto* box = net->addConvolutionNd(*b, 64, DimsHW{1, 1}, need(wm, s + ".2.weight"), need(wm, s + ".2.bias"));
            box->setStrideNd(DimsHW{1, 1});
            box->setPaddingNd(DimsHW{0, 0});
            ITensor* k = DWConv(c, *feats[lv], feat_w[lv], 3, 1, t + ".0.0");
            k = convBnSiLU(c, *k, c3, 1, 1, t + ".0.1");
            k = DWConv(c, *k, c3, 3, 1, t + ".1.0");
            k = convBnSiLU(c, *k, c3, 1, 1, t + ".1.1");
            auto* cls = net->addConvolutionNd(*k, nc, DimsHW{1, 1}, need(wm, t + ".2.weight"), need(wm, t + ".2.bias"));
            cls->setStrideNd(DimsHW{1, 1});
            cls->setPaddingNd(DimsHW{0, 0});
            cats.push_back(cat2(c, box->getOutput(0), cls->getOutput(0)));
        }
        // ---- detect tail (model.cpp:197-252): strides from the backbone maps, flatten, split, DFL, re-join along axis 1
        std::vector<int> strides;
        for (ITensor* t : {conv3, conv5, conv7}) strides.push_back(cfg.input_h / (int)t->getDimensions().d[2]);
        std::vector<ITensor*> dets;
        for (int lv = 0; lv < 3; ++lv) {
            const int grid = (cfg.input_h / strides[lv]) * (cfg.input_w / strides[lv]);
            auto* flat = net->addShuffle(*cats[lv]);
            flat->setReshapeDimensions(Dims3{B, 64 + nc, grid});
            ITensor* boxPart = net->addSlice(*flat->getOutput(0), Dims3{0, 0, 0}, Dims3{B, 64, grid}, Dims3{1, 1, 1})->getOutput(0);
            ITensor* clsPart = net->addSlice(*flat->getOutput(0), Dims3{0, 64, 0}, Dims3{B, nc, grid}, Dims3{1, 1, 1})->getOutput(0);
            ITensor* v[] = {DFL(c, *boxPart, B, grid, "model.23.dfl.conv.weight"), clsPart};
            auto* cat = net->addConcatenation(v, 2);
            cat->setAxis(1);
            dets.push_back(cat->getOutput(0));
        }
        if (cfg.mark_heads)
            for (size_t i = 0; i < dets.size(); ++i) {
                dets[i]->setName(("head" + std::to_string(i)).c_str());
                net->markOutput(*dets[i]);
            }
        // addYoLoLayer (block.cpp:235-277): "combinedInfo" = {classes, W, H, maxOut, strides...}, the 6-float form of YoloLayer_TRT
        IPluginV2Layer* yolo = blocks::addYoLoLayer(c, dets, strides, {nc, cfg.input_w, cfg.input_h, cfg.max_out_bbox});
        assert(yolo);
        yolo->getOutput(0)->setName("output");
        net->markOutput(*yolo->getOutput(0));

        config->setMaxWorkspaceSize(16 * (1 << 20));
        if (cfg.fp16) config->setFlag(BuilderFlag::kFP16);
        plan = builder->buildSerializedNetwork(*net, *config);
    }
    delete net;
    freeWeights(wm);
    return plan;
}

}  // namespace trtx_host
