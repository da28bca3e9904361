// YOLO11 detection network through the network-definition API, explicit batch like the reference.
// Mirrors the reference blocks and builder:
//   convBnSiLU / bottleneck / SPPF / DFL / addYoLoLayer / C3k / C3K2 / convBn / Attention / PSABlock / C2PSA / DWConv
//                                                              yolo11/src/block.cpp:73-437
//   get_width / get_depth / calculateStrides / buildEngineYolo11Det   yolo11/src/model.cpp:9-31, 138-400
//   Proto / cv4_conv_combined / buildEngineYolo11{Seg,Pose,Obb}       yolo11/src/model.cpp:412-1389
//   buildEngineYolo11Cls                                             yolo11/src/model.cpp:33-136
// Graph, weight keys ("model.<n>...") and layer order are those of the reference.
// The blocks that YOLOv12 restates with the same bodies (convBnSiLU, convBn, bottleneck, C3k, C3K2, DWConv, DFL, addYoLoLayer, get_width,
// get_depth) live in yolo_blocks.h, and so do SPPF and Attention, which YOLOv10 restates.
#include <cmath>
#include <vector>

#include "common.h"
#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

ITensor* PSABlock(Ctx& c, ITensor& in, int dim, float attn_ratio, int num_heads, bool shortcut, const std::string& lname) {  // block.cpp:341-364
    ITensor* a = Attention(c, in, dim, num_heads, attn_ratio, lname + ".attn");
    ITensor* x = shortcut ? c.net->addElementWise(in, *a, ElementWiseOperation::kSUM)->getOutput(0) : a;
    ITensor* f0 = convBnSiLU(c, *x, dim * 2, 1, 1, lname + ".ffn.0");
    ITensor* f1 = convBn(c, *f0, dim, 1, 1, lname + ".ffn.1");
    return shortcut ? c.net->addElementWise(*x, *f1, ElementWiseOperation::kSUM)->getOutput(0) : f1;
}

ITensor* C2PSA(Ctx& c, ITensor& in, int c1, int c2, int n, float e, const std::string& lname) {  // block.cpp:366-415
    const int ch = (int)(c1 * e);
    ITensor* cv1 = convBnSiLU(c, in, 2 * ch, 1, 1, lname + ".cv1");
    const Dims d = cv1->getDimensions();
    const Dims4 half{d.d[0], d.d[1] / 2, d.d[2], d.d[3]}, unit{1, 1, 1, 1};
    ITensor* s1 = c.net->addSlice(*cv1, Dims4{0, 0, 0, 0}, half, unit)->getOutput(0);
    ITensor* y = c.net->addSlice(*cv1, Dims4{0, d.d[1] / 2, 0, 0}, half, unit)->getOutput(0);
    for (int i = 0; i < n; ++i) y = PSABlock(c, *y, ch, 0.5f, ch / 64, true, lname + ".m." + std::to_string(i));
    return convBnSiLU(c, *cat2(c, s1, y), c2, 1, 1, lname + ".cv2");
}

// the 9 netinfo fields of block.cpp:162-205 (the keypoint threshold truncated to int like the reference)
IPluginV2Layer* addYoLoLayer(Ctx& c, const std::vector<ITensor*>& dets, const std::vector<int>& strides, const Yolo11Config& cfg) {
    return blocks::addYoLoLayer(c, dets, strides, {cfg.num_class, cfg.num_points, (int)cfg.kpt_conf, cfg.input_w, cfg.input_h, cfg.max_out_bbox,
                                                   cfg.task == 1, cfg.task == 2, cfg.task == 3});
}

// cv4_conv_combined (model.cpp:474-507): two 3x3 convBnSiLU to c4, a biased 1x1 conv to the task's extra channels (32 mask
// coefficients, 3 * nk keypoint values or kObbNe = 1 angle logit), reshaped to (B, extra, grid)
ITensor* cv4Branch(Ctx& c, ITensor& in, const std::string& lname, int B, int grid, int w256, const Yolo11Config& cfg) {
    const int extra = cfg.task == 1 ? 32 : (cfg.task == 2 ? cfg.num_points * 3 : 1);
    const int c4 = std::max(w256 / 4, extra);
    ITensor* a = convBnSiLU(c, in, c4, 3, 1, lname + ".0");
    ITensor* b = convBnSiLU(c, *a, c4, 3, 1, lname + ".1");
    auto* cv = c.net->addConvolutionNd(*b, extra, DimsHW{1, 1}, need(c.wm, lname + ".2.weight"), need(c.wm, lname + ".2.bias"));
    assert(cv);
    cv->setStrideNd(DimsHW{1, 1});
    auto* sh = c.net->addShuffle(*cv->getOutput(0));
    sh->setReshapeDimensions(Dims3{B, extra, grid});
    return sh->getOutput(0);
}

// Proto (model.cpp:412-472): 3x3 convBnSiLU -> 2x2 stride-2 deconvolution with bias -> 3x3 convBnSiLU -> 1x1 convBnSiLU to 32
ITensor* proto(Ctx& c, ITensor& in, int mid) {
    ITensor* a = convBnSiLU(c, in, mid, 3, 1, "model.23.proto.cv1");
    auto* up = c.net->addDeconvolutionNd(*a, mid, DimsHW{2, 2}, need(c.wm, "model.23.proto.upsample.weight"),
                                         need(c.wm, "model.23.proto.upsample.bias"));
    assert(up);
    up->setStrideNd(DimsHW{2, 2});
    up->setPaddingNd(DimsHW{0, 0});
    ITensor* b = convBnSiLU(c, *up->getOutput(0), mid, 3, 1, "model.23.proto.cv2");
    return convBnSiLU(c, *b, 32, 1, 1, "model.23.proto.cv3");
}

// buildEngineYolo11Cls (model.cpp:33-136): the backbone to model.8, C2PSA as model.9 (no SPPF), then model.10: 1x1 convBnSiLU to
// 1280, average pool over the whole map, (B, 1280) x linear.weight^T + linear.bias
IHostMemory* buildCls(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolo11Config& cfg) {
    WeightMap wm = loadWeights(wts);
    INetworkDefinition* net = builder->createNetworkV2(1U << static_cast<uint32_t>(NetworkDefinitionCreationFlag::kEXPLICIT_BATCH));
    IHostMemory* plan = nullptr;
    {
        Ctx c{net, wm, {}};
        const float gd = cfg.gd, gw = cfg.gw;
        const int mc = cfg.max_channels, B = cfg.batch, nc = cfg.num_class;
        const bool c3k = cfg.c3k;
        auto W = [&](int x) { return get_width(x, gw, mc); };
        ITensor* data = net->addInput("images", DataType::kFLOAT, Dims4{B, 3, cfg.input_h, cfg.input_w});
        assert(data);
        ITensor* x = convBnSiLU(c, *data, W(64), 3, 2, "model.0");
        x = convBnSiLU(c, *x, W(128), 3, 2, "model.1");
        x = C3K2(c, *x, W(256), get_depth(2, gd), c3k, true, 0.25f, "model.2");
        x = convBnSiLU(c, *x, W(256), 3, 2, "model.3");
        x = C3K2(c, *x, W(512), get_depth(2, gd), c3k, true, 0.25f, "model.4");
        x = convBnSiLU(c, *x, W(512), 3, 2, "model.5");
        x = C3K2(c, *x, W(512), get_depth(2, gd), true, true, 0.5f, "model.6");
        x = convBnSiLU(c, *x, W(1024), 3, 2, "model.7");
        x = C3K2(c, *x, W(1024), get_depth(2, gd), true, true, 0.5f, "model.8");
        x = C2PSA(c, *x, W(1024), W(1024), get_depth(2, gd), 0.5f, "model.9");
        ITensor* head = convBnSiLU(c, *x, 1280, 1, 1, "model.10.conv");
        const Dims d = head->getDimensions();
        auto* pool = net->addPoolingNd(*head, PoolingType::kAVERAGE, DimsHW{(int)d.d[2], (int)d.d[3]});
        assert(pool);
        auto* flat = net->addShuffle(*pool->getOutput(0));
        flat->setReshapeDimensions(Dims2{B, 1280});
        ITensor* w = net->addConstant(Dims2{nc, 1280}, need(wm, "model.10.linear.weight"))->getOutput(0);
        // The reference declares the bias as Dims2{kBatchSize, kClsNumClass} over kClsNumClass values (model.cpp:104-105), which
        // holds only for kBatchSize = 1.  Here it is (1, classes) and the element-wise sum broadcasts it over the batch.
        ITensor* bias = net->addConstant(Dims2{1, nc}, need(wm, "model.10.linear.bias"))->getOutput(0);
        ITensor* mm = net->addMatrixMultiply(*flat->getOutput(0), MatrixOperation::kNONE, *w, MatrixOperation::kTRANSPOSE)->getOutput(0);
        ITensor* y = net->addElementWise(*mm, *bias, ElementWiseOperation::kSUM)->getOutput(0);
        y->setName("output");
        net->markOutput(*y);
        config->setMaxWorkspaceSize(16 * (1 << 20));
        if (cfg.fp16) config->setFlag(BuilderFlag::kFP16);
        plan = builder->buildSerializedNetwork(*net, *config);
    }
    delete net;
    freeWeights(wm);
    return plan;
}

}  // namespace

bool yolo11_scale(char type, Yolo11Config* cfg) {  // yolo11_det.cpp:120-150
    switch (type) {
        case 'n': cfg->gd = 0.50f; cfg->gw = 0.25f; cfg->max_channels = 1024; break;
        case 's': cfg->gd = 0.50f; cfg->gw = 0.50f; cfg->max_channels = 1024; break;
        case 'm': cfg->gd = 0.50f; cfg->gw = 1.00f; cfg->max_channels = 512; break;
        case 'l': cfg->gd = 1.00f; cfg->gw = 1.00f; cfg->max_channels = 512; break;
        case 'x': cfg->gd = 1.00f; cfg->gw = 1.50f; cfg->max_channels = 512; break;
        default: return false;
    }
    cfg->c3k = type == 'm' || type == 'l' || type == 'x';   // model.cpp:160-163
    return true;
}

IHostMemory* buildEngineYolo11Det(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolo11Config& cfg) {
    if (cfg.task == 4) return buildCls(builder, config, wts, cfg);
    if (cfg.task < 0 || cfg.task > 4) return nullptr;
    WeightMap wm = loadWeights(wts);
    INetworkDefinition* net = builder->createNetworkV2(1U << static_cast<uint32_t>(NetworkDefinitionCreationFlag::kEXPLICIT_BATCH));
    IHostMemory* plan = nullptr;
    {
        Ctx c{net, wm, {}};
        const float gd = cfg.gd, gw = cfg.gw;
        const int mc = cfg.max_channels, B = cfg.batch, nc = cfg.num_class;
        const bool c3k = cfg.c3k;
        auto W = [&](int x) { return get_width(x, gw, mc); };

        ITensor* data = net->addInput("images", DataType::kFLOAT, Dims4{B, 3, cfg.input_h, cfg.input_w});
        assert(data);
        // ---- backbone (model.cpp:156-199)
        ITensor* conv0 = convBnSiLU(c, *data, W(64), 3, 2, "model.0");
        ITensor* conv1 = convBnSiLU(c, *conv0, W(128), 3, 2, "model.1");
        ITensor* conv2 = C3K2(c, *conv1, W(256), get_depth(2, gd), c3k, true, 0.25f, "model.2");
        ITensor* conv3 = convBnSiLU(c, *conv2, W(256), 3, 2, "model.3");
        ITensor* conv4 = C3K2(c, *conv3, W(512), get_depth(2, gd), c3k, true, 0.25f, "model.4");
        ITensor* conv5 = convBnSiLU(c, *conv4, W(512), 3, 2, "model.5");
        ITensor* conv6 = C3K2(c, *conv5, W(512), get_depth(2, gd), true, true, 0.5f, "model.6");
        ITensor* conv7 = convBnSiLU(c, *conv6, W(1024), 3, 2, "model.7");
        ITensor* conv8 = C3K2(c, *conv7, W(1024), get_depth(2, gd), true, true, 0.5f, "model.8");
        ITensor* conv9 = SPPF(c, *conv8, W(1024), W(1024), 5, "model.9");
        ITensor* conv10 = C2PSA(c, *conv9, W(1024), W(1024), get_depth(2, gd), 0.5f, "model.10");
        // ---- neck (model.cpp:203-254)
        ITensor* conv13 = C3K2(c, *cat2(c, upsample2x(c, *conv10), conv6), W(512), get_depth(2, gd), c3k, true, 0.5f, "model.13");
        ITensor* conv16 = C3K2(c, *cat2(c, upsample2x(c, *conv13), conv4), W(256), get_depth(2, gd), c3k, true, 0.5f, "model.16");
        ITensor* conv17 = convBnSiLU(c, *conv16, W(256), 3, 2, "model.17");
        ITensor* conv19 = C3K2(c, *cat2(c, conv17, conv13), W(512), get_depth(2, gd), c3k, true, 0.5f, "model.19");
        ITensor* conv20 = convBnSiLU(c, *conv19, W(512), 3, 2, "model.20");
        ITensor* conv22 = C3K2(c, *cat2(c, conv20, conv10), W(1024), get_depth(2, gd), true, true, 0.5f, "model.22");

        // ---- detect head (model.cpp:259-334): per level a 64-channel box branch and a DWConv class branch
        const int c2 = std::max(std::max(16, W(256) / 4), 16 * 4);
        const int c3 = std::max(W(256), std::min(nc, 100));
        ITensor* feats[3] = {conv16, conv19, conv22};
        const int feat_w[3] = {W(256), W(512), W(1024)};
        std::vector<ITensor*> cats;
        for (int lv = 0; lv < 3; ++lv) {
            const std::string s = "model.23.cv2." + std::to_string(lv), t = "model.23.cv3." + std::to_string(lv);
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
        // ---- detect tail (model.cpp:336-390): strides from the backbone maps, flatten, split, DFL, re-join along axis 1
        std::vector<int> strides;
        for (ITensor* t : {conv3, conv5, conv7}) strides.push_back(cfg.input_h / (int)t->getDimensions().d[2]);
        std::vector<ITensor*> dets;
        std::vector<std::pair<ITensor*, ITensor*>> tails;
        for (int lv = 0; lv < 3; ++lv) {
            const int grid = (cfg.input_h / strides[lv]) * (cfg.input_w / strides[lv]);
            auto* flat = net->addShuffle(*cats[lv]);
            flat->setReshapeDimensions(Dims3{B, 64 + nc, grid});
            ITensor* boxPart = net->addSlice(*flat->getOutput(0), Dims3{0, 0, 0}, Dims3{B, 64, grid}, Dims3{1, 1, 1})->getOutput(0);
            ITensor* clsPart = net->addSlice(*flat->getOutput(0), Dims3{0, 64, 0}, Dims3{B, nc, grid}, Dims3{1, 1, 1})->getOutput(0);
            ITensor* dfl = DFL(c, *boxPart, B, grid, "model.23.dfl.conv.weight");
            if (cfg.task == 0) {
                ITensor* v[] = {dfl, clsPart};
                auto* cat = net->addConcatenation(v, 2);
                cat->setAxis(1);
                dets.push_back(cat->getOutput(0));
            } else if (cfg.task == 2) {   // pose joins each level right after its DFL: [dfl(4), classes, keypoints] (model.cpp:1000-1060)
                ITensor* v[] = {dfl, clsPart, cv4Branch(c, *feats[lv], "model.23.cv4." + std::to_string(lv), B, grid, W(256), cfg)};
                auto* cat = net->addConcatenation(v, 3);
                cat->setAxis(1);
                dets.push_back(cat->getOutput(0));
            } else {                      // seg / obb finish all three DFL tails first (model.cpp:695-730, 1290-1330)
                tails.push_back({dfl, clsPart});
            }
        }
        for (size_t lv = 0; lv < tails.size(); ++lv) {   // seg / obb: [dfl(4), classes, mask coefficients | angle] (model.cpp:732-756, 1332-1358)
            const int grid = (cfg.input_h / strides[lv]) * (cfg.input_w / strides[lv]);
            ITensor* v[] = {tails[lv].first, tails[lv].second,
                            cv4Branch(c, *feats[lv], "model.23.cv4." + std::to_string(lv), B, grid, W(256), cfg)};
            auto* cat = net->addConcatenation(v, 3);
            cat->setAxis(1);
            dets.push_back(cat->getOutput(0));
        }
        if (cfg.mark_heads)
            for (size_t i = 0; i < dets.size(); ++i) {
                dets[i]->setName(("head" + std::to_string(i)).c_str());
                net->markOutput(*dets[i]);
            }
        IPluginV2Layer* yolo = addYoLoLayer(c, dets, strides, cfg);
        assert(yolo);
        yolo->getOutput(0)->setName("output");
        net->markOutput(*yolo->getOutput(0));
        if (cfg.task == 1) {   // model.cpp:765-767
            ITensor* pr = proto(c, *conv16, W(256));
            pr->setName("proto");
            net->markOutput(*pr);
        }

        config->setMaxWorkspaceSize(16 * (1 << 20));
        if (cfg.fp16) config->setFlag(BuilderFlag::kFP16);
        plan = builder->buildSerializedNetwork(*net, *config);
    }
    delete net;
    freeWeights(wm);
    return plan;
}

}  // namespace trtx_host
