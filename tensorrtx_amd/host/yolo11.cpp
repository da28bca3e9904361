// YOLO11 detection network through the network-definition API, explicit batch like the reference.
// Mirrors the reference blocks and builder:
//   convBnSiLU / bottleneck / SPPF / DFL / addYoLoLayer / C3k / C3K2 / convBn / Attention / PSABlock / C2PSA / DWConv
//                                                              yolo11/src/block.cpp:73-437
//   get_width / get_depth / calculateStrides / buildEngineYolo11Det   yolo11/src/model.cpp:9-31, 138-400
//   Proto / cv4_conv_combined / buildEngineYolo11{Seg,Pose,Obb}       yolo11/src/model.cpp:412-1389
//   buildEngineYolo11Cls                                             yolo11/src/model.cpp:33-136
// Graph, weight keys ("model.<n>...") and layer order are those of the reference.
// Only PSABlock, C2PSA, Proto and the classifier are this file's; every other block, the detect head and tail (detect_v8) and the build
// session are the shared ones (yolo_blocks.h, build.h).
#include <cmath>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

ITensor* PSABlock(Ctx& c, ITensor& in, int dim, float attn_ratio, int num_heads, bool shortcut, const std::string& lname) {  // block.cpp:341-364
    ITensor* a = Attention(c, in, dim, num_heads, attn_ratio, lname + ".attn");
    ITensor* x = shortcut ? sum(c, in, *a) : a;
    ITensor* f0 = convBnSiLU(c, *x, dim * 2, 1, 1, lname + ".ffn.0");
    ITensor* f1 = convBn(c, *f0, dim, 1, 1, lname + ".ffn.1");
    return shortcut ? sum(c, *x, *f1) : f1;
}

ITensor* C2PSA(Ctx& c, ITensor& in, int c1, int c2, int n, float e, const std::string& lname) {  // block.cpp:366-415
    const int ch = (int)(c1 * e);
    ITensor *s1, *y;
    halves(c, *convBnSiLU(c, in, 2 * ch, 1, 1, lname + ".cv1"), &s1, &y);
    for (int i = 0; i < n; ++i) y = PSABlock(c, *y, ch, 0.5f, ch / 64, true, lname + ".m." + std::to_string(i));
    return convBnSiLU(c, *cat2(c, s1, y), c2, 1, 1, lname + ".cv2");
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

// the backbone to model.8, which detection and the classifier share (model.cpp:156-197, 52-90); `maps`: conv3, conv5, conv7 (the strides)
// and conv4, conv6 (the neck's laterals)
ITensor* backbone(Ctx& c, ITensor* data, const Yolo11Config& cfg, ITensor** maps) {
    const float gd = cfg.gd;
    auto W = [&](int x) { return get_width(x, cfg.gw, cfg.max_channels); };
    ITensor* conv0 = convBnSiLU(c, *data, W(64), 3, 2, "model.0");
    ITensor* conv1 = convBnSiLU(c, *conv0, W(128), 3, 2, "model.1");
    ITensor* conv2 = C3K2(c, *conv1, W(256), get_depth(2, gd), cfg.c3k, true, 0.25f, "model.2");
    ITensor* conv3 = convBnSiLU(c, *conv2, W(256), 3, 2, "model.3");
    ITensor* conv4 = C3K2(c, *conv3, W(512), get_depth(2, gd), cfg.c3k, true, 0.25f, "model.4");
    ITensor* conv5 = convBnSiLU(c, *conv4, W(512), 3, 2, "model.5");
    ITensor* conv6 = C3K2(c, *conv5, W(512), get_depth(2, gd), true, true, 0.5f, "model.6");
    ITensor* conv7 = convBnSiLU(c, *conv6, W(1024), 3, 2, "model.7");
    ITensor* all[] = {conv3, conv5, conv7, conv4, conv6};
    for (int i = 0; i < 5; ++i) maps[i] = all[i];
    return C3K2(c, *conv7, W(1024), get_depth(2, gd), true, true, 0.5f, "model.8");
}

// buildEngineYolo11Cls (model.cpp:33-136): the backbone to model.8, C2PSA as model.9 (no SPPF), then model.10: 1x1 convBnSiLU to
// 1280, average pool over the whole map, (B, 1280) x linear.weight^T + linear.bias
IHostMemory* buildCls(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolo11Config& cfg) {
    Session s(builder, wts, cfg.batch);
    Ctx& c = s.c;
    const int B = cfg.batch, nc = cfg.num_class;
    const int w1024 = get_width(1024, cfg.gw, cfg.max_channels);
    ITensor* maps[5];
    ITensor* x = backbone(c, s.input("images", cfg.input_h, cfg.input_w), cfg, maps);
    x = C2PSA(c, *x, w1024, w1024, get_depth(2, cfg.gd), 0.5f, "model.9");
    ITensor* head = convBnSiLU(c, *x, 1280, 1, 1, "model.10.conv");
    const Dims d = head->getDimensions();
    auto* pool = s.net->addPoolingNd(*head, PoolingType::kAVERAGE, DimsHW{(int)d.d[2], (int)d.d[3]});
    assert(pool);
    auto* flat = s.net->addShuffle(*pool->getOutput(0));
    flat->setReshapeDimensions(Dims2{B, 1280});
    ITensor* w = s.net->addConstant(Dims2{nc, 1280}, need(s.wm, "model.10.linear.weight"))->getOutput(0);
    // The reference declares the bias as Dims2{kBatchSize, kClsNumClass} over kClsNumClass values (model.cpp:104-105), which
    // holds only for kBatchSize = 1.  Here it is (1, classes) and the element-wise sum broadcasts it over the batch.
    ITensor* bias = s.net->addConstant(Dims2{1, nc}, need(s.wm, "model.10.linear.bias"))->getOutput(0);
    ITensor* mm = s.net->addMatrixMultiply(*flat->getOutput(0), MatrixOperation::kNONE, *w, MatrixOperation::kTRANSPOSE)->getOutput(0);
    s.output(sum(c, *mm, *bias), "output");
    return s.finish(builder, config, B, cfg.fp16);
}

}  // namespace

bool yolo11_scale(char type, Yolo11Scale* cfg) {  // yolo11_det.cpp:120-150, yolo12_det.cpp:120-150
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
    Session s(builder, wts, cfg.batch);
    Ctx& c = s.c;
    const float gd = cfg.gd;
    const int nc = cfg.num_class;
    const bool c3k = cfg.c3k;
    auto W = [&](int x) { return get_width(x, cfg.gw, cfg.max_channels); };

    // ---- backbone (model.cpp:156-199)
    ITensor* maps[5];
    ITensor* conv8 = backbone(c, s.input("images", cfg.input_h, cfg.input_w), cfg, maps);
    ITensor *conv4 = maps[3], *conv6 = maps[4];
    ITensor* conv9 = SPPF(c, *conv8, W(1024), W(1024), 5, "model.9");
    ITensor* conv10 = C2PSA(c, *conv9, W(1024), W(1024), get_depth(2, gd), 0.5f, "model.10");
    // ---- neck (model.cpp:203-254)
    ITensor* conv13 = C3K2(c, *cat2(c, upsample2x(c, *conv10), conv6), W(512), get_depth(2, gd), c3k, true, 0.5f, "model.13");
    ITensor* conv16 = C3K2(c, *cat2(c, upsample2x(c, *conv13), conv4), W(256), get_depth(2, gd), c3k, true, 0.5f, "model.16");
    ITensor* conv17 = convBnSiLU(c, *conv16, W(256), 3, 2, "model.17");
    ITensor* conv19 = C3K2(c, *cat2(c, conv17, conv13), W(512), get_depth(2, gd), c3k, true, 0.5f, "model.19");
    ITensor* conv20 = convBnSiLU(c, *conv19, W(512), 3, 2, "model.20");
    ITensor* conv22 = C3K2(c, *cat2(c, conv20, conv10), W(1024), get_depth(2, gd), true, true, 0.5f, "model.22");

    // ---- detect head (model.cpp:259-334) and tail (:336-390); cv4_conv_combined (:474-507): the task's extra channels are 32 mask
    // coefficients, 3 * nk keypoint values or kObbNe = 1 angle logit
    DetectV8 h{"model.23.", "model.23.dfl.conv.weight", true, std::max(std::max(16, W(256) / 4), 16 * 4), std::max(W(256), std::min(nc, 100)),
               nc, cfg.batch, cfg.input_h, cfg.input_w, cfg.task};
    h.cv4_out = cfg.task == 1 ? 32 : (cfg.task == 2 ? cfg.num_points * 3 : 1);
    h.cv4_mid = std::max(W(256) / 4, h.cv4_out);
    const std::vector<int> strides = strides_from(cfg.input_h, {maps[0], maps[1], maps[2]});
    const std::vector<ITensor*> dets = detect_v8(c, h, {conv16, conv19, conv22}, strides);
    if (cfg.mark_heads) s.mark_heads(dets);
    // the 9 netinfo fields of block.cpp:162-205 (the keypoint threshold truncated to int like the reference)
    IPluginV2Layer* yolo = addYoLoLayer(c, dets, strides, {nc, cfg.num_points, (int)cfg.kpt_conf, cfg.input_w, cfg.input_h, cfg.max_out_bbox,
                                                          cfg.task == 1, cfg.task == 2, cfg.task == 3});
    assert(yolo);
    s.output(yolo->getOutput(0), "output");
    if (cfg.task == 1) s.output(proto(c, *conv16, W(256)), "proto");   // model.cpp:765-767
    return s.finish(builder, config, cfg.batch, cfg.fp16);
}

}  // namespace trtx_host
