// YOLOv12 detection network through the network-definition API, explicit batch like the reference.
// Mirrors the reference blocks and builder:
//   convBnSiLU / bottleneck / DFL / addYoLoLayer / C3k / C3K2 / convBn / DWConv     yolov12/src/block.cpp:73-458 (yolo_blocks.h: the
//                                                                                   bodies are YOLO11's, and so are the detect head and tail)
//   A2C2f / ABlock / AAttn                                                         yolov12/src/block.cpp:459-625
//   get_width / get_depth / calculateStrides / buildEngineYolo12Det                yolov12/src/model.cpp:9-302
// Graph, weight keys ("model.<n>...") and layer order are those of the reference; where the reference is odd it is kept and said so.
#include <cmath>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

ITensor* transpose(Ctx& c, ITensor& in, Permutation p) {
    auto* sh = c.net->addShuffle(in);
    sh->setFirstTranspose(p);
    return sh->getOutput(0);
}

// AAttn (block.cpp:522-625), area attention.  `dim` is HALF the channel count of `in` (see A2C2f): head_dim = dim / num_heads = 16,
// the qkv convolution has all_head_dim * 3 * 2 = 6 dim outputs, and each head owns head_dim * 3 * 2 = 96 rows: q, k and v of 32 each.
// The scale is the constant 0.176777 the reference writes (32^-0.5 rounded to six digits), not a computed one.
//   qkv (B, 6 dim, H, W) -> (B, N, 6 dim) -> (B area, N / area, heads, 96) -> (B area, heads, 96, N / area) -> q | k | v slices
//   softmax(scale * q^T k) over the keys of the area, v @ attn^T -> (B area, N / area, heads, 32) -> (B, H, W, C) -> (B, C, H, W)
//   + pe(v brought to (B, C, H, W) the same way), a 7x7 depthwise convolution with bias and BN; then proj.
// Unlike the reference, which leaves the sizes to -1 and asserts nothing, a grid that `area` does not divide is an error (returns null).
ITensor* AAttn(Ctx& c, ITensor& in, int dim, int num_heads, int area, const std::string& lname) {
    const int head_dim = dim / num_heads;
    const int all_head_dim = head_dim * num_heads;
    const float scale = 0.176777f;
    const Dims d = in.getDimensions();
    int B = (int)d.d[0], C = (int)d.d[1], H = (int)d.d[2], W = (int)d.d[3], N = H * W;
    if (area < 1 || N % area != 0) return nullptr;
    ITensor* qkv = convBn(c, in, all_head_dim * 3 * 2, 1, 1, lname + ".qkv");
    auto* reshape = c.net->addShuffle(*qkv);
    reshape->setReshapeDimensions(Dims3{B, -1, N});
    reshape->setSecondTranspose(Permutation{0, 2, 1});
    if (area > 1) {
        B = B * area;
        N = N / area;
    }
    auto* reshape1 = c.net->addShuffle(*reshape->getOutput(0));
    reshape1->setReshapeDimensions(Dims4{B, N, num_heads, head_dim * 3 * 2});
    reshape1->setSecondTranspose(Permutation{0, 2, 3, 1});
    ITensor* x = reshape1->getOutput(0);
    const Dims dx = x->getDimensions();
    const int rows = (int)dx.d[2] / 3;
    const Dims4 part{dx.d[0], dx.d[1], rows, dx.d[3]}, unit{1, 1, 1, 1};
    ITensor* q = c.net->addSlice(*x, Dims4{0, 0, 0, 0}, part, unit)->getOutput(0);
    ITensor* k = c.net->addSlice(*x, Dims4{0, 0, rows, 0}, part, unit)->getOutput(0);
    ITensor* v = c.net->addSlice(*x, Dims4{0, 0, 2 * (int)dx.d[2] / 3, 0}, part, unit)->getOutput(0);
    ITensor* qT = transpose(c, *q, Permutation{0, 1, 3, 2});
    ITensor* attn = c.net->addMatrixMultiply(*qT, MatrixOperation::kNONE, *k, MatrixOperation::kNONE)->getOutput(0);
    attn = c.net->addScale(*attn, ScaleMode::kUNIFORM, c.scalar(0.f), c.scalar(scale), c.scalar(1.f))->getOutput(0);
    auto* sm = c.net->addSoftMax(*attn);
    sm->setAxes(1 << 3);
    ITensor* attnT = transpose(c, *sm->getOutput(0), Permutation{0, 1, 3, 2});
    ITensor* o = c.net->addMatrixMultiply(*v, MatrixOperation::kNONE, *attnT, MatrixOperation::kNONE)->getOutput(0);
    ITensor* oT = transpose(c, *o, Permutation{0, 3, 1, 2});
    if (area > 1) {
        B = B / area;
        N = N * area;
    }
    auto* reshape3 = c.net->addShuffle(*oT);
    reshape3->setReshapeDimensions(Dims4{B, H, W, -1});
    ITensor* oImg = transpose(c, *reshape3->getOutput(0), Permutation{0, 3, 1, 2});
    ITensor* vT = transpose(c, *v, Permutation{0, 3, 1, 2});
    auto* reshape4 = c.net->addShuffle(*vT);
    reshape4->setReshapeDimensions(Dims4{B, H, W, C});
    ITensor* vImg = transpose(c, *reshape4->getOutput(0), Permutation{0, 3, 1, 2});
    ITensor* pe = convBn(c, *vImg, all_head_dim * 2, 7, 1, lname + ".pe", all_head_dim * 2, /*bias=*/true);
    return convBn(c, *sum(c, *pe, *oImg), all_head_dim * 2, 1, 1, lname + ".proj");
}

// ABlock (block.cpp:497-520): x + AAttn(x), then + mlp.  `dim` is half the channel count (A2C2f), so mlp.0 has
// 2 * (int)(dim * mlp_ratio) outputs and mlp.1 has 2 * dim: written with the factor 2 as the reference does.
ITensor* ABlock(Ctx& c, ITensor& in, int dim, int num_heads, float mlp_ratio, int area, const std::string& lname) {
    const int mlp_hidden_dim = (int)(dim * mlp_ratio);
    ITensor* attn = AAttn(c, in, dim, num_heads, area, lname + ".attn");
    if (!attn) return nullptr;
    ITensor* x = sum(c, in, *attn);
    ITensor* mlp1 = convBnSiLU(c, *x, mlp_hidden_dim * 2, 1, 1, lname + ".mlp.0");
    ITensor* mlp2 = convBn(c, *mlp1, dim * 2, 1, 1, lname + ".mlp.1");
    return sum(c, *x, *mlp2);
}

// A2C2f (block.cpp:459-495).  The reference computes c = c2 * e with e = 0.25 where ultralytics has e = 0.5, and then uses 2c for cv1 and
// for everything the blocks see, while handing c to ABlock as `dim`; num_heads = c / 32 * 2 is therefore 2c / 32.  `n`, `residual` and
// `g` are accepted and unused there (four ABlocks, or one C3k, whatever n says; no gamma): this signature drops them.
ITensor* A2C2f(Ctx& c, ITensor& in, int c2, bool a2, int area, float mlp_ratio, float e, bool shortcut, const std::string& lname) {
    const int ch = (int)((float)c2 * e);
    const int num_heads = ch / 32 * 2;
    ITensor* cv1 = convBnSiLU(c, in, ch * 2, 1, 1, lname + ".cv1");
    if (a2) {
        if (num_heads < 1) return nullptr;
        ITensor* y = cv1;
        ITensor* parts[3] = {cv1, nullptr, nullptr};
        static const char* const names[4] = {".m.0.0", ".m.0.1", ".m.1.0", ".m.1.1"};
        for (int i = 0; i < 4; ++i) {
            y = ABlock(c, *y, ch, num_heads, mlp_ratio, area, lname + names[i]);
            if (!y) return nullptr;
            if (i & 1) parts[1 + i / 2] = y;
        }
        return convBnSiLU(c, *cat(c, {parts[0], parts[1], parts[2]}), c2, 1, 1, lname + ".cv2");
    }
    ITensor* y = C3k(c, *cv1, ch * 2, 2, shortcut, 0.5f, lname + ".m.0");
    return convBnSiLU(c, *cat2(c, cv1, y), c2, 1, 1, lname + ".cv2");
}

}  // namespace

IHostMemory* buildEngineYolo12Det(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolo12Config& cfg) {
    Session s(builder, wts, cfg.batch);
    Ctx& c = s.c;
    const float gd = cfg.gd;
    const int nc = cfg.num_class;
    const bool c3k = cfg.c3k;
    auto W = [&](int x) { return get_width(x, cfg.gw, cfg.max_channels); };

    ITensor* data = s.input("images", cfg.input_h, cfg.input_w);
    // ---- backbone (model.cpp:52-88): A2C2f with area attention at stride 16 (area 4) and stride 32 (area 1)
    ITensor* conv0 = convBnSiLU(c, *data, W(64), 3, 2, "model.0");
    ITensor* conv1 = convBnSiLU(c, *conv0, W(128), 3, 2, "model.1");
    ITensor* conv2 = C3K2(c, *conv1, W(256), get_depth(2, gd), c3k, true, 0.25f, "model.2");
    ITensor* conv3 = convBnSiLU(c, *conv2, W(256), 3, 2, "model.3");
    ITensor* conv4 = C3K2(c, *conv3, W(512), get_depth(2, gd), c3k, true, 0.25f, "model.4");
    ITensor* conv5 = convBnSiLU(c, *conv4, W(512), 3, 2, "model.5");
    ITensor* conv6 = A2C2f(c, *conv5, W(512), true, 4, 2.0f, 0.25f, true, "model.6");
    if (!conv6) return nullptr;   // the grid is not divisible by the area count
    ITensor* conv7 = convBnSiLU(c, *conv6, W(1024), 3, 2, "model.7");
    ITensor* conv8 = A2C2f(c, *conv7, W(1024), true, 1, 2.0f, 0.25f, true, "model.8");
    if (!conv8) return nullptr;
    // ---- head (model.cpp:94-135): the A2C2f blocks here take the C3k branch (a2 = false)
    ITensor* conv11 = A2C2f(c, *cat2(c, upsample2x(c, *conv8), conv6), W(512), false, 1, 2.0f, 0.25f, true, "model.11");
    ITensor* conv14 = A2C2f(c, *cat2(c, upsample2x(c, *conv11), conv4), W(256), false, 1, 2.0f, 0.25f, true, "model.14");
    ITensor* conv15 = convBnSiLU(c, *conv14, W(256), 3, 2, "model.15");
    ITensor* conv17 = A2C2f(c, *cat2(c, conv15, conv11), W(512), false, 1, 2.0f, 0.25f, true, "model.17");
    ITensor* conv18 = convBnSiLU(c, *conv17, W(512), 3, 2, "model.18");
    ITensor* conv20 = C3K2(c, *cat2(c, conv18, conv8), W(1024), get_depth(2, gd), true, true, 0.5f, "model.20");

    // ---- detect head (model.cpp:141-229) and tail (:235-290)
    const DetectV8 h{"model.21.", "model.21.dfl.conv.weight", true, std::max(std::max(16, W(256) / 4), 16 * 4), std::max(W(256), std::min(nc, 100)),
                     nc, cfg.batch, cfg.input_h, cfg.input_w};
    const std::vector<int> strides = strides_from(cfg.input_h, {conv3, conv5, conv7});
    const std::vector<ITensor*> dets = detect_v8(c, h, {conv14, conv17, conv20}, strides);
    if (cfg.mark_heads) s.mark_heads(dets);
    // model.cpp:292-294: detection only (is_seg, is_pose, is_obb all false; the keypoint fields are the config's constants)
    IPluginV2Layer* yolo = addYoLoLayer(c, dets, strides, {nc, 17, 0, cfg.input_w, cfg.input_h, cfg.max_out_bbox, 0, 0, 0});
    assert(yolo);
    s.output(yolo->getOutput(0), "output");
    return s.finish(builder, config, cfg.batch, cfg.fp16);
}

}  // namespace trtx_host
