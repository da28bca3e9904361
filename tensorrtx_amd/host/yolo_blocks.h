// Blocks that the YOLO11 and YOLOv12 builders share, written against the network-definition API.  The reference restates them per model
// with the same bodies (yolo11/src/block.cpp and yolov12/src/block.cpp: convBnSiLU, convBn, bottleneck, C3k, C3K2, DWConv, DFL,
// addYoLoLayer; get_width / get_depth in both model.cpp); line numbers in the comments are yolo11's unless a builder says otherwise.
// YOLOv10 restates convBnSiLU, convBn, bottleneck, SPPF, DFL, Attention, get_width and get_depth once more (yolov10/src/block.cpp,
// model.cpp:9-22) and adds C2F, SCDown, PSA, RepVGGDW, CIB and C2fCIB, which are here too.
#pragma once
#include <cassert>
#include <cmath>
#include <string>
#include <vector>

#include "common.h"

namespace trtx_host {
namespace blocks {
using namespace nvinfer1;

inline int get_width(int x, float gw, int max_channels, int divisor = 8) {  // model.cpp:9-13 (YOLO11 caps before scaling, unlike v8)
    const int ch = std::min(x, max_channels);
    return int(ceil((ch * gw) / divisor)) * divisor;
}

inline int get_depth(int x, float gd) {  // model.cpp:15-22
    if (x == 1) return 1;
    int r = (int)round(x * gd);
    if (x * gd - int(x * gd) == 0.5 && (int(x * gd) % 2) == 0) --r;
    return std::max<int>(r, 1);
}

struct Ctx {
    INetworkDefinition* net;
    WeightMap& wm;
    std::vector<float*> owned;   // the Attention's 1-element scale weights (block.cpp:313-322), alive until the plan is built
    ~Ctx() {
        for (float* p : owned) delete[] p;
    }
    Weights scalar(float v) {
        float* p = new float[1]{v};
        owned.push_back(p);
        return Weights{DataType::kFLOAT, p, 1};
    }
};

// Conv (no bias, 'same' padding k/2, groups g) + BN (eps 1e-3)   (block.cpp:73-92 without the SiLU; convBn :271-285)
// `bias`: the convolution carries lname.conv.bias (YOLOv12's convBn does for names that hold ".pe", yolov12/src/block.cpp:282-296)
inline ITensor* convBn(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname, int g = 1, bool bias = false) {
    auto* conv = c.net->addConvolutionNd(in, ch, DimsHW{k, k}, need(c.wm, lname + ".conv.weight"),
                                         bias ? need(c.wm, lname + ".conv.bias") : noWeights());
    assert(conv);
    conv->setStrideNd(DimsHW{s, s});
    conv->setPaddingNd(DimsHW{k / 2, k / 2});
    if (g != 1) conv->setNbGroups(g);
    return addBatchNorm2d(c.net, c.wm, *conv->getOutput(0), lname + ".bn", 1e-3f)->getOutput(0);
}

// SiLU spelled Sigmoid * x (block.cpp:88-91)
inline ITensor* silu(Ctx& c, ITensor* x) {
    ITensor* sig = c.net->addActivation(*x, ActivationType::kSIGMOID)->getOutput(0);
    return c.net->addElementWise(*x, *sig, ElementWiseOperation::kPROD)->getOutput(0);
}

inline ITensor* convBnSiLU(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname) { return silu(c, convBn(c, in, ch, k, s, lname)); }

// DWConv: depthwise conv (groups = ch) + BN + SiLU (block.cpp:417-437)
inline ITensor* DWConv(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname) { return silu(c, convBn(c, in, ch, k, s, lname, ch)); }

inline ITensor* bottleneck(Ctx& c, ITensor& in, int c1, int c2, bool shortcut, float e, const std::string& lname) {  // block.cpp:94-109 (k 3x3, 3x3)
    const int c_ = (int)((float)c2 * e);
    ITensor* a = convBnSiLU(c, in, c_, 3, 1, lname + ".cv1");
    ITensor* b = convBnSiLU(c, *a, c2, 3, 1, lname + ".cv2");
    if (shortcut && c1 == c2) return c.net->addElementWise(in, *b, ElementWiseOperation::kSUM)->getOutput(0);
    return b;
}

inline ITensor* cat2(Ctx& c, ITensor* a, ITensor* b) {
    ITensor* v[] = {a, b};
    return c.net->addConcatenation(v, 2)->getOutput(0);
}

inline ITensor* C3k(Ctx& c, ITensor& in, int c2, int n, bool shortcut, float e, const std::string& lname) {  // block.cpp:207-224
    const int c_ = (int)((float)c2 * e);
    ITensor* y = convBnSiLU(c, in, c_, 1, 1, lname + ".cv1");
    ITensor* b = convBnSiLU(c, in, c_, 1, 1, lname + ".cv2");
    for (int i = 0; i < n; ++i) y = bottleneck(c, *y, c_, c_, shortcut, 1.0f, lname + ".m." + std::to_string(i));
    return convBnSiLU(c, *cat2(c, y, b), c2, 1, 1, lname + ".cv3");
}

// C3K2 (block.cpp:226-262): cv1 to 2c_, split in halves along channels, n C3k / bottleneck blocks on the second half, every
// result appended to the running concat, cv2
inline ITensor* C3K2(Ctx& c, ITensor& in, int c2, int n, bool c3k, bool shortcut, float e, const std::string& lname) {
    const int c_ = (int)((float)c2 * e);
    ITensor* cv1 = convBnSiLU(c, in, 2 * c_, 1, 1, lname + ".cv1");
    const Dims d = cv1->getDimensions();
    const Dims4 half{d.d[0], d.d[1] / 2, d.d[2], d.d[3]}, unit{1, 1, 1, 1};
    ITensor* s1 = c.net->addSlice(*cv1, Dims4{0, 0, 0, 0}, half, unit)->getOutput(0);
    ITensor* s2 = c.net->addSlice(*cv1, Dims4{0, d.d[1] / 2, 0, 0}, half, unit)->getOutput(0);
    ITensor* cat = cat2(c, s1, s2);
    ITensor* y = s2;
    for (int i = 0; i < n; ++i) {
        const std::string m = lname + ".m." + std::to_string(i);
        y = c3k ? C3k(c, *y, c_, 2, shortcut, 0.5f, m) : bottleneck(c, *y, c_, c_, shortcut, 0.5f, m);
        cat = cat2(c, cat, y);
    }
    return convBnSiLU(c, *cat, c2, 1, 1, lname + ".cv2");
}

inline ITensor* upsample2x(Ctx& c, ITensor& in) {  // model.cpp:205-209
    const float scale[] = {1.0f, 1.0f, 2.0f, 2.0f};
    auto* r = c.net->addResize(in);
    assert(r);
    r->setResizeMode(ResizeMode::kNEAREST);
    r->setScales(scale, 4);
    return r->getOutput(0);
}

inline ITensor* SPPF(Ctx& c, ITensor& in, int c1, int c2, int k, const std::string& lname) {  // block.cpp:111-138; yolov10/src/block.cpp:190-212
    ITensor* x = convBnSiLU(c, in, c1 / 2, 1, 1, lname + ".cv1");
    std::vector<ITensor*> parts{x};
    for (int i = 0; i < 3; ++i) {
        auto* pool = c.net->addPoolingNd(*parts.back(), PoolingType::kMAX, DimsHW{k, k});
        pool->setStrideNd(DimsHW{1, 1});
        pool->setPaddingNd(DimsHW{k / 2, k / 2});
        parts.push_back(pool->getOutput(0));
    }
    return convBnSiLU(c, *c.net->addConcatenation(parts.data(), 4)->getOutput(0), c2, 1, 1, lname + ".cv2");
}

// Attention (block.cpp:287-339; yolov10/src/block.cpp:297-358, the same layers in the same order): qkv 1x1 conv+BN, view (B, heads, 2*kd + hd, N), split q / k / v, softmax(scale * q^T k) over the
// keys, v @ attn^T viewed back as (B, dim, H, W), plus the depthwise positional conv pe(v), then proj 1x1 conv+BN
inline ITensor* Attention(Ctx& c, ITensor& in, int dim, int num_heads, float attn_ratio, const std::string& lname) {
    const int head_dim = dim / num_heads;
    const int key_dim = (int)(head_dim * attn_ratio);
    const float scale = (float)pow(key_dim, -0.5);
    const int nh_kd = key_dim * num_heads;
    const int h = dim + nh_kd * 2;
    const Dims d = in.getDimensions();
    const int B = (int)d.d[0], H = (int)d.d[2], W = (int)d.d[3], N = H * W;
    ITensor* qkv = convBn(c, in, h, 1, 1, lname + ".qkv");
    auto* sh = c.net->addShuffle(*qkv);
    sh->setReshapeDimensions(Dims4{B, num_heads, -1, N});
    ITensor* x = sh->getOutput(0);
    const Dims d1 = x->getDimensions();
    const Dims4 unit{1, 1, 1, 1};
    ITensor* q = c.net->addSlice(*x, Dims4{0, 0, 0, 0}, Dims4{d1.d[0], d1.d[1], key_dim, d1.d[3]}, unit)->getOutput(0);
    ITensor* k = c.net->addSlice(*x, Dims4{0, 0, key_dim, 0}, Dims4{d1.d[0], d1.d[1], key_dim, d1.d[3]}, unit)->getOutput(0);
    ITensor* v = c.net->addSlice(*x, Dims4{0, 0, key_dim * 2, 0}, Dims4{d1.d[0], d1.d[1], head_dim, d1.d[3]}, unit)->getOutput(0);
    auto* qT = c.net->addShuffle(*q);
    qT->setFirstTranspose(Permutation{0, 1, 3, 2});
    ITensor* attn = c.net->addMatrixMultiply(*qT->getOutput(0), MatrixOperation::kNONE, *k, MatrixOperation::kNONE)->getOutput(0);
    attn = c.net->addScale(*attn, ScaleMode::kUNIFORM, c.scalar(0.f), c.scalar(scale), c.scalar(1.f))->getOutput(0);
    auto* sm = c.net->addSoftMax(*attn);
    sm->setAxes(1 << 3);
    auto* attnT = c.net->addShuffle(*sm->getOutput(0));
    attnT->setFirstTranspose(Permutation{0, 1, 3, 2});
    ITensor* o = c.net->addMatrixMultiply(*v, MatrixOperation::kNONE, *attnT->getOutput(0), MatrixOperation::kNONE)->getOutput(0);
    auto* re = c.net->addShuffle(*o);
    re->setReshapeDimensions(Dims4{B, -1, H, W});
    auto* vre = c.net->addShuffle(*v);
    vre->setReshapeDimensions(Dims4{B, -1, H, W});
    ITensor* pe = convBn(c, *vre->getOutput(0), dim, 3, 1, lname + ".pe", dim);
    ITensor* sum = c.net->addElementWise(*re->getOutput(0), *pe, ElementWiseOperation::kSUM)->getOutput(0);
    return convBn(c, *sum, dim, 1, 1, lname + ".proj");
}

// ---- YOLOv10 (yolov10/src/block.cpp).  Its convBnSiLU takes a group count; with g = channels that is DWConv above.

// C2F (yolov10/src/block.cpp:122-150): cv1 to 2c_, split in halves, n 3x3 + 3x3 bottlenecks (e = 1) on the second half, every result
// appended to the running concat, cv2.  YOLOv8's C2F (host/yolov8.cpp) is this graph on implicit-batch Dims3 slices, so it is not shared.
inline ITensor* C2F(Ctx& c, ITensor& in, int c2, int n, bool shortcut, float e, const std::string& lname) {
    const int c_ = (int)((float)c2 * e);
    ITensor* cv1 = convBnSiLU(c, in, 2 * c_, 1, 1, lname + ".cv1");
    const Dims d = cv1->getDimensions();
    const Dims4 half{d.d[0], d.d[1] / 2, d.d[2], d.d[3]}, unit{1, 1, 1, 1};
    ITensor* s1 = c.net->addSlice(*cv1, Dims4{0, 0, 0, 0}, half, unit)->getOutput(0);
    ITensor* s2 = c.net->addSlice(*cv1, Dims4{0, d.d[1] / 2, 0, 0}, half, unit)->getOutput(0);
    ITensor* cat = cat2(c, s1, s2);
    ITensor* y = s2;
    for (int i = 0; i < n; ++i) {
        y = bottleneck(c, *y, c_, c_, shortcut, 1.0f, lname + ".m." + std::to_string(i));
        cat = cat2(c, cat, y);
    }
    return convBnSiLU(c, *cat, c2, 1, 1, lname + ".cv2");
}

// SCDown (yolov10/src/block.cpp:279-295): 1x1 + SiLU, then depthwise k x k stride s + BN with no activation
inline ITensor* SCDown(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname) {
    ITensor* a = convBnSiLU(c, in, ch, 1, 1, lname + ".cv1");
    return convBn(c, *a, ch, k, s, lname + ".cv2", ch);
}

// PSA (yolov10/src/block.cpp:360-386): cv1 to 2c, split (a, b), b += attn(b), b += ffn(b), cv2(cat(a, b))
inline ITensor* PSA(Ctx& c, ITensor& in, int ch, const std::string& lname) {
    const int h = (int)(ch * 0.5);
    ITensor* cv1 = convBnSiLU(c, in, 2 * h, 1, 1, lname + ".cv1");
    const Dims d = cv1->getDimensions();
    const Dims4 half{d.d[0], h, d.d[2], d.d[3]}, unit{1, 1, 1, 1};
    ITensor* a = c.net->addSlice(*cv1, Dims4{0, 0, 0, 0}, half, unit)->getOutput(0);
    ITensor* b = c.net->addSlice(*cv1, Dims4{0, h, 0, 0}, half, unit)->getOutput(0);
    ITensor* attn = Attention(c, *b, h, h / 64, 0.5f, lname + ".attn");
    ITensor* x = c.net->addElementWise(*b, *attn, ElementWiseOperation::kSUM)->getOutput(0);
    ITensor* f0 = convBnSiLU(c, *x, 2 * h, 1, 1, lname + ".ffn.0");
    ITensor* f1 = convBn(c, *f0, h, 1, 1, lname + ".ffn.1");
    ITensor* y = c.net->addElementWise(*x, *f1, ElementWiseOperation::kSUM)->getOutput(0);
    return convBnSiLU(c, *cat2(c, a, y), ch, 1, 1, lname + ".cv2");
}

// RepVGGDW (yolov10/src/block.cpp:388-403): SiLU(dw7x7+BN(x) + dw3x3+BN(x))
inline ITensor* RepVGGDW(Ctx& c, ITensor& in, int ch, const std::string& lname) {
    ITensor* a = convBn(c, in, ch, 7, 1, lname + ".conv", ch);
    ITensor* b = convBn(c, in, ch, 3, 1, lname + ".conv1", ch);
    return silu(c, c.net->addElementWise(*a, *b, ElementWiseOperation::kSUM)->getOutput(0));
}

// CIB (yolov10/src/block.cpp:405-431): dw3x3, 1x1 to 2c_, dw3x3 or RepVGGDW (lk), 1x1 to c2, dw3x3, all with SiLU; + shortcut
inline ITensor* CIB(Ctx& c, ITensor& in, int c1, int c2, bool shortcut, float e, bool lk, const std::string& lname) {
    const int c_ = (int)((float)c2 * e);
    ITensor* x = DWConv(c, in, c1, 3, 1, lname + ".cv1.0");
    x = convBnSiLU(c, *x, 2 * c_, 1, 1, lname + ".cv1.1");
    x = lk ? RepVGGDW(c, *x, 2 * c_, lname + ".cv1.2") : DWConv(c, *x, 2 * c_, 3, 1, lname + ".cv1.2");
    x = convBnSiLU(c, *x, c2, 1, 1, lname + ".cv1.3");
    x = DWConv(c, *x, c2, 3, 1, lname + ".cv1.4");
    if (shortcut && c1 == c2) return c.net->addElementWise(in, *x, ElementWiseOperation::kSUM)->getOutput(0);
    return x;
}

// C2fCIB (yolov10/src/block.cpp:433-461): C2F with CIB blocks (e = 1) in place of the bottlenecks
inline ITensor* C2fCIB(Ctx& c, ITensor& in, int c2, int n, bool shortcut, bool lk, float e, const std::string& lname) {
    const int c_ = (int)((float)c2 * e);
    ITensor* cv1 = convBnSiLU(c, in, 2 * c_, 1, 1, lname + ".cv1");
    const Dims d = cv1->getDimensions();
    const Dims4 half{d.d[0], d.d[1] / 2, d.d[2], d.d[3]}, unit{1, 1, 1, 1};
    ITensor* s1 = c.net->addSlice(*cv1, Dims4{0, 0, 0, 0}, half, unit)->getOutput(0);
    ITensor* s2 = c.net->addSlice(*cv1, Dims4{0, d.d[1] / 2, 0, 0}, half, unit)->getOutput(0);
    ITensor* cat = cat2(c, s1, s2);
    ITensor* y = s2;
    for (int i = 0; i < n; ++i) {
        y = CIB(c, *y, c_, c_, shortcut, 1.0f, lk, lname + ".m." + std::to_string(i));
        cat = cat2(c, cat, y);
    }
    return convBnSiLU(c, *cat, c2, 1, 1, lname + ".cv2");
}

// (B, 64, g) -> (B, 4, 16, g) -> transpose (B, 16, 4, g) -> softmax over the 16 bins -> 1x1 conv with weights arange(16) -> (B, 4, g)
// (block.cpp:140-160)
inline ITensor* DFL(Ctx& c, ITensor& in, int B, int grid, const std::string& wkey) {
    auto* sh1 = c.net->addShuffle(in);
    sh1->setReshapeDimensions(Dims4{B, 4, 16, grid});
    sh1->setSecondTranspose(Permutation{0, 2, 1, 3});
    auto* sm = c.net->addSoftMax(*sh1->getOutput(0));
    sm->setAxes(1 << 1);
    auto* conv = c.net->addConvolutionNd(*sm->getOutput(0), 1, DimsHW{1, 1}, need(c.wm, wkey), noWeights());
    conv->setStrideNd(DimsHW{1, 1});
    conv->setPaddingNd(DimsHW{0, 0});
    auto* sh2 = c.net->addShuffle(*conv->getOutput(0));
    sh2->setReshapeDimensions(Dims3{B, 4, grid});
    return sh2->getOutput(0);
}


// block.cpp:162-205: `info` holds the 9 netinfo fields (classes, keypoints, keypoint threshold truncated to int, width, height, max
// boxes, is_seg, is_pose, is_obb); the strides are appended here
inline IPluginV2Layer* addYoLoLayer(Ctx& c, const std::vector<ITensor*>& dets, const std::vector<int>& strides, std::vector<int> info) {
    auto* creator = getPluginRegistry()->getPluginCreator("YoloLayer_TRT", "1");
    assert(creator && "YoloLayer_TRT creator not registered");
    info.insert(info.end(), strides.begin(), strides.end());
    PluginField field("combinedInfo", info.data(), PluginFieldType::kINT32, (int32_t)info.size());
    PluginFieldCollection fc{1, &field};
    IPluginV2* plugin = creator->createPlugin("yololayer", &fc);
    assert(plugin);
    std::vector<ITensor*> ins(dets);
    auto* layer = c.net->addPluginV2(ins.data(), (int32_t)ins.size(), *plugin);
    plugin->destroy();  // the network holds its own clone
    return layer;
}

}  // namespace blocks
}  // namespace trtx_host
