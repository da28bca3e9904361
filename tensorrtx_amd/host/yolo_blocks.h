// The block library of the YOLO host builders, written against the network-definition API.  The reference restates these blocks in every
// model directory (yolov8, yolo11, yolov12, yolov10, yolov5, yolov9, yolov7: src/block.cpp and model.cpp); here each exists once:
//   - the primitives: one Conv + BN (conv_bn; the activation is the caller's: silu, leaky), channel slices, upsample, max-pool, pool
//     chain, concat, DFL, plugin_layer.  They read the rank of the tensor they are given, so implicit-batch (C, H, W) and explicit-batch
//     (B, C, H, W) builders share them, and they emit Dims of exactly that rank;
//   - the ultralytics blocks on top of them (bottleneck, C3k, C3K2, C2F, SPPF, Attention, SCDown, PSA, RepVGGDW, CIB, C2fCIB);
//   - the v8-style detect head and tail (detect_v8: YOLOv8, YOLO11, YOLOv12, YOLOv10) and the two YoloLayer_TRT field sets that more
//     than one family uses ("combinedInfo", and "netinfo" + "kernels" of the anchor models).
// What only one family has stays in its file.  Line numbers in the comments are yolo11's unless they name another directory.
#pragma once
#include <cassert>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "build.h"

namespace trtx_host {
namespace blocks {
using namespace nvinfer1;

// ---- channel arithmetic.  The three widths differ on purpose; the depth is the same everywhere.
inline int get_width_v8(int x, float gw, int max_channels, int divisor = 8) {  // yolov8/src/model.cpp:13-16: scales, then caps
    const int ch = int(ceil((x * gw) / divisor)) * divisor;
    return ch >= max_channels ? max_channels : ch;
}
inline int get_width(int x, float gw, int max_channels, int divisor = 8) {  // model.cpp:9-13 (YOLO11, 12, 10): caps, then scales
    const int ch = std::min(x, max_channels);
    return int(ceil((ch * gw) / divisor)) * divisor;
}
inline int get_width_v5(int x, float gw, int divisor = 8) { return int(ceil((x * gw) / divisor)) * divisor; }   // yolov5/src/model.cpp:53-55: no cap

// model.cpp:15-22.  The reference rounds half away from zero and then takes one off when the fraction is exactly 0.5 and the integer
// part is even: round-half-to-even, Python's round() that the yaml depths went through.
inline int get_depth(int x, float gd) {
    if (x == 1) return 1;
    int r = (int)round(x * gd);
    if (x * gd - int(x * gd) == 0.5 && (int(x * gd) % 2) == 0) --r;
    return std::max<int>(r, 1);
}

// ---- primitives
inline int rank_of(ITensor& t) { return t.getDimensions().nbDims; }
inline int channels_of(ITensor& t) { return (int)t.getDimensions().d[rank_of(t) - 3]; }
inline Dims dims_of(int rank, int64_t v) {
    Dims d;
    d.nbDims = rank;
    for (int i = 0; i < rank; ++i) d.d[i] = v;
    return d;
}

// Conv (k x k, stride s, padding p, groups g, optional bias) + BN folded with `eps`.  The convolution reads <conv>.weight / .bias, the
// BN <bn>.*; `named` gives the convolution layer the name <conv>, as the reference does in some models.
inline ITensor* conv_bn(Ctx& c, ITensor& in, int ch, int k, int s, int p, const std::string& conv, const std::string& bn, int g = 1,
                        bool bias = false, float eps = 1e-3f, bool named = false) {
    auto* l = c.net->addConvolutionNd(in, ch, DimsHW{k, k}, need(c.wm, conv + ".weight"), bias ? need(c.wm, conv + ".bias") : noWeights());
    assert(l);
    if (named) l->setName(conv.c_str());
    l->setStrideNd(DimsHW{s, s});
    l->setPaddingNd(DimsHW{p, p});
    if (g != 1) l->setNbGroups(g);
    return addBatchNorm2d(c.net, c.wm, *l->getOutput(0), bn, eps)->getOutput(0);
}
// the ultralytics spelling: <lname>.conv and <lname>.bn, BN eps 1e-3
inline ITensor* conv_p(Ctx& c, ITensor& in, int ch, int k, int s, int p, const std::string& lname, int g = 1, bool bias = false) {
    return conv_bn(c, in, ch, k, s, p, lname + ".conv", lname + ".bn", g, bias);
}
// ... with 'same' padding k/2 (block.cpp:73-92 without the SiLU; convBn :271-285).  `bias`: YOLOv12's convBn carries <lname>.conv.bias
// for names that hold ".pe" (yolov12/src/block.cpp:282-296)
inline ITensor* convBn(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname, int g = 1, bool bias = false) {
    return conv_p(c, in, ch, k, s, k / 2, lname, g, bias);
}
// the biased 1x1 convolution that ends a detect arm
inline IConvolutionLayer* conv1x1_bias(Ctx& c, ITensor& in, int ch, const std::string& lname) {
    auto* l = c.net->addConvolutionNd(in, ch, DimsHW{1, 1}, need(c.wm, lname + ".weight"), need(c.wm, lname + ".bias"));
    assert(l);
    l->setStrideNd(DimsHW{1, 1});
    l->setPaddingNd(DimsHW{0, 0});
    return l;
}

// SiLU spelled Sigmoid * x (block.cpp:88-91)
inline ITensor* silu(Ctx& c, ITensor* x) {
    ITensor* sig = c.net->addActivation(*x, ActivationType::kSIGMOID)->getOutput(0);
    return c.net->addElementWise(*x, *sig, ElementWiseOperation::kPROD)->getOutput(0);
}
inline ITensor* leaky(Ctx& c, ITensor* x) {   // LeakyReLU(0.1)
    auto* act = c.net->addActivation(*x, ActivationType::kLEAKY_RELU);
    assert(act);
    act->setAlpha(0.1f);
    return act->getOutput(0);
}
inline ITensor* sum(Ctx& c, ITensor& a, ITensor& b) { return c.net->addElementWise(a, b, ElementWiseOperation::kSUM)->getOutput(0); }

inline ITensor* convBnSiLU(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname, int g = 1) { return silu(c, convBn(c, in, ch, k, s, lname, g)); }
// DWConv: depthwise conv (groups = ch) + BN + SiLU (block.cpp:417-437)
inline ITensor* DWConv(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname) { return convBnSiLU(c, in, ch, k, s, lname, ch); }

// `len` channels from `start`, every other axis whole
inline ITensor* channels(Ctx& c, ITensor& in, int start, int len) {
    Dims size = in.getDimensions();
    const int rank = size.nbDims;
    Dims at = dims_of(rank, 0);
    at.d[rank - 3] = start;
    size.d[rank - 3] = len;
    return c.net->addSlice(in, at, size, dims_of(rank, 1))->getOutput(0);
}
// chunk(2) along the channels
inline void halves(Ctx& c, ITensor& in, ITensor** lo, ITensor** hi) {
    const int h = channels_of(in) / 2;
    *lo = channels(c, in, 0, h);
    *hi = channels(c, in, h, h);
}

inline ITensor* cat(Ctx& c, const std::vector<ITensor*>& v, int axis = -1) {   // axis -1: the layer's default, the channels
    auto* l = c.net->addConcatenation(v.data(), (int32_t)v.size());
    assert(l);
    if (axis >= 0) l->setAxis(axis);
    return l->getOutput(0);
}
inline ITensor* cat2(Ctx& c, ITensor* a, ITensor* b) { return cat(c, {a, b}); }

inline ITensor* upsample2x(Ctx& c, ITensor& in) {  // nn.Upsample(None, 2, 'nearest') (model.cpp:205-209)
    const int rank = rank_of(in);
    float scale[Dims::MAX_DIMS];
    for (int i = 0; i < rank; ++i) scale[i] = i < rank - 2 ? 1.0f : 2.0f;
    auto* r = c.net->addResize(in);
    assert(r);
    r->setResizeMode(ResizeMode::kNEAREST);
    r->setScales(scale, rank);
    return r->getOutput(0);
}

inline ITensor* maxpool(Ctx& c, ITensor& in, int k, int s, int p) {
    auto* m = c.net->addPoolingNd(in, PoolingType::kMAX, DimsHW{k, k});
    assert(m);
    m->setStrideNd(DimsHW{s, s});
    m->setPaddingNd(DimsHW{p, p});
    return m->getOutput(0);
}
// x and three chained k x k stride-1 max-pools of it, joined: the middle of SPPF and SPPELAN
inline ITensor* pool_chain(Ctx& c, ITensor* x, int k) {
    std::vector<ITensor*> parts{x};
    for (int i = 0; i < 3; ++i) parts.push_back(maxpool(c, *parts.back(), k, 1, k / 2));
    return cat(c, parts);
}

// Distribution-focal-loss decode (block.cpp:140-160; yolov8/src/block.cpp:239-257; yolov9/src/block.cpp:380-399): 64 box channels over
// `grid` cells -> (4, 16, grid) -> transpose (16, 4, grid) -> softmax over the 16 bins -> 1x1 conv with weights arange(16) -> (4, grid).
// B > 0: explicit batch, every shape has B in front and the softmax names its axis; B == 0: implicit batch, the softmax's default axis.
inline ITensor* DFL(Ctx& c, ITensor& in, int B, int grid, const std::string& wkey) {
    auto* sh1 = c.net->addShuffle(in);
    sh1->setReshapeDimensions(B ? Dims(Dims4{B, 4, 16, grid}) : Dims(Dims3{4, 16, grid}));
    sh1->setSecondTranspose(B ? Permutation{0, 2, 1, 3} : Permutation{1, 0, 2});
    auto* sm = c.net->addSoftMax(*sh1->getOutput(0));
    if (B) sm->setAxes(1 << 1);
    auto* conv = c.net->addConvolutionNd(*sm->getOutput(0), 1, DimsHW{1, 1}, need(c.wm, wkey), noWeights());
    assert(conv);
    conv->setStrideNd(DimsHW{1, 1});
    conv->setPaddingNd(DimsHW{0, 0});
    auto* sh2 = c.net->addShuffle(*conv->getOutput(0));
    sh2->setReshapeDimensions(B ? Dims(Dims3{B, 4, grid}) : Dims(Dims2{4, grid}));
    return sh2->getOutput(0);
}

// The one place a plugin enters a network: the registry's creator `creator_name` / "1" makes the plugin from `fc` (null: the creator's own,
// empty, field collection, which is how Darknet's YoloLayer_TRT and Mish_TRT are created), the network clones it.  Null where the creator
// refuses the fields.
inline IPluginV2Layer* plugin_layer(Ctx& c, const char* creator_name, const std::string& layer_name, const PluginFieldCollection* fc,
                                    const std::vector<ITensor*>& inputs) {
    auto* creator = getPluginRegistry()->getPluginCreator(creator_name, "1");
    assert(creator && "plugin creator not registered");
    IPluginV2* plugin = creator->createPlugin(layer_name.c_str(), fc ? fc : creator->getFieldNames());
    if (!plugin) return nullptr;
    std::vector<ITensor*> ins(inputs);
    auto* layer = c.net->addPluginV2(ins.data(), (int32_t)ins.size(), *plugin);
    plugin->destroy();  // the network holds its own clone
    return layer;
}

// ---- ultralytics blocks
inline ITensor* bottleneck(Ctx& c, ITensor& in, int c1, int c2, bool shortcut, float e, const std::string& lname) {  // block.cpp:94-109 (k 3x3, 3x3)
    const int c_ = (int)((float)c2 * e);
    ITensor* a = convBnSiLU(c, in, c_, 3, 1, lname + ".cv1");
    ITensor* b = convBnSiLU(c, *a, c2, 3, 1, lname + ".cv2");
    return shortcut && c1 == c2 ? sum(c, in, *b) : b;
}

inline ITensor* C3k(Ctx& c, ITensor& in, int c2, int n, bool shortcut, float e, const std::string& lname) {  // block.cpp:207-224
    const int c_ = (int)((float)c2 * e);
    ITensor* y = convBnSiLU(c, in, c_, 1, 1, lname + ".cv1");
    ITensor* b = convBnSiLU(c, in, c_, 1, 1, lname + ".cv2");
    for (int i = 0; i < n; ++i) y = bottleneck(c, *y, c_, c_, shortcut, 1.0f, lname + ".m." + std::to_string(i));
    return convBnSiLU(c, *cat2(c, y, b), c2, 1, 1, lname + ".cv3");
}

// The C2f frame (C3K2 block.cpp:226-262; C2F yolov8/src/block.cpp:126-155, yolov10/src/block.cpp:122-150; C2fCIB yolov10/src/block.cpp:433-461):
// cv1 to 2c_, split in halves along the channels, n blocks `m(y, c_, name)` chained on the second half, every result appended to the
// running concat, cv2
template <class Block>
inline ITensor* c2f_frame(Ctx& c, ITensor& in, int c2, int n, float e, const std::string& lname, Block m) {
    const int c_ = (int)((float)c2 * e);
    ITensor *s1, *y;
    halves(c, *convBnSiLU(c, in, 2 * c_, 1, 1, lname + ".cv1"), &s1, &y);
    ITensor* all = cat2(c, s1, y);
    for (int i = 0; i < n; ++i) {
        y = m(y, c_, lname + ".m." + std::to_string(i));
        all = cat2(c, all, y);
    }
    return convBnSiLU(c, *all, c2, 1, 1, lname + ".cv2");
}
inline ITensor* C3K2(Ctx& c, ITensor& in, int c2, int n, bool c3k, bool shortcut, float e, const std::string& lname) {
    return c2f_frame(c, in, c2, n, e, lname, [&](ITensor* y, int c_, const std::string& m) {
        return c3k ? C3k(c, *y, c_, 2, shortcut, 0.5f, m) : bottleneck(c, *y, c_, c_, shortcut, 0.5f, m);
    });
}
inline ITensor* C2F(Ctx& c, ITensor& in, int c2, int n, bool shortcut, float e, const std::string& lname) {   // 3x3 + 3x3 bottlenecks, e = 1
    return c2f_frame(c, in, c2, n, e, lname, [&](ITensor* y, int c_, const std::string& m) { return bottleneck(c, *y, c_, c_, shortcut, 1.0f, m); });
}

inline ITensor* SPPF(Ctx& c, ITensor& in, int c1, int c2, int k, const std::string& lname) {  // block.cpp:111-138; yolov8/src/block.cpp:214-237; yolov10/src/block.cpp:190-212
    ITensor* x = convBnSiLU(c, in, c1 / 2, 1, 1, lname + ".cv1");
    return convBnSiLU(c, *pool_chain(c, x, k), c2, 1, 1, lname + ".cv2");
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
    return convBn(c, *sum(c, *re->getOutput(0), *pe), dim, 1, 1, lname + ".proj");
}

// ---- YOLOv10 (yolov10/src/block.cpp).  Its convBnSiLU takes a group count; with g = channels that is DWConv above.

// SCDown (yolov10/src/block.cpp:279-295): 1x1 + SiLU, then depthwise k x k stride s + BN with no activation
inline ITensor* SCDown(Ctx& c, ITensor& in, int ch, int k, int s, const std::string& lname) {
    ITensor* a = convBnSiLU(c, in, ch, 1, 1, lname + ".cv1");
    return convBn(c, *a, ch, k, s, lname + ".cv2", ch);
}

// PSA (yolov10/src/block.cpp:360-386): cv1 to 2c, split (a, b), b += attn(b), b += ffn(b), cv2(cat(a, b))
inline ITensor* PSA(Ctx& c, ITensor& in, int ch, const std::string& lname) {
    const int h = (int)(ch * 0.5);
    ITensor *a, *b;
    halves(c, *convBnSiLU(c, in, 2 * h, 1, 1, lname + ".cv1"), &a, &b);
    ITensor* attn = Attention(c, *b, h, h / 64, 0.5f, lname + ".attn");
    ITensor* x = sum(c, *b, *attn);
    ITensor* f0 = convBnSiLU(c, *x, 2 * h, 1, 1, lname + ".ffn.0");
    ITensor* f1 = convBn(c, *f0, h, 1, 1, lname + ".ffn.1");
    ITensor* y = sum(c, *x, *f1);
    return convBnSiLU(c, *cat2(c, a, y), ch, 1, 1, lname + ".cv2");
}

// RepVGGDW (yolov10/src/block.cpp:388-403): SiLU(dw7x7+BN(x) + dw3x3+BN(x))
inline ITensor* RepVGGDW(Ctx& c, ITensor& in, int ch, const std::string& lname) {
    ITensor* a = convBn(c, in, ch, 7, 1, lname + ".conv", ch);
    ITensor* b = convBn(c, in, ch, 3, 1, lname + ".conv1", ch);
    return silu(c, sum(c, *a, *b));
}

// CIB (yolov10/src/block.cpp:405-431): dw3x3, 1x1 to 2c_, dw3x3 or RepVGGDW (lk), 1x1 to c2, dw3x3, all with SiLU; + shortcut
inline ITensor* CIB(Ctx& c, ITensor& in, int c1, int c2, bool shortcut, float e, bool lk, const std::string& lname) {
    const int c_ = (int)((float)c2 * e);
    ITensor* x = DWConv(c, in, c1, 3, 1, lname + ".cv1.0");
    x = convBnSiLU(c, *x, 2 * c_, 1, 1, lname + ".cv1.1");
    x = lk ? RepVGGDW(c, *x, 2 * c_, lname + ".cv1.2") : DWConv(c, *x, 2 * c_, 3, 1, lname + ".cv1.2");
    x = convBnSiLU(c, *x, c2, 1, 1, lname + ".cv1.3");
    x = DWConv(c, *x, c2, 3, 1, lname + ".cv1.4");
    return shortcut && c1 == c2 ? sum(c, in, *x) : x;
}

// C2fCIB (yolov10/src/block.cpp:433-461): C2F with CIB blocks (e = 1) in place of the bottlenecks
inline ITensor* C2fCIB(Ctx& c, ITensor& in, int c2, int n, bool shortcut, bool lk, float e, const std::string& lname) {
    return c2f_frame(c, in, c2, n, e, lname, [&](ITensor* y, int c_, const std::string& m) { return CIB(c, *y, c_, c_, shortcut, 1.0f, lk, m); });
}

// ---- the v8-style detect head and tail (yolov8/src/model.cpp:188-303; yolo11 model.cpp:259-390; yolov12 :141-290; yolov10 :113-252)
struct DetectV8 {
    std::string arms;        // weight-key prefix of the arms: <arms>cv2.<lv>, <arms>cv3.<lv>, <arms>cv4.<lv> ("model.22.", "model.23.one2one_")
    std::string dfl;         // the DFL convolution's weight key
    bool dw_cls;             // class arm: DWConv, 1x1, DWConv, 1x1 (YOLO11 on), else 3x3, 3x3 (YOLOv8)
    int c2, c3;              // widths of the box arm and of the class arm
    int nc, B;               // classes; batch of an explicit-batch network, 0 for implicit batch
    int input_h, input_w;
    int task = 0;            // 1 seg, 2 pose, 3 obb: the extra cv4 branch, two 3x3 to cv4_mid and a biased 1x1 to cv4_out, flattened
    int cv4_mid = 0, cv4_out = 0;
};

// The strides are read off the backbone maps p3, p4, p5 (calculateStrides, model.cpp:24-31)
inline std::vector<int> strides_from(int input_h, const std::vector<ITensor*>& maps) {
    std::vector<int> s;
    for (ITensor* t : maps) s.push_back(input_h / (int)t->getDimensions().d[rank_of(*t) - 2]);
    return s;
}

// Per level a box arm to 64 channels and a class arm, joined; then - after all three heads, which is the reference's layer order - per
// level: flatten the grid, split box / classes, DFL the box half, re-join.  Pose joins its cv4 branch per level right after the DFL;
// seg / obb finish all three DFL tails first.  Returns the plugin's inputs.
inline std::vector<ITensor*> detect_v8(Ctx& c, const DetectV8& h, const std::vector<ITensor*>& feats, const std::vector<int>& strides) {
    const int axis = h.B ? 1 : -1;   // explicit-batch joins name the channel axis, as the reference does
    auto flat = [&](ITensor* t, int ch, int grid) {
        auto* sh = c.net->addShuffle(*t);
        if (h.B) sh->setReshapeDimensions(Dims3{h.B, ch, grid});
        else sh->setReshapeDimensions(Dims2{ch, grid});
        return sh->getOutput(0);
    };
    auto cv4 = [&](int lv, int grid) {   // cv4_conv_combined (yolov8/src/model.cpp:54-96; yolo11 model.cpp:474-507)
        const std::string l = h.arms + "cv4." + std::to_string(lv);
        ITensor* a = convBnSiLU(c, *feats[lv], h.cv4_mid, 3, 1, l + ".0");
        ITensor* b = convBnSiLU(c, *a, h.cv4_mid, 3, 1, l + ".1");
        auto* cv = c.net->addConvolutionNd(*b, h.cv4_out, DimsHW{1, 1}, need(c.wm, l + ".2.weight"), need(c.wm, l + ".2.bias"));
        assert(cv);
        cv->setStrideNd(DimsHW{1, 1});
        return flat(cv->getOutput(0), h.cv4_out, grid);
    };
    std::vector<ITensor*> cats, dets;
    for (size_t lv = 0; lv < feats.size(); ++lv) {
        const std::string s = h.arms + "cv2." + std::to_string(lv), t = h.arms + "cv3." + std::to_string(lv);
        ITensor* b = convBnSiLU(c, *feats[lv], h.c2, 3, 1, s + ".0");
        b = convBnSiLU(c, *b, h.c2, 3, 1, s + ".1");
        ITensor* box = conv1x1_bias(c, *b, 64, s + ".2")->getOutput(0);
        ITensor* k;
        if (h.dw_cls) {
            k = DWConv(c, *feats[lv], channels_of(*feats[lv]), 3, 1, t + ".0.0");
            k = convBnSiLU(c, *k, h.c3, 1, 1, t + ".0.1");
            k = DWConv(c, *k, h.c3, 3, 1, t + ".1.0");
            k = convBnSiLU(c, *k, h.c3, 1, 1, t + ".1.1");
        } else {
            k = convBnSiLU(c, *feats[lv], h.c3, 3, 1, t + ".0");
            k = convBnSiLU(c, *k, h.c3, 3, 1, t + ".1");
        }
        ITensor* cls = conv1x1_bias(c, *k, h.nc, t + ".2")->getOutput(0);
        cats.push_back(cat2(c, box, cls));
    }
    std::vector<std::pair<ITensor*, ITensor*>> tails;
    auto grid_of = [&](size_t lv) { return (h.input_h / strides[lv]) * (h.input_w / strides[lv]); };
    for (size_t lv = 0; lv < feats.size(); ++lv) {
        const int grid = grid_of(lv);
        ITensor* f = flat(cats[lv], 64 + h.nc, grid);
        // the two slices are (64 | nc, grid) of a (64 + nc, grid) tensor: flattened, the channel axis is the second from the end
        Dims at = dims_of(rank_of(*f), 0), size = f->getDimensions();
        const Dims unit = dims_of(rank_of(*f), 1);
        const int ax = rank_of(*f) - 2;
        size.d[ax] = 64;
        ITensor* boxPart = c.net->addSlice(*f, at, size, unit)->getOutput(0);
        at.d[ax] = 64;
        size.d[ax] = h.nc;
        ITensor* clsPart = c.net->addSlice(*f, at, size, unit)->getOutput(0);
        ITensor* dfl = DFL(c, *boxPart, h.B, grid, h.dfl);
        if (h.task == 0) dets.push_back(cat(c, {dfl, clsPart}, axis));
        else if (h.task == 2) dets.push_back(cat(c, {dfl, clsPart, cv4((int)lv, grid)}, axis));
        else tails.push_back({dfl, clsPart});
    }
    for (size_t lv = 0; lv < tails.size(); ++lv) dets.push_back(cat(c, {tails[lv].first, tails[lv].second, cv4((int)lv, grid_of(lv))}, axis));
    return dets;
}

// ---- YoloLayer_TRT, the field sets more than one family writes
// block.cpp:162-205: "combinedInfo" = `info` (9 netinfo fields: classes, keypoints, keypoint threshold truncated to int, width, height, max
// boxes, is_seg, is_pose, is_obb; YOLOv10's 6-float form has 4: classes, width, height, max boxes) with the strides appended
inline IPluginV2Layer* addYoLoLayer(Ctx& c, const std::vector<ITensor*>& dets, const std::vector<int>& strides, std::vector<int> info) {
    info.insert(info.end(), strides.begin(), strides.end());
    PluginField field("combinedInfo", info.data(), PluginFieldType::kINT32, (int32_t)info.size());
    PluginFieldCollection fc{1, &field};
    return plugin_layer(c, "YoloLayer_TRT", "yololayer", &fc, dets);
}

// yolov5/src/model.cpp:234-284, yolov7/src/block.cpp:208-255: "netinfo" carries its ints under the field type kFLOAT32 and "kernels" is
// counted in YoloKernel elements (yolov5/src/types.h:5-9), as the reference does: per level the grid of `scales[i]` and the six floats
// of <lname>.anchor_grid.  Null when anchor_grid does not hold one level per detect convolution and scale.
inline IPluginV2Layer* addAnchorYoLoLayer(Ctx& c, const std::string& lname, const std::vector<ITensor*>& dets, std::vector<int> netinfo,
                                          const std::vector<int>& scales) {
    constexpr int kNumAnchor = 3;   // yolov5/src/config.h:35, yolov7/include/config.h:28
    struct YoloKernel {
        int width, height;
        float anchors[kNumAnchor * 2];
    };
    const Weights& ag = need(c.wm, lname + ".anchor_grid");
    const size_t levels = dets.size();
    if ((size_t)ag.count / (kNumAnchor * 2) != levels || scales.size() != levels) return nullptr;
    std::vector<YoloKernel> kernels(levels);
    for (size_t i = 0; i < levels; ++i) {
        if (scales[i] < 1) return nullptr;
        kernels[i].width = netinfo[1] / scales[i];    // netinfo = {classes, input_w, input_h, ...}
        kernels[i].height = netinfo[2] / scales[i];
        memcpy(kernels[i].anchors, static_cast<const float*>(ag.values) + i * kNumAnchor * 2, sizeof(kernels[i].anchors));
    }
    PluginField fields[2] = {PluginField("netinfo", netinfo.data(), PluginFieldType::kFLOAT32, (int32_t)netinfo.size()),
                             PluginField("kernels", kernels.data(), PluginFieldType::kFLOAT32, (int32_t)kernels.size())};
    PluginFieldCollection fc{2, fields};
    return plugin_layer(c, "YoloLayer_TRT", "yololayer", &fc, dets);
}

}  // namespace blocks
}  // namespace trtx_host
