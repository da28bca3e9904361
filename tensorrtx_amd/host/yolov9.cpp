// YOLOv9 (t / s / m / c) and GELAN-c detection through the network-definition API, implicit batch like the reference.  Mirrors the
// reference blocks and builders:
//   convBnSiLU / convBnNoAct / RepConvN / RepNBottleneck / RepNCSP / ELAN1 / RepNCSPELAN4        yolov9/src/block.cpp:111-142, 156-254
//   AConv / ADown / CBLinear / CBFuse / SP / SPPELAN                                             yolov9/src/block.cpp:256-353
//   DetectBbox_Conv / DetectCls_Conv / DFL / addYoLoLayer / DualDDetect / DDetect                yolov9/src/block.cpp:355-489
//   build_engine_yolov9_t / _s / _m / _c / build_engine_gelan_c                                   yolov9/src/model.cpp:25-176, 178-320, 321-555, 557-740, 1160-1286
// The five builders differ in channel tables, in the block at model.2 (ELAN1 or RepNCSPELAN4), in the downsampling block (AConv or ADown)
// and in the first "model.N" index, so they are one function over a table here (struct Spec); graph, weight keys and the order in which
// the head layers are added are the reference's.  The reference's builder is the specification also where it differs from the upstream
// PyTorch model: unconverted t / s apply the DualDDetect weights cv2 / cv3 / dfl of model.29 to the MAIN features (model.15 / 18 / 21),
// unconverted m and c apply those of model.38 to the AUXILIARY features (model.31 / 34 / 37), s builds model.21 with one RepNCSP repeat.
//
// Layers that cannot reach the output are not created.  The reference creates the auxiliary branch of unconverted t / s (model.22 - 28)
// and the main-branch tail of unconverted m and of c (model.10 - 22) and never connects them to the plugin; TensorRT drops them when it
// builds.  This lowering has no dead-layer removal, so the builder leaves them out and their .wts entries are simply not read.
// Not built: yolov9e / gelan_e, INT8, RepConvN folding.
#include <algorithm>
#include <numeric>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

// Conv (no bias, padding p, groups g) + BN (eps 1e-3)   (block.cpp:129-142), and ... + SiLU (block.cpp:111-128)
ITensor* convBnNoAct(Ctx& c, ITensor& in, int ch, int k, int s, int p, const std::string& lname, int g = 1) { return conv_p(c, in, ch, k, s, p, lname, g); }
ITensor* convBnSiLU(Ctx& c, ITensor& in, int ch, int k, int s, int p, const std::string& lname, int g = 1) { return silu(c, conv_p(c, in, ch, k, s, p, lname, g)); }

// RepConvN (block.cpp:156-170): 3x3 + BN and 1x1 + BN (padding p - k / 2 = 0) on the same input, summed, then SiLU.  The 1x1 is not
// folded into the 3x3: the graph stays the reference's.
ITensor* RepConvN(Ctx& c, ITensor& in, int c2, int s, int g, const std::string& lname) {
    ITensor* a = convBnNoAct(c, in, c2, 3, s, 1, lname + ".conv1", g);
    ITensor* b = convBnNoAct(c, in, c2, 1, s, 0, lname + ".conv2", g);
    return silu(c, sum(c, *a, *b));
}

ITensor* RepNBottleneck(Ctx& c, ITensor& in, int c1, int c2, bool shortcut, int g, float e, const std::string& lname) {  // block.cpp:172-183
    const int c_ = int(c2 * e);
    ITensor* cv1 = RepConvN(c, in, c_, 1, g, lname + ".cv1");
    ITensor* cv2 = convBnSiLU(c, *cv1, c2, 3, 1, 1, lname + ".cv2", g);
    return shortcut && c1 == c2 ? sum(c, in, *cv2) : cv2;
}

ITensor* RepNCSP(Ctx& c, ITensor& in, int c2, int n, bool shortcut, int g, float e, const std::string& lname) {  // block.cpp:185-206
    const int c_ = int(c2 * e);
    ITensor* m = convBnSiLU(c, in, c_, 1, 1, 0, lname + ".cv1");
    for (int i = 0; i < n; ++i) m = RepNBottleneck(c, *m, c_, c_, shortcut, g, 1.0f, lname + ".m." + std::to_string(i));
    ITensor* cv2 = convBnSiLU(c, in, c_, 1, 1, 0, lname + ".cv2");
    return convBnSiLU(c, *cat2(c, m, cv2), c2, 1, 1, 0, lname + ".cv3");
}

ITensor* ELAN1(Ctx& c, ITensor& in, int c2, int c3, int c4, const std::string& lname) {  // block.cpp:208-228
    ITensor *s1, *s2;
    halves(c, *convBnSiLU(c, in, c3, 1, 1, 0, lname + ".cv1"), &s1, &s2);
    ITensor* cv2 = convBnSiLU(c, *s2, c4, 3, 1, 1, lname + ".cv2");
    ITensor* cv3 = convBnSiLU(c, *cv2, c4, 3, 1, 1, lname + ".cv3");
    return convBnSiLU(c, *cat(c, {s1, s2, cv2, cv3}), c2, 1, 1, 0, lname + ".cv4");
}

ITensor* RepNCSPELAN4(Ctx& c, ITensor& in, int c2, int c3, int c4, int c5, const std::string& lname) {  // block.cpp:230-254
    ITensor *s1, *s2;
    halves(c, *convBnSiLU(c, in, c3, 1, 1, 0, lname + ".cv1"), &s1, &s2);
    ITensor* cv2 = convBnSiLU(c, *RepNCSP(c, *s2, c4, c5, true, 1, 0.5f, lname + ".cv2.0"), c4, 3, 1, 1, lname + ".cv2.1");
    ITensor* cv3 = convBnSiLU(c, *RepNCSP(c, *cv2, c4, c5, true, 1, 0.5f, lname + ".cv3.0"), c4, 3, 1, 1, lname + ".cv3.1");
    return convBnSiLU(c, *cat(c, {s1, s2, cv2, cv3}), c2, 1, 1, 0, lname + ".cv4");
}

ITensor* avgPool2(Ctx& c, ITensor& in) {  // avg-pool 2x2, stride 1, padding 0 (block.cpp:258-260, 267-269)
    auto* pool = c.net->addPoolingNd(in, PoolingType::kAVERAGE, DimsHW{2, 2});
    assert(pool);
    pool->setStrideNd(DimsHW{1, 1});
    pool->setPaddingNd(DimsHW{0, 0});
    return pool->getOutput(0);
}

ITensor* AConv(Ctx& c, ITensor& in, int c2, const std::string& lname) {  // block.cpp:256-263
    return convBnSiLU(c, *avgPool2(c, in), c2, 3, 2, 1, lname + ".cv1");
}

ITensor* ADown(Ctx& c, ITensor& in, int c2, const std::string& lname) {  // block.cpp:264-290
    const int c_ = c2 / 2;
    ITensor *s1, *s2;
    halves(c, *avgPool2(c, in), &s1, &s2);
    ITensor* cv1 = convBnSiLU(c, *s1, c_, 3, 2, 1, lname + ".cv1");
    ITensor* cv2 = convBnSiLU(c, *maxpool(c, *s2, 3, 2, 1), c_, 1, 1, 0, lname + ".cv2");
    return cat2(c, cv1, cv2);
}

// CBLinear (block.cpp:292-312): one biased 1x1 convolution to sum(c2s) channels, sliced into the c2s
std::vector<ITensor*> CBLinear(Ctx& c, ITensor& in, const std::vector<int>& c2s, const std::string& lname) {
    auto* conv = conv1x1_bias(c, in, std::accumulate(c2s.begin(), c2s.end(), 0), lname + ".conv");
    conv->setName((lname + ".conv").c_str());
    std::vector<ITensor*> out;
    int start = 0;
    for (int ch : c2s) {
        out.push_back(channels(c, *conv->getOutput(0), start, ch));
        start += ch;
    }
    return out;
}

// CBFuse (block.cpp:314-332): every input but the last is resized (nearest) by strides[i] / strides.back() (integer division) and all
// are summed onto the first, left to right
ITensor* CBFuse(Ctx& c, const std::vector<std::vector<ITensor*>>& in, const std::vector<int>& idx, const std::vector<int>& strides) {
    std::vector<ITensor*> res(in.size());
    res.back() = in.back()[0];
    for (int i = (int)in.size() - 2; i >= 0; --i) {
        auto* up = c.net->addResize(*in[i][idx[i]]);
        assert(up);
        up->setResizeMode(ResizeMode::kNEAREST);
        const float f = (float)(strides[i] / strides.back());
        const float scales[] = {1, f, f};
        up->setScales(scales, 3);
        res[i] = up->getOutput(0);
    }
    for (size_t i = 1; i < in.size(); ++i) res[0] = sum(c, *res[0], *res[i]);
    return res[0];
}

ITensor* SPPELAN(Ctx& c, ITensor& in, int c2, int c3, const std::string& lname) {  // block.cpp:334-353: three chained 5x5 stride-1 max-pools
    ITensor* x = convBnSiLU(c, in, c3, 1, 1, 0, lname + ".cv1");
    return convBnSiLU(c, *pool_chain(c, x, 5), c2, 1, 1, 0, lname + ".cv5");
}

// Conv(x, c2, 3), Conv(c2, c2, 3, g = 4), nn.Conv2d(c2, 4 * reg_max, 1, groups = 4) with bias   (block.cpp:355-366)
ITensor* DetectBbox_Conv(Ctx& c, ITensor& in, int c2, int reg_max, const std::string& lname) {
    ITensor* cv0 = convBnSiLU(c, in, c2, 3, 1, 1, lname + ".0");
    ITensor* cv1 = convBnSiLU(c, *cv0, c2, 3, 1, 1, lname + ".1", 4);
    auto* cv2 = conv1x1_bias(c, *cv1, reg_max * 4, lname + ".2");
    cv2->setName((lname + ".conv").c_str());
    cv2->setNbGroups(4);
    return cv2->getOutput(0);
}

// Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, nc, 1) with bias   (block.cpp:368-378)
ITensor* DetectCls_Conv(Ctx& c, ITensor& in, int c3, int cls, const std::string& lname) {
    ITensor* cv0 = convBnSiLU(c, in, c3, 3, 1, 1, lname + ".0");
    ITensor* cv1 = convBnSiLU(c, *cv0, c3, 3, 1, 1, lname + ".1");
    auto* cv2 = conv1x1_bias(c, *cv1, cls, lname + ".2");
    cv2->setName((lname + ".conv").c_str());
    return cv2->getOutput(0);
}

// DualDDetect (block.cpp:424-455) and DDetect (:457-489): the same body but for c3 = max(ch0, min(2 nc, 128)) against max(ch0, min(nc, 128)).
// All three levels' convolution arms first, then the three DFL tails, as there.  Returns the concats (4 + nc, grid).
std::vector<ITensor*> detect(Ctx& c, const std::vector<ITensor*>& feats, int cls, int ch0, bool dual, const std::string& lname) {
    const int c2 = std::max(ch0 / 4, 16 * 4);
    const int c3 = std::max(ch0, std::min(dual ? cls * 2 : cls, 128));
    std::vector<ITensor*> boxes, clss, ret;
    for (size_t i = 0; i < feats.size(); ++i) {
        boxes.push_back(DetectBbox_Conv(c, *feats[i], c2, 16, lname + ".cv2." + std::to_string(i)));
        ITensor* k = DetectCls_Conv(c, *feats[i], c3, cls, lname + ".cv3." + std::to_string(i));
        const Dims d = k->getDimensions();
        auto* sh = c.net->addShuffle(*k);
        sh->setReshapeDimensions(Dims2{cls, d.d[1] * d.d[2]});
        clss.push_back(sh->getOutput(0));
    }
    for (size_t i = 0; i < feats.size(); ++i) {   // DFL (block.cpp:380-399): blocks::DFL on the (64, gh, gw) arm
        const Dims d = boxes[i]->getDimensions();
        ret.push_back(cat2(c, DFL(c, *boxes[i], 0, d.d[1] * d.d[2], lname + ".dfl.conv.weight"), clss[i]));
    }
    return ret;
}

// block.cpp:401-422: one field "netinfo" = {classes, W, H, maxOut, isSeg} under the field type kFLOAT32, as the reference does
IPluginV2Layer* addYoLoLayer(Ctx& c, const std::vector<ITensor*>& dets, const Yolov9Config& cfg) {
    int netinfo[5] = {cfg.num_class, cfg.input_w, cfg.input_h, cfg.max_out_bbox, 0};
    PluginField field("netinfo", netinfo, PluginFieldType::kFLOAT32, 5);
    PluginFieldCollection fc{1, &field};
    return plugin_layer(c, "YoloLayer_TRT", "yololayer", &fc, dets);
}

struct Rep {   // RepNCSPELAN4's c2, c3, c4 and the RepNCSP repeat count (ELAN1: c2, c3, c4)
    int c2, c3, c4, n;
};
// One row per model: the arguments the reference's builders pass, in the order of the main branch.  "L<k>" is the layer the yaml numbers
// k + 1 and the weights name model.<k + first>.
struct Spec {
    int first;          // index of the stem in the .wts: 1 where the checkpoint keeps its leading Silence layer (unconverted m, c), else 0
    int stem0, stem1;   // L0, L1
    bool elan1;         // L2 is ELAN1 (t / s), else RepNCSPELAN4
    Rep b2;             // L2
    bool adown;         // the downsampling block is ADown (c / gelan-c), else AConv
    int d3;  Rep r4;    // L3, L4
    int d5;  Rep r6;
    int d7;  Rep r8;
    int spp_c2, spp_c3; // L9
    Rep r12, r15;
    int d16; Rep r18;
    int d19; Rep r21;
    bool aux;           // the head reads the auxiliary branch (model.23 - 37) and is model.38
};

const Spec* spec_of(const std::string& name, bool converted) {
    // model.cpp:35-109 (t), 188-254 (s), 334-435 (m), 568-645 (c), 1171-1248 (gelan-c)
    static const Spec t{0, 16, 32, true, {32, 32, 16, 0}, false, 64, {64, 64, 32, 3}, 96, {96, 96, 48, 3}, 128, {128, 128, 64, 3}, 128, 64,
                        {96, 96, 48, 3}, {64, 64, 32, 3}, 48, {96, 96, 48, 3}, 64, {128, 128, 64, 3}, false};
    static const Spec s{0, 32, 64, true, {64, 64, 32, 0}, false, 128, {128, 128, 64, 3}, 192, {192, 192, 96, 3}, 256, {256, 256, 128, 3}, 256, 128,
                        {192, 192, 96, 3}, {128, 128, 64, 3}, 96, {192, 192, 96, 3}, 128, {256, 256, 128, 1}, false};
    static const Spec m1{1, 32, 64, false, {128, 128, 64, 1}, false, 240, {240, 240, 120, 1}, 360, {360, 360, 180, 1}, 480, {480, 480, 240, 1}, 480, 240,
                         {360, 360, 180, 1}, {240, 240, 120, 1}, 184, {360, 360, 180, 1}, 240, {480, 480, 240, 1}, true};
    static const Spec m0 = [] { Spec v = m1; v.first = 0; v.aux = false; return v; }();
    static const Spec cc{1, 64, 128, false, {256, 128, 64, 1}, true, 256, {512, 256, 128, 1}, 512, {512, 512, 256, 1}, 512, {512, 512, 256, 1}, 512, 256,
                         {512, 512, 256, 1}, {256, 256, 128, 1}, 256, {512, 512, 256, 1}, 512, {512, 512, 256, 1}, true};
    static const Spec gc = [] { Spec v = cc; v.first = 0; v.aux = false; return v; }();
    if (name == "yolov9t") return &t;
    if (name == "yolov9s") return &s;
    if (name == "yolov9m") return converted ? &m0 : &m1;
    if (name == "yolov9c") return converted ? nullptr : &cc;
    if (name == "gelanc") return converted ? nullptr : &gc;
    return nullptr;
}

}  // namespace

bool yolov9_model_valid(const std::string& name, bool converted) { return spec_of(name, converted) != nullptr; }

IHostMemory* buildEngineYolov9(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolov9Config& cfg) {
    const Spec* sp = spec_of(cfg.model, cfg.converted);
    if (!sp) return nullptr;
    Session s(builder, wts);
    Ctx& c = s.c;
    auto M = [&](int k) { return "model." + std::to_string(k + sp->first); };
    auto rep = [&](ITensor* x, const Rep& r, const std::string& lname) { return RepNCSPELAN4(c, *x, r.c2, r.c3, r.c4, r.n, lname); };
    auto down = [&](ITensor* x, int c2, const std::string& lname) { return sp->adown ? ADown(c, *x, c2, lname) : AConv(c, *x, c2, lname); };
    auto block2 = [&](ITensor* x, const std::string& lname) {
        return sp->elan1 ? ELAN1(c, *x, sp->b2.c2, sp->b2.c3, sp->b2.c4, lname) : rep(x, sp->b2, lname);
    };
    auto upcat = [&](ITensor* x, ITensor* lateral) { return cat2(c, upsample2x(c, *x), lateral); };   // nn.Upsample(None, 2, 'nearest') and Concat (model.cpp:64-70)

    ITensor* data = s.input("images", cfg.input_h, cfg.input_w);   // kInputTensorName (include/config.h)
    // ---- backbone: what every model and both heads read
    ITensor* x = convBnSiLU(c, *data, sp->stem0, 3, 2, 1, M(0));
    x = convBnSiLU(c, *x, sp->stem1, 3, 2, 1, M(1));
    x = block2(x, M(2));
    ITensor* r4 = rep(down(x, sp->d3, M(3)), sp->r4, M(4));
    ITensor* r6 = rep(down(r4, sp->d5, M(5)), sp->r6, M(6));
    ITensor* r8 = rep(down(r6, sp->d7, M(7)), sp->r8, M(8));

    std::vector<ITensor*> feats;
    std::string head_name;
    bool dual;
    if (!sp->aux) {
        // ---- main-branch neck (model.cpp:60-109): SPPELAN, two up-concat merges, two down-concat merges
        ITensor* spp = SPPELAN(c, *r8, sp->spp_c2, sp->spp_c3, M(9));
        ITensor* r12 = rep(upcat(spp, r6), sp->r12, M(12));
        ITensor* r15 = rep(upcat(r12, r4), sp->r15, M(15));
        ITensor* r18 = rep(cat2(c, down(r15, sp->d16, M(16)), r12), sp->r18, M(18));
        ITensor* r21 = rep(cat2(c, down(r18, sp->d19, M(19)), spp), sp->r21, M(21));
        feats = {r15, r18, r21};
        // t / s keep the auxiliary branch in the checkpoint (model.22 - 28) until it is converted: DualDDetect is model.29 then
        // (model.cpp:139-143, 283-287); converted t / s / m and gelan-c: DDetect, model.22 (:142, :521, :1253)
        dual = sp->elan1 && !cfg.converted;
        head_name = dual ? "model.29" : "model.22";
    } else {
        // ---- multi-level reversible auxiliary branch (model.cpp:441-509, 651-701), fed by the backbone through CBLinear / CBFuse
        const std::vector<ITensor*> cb23 = CBLinear(c, *r4, {sp->d3}, M(22));
        const std::vector<ITensor*> cb24 = CBLinear(c, *r6, {sp->d3, sp->d5}, M(23));
        const std::vector<ITensor*> cb25 = CBLinear(c, *r8, {sp->d3, sp->d5, sp->d7}, M(24));
        ITensor* a = convBnSiLU(c, *data, sp->stem0, 3, 2, 1, M(25));
        a = convBnSiLU(c, *a, sp->stem1, 3, 2, 1, M(26));
        a = rep(a, sp->b2, M(27));
        ITensor* d29 = down(a, sp->d3, M(28));
        ITensor* r31 = rep(CBFuse(c, {cb23, cb24, cb25, {d29}}, {0, 0, 0, 0}, {8, 16, 32, 8}), sp->r4, M(30));
        ITensor* d32 = down(r31, sp->d5, M(31));
        ITensor* r34 = rep(CBFuse(c, {cb24, cb25, {d32}}, {1, 1, 0}, {16, 32, 16}), sp->r6, M(33));
        ITensor* d35 = down(r34, sp->d7, M(34));
        ITensor* r37 = rep(CBFuse(c, {cb25, {d35}}, {2, 0}, {32, 32}), sp->r8, M(36));
        feats = {r31, r34, r37};
        dual = true;
        head_name = M(37);   // model.38 (model.cpp:515-516, 706-708)
    }
    const int ch0 = (int)feats[0]->getDimensions().d[0];   // ch[0] of the reference's calls: the stride-8 feature's channels
    std::vector<ITensor*> dets = detect(c, feats, cfg.num_class, ch0, dual, head_name);
    if (cfg.mark_heads) s.mark_heads(dets);
    IPluginV2Layer* yolo = addYoLoLayer(c, dets, cfg);
    if (!yolo) return nullptr;
    s.output(yolo->getOutput(0), "output");   // kOutputTensorName
    return s.finish(builder, config, cfg.max_batch, cfg.fp16);
}

}  // namespace trtx_host
