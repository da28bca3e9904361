// YOLOv7 detection (tiny, v7, x, w6, e6) through the network-definition API, implicit batch like the reference.  Restates
//   convBnSilu / convBlockLeakRelu / ReOrg / DownC / SPPCSPC / RepConv / getAnchors / addYoLoLayer     yolov7/src/block.cpp:85-255
//   build_engine_yolov7_tiny / yolov7 / yolov7x / yolov7w6 / yolov7e6                                   yolov7/src/model.cpp:1775-2100, 1567-1773,
//                                                                                                        1284-1565, 1046-1282, 775-1044
// The reference writes every builder out layer by layer, one variable per row of the model's yaml; the rows repeat a handful of blocks
// (ELAN with 4 or 6 3x3 convolutions, the MP / DownC transition, the upsample-and-join of the head), so here a builder is a list of block
// calls over one list of row outputs: a row's weights are "model.<row>", and `from` arguments are row numbers (negative: relative, as
// in the yaml).  The layer sequence is the reference's: ReOrg is four slices and a concat, SPP / SPPCSPC are three parallel pooling
// layers, RepConv is two convolutions, two scales, a sum and SiLU - the lowering folds the first two (runtime/lower_match.cpp
// match_reorg_fold, runtime/plan_passes.cpp chain_spp_parallel_pools).  The detect convolutions are the plain biased 1x1 `m.i`
// convolutions: like the reference, the builder does not read the implicit `ia` / `im` tensors of the checkpoint (a checkpoint must
// have them fused in, as the reference's gen_wts does for the deploy model).  Not built: yolov7d6, yolov7e6e, INT8.
#include <cmath>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using namespace blocks;
namespace {

// One model under construction: y[i] is the output of yaml row i.
struct Rows {
    Ctx& c;
    const Yolov7Config& cfg;
    bool leaky;   // yolov7-tiny: Conv + BN (eps 1e-5) + LeakyReLU(0.1) (convBlockLeakRelu); the others Conv + BN (eps 1e-3) + SiLU (convBnSilu)
    ITensor* image;   // what row 0 reads ("from" -1 of the first row)
    std::vector<ITensor*> y;

    ITensor* at(int from) const {
        if (from >= 0) return y[from];
        return (size_t)(-from) > y.size() ? image : y[y.size() + from];
    }
    std::string name() const { return "model." + std::to_string(y.size()); }
    int push(ITensor* t) {
        y.push_back(t);
        return (int)y.size() - 1;
    }

    // block.cpp:85-104 / 192-206; the builders pass padding 1 with k = 3 and 0 with k = 1.  The convolution layer is named <lname>.conv
    ITensor* convAct(ITensor& in, int ch, int k, int s, const std::string& lname) {
        ITensor* bn = conv_bn(c, in, ch, k, s, k / 2, lname + ".conv", lname + ".bn", 1, false, leaky ? 1e-5f : 1e-3f, /*named=*/true);
        return leaky ? blocks::leaky(c, bn) : silu(c, bn);
    }
    ITensor* maxpool(ITensor& in, int k, int s, int p) { return blocks::maxpool(c, in, k, s, p); }
    ITensor* concat(const std::vector<ITensor*>& v) { return blocks::cat(c, v); }

    // ---- yaml rows
    int conv(int from, int ch, int k, int s) { return push(convAct(*at(from), ch, k, s, name())); }
    int mp(int from) { return push(maxpool(*at(from), 2, 2, 0)); }
    int cat(const std::vector<int>& from) {
        std::vector<ITensor*> v;
        for (int f : from) v.push_back(at(f));
        return push(concat(v));
    }
    int up(int from) { return push(upsample2x(c, *at(from))); }   // nn.Upsample(None, 2, 'nearest')
    int reorg(int from) {   // block.cpp:106-114
        ITensor& in = *at(from);
        const int ch = in.getDimensions().d[0], h = cfg.input_h / 2, w = cfg.input_w / 2;
        std::vector<ITensor*> v;
        for (const Dims3& start : {Dims3{0, 0, 0}, Dims3{0, 1, 0}, Dims3{0, 0, 1}, Dims3{0, 1, 1}})
            v.push_back(c.net->addSlice(in, start, Dims3{ch, h, w}, Dims3{1, 2, 2})->getOutput(0));
        return push(concat(v));
    }
    int downc(int from, int c1, int c2) {   // block.cpp:116-130
        const std::string l = name();
        ITensor& in = *at(from);
        ITensor* cv1 = convAct(in, c1, 1, 1, l + ".cv1");
        ITensor* cv2 = convAct(*cv1, c2 / 2, 3, 2, l + ".cv2");
        ITensor* cv3 = convAct(*maxpool(in, 2, 2, 0), c2 / 2, 1, 1, l + ".cv3");
        return push(concat({cv2, cv3}));
    }
    int sppcspc(int from, int c2) {   // block.cpp:132-166: c_ = int(2 * c2 * 0.5)
        const std::string l = name();
        ITensor& in = *at(from);
        ITensor* cv1 = convAct(in, c2, 1, 1, l + ".cv1");
        ITensor* cv2 = convAct(in, c2, 1, 1, l + ".cv2");
        ITensor* cv3 = convAct(*cv1, c2, 3, 1, l + ".cv3");
        ITensor* cv4 = convAct(*cv3, c2, 1, 1, l + ".cv4");
        ITensor* m1 = maxpool(*cv4, 5, 1, 2);
        ITensor* m2 = maxpool(*cv4, 9, 1, 4);
        ITensor* m3 = maxpool(*cv4, 13, 1, 6);
        ITensor* cv5 = convAct(*concat({cv4, m1, m2, m3}), c2, 1, 1, l + ".cv5");
        ITensor* cv6 = convAct(*cv5, c2, 3, 1, l + ".cv6");
        return push(convAct(*concat({cv6, cv2}), c2, 1, 1, l + ".cv7"));
    }
    int repconv(int from, int c2) {   // block.cpp:168-190, k = 3, s = 1: 3x3 + BN and 1x1 + BN summed, then SiLU; no identity branch (c1 != c2)
        const std::string l = name();
        ITensor& in = *at(from);
        ITensor* a = conv_bn(c, in, c2, 3, 1, 1, l + ".rbr_dense.0", l + ".rbr_dense.1", 1, false, 1e-3f, /*named=*/true);
        ITensor* b = conv_bn(c, in, c2, 1, 1, 0, l + ".rbr_1x1.0", l + ".rbr_1x1.1", 1, false, 1e-3f, /*named=*/true);
        return push(silu(c, sum(c, *a, *b)));
    }

    // ---- the repeating groups of rows
    // ELAN: two 1x1 convolutions of the same input, n 3x3 convolutions behind the second, the rows `picks` (relative to the concat) joined,
    // 1x1 to `out`.  Backbones pick every other 3x3 and keep c1 == c3; the heads pick all of them and halve c3.
    int elan(int c1, int c3, int n, const std::vector<int>& picks, int out) {
        conv(-1, c1, 1, 1);
        conv(-2, c1, 1, 1);
        for (int i = 0; i < n; ++i) conv(-1, c3, 3, 1);
        cat(picks);
        return conv(-1, out, 1, 1);
    }
    // MP transition of v7 / x: [maxpool, 1x1] beside [1x1, 3x3 stride 2], joined (with `extra`, a row of the top-down path, in the head)
    int mpdown(int ch, int extra = -1000) {
        mp(-1);
        conv(-1, ch, 1, 1);
        conv(-3, ch, 1, 1);
        conv(-1, ch, 3, 2);
        return extra == -1000 ? cat({-1, -3}) : cat({-1, -3, extra});
    }
    // top-down step of the head: 1x1, upsample, 1x1 of the backbone row `lateral`, joined
    int upjoin(int ch, int lateral) {
        conv(-1, ch, 1, 1);
        up(-1);
        conv(lateral, ch, 1, 1);
        return cat({-1, -2});
    }
};

// block.cpp:208-255: grids are the input over 8, 16, 32 (, 64); "netinfo" carries FOUR ints.  The registry's YoloLayer_TRT / 1 creator
// resolves this field set to the 6-float plugin.  Null when <detect>.anchor_grid does not describe exactly one level per detect convolution.
IPluginV2Layer* addYoLoLayer(Ctx& c, const std::string& lname, const std::vector<ITensor*>& dets, const Yolov7Config& cfg) {
    if ((size_t)need(c.wm, lname + ".anchor_grid").count != dets.size() * 6) return nullptr;
    std::vector<int> scales;
    for (size_t i = 0; i < dets.size(); ++i) scales.push_back(8 << i);
    return addAnchorYoLoLayer(c, lname, dets, {cfg.num_class, cfg.input_w, cfg.input_h, cfg.max_out_bbox}, scales);
}

// Each function leaves the rows the detect layer reads in `feats`; the detect layer is the next row.

void tiny(Rows& r, std::vector<int>& feats) {   // model.cpp:1775-2100
    const std::vector<int> pick4{-1, -2, -3, -4};
    auto stage = [&](int ch, int out) {   // two 1x1 of one input, two 3x3, all four joined
        r.conv(-1, ch, 1, 1);
        r.conv(-2, ch, 1, 1);
        r.conv(-1, ch, 3, 1);
        r.conv(-1, ch, 3, 1);
        r.cat(pick4);
        return r.conv(-1, out, 1, 1);
    };
    r.conv(-1, 32, 3, 2);
    r.conv(-1, 64, 3, 2);
    stage(32, 64);                          // 7
    r.mp(-1);
    const int p3 = stage(64, 128);          // 14
    r.mp(-1);
    const int p4 = stage(128, 256);         // 21
    r.mp(-1);
    stage(256, 512);                        // 28
    // SPP (model.cpp:1896-1935): the three pools read row 30 and are joined largest first
    r.conv(-1, 256, 1, 1);                  // 29
    r.conv(-2, 256, 1, 1);                  // 30
    r.push(r.maxpool(*r.at(-1), 5, 1, 2));  // 31
    r.push(r.maxpool(*r.at(-2), 9, 1, 4));  // 32
    r.push(r.maxpool(*r.at(-3), 13, 1, 6)); // 33
    r.cat({-1, -2, -3, -4});
    r.conv(-1, 256, 1, 1);                  // 35
    r.cat({-1, -7});
    const int p5 = r.conv(-1, 256, 1, 1);   // 37
    r.upjoin(128, p4);                      // 38-41
    const int n4 = stage(64, 128);          // 47
    r.upjoin(64, p3);                       // 48-51
    const int n3 = stage(32, 64);           // 57
    r.conv(-1, 128, 3, 2);
    r.cat({-1, n4});
    const int m4 = stage(64, 128);          // 65
    r.conv(-1, 256, 3, 2);
    r.cat({-1, p5});
    const int m5 = stage(128, 256);         // 73
    feats = {r.conv(n3, 128, 3, 1), r.conv(m4, 256, 3, 1), r.conv(m5, 512, 3, 1)};   // 74-76
}

void v7(Rows& r, std::vector<int>& feats) {   // model.cpp:1567-1773
    const std::vector<int> back{-1, -3, -5, -6}, head{-1, -2, -3, -4, -5, -6};
    r.conv(-1, 32, 3, 1);
    r.conv(-1, 64, 3, 2);
    r.conv(-1, 64, 3, 1);
    r.conv(-1, 128, 3, 2);
    r.elan(64, 64, 4, back, 256);                  // 11
    r.mpdown(128);
    const int p3 = r.elan(128, 128, 4, back, 512);   // 24
    r.mpdown(256);
    const int p4 = r.elan(256, 256, 4, back, 1024);  // 37
    r.mpdown(512);
    r.elan(256, 256, 4, back, 1024);               // 50
    const int p5 = r.sppcspc(-1, 512);             // 51
    r.upjoin(256, p4);
    const int n4 = r.elan(256, 128, 4, head, 256);   // 63
    r.upjoin(128, p3);
    const int n3 = r.elan(128, 64, 4, head, 128);    // 75
    r.mpdown(128, n4);
    const int m4 = r.elan(256, 128, 4, head, 256);   // 88
    r.mpdown(256, p5);
    const int m5 = r.elan(512, 256, 4, head, 512);   // 101
    feats = {r.repconv(n3, 256), r.repconv(m4, 512), r.repconv(m5, 1024)};   // 102-104
}

void v7x(Rows& r, std::vector<int>& feats) {   // model.cpp:1284-1565: the wide ELAN, six 3x3 convolutions, five rows joined
    const std::vector<int> pick{-1, -3, -5, -7, -8};
    r.conv(-1, 40, 3, 1);
    r.conv(-1, 80, 3, 2);
    r.conv(-1, 80, 3, 1);
    r.conv(-1, 160, 3, 2);
    r.elan(64, 64, 6, pick, 320);                  // 13
    r.mpdown(160);
    const int p3 = r.elan(128, 128, 6, pick, 640);   // 28
    r.mpdown(320);
    const int p4 = r.elan(256, 256, 6, pick, 1280);  // 43
    r.mpdown(640);
    r.elan(256, 256, 6, pick, 1280);               // 58
    const int p5 = r.sppcspc(-1, 640);             // 59
    r.upjoin(320, p4);
    const int n4 = r.elan(256, 256, 6, pick, 320);   // 73
    r.upjoin(160, p3);
    const int n3 = r.elan(128, 128, 6, pick, 160);   // 87
    r.mpdown(160, n4);
    const int m4 = r.elan(256, 256, 6, pick, 320);   // 102
    r.mpdown(320, p5);
    const int m5 = r.elan(512, 512, 6, pick, 640);   // 117
    feats = {r.conv(n3, 320, 3, 1), r.conv(m4, 640, 3, 1), r.conv(m5, 1280, 3, 1)};   // 118-120
}

void w6(Rows& r, std::vector<int>& feats) {   // model.cpp:1046-1282: ReOrg, stride-2 3x3 transitions, four levels
    const std::vector<int> back{-1, -3, -5, -6}, head{-1, -2, -3, -4, -5, -6};
    r.reorg(-1);
    r.conv(-1, 64, 3, 1);
    r.conv(-1, 128, 3, 2);
    r.elan(64, 64, 4, back, 128);                  // 10
    r.conv(-1, 256, 3, 2);
    const int p3 = r.elan(128, 128, 4, back, 256);   // 19
    r.conv(-1, 512, 3, 2);
    const int p4 = r.elan(256, 256, 4, back, 512);   // 28
    r.conv(-1, 768, 3, 2);
    const int p5 = r.elan(384, 384, 4, back, 768);   // 37
    r.conv(-1, 1024, 3, 2);
    r.elan(512, 512, 4, back, 1024);               // 46
    const int p6 = r.sppcspc(-1, 512);             // 47
    r.upjoin(384, p5);
    const int n5 = r.elan(384, 192, 4, head, 384);   // 59
    r.upjoin(256, p4);
    const int n4 = r.elan(256, 128, 4, head, 256);   // 71
    r.upjoin(128, p3);
    const int n3 = r.elan(128, 64, 4, head, 128);    // 83
    r.conv(-1, 256, 3, 2);
    r.cat({-1, n4});
    const int m4 = r.elan(256, 128, 4, head, 256);   // 93
    r.conv(-1, 384, 3, 2);
    r.cat({-1, n5});
    const int m5 = r.elan(384, 192, 4, head, 384);   // 103
    r.conv(-1, 512, 3, 2);
    r.cat({-1, p6});
    const int m6 = r.elan(512, 256, 4, head, 512);   // 113
    feats = {r.conv(n3, 256, 3, 1), r.conv(m4, 512, 3, 1), r.conv(m5, 768, 3, 1), r.conv(m6, 1024, 3, 1)};   // 114-117
}

void e6(Rows& r, std::vector<int>& feats) {   // model.cpp:775-1044: ReOrg, DownC transitions, six 3x3 convolutions per ELAN, four levels
    const std::vector<int> back{-1, -3, -5, -7, -8}, head{-1, -2, -3, -4, -5, -6, -7, -8};
    r.reorg(-1);
    r.conv(-1, 80, 3, 1);
    r.downc(-1, 80, 160);
    r.elan(64, 64, 6, back, 160);                  // 12
    r.downc(-1, 160, 320);
    const int p3 = r.elan(128, 128, 6, back, 320);   // 23
    r.downc(-1, 320, 640);
    const int p4 = r.elan(256, 256, 6, back, 640);   // 34
    r.downc(-1, 640, 960);
    const int p5 = r.elan(384, 384, 6, back, 960);   // 45
    r.downc(-1, 960, 1280);
    r.elan(512, 512, 6, back, 1280);               // 56
    const int p6 = r.sppcspc(-1, 640);             // 57
    r.upjoin(480, p5);
    const int n5 = r.elan(384, 192, 6, head, 480);   // 71
    r.upjoin(320, p4);
    const int n4 = r.elan(256, 128, 6, head, 320);   // 85
    r.upjoin(160, p3);
    const int n3 = r.elan(128, 64, 6, head, 160);    // 99
    r.downc(-1, 160, 320);
    r.cat({-1, n4});
    const int m4 = r.elan(256, 128, 6, head, 320);   // 111
    r.downc(-1, 320, 480);
    r.cat({-1, n5});
    const int m5 = r.elan(384, 192, 6, head, 480);   // 123
    r.downc(-1, 480, 640);
    r.cat({-1, p6});
    const int m6 = r.elan(512, 256, 6, head, 640);   // 135
    feats = {r.conv(n3, 320, 3, 1), r.conv(m4, 640, 3, 1), r.conv(m5, 960, 3, 1), r.conv(m6, 1280, 3, 1)};   // 136-139
}

}  // namespace

bool yolov7_model_valid(const std::string& name) {
    return name == "yolov7tiny" || name == "yolov7" || name == "yolov7x" || name == "yolov7w6" || name == "yolov7e6";
}

bool yolov7_model_p6(const std::string& name) { return name == "yolov7w6" || name == "yolov7e6"; }

IHostMemory* buildEngineYolov7(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const Yolov7Config& cfg) {
    if (!yolov7_model_valid(cfg.model)) return nullptr;
    Session s(builder, wts);
    Ctx& c = s.c;
    Rows r{c, cfg, cfg.model == "yolov7tiny", s.input("data", cfg.input_h, cfg.input_w), {}};
    std::vector<int> feats;
    if (cfg.model == "yolov7tiny") tiny(r, feats);
    else if (cfg.model == "yolov7") v7(r, feats);
    else if (cfg.model == "yolov7x") v7x(r, feats);
    else if (cfg.model == "yolov7w6") w6(r, feats);
    else e6(r, feats);

    const std::string detect = r.name();
    std::vector<ITensor*> dets;
    for (size_t i = 0; i < feats.size(); ++i) {   // the biased 1x1 `m.i` convolutions
        const std::string m = detect + ".m." + std::to_string(i);
        auto* det = s.net->addConvolutionNd(*r.at(feats[i]), 3 * (cfg.num_class + 5), DimsHW{1, 1}, need(s.wm, m + ".weight"), need(s.wm, m + ".bias"));
        assert(det);
        dets.push_back(det->getOutput(0));
    }
    if (cfg.mark_heads) s.mark_heads(dets);
    IPluginV2Layer* yolo = addYoLoLayer(c, detect, dets, cfg);
    if (!yolo) return nullptr;
    s.output(yolo->getOutput(0), "prob");
    return s.finish(builder, config, cfg.max_batch, cfg.fp16);
}

}  // namespace trtx_host
