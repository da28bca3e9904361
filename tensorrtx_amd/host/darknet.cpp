// Darknet YOLO detection (YOLOv3, YOLOv3-tiny, YOLOv4) through the network-definition API, implicit batch like the reference.  Restates
//   createEngine, convBnLeaky, addBatchNorm2d                       yolov3/yolov3.cpp:141-340
//   createEngine, convBnLeaky                                       yolov3-tiny/yolov3-tiny.cpp:173-296
//   createEngine, convBnMish, convBnLeaky                           yolov4/yolov4.cpp:166-480
// The reference writes each network out one variable per module of the Darknet cfg ("I just want to expand the complete arch of darknet"),
// and the module number is what names the weights: module_list.<i>.Conv2d.weight, module_list.<i>.BatchNorm2d.{weight,bias,running_mean,
// running_var}, and module_list.<i>.Conv2d.bias for the detect convolutions.  So here a network is a table with one row per module - kind,
// output channels, kernel, stride, padding, the modules it reads - and the row's position is its module number; route, shortcut, upsample
// and yolo modules hold their rows as they hold their numbers in the cfg.  The repeating groups (Darknet-53's residual stages, CSPDarknet's
// split stages) are appended by small generators; every row a generator appends is checked against the reference's numbering in
// tests/test_darknet_cpu.py.  What a row becomes is the reference's layer sequence:
//   convBnLeaky  Conv (no bias) -> Scale -> kLEAKY_RELU with alpha 0.1
//   convBnMish   Conv (no bias) -> Scale -> "Mish_TRT" / "1" from the registry, created with the creator's own (empty) field collection
//   upsample     addDeconvolutionNd(ch, 2x2, all ones) with stride 2 and ch groups
//   maxpool      addPoolingNd with the stride and padding the reference sets; yolov3-tiny's module 11 is addPaddingNd(0,0; 1,1) in front of a 2x2
//                stride-1 pool
//   detect       the biased 1x1 convolution with 3 * (classes + 5) outputs
// and at the end "YoloLayer_TRT" / "1" created with the creator's own empty field collection on the detect convolutions in the reference's
// order (coarsest first in yolov3 and yolov3-tiny, finest first in yolov4).  BatchNorm eps is what each file passes: 1e-5 in yolov3.cpp:181,
// 1e-4 in yolov3-tiny.cpp:213 and yolov4.cpp:206 / :223; the fold is float arithmetic (addBatchNorm2d's default here).
#include <cstring>
#include <vector>

#include "models.h"
#include "yolo_blocks.h"

using namespace nvinfer1;

namespace trtx_host {
using blocks::plugin_layer;
namespace {

enum Kind : char {
    LEAKY = 'L',      // convBnLeaky
    MISH = 'M',       // convBnMish
    DETECT = 'D',     // biased 1x1 convolution, 3 * (classes + 5) outputs
    SHORTCUT = 'S',   // element-wise sum of two modules
    ROUTE = 'R',      // one module: the same tensor; several: their concatenation in the order given
    POOL = 'P',       // max-pool k, stride s, padding p
    PADPOOL = 'Z',    // Pad(0,0; 1,1) -> max-pool 2x2 stride 1 (yolov3-tiny module 11)
    UPSAMPLE = 'U',   // the all-ones grouped 2x2 stride-2 deconvolution
    YOLO = 'Y',       // a yolo module: no layer of its own, the plugin at the end reads the detect convolution in front of it
};

struct Row {
    Kind kind;
    int ch, k, s, p;
    std::vector<int> from;   // module numbers; empty = the module in front
};

struct Table {
    std::vector<Row> rows;
    int size() const { return (int)rows.size(); }
    int add(Kind kind, int ch = 0, int k = 0, int s = 0, int p = 0, std::vector<int> from = {}) {
        rows.push_back(Row{kind, ch, k, s, p, std::move(from)});
        return size() - 1;
    }
    int conv(Kind kind, int ch, int k, int s = 1) { return add(kind, ch, k, s, k / 2); }
    int shortcut() { return add(SHORTCUT, 0, 0, 0, 0, {size() - 1, size() - 3}); }
    int route(std::vector<int> from) { return add(ROUTE, 0, 0, 0, 0, std::move(from)); }
};

// Darknet-53 stage (yolov3.cpp:202-275): a 3x3 stride-2 convolution, then n times [1x1 to half, 3x3 back, shortcut over the pair]
void residual_stage(Table& t, int ch, int n) {
    t.conv(LEAKY, ch, 3, 2);
    for (int i = 0; i < n; ++i) {
        t.conv(LEAKY, ch / 2, 1);
        t.conv(LEAKY, ch, 3);
        t.shortcut();
    }
}

// the six alternating 1x1 / 3x3 convolutions in front of a detect convolution, or five and no last 3x3 (`n` rows)
void neck(Table& t, Kind kind, int ch, int n) {
    for (int i = 0; i < n; ++i) t.conv(kind, i % 2 ? 2 * ch : ch, i % 2 ? 3 : 1);
}

Table yolov3_table() {   // yolov3.cpp:201-326, modules 0 .. 105
    Table t;
    t.conv(LEAKY, 32, 3);
    residual_stage(t, 64, 1);      // 1 .. 4
    residual_stage(t, 128, 2);     // 5 .. 11
    residual_stage(t, 256, 8);     // 12 .. 36
    residual_stage(t, 512, 8);     // 37 .. 61
    residual_stage(t, 1024, 4);    // 62 .. 74
    neck(t, LEAKY, 512, 6);        // 75 .. 80
    t.add(DETECT);                 // 81
    t.add(YOLO);                   // 82
    t.route({79});                 // 83
    t.conv(LEAKY, 256, 1);         // 84
    t.add(UPSAMPLE);               // 85
    t.route({85, 61});             // 86
    neck(t, LEAKY, 256, 6);        // 87 .. 92
    t.add(DETECT);                 // 93
    t.add(YOLO);                   // 94
    t.route({91});                 // 95
    t.conv(LEAKY, 128, 1);         // 96
    t.add(UPSAMPLE);               // 97
    t.route({97, 36});             // 98
    neck(t, LEAKY, 128, 6);        // 99 .. 104
    t.add(DETECT);                 // 105
    t.add(YOLO);                   // 106
    return t;
}

Table yolov3_tiny_table() {   // yolov3-tiny.cpp:232-273, modules 0 .. 22
    Table t;
    for (int ch = 16; ch <= 256; ch *= 2) {   // 0 .. 9
        t.conv(LEAKY, ch, 3);
        t.add(POOL, 0, 2, 2, 0);
    }
    t.conv(LEAKY, 512, 3);         // 10
    t.add(PADPOOL);                // 11
    t.conv(LEAKY, 1024, 3);        // 12
    t.conv(LEAKY, 256, 1);         // 13
    t.conv(LEAKY, 512, 3);         // 14
    t.add(DETECT);                 // 15
    t.add(YOLO);                   // 16
    t.route({13});                 // 17
    t.conv(LEAKY, 128, 1);         // 18
    t.add(UPSAMPLE);               // 19
    t.route({19, 8});              // 20
    t.conv(LEAKY, 256, 3);         // 21
    t.add(DETECT);                 // 22
    t.add(YOLO);                   // 23
    return t;
}

// CSPDarknet stage (yolov4.cpp:244-256 and on): a 3x3 stride-2 convolution d; a 1x1 of d kept aside; a route back to d; another 1x1 of d;
// n residual blocks [1x1, 3x3, shortcut]; a 1x1; the concatenation with the one kept aside; a 1x1 to ch.  The first stage keeps the full
// width in both branches and narrows only inside its block.
void csp_stage(Table& t, int ch, int n, bool first) {
    const int half = first ? ch : ch / 2;
    const int d = t.conv(MISH, ch, 3, 2);
    const int aside = t.conv(MISH, half, 1);
    t.route({d});
    t.conv(MISH, half, 1);
    for (int i = 0; i < n; ++i) {
        t.conv(MISH, first ? ch / 2 : half, 1);
        t.conv(MISH, half, 3);
        t.shortcut();
    }
    const int last = t.conv(MISH, half, 1);
    t.route({last, aside});
    t.conv(MISH, ch, 1);
}

Table yolov4_table() {   // yolov4.cpp:243-469, modules 0 .. 160
    Table t;
    t.conv(MISH, 32, 3);
    csp_stage(t, 64, 1, true);     // 1 .. 10
    csp_stage(t, 128, 2, false);   // 11 .. 23
    csp_stage(t, 256, 8, false);   // 24 .. 54
    csp_stage(t, 512, 8, false);   // 55 .. 85
    csp_stage(t, 1024, 4, false);  // 86 .. 104
    neck(t, LEAKY, 512, 3);        // 105 .. 107
    t.add(POOL, 0, 5, 1, 2);       // 108: SPP, three stride-1 pools of module 107
    t.route({107});                // 109
    t.add(POOL, 0, 9, 1, 4);       // 110
    t.route({107});                // 111
    t.add(POOL, 0, 13, 1, 6);      // 112
    t.route({112, 110, 108, 107}); // 113
    neck(t, LEAKY, 512, 3);        // 114 .. 116
    t.conv(LEAKY, 256, 1);         // 117
    t.add(UPSAMPLE);               // 118
    t.route({85});                 // 119
    t.conv(LEAKY, 256, 1);         // 120
    t.route({120, 118});           // 121
    neck(t, LEAKY, 256, 5);        // 122 .. 126
    t.conv(LEAKY, 128, 1);         // 127
    t.add(UPSAMPLE);               // 128
    t.route({54});                 // 129
    t.conv(LEAKY, 128, 1);         // 130
    t.route({130, 128});           // 131
    neck(t, LEAKY, 128, 6);        // 132 .. 137
    t.add(DETECT);                 // 138
    t.add(YOLO);                   // 139
    t.route({136});                // 140
    t.conv(LEAKY, 256, 3, 2);      // 141
    t.route({141, 126});           // 142
    neck(t, LEAKY, 256, 6);        // 143 .. 148
    t.add(DETECT);                 // 149
    t.add(YOLO);                   // 150
    t.route({147});                // 151
    t.conv(LEAKY, 512, 3, 2);      // 152
    t.route({152, 116});           // 153
    neck(t, LEAKY, 512, 6);        // 154 .. 159
    t.add(DETECT);                 // 160
    t.add(YOLO);                   // 161
    return t;
}

// One network under construction: y[i] is the output of module i (null for a yolo module).
struct Build {
    Ctx& c;
    const DarknetConfig& cfg;
    float eps;
    std::vector<ITensor*> y;
    std::vector<ITensor*> dets;

    ITensor* convBn(ITensor& in, const Row& r, int i) {   // the convolution layer is named module_list.<i>.Conv2d
        const std::string m = "module_list." + std::to_string(i);
        return blocks::conv_bn(c, in, r.ch, r.k, r.s, r.p, m + ".Conv2d", m + ".BatchNorm2d", 1, false, eps, /*named=*/true);
    }
    ITensor* mish(ITensor& in, int i) {   // yolov4.cpp:208-212
        auto* layer = plugin_layer(c, "Mish_TRT", "mish" + std::to_string(i), nullptr, {&in});
        assert(layer);
        return layer->getOutput(0);
    }
    ITensor* upsample(ITensor& in, int i) {   // yolov4.cpp:393-402
        const int ch = (int)in.getDimensions().d[0];
        float* ones = static_cast<float*>(std::malloc(sizeof(float) * ch * 4));
        for (int j = 0; j < ch * 4; ++j) ones[j] = 1.0f;
        const Weights w{DataType::kFLOAT, ones, (int64_t)ch * 4};
        c.wm["deconv" + std::to_string(i)] = w;   // released with the map
        auto* up = c.net->addDeconvolutionNd(in, ch, DimsHW{2, 2}, w, noWeights());
        assert(up);
        up->setStrideNd(DimsHW{2, 2});
        up->setNbGroups(ch);
        return up->getOutput(0);
    }

    void run(const Table& t, ITensor* image) {
        for (int i = 0; i < t.size(); ++i) {
            const Row& r = t.rows[i];
            ITensor* in = r.from.empty() ? (i ? y[i - 1] : image) : y[r.from[0]];
            ITensor* out = nullptr;
            switch (r.kind) {
                case LEAKY: out = blocks::leaky(c, convBn(*in, r, i)); break;
                case MISH: out = mish(*convBn(*in, r, i), i); break;
                case DETECT: {
                    const std::string m = "module_list." + std::to_string(i) + ".Conv2d";
                    auto* det = c.net->addConvolutionNd(*in, 3 * (cfg.num_class + 5), DimsHW{1, 1}, need(c.wm, m + ".weight"), need(c.wm, m + ".bias"));
                    assert(det);
                    det->setName(m.c_str());
                    out = det->getOutput(0);
                    dets.push_back(out);
                    break;
                }
                case SHORTCUT: out = blocks::sum(c, *y[r.from[0]], *y[r.from[1]]); break;
                case ROUTE:
                    if (r.from.size() == 1) {
                        out = y[r.from[0]];
                    } else {
                        std::vector<ITensor*> v;
                        for (int f : r.from) v.push_back(y[f]);
                        out = blocks::cat(c, v);
                    }
                    break;
                case POOL: out = blocks::maxpool(c, *in, r.k, r.s, r.p); break;
                case PADPOOL: {   // yolov3-tiny.cpp:248-250
                    auto* pad = c.net->addPaddingNd(*in, DimsHW{0, 0}, DimsHW{1, 1});
                    assert(pad);
                    out = blocks::maxpool(c, *pad->getOutput(0), 2, 1, 0);
                    break;
                }
                case UPSAMPLE: out = upsample(*in, i); break;
                case YOLO: break;
            }
            y.push_back(out);
        }
    }
};

}  // namespace

bool darknet_model_valid(const std::string& name) { return name == "yolov3" || name == "yolov3-tiny" || name == "yolov4"; }

std::string darknet_rows_json(const std::string& name) {
    if (!darknet_model_valid(name)) return "";
    const Table t = name == "yolov3" ? yolov3_table() : (name == "yolov4" ? yolov4_table() : yolov3_tiny_table());
    std::string o = "[";
    for (int i = 0; i < t.size(); ++i) {
        const Row& r = t.rows[i];
        o += std::string(i ? "," : "") + "[" + std::to_string(i) + ",\"" + (char)r.kind + "\"," + std::to_string(r.ch) + "," + std::to_string(r.k) + "," +
             std::to_string(r.s) + "," + std::to_string(r.p) + ",[";
        for (size_t j = 0; j < r.from.size(); ++j) o += (j ? "," : "") + std::to_string(r.from[j]);
        o += "]]";
    }
    return o + "]";
}

IHostMemory* buildEngineDarknet(IBuilder* builder, IBuilderConfig* config, const std::string& wts, const DarknetConfig& cfg) {
    if (!darknet_model_valid(cfg.model)) return nullptr;
    const Table t = cfg.model == "yolov3" ? yolov3_table() : (cfg.model == "yolov4" ? yolov4_table() : yolov3_tiny_table());
    Session s(builder, wts);
    Build b{s.c, cfg, cfg.model == "yolov3" ? 1e-5f : 1e-4f, {}, {}};
    b.run(t, s.input("data", cfg.input_h, cfg.input_w));
    if (cfg.mark_heads) s.mark_heads(b.dets);
    // yolov4.cpp:471-473: created with the creator's own field collection, which is empty; that is what tells the registry's creator the Darknet form
    auto* yolo = plugin_layer(s.c, "YoloLayer_TRT", "yololayer", nullptr, b.dets);
    if (!yolo) return nullptr;
    s.output(yolo->getOutput(0), "prob");
    return s.finish(builder, config, cfg.max_batch, cfg.fp16);
}

}  // namespace trtx_host
