// Built-in HIP plugins, registered under the names the reference host code asks the registry for.
//   "YoloLayer_TRT"/"1"  — yolov8/plugin/yololayer.{h,cu} (creator: yololayer.cu:320-369); the yolov5 and yolov9 plugins of that name too
// Each plugin is a small host object exposed through the C v-table of include/trtx_hip.h; its
// enqueue calls the HIP operator entry points of section 1.  Serialization blobs keep the reference's
// field order so a plan round-trips byte for byte.
#include <string.h>

#include <vector>

#include "../common.h"
#include "../runtime/plugin.h"

namespace trtx {
namespace {

template <typename T>
void put(std::vector<uint8_t>& b, const T& v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
}
template <typename T>
bool get(const uint8_t*& p, const uint8_t* end, T& v) {
    if (p + sizeof(T) > end) return false;
    memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return true;
}

// ------------------------------------------------------------------------------------------------
struct YoloLayer {
    int class_count = 80, n_kpt = 17;
    float kpt_conf = 0.f;
    int thread_count = 256, net_w = 640, net_h = 640, max_out = 1000;
    std::vector<int> strides;
    bool seg = false, pose = false, obb = false;
    int max_batch = 1;

    std::vector<uint8_t> blob() const {  // yololayer.cu:75-101
        std::vector<uint8_t> b;
        put(b, class_count);
        put(b, n_kpt);
        put(b, kpt_conf);
        put(b, thread_count);
        put(b, net_w);
        put(b, net_h);
        put(b, max_out);
        put(b, (int)strides.size());
        for (int s : strides) put(b, s);
        put(b, seg);
        put(b, pose);
        put(b, obb);
        return b;
    }
    static YoloLayer* from_blob(const void* data, size_t len) {  // yololayer.cu:53-73
        const uint8_t* p = static_cast<const uint8_t*>(data);
        const uint8_t* end = p + len;
        auto* y = new YoloLayer();
        int ns = 0;
        bool ok = get(p, end, y->class_count) && get(p, end, y->n_kpt) && get(p, end, y->kpt_conf) &&
                  get(p, end, y->thread_count) && get(p, end, y->net_w) && get(p, end, y->net_h) &&
                  get(p, end, y->max_out) && get(p, end, ns) && ns >= 0 && ns <= 8;
        for (int i = 0; ok && i < ns; ++i) {
            int s = 0;
            ok = get(p, end, s);
            y->strides.push_back(s);
        }
        ok = ok && get(p, end, y->seg) && get(p, end, y->pose) && get(p, end, y->obb) && p == end;
        if (!ok) {
            delete y;
            return nullptr;
        }
        return y;
    }
};

void yolo_fill(trtx_plugin_vtbl* v, YoloLayer* y);

int32_t yolo_nb_outputs(void*) { return 1; }
int32_t yolo_output_dims(void* s, int32_t, const trtx_dims*, int32_t, trtx_dims* out) {
    auto* y = static_cast<YoloLayer*>(s);
    out->nb = 3;  // Dims3(total_size + 1, 1, 1), yololayer.cu:107-111
    out->d[0] = (int64_t)y->max_out * kYoloDetFloats + 1;
    out->d[1] = 1;
    out->d[2] = 1;
    return 0;
}
int32_t yolo_configure(void* s, const trtx_dims* in, int32_t nb_in, const trtx_dims*, int32_t, int32_t max_batch) {
    auto* y = static_cast<YoloLayer*>(s);
    y->max_batch = max_batch;
    if (nb_in != (int)y->strides.size()) return 1;
    for (int i = 0; i < nb_in; ++i) {
        const int64_t cells = (int64_t)(y->net_h / y->strides[i]) * (y->net_w / y->strides[i]);
        int64_t vol = 1;
        for (int k = 0; k < in[i].nb; ++k) vol *= in[i].d[k];
        const int info = 4 + y->class_count + (y->seg ? 32 : 0) + (y->pose ? y->n_kpt * 3 : 0) + (y->obb ? 1 : 0);
        if (vol != cells * info) return 1;  // [4 + classes (+32) (+3*nk) (+1), cells]
    }
    return 0;
}
int32_t yolo_initialize(void* s) {
    auto* y = static_cast<YoloLayer*>(s);
    return (y->n_kpt < 0 || y->n_kpt > 17) ? 1 : 0;  // Detection::keypoints holds kNumberOfPoints = 17 triples
}
void yolo_terminate(void*) {}
size_t yolo_workspace(void* s, int32_t max_batch) {
    auto* y = static_cast<YoloLayer*>(s);
    return trtx_yolo_decode_workspace(max_batch, y->net_h, y->net_w, y->strides.data(), (int)y->strides.size());
}
int32_t yolo_enqueue(void* s, int32_t batch, const void* const* inputs, void* const* outputs, void* ws,
                     trtx_stream_t stream) {
    auto* y = static_cast<YoloLayer*>(s);
    const size_t ws_bytes =
            trtx_yolo_decode_workspace(batch, y->net_h, y->net_w, y->strides.data(), (int)y->strides.size());
    return trtx_yolo_decode_ex(reinterpret_cast<const float* const*>(inputs), (int)y->strides.size(), batch, y->class_count, y->net_h,
                               y->net_w, y->strides.data(), y->max_out, y->n_kpt, y->kpt_conf, y->seg, y->pose, y->obb,
                               static_cast<float*>(outputs[0]), ws, ws_bytes, stream);
}
size_t yolo_ser_size(void* s) { return static_cast<YoloLayer*>(s)->blob().size(); }
void yolo_serialize(void* s, void* buf) {
    const auto b = static_cast<YoloLayer*>(s)->blob();
    memcpy(buf, b.data(), b.size());
}
const char* yolo_type(void*) { return "YoloLayer_TRT"; }
const char* yolo_version(void*) { return "1"; }
int32_t yolo_clone(void* s, trtx_plugin_vtbl* out) {
    yolo_fill(out, new YoloLayer(*static_cast<YoloLayer*>(s)));
    return 0;
}
void yolo_destroy(void* s) { delete static_cast<YoloLayer*>(s); }

void yolo_fill(trtx_plugin_vtbl* v, YoloLayer* y) {
    v->self = y;
    v->get_nb_outputs = yolo_nb_outputs;
    v->get_output_dims = yolo_output_dims;
    v->configure = yolo_configure;
    v->initialize = yolo_initialize;
    v->terminate = yolo_terminate;
    v->workspace_size = yolo_workspace;
    v->enqueue = yolo_enqueue;
    v->serialization_size = yolo_ser_size;
    v->serialize = yolo_serialize;
    v->plugin_type = yolo_type;
    v->plugin_version = yolo_version;
    v->clone = yolo_clone;
    v->destroy = yolo_destroy;
}

// ------------------------------------------------------------------------------------------------
// The anchor-based forms of "YoloLayer_TRT"/"1" (the same registered name as the YOLOv8 plugin in the reference, other parameter sets),
// one state for both:
//   YOLOv5 (yolov5/plugin/yololayer.{h,cu}): creator fields "netinfo" = int32[5] {classes, W, H, maxOut, isSeg} and "kernels" =
//     YoloKernel[n] {int width, height; float anchors[6]} (yolov5/src/model.cpp:246-275, yololayer.cu:250-266); blob int classCount,
//     threadCount, kernelCount, netW, netH, maxOut, bool isSeg, YoloKernel[n] = 25 + 32 n bytes (yololayer.cu:49-89); Detection
//     records of 38 floats.
//   YOLOv7 (yolov7/plugin/yololayer.{h,cu}): the same without the segmentation flag and with records of 6 floats.  "netinfo" =
//     int32[4] {classes, W, H, maxOut} - exactly four, five and more are YOLOv5's - and "kernels" (yolov7/src/block.cpp:220-255); the
//     blob has no isSeg byte, 24 + 32 n bytes (yololayer.cu:40-78).
//   Darknet (yolov3, yolov3-tiny, yolov4 / yololayer.{h,cu}): the creator takes NO fields and the reference compiles classes, input size,
//     the YoloKernel table and maxOut = 1000 in (yolov4/yololayer.h:10-38, yololayer.cu:9-27, 258-263).  Here the plugin learns them from
//     its inputs (darknet_geometry below) when the layer is added and again in configurePlugin; records of 7 floats.  The blob is the
//     reference's - int classCount, threadCount, kernelCount, YoloKernel[n] (yololayer.cu:58-75) - plus int netW, netH behind it, as
//     Decode_TRT extends an empty blob: 20 + 32 n bytes, n = 0 for a plugin that has not seen its inputs.
struct AnchorKernel {
    int width, height;
    float anchors[6];
};
enum AnchorForm { FORM_V5 = 0, FORM_V7 = 1, FORM_DARKNET = 2 };
constexpr int kDarknetMaxOut = 1000;   // MAX_OUTPUT_BBOX_COUNT, yololayer.h:12 of all three
struct AnchorLayer {
    int form = FORM_V5;   // never serialised, the blob's length tells
    int class_count = 80, thread_count = 256, net_w = 640, net_h = 640, max_out = 1000;
    bool seg = false;  // YOLOv5 only
    std::vector<AnchorKernel> kernels;

    int det_floats() const { return form == FORM_DARKNET ? 7 : (form == FORM_V7 ? 6 : 38); }
    std::vector<uint8_t> blob() const {
        std::vector<uint8_t> b;
        put(b, class_count);
        put(b, thread_count);
        put(b, (int)kernels.size());
        if (form == FORM_DARKNET) {
            for (const auto& k : kernels) put(b, k);
            put(b, net_w);
            put(b, net_h);
            return b;
        }
        put(b, net_w);
        put(b, net_h);
        put(b, max_out);
        if (form == FORM_V5) put(b, seg);
        for (const auto& k : kernels) put(b, k);
        return b;
    }
    // the Darknet blob, by its exact length: 20 + 32 n bytes, n = 0 .. 8
    static AnchorLayer* from_darknet_blob(const void* data, size_t len) {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        const uint8_t* end = p + len;
        auto* y = new AnchorLayer();
        y->form = FORM_DARKNET;
        y->max_out = kDarknetMaxOut;
        int nk = 0;
        bool ok = get(p, end, y->class_count) && get(p, end, y->thread_count) && get(p, end, nk) && nk >= 0 && nk <= 8 &&
                  (size_t)(end - p) == (size_t)nk * sizeof(AnchorKernel) + 2 * sizeof(int);
        for (int i = 0; ok && i < nk; ++i) {
            AnchorKernel k{};
            ok = get(p, end, k) && k.width > 0 && k.height > 0;
            y->kernels.push_back(k);
        }
        ok = ok && get(p, end, y->net_w) && get(p, end, y->net_h) && y->class_count >= 1 && (nk == 0 || (y->net_w >= 1 && y->net_h >= 1));
        if (!ok) {
            delete y;
            return nullptr;
        }
        return y;
    }
    // accepted by its exact length and a kernelCount that agrees with it only
    static AnchorLayer* from_blob(const void* data, size_t len, bool v7) {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        const uint8_t* end = p + len;
        auto* y = new AnchorLayer();
        y->form = v7 ? FORM_V7 : FORM_V5;
        int nk = 0;
        bool ok = get(p, end, y->class_count) && get(p, end, y->thread_count) && get(p, end, nk) && get(p, end, y->net_w) &&
                  get(p, end, y->net_h) && get(p, end, y->max_out) && (v7 || get(p, end, y->seg)) && nk >= 1 && nk <= 8 &&
                  (size_t)(end - p) == (size_t)nk * sizeof(AnchorKernel);
        for (int i = 0; ok && i < nk; ++i) {
            AnchorKernel k{};
            ok = get(p, end, k) && k.width > 0 && k.height > 0;
            y->kernels.push_back(k);
        }
        if (!ok || y->class_count < 1 || y->max_out < 1 || (v7 && (y->net_w < 1 || y->net_h < 1))) {
            delete y;
            return nullptr;
        }
        return y;
    }
    void geometry(std::vector<int>* gw, std::vector<int>* gh, std::vector<float>* an) const {
        for (const auto& k : kernels) {
            gw->push_back(k.width);
            gh->push_back(k.height);
            an->insert(an->end(), k.anchors, k.anchors + 6);
        }
    }
};

// What the Darknet form reads off its inputs (CHW each, 3 * (5 + classes) channels): the family and with it the anchor table of that
// family's yololayer.h, the grids, and the network size = grid x stride.
//   two inputs, strides 32 and 16 (coarsest first): yolov3-tiny      {81,82, 135,169, 344,319}, {23,27, 37,58, 81,82}
//   three inputs, strides 32, 16, 8 (coarsest first): yolov3         {116,90, 156,198, 373,326}, {30,61, 62,45, 59,119}, {10,13, 16,30, 33,23}
//   three inputs, strides 8, 16, 32 (finest first): yolov4           {12,16, 19,36, 40,28}, {36,75, 76,55, 72,146}, {142,110, 192,243, 459,401}
// Anything else is refused.
bool darknet_geometry(const trtx_dims* in, int nb_in, AnchorLayer* y) {
    static const float kTiny[2][6] = {{81, 82, 135, 169, 344, 319}, {23, 27, 37, 58, 81, 82}};
    static const float kV3[3][6] = {{116, 90, 156, 198, 373, 326}, {30, 61, 62, 45, 59, 119}, {10, 13, 16, 30, 33, 23}};
    static const float kV4[3][6] = {{12, 16, 19, 36, 40, 28}, {36, 75, 76, 55, 72, 146}, {142, 110, 192, 243, 459, 401}};
    if (!in || (nb_in != 2 && nb_in != 3)) return false;
    for (int i = 0; i < nb_in; ++i)
        if (in[i].nb != 3 || in[i].d[0] != in[0].d[0] || in[i].d[1] < 1 || in[i].d[2] < 1) return false;
    const int64_t ch = in[0].d[0];
    if (ch % 3 || ch / 3 - 5 < 1) return false;
    auto ratio = [&](int a, int b, int r) { return in[a].d[1] == r * in[b].d[1] && in[a].d[2] == r * in[b].d[2]; };
    const float(*table)[6] = nullptr;
    int coarsest = 0;
    if (nb_in == 2 && ratio(1, 0, 2)) table = kTiny;
    else if (nb_in == 3 && ratio(1, 0, 2) && ratio(2, 0, 4)) table = kV3;
    else if (nb_in == 3 && ratio(1, 2, 2) && ratio(0, 2, 4)) table = kV4, coarsest = 2;
    if (!table || in[coarsest].d[1] * 32 > INT32_MAX || in[coarsest].d[2] * 32 > INT32_MAX) return false;
    y->class_count = (int)(ch / 3 - 5);
    y->net_h = (int)in[coarsest].d[1] * 32;
    y->net_w = (int)in[coarsest].d[2] * 32;
    y->kernels.resize(nb_in);
    for (int i = 0; i < nb_in; ++i) {
        y->kernels[i].width = (int)in[i].d[2];
        y->kernels[i].height = (int)in[i].d[1];
        memcpy(y->kernels[i].anchors, table[i], sizeof(y->kernels[i].anchors));
    }
    return true;
}

void anchor_fill(trtx_plugin_vtbl* v, AnchorLayer* y);
int32_t anchor_output_dims(void* s, int32_t, const trtx_dims* in, int32_t nb_in, trtx_dims* out) {
    auto* y = static_cast<AnchorLayer*>(s);
    if (y->form == FORM_DARKNET && !darknet_geometry(in, nb_in, y)) return 1;
    out->nb = 3;  // Dims3(maxOut * sizeof(Detection) / 4 + 1, 1, 1), yolov5 yololayer.cu:101-105, yolov7 yololayer.cu:90-94
    out->d[0] = (int64_t)y->max_out * y->det_floats() + 1;
    out->d[1] = 1;
    out->d[2] = 1;
    return 0;
}
int32_t anchor_configure(void* s, const trtx_dims* in, int32_t nb_in, const trtx_dims*, int32_t, int32_t) {
    auto* y = static_cast<AnchorLayer*>(s);
    if (y->form == FORM_DARKNET) return darknet_geometry(in, nb_in, y) ? 0 : 1;
    if (nb_in != (int)y->kernels.size()) return 1;
    const int info = 5 + y->class_count + (y->seg ? 32 : 0);
    for (int i = 0; i < nb_in; ++i) {
        int64_t vol = 1;
        for (int k = 0; k < in[i].nb; ++k) vol *= in[i].d[k];
        if (vol != (int64_t)3 * info * y->kernels[i].width * y->kernels[i].height) return 1;
    }
    return 0;
}
int32_t no_initialize(void*) { return 0; }
size_t anchor_workspace(void* s, int32_t max_batch) {
    auto* y = static_cast<AnchorLayer*>(s);
    std::vector<int> gw, gh;
    std::vector<float> an;
    y->geometry(&gw, &gh, &an);
    return trtx_yolov5_decode_workspace(max_batch, gw.data(), gh.data(), (int)gw.size());   // the same for the three forms
}
int32_t anchor_enqueue(void* s, int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) {
    auto* y = static_cast<AnchorLayer*>(s);
    std::vector<int> gw, gh;
    std::vector<float> an;
    y->geometry(&gw, &gh, &an);
    const size_t ws_bytes = trtx_yolov5_decode_workspace(batch, gw.data(), gh.data(), (int)gw.size());
    const auto* in = reinterpret_cast<const float* const*>(inputs);
    float* out = static_cast<float*>(outputs[0]);
    if (y->form == FORM_DARKNET)
        return trtx_darknet_decode(in, (int)gw.size(), batch, y->class_count, y->net_h, y->net_w, gw.data(), gh.data(), an.data(), y->max_out, out,
                                   ws, ws_bytes, stream);
    if (y->form == FORM_V7)
        return trtx_yolov7_decode(in, (int)gw.size(), batch, y->class_count, y->net_h, y->net_w, gw.data(), gh.data(), an.data(), y->max_out, out,
                                  ws, ws_bytes, stream);
    return trtx_yolov5_decode(in, (int)gw.size(), batch, y->class_count, y->net_h, y->net_w, gw.data(), gh.data(), an.data(), y->max_out,
                              y->seg ? 1 : 0, out, ws, ws_bytes, stream);
}
size_t anchor_ser_size(void* s) { return static_cast<AnchorLayer*>(s)->blob().size(); }
void anchor_serialize(void* s, void* buf) {
    const auto b = static_cast<AnchorLayer*>(s)->blob();
    memcpy(buf, b.data(), b.size());
}
int32_t anchor_clone(void* s, trtx_plugin_vtbl* out) {
    anchor_fill(out, new AnchorLayer(*static_cast<AnchorLayer*>(s)));
    return 0;
}
void anchor_destroy(void* s) { delete static_cast<AnchorLayer*>(s); }
void anchor_fill(trtx_plugin_vtbl* v, AnchorLayer* y) {
    v->self = y;
    v->get_nb_outputs = yolo_nb_outputs;
    v->get_output_dims = anchor_output_dims;
    v->configure = anchor_configure;
    v->initialize = no_initialize;
    v->terminate = yolo_terminate;
    v->workspace_size = anchor_workspace;
    v->enqueue = anchor_enqueue;
    v->serialization_size = anchor_ser_size;
    v->serialize = anchor_serialize;
    v->plugin_type = yolo_type;
    v->plugin_version = yolo_version;
    v->clone = anchor_clone;
    v->destroy = anchor_destroy;
}
// netinfo of exactly four ints, all >= 1: YOLOv7's; of five and more, taken as they come: YOLOv5's
int32_t anchor_create(const trtx_plugin_field* f, trtx_plugin_vtbl* out) {
    if (!f[0].data || !f[1].data || f[0].length < 4 || f[1].length < 1 || f[1].length > 8) return 1;
    const bool v7 = f[0].length == 4;
    const int* ni = static_cast<const int*>(f[0].data);
    if (v7 && (ni[0] < 1 || ni[1] < 1 || ni[2] < 1 || ni[3] < 1)) return 1;
    auto* y = new AnchorLayer();
    y->form = v7 ? FORM_V7 : FORM_V5;
    y->class_count = ni[0];
    y->net_w = ni[1];
    y->net_h = ni[2];
    y->max_out = ni[3];
    y->seg = !v7 && ni[4] != 0;
    y->kernels.resize(f[1].length);  // the reference counts this field in YoloKernel elements (model.cpp:272-273, block.cpp:241-242)
    memcpy(y->kernels.data(), f[1].data, sizeof(AnchorKernel) * f[1].length);
    anchor_fill(out, y);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The YOLOv9 form of "YoloLayer_TRT"/"1" (yolov9/plugin/yololayer.{h,cu}; the same registered name again): ONE creator field "netinfo" =
// int32[5] {classes, W, H, maxOut, isSeg} (yololayer.cu:220-232); blob int classCount, threadCount, netW, netH, maxOut, bool isSeg
// = 21 bytes (yololayer.cu:36-60).  Three inputs on the strides 8 / 16 / 32 with grids H / s x W / s (:185-186), each
// (4 + classes (+ 32), cells); output 1 + maxOut * 38 floats.
struct Yolo9Layer {
    int class_count = 80, thread_count = 256, net_w = 640, net_h = 640, max_out = 1000;
    bool seg = false;

    std::vector<uint8_t> blob() const {
        std::vector<uint8_t> b;
        put(b, class_count);
        put(b, thread_count);
        put(b, net_w);
        put(b, net_h);
        put(b, max_out);
        put(b, seg);
        return b;
    }
    static Yolo9Layer* from_blob(const void* data, size_t len) {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        const uint8_t* end = p + len;
        auto* y = new Yolo9Layer();
        const bool ok = get(p, end, y->class_count) && get(p, end, y->thread_count) && get(p, end, y->net_w) && get(p, end, y->net_h) &&
                        get(p, end, y->max_out) && get(p, end, y->seg) && p == end;
        if (!ok || y->class_count < 1 || y->max_out < 1 || y->net_w < 32 || y->net_h < 32) {
            delete y;
            return nullptr;
        }
        return y;
    }
};

void yolo9_fill(trtx_plugin_vtbl* v, Yolo9Layer* y);
int32_t yolo9_output_dims(void* s, int32_t, const trtx_dims*, int32_t, trtx_dims* out) {
    auto* y = static_cast<Yolo9Layer*>(s);
    out->nb = 3;  // Dims3(maxOut * sizeof(Detection) / 4 + 1, 1, 1), yololayer.cu:70-73
    out->d[0] = (int64_t)y->max_out * 38 + 1;
    out->d[1] = 1;
    out->d[2] = 1;
    return 0;
}
int32_t yolo9_configure(void* s, const trtx_dims* in, int32_t nb_in, const trtx_dims*, int32_t, int32_t) {
    auto* y = static_cast<Yolo9Layer*>(s);
    if (nb_in != 3) return 1;
    const int info = 4 + y->class_count + (y->seg ? 32 : 0);
    for (int i = 0; i < nb_in; ++i) {
        int64_t vol = 1;
        for (int k = 0; k < in[i].nb; ++k) vol *= in[i].d[k];
        if (vol != (int64_t)info * (y->net_h / (8 << i)) * (y->net_w / (8 << i))) return 1;
    }
    return 0;
}
size_t yolo9_workspace(void* s, int32_t max_batch) {
    auto* y = static_cast<Yolo9Layer*>(s);
    return trtx_yolov9_decode_workspace(max_batch, y->net_h, y->net_w);
}
int32_t yolo9_enqueue(void* s, int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) {
    auto* y = static_cast<Yolo9Layer*>(s);
    return trtx_yolov9_decode(reinterpret_cast<const float* const*>(inputs), batch, y->class_count, y->net_h, y->net_w, y->max_out, y->seg ? 1 : 0,
                              static_cast<float*>(outputs[0]), ws, trtx_yolov9_decode_workspace(batch, y->net_h, y->net_w), stream);
}
size_t yolo9_ser_size(void* s) { return static_cast<Yolo9Layer*>(s)->blob().size(); }
void yolo9_serialize(void* s, void* buf) {
    const auto b = static_cast<Yolo9Layer*>(s)->blob();
    memcpy(buf, b.data(), b.size());
}
int32_t yolo9_clone(void* s, trtx_plugin_vtbl* out) {
    yolo9_fill(out, new Yolo9Layer(*static_cast<Yolo9Layer*>(s)));
    return 0;
}
void yolo9_destroy(void* s) { delete static_cast<Yolo9Layer*>(s); }
void yolo9_fill(trtx_plugin_vtbl* v, Yolo9Layer* y) {
    v->self = y;
    v->get_nb_outputs = yolo_nb_outputs;
    v->get_output_dims = yolo9_output_dims;
    v->configure = yolo9_configure;
    v->initialize = no_initialize;
    v->terminate = yolo_terminate;
    v->workspace_size = yolo9_workspace;
    v->enqueue = yolo9_enqueue;
    v->serialization_size = yolo9_ser_size;
    v->serialize = yolo9_serialize;
    v->plugin_type = yolo_type;
    v->plugin_version = yolo_version;
    v->clone = yolo9_clone;
    v->destroy = yolo9_destroy;
}
int32_t yolo9_create(const trtx_plugin_field* f, trtx_plugin_vtbl* out) {
    if (!f[0].data || f[0].length != 5) return 1;
    const int* ni = static_cast<const int*>(f[0].data);
    if (ni[0] < 1 || ni[1] < 32 || ni[2] < 32 || ni[3] < 1) return 1;
    auto* y = new Yolo9Layer();
    y->class_count = ni[0];
    y->net_w = ni[1];
    y->net_h = ni[2];
    y->max_out = ni[3];
    y->seg = ni[4] != 0;
    yolo9_fill(out, y);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The YOLOv10 form of "YoloLayer_TRT"/"1" (yolov10/plugin/yololayer.{h,cu}; the same registered name once more): ONE creator field
// "combinedInfo" = int32[4 + n] {classes, W, H, maxOut, strides...} (yolov10/src/block.cpp:235-277, yololayer.cu:263-278) with n = 1..5,
// i.e. 5 to 9 ints, all >= 1; ten and more are YOLOv8's.  Blob in the reference's order (yololayer.cu:64-79): int classCount,
// threadCount (256), netW, netH, maxOut, nStrides, strides[n] = 24 + 4 n bytes.  One (4 + classes, cells) input per level; output
// 1 + maxOut * 6 floats (Detection = bbox[4], conf, class_id).
// The lengths 28, 32, 36, 40 and 44 belong to no other form: YOLOv8's 35 + 4 n and YOLOv5's 25 + 32 n are odd, YOLOv9's is 21, and the
// smallest YOLOv7 (24 + 32 n, n >= 1) and non-empty Darknet (20 + 32 n) blobs are 56 and 52 bytes, the empty Darknet one 20.
constexpr int kYolo10DetFloats = 6;
struct Yolo10Layer {
    int class_count = 80, thread_count = 256, net_w = 640, net_h = 640, max_out = 1000;
    std::vector<int> strides;

    std::vector<uint8_t> blob() const {
        std::vector<uint8_t> b;
        put(b, class_count);
        put(b, thread_count);
        put(b, net_w);
        put(b, net_h);
        put(b, max_out);
        put(b, (int)strides.size());
        for (int s : strides) put(b, s);
        return b;
    }
    // accepted by its exact length and a stride count that agrees with it only
    static Yolo10Layer* from_blob(const void* data, size_t len) {
        if (len < 28 || len > 44 || len % 4) return nullptr;
        const uint8_t* p = static_cast<const uint8_t*>(data);
        const uint8_t* end = p + len;
        auto* y = new Yolo10Layer();
        int ns = 0;
        bool ok = get(p, end, y->class_count) && get(p, end, y->thread_count) && get(p, end, y->net_w) && get(p, end, y->net_h) &&
                  get(p, end, y->max_out) && get(p, end, ns) && ns >= 1 && ns <= 5 && (size_t)(end - p) == (size_t)ns * sizeof(int);
        for (int i = 0; ok && i < ns; ++i) {
            int s = 0;
            ok = get(p, end, s) && s >= 1;
            y->strides.push_back(s);
        }
        if (!ok || y->class_count < 1 || y->net_w < 1 || y->net_h < 1 || y->max_out < 1) {
            delete y;
            return nullptr;
        }
        return y;
    }
};
void yolo10_fill(trtx_plugin_vtbl* v, Yolo10Layer* y);
int32_t yolo10_output_dims(void* s, int32_t, const trtx_dims*, int32_t, trtx_dims* out) {
    auto* y = static_cast<Yolo10Layer*>(s);
    out->nb = 3;  // Dims3(maxOut * sizeof(Detection) / 4 + 1, 1, 1), yololayer.cu:90-94
    out->d[0] = (int64_t)y->max_out * kYolo10DetFloats + 1;
    out->d[1] = 1;
    out->d[2] = 1;
    return 0;
}
int32_t yolo10_configure(void* s, const trtx_dims* in, int32_t nb_in, const trtx_dims*, int32_t, int32_t) {
    auto* y = static_cast<Yolo10Layer*>(s);
    if (nb_in != (int)y->strides.size()) return 1;
    for (int i = 0; i < nb_in; ++i) {
        const int64_t cells = (int64_t)(y->net_h / y->strides[i]) * (y->net_w / y->strides[i]);
        int64_t vol = 1;
        for (int k = 0; k < in[i].nb; ++k) vol *= in[i].d[k];
        if (cells < 1 || vol % (cells * (4 + y->class_count))) return 1;  // [batch][4 + classes][cells]
    }
    return 0;
}
size_t yolo10_workspace(void* s, int32_t max_batch) {
    auto* y = static_cast<Yolo10Layer*>(s);
    return trtx_yolo_decode_workspace(max_batch, y->net_h, y->net_w, y->strides.data(), (int)y->strides.size());
}
int32_t yolo10_enqueue(void* s, int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) {
    auto* y = static_cast<Yolo10Layer*>(s);
    const size_t ws_bytes = trtx_yolo_decode_workspace(batch, y->net_h, y->net_w, y->strides.data(), (int)y->strides.size());
    return trtx_yolov10_decode(reinterpret_cast<const float* const*>(inputs), (int)y->strides.size(), batch, y->class_count, y->net_h, y->net_w,
                               y->strides.data(), y->max_out, static_cast<float*>(outputs[0]), ws, ws_bytes, stream);
}
size_t yolo10_ser_size(void* s) { return static_cast<Yolo10Layer*>(s)->blob().size(); }
void yolo10_serialize(void* s, void* buf) {
    const auto b = static_cast<Yolo10Layer*>(s)->blob();
    memcpy(buf, b.data(), b.size());
}
int32_t yolo10_clone(void* s, trtx_plugin_vtbl* out) {
    yolo10_fill(out, new Yolo10Layer(*static_cast<Yolo10Layer*>(s)));
    return 0;
}
void yolo10_destroy(void* s) { delete static_cast<Yolo10Layer*>(s); }
void yolo10_fill(trtx_plugin_vtbl* v, Yolo10Layer* y) {
    v->self = y;
    v->get_nb_outputs = yolo_nb_outputs;
    v->get_output_dims = yolo10_output_dims;
    v->configure = yolo10_configure;
    v->initialize = no_initialize;
    v->terminate = yolo_terminate;
    v->workspace_size = yolo10_workspace;
    v->enqueue = yolo10_enqueue;
    v->serialization_size = yolo10_ser_size;
    v->serialize = yolo10_serialize;
    v->plugin_type = yolo_type;
    v->plugin_version = yolo_version;
    v->clone = yolo10_clone;
    v->destroy = yolo10_destroy;
}
// "combinedInfo" of 5 to 9 ints, all >= 1
int32_t yolo10_create(const trtx_plugin_field* f, trtx_plugin_vtbl* out) {
    if (!f[0].data || f[0].length < 5 || f[0].length > 9) return 1;
    const int* ci = static_cast<const int*>(f[0].data);
    for (int i = 0; i < f[0].length; ++i)
        if (ci[i] < 1) return 1;
    auto* y = new Yolo10Layer();
    y->class_count = ci[0];
    y->net_w = ci[1];
    y->net_h = ci[2];
    y->max_out = ci[3];
    y->strides.assign(ci + 4, ci + f[0].length);
    yolo10_fill(out, y);
    return 0;
}

// creator: one field "combinedInfo" = int32[9 + nStrides] (yolov8/src/block.cpp:267-293, yololayer.cu:339-360)
int32_t yolo_create(void*, const char*, const trtx_plugin_field* f, int32_t nb, trtx_plugin_vtbl* out) {
    // no fields at all: the Darknet form (yolov4/yololayer.cu:258-263 ignores its field collection, and the creator's own is empty)
    if (nb == 0) {
        auto* y = new AnchorLayer();
        y->form = FORM_DARKNET;
        y->max_out = kDarknetMaxOut;
        y->kernels.clear();
        anchor_fill(out, y);
        return 0;
    }
    // the anchor-based plugin shares the registered name: told apart by its two fields "netinfo" + "kernels"
    // (four netinfo ints: YOLOv7's, which has no is_segmentation; five and more: YOLOv5's; fewer are refused by either)
    if (nb == 2 && f && f[0].name && f[1].name && !strcmp(f[0].name, "netinfo") && !strcmp(f[1].name, "kernels"))
        return anchor_create(f, out);
    // ... and so does the YOLOv9 one: its single field is "netinfo"
    if (nb == 1 && f && f[0].name && !strcmp(f[0].name, "netinfo")) return yolo9_create(f, out);
    // "combinedInfo" of 5 to 9 ints is YOLOv10's (four ints + 1 to 5 strides); ten and more is YOLOv8's, fewer are refused
    if (nb == 1 && f && f[0].name && !strcmp(f[0].name, "combinedInfo") && f[0].length >= 5 && f[0].length <= 9) return yolo10_create(f, out);
    if (nb != 1 || !f || !f[0].name || strcmp(f[0].name, "combinedInfo") != 0 || f[0].length < 10) return 1;
    const int* ci = static_cast<const int*>(f[0].data);
    auto* y = new YoloLayer();
    y->class_count = ci[0];
    y->n_kpt = ci[1];
    y->kpt_conf = (float)ci[2];
    y->net_w = ci[3];
    y->net_h = ci[4];
    y->max_out = ci[5];
    y->seg = ci[6] != 0;
    y->pose = ci[7] != 0;
    y->obb = ci[8] != 0;
    y->strides.assign(ci + 9, ci + f[0].length);
    yolo_fill(out, y);
    return 0;
}
int32_t yolo_deserialize(void*, const char*, const void* data, size_t len, trtx_plugin_vtbl* out) {
    YoloLayer* y = YoloLayer::from_blob(data, len);
    if (y) {
        yolo_fill(out, y);
        return 0;
    }
    // not the YOLOv8 layout (both parsers check the exact length): the anchor-based blob
    AnchorLayer* y5 = AnchorLayer::from_blob(data, len, false);
    if (y5) {
        anchor_fill(out, y5);
        return 0;
    }
    // ... nor the anchor-based one: the YOLOv9 blob, 21 bytes
    Yolo9Layer* y9 = Yolo9Layer::from_blob(data, len);
    if (y9) {
        yolo9_fill(out, y9);
        return 0;
    }
    // ... and last the YOLOv7 blob, 24 + 32 n bytes: no earlier parser takes that length (35 + 4 n, 25 + 32 n, 21)
    AnchorLayer* y7 = AnchorLayer::from_blob(data, len, true);
    if (y7) {
        anchor_fill(out, y7);
        return 0;
    }
    // ... and the Darknet blob, 20 + 32 n bytes: even, so none of 35 + 4 n, 25 + 32 n and 21, and 4 short of YOLOv7's 24 + 32 n
    AnchorLayer* yd = AnchorLayer::from_darknet_blob(data, len);
    if (yd) {
        anchor_fill(out, yd);
        return 0;
    }
    // ... and the YOLOv10 blob, 24 + 4 n bytes with n = 1..5: a length no parser above accepts (see Yolo10Layer)
    Yolo10Layer* y10 = Yolo10Layer::from_blob(data, len);
    if (!y10) return 1;
    yolo10_fill(out, y10);
    return 0;
}
const char* yolo_creator_name(void*) { return "YoloLayer_TRT"; }
const char* yolo_creator_version(void*) { return "1"; }

// ------------------------------------------------------------------------------------------------
// "Decode_TRT"/"1" — retinaface/decode.{h,cu}.  The reference fixes INPUT_H/W at compile time and serializes
// nothing (decode.cu:19-26); here the network size is learnt in configurePlugin from the stride-8 input
// (32, H/8, W/8) and stored in the blob as two ints so 1280x1280 engines deserialize without recompiling
// (SURVEY.md Appendix A.9).  An empty blob means the reference's 480x640.
struct RetinaDecode {
    int net_h = 480, net_w = 640;
};
void rdec_fill(trtx_plugin_vtbl* v, RetinaDecode* d);
int32_t rdec_nb_outputs(void*) { return 1; }
int32_t rdec_output_dims(void*, int32_t, const trtx_dims* in, int32_t nb, trtx_dims* out) {
    if (nb != 3 || in[0].nb != 3) return 1;
    const int64_t h = in[0].d[1] * 8, w = in[0].d[2] * 8;
    out->nb = 3;  // Dims3(totalCount, 1, 1), decode.cu:33-42
    out->d[0] = (int64_t)trtx_retina_decode_output_floats((int)h, (int)w);
    out->d[1] = 1;
    out->d[2] = 1;
    return 0;
}
int32_t rdec_configure(void* s, const trtx_dims* in, int32_t nb_in, const trtx_dims*, int32_t, int32_t) {
    auto* d = static_cast<RetinaDecode*>(s);
    if (nb_in != 3) return 1;
    d->net_h = (int)in[0].d[1] * 8;
    d->net_w = (int)in[0].d[2] * 8;
    for (int l = 0; l < 3; ++l)
        if (in[l].nb != 3 || in[l].d[0] != 32 || in[l].d[1] != d->net_h / (8 << l) || in[l].d[2] != d->net_w / (8 << l)) return 1;
    return 0;
}
int32_t rdec_initialize(void*) { return 0; }
void rdec_terminate(void*) {}
size_t rdec_workspace(void* s, int32_t max_batch) {
    auto* d = static_cast<RetinaDecode*>(s);
    return trtx_retina_decode_workspace(max_batch, d->net_h, d->net_w);
}
int32_t rdec_enqueue(void* s, int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) {
    auto* d = static_cast<RetinaDecode*>(s);
    return trtx_retina_decode(reinterpret_cast<const float* const*>(inputs), batch, d->net_h, d->net_w,
                              static_cast<float*>(outputs[0]), ws, trtx_retina_decode_workspace(batch, d->net_h, d->net_w), stream);
}
size_t rdec_ser_size(void*) { return 2 * sizeof(int); }
void rdec_serialize(void* s, void* buf) {
    auto* d = static_cast<RetinaDecode*>(s);
    const int v[2] = {d->net_h, d->net_w};
    memcpy(buf, v, sizeof v);
}
const char* rdec_type(void*) { return "Decode_TRT"; }
const char* rdec_version(void*) { return "1"; }
int32_t rdec_clone(void* s, trtx_plugin_vtbl* out) {
    rdec_fill(out, new RetinaDecode(*static_cast<RetinaDecode*>(s)));
    return 0;
}
void rdec_destroy(void* s) { delete static_cast<RetinaDecode*>(s); }
void rdec_fill(trtx_plugin_vtbl* v, RetinaDecode* d) {
    v->self = d;
    v->get_nb_outputs = rdec_nb_outputs;
    v->get_output_dims = rdec_output_dims;
    v->configure = rdec_configure;
    v->initialize = rdec_initialize;
    v->terminate = rdec_terminate;
    v->workspace_size = rdec_workspace;
    v->enqueue = rdec_enqueue;
    v->serialization_size = rdec_ser_size;
    v->serialize = rdec_serialize;
    v->plugin_type = rdec_type;
    v->plugin_version = rdec_version;
    v->clone = rdec_clone;
    v->destroy = rdec_destroy;
}
int32_t rdec_create(void*, const char*, const trtx_plugin_field*, int32_t, trtx_plugin_vtbl* out) {  // empty field collection, retina_r50.cpp:204-206
    rdec_fill(out, new RetinaDecode());
    return 0;
}
int32_t rdec_deserialize(void*, const char*, const void* data, size_t len, trtx_plugin_vtbl* out) {
    auto* d = new RetinaDecode();
    if (len == 2 * sizeof(int)) {
        int v[2];
        memcpy(v, data, sizeof v);
        d->net_h = v[0];
        d->net_w = v[1];
    } else if (len != 0) {
        delete d;
        return 1;
    }
    rdec_fill(out, d);
    return 0;
}
const char* rdec_creator_name(void*) { return "Decode_TRT"; }
const char* rdec_creator_version(void*) { return "1"; }

// ------------------------------------------------------------------------------------------------------------------
// "Mish_TRT"/"1" - yolov4/mish.{h,cu} (the same plugin ships with yolov5-v1..v3 era samples and scaled-yolov4): one input of any CHW
// shape, output of the same shape, out = x * tanh(softplus(x)) with the reference's threshold-20 softplus (mish.cu:113-135).
// Blob = int input_size_ (elements per sample, mish.cu:18-32), learnt in getOutputDimensions (mish.cu:40-47).
// Inside an engine the lowering pass never calls enqueue: Conv -> Scale -> Mish_TRT becomes the convolution's epilogue.
struct Mish {
    int input_size = 0;
};
void mish_fill(trtx_plugin_vtbl* v, Mish* m);
int32_t mish_nb_outputs(void*) { return 1; }
int32_t mish_output_dims(void* s, int32_t idx, const trtx_dims* in, int32_t nb, trtx_dims* out) {
    if (nb != 1 || idx != 0 || in[0].nb < 1) return 1;
    int64_t n = 1;
    for (int k = 0; k < in[0].nb; ++k) n *= in[0].d[k];
    static_cast<Mish*>(s)->input_size = (int)n;
    *out = in[0];
    return 0;
}
int32_t mish_configure(void* s, const trtx_dims* in, int32_t nb_in, const trtx_dims*, int32_t, int32_t) {
    if (nb_in != 1) return 1;
    int64_t n = 1;
    for (int k = 0; k < in[0].nb; ++k) n *= in[0].d[k];
    static_cast<Mish*>(s)->input_size = (int)n;
    return 0;
}
int32_t mish_initialize(void*) { return 0; }
void mish_terminate(void*) {}
size_t mish_workspace(void*, int32_t) { return 0; }
int32_t mish_enqueue(void* s, int32_t batch, const void* const* inputs, void* const* outputs, void*, trtx_stream_t stream) {
    return trtx_mish(static_cast<const float*>(inputs[0]), static_cast<float*>(outputs[0]), (size_t)static_cast<Mish*>(s)->input_size * (size_t)batch,
                     stream);
}
size_t mish_ser_size(void*) { return sizeof(int); }
void mish_serialize(void* s, void* buf) { memcpy(buf, &static_cast<Mish*>(s)->input_size, sizeof(int)); }
const char* mish_type(void*) { return "Mish_TRT"; }
const char* mish_version(void*) { return "1"; }
int32_t mish_clone(void* s, trtx_plugin_vtbl* out) {
    mish_fill(out, new Mish(*static_cast<Mish*>(s)));
    return 0;
}
void mish_destroy(void* s) { delete static_cast<Mish*>(s); }
void mish_fill(trtx_plugin_vtbl* v, Mish* m) {
    v->self = m;
    v->get_nb_outputs = mish_nb_outputs;
    v->get_output_dims = mish_output_dims;
    v->configure = mish_configure;
    v->initialize = mish_initialize;
    v->terminate = mish_terminate;
    v->workspace_size = mish_workspace;
    v->enqueue = mish_enqueue;
    v->serialization_size = mish_ser_size;
    v->serialize = mish_serialize;
    v->plugin_type = mish_type;
    v->plugin_version = mish_version;
    v->clone = mish_clone;
    v->destroy = mish_destroy;
}
int32_t mish_create(void*, const char*, const trtx_plugin_field*, int32_t, trtx_plugin_vtbl* out) {  // empty field collection, mish.cu:166-178
    mish_fill(out, new Mish());
    return 0;
}
int32_t mish_deserialize(void*, const char*, const void* data, size_t len, trtx_plugin_vtbl* out) {  // mish.cu:18-22
    if (len != sizeof(int)) return 1;
    auto* m = new Mish();
    memcpy(&m->input_size, data, sizeof(int));
    mish_fill(out, m);
    return 0;
}
const char* mish_creator_name(void*) { return "Mish_TRT"; }
const char* mish_creator_version(void*) { return "1"; }

}  // namespace

bool builtin_is_mish(const trtx_plugin_vtbl& v) { return v.enqueue == mish_enqueue && v.self; }

bool builtin_yolo_params(const trtx_plugin_vtbl& v, YoloLayerParams* out) {
    if (v.enqueue != yolo_enqueue || !v.self) return false;
    const auto* y = static_cast<const YoloLayer*>(v.self);
    out->classes = y->class_count;
    out->net_w = y->net_w;
    out->net_h = y->net_h;
    out->max_out = y->max_out;
    out->strides = y->strides;
    out->det_only = !(y->seg || y->pose || y->obb);
    out->seg = y->seg;
    out->pose = y->pose;
    out->obb = y->obb;
    out->nk = y->n_kpt;
    out->kpt_conf = y->kpt_conf;
    return true;
}

static bool anchor_params(const trtx_plugin_vtbl& v, int form, Yolo5LayerParams* out) {
    if (v.enqueue != anchor_enqueue || !v.self) return false;
    const auto* y = static_cast<const AnchorLayer*>(v.self);
    if (y->form != form) return false;
    out->classes = y->class_count;
    out->net_w = y->net_w;
    out->net_h = y->net_h;
    out->max_out = y->max_out;
    out->seg = y->seg;
    out->grid_w.clear();
    out->grid_h.clear();
    out->anchors.clear();
    y->geometry(&out->grid_w, &out->grid_h, &out->anchors);
    return true;
}
bool builtin_yolo5_params(const trtx_plugin_vtbl& v, Yolo5LayerParams* out) { return anchor_params(v, FORM_V5, out); }
bool builtin_yolo7_params(const trtx_plugin_vtbl& v, Yolo5LayerParams* out) { return anchor_params(v, FORM_V7, out); }
// the Darknet form has them once it has seen its inputs (the layer's shape inference shows them to it): false before
bool builtin_darknet_params(const trtx_plugin_vtbl& v, Yolo5LayerParams* out) { return anchor_params(v, FORM_DARKNET, out) && !out->grid_w.empty(); }

bool builtin_yolo9_params(const trtx_plugin_vtbl& v, Yolo9LayerParams* out) {
    if (v.enqueue != yolo9_enqueue || !v.self) return false;
    const auto* y = static_cast<const Yolo9Layer*>(v.self);
    out->classes = y->class_count;
    out->net_w = y->net_w;
    out->net_h = y->net_h;
    out->max_out = y->max_out;
    out->seg = y->seg;
    return true;
}

bool builtin_yolo10_params(const trtx_plugin_vtbl& v, YoloLayerParams* out) {
    if (v.enqueue != yolo10_enqueue || !v.self) return false;
    const auto* y = static_cast<const Yolo10Layer*>(v.self);
    out->classes = y->class_count;
    out->net_w = y->net_w;
    out->net_h = y->net_h;
    out->max_out = y->max_out;
    out->strides = y->strides;
    out->det_only = true;
    out->seg = out->pose = out->obb = false;
    out->nk = 0;
    out->kpt_conf = 0.f;
    return true;
}

// built-in plugins only enqueue kernels and stream-ordered memsets on the caller's stream: safe inside a stream capture
bool builtin_plugin_capturable(const trtx_plugin_vtbl& v) {
    return v.enqueue == yolo_enqueue || v.enqueue == anchor_enqueue || v.enqueue == yolo9_enqueue || v.enqueue == yolo10_enqueue || v.enqueue == rdec_enqueue || v.enqueue == mish_enqueue;
}

void register_builtin_plugins(PluginRegistry& r) {
    trtx_creator_vtbl c{};
    c.plugin_name = yolo_creator_name;
    c.plugin_version = yolo_creator_version;
    c.create = yolo_create;
    c.deserialize = yolo_deserialize;
    r.add(c);
    trtx_creator_vtbl d{};
    d.plugin_name = rdec_creator_name;
    d.plugin_version = rdec_creator_version;
    d.create = rdec_create;
    d.deserialize = rdec_deserialize;
    r.add(d);
    trtx_creator_vtbl m{};
    m.plugin_name = mish_creator_name;
    m.plugin_version = mish_creator_version;
    m.create = mish_create;
    m.deserialize = mish_deserialize;
    r.add(m);
}

}  // namespace trtx
