// Built-in HIP plugins, registered under the names the reference host code asks the registry for.
//   "YoloLayer_TRT"/"1"  — six plugins of the reference share this name; kYoloForms below lists them: YOLOv8 / 11 / 12
//                          (yolov8/plugin/yololayer.{h,cu}), YOLOv5, YOLOv9, YOLOv7, Darknet (yolov3, yolov3-tiny, yolov4) and YOLOv10
//   "Decode_TRT"/"1"     — retinaface/decode.{h,cu}
//   "Mish_TRT"/"1"       — yolov4/mish.{h,cu}
// Each plugin is a small host state class; Builtin<T> exposes it through the C v-table of include/trtx_hip.h, and its enqueue calls the
// HIP operator entry points of section 1.  Serialization blobs keep the reference's field order so a plan round-trips byte for byte
// (SURVEY.md §8b).
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
// The v-table of a state class T, built from T's ordinary members:
//   int32_t output_dims(int32_t index, const trtx_dims* in, int32_t nb_in, trtx_dims* out)
//   int32_t configure(const trtx_dims* in, int32_t nb_in, int32_t max_batch)
//   int32_t initialize()                                  (BuiltinState's returns 0)
//   size_t workspace(int32_t max_batch) const
//   int32_t enqueue(int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) const
//   std::vector<uint8_t> blob() const
//   static constexpr const char* kType, the registered name (BuiltinState's version is "1")
// One output, nothing to terminate, serialization from blob(), clone by copy construction.
void builtin_terminate(void*) {}   // every built-in's terminate, and so the mark of one
struct BuiltinState {
    int32_t initialize() { return 0; }
    static constexpr const char* kVersion = "1";
};
void dims3(int64_t d0, trtx_dims* out) {   // Dims3(d0, 1, 1)
    out->nb = 3;
    out->d[0] = d0;
    out->d[1] = 1;
    out->d[2] = 1;
}
int det_floats(YoloForm form);   // floats per Detection record of a YoloLayer_TRT form (kYoloForms)
int64_t volume(const trtx_dims& d) {
    int64_t vol = 1;
    for (int k = 0; k < d.nb; ++k) vol *= d.d[k];
    return vol;
}

template <typename T>
struct Builtin {
    static T* self(void* s) { return static_cast<T*>(s); }
    static int32_t nb_outputs(void*) { return 1; }
    static int32_t output_dims(void* s, int32_t idx, const trtx_dims* in, int32_t nb_in, trtx_dims* out) { return self(s)->output_dims(idx, in, nb_in, out); }
    static int32_t configure(void* s, const trtx_dims* in, int32_t nb_in, const trtx_dims*, int32_t, int32_t max_batch) {
        return self(s)->configure(in, nb_in, max_batch);
    }
    static int32_t initialize(void* s) { return self(s)->initialize(); }
    static size_t workspace(void* s, int32_t max_batch) { return self(s)->workspace(max_batch); }
    static int32_t enqueue(void* s, int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) {
        return self(s)->enqueue(batch, inputs, outputs, ws, stream);
    }
    static size_t ser_size(void* s) { return self(s)->blob().size(); }
    static void serialize(void* s, void* buf) {
        const auto b = self(s)->blob();
        memcpy(buf, b.data(), b.size());
    }
    static const char* type(void*) { return T::kType; }
    static const char* version(void*) { return T::kVersion; }
    static int32_t clone(void* s, trtx_plugin_vtbl* out) { return give(new T(*self(s)), out); }
    static void destroy(void* s) { delete self(s); }

    // hands the instance `t` (or a parser's nullptr) to the v-table `out`: the creators' and deserializers' return value
    static int32_t give(T* t, trtx_plugin_vtbl* out) {
        if (!t) return 1;
        *out = trtx_plugin_vtbl{t,         nb_outputs, output_dims, configure, initialize, builtin_terminate, workspace,
                                enqueue,   ser_size,   serialize,   type,      version,    clone,     destroy};
        return 0;
    }
    // `v` was filled for T: its state, else null
    static T* of(const trtx_plugin_vtbl& v) { return v.enqueue == enqueue ? static_cast<T*>(v.self) : nullptr; }
};

// ------------------------------------------------------------------------------------------------
// YOLOv8 / 11 / 12 (yolov8/plugin/yololayer.{h,cu}; creator: yololayer.cu:320-369)
struct YoloLayer : BuiltinState {
    static constexpr const char* kType = "YoloLayer_TRT";
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
    // creator: one field "combinedInfo" = int32[9 + nStrides] (yolov8/src/block.cpp:267-293, yololayer.cu:339-360)
    static YoloLayer* create(const trtx_plugin_field* f) {
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
        return y;
    }

    int32_t output_dims(int32_t, const trtx_dims*, int32_t, trtx_dims* out) const {
        dims3((int64_t)max_out * det_floats(YOLO_V8) + 1, out);  // Dims3(total_size + 1, 1, 1), yololayer.cu:107-111
        return 0;
    }
    int32_t configure(const trtx_dims* in, int32_t nb_in, int32_t mb) {
        max_batch = mb;
        if (nb_in != (int)strides.size()) return 1;
        for (int i = 0; i < nb_in; ++i) {
            const int64_t cells = (int64_t)(net_h / strides[i]) * (net_w / strides[i]);
            const int info = 4 + class_count + (seg ? 32 : 0) + (pose ? n_kpt * 3 : 0) + (obb ? 1 : 0);
            if (volume(in[i]) != cells * info) return 1;  // [4 + classes (+32) (+3*nk) (+1), cells]
        }
        return 0;
    }
    int32_t initialize() { return (n_kpt < 0 || n_kpt > 17) ? 1 : 0; }  // Detection::keypoints holds kNumberOfPoints = 17 triples
    size_t workspace(int32_t batch) const { return trtx_yolo_decode_workspace(batch, net_h, net_w, strides.data(), (int)strides.size()); }
    int32_t enqueue(int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) const {
        return trtx_yolo_decode_ex(reinterpret_cast<const float* const*>(inputs), (int)strides.size(), batch, class_count, net_h, net_w, strides.data(),
                                   max_out, n_kpt, kpt_conf, seg, pose, obb, static_cast<float*>(outputs[0]), ws, workspace(batch), stream);
    }
    void params(YoloParams* out) const {
        *out = YoloParams{YOLO_V8, class_count, net_w, net_h, max_out, seg, pose, obb, n_kpt, kpt_conf, strides};
    }
};

// ------------------------------------------------------------------------------------------------
// The anchor-based forms, one state for the three:
//   YOLOv5 (yolov5/plugin/yololayer.{h,cu}): creator fields "netinfo" = int32[5] {classes, W, H, maxOut, isSeg} and "kernels" =
//     YoloKernel[n] {int width, height; float anchors[6]} (yolov5/src/model.cpp:246-275, yololayer.cu:250-266); blob int classCount,
//     threadCount, kernelCount, netW, netH, maxOut, bool isSeg, YoloKernel[n] (yololayer.cu:49-89); Detection records of 38 floats.
//   YOLOv7 (yolov7/plugin/yololayer.{h,cu}): the same without the segmentation flag and with records of 6 floats.  "netinfo" =
//     int32[4] {classes, W, H, maxOut} - exactly four, five and more are YOLOv5's - and "kernels" (yolov7/src/block.cpp:220-255); the
//     blob has no isSeg byte (yololayer.cu:40-78).
//   Darknet (yolov3, yolov3-tiny, yolov4 / yololayer.{h,cu}): the creator takes NO fields and the reference compiles classes, input size,
//     the YoloKernel table and maxOut = 1000 in (yolov4/yololayer.h:10-38, yololayer.cu:9-27, 258-263).  Here the plugin learns them from
//     its inputs (darknet_geometry below) when the layer is added and again in configurePlugin; records of 7 floats.  The blob is the
//     reference's - int classCount, threadCount, kernelCount, YoloKernel[n] (yololayer.cu:58-75) - plus int netW, netH behind it, as
//     Decode_TRT extends an empty blob; n = 0 for a plugin that has not seen its inputs.
struct AnchorKernel {
    int width, height;
    float anchors[6];
};
constexpr int kDarknetMaxOut = 1000;   // MAX_OUTPUT_BBOX_COUNT, yololayer.h:12 of all three
struct AnchorLayer;
bool darknet_geometry(const trtx_dims* in, int nb_in, AnchorLayer* y);
struct AnchorLayer : BuiltinState {
    static constexpr const char* kType = "YoloLayer_TRT";
    YoloForm form = YOLO_V5;   // never serialised, the blob's length tells
    int class_count = 80, thread_count = 256, net_w = 640, net_h = 640, max_out = 1000;
    bool seg = false;  // YOLOv5 only
    std::vector<AnchorKernel> kernels;

    std::vector<uint8_t> blob() const {
        std::vector<uint8_t> b;
        put(b, class_count);
        put(b, thread_count);
        put(b, (int)kernels.size());
        if (form == YOLO_DARKNET) {
            for (const auto& k : kernels) put(b, k);
            put(b, net_w);
            put(b, net_h);
            return b;
        }
        put(b, net_w);
        put(b, net_h);
        put(b, max_out);
        if (form == YOLO_V5) put(b, seg);
        for (const auto& k : kernels) put(b, k);
        return b;
    }
    // the Darknet blob: a kernelCount of 0 .. 8 that agrees with the length
    static AnchorLayer* from_darknet_blob(const void* data, size_t len) {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        const uint8_t* end = p + len;
        auto* y = new AnchorLayer();
        y->form = YOLO_DARKNET;
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
    // the YOLOv5 and YOLOv7 blobs: a kernelCount of 1 .. 8 that agrees with the length
    static AnchorLayer* from_blob(const void* data, size_t len, bool v7) {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        const uint8_t* end = p + len;
        auto* y = new AnchorLayer();
        y->form = v7 ? YOLO_V7 : YOLO_V5;
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
    static AnchorLayer* from_v5_blob(const void* data, size_t len) { return from_blob(data, len, false); }
    static AnchorLayer* from_v7_blob(const void* data, size_t len) { return from_blob(data, len, true); }
    // "netinfo" of exactly four ints, all >= 1: YOLOv7's; of five and more, taken as they come: YOLOv5's
    static AnchorLayer* create(const trtx_plugin_field* f) {
        if (!f[0].data || !f[1].data || f[0].length < 4 || f[1].length < 1 || f[1].length > 8) return nullptr;
        const bool v7 = f[0].length == 4;
        const int* ni = static_cast<const int*>(f[0].data);
        if (v7 && (ni[0] < 1 || ni[1] < 1 || ni[2] < 1 || ni[3] < 1)) return nullptr;
        auto* y = new AnchorLayer();
        y->form = v7 ? YOLO_V7 : YOLO_V5;
        y->class_count = ni[0];
        y->net_w = ni[1];
        y->net_h = ni[2];
        y->max_out = ni[3];
        y->seg = !v7 && ni[4] != 0;
        y->kernels.resize(f[1].length);  // the reference counts this field in YoloKernel elements (model.cpp:272-273, block.cpp:241-242)
        memcpy(y->kernels.data(), f[1].data, sizeof(AnchorKernel) * f[1].length);
        return y;
    }
    // no fields at all: the Darknet form (yolov4/yololayer.cu:258-263 ignores its field collection, and the creator's own is empty)
    static AnchorLayer* create_darknet(const trtx_plugin_field*) {
        auto* y = new AnchorLayer();
        y->form = YOLO_DARKNET;
        y->max_out = kDarknetMaxOut;
        return y;
    }

    void geometry(std::vector<int>* gw, std::vector<int>* gh, std::vector<float>* an) const {
        for (const auto& k : kernels) {
            gw->push_back(k.width);
            gh->push_back(k.height);
            an->insert(an->end(), k.anchors, k.anchors + 6);
        }
    }
    int32_t output_dims(int32_t, const trtx_dims* in, int32_t nb_in, trtx_dims* out) {
        if (form == YOLO_DARKNET && !darknet_geometry(in, nb_in, this)) return 1;
        // Dims3(maxOut * sizeof(Detection) / 4 + 1, 1, 1), yolov5 yololayer.cu:101-105, yolov7 yololayer.cu:90-94
        dims3((int64_t)max_out * det_floats(form) + 1, out);
        return 0;
    }
    int32_t configure(const trtx_dims* in, int32_t nb_in, int32_t) {
        if (form == YOLO_DARKNET) return darknet_geometry(in, nb_in, this) ? 0 : 1;
        if (nb_in != (int)kernels.size()) return 1;
        const int info = 5 + class_count + (seg ? 32 : 0);
        for (int i = 0; i < nb_in; ++i)
            if (volume(in[i]) != (int64_t)3 * info * kernels[i].width * kernels[i].height) return 1;
        return 0;
    }
    size_t workspace(int32_t batch) const {
        std::vector<int> gw, gh;
        std::vector<float> an;
        geometry(&gw, &gh, &an);
        return trtx_yolov5_decode_workspace(batch, gw.data(), gh.data(), (int)gw.size());   // the same for the three forms
    }
    int32_t enqueue(int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) const {
        std::vector<int> gw, gh;
        std::vector<float> an;
        geometry(&gw, &gh, &an);
        const size_t ws_bytes = trtx_yolov5_decode_workspace(batch, gw.data(), gh.data(), (int)gw.size());
        const auto* in = reinterpret_cast<const float* const*>(inputs);
        float* out = static_cast<float*>(outputs[0]);
        if (form == YOLO_DARKNET)
            return trtx_darknet_decode(in, (int)gw.size(), batch, class_count, net_h, net_w, gw.data(), gh.data(), an.data(), max_out, out, ws, ws_bytes,
                                       stream);
        if (form == YOLO_V7)
            return trtx_yolov7_decode(in, (int)gw.size(), batch, class_count, net_h, net_w, gw.data(), gh.data(), an.data(), max_out, out, ws, ws_bytes,
                                      stream);
        return trtx_yolov5_decode(in, (int)gw.size(), batch, class_count, net_h, net_w, gw.data(), gh.data(), an.data(), max_out, seg ? 1 : 0, out, ws,
                                  ws_bytes, stream);
    }
    // the Darknet form has its parameters once it has seen its inputs (the layer's shape inference shows them to it): false before
    bool params(YoloParams* out) const {
        *out = YoloParams{form, class_count, net_w, net_h, max_out, seg};
        geometry(&out->grid_w, &out->grid_h, &out->anchors);
        return form != YOLO_DARKNET || !kernels.empty();
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

// ------------------------------------------------------------------------------------------------
// YOLOv9 (yolov9/plugin/yololayer.{h,cu}): ONE creator field "netinfo" = int32[5] {classes, W, H, maxOut, isSeg} (yololayer.cu:220-232);
// blob int classCount, threadCount, netW, netH, maxOut, bool isSeg (yololayer.cu:36-60).  Three inputs on the strides 8 / 16 / 32 with
// grids H / s x W / s (:185-186), each (4 + classes (+ 32), cells); output 1 + maxOut * 38 floats.
struct Yolo9Layer : BuiltinState {
    static constexpr const char* kType = "YoloLayer_TRT";
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
    static Yolo9Layer* create(const trtx_plugin_field* f) {
        if (!f[0].data || f[0].length != 5) return nullptr;
        const int* ni = static_cast<const int*>(f[0].data);
        if (ni[0] < 1 || ni[1] < 32 || ni[2] < 32 || ni[3] < 1) return nullptr;
        auto* y = new Yolo9Layer();
        y->class_count = ni[0];
        y->net_w = ni[1];
        y->net_h = ni[2];
        y->max_out = ni[3];
        y->seg = ni[4] != 0;
        return y;
    }

    int32_t output_dims(int32_t, const trtx_dims*, int32_t, trtx_dims* out) const {
        dims3((int64_t)max_out * det_floats(YOLO_V9) + 1, out);  // Dims3(maxOut * sizeof(Detection) / 4 + 1, 1, 1), yololayer.cu:70-73
        return 0;
    }
    int32_t configure(const trtx_dims* in, int32_t nb_in, int32_t) const {
        if (nb_in != 3) return 1;
        const int info = 4 + class_count + (seg ? 32 : 0);
        for (int i = 0; i < nb_in; ++i)
            if (volume(in[i]) != (int64_t)info * (net_h / (8 << i)) * (net_w / (8 << i))) return 1;
        return 0;
    }
    size_t workspace(int32_t batch) const { return trtx_yolov9_decode_workspace(batch, net_h, net_w); }
    int32_t enqueue(int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) const {
        return trtx_yolov9_decode(reinterpret_cast<const float* const*>(inputs), batch, class_count, net_h, net_w, max_out, seg ? 1 : 0,
                                  static_cast<float*>(outputs[0]), ws, workspace(batch), stream);
    }
    void params(YoloParams* out) const { *out = YoloParams{YOLO_V9, class_count, net_w, net_h, max_out, seg}; }
};

// ------------------------------------------------------------------------------------------------
// YOLOv10 (yolov10/plugin/yololayer.{h,cu}): ONE creator field "combinedInfo" = int32[4 + n] {classes, W, H, maxOut, strides...}
// (yolov10/src/block.cpp:235-277, yololayer.cu:263-278) with n = 1..5, i.e. 5 to 9 ints, all >= 1; ten and more are YOLOv8's.  Blob in the
// reference's order (yololayer.cu:64-79): int classCount, threadCount (256), netW, netH, maxOut, nStrides, strides[n].  One
// (4 + classes, cells) input per level; output 1 + maxOut * 6 floats (Detection = bbox[4], conf, class_id).
struct Yolo10Layer : BuiltinState {
    static constexpr const char* kType = "YoloLayer_TRT";
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
    // a stride count of 1 .. 5 that agrees with the length
    static Yolo10Layer* from_blob(const void* data, size_t len) {
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
    static Yolo10Layer* create(const trtx_plugin_field* f) {
        if (!f[0].data) return nullptr;
        const int* ci = static_cast<const int*>(f[0].data);
        for (int i = 0; i < f[0].length; ++i)
            if (ci[i] < 1) return nullptr;
        auto* y = new Yolo10Layer();
        y->class_count = ci[0];
        y->net_w = ci[1];
        y->net_h = ci[2];
        y->max_out = ci[3];
        y->strides.assign(ci + 4, ci + f[0].length);
        return y;
    }

    int32_t output_dims(int32_t, const trtx_dims*, int32_t, trtx_dims* out) const {
        dims3((int64_t)max_out * det_floats(YOLO_V10) + 1, out);  // Dims3(maxOut * sizeof(Detection) / 4 + 1, 1, 1), yololayer.cu:90-94
        return 0;
    }
    int32_t configure(const trtx_dims* in, int32_t nb_in, int32_t) const {
        if (nb_in != (int)strides.size()) return 1;
        for (int i = 0; i < nb_in; ++i) {
            const int64_t cells = (int64_t)(net_h / strides[i]) * (net_w / strides[i]);
            if (cells < 1 || volume(in[i]) % (cells * (4 + class_count))) return 1;  // [batch][4 + classes][cells]
        }
        return 0;
    }
    size_t workspace(int32_t batch) const { return trtx_yolo_decode_workspace(batch, net_h, net_w, strides.data(), (int)strides.size()); }
    int32_t enqueue(int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) const {
        return trtx_yolov10_decode(reinterpret_cast<const float* const*>(inputs), (int)strides.size(), batch, class_count, net_h, net_w, strides.data(),
                                   max_out, static_cast<float*>(outputs[0]), ws, workspace(batch), stream);
    }
    void params(YoloParams* out) const {
        *out = YoloParams{YOLO_V10, class_count, net_w, net_h, max_out, false, false, false, 0, 0.f, strides};
    }
};

// ------------------------------------------------------------------------------------------------
// The forms of "YoloLayer_TRT"/"1", in YoloForm's order, which is the order yolo_deserialize probes them in.
//
// A plugin is CREATED as the form whose field set it is given: the number of fields, their names, and where two forms share the names,
// the length of the first field.  The field sets exclude each other.
//
// A blob is DESERIALIZED as the form whose length it has: form k owns the lengths base + per_level * n for n = n_min .. n_max, and no
// length belongs to two forms (the static_assert below enumerates them).  The blob carries no tag besides that; each parser then checks
// that the level count inside the blob agrees with the length, and its own bounds.
template <typename T, T* (*make)(const trtx_plugin_field*)>
int32_t create_as(const trtx_plugin_field* f, trtx_plugin_vtbl* out) { return Builtin<T>::give(make(f), out); }
template <typename T, T* (*parse)(const void*, size_t)>
int32_t parse_as(const void* data, size_t len, trtx_plugin_vtbl* out) { return Builtin<T>::give(parse(data, len), out); }

struct YoloFormDef {
    const char* name;
    int nb_fields;                    // creator: this many fields ...
    const char* field[2];             // ... of these names ...
    int len0_min, len0_max;           // ... the first of them with a length in this range
    int32_t (*create)(const trtx_plugin_field* f, trtx_plugin_vtbl* out);
    size_t base, per_level;           // blob: base + per_level * n bytes ...
    int n_min, n_max;                 // ... for n levels in this range
    int det_floats;                   // floats per Detection record: the output is 1 + max_out * det_floats floats
    int32_t (*parse)(const void* data, size_t len, trtx_plugin_vtbl* out);

    constexpr bool owns(size_t len) const {
        for (int n = n_min; n <= n_max; ++n)
            if (len == base + per_level * n) return true;
        return false;
    }
};
constexpr int kAnyLen = INT32_MAX;
constexpr YoloFormDef kYoloForms[YOLO_FORMS] = {
        {"v8", 1, {"combinedInfo", nullptr}, 10, kAnyLen, create_as<YoloLayer, YoloLayer::create>,  //
         35, 4, 0, 8, kYoloDetFloats, parse_as<YoloLayer, YoloLayer::from_blob>},
        {"v5", 2, {"netinfo", "kernels"}, 5, kAnyLen, create_as<AnchorLayer, AnchorLayer::create>,  //
         25, 32, 1, 8, 38, parse_as<AnchorLayer, AnchorLayer::from_v5_blob>},
        {"v9", 1, {"netinfo", nullptr}, 0, kAnyLen, create_as<Yolo9Layer, Yolo9Layer::create>,  //
         21, 0, 0, 0, 38, parse_as<Yolo9Layer, Yolo9Layer::from_blob>},
        {"v7", 2, {"netinfo", "kernels"}, 4, 4, create_as<AnchorLayer, AnchorLayer::create>,  //
         24, 32, 1, 8, 6, parse_as<AnchorLayer, AnchorLayer::from_v7_blob>},
        {"darknet", 0, {nullptr, nullptr}, 0, 0, create_as<AnchorLayer, AnchorLayer::create_darknet>,  //
         20, 32, 0, 8, 7, parse_as<AnchorLayer, AnchorLayer::from_darknet_blob>},
        {"v10", 1, {"combinedInfo", nullptr}, 5, 9, create_as<Yolo10Layer, Yolo10Layer::create>,  //
         24, 4, 1, 5, 6, parse_as<Yolo10Layer, Yolo10Layer::from_blob>},
};
constexpr bool yolo_blob_lengths_disjoint() {
    for (size_t len = 0; len <= 35 + 32 * 8; ++len) {   // beyond every form's longest blob
        int owners = 0;
        for (const YoloFormDef& f : kYoloForms) owners += f.owns(len) ? 1 : 0;
        if (owners > 1) return false;
    }
    return true;
}
static_assert(yolo_blob_lengths_disjoint(), "two forms of YoloLayer_TRT claim the same blob length");
int det_floats(YoloForm form) { return kYoloForms[form].det_floats; }

int32_t yolo_create(void*, const char*, const trtx_plugin_field* f, int32_t nb, trtx_plugin_vtbl* out) {
    for (const YoloFormDef& d : kYoloForms) {
        if (nb != d.nb_fields) continue;
        bool named = nb == 0 || f != nullptr;
        for (int k = 0; named && k < nb; ++k) named = f[k].name && !strcmp(f[k].name, d.field[k]);
        if (named && (nb == 0 || (f[0].length >= d.len0_min && f[0].length <= d.len0_max))) return d.create(f, out);
    }
    return 1;
}
int32_t yolo_deserialize(void*, const char*, const void* data, size_t len, trtx_plugin_vtbl* out) {
    for (const YoloFormDef& d : kYoloForms)
        if (d.owns(len) && d.parse(data, len, out) == 0) return 0;
    return 1;
}

// ------------------------------------------------------------------------------------------------
// "Decode_TRT"/"1" — retinaface/decode.{h,cu}.  The reference fixes INPUT_H/W at compile time and serializes
// nothing (decode.cu:19-26); here the network size is learnt in configurePlugin from the stride-8 input
// (32, H/8, W/8) and stored in the blob as two ints so 1280x1280 engines deserialize without recompiling
// (SURVEY.md Appendix A.9).  An empty blob means the reference's 480x640.
struct RetinaDecode : BuiltinState {
    static constexpr const char* kType = "Decode_TRT";
    int net_h = 480, net_w = 640;

    std::vector<uint8_t> blob() const {
        std::vector<uint8_t> b;
        put(b, net_h);
        put(b, net_w);
        return b;
    }
    int32_t output_dims(int32_t, const trtx_dims* in, int32_t nb, trtx_dims* out) const {
        if (nb != 3 || in[0].nb != 3) return 1;
        const int64_t h = in[0].d[1] * 8, w = in[0].d[2] * 8;
        dims3((int64_t)trtx_retina_decode_output_floats((int)h, (int)w), out);  // Dims3(totalCount, 1, 1), decode.cu:33-42
        return 0;
    }
    int32_t configure(const trtx_dims* in, int32_t nb_in, int32_t) {
        if (nb_in != 3) return 1;
        net_h = (int)in[0].d[1] * 8;
        net_w = (int)in[0].d[2] * 8;
        for (int l = 0; l < 3; ++l)
            if (in[l].nb != 3 || in[l].d[0] != 32 || in[l].d[1] != net_h / (8 << l) || in[l].d[2] != net_w / (8 << l)) return 1;
        return 0;
    }
    size_t workspace(int32_t batch) const { return trtx_retina_decode_workspace(batch, net_h, net_w); }
    int32_t enqueue(int32_t batch, const void* const* inputs, void* const* outputs, void* ws, trtx_stream_t stream) const {
        return trtx_retina_decode(reinterpret_cast<const float* const*>(inputs), batch, net_h, net_w, static_cast<float*>(outputs[0]), ws,
                                  workspace(batch), stream);
    }
};
int32_t rdec_create(void*, const char*, const trtx_plugin_field*, int32_t, trtx_plugin_vtbl* out) {  // empty field collection, retina_r50.cpp:204-206
    return Builtin<RetinaDecode>::give(new RetinaDecode(), out);
}
int32_t rdec_deserialize(void*, const char*, const void* data, size_t len, trtx_plugin_vtbl* out) {
    if (len != 0 && len != 2 * sizeof(int)) return 1;
    auto* d = new RetinaDecode();
    if (len) {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        get(p, p + len, d->net_h);
        get(p, p + len, d->net_w);
    }
    return Builtin<RetinaDecode>::give(d, out);
}

// ------------------------------------------------------------------------------------------------------------------
// "Mish_TRT"/"1" - yolov4/mish.{h,cu} (the same plugin ships with yolov5-v1..v3 era samples and scaled-yolov4): one input of any CHW
// shape, output of the same shape, out = x * tanh(softplus(x)) with the reference's threshold-20 softplus (mish.cu:113-135).
// Blob = int input_size_ (elements per sample, mish.cu:18-32), learnt in getOutputDimensions (mish.cu:40-47).
// Inside an engine the lowering pass never calls enqueue: Conv -> Scale -> Mish_TRT becomes the convolution's epilogue.
struct Mish : BuiltinState {
    static constexpr const char* kType = "Mish_TRT";
    int input_size = 0;

    std::vector<uint8_t> blob() const {
        std::vector<uint8_t> b;
        put(b, input_size);
        return b;
    }
    int32_t output_dims(int32_t idx, const trtx_dims* in, int32_t nb, trtx_dims* out) {
        if (nb != 1 || idx != 0 || in[0].nb < 1) return 1;
        input_size = (int)volume(in[0]);
        *out = in[0];
        return 0;
    }
    int32_t configure(const trtx_dims* in, int32_t nb_in, int32_t) {
        if (nb_in != 1) return 1;
        input_size = (int)volume(in[0]);
        return 0;
    }
    size_t workspace(int32_t) const { return 0; }
    int32_t enqueue(int32_t batch, const void* const* inputs, void* const* outputs, void*, trtx_stream_t stream) const {
        return trtx_mish(static_cast<const float*>(inputs[0]), static_cast<float*>(outputs[0]), (size_t)input_size * (size_t)batch, stream);
    }
};
int32_t mish_create(void*, const char*, const trtx_plugin_field*, int32_t, trtx_plugin_vtbl* out) {  // empty field collection, mish.cu:166-178
    return Builtin<Mish>::give(new Mish(), out);
}
int32_t mish_deserialize(void*, const char*, const void* data, size_t len, trtx_plugin_vtbl* out) {  // mish.cu:18-22
    if (len != sizeof(int)) return 1;
    auto* m = new Mish();
    memcpy(&m->input_size, data, sizeof(int));
    return Builtin<Mish>::give(m, out);
}

template <typename T>
void add_creator(PluginRegistry& r, decltype(trtx_creator_vtbl::create) create, decltype(trtx_creator_vtbl::deserialize) deserialize) {
    trtx_creator_vtbl c{};
    c.plugin_name = Builtin<T>::type;   // neither reads its argument: the creator's name and version are its plugins'
    c.plugin_version = Builtin<T>::version;
    c.create = create;
    c.deserialize = deserialize;
    r.add(c);
}

}  // namespace

bool builtin_is_mish(const trtx_plugin_vtbl& v) { return Builtin<Mish>::of(v) != nullptr; }

bool builtin_yolo_params(const trtx_plugin_vtbl& v, YoloParams* out) {
    if (const auto* y = Builtin<YoloLayer>::of(v)) return y->params(out), true;
    if (const auto* y = Builtin<AnchorLayer>::of(v)) return y->params(out);
    if (const auto* y = Builtin<Yolo9Layer>::of(v)) return y->params(out), true;
    if (const auto* y = Builtin<Yolo10Layer>::of(v)) return y->params(out), true;
    return false;
}

// built-in plugins only enqueue kernels and stream-ordered memsets on the caller's stream: safe inside a stream capture
bool builtin_plugin_capturable(const trtx_plugin_vtbl& v) {
    return v.terminate == builtin_terminate;
}

void register_builtin_plugins(PluginRegistry& r) {
    add_creator<YoloLayer>(r, yolo_create, yolo_deserialize);
    add_creator<RetinaDecode>(r, rdec_create, rdec_deserialize);
    add_creator<Mish>(r, mish_create, mish_deserialize);
}

}  // namespace trtx
