// extern "C" doorway so tests/bench (ctypes) can drive the C++ host builders.  `options` is a flat
// "key=value;key=value" string.  Returns a malloc'd copy of the serialized plan.
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <sstream>

#include "calibrator.h"
#include "common.h"
#include "models.h"
#include "options.h"

using namespace nvinfer1;

static std::map<std::string, std::string> parse_opts(const char* s) {
    std::map<std::string, std::string> m;
    std::stringstream ss(s ? s : "");
    std::string kv;
    while (std::getline(ss, kv, ';')) {
        const auto eq = kv.find('=');
        if (eq != std::string::npos) m[kv.substr(0, eq)] = kv.substr(eq + 1);
    }
    return m;
}
static int geti(const std::map<std::string, std::string>& m, const char* k, int d) {
    auto it = m.find(k);
    return it == m.end() ? d : std::atoi(it->second.c_str());
}

// calibrator used by builds with int8=1: a C v-table supplied by the caller (tests / Python tools), or, when none is set,
// the reference-style directory calibrator over the calibration directory (*.ppm) and cache file of host/options.h (calib_dir= / calib_table= or the environment)
static trtx_calibrator_vtbl g_calib{};
static bool g_have_calib = false;
extern "C" void trtx_host_set_calibrator(const trtx_calibrator_vtbl* v) {
    g_have_calib = v != nullptr;
    if (v) g_calib = *v;
}

// ---- the family table: what trtx_host_build knows of a model name --------------------------------------------------------------------
namespace {
using Options = std::map<std::string, std::string>;
using trtx_host::YoloConfig;
struct Common : YoloConfig { int task = 0; };   // the options every family reads, parsed once
enum Checks { NONE, BATCH, ALL };   // which of batch / classes / max_out must be at least 1: none, the batch, all three
constexpr unsigned DET = 1u << 0, SEG = 1u << 1, POSE = 1u << 2, OBB = 1u << 3, CLS = 1u << 4, ANY = ~0u;   // ANY: the family has no tasks

struct Call {   // what a family's build function gets
    IBuilder* b; IBuilderConfig* bc; const char* wts;
    const std::string& m; const Common& c; const Options& o;   // the model name, the common options, all options
    int32_t* status;                                           // a refusal of the build function's own goes here
};
struct Family {
    bool (*match)(const std::string& m);   // the names of the family
    bool (*valid)(const std::string& m);   // null, or: which matching names exist; the others are INVALID before int8 is looked at
    unsigned int8_tasks;                   // the tasks an INT8 engine is built for; 0: int8=1 is UNSUPPORTED whatever else is asked
    int h, w;                              // default size
    bool task_classes;                     // classes default to kTaskClasses[task], else to 80
    int cls_size;                          // nonzero: task 4 defaults to this size (kClsInputH / kClsInputW, yolov5/src/config.h)
    int top;                               // the largest stride: h and w must be multiples of it (the pyramid levels meet only there); 0: any size
    unsigned tasks;                        // accepted tasks
    Checks checks;
    const char* calib_blob;                // the input blob the directory calibrator feeds
    int32_t null_status;                   // what a null plan means
    IHostMemory* (*build)(const Call& k);  // fills the family's own fields and builds
};

// kNumClass, kNumClass, kPoseNumClass, kObbNumClass, kClsNumClass (yolo11/include/config.h; yolov5/src/config.h for det / seg / cls)
const int kTaskClasses[] = {80, 80, 1, 15, 1000};
template <class Cfg> Cfg with(const Common& c) {
    Cfg cfg;
    static_cast<YoloConfig&>(cfg) = c;
    return cfg;
}
// <prefix><n | s | m | l | x><tail>
bool scaled(const std::string& m, const char* prefix, const char* tail = "") { return m.size() == 7 + strlen(tail) && m.compare(0, 6, prefix) == 0 && strchr("nsmlx", m[6]) && m.compare(7, 8, tail) == 0; }

IHostMemory* build_yolov5(const Call& k) {
    auto cfg = with<trtx_host::Yolov5Config>(k.c);
    trtx_host::yolov5_scale(k.m[6], &cfg);
    cfg.p6 = k.m.size() == 8;
    cfg.task = k.c.task;
    return trtx_host::buildEngineYolov5(k.b, k.bc, k.wts, cfg);
}
IHostMemory* build_yolov7(const Call& k) {
    auto cfg = with<trtx_host::Yolov7Config>(k.c);
    cfg.model = k.m;
    return trtx_host::buildEngineYolov7(k.b, k.bc, k.wts, cfg);
}

// match, valid, int8_tasks, h, w, task_classes, cls_size, top, tasks, checks, calib_blob, null_status, build
#define BUILD [](const Call& k) -> IHostMemory*
const Family kFamilies[] = {
    {[](const std::string& m) { return m == "lenet"; }, nullptr, ANY, 32, 32, false, 0, 0, ANY, NONE, "data", TRTX_ERR_UNSUPPORTED,
     BUILD { return trtx_host::buildLenet(k.b, k.bc, k.wts, k.c.batch); }},
    {[](const std::string& m) { return m == "resnet50"; }, nullptr, ANY, 224, 224, false, 0, 0, ANY, NONE, "data", TRTX_ERR_UNSUPPORTED,
     BUILD { return trtx_host::buildResnet50(k.b, k.bc, k.wts, k.c.batch, k.c.fp16, k.c.input_h, k.c.input_w); }},
    {[](const std::string& m) { return m == "retinaface_r50"; }, nullptr, ANY, 480, 640, false, 0, 0, ANY, NONE, "data", TRTX_ERR_UNSUPPORTED,
     BUILD { return trtx_host::buildRetinaFaceR50(k.b, k.bc, k.wts, k.c.batch, k.c.fp16, k.c.input_h, k.c.input_w); }},
    {[](const std::string& m) { return m == "yolov8n"; }, nullptr, ANY, 640, 640, false, 0, 0, DET | SEG | POSE | OBB, NONE, "images", TRTX_ERR_UNSUPPORTED,
     BUILD {
         auto cfg = with<trtx_host::Yolov8Config>(k.c);
         cfg.task = k.c.task;
         cfg.num_points = geti(k.o, "points", cfg.num_points);
         return trtx_host::buildEngineYolov8Det(k.b, k.bc, k.wts, cfg);
     }},
    {[](const std::string& m) { return scaled(m, "yolo11"); }, nullptr, ANY, 640, 640, true, 0, 0, DET | SEG | POSE | OBB | CLS, BATCH, "images", TRTX_ERR_UNSUPPORTED,
     BUILD {
         auto cfg = with<trtx_host::Yolo11Config>(k.c);
         trtx_host::yolo11_scale(k.m[6], &cfg);
         cfg.task = k.c.task;
         cfg.num_points = geti(k.o, "points", cfg.num_points);
         return trtx_host::buildEngineYolo11Det(k.b, k.bc, k.wts, cfg);
     }},
    // null: the stride-16 grid is not divisible by the attention's area count
    {[](const std::string& m) { return scaled(m, "yolo12"); }, nullptr, ANY, 640, 640, false, 0, 0, DET, BATCH, "images", TRTX_ERR_INVALID,
     BUILD {
         auto cfg = with<trtx_host::Yolo12Config>(k.c);
         trtx_host::yolo11_scale(k.m[6], &cfg);
         return trtx_host::buildEngineYolo12Det(k.b, k.bc, k.wts, cfg);
     }},
    // yolov5n / s / m / l / x: det, seg and cls (kClsInputH / kClsInputW 224), INT8 for det alone; and the P6 models yolov5n6 ...: det
    {[](const std::string& m) { return scaled(m, "yolov5"); }, nullptr, DET, 640, 640, true, 224, 32, DET | SEG | CLS, ALL, "data", TRTX_ERR_UNSUPPORTED, build_yolov5},
    {[](const std::string& m) { return scaled(m, "yolov5", "6"); }, nullptr, DET, 640, 640, true, 224, 64, DET, ALL, "data", TRTX_ERR_UNSUPPORTED, build_yolov5},
    {[](const std::string& m) { return trtx_host::yolov9_model_valid(m, false); }, nullptr, 0, 640, 640, false, 0, 32, DET, ALL, "data", TRTX_ERR_UNSUPPORTED,
     BUILD {
         auto cfg = with<trtx_host::Yolov9Config>(k.c);
         cfg.model = k.m;
         cfg.converted = geti(k.o, "converted", 0) != 0;   // isConvert: t / s / m only
         if (!trtx_host::yolov9_model_valid(k.m, cfg.converted)) return *k.status = TRTX_ERR_INVALID, nullptr;
         return trtx_host::buildEngineYolov9(k.b, k.bc, k.wts, cfg);
     }},
    // yolov7tiny / yolov7 / yolov7x, and the four-level yolov7w6 / yolov7e6; null: anchor_grid does not describe one level per detect convolution
    {[](const std::string& m) { return trtx_host::yolov7_model_valid(m) && !trtx_host::yolov7_model_p6(m); }, nullptr, 0, 640, 640, false, 0, 32, DET, ALL, "data", TRTX_ERR_INVALID, build_yolov7},
    {trtx_host::yolov7_model_p6, nullptr, 0, 640, 640, false, 0, 64, DET, ALL, "data", TRTX_ERR_INVALID, build_yolov7},
    {trtx_host::darknet_model_valid, nullptr, 0, 608, 608, false, 0, 32, DET, ALL, "data", TRTX_ERR_UNSUPPORTED,   // yolov3 / yolov3-tiny / yolov4
     BUILD {
         // MAX_OUTPUT_BBOX_COUNT is compiled into the reference's plugin (yololayer.h:12 of all three): 1000 and nothing else
         if (k.c.max_out_bbox != 1000) return *k.status = TRTX_ERR_INVALID, nullptr;
         auto cfg = with<trtx_host::DarknetConfig>(k.c);
         cfg.model = k.m;
         return trtx_host::buildEngineDarknet(k.b, k.bc, k.wts, cfg);
     }},
    {[](const std::string& m) { return m.size() == 8 && m.compare(0, 7, "yolov10") == 0; }, trtx_host::yolov10_model_valid, 0, 640, 640, false, 0, 32, DET, ALL,
     "data", TRTX_ERR_UNSUPPORTED,
     BUILD {
         auto cfg = with<trtx_host::Yolov10Config>(k.c);
         cfg.model = k.m;
         return trtx_host::buildEngineYolov10(k.b, k.bc, k.wts, cfg);
     }},
    {[](const std::string& m) { return m == "rcnn_r50c4"; }, nullptr, ANY, 800, 1067, false, 0, 0, ANY, NONE, "data", TRTX_ERR_UNSUPPORTED,
     BUILD {
         trtx_host::RcnnConfig cfg;
         cfg.max_batch = k.c.batch;
         cfg.fp16 = k.c.fp16;
         cfg.input_h = k.c.input_h;
         cfg.input_w = k.c.input_w;
         cfg.num_classes = k.c.num_class;
         cfg.pre_nms_topk = geti(k.o, "pre_nms_topk", cfg.pre_nms_topk);
         cfg.post_nms_topk = geti(k.o, "post_nms_topk", cfg.post_nms_topk);
         cfg.detections_per_image = geti(k.o, "detections", cfg.detections_per_image);
         cfg.nms_method = geti(k.o, "nms_method", cfg.nms_method);
         cfg.mark_stages = geti(k.o, "mark_stages", 0) != 0;
         cfg.mask_on = geti(k.o, "mask", 0) != 0;
         return trtx_host::buildRcnnR50C4(k.b, k.bc, k.wts, cfg);
     }},
};
#undef BUILD

}  // namespace

// The order of the refusals is part of the interface (tests/host_plan_cases.py): a name with an unknown variant letter is INVALID before
// int8 is looked at; int8=1 on a family that has no INT8 at all is UNSUPPORTED before any size or task is; then aux_streams, the task,
// int8 on a task without it, and the sizes.
extern "C" int32_t trtx_host_build(const char* model, const char* wts_path, const char* options, void** blob, size_t* size) {
    if (!model || !wts_path || !blob || !size) return TRTX_ERR_INVALID;
    const auto o = parse_opts(options);
    const std::string m(model);
    const Family* f = nullptr;
    for (const Family& row : kFamilies)
        if (!f && row.match(m)) f = &row;
    const bool int8 = geti(o, "int8", 0) != 0;
    if (f && f->valid && !f->valid(m)) return TRTX_ERR_INVALID;
    if (f && int8 && !f->int8_tasks) return TRTX_ERR_UNSUPPORTED;
    trtx_host::Logger logger;
    std::unique_ptr<IBuilder> builder(createInferBuilder(logger));
    std::unique_ptr<IBuilderConfig> config(builder->createBuilderConfig());
    std::unique_ptr<IInt8Calibrator> calibrator;
    if (int8) {  // USE_INT8 of the reference builders (yolov8/src/model.cpp:317-324, retinaface/retina_r50.cpp:219-225)
        if (!builder->platformHasFastInt8()) return TRTX_ERR_UNSUPPORTED;
        config->setFlag(BuilderFlag::kINT8);
        if (g_have_calib) {
            calibrator.reset(new trtx_host::CallbackCalibrator(g_calib));
        } else {
            const trtx_host::HostOptions ho = trtx_host::read_host_options(o);   // calibration directory / cache: option string, else environment (host/options.h)
            calibrator.reset(new trtx_host::Int8EntropyCalibrator2(geti(o, "calib_batch", 1), geti(o, "w", 640), geti(o, "h", 640), ho.calib_dir.c_str(),
                                                                   ho.calib_table.c_str(), f ? f->calib_blob : "data"));
        }
        config->setInt8Calibrator(calibrator.get());
    }
    if (o.count("aux_streams")) {
        const int aux = geti(o, "aux_streams", -1);
        if (aux < -1 || aux > 15) return TRTX_ERR_INVALID;  // the shim's setter is void (as TensorRT's): range-check here
        config->setMaxAuxStreams(aux);
    }
    if (!f) return TRTX_ERR_INVALID;

    Common c;
    c.task = geti(o, "task", 0);   // 0 det, 1 seg, 2 pose, 3 obb, 4 cls
    if (f->tasks != ANY && (c.task < 0 || c.task > 4 || !(f->tasks >> c.task & 1))) return TRTX_ERR_INVALID;
    if (int8 && f->int8_tasks != ANY && !(f->int8_tasks >> c.task & 1)) return TRTX_ERR_UNSUPPORTED;
    const bool cls = c.task == 4 && f->cls_size;   // the classifier's own default size
    c.batch = geti(o, "batch", 1);
    c.fp16 = geti(o, "fp16", 1) != 0;
    c.input_h = geti(o, "h", cls ? f->cls_size : f->h);
    c.input_w = geti(o, "w", cls ? f->cls_size : f->w);
    c.num_class = geti(o, "classes", f->task_classes ? kTaskClasses[c.task] : 80);
    c.max_out_bbox = geti(o, "max_out", 1000);
    c.mark_heads = geti(o, "mark_heads", 0) != 0;
    if (f->checks != NONE && c.batch < 1) return TRTX_ERR_INVALID;
    if (f->checks == ALL && (c.num_class < 1 || c.max_out_bbox < 1)) return TRTX_ERR_INVALID;
    if (f->top && (c.input_h < f->top || c.input_w < f->top || c.input_h % f->top || c.input_w % f->top)) return TRTX_ERR_INVALID;

    int32_t status = f->null_status;
    std::unique_ptr<IHostMemory> plan(f->build(Call{builder.get(), config.get(), wts_path, m, c, o, &status}));
    if (!plan) return status;
    *size = plan->size();
    *blob = std::malloc(*size);
    std::memcpy(*blob, plan->data(), *size);
    return TRTX_OK;
}

extern "C" void trtx_host_free(void* blob) { std::free(blob); }

// the module table of a Darknet model as JSON (the tests compare the builder's own table with theirs); null for another name.
// The string is malloc'd: the caller releases it with trtx_host_free.
extern "C" char* trtx_host_darknet_rows(const char* model) {
    const std::string s = model ? trtx_host::darknet_rows_json(model) : "";
    if (s.empty()) return nullptr;
    char* out = static_cast<char*>(std::malloc(s.size() + 1));
    if (out) std::memcpy(out, s.c_str(), s.size() + 1);
    return out;
}
