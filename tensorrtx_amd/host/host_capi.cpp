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

extern "C" int32_t trtx_host_build(const char* model, const char* wts_path, const char* options, void** blob, size_t* size) {
    if (!model || !wts_path || !blob || !size) return TRTX_ERR_INVALID;
    const auto o = parse_opts(options);
    trtx_host::Logger logger;
    std::unique_ptr<IBuilder> builder(createInferBuilder(logger));
    std::unique_ptr<IBuilderConfig> config(builder->createBuilderConfig());
    std::unique_ptr<IInt8Calibrator> calibrator;
    const bool yolov9 = trtx_host::yolov9_model_valid(model, false);   // yolov9t / s / m / c, gelanc
    if (yolov9 && geti(o, "int8", 0)) return TRTX_ERR_UNSUPPORTED;      // no INT8 YOLOv9 is built
    const bool yolov7 = trtx_host::yolov7_model_valid(model);          // yolov7tiny / yolov7 / yolov7x / yolov7w6 / yolov7e6
    if (yolov7 && geti(o, "int8", 0)) return TRTX_ERR_UNSUPPORTED;      // ... nor INT8 YOLOv7
    const bool darknet = trtx_host::darknet_model_valid(model);        // yolov3 / yolov3-tiny / yolov4
    if (darknet && geti(o, "int8", 0)) return TRTX_ERR_UNSUPPORTED;     // ... nor INT8 Darknet models
    const std::string m_in(model);
    const bool yolov10 = m_in.size() == 8 && m_in.compare(0, 7, "yolov10") == 0;   // yolov10n / s / m / b / l / x
    if (yolov10 && !trtx_host::yolov10_model_valid(m_in)) return TRTX_ERR_INVALID;   // another letter
    if (yolov10 && geti(o, "int8", 0)) return TRTX_ERR_UNSUPPORTED;    // ... nor INT8 YOLOv10: no calibration for this family
    if (geti(o, "int8", 0)) {  // USE_INT8 of the reference builders (yolov8/src/model.cpp:317-324, retinaface/retina_r50.cpp:219-225)
        if (!builder->platformHasFastInt8()) return TRTX_ERR_UNSUPPORTED;
        config->setFlag(BuilderFlag::kINT8);
        if (g_have_calib) {
            calibrator.reset(new trtx_host::CallbackCalibrator(g_calib));
        } else {
            const trtx_host::HostOptions ho = trtx_host::read_host_options(o);   // calibration directory / cache: option string, else environment (host/options.h)
            const std::string m0(model);
            calibrator.reset(new trtx_host::Int8EntropyCalibrator2(geti(o, "calib_batch", 1), geti(o, "w", 640), geti(o, "h", 640), ho.calib_dir.c_str(),
                                                                   ho.calib_table.c_str(), (m0 == "yolov8n" || m0.compare(0, 6, "yolo11") == 0 || m0.compare(0, 6, "yolo12") == 0) ? "images" : "data"));
        }
        config->setInt8Calibrator(calibrator.get());
    }
    if (o.count("aux_streams")) {
        const int aux = geti(o, "aux_streams", -1);
        if (aux < -1 || aux > 15) return TRTX_ERR_INVALID;  // the shim's setter is void (as TensorRT's): range-check here
        config->setMaxAuxStreams(aux);
    }
    std::unique_ptr<IHostMemory> plan;
    const std::string m(model);
    if (m == "lenet") {
        plan.reset(trtx_host::buildLenet(builder.get(), config.get(), wts_path, geti(o, "batch", 1)));
    } else if (m == "resnet50") {
        plan.reset(trtx_host::buildResnet50(builder.get(), config.get(), wts_path, geti(o, "batch", 1), geti(o, "fp16", 1) != 0,
                                            geti(o, "h", 224), geti(o, "w", 224)));
    } else if (m == "retinaface_r50") {
        plan.reset(trtx_host::buildRetinaFaceR50(builder.get(), config.get(), wts_path, geti(o, "batch", 1), geti(o, "fp16", 1) != 0,
                                                 geti(o, "h", 480), geti(o, "w", 640)));
    } else if (m == "yolov8n") {
        trtx_host::Yolov8Config cfg;
        cfg.max_batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 640);
        cfg.input_w = geti(o, "w", 640);
        cfg.num_class = geti(o, "classes", 80);
        cfg.max_out_bbox = geti(o, "max_out", 1000);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        cfg.task = geti(o, "task", 0);  // 0 det, 1 seg, 2 pose, 3 obb
        cfg.num_points = geti(o, "points", cfg.num_points);
        if (cfg.task < 0 || cfg.task > 3) return TRTX_ERR_INVALID;
        plan.reset(trtx_host::buildEngineYolov8Det(builder.get(), config.get(), wts_path, cfg));
    } else if (m.size() == 7 && m.compare(0, 6, "yolo11") == 0) {   // yolo11n / s / m / l / x
        trtx_host::Yolo11Config cfg;
        if (!trtx_host::yolo11_scale(m[6], &cfg)) return TRTX_ERR_INVALID;
        cfg.batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 640);
        cfg.input_w = geti(o, "w", 640);
        cfg.task = geti(o, "task", 0);  // 0 det, 1 seg, 2 pose, 3 obb, 4 cls
        if (cfg.task < 0 || cfg.task > 4 || cfg.batch < 1) return TRTX_ERR_INVALID;
        static const int kClasses[] = {80, 80, 1, 15, 1000};   // kNumClass, kPoseNumClass, kObbNumClass, kClsNumClass (yolo11/include/config.h)
        cfg.num_class = geti(o, "classes", kClasses[cfg.task]);
        cfg.max_out_bbox = geti(o, "max_out", 1000);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        cfg.num_points = geti(o, "points", cfg.num_points);
        plan.reset(trtx_host::buildEngineYolo11Det(builder.get(), config.get(), wts_path, cfg));
    } else if (m.size() == 7 && m.compare(0, 6, "yolo12") == 0) {   // yolo12n / s / m / l / x (detection only)
        trtx_host::Yolo12Config cfg;
        if (!trtx_host::yolo12_scale(m[6], &cfg)) return TRTX_ERR_INVALID;
        cfg.batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 640);
        cfg.input_w = geti(o, "w", 640);
        if (geti(o, "task", 0) != 0 || cfg.batch < 1) return TRTX_ERR_INVALID;
        cfg.num_class = geti(o, "classes", 80);
        cfg.max_out_bbox = geti(o, "max_out", 1000);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        plan.reset(trtx_host::buildEngineYolo12Det(builder.get(), config.get(), wts_path, cfg));
        if (!plan) return TRTX_ERR_INVALID;   // the stride-16 grid is not divisible by the attention's area count
    } else if ((m.size() == 7 || (m.size() == 8 && m[7] == '6')) && m.compare(0, 6, "yolov5") == 0) {   // yolov5n / s / m / l / x and the P6 models yolov5n6 ...
        trtx_host::Yolov5Config cfg;
        if (!trtx_host::yolov5_scale(m[6], &cfg)) return TRTX_ERR_INVALID;
        cfg.p6 = m.size() == 8;
        cfg.max_batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 640);
        cfg.input_w = geti(o, "w", 640);
        cfg.task = geti(o, "task", 0);  // 0 det, 1 seg, 4 cls (yolo11's numbers); P5 only, and no INT8, like the det builder
        if (!trtx_host::yolov5_task_valid(cfg.task, cfg.p6)) return TRTX_ERR_INVALID;
        if (cfg.task != 0 && geti(o, "int8", 0)) return TRTX_ERR_UNSUPPORTED;
        if (cfg.task == 4) {   // kClsInputH / kClsInputW / kClsNumClass (yolov5/src/config.h)
            cfg.input_h = geti(o, "h", 224);
            cfg.input_w = geti(o, "w", 224);
        }
        cfg.num_class = geti(o, "classes", cfg.task == 4 ? 1000 : 80);
        cfg.max_out_bbox = geti(o, "max_out", 1000);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        const int top = cfg.p6 ? 64 : 32;   // the largest stride: the down- and upsampled pyramid levels meet only on sizes it divides
        if (cfg.max_batch < 1 || cfg.num_class < 1 || cfg.max_out_bbox < 1 || cfg.input_h < top || cfg.input_w < top || cfg.input_h % top || cfg.input_w % top)
            return TRTX_ERR_INVALID;
        plan.reset(trtx_host::buildEngineYolov5(builder.get(), config.get(), wts_path, cfg));
    } else if (yolov9) {
        trtx_host::Yolov9Config cfg;
        cfg.model = m;
        cfg.max_batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 640);
        cfg.input_w = geti(o, "w", 640);
        cfg.num_class = geti(o, "classes", 80);
        cfg.max_out_bbox = geti(o, "max_out", 1000);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        cfg.converted = geti(o, "converted", 0) != 0;   // isConvert: t / s / m only
        if (geti(o, "task", 0) != 0 || !trtx_host::yolov9_model_valid(m, cfg.converted)) return TRTX_ERR_INVALID;
        // the three pyramid levels (strides 8 / 16 / 32) meet only on sizes that 32 divides
        if (cfg.max_batch < 1 || cfg.num_class < 1 || cfg.max_out_bbox < 1 || cfg.input_h < 32 || cfg.input_w < 32 || cfg.input_h % 32 || cfg.input_w % 32)
            return TRTX_ERR_INVALID;
        plan.reset(trtx_host::buildEngineYolov9(builder.get(), config.get(), wts_path, cfg));
    } else if (yolov7) {
        trtx_host::Yolov7Config cfg;
        cfg.model = m;
        cfg.max_batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 640);
        cfg.input_w = geti(o, "w", 640);
        cfg.num_class = geti(o, "classes", 80);
        cfg.max_out_bbox = geti(o, "max_out", 1000);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        if (geti(o, "task", 0) != 0) return TRTX_ERR_INVALID;
        const int top = trtx_host::yolov7_model_p6(m) ? 64 : 32;   // the largest stride: the pyramid levels meet only on sizes it divides
        if (cfg.max_batch < 1 || cfg.num_class < 1 || cfg.max_out_bbox < 1 || cfg.input_h < top || cfg.input_w < top || cfg.input_h % top || cfg.input_w % top)
            return TRTX_ERR_INVALID;
        plan.reset(trtx_host::buildEngineYolov7(builder.get(), config.get(), wts_path, cfg));
        if (!plan) return TRTX_ERR_INVALID;   // anchor_grid does not describe one level per detect convolution
    } else if (darknet) {
        trtx_host::DarknetConfig cfg;
        cfg.model = m;
        cfg.max_batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 608);
        cfg.input_w = geti(o, "w", 608);
        cfg.num_class = geti(o, "classes", 80);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        // MAX_OUTPUT_BBOX_COUNT is compiled into the reference's plugin (yololayer.h:12 of all three): 1000 and nothing else
        if (geti(o, "task", 0) != 0 || geti(o, "max_out", 1000) != 1000) return TRTX_ERR_INVALID;
        // the pyramid levels (strides 8 / 16 / 32, tiny 16 / 32) meet only on sizes that 32 divides
        if (cfg.max_batch < 1 || cfg.num_class < 1 || cfg.input_h < 32 || cfg.input_w < 32 || cfg.input_h % 32 || cfg.input_w % 32) return TRTX_ERR_INVALID;
        plan.reset(trtx_host::buildEngineDarknet(builder.get(), config.get(), wts_path, cfg));
    } else if (yolov10) {
        trtx_host::Yolov10Config cfg;
        cfg.model = m;
        cfg.max_batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", 640);
        cfg.input_w = geti(o, "w", 640);
        cfg.num_class = geti(o, "classes", 80);
        cfg.max_out_bbox = geti(o, "max_out", 1000);
        cfg.mark_heads = geti(o, "mark_heads", 0) != 0;
        // the three pyramid levels (strides 8 / 16 / 32) meet only on sizes that 32 divides
        if (geti(o, "task", 0) != 0 || cfg.max_batch < 1 || cfg.num_class < 1 || cfg.max_out_bbox < 1 || cfg.input_h < 32 || cfg.input_w < 32 ||
            cfg.input_h % 32 || cfg.input_w % 32)
            return TRTX_ERR_INVALID;
        plan.reset(trtx_host::buildEngineYolov10(builder.get(), config.get(), wts_path, cfg));
    } else if (m == "rcnn_r50c4") {
        trtx_host::RcnnConfig cfg;
        cfg.max_batch = geti(o, "batch", 1);
        cfg.fp16 = geti(o, "fp16", 1) != 0;
        cfg.input_h = geti(o, "h", cfg.input_h);
        cfg.input_w = geti(o, "w", cfg.input_w);
        cfg.num_classes = geti(o, "classes", cfg.num_classes);
        cfg.pre_nms_topk = geti(o, "pre_nms_topk", cfg.pre_nms_topk);
        cfg.post_nms_topk = geti(o, "post_nms_topk", cfg.post_nms_topk);
        cfg.detections_per_image = geti(o, "detections", cfg.detections_per_image);
        cfg.nms_method = geti(o, "nms_method", cfg.nms_method);
        cfg.mark_stages = geti(o, "mark_stages", 0) != 0;
        cfg.mask_on = geti(o, "mask", 0) != 0;
        plan.reset(trtx_host::buildRcnnR50C4(builder.get(), config.get(), wts_path, cfg));
    } else {
        return TRTX_ERR_INVALID;
    }
    if (!plan) return TRTX_ERR_UNSUPPORTED;
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
