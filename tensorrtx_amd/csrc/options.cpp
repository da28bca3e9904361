#include "options.h"

#include <stdlib.h>

namespace trtx {
namespace {
const char* env(const char* name) { return getenv(name); }   // the library's only getenv
int env_int(const char* name, int unset) {
    const char* v = env(name);
    return (v && *v) ? atoi(v) : unset;
}
bool env_is(const char* name, int value) {
    const char* v = env(name);
    return v && *v && atoi(v) == value;
}
bool env_set(const char* name) { return env(name) != nullptr; }
}  // namespace

Options read_options() {
    Options o;
    o.tune = env_int("TRTX_TUNE", -1);
    o.tune_verbose = env_set("TRTX_TUNE_VERBOSE");
    o.tune_margin = env_int("TRTX_TUNE_MARGIN", -1);
    if (const char* v = env("TRTX_TACTIC_CACHE")) o.tactic_cache = v;
    o.graph = env_is("TRTX_GRAPH", 1);
    if (const char* v = env("TRTX_CALIB_REPORT")) o.calib_report = v;
    if (const char* v = env("TRTX_INT8_CLIP_LIMIT"); v && *v) o.int8_clip_limit = atof(v);
    o.lanes = env_int("TRTX_LANES", 0);
    o.group_convs = !env_is("TRTX_GROUP_CONVS", 0);
    o.fold_upsample = !env_is("TRTX_FOLD_UPSAMPLE", 0);
    o.stem_pair = !env_is("TRTX_STEM_PAIR", 0);
    o.bneck_pair = !env_is("TRTX_BNECK_PAIR", 0);
    o.sibling_pair = !env_is("TRTX_SIBLING_PAIR", 0);
    o.ws = !env_set("TRTX_CONV_NOWS");
    o.wsk = !env_set("TRTX_CONV_NOWSK");
    o.gemm256 = !env_is("TRTX_GEMM256", 0);
    o.patch = !env_is("TRTX_CONV_PATCH", 0);
    o.res = env_int("TRTX_CONV_RES", 7);
    o.roles = !env_is("TRTX_CONV_ROLES", 0);
    o.f32_mfma = !env_set("TRTX_F32_DIRECT");
    o.conv_grouped = !env_is("TRTX_CONV_GROUPED", 0);
    o.area_attention = !env_is("TRTX_AREA_ATTENTION", 0);
    o.aattn_split = !env_is("TRTX_AATTN_SPLIT", 0);
    o.hgconv = !env_is("TRTX_HGCONV", 0);
    o.gated_add = !env_is("TRTX_GATED_ADD", 0);
    o.yolo5_head = !env_is("TRTX_YOLO5_HEAD", 0);
    o.yolo7_head = !env_is("TRTX_YOLO7_HEAD", 0);
    o.darknet_head = !env_is("TRTX_DARKNET_HEAD", 0);
    o.yolo10_head = !env_is("TRTX_YOLO10_HEAD", 0);
    o.repvggdw_fold = !env_is("TRTX_REPVGGDW_FOLD", 0);
    o.reorg_fold = !env_is("TRTX_REORG_FOLD", 0);
    o.spp_parallel_chain = !env_is("TRTX_SPP_PARALLEL_CHAIN", 0);
    o.yolo9_head = !env_is("TRTX_YOLO9_HEAD", 0);
    o.roialign_fused = !env_set("TRTX_ROIALIGN_PLUGIN");
    o.roialign_fold_stride = !env_is("TRTX_ROIALIGN_FOLD_STRIDE", 0);
    o.profile_kernel_events = !env_set("TRTX_PROFILE_NO_KERNEL_EVENTS");
    o.op_reps = env_int("TRTX_OP_REPS", 1);
    return o;
}

const Options& options() {
    static const Options o = read_options();
    return o;
}

}  // namespace trtx
