// Lowered execution plan: the network definition turned into a static schedule of fused HIP kernel
// launches over a static memory plan.  This is the MI355X-native replacement for what the reference
// hands to TensorRT's builder (IBuilder::buildSerializedNetwork, yolov8/src/model.cpp:327): layer
// fusion (Conv+BN+SiLU/ReLU+residual), layout selection (NHWC fp16 for image tensors, fp32 LINEAR for
// the reshaped heads and plugin edges), concat/slice elimination by channel-offset views, liveness-based
// buffer reuse, weight pre-packing.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../kernels/kernels.h"
#include "graph.h"
#include "plugin.h"

namespace trtx {

enum Layout : int { LAY_LINEAR = 0, LAY_NHWC = 1 };
enum StorageKind : int { ST_ARENA = 0, ST_WEIGHTS = 1, ST_BINDING = 2 };

enum OpKind : int {
    OP_CONV = 0,      // fused conv (+bias/BN, act1, residual, act2): igemm (MFMA) or direct
    OP_DECONV,
    OP_POOL,
    OP_RESIZE,
    OP_EW_NHWC,
    OP_ACT_NHWC,
    OP_SCALE_NHWC,
    OP_COPY_NHWC,
    OP_REDUCE_HW,
    OP_TO_NHWC,       // LINEAR fp32 -> NHWC
    OP_TO_LINEAR,     // NHWC -> LINEAR fp32
    OP_GATHER,        // LINEAR permute / slice / broadcast copy
    OP_SCATTER,       // LINEAR concat placement
    OP_EW_LIN,
    OP_ACT_LIN,
    OP_SCALE_LIN,
    OP_SOFTMAX,
    OP_MATMUL,
    OP_REDUCE_LIN,
    OP_PLUGIN,
    OP_COPY_LIN,      // dense copy (e.g. into an output binding)
    OP_YOLO_HEAD,     // fused DFL + YoloLayer decode on the NHWC head tensors
    OP_POOL_CHAIN,    // three chained k x k stride-1 'same' max-pools (SPPF) in one launch, three outputs
    OP_D2S,           // depth-to-space: [N,H,W,(r,q,c)] -> [N,H*bh,W*bw,c] (second half of a kernel == stride deconvolution)
    OP_ROI_ALIGN,     // detectron2 ROIAlign on the NHWC feature map, NHWC [P][res][res][C] out (fused form of the "RoiAlign" plugin)
    OP_RESERVED_47,   // (rounds 3-4: OP_CONV_CHAIN, the fused convolution chains - tools/hip/experiments/)
    OP_CONV_GROUP,    // 2..4 INDEPENDENT implicit-GEMM convolutions of one kernel instantiation in one launch (POp::group; round 4)
    OP_ATTENTION,     // YOLO11 PSA attention on the NHWC fp16 qkv tensor: O and the V image (kernels/attention.hip); i = heads, N, kd, hd, f[0] = scale;
                      // i[4] = 0.  With i[4] = area >= 1: YOLOv12 area attention on the same tensors (kernels/attention_mfma.hip), N / area keys per query
    OP_YOLO_TASK_HEAD,  // fused DFL + YoloLayer seg / pose / obb decode (explicit batch): `in` = NHWC heads, `extra_in` = NHWC task branches;
                        // i as OP_YOLO_HEAD with at most 4 strides in i[5..8], i[9] = 1 seg / 2 pose / 3 obb, i[10] = keypoints, f[0] = kpt_conf
    OP_YOLO5_HEAD,      // fused anchor-based YoloLayer decode (YOLOv5) on the detect convolutions' NHWC output (plugins/anchor_head.hip): i[0] = classes,
                        // i[1] / i[2] = net h / w, i[3] = max_out, i[4] = levels, i[11] as OP_YOLO_HEAD; iv = (grid_w, grid_h) per level, fv = 6 anchors per level
    OP_YOLO9_HEAD,      // fused DFL + YOLOv9 YoloLayer decode (38-float records) on the NHWC outputs of the head's last convolutions (plugins/yolo9_head.hip):
                        // `in` = the three box tensors (64 DFL bins), `extra_in` = the three class tensors; i[0] = classes, i[1] / i[2] = net h / w,
                        // i[3] = max_out, i[4] = levels (3: strides 8 / 16 / 32); src_layer = the DFL 1x1 convolution
    OP_YOLO7_HEAD,      // OP_YOLO5_HEAD with YOLOv7's 6-float records (plugins/anchor_head.hip): the same i / iv / fv
    OP_HGCONV,          // YOLOv13's adaptive hypergraph convolution (kernels/hgconv.hip) on the NHWC fp16 token image: i[0] = N, i[1] = D, i[2] = E,
                        // f[0] = the logit scale 1 / (heads * scaling); iv = the five network layers that hold the weights (context_net, the prototype
                        // constant, pre_head_proj, edge_proj, node_proj), packed at w_off as nine fp32 arrays in HgconvWeights' order; ws = its workspace
    OP_GATED_ADD,       // out = in[0] + gate (.) in[1] on NHWC tensors (nhwc_gated_add): src_layer = the constant layer that holds the gate (one value, or one per
                        // channel), packed at w_off as C fp32 values
    OP_ATTENTION_SPLIT, // YOLOv13 area attention (kernels/attention_mfma.hip, area_attention_split_f16): in[0] = the NHWC fp16 q | k tensor (head h's q at channel
                        // h*kd, its k at i[5] + h*kd), in[1] = the NHWC fp16 v tensor, out[0] = O; i = heads, N, kd, hd, area, the k channel offset; f[0] = scale
    OP_DARKNET_HEAD,    // OP_YOLO5_HEAD with the Darknet plugin's arithmetic and 7-float records (YOLOv3 / YOLOv3-tiny / YOLOv4; plugins/anchor_head.hip):
                        // the same i / iv / fv, levels in the plugin's input order
    OP_PAD_NHWC,        // IPaddingLayer, zero fill (nhwc_zero_pad): i[0] / i[1] = rows above / columns left of the image; the output tensor's H x W say the rest
    OP_YOLO10_HEAD,     // OP_YOLO_HEAD with YOLOv10's 6-float records and any class count >= 1 (plugins/yolo_decode.hip, trtx_yolov10_head_decode_nhwc): the
                        // same i, at most 5 strides in i[5..9]
};
const char* op_kind_name(int k);

// The fused detect heads: the op that stands in for one form of YoloLayer_TRT and the tail in front of it, and the YOLO11 task head.
// One row each (plan.cpp): what the emission, the engine and describe_json would otherwise choose by comparing kinds.
struct HeadOp {
    int kind;                     // OP_*
    const char* suffix;           // of the op's name, behind the plugin layer's
    int min_levels, max_levels;   // the i[4] the engine runs
    bool dfl;                     // carries the 16 DFL weights, packed from src_layer
    // the entry points, [1] for fp32 tensors, and the workspace size, of the kinds whose levels are told by strides (i[5..]) ...
    decltype(&trtx_yolo_head_decode_nhwc) stride_decode[2];
    decltype(&trtx_yolo_head_decode_workspace) stride_ws;
    // ... and of those told by grids and anchors (iv, fv); OP_YOLO_TASK_HEAD's and OP_YOLO9_HEAD's argument lists are their own
    decltype(&trtx_yolov5_head_decode_nhwc) anchor_decode[2];
    decltype(&trtx_yolov5_head_decode_workspace) anchor_ws;
};
const HeadOp* head_op(int kind);          // null for any other kind
const HeadOp& head_op_of(YoloForm form);  // the detection head of that form
inline bool is_fused_head(int kind) { return head_op(kind) != nullptr; }
inline bool head_has_dfl(int kind) { return is_fused_head(kind) && head_op(kind)->dfl; }

struct PTensor {
    int id = -1;
    int net_tensor = -1;
    std::string name;
    Dims dims;           // logical dims (implicit batch: per sample)
    bool batched = true; // carries the runtime batch as outermost dimension
    int layout = LAY_LINEAR;
    int dtype = DT_F32;
    int nfix = 0;        // NHWC with explicit batch: N taken from dims[0]; 0 = runtime batch
    int nmul = 1;        // NHWC with a leading per-sample dim (P,C,H,W): image count = batch * nmul
    int C = 0, H = 0, W = 0;
    bool pad_zeroed = false;  // channels [C, ld) of an owning NHWC tensor are guaranteed zero
    // storage
    int parent = -1;     // aliasing: this tensor lives inside `parent` ...
    int coff = 0;        // ... starting at this channel (NHWC) ...
    long eoff = 0;       // ... or element offset (LINEAR reshape/identity views)
    int ld = 0;          // resolved channel stride (NHWC)
    int storage = -1;    // resolved storage id
    int rcoff = 0;       // resolved channel offset within the storage
    long reoff = 0;      // resolved element offset within the storage (LINEAR)
    int Calloc = 0;      // owning NHWC tensor: allocated channel count
    float scale = 0.f;   // DT_I8 tensors: real value = int8 value * scale (the calibrated scale of the owning tensor)
    long sample_elems() const { return layout == LAY_NHWC ? (long)nmul * H * W * ld : (long)dims.volume(); }
};

struct Storage {
    int kind = ST_ARENA;
    size_t bytes = 0;      // total bytes at max batch
    size_t offset = 0;     // within the arena / weights blob
    int binding = -1;      // ST_BINDING
    int first_use = 1 << 30, last_use = -1;
};
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }   // every block of the arena and of the weight blob starts on 256 bytes

struct POp {
    int kind = 0;
    std::string name;
    std::vector<int> in, out;  // plan tensor ids
    std::vector<int> extra_in; // tensors read besides `in` (conv with a folded upsample: the half-resolution source); they count for
                               // dependencies and buffer lifetimes like `in`
    int dtype = DT_F32;
    // conv / deconv
    ConvArgs conv{};
    bool igemm = false;
    bool stem = false;         // conv_stem kernel: reads the LINEAR fp32 input directly
    bool stem_pair = false;    // the op right after the stem: the engine computes it straight from the network input in ONE launch with the stem
                               // (kernels/conv_stem_pair.hip); the stem op before it then launches nothing and the tensor between them stays unwritten
    bool bneck_pair = false;   // the second 3x3 convolution of a 16-channel bottleneck: the engine computes it in ONE launch with the convolution right before it
                               // (kernels/conv_bneck_pair.hip); that op then launches nothing and the tensor between them stays unwritten
    bool from_deconv = false;  // 1x1 conv standing in for a kernel == stride deconvolution (weights re-laid from CKRS)
    bool dw = false;           // depthwise kernel (kernels/conv_dw.hip; weights fp32 [kh*kw][C]) instead of the direct one
    bool grouped = false;      // grouped MFMA kernel (kernels/conv_grouped.hip; weights fp16 [group][Cout_g][Kpad]) instead of the direct one
    int fold_layer = -1, fold_scale = -1;   // >= 0: a 7x7 depthwise convolution that took RepVGGDW's 3x3 branch (match_repvggdw_fold): the network layers
                               // of that branch's convolution and scale; pack_weights adds its scaled filter into the centre and its shift to the shift
    int reorg_cin = 0;         // > 0: a convolution that absorbed the ReOrg in front of it (match_reorg_fold): conv is the 2k x 2k stride-2 form over this
                               // many channels and pack_weights re-indexes the layer's k x k filter over 4 x as many (reorg_fold_weights)
    int cout_real = 0;         // > 0: conv.Cout is this channel count rounded up to a 16-byte multiple; the filter rows and biases beyond it are zero
                               // and the output tensor's padding channels take the zeros (a detect convolution under OP_YOLO5_HEAD)
    // OP_CONV_GROUP: the member convolutions, each a complete OP_CONV record (its own in / out tensors, ConvArgs, weights); the group's
    // in / out are the unions, so dependencies, lanes and buffer lifetimes see one op
    std::vector<POp> group;
    bool sibling_pair = false; // OP_CONV_GROUP right behind another one whose members read the same tensors with the same geometry: the engine computes BOTH groups in
                               // ONE launch at this op (kernels/igemm_tile.h, the dual tile); the op before it then launches nothing
    int src_layer = -1;        // network layer holding the kernel weights
    int scale_layer = -1;      // folded IScaleLayer (BatchNorm) or -1
    size_t w_off = 0, b_off = 0, s_off = 0;  // byte offsets into the device weight blob
    // generic parameters
    int i[12] = {0};
    float f[4] = {0};
    std::vector<int> iv;       // per-level tables of ops that have them (OP_YOLO5_HEAD)
    std::vector<float> fv;
    StridedView view{};
    long off0 = 0;             // element offset applied to the strided side of a gather/scatter
    bool view_batched_in = false, view_batched_in2 = false, view_batched_out = true;
    std::shared_ptr<PluginHolder> plugin;
    size_t ws_off = 0, ws_bytes = 0;
    // concurrency: lane = HIP stream the op is issued on; before it, the lane waits for the events of wait_ops;
    // signal = some op on another lane waits for this one (an event is recorded after it)
    int lane = 0;
    std::vector<int> wait_ops;
    bool signal = false;
    double flops = 0;   // algorithmic FLOP per sample (2*MAC)
    double bytes = 0;   // algorithmic bytes per sample (activations in + out) + weights
};

struct Plan {
    bool explicit_batch = false;
    bool fp16 = false;
    int max_batch = 1;
    std::vector<PTensor> tensors;
    std::vector<Storage> storages;
    std::vector<POp> ops;
    std::vector<int> binding_tensor;      // binding index -> network tensor id (inputs first, then outputs)
    std::vector<int> binding_ptensor;     // binding index -> plan tensor id
    std::vector<bool> binding_is_input;
    int num_lanes = 1;
    size_t arena_bytes = 0;
    size_t weight_bytes = 0;
    std::vector<uint8_t> weight_blob;     // host image of the device weight blob (filled by pack_weights)
    std::string error;

    std::string describe_json() const;
};

// Lower a network into a plan (pure host work; no device needed).  Returns false and sets plan.error.
bool lower_network(const Network& net, Plan* plan);
// While > 0 on the calling thread, lower_network keeps every tensor of the definition that a kINT8 engine of it would keep: the passes
// that make a tensor disappear from an fp16 plan but not from the int8 plan (fold_upsample) are off.  Set by
// run_int8_calibration around the statistics engine: the observer sees a tensor only where an op writes it, and the upsampled slice of
// a concat buffer must reach that buffer's histogram (the int8 engine requantises the upsampled feature into the shared
// scale and would clip it if the scale came from the skip slice alone).
struct CalibrationLowering {
    CalibrationLowering();
    ~CalibrationLowering();
    static bool active();
};
// Fill plan.weight_blob (folded BN, packed fp16 igemm weights, biases, constants).
bool pack_weights(const Network& net, Plan* plan);

}  // namespace trtx
