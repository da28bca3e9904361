// Graph pattern matching for the lowering (internal to runtime/): which layers of a Network collapse into one fused plan op.
// A matcher reads the network through a NetView and claims layers in Fusions::absorbed; it never sees the Plan.  lower.cpp emits
// one op per fusion record at the layer index the *_at tables name.
#pragma once
#include <initializer_list>
#include <utility>
#include <vector>

#include "../kernels/kernels.h"
#include "../options.h"
#include "graph.h"
#include "plugin.h"

namespace trtx {

struct FusedConv {
    int conv_layer = -1;
    int scale_layer = -1;
    int act1 = ACT_NONE, act2 = ACT_NONE;   // before / after the residual add
    float alpha1 = 0.f, alpha2 = 0.f;
    int residual = -1;  // network tensor id
    int out_tensor = -1;  // network tensor the fused op produces
    int emit_at = -1;     // layer index at which the fused op is scheduled
    int fold_conv = -1, fold_scale = -1;   // RepVGGDW (match_repvggdw_fold): the 3x3 depthwise branch and its scale, folded into this 7x7 one's filter
};

struct YoloHeadFuse {
    int plugin_layer = -1;
    std::vector<int> head_tensor;  // network tensor per level: CHW (64 + classes, gh, gw)
    std::vector<int> branch_tensor;  // task head: network tensor per level, the cv4 convolution's output (B, extra, gh, gw)
    int dfl_conv_layer = -1;
    YoloParams params;              // form YOLO_V8, or YOLO_V10: 6-float records, any class count, OP_YOLO10_HEAD
};

// RepVGGDW (yolov10/src/block.cpp:388-403) on one tensor: depthwise 7x7 s1 p3 + scale, depthwise 3x3 s1 p1 + scale, their sum; the SiLU
// behind the sum is the 7x7 convolution's epilogue (match_conv_fusion continues at the sum's output)
struct RepDwFuse {
    int conv3 = -1, scale3 = -1, sum = -1;   // layers
};

struct Yolo5HeadFuse {
    int plugin_layer = -1;
    std::vector<int> head_tensor;   // network tensor per level: a detect convolution's output (3 * (5 + classes), gh, gw)
    std::vector<int> conv_layer;    // ... and the layer that produces it
    YoloParams params;              // form YOLO_V5, YOLO_V7 (6-float records, OP_YOLO7_HEAD) or YOLO_DARKNET (YOLOv3 / YOLOv3-tiny / YOLOv4: 7-float
                                    // records, OP_DARKNET_HEAD)
};

struct Yolo9HeadFuse {
    int plugin_layer = -1;
    std::vector<int> box_tensor;    // network tensor per level: the grouped 1x1 convolution's output (64, gh, gw)
    std::vector<int> cls_tensor;    // ... and the class convolution's output (classes, gh, gw)
    std::vector<int> cls_conv;      // the layers that produce the class tensors
    int dfl_conv_layer = -1;
    YoloParams params;              // form YOLO_V9
};

struct AttentionFuse {
    int qkv = -1;                    // network tensor: the qkv convolution's output (B, heads*(2kd+hd), H, W)
    int out_o = -1, out_v = -1;      // network tensors: O reshaped to (B, heads*hd, H, W), and v reshaped the same way
    int heads = 0, N = 0, kd = 0, hd = 0;
    float scale = 0.f;
    int area = 0;                    // 0: YOLO11 PSA (psa_attention_kernel); >= 1: YOLOv12 area attention (area_attention_mfma_kernel), N / area keys per query
};

struct AttentionSplitFuse {
    int qk = -1, v = -1, out = -1;   // network tensors: the qk convolution's output (B, 2 heads*hd, H, W), the v convolution's (B, heads*hd, H, W), O as an image
    int heads = 0, N = 0, hd = 0, area = 1;
    float scale = 0.f;
};

struct HgconvFuse {
    int x = -1, out = -1;            // network tensors: the image AdaHGComputation reads (B, D, H, W) and the one its x_out shuffle produces
    int N = 0, D = 0, E = 0;
    float logit_scale = 0.f;         // 1 / (heads * the scaling constant)
    int l_ctx = -1, l_proto = -1, l_pre = -1, l_edge = -1, l_node = -1;   // the layers that hold the weights: context_net, the prototype constant, three Linears
};

struct GeluFuse {
    int in = -1, out = -1;           // network tensors: the chain's input and the result of its last product
    std::vector<int> layers;         // the chain's nine computing layers and its four constants; back() is the last product
};
// The reference's tanh GELU (yolov13/src/block.cpp:702-744) ending in layer `last`: x2 = x x, x3 = x2 x, x3 kappa, + x, * sqrt(2 / pi), tanh, + 1, * x,
// * 0.5, with the constants 0.044715f, 0.797885f, 1 and 0.5 as one-element constant layers.  Fills `f` when every layer is that chain's and none of the
// tensors inside it has a reader outside it or is a network output (the last product's result is the chain's own).
struct NetView;
bool match_tanh_gelu(const NetView& g, int last, GeluFuse* f);

struct SoftmaxChainFuse {
    int in = -1, out = -1;           // network tensors: the scores and the result of the division
    int axis = -1;                   // the dim both reductions run over
    std::vector<int> layers;         // reduce-max, sub, exp, reduce-sum, div; back() is the division
};
// The reference's spelled-out softmax (AAttn, yolov13/src/block.cpp:384-394) ending in the division `last`: m = reduce-max(x) over one axis with keepDims,
// x - m, exp, s = reduce-sum of the exp over the same axis with keepDims, exp / s.  Fills `f` when every layer is that chain's and none of the tensors inside
// it has a reader outside it or is a network output.
bool match_exp_softmax(const NetView& g, int last, SoftmaxChainFuse* f);

struct GatedAddFuse {
    int a = -1, b = -1, out = -1;    // network tensors: out = a + gate (.) b, three images of the same dims
    int gate_layer = -1;             // the constant layer that holds the gate: one element, or one per channel
};

// What the matchers found.  *_at[layer] = index of the record whose op is emitted at that layer, or -1.
struct Fusions {
    std::vector<GatedAddFuse> gated_adds;
    std::vector<int> gated_at;
    std::vector<HgconvFuse> hgconvs;
    std::vector<GeluFuse> gelus;
    std::vector<SoftmaxChainFuse> softmax_chains;
    std::vector<int> hgconv_at, gelu_at, softmax_at;
    std::vector<FusedConv> groups;
    std::vector<YoloHeadFuse> yolo_heads;
    std::vector<AttentionFuse> attns;
    std::vector<Yolo5HeadFuse> yolo5_heads;
    std::vector<Yolo9HeadFuse> yolo9_heads;
    std::vector<AttentionSplitFuse> attn_splits;
    std::vector<int> group_at, yolo_at, attn_at, attn_split_at, yolo5_at, yolo9_at;
    std::vector<bool> pad_cout;                // per layer: a detect convolution whose only reader is a fused anchor or DDetect head: its output channels round up to 16 bytes
    std::vector<RepDwFuse> repdws;
    std::vector<int> repdw_at;                 // per layer: the record of a 7x7 depthwise convolution that takes a RepVGGDW's 3x3 branch into its filter, or -1
    std::vector<int> reorg_src;                // per layer: >= 0 for a convolution that absorbed the ReOrg in front of it - the network tensor the four slices read
    std::vector<bool> absorbed;                // per layer: claimed by a fusion (first claim wins), emits nothing of its own
    std::vector<std::pair<int, int>> aliases;  // (dst network tensor, src network tensor): dst is the same data as src
};

inline bool ident(const int32_t* p, int n) {
    for (int k = 0; k < n; ++k)
        if (p[k] != k) return false;
    return true;
}
inline bool perm_is(const int32_t* p, std::initializer_list<int> want) {
    int k = 0;
    for (int v : want)
        if (p[k++] != v) return false;
    return true;
}
int act_code(int trt_type);   // ACT_* of a TRTX_ACTIVATION_* type the kernels' epilogues know, or -1

// The network as the matchers (and the emission) read it: the definition, who reads each tensor, and the switches of THIS lowering.
struct NetView {
    const Network& net;
    const int dt;                             // dtype of NHWC tensors (the engine's)
    const Options opt = read_options();       // the environment's A/B switches as of THIS lowering (tests flip them inside one process)
    std::vector<std::vector<int>> consumers;  // per tensor: the layers that read it
    explicit NetView(const Network& n);

    int producer(int tensor) const { return net.tensors[tensor].producer; }
    bool sole_consumer(int tensor, int* layer) const {
        if (consumers[tensor].size() != 1 || net.tensors[tensor].is_output) return false;
        *layer = consumers[tensor][0];
        return true;
    }
    bool only_used_by(int tensor, std::initializer_list<int> layers) const;
    // image tensors: (C,H,W) per sample, or (P,C,H,W) per sample where the leading P folds into the image count
    // (TensorRT applies conv/pool/FC to the last three dims; rcnn.cpp:154-160 runs res5 on a (1000,C,14,14) tensor)
    bool spatial(const Dims& d) const { return net.explicit_batch ? d.nb == 4 : (d.nb == 3 || d.nb == 4); }
    bool is_builtin_mish(int li) const {
        const LayerDef& l = net.layers[li];
        return l.kind == L_PLUGIN && l.plugin && l.inputs.size() == 1 && l.outputs.size() == 1 && builtin_is_mish(l.plugin->v);
    }
};

// Runs every matcher, in the order that is part of the behaviour (see the definition).
Fusions match_fusions(const NetView& g);

}  // namespace trtx
