// The lowering's graph matchers.  See lower_match.h.
#include "lower_match.h"

#include <algorithm>

namespace trtx {

int act_code(int trt_type) {
    switch (trt_type) {
        case TRTX_ACTIVATION_RELU: return ACT_RELU;
        case TRTX_ACTIVATION_SIGMOID: return ACT_SIGMOID;
        case TRTX_ACTIVATION_TANH: return ACT_TANH;
        case TRTX_ACTIVATION_LEAKY_RELU: return ACT_LEAKY;
        default: return -1;
    }
}

NetView::NetView(const Network& n) : net(n), dt(n.fp16 ? DT_F16 : DT_F32), consumers(n.tensors.size()) {
    for (size_t li = 0; li < n.layers.size(); ++li)
        for (int t : n.layers[li].inputs) consumers[t].push_back((int)li);
}

bool NetView::only_used_by(int tensor, std::initializer_list<int> layers) const {
    if (net.tensors[tensor].is_output) return false;
    std::vector<int> want(layers), have(consumers[tensor]);
    std::sort(want.begin(), want.end());
    std::sort(have.begin(), have.end());
    return want == have;
}

namespace {

// ---- Conv (+ Scale) (+ activation) (+ residual (+ activation)) -> one fused convolution ---------------------
void match_conv_fusion(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        const LayerDef& l = net.layers[li];
        if (l.kind != L_CONV && l.kind != L_FULLY_CONNECTED) continue;
        if (f.absorbed[li]) continue;  // already claimed (fused YOLO head)
        if (!g.spatial(net.tensors[l.inputs[0]].dims)) continue;
        FusedConv c;
        c.conv_layer = (int)li;
        int t = l.outputs[0], last = (int)li, nx;
        auto take = [&](int layer, int out) {   // `layer` joins the fused op, whose result is now tensor `out`
            f.absorbed[layer] = true;
            t = out;
            last = std::max(last, layer);
        };
        // Conv -> Scale (BatchNorm folded by the host code, block.cpp:45-77)
        if (g.sole_consumer(t, &nx) && !f.absorbed[nx] && net.layers[nx].kind == L_SCALE && net.layers[nx].op != TRTX_SCALE_ELEMENTWISE) {
            const LayerDef& s = net.layers[nx];
            bool pow1 = true;
            for (float p : s.w2) pow1 = pow1 && p == 1.0f;
            if (pow1) {
                c.scale_layer = nx;
                take(nx, s.outputs[0]);
            }
        }
        // RepVGGDW (match_repvggdw_fold): the 3x3 branch goes into this convolution's filter, so its result is the sum's
        if (f.repdw_at[li] >= 0 && c.scale_layer >= 0) {
            const RepDwFuse& r = f.repdws[f.repdw_at[li]];
            c.fold_conv = r.conv3;
            c.fold_scale = r.scale3;
            t = net.layers[r.sum].outputs[0];
            last = std::max(last, r.sum);
        }
        // SiLU spelled as Sigmoid + Prod (block.cpp:91-94), or a plain activation
        if (!net.tensors[t].is_output && g.consumers[t].size() == 2) {
            int a = g.consumers[t][0], b = g.consumers[t][1];
            if (net.layers[a].kind != L_ACTIVATION) std::swap(a, b);
            const LayerDef &la = net.layers[a], &lb = net.layers[b];
            if (la.kind == L_ACTIVATION && la.op == TRTX_ACTIVATION_SIGMOID && lb.kind == L_ELEMENTWISE &&
                lb.op == TRTX_ELEMENTWISE_PROD && a != b && !f.absorbed[a] && !f.absorbed[b]) {
                const int so = la.outputs[0];
                const bool uses = (lb.inputs[0] == t && lb.inputs[1] == so) || (lb.inputs[1] == t && lb.inputs[0] == so);
                int only;
                if (uses && g.sole_consumer(so, &only) && only == b) {
                    c.act1 = ACT_SILU;
                    take(a, lb.outputs[0]);
                    take(b, lb.outputs[0]);
                }
            }
        } else if (g.sole_consumer(t, &nx) && !f.absorbed[nx] && net.layers[nx].kind == L_ACTIVATION && act_code(net.layers[nx].op) >= 0) {
            c.act1 = act_code(net.layers[nx].op);
            c.alpha1 = net.layers[nx].alpha;
            take(nx, net.layers[nx].outputs[0]);
        } else if (g.sole_consumer(t, &nx) && !f.absorbed[nx] && g.is_builtin_mish(nx)) {
            // Conv -> Scale(BN) -> Mish_TRT (convBnMish, yolov4/yolov4.cpp:199-213): the plugin is a pointwise activation
            c.act1 = ACT_MISH;
            take(nx, net.layers[nx].outputs[0]);
        }
        // + residual (block.cpp:104-108 ; resnet50.cpp:146), then an optional trailing activation
        if (g.sole_consumer(t, &nx) && !f.absorbed[nx] && net.layers[nx].kind == L_ELEMENTWISE && net.layers[nx].op == TRTX_ELEMENTWISE_SUM) {
            const LayerDef& e = net.layers[nx];
            const int other = e.inputs[0] == t ? e.inputs[1] : e.inputs[0];
            if (other != t && net.tensors[other].dims == net.tensors[t].dims) {
                c.residual = other;
                take(nx, e.outputs[0]);
                int n2;
                if (g.sole_consumer(t, &n2) && !f.absorbed[n2] && net.layers[n2].kind == L_ACTIVATION && act_code(net.layers[n2].op) >= 0) {
                    c.act2 = act_code(net.layers[n2].op);
                    c.alpha2 = net.layers[n2].alpha;
                    take(n2, net.layers[n2].outputs[0]);
                }
            }
        }
        c.out_tensor = t;
        c.emit_at = last;
        f.absorbed[li] = true;
        f.group_at[last] = (int)f.groups.size();
        f.groups.push_back(c);
    }
}

// Activation applied to a concatenation of un-activated convolution outputs (RetinaFace SSH, retina_r50.cpp:87-98):
// relu(cat(a, b, c)) == cat(relu a, relu b, relu c), so the activation moves into the producers' epilogues (it edits the records of
// match_conv_fusion) and the concat output is used as is.
void match_concat_activation(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        const LayerDef& l = net.layers[li];
        if (l.kind != L_CONCAT || f.absorbed[li]) continue;
        int nx;
        if (!g.sole_consumer(l.outputs[0], &nx) || f.absorbed[nx] || net.layers[nx].kind != L_ACTIVATION) continue;
        const int code = act_code(net.layers[nx].op);
        if (code < 0) continue;
        std::vector<int> gs;
        bool ok = true;
        for (int t : l.inputs) {
            int gi = -1;
            for (size_t k = 0; k < f.groups.size(); ++k)
                if (f.groups[k].out_tensor == t) gi = (int)k;
            int only;
            ok = ok && gi >= 0 && f.groups[gi].act1 == ACT_NONE && f.groups[gi].residual < 0 && f.groups[gi].act2 == ACT_NONE &&
                 g.sole_consumer(t, &only) && only == (int)li;
            gs.push_back(gi);
        }
        if (!ok) continue;
        for (int gi : gs) {
            f.groups[gi].act1 = code;
            f.groups[gi].alpha1 = net.layers[nx].alpha;
        }
        f.absorbed[nx] = true;
        f.aliases.push_back({net.layers[nx].outputs[0], l.outputs[0]});
    }
}

// ---- YOLOv8 detect tail: flatten -> slice -> DFL(shuffle, softmax, 1x1 conv, shuffle) -> concat -> YoloLayer_TRT
// (yolov8/src/model.cpp:263-303, block.cpp:239-257) collapses into one fused kernel when the plugin is the
// built-in one and every intermediate tensor has no other use.  Explicit batch (YOLO11, yolo11/src/model.cpp:336-390): the same graph
// with a leading batch dimension B on every tensor; e = 1 shifts every per-sample axis, and each tensor's dim 0 must be that B (full,
// unsliced).  One level of it, from the two first inputs of the head concat `lc`: ta = DFL(slice [0, 64) of the flattened head),
// tb = slice [64, 64 + classes) of it.
bool match_dfl_classes(const NetView& g, int lc, int ta, int tb, int64_t B, int classes, int* head, int* conv_layer, std::vector<int>* used) {
    const Network& net = g.net;
    const int e = net.explicit_batch ? 1 : 0;
    // box branch
    const int lsh2 = g.producer(ta);
    if (lsh2 < 0 || net.layers[lsh2].kind != L_SHUFFLE || !g.only_used_by(ta, {lc})) return false;
    const LayerDef& sh2 = net.layers[lsh2];
    const Dims& d2 = net.tensors[ta].dims;
    if (d2.nb != 2 + e || (e && d2.d[0] != B) || d2.d[e] != 4 || !ident(sh2.perm1, 3 + e) || !ident(sh2.perm2, 2 + e)) return false;
    const int64_t ng = d2.d[1 + e];
    const int tconv = sh2.inputs[0];
    const int lconv = g.producer(tconv);
    if (lconv < 0 || net.layers[lconv].kind != L_CONV || !g.only_used_by(tconv, {lsh2})) return false;
    const LayerDef& cv = net.layers[lconv];
    if (cv.nb_out != 1 || cv.kernel[0] != 1 || cv.kernel[1] != 1 || cv.groups != 1 || cv.stride[0] != 1 || cv.stride[1] != 1 ||
        cv.padding[0] != 0 || cv.padding[1] != 0 || cv.w0.size() != 16 || !cv.w1.empty())
        return false;
    const int tsm = cv.inputs[0];
    const int lsm = g.producer(tsm);
    if (lsm < 0 || net.layers[lsm].kind != L_SOFTMAX || !g.only_used_by(tsm, {lconv})) return false;
    if (!(net.layers[lsm].axis < 0 || net.layers[lsm].axis == (1 << e))) return false;
    const int tsh1 = net.layers[lsm].inputs[0];
    const int lsh1 = g.producer(tsh1);
    if (lsh1 < 0 || net.layers[lsh1].kind != L_SHUFFLE || !g.only_used_by(tsh1, {lsm})) return false;
    const LayerDef& sh1 = net.layers[lsh1];
    const Dims& d1 = net.tensors[tsh1].dims;
    if (d1.nb != 3 + e || (e && d1.d[0] != B) || d1.d[e] != 16 || d1.d[1 + e] != 4 || d1.d[2 + e] != ng) return false;
    if (!ident(sh1.perm1, 2 + e) || sh1.reshape.nb != 3 + e || (e && sh1.perm2[0] != 0) || sh1.perm2[e] != 1 + e || sh1.perm2[1 + e] != e ||
        sh1.perm2[2 + e] != 2 + e)
        return false;
    const int tsa = sh1.inputs[0];
    const int lsa = g.producer(tsa);
    if (lsa < 0 || net.layers[lsa].kind != L_SLICE || !g.only_used_by(tsa, {lsh1})) return false;
    const LayerDef& sa = net.layers[lsa];
    auto lead_ok = [&](const LayerDef& sl) { return !e || (sl.start.d[0] == 0 && sl.size.d[0] == B && sl.step.d[0] == 1); };
    if (sa.start.nb != 2 + e || !lead_ok(sa) || sa.start.d[e] != 0 || sa.start.d[1 + e] != 0 || sa.size.d[e] != 64 || sa.size.d[1 + e] != ng ||
        sa.step.d[e] != 1 || sa.step.d[1 + e] != 1)
        return false;
    // class branch
    const int lsb = g.producer(tb);
    if (lsb < 0 || net.layers[lsb].kind != L_SLICE || !g.only_used_by(tb, {lc})) return false;
    const LayerDef& sb = net.layers[lsb];
    if (sb.start.nb != 2 + e || !lead_ok(sb) || sb.start.d[e] != 64 || sb.start.d[1 + e] != 0 || sb.size.d[e] != classes ||
        sb.size.d[1 + e] != ng || sb.step.d[e] != 1 || sb.step.d[1 + e] != 1 || sb.inputs[0] != sa.inputs[0])
        return false;
    const int tflat = sa.inputs[0];
    const int lflat = g.producer(tflat);
    if (lflat < 0 || net.layers[lflat].kind != L_SHUFFLE || !g.only_used_by(tflat, {lsa, lsb})) return false;
    const LayerDef& fl = net.layers[lflat];
    const Dims& dx = net.tensors[fl.inputs[0]].dims;
    if (!ident(fl.perm1, 3 + e) || !ident(fl.perm2, 2 + e) || !g.spatial(dx) || (e && dx.d[0] != B) || dx.d[e] != 64 + classes ||
        dx.d[1 + e] * dx.d[2 + e] != ng)
        return false;
    *head = fl.inputs[0];
    *conv_layer = lconv;
    for (int l : {lc, lsh2, lconv, lsm, lsh1, lsa, lsb, lflat}) used->push_back(l);
    return true;
}

// One loop for both fused heads (fp16 and fp32 engines: the kernel reads either element type):
//  - OP_YOLO_HEAD (task = false; implicit and explicit batch): each plugin input is the concat of [DFL chain, class slice] above.
//  - OP_YOLO_TASK_HEAD (task = true), the YOLO11 seg / pose / obb tail (yolo11/src/model.cpp:595-756, 960-1060, 1265-1358), explicit batch
//    only: each plugin input is the axis-1 concat of [DFL chain, class slice, the cv4 branch reshaped (B, extra, H, W) -> (B, extra, g)].
//    The branch convolution keeps its NHWC output, which the fused op reads next to the head (extra_in).
// The parameter gates are disjoint (det_only = none of seg / pose / obb), so a plugin layer is claimed by at most one of the two.
void match_yolo_heads(const NetView& g, bool task, Fusions& f) {
    const Network& net = g.net;
    const int e = net.explicit_batch ? 1 : 0;
    if (task && !e) return;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        const LayerDef& l = net.layers[li];
        if (l.kind != L_PLUGIN || l.outputs.size() != 1 || f.absorbed[li]) continue;
        YoloHeadFuse h;
        if (!builtin_yolo_params(l.plugin->v, &h.params)) continue;
        const YoloParams& pr = h.params;
        // the YOLOv10 plugin (yolov10/src/model.cpp:202-255: the same tail in front of 6-float records), explicit batch only, any class count
        const bool v10 = pr.form == YOLO_V10;
        if (v10 ? (task || !e || !g.opt.yolo10_head) : pr.form != YOLO_V8) continue;
        if (pr.strides.size() != l.inputs.size()) continue;
        if (task ? (pr.seg + pr.pose + pr.obb != 1 || l.inputs.size() > 4 || (pr.pose && (pr.nk < 1 || pr.nk > 17)))
                 : (!pr.det_only() || (!v10 && pr.classes % 8) || l.inputs.size() > 6))
            continue;
        const int64_t extra = pr.seg ? 32 : (pr.pose ? 3 * pr.nk : 1);
        std::vector<int> used;
        bool ok = true;
        for (size_t k = 0; ok && k < l.inputs.size(); ++k) {
            const int t_in = l.inputs[k];
            const int64_t B = e ? net.tensors[t_in].dims.d[0] : 1;
            const int lc = g.producer(t_in);
            ok = lc >= 0 && net.layers[lc].kind == L_CONCAT && net.layers[lc].inputs.size() == (task ? 3u : 2u) && net.layers[lc].axis == e &&
                 g.only_used_by(t_in, {(int)li}) && (!e || B == net.tensors[l.inputs[0]].dims.d[0]);
            int head = -1, conv = -1;
            ok = ok && match_dfl_classes(g, lc, net.layers[lc].inputs[0], net.layers[lc].inputs[1], B, pr.classes, &head, &conv, &used);
            if (!ok) break;
            const Dims& dh = net.tensors[head].dims;
            ok = dh.d[1 + e] == pr.net_h / pr.strides[k] && dh.d[2 + e] == pr.net_w / pr.strides[k];
            if (h.dfl_conv_layer >= 0 && net.layers[conv].w0 != net.layers[h.dfl_conv_layer].w0) ok = false;   // one DFL kernel for all levels
            h.dfl_conv_layer = conv;
            h.head_tensor.push_back(head);
            if (!task) continue;
            // the branch: a reshape-only shuffle of a convolution's (B, extra, H, W) output to (B, extra, H * W)
            const int tc = net.layers[lc].inputs[2];
            const int lsh = g.producer(tc);
            ok = ok && lsh >= 0 && net.layers[lsh].kind == L_SHUFFLE && g.only_used_by(tc, {lc});
            if (!ok) break;
            const LayerDef& sh = net.layers[lsh];
            const int tb = sh.inputs[0];
            const Dims &dx = net.tensors[tb].dims, &dc = net.tensors[tc].dims;
            const int lb = g.producer(tb);
            ok = ident(sh.perm1, 4) && ident(sh.perm2, 3) && dx.nb == 4 && dc.nb == 3 && dx.d[0] == B && dc.d[0] == B && dx.d[1] == extra &&
                 dc.d[1] == extra && dx.d[2] == dh.d[2] && dx.d[3] == dh.d[3] && dc.d[2] == dx.d[2] * dx.d[3] && lb >= 0 &&
                 net.layers[lb].kind == L_CONV && g.only_used_by(tb, {lsh});
            for (int u : {lc, lsh}) used.push_back(u);
            h.branch_tensor.push_back(tb);
        }
        for (int u : used) ok = ok && !f.absorbed[u];
        if (!ok) continue;
        for (int u : used) f.absorbed[u] = true;
        h.plugin_layer = (int)li;
        f.absorbed[li] = true;
        f.yolo_at[li] = (int)f.yolo_heads.size();
        f.yolo_heads.push_back(h);
    }
}

// ---- YOLOv5 detect tail (yolov5/src/model.cpp:331-343): three or four biased 1x1 detect convolutions straight into the anchor-based
// YoloLayer_TRT.  When the plugin is the built-in one (detection, no mask coefficients) and every input is the output of a groups-1,
// 1x1, stride-1 convolution with 3 * (5 + classes) outputs that nobody else reads and that is no network output, the plugin becomes one
// OP_YOLO5_HEAD on the convolutions' NHWC tensors (fp16 and fp32 engines).  The convolutions stay ordinary convolutions; pad_cout marks
// them so that a channel count that is no 16-byte multiple (255) does not cost them their vector stores.  Anything else keeps the
// plugin: marked heads, a second reader, another kernel or channel count, a grid that is not the tensor's, TRTX_YOLO5_HEAD=0.
//
// YOLOv7's tail (yolov7/src/block.cpp:220-255) is the same graph in front of the 6-float plugin (`v7`): the same conditions, one
// OP_YOLO7_HEAD, TRTX_YOLO7_HEAD=0.  A plugin instance is one form or the other, so the two calls cannot claim the same layer.
//
// The Darknet tail (yolov3/yolov3.cpp:282-332, yolov3-tiny/yolov3-tiny.cpp:254-280, yolov4/yolov4.cpp:435-475) is that graph once more in front of
// the zero-field plugin (`form` YOLO_DARKNET): two or three detect convolutions in the plugin's own order, one OP_DARKNET_HEAD, TRTX_DARKNET_HEAD=0.
void match_anchor_heads(const NetView& g, YoloForm form, Fusions& f) {
    const Network& net = g.net;
    const int e = net.explicit_batch ? 1 : 0;
    const bool v7 = form == YOLO_V7, darknet = form == YOLO_DARKNET;
    if (!(darknet ? g.opt.darknet_head : (v7 ? g.opt.yolo7_head : g.opt.yolo5_head))) return;
    if ((v7 || darknet) && net.int8) return;   // kINT8 YOLOv7 networks keep the plugin route: the 6-float head was never run behind a calibrated convolution
    for (size_t li = 0; li < net.layers.size(); ++li) {
        const LayerDef& l = net.layers[li];
        if (l.kind != L_PLUGIN || l.outputs.size() != 1 || f.absorbed[li] || !l.plugin) continue;
        Yolo5HeadFuse h;
        if (!builtin_yolo_params(l.plugin->v, &h.params) || h.params.form != form) continue;
        const YoloParams& pr = h.params;
        if (pr.seg || pr.classes < 1 || l.inputs.empty() || l.inputs.size() > 8 || l.inputs.size() != pr.grid_w.size()) continue;
        bool ok = true;
        for (size_t k = 0; ok && k < l.inputs.size(); ++k) {
            const int t = l.inputs[k];
            const int lc = g.producer(t);
            const Dims& d = net.tensors[t].dims;
            ok = lc >= 0 && net.layers[lc].kind == L_CONV && !f.absorbed[lc] && g.only_used_by(t, {(int)li}) && d.nb == 3 + e;
            if (!ok) break;
            const LayerDef& cv = net.layers[lc];
            ok = cv.groups == 1 && cv.kernel[0] == 1 && cv.kernel[1] == 1 && cv.stride[0] == 1 && cv.stride[1] == 1 && cv.padding[0] == 0 &&
                 cv.padding[1] == 0 && cv.nb_out == 3 * (5 + pr.classes) && d.d[e] == cv.nb_out && d.d[1 + e] == pr.grid_h[k] &&
                 d.d[2 + e] == pr.grid_w[k] && (!e || d.d[0] == net.tensors[l.inputs[0]].dims.d[0]);
            for (size_t j = 0; j < k; ++j) ok = ok && l.inputs[j] != t;
            h.head_tensor.push_back(t);
            h.conv_layer.push_back(lc);
        }
        if (!ok) continue;
        h.plugin_layer = (int)li;
        f.absorbed[li] = true;
        for (int lc : h.conv_layer) f.pad_cout[lc] = true;
        f.yolo5_at[li] = (int)f.yolo5_heads.size();
        f.yolo5_heads.push_back(h);
    }
}

void match_yolo5_heads(const NetView& g, Fusions& f) { match_anchor_heads(g, YOLO_V5, f); }

// ---- ReOrg (yolov7/src/block.cpp:106-114; YOLOv5's Focus is the same graph): four slices of one image tensor with step (1, 2, 2) and
// starts (0,0,0), (0,1,0), (0,0,1), (0,1,1), whole-channel, concatenated in that order on the channel axis, read by nothing but one
// k x k stride-1, dilation-1, groups-1 convolution with padding p.  Slice q = 2 dx + dy holds x[c][2 y + dy][2 x + dx], so the
// convolution is one 2k x 2k stride-2 padding-2p convolution of the slices' input with W'[o][c][2 i + dy][2 j + dx] = W[o][q Cin + c][i][j]
// (reorg_fold_weights, pack.cpp): tap (i, j) of slice q reads x[c][2 (y + i - p) + dy][2 (x + j - p) + dx], and a padded tap of the
// slices is a padded tap of x.  The slices and the concat emit nothing (on the linear layout they would be four gathers over the
// network's largest tensor, a concat and a layout pass); reorg_src names the convolution's new input.  Misses: odd H or W, other
// starts, steps, sizes or order, a second reader of a slice or of the concat, a network output among them.  TRTX_REORG_FOLD=0.
void match_reorg_fold(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    // kINT8 networks keep the gathers: the folded convolution would quantise the slices' input with a scale calibrated for another tensor
    // (the concat's), and no INT8 engine with a ReOrg has been run
    if (!g.opt.reorg_fold || net.int8) return;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        const LayerDef& cat = net.layers[li];
        if (cat.kind != L_CONCAT || f.absorbed[li] || cat.inputs.size() != 4 || cat.outputs.size() != 1) continue;
        const Dims& dc = net.tensors[cat.outputs[0]].dims;
        if (!g.spatial(dc) || cat.axis != dc.nb - 3) continue;
        int lcv;
        if (!g.sole_consumer(cat.outputs[0], &lcv) || f.absorbed[lcv]) continue;
        const LayerDef& cv = net.layers[lcv];
        if (cv.kind != L_CONV || cv.inputs.size() != 1 || cv.groups != 1 || cv.stride[0] != 1 || cv.stride[1] != 1 || cv.dilation[0] != 1 ||
            cv.dilation[1] != 1)
            continue;
        static const int want[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};   // (dy, dx) in concat order
        int src = -1;
        bool ok = true;
        std::vector<int> slices;
        for (int q = 0; ok && q < 4; ++q) {
            const int t = cat.inputs[q];
            const int ls = g.producer(t);
            ok = ls >= 0 && net.layers[ls].kind == L_SLICE && !f.absorbed[ls] && g.only_used_by(t, {(int)li});
            if (!ok) break;
            const LayerDef& s = net.layers[ls];
            const Dims& di = net.tensors[s.inputs[0]].dims;
            const int n = di.nb;
            ok = g.spatial(di) && (src < 0 || src == s.inputs[0]) && di.d[n - 2] % 2 == 0 && di.d[n - 1] % 2 == 0 && s.start.nb == n &&
                 s.size.nb == n && s.step.nb == n;
            if (!ok) break;
            src = s.inputs[0];
            for (int k = 0; k < n - 2; ++k) ok = ok && s.start.d[k] == 0 && s.step.d[k] == 1 && s.size.d[k] == di.d[k];
            ok = ok && s.start.d[n - 2] == want[q][0] && s.start.d[n - 1] == want[q][1] && s.step.d[n - 2] == 2 && s.step.d[n - 1] == 2 &&
                 s.size.d[n - 2] == di.d[n - 2] / 2 && s.size.d[n - 1] == di.d[n - 1] / 2;
            for (int p : slices) ok = ok && p != ls;
            slices.push_back(ls);
        }
        if (!ok) continue;
        const Dims& dx = net.tensors[src].dims;
        if ((size_t)cv.w0.size() != (size_t)cv.nb_out * 4 * dx.d[dx.nb - 3] * cv.kernel[0] * cv.kernel[1]) continue;
        for (int ls : slices) f.absorbed[ls] = true;
        f.absorbed[li] = true;
        f.reorg_src[lcv] = src;
    }
}
// ---- RepVGGDW (yolov10/src/block.cpp:388-403): act(conv7(x) + conv3(x)) with both convolutions depthwise, stride 1, 'same' padding, no
// dilation, each behind its own per-channel scale (the folded BatchNorm, power 1).  A 3x3 filter in the centre of a 7x7 one reads the same
// pixels, so conv7 + conv3 is ONE 7x7 depthwise convolution whose filter is scale7 * w7 + scale3 * w3 (centre) and whose shift is the
// two shifts' sum (pack_weights does that in double).  Applies only when neither convolution's, neither scale's output has another
// reader or is a network output.  What follows the sum (the SiLU) is left to match_conv_fusion.  TRTX_REPVGGDW_FOLD=0 turns it off.
void match_repvggdw_fold(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    if (!g.opt.repvggdw_fold || net.int8) return;
    auto dw_same = [&](const LayerDef& l, int k) {
        const Dims& di = net.tensors[l.inputs[0]].dims;
        return l.kind == L_CONV && g.spatial(di) && l.kernel[0] == k && l.kernel[1] == k && l.stride[0] == 1 && l.stride[1] == 1 && l.padding[0] == k / 2 &&
               l.padding[1] == k / 2 && l.dilation[0] == 1 && l.dilation[1] == 1 && l.nb_out == di.d[di.nb - 3] && l.groups == l.nb_out &&
               (int64_t)l.w0.size() == (int64_t)l.nb_out * k * k;
    };
    // the per-channel scale behind convolution `lc`, read by `reader` only
    auto scale_of = [&](int lc, int* ls) {
        int nx;
        if (!g.sole_consumer(net.layers[lc].outputs[0], &nx) || f.absorbed[nx] || net.layers[nx].kind != L_SCALE || net.layers[nx].op == TRTX_SCALE_ELEMENTWISE) return false;
        for (float p : net.layers[nx].w2)
            if (p != 1.0f) return false;
        *ls = nx;
        return true;
    };
    for (size_t li = 0; li < net.layers.size(); ++li) {
        const LayerDef& l7 = net.layers[li];
        if (f.absorbed[li] || !dw_same(l7, 7)) continue;
        int s7 = -1, sum = -1;
        if (!scale_of((int)li, &s7) || !g.sole_consumer(net.layers[s7].outputs[0], &sum) || f.absorbed[sum]) continue;
        const LayerDef& ls = net.layers[sum];
        if (ls.kind != L_ELEMENTWISE || ls.op != TRTX_ELEMENTWISE_SUM || ls.inputs.size() != 2) continue;
        const int t7 = net.layers[s7].outputs[0];
        const int t3 = ls.inputs[0] == t7 ? ls.inputs[1] : ls.inputs[0];
        if (t3 == t7) continue;
        const int s3 = g.producer(t3);
        if (s3 < 0 || f.absorbed[s3] || net.layers[s3].kind != L_SCALE || !g.only_used_by(t3, {sum})) continue;
        const int c3 = g.producer(net.layers[s3].inputs[0]);
        int s3_again = -1;
        if (c3 < 0 || c3 == (int)li || f.absorbed[c3] || !dw_same(net.layers[c3], 3) || !scale_of(c3, &s3_again) || s3_again != s3) continue;
        if (net.layers[c3].inputs[0] != l7.inputs[0] || net.layers[c3].nb_out != l7.nb_out) continue;
        f.absorbed[c3] = f.absorbed[s3] = f.absorbed[sum] = true;
        f.repdw_at[li] = (int)f.repdws.size();
        f.repdws.push_back(RepDwFuse{c3, s3, sum});
    }
}

void match_yolo7_heads(const NetView& g, Fusions& f) { match_anchor_heads(g, YOLO_V7, f); }
void match_darknet_heads(const NetView& g, Fusions& f) { match_anchor_heads(g, YOLO_DARKNET, f); }

// ---- YOLOv9 / GELAN detect tail (yolov9/src/block.cpp:424-489): per level the concat of [DFL chain on the grouped 1x1 convolution's
// (64, gh, gw) output, reshape (classes, gh * gw) of the class convolution's output] into the YOLOv9 YoloLayer_TRT.  Unlike YOLOv8's tail
// the two branches end in two different convolutions, so there is no flatten and no slice to match.  When the plugin is the built-in one
// without mask coefficients, every intermediate tensor has no other reader and is no network output, the DFL convolution has 16 weights
// (the same on every level) and no bias, and the grids are the tensors', the whole tail becomes one OP_YOLO9_HEAD on the two NHWC tensors
// per level (fp16 and fp32 engines).  pad_cout marks the class convolutions, so that a class count that is no 16-byte multiple keeps their
// vector stores.  Anything else keeps the plugin: marked heads, a second reader, a kINT8 engine, TRTX_YOLO9_HEAD=0.  Implicit batch, as the reference builds.
void match_yolo9_heads(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    // kINT8 engines keep the plugin route too: the fused op reads fp16 or fp32 tensors, and the int8 assignment does not see its class
    // tensors (they are extra inputs), so a calibrated class convolution would hand it int8 values
    if (!g.opt.yolo9_head || net.explicit_batch || net.int8) return;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        const LayerDef& l = net.layers[li];
        if (l.kind != L_PLUGIN || l.outputs.size() != 1 || f.absorbed[li] || !l.plugin) continue;
        Yolo9HeadFuse h;
        if (!builtin_yolo_params(l.plugin->v, &h.params) || h.params.form != YOLO_V9) continue;
        const YoloParams& pr = h.params;
        if (pr.seg || pr.classes < 1 || l.inputs.size() != 3) continue;
        std::vector<int> used;
        bool ok = true;
        for (size_t k = 0; ok && k < l.inputs.size(); ++k) {
            ok = false;
            const int64_t gh = pr.net_h / (8 << k), gw = pr.net_w / (8 << k), ng = gh * gw;
            const int t_in = l.inputs[k];
            const int lc = g.producer(t_in);
            if (lc < 0 || net.layers[lc].kind != L_CONCAT || net.layers[lc].inputs.size() != 2 || net.layers[lc].axis != 0 ||
                !g.only_used_by(t_in, {(int)li}))
                break;
            const int ta = net.layers[lc].inputs[0], tb = net.layers[lc].inputs[1];
            // box branch, from the concat back to the convolution: shuffle (4, ng) <- 1x1 conv <- softmax <- shuffle (16, 4, ng)
            const int lsh2 = g.producer(ta);
            if (lsh2 < 0 || net.layers[lsh2].kind != L_SHUFFLE || !g.only_used_by(ta, {lc})) break;
            const LayerDef& sh2 = net.layers[lsh2];
            const Dims& d2 = net.tensors[ta].dims;
            if (d2.nb != 2 || d2.d[0] != 4 || d2.d[1] != ng || !ident(sh2.perm1, 3) || !ident(sh2.perm2, 2)) break;
            const int tconv = sh2.inputs[0];
            const int lconv = g.producer(tconv);
            if (lconv < 0 || net.layers[lconv].kind != L_CONV || !g.only_used_by(tconv, {lsh2})) break;
            const LayerDef& cv = net.layers[lconv];
            if (cv.nb_out != 1 || cv.kernel[0] != 1 || cv.kernel[1] != 1 || cv.groups != 1 || cv.stride[0] != 1 || cv.stride[1] != 1 ||
                cv.padding[0] != 0 || cv.padding[1] != 0 || cv.w0.size() != 16 || !cv.w1.empty())
                break;
            if (h.dfl_conv_layer >= 0 && cv.w0 != net.layers[h.dfl_conv_layer].w0) break;   // one DFL kernel for all levels
            const int tsm = cv.inputs[0];
            const int lsm = g.producer(tsm);
            if (lsm < 0 || net.layers[lsm].kind != L_SOFTMAX || !g.only_used_by(tsm, {lconv})) break;
            if (!(net.layers[lsm].axis < 0 || net.layers[lsm].axis == 1)) break;
            const int tsh1 = net.layers[lsm].inputs[0];
            const int lsh1 = g.producer(tsh1);
            if (lsh1 < 0 || net.layers[lsh1].kind != L_SHUFFLE || !g.only_used_by(tsh1, {lsm})) break;
            const LayerDef& sh1 = net.layers[lsh1];
            const Dims& d1 = net.tensors[tsh1].dims;
            if (d1.nb != 3 || d1.d[0] != 16 || d1.d[1] != 4 || d1.d[2] != ng || !ident(sh1.perm1, 3) || sh1.reshape.nb != 3 ||
                !perm_is(sh1.perm2, {1, 0, 2}))
                break;
            const int tbox = sh1.inputs[0];
            const int lbox = g.producer(tbox);
            const Dims& db = net.tensors[tbox].dims;
            if (lbox < 0 || net.layers[lbox].kind != L_CONV || !g.only_used_by(tbox, {lsh1}) || db.nb != 3 || db.d[0] != 64 || db.d[1] != gh ||
                db.d[2] != gw)
                break;
            // class branch: a reshape-only shuffle of a convolution's (classes, gh, gw) output
            const int lshc = g.producer(tb);
            if (lshc < 0 || net.layers[lshc].kind != L_SHUFFLE || !g.only_used_by(tb, {lc})) break;
            const LayerDef& shc = net.layers[lshc];
            const Dims& dc = net.tensors[tb].dims;
            if (dc.nb != 2 || dc.d[0] != pr.classes || dc.d[1] != ng || !ident(shc.perm1, 3) || !ident(shc.perm2, 2)) break;
            const int tcls = shc.inputs[0];
            const int lcls = g.producer(tcls);
            const Dims& dk = net.tensors[tcls].dims;
            if (lcls < 0 || net.layers[lcls].kind != L_CONV || !g.only_used_by(tcls, {lshc}) || dk.nb != 3 || dk.d[0] != pr.classes ||
                dk.d[1] != gh || dk.d[2] != gw || net.layers[lcls].nb_out != pr.classes || tcls == tbox)
                break;
            h.dfl_conv_layer = lconv;
            h.box_tensor.push_back(tbox);
            h.cls_tensor.push_back(tcls);
            h.cls_conv.push_back(lcls);
            for (int u : {lc, lsh2, lconv, lsm, lsh1, lshc}) used.push_back(u);
            if (f.absorbed[lbox] || f.absorbed[lcls]) break;
            ok = true;
        }
        for (int u : used) ok = ok && !f.absorbed[u];
        if (!ok) continue;
        for (int u : used) f.absorbed[u] = true;
        h.plugin_layer = (int)li;
        f.absorbed[li] = true;
        for (int lc : h.cls_conv) f.pad_cout[lc] = true;
        f.yolo9_at[li] = (int)f.yolo9_heads.size();
        f.yolo9_heads.push_back(h);
    }
}

// ---- attention: what the YOLO11 PSA block and the YOLOv12 area attention share, from the first matmul to the second one:
// x (B', heads, 2kd+hd, N') -> q / k / v slices of rows -> q^T k -> uniform scale -> softmax over the keys -> v @ attn^T.
// Every shape, permutation, slice and the scale are checked and q, k and the scores must have no other reader.  How the qkv image
// becomes x, and how O and v (which has exactly one more reader) become images again, is each caller's part.
struct AttentionCore {
    int lq, lk, lv, lqt, m1, lsc, lsm, lat, m2;   // the layers, all claimed by the fused op
    int tx;                                       // network tensor x
    int64_t kd, hd;
    float scale;
};
bool transpose_only(const LayerDef& l, std::initializer_list<int> p) {   // a shuffle that is one first transpose of a 4-d tensor
    return l.kind == L_SHUFFLE && l.reshape.nb == 0 && perm_is(l.perm1, p) && ident(l.perm2, 4);
}
bool plain_matmul(const LayerDef& l) { return l.kind == L_MATMUL && l.mm_op[0] == TRTX_MATMUL_NONE && l.mm_op[1] == TRTX_MATMUL_NONE; }

bool match_attention_core(const NetView& g, int li, AttentionCore* c) {
    const Network& net = g.net;
    const LayerDef& m1 = net.layers[li];
    if (!plain_matmul(m1)) return false;
    c->m1 = li;
    const int lqt = c->lqt = g.producer(m1.inputs[0]), lk = c->lk = g.producer(m1.inputs[1]);
    if (lqt < 0 || lk < 0 || !transpose_only(net.layers[lqt], {0, 1, 3, 2}) || net.layers[lk].kind != L_SLICE) return false;
    const int lq = c->lq = g.producer(net.layers[lqt].inputs[0]);
    if (lq < 0 || net.layers[lq].kind != L_SLICE) return false;
    const int tx = c->tx = net.layers[lq].inputs[0];
    const Dims& dx = net.tensors[tx].dims;
    if (net.layers[lk].inputs[0] != tx || dx.nb != 4) return false;
    auto slice_rows = [&](const LayerDef& sl, int64_t r0, int64_t nr) {   // rows [r0, r0 + nr) of every head, everything else whole
        return sl.start.nb == 4 && sl.start.d[0] == 0 && sl.start.d[1] == 0 && sl.start.d[2] == r0 && sl.start.d[3] == 0 && sl.size.d[0] == dx.d[0] &&
               sl.size.d[1] == dx.d[1] && sl.size.d[2] == nr && sl.size.d[3] == dx.d[3] && sl.step.d[0] == 1 && sl.step.d[1] == 1 && sl.step.d[2] == 1 &&
               sl.step.d[3] == 1;
    };
    const int64_t kd = c->kd = net.layers[lq].size.d[2];
    const int64_t hd = c->hd = dx.d[2] - 2 * kd;
    if (!slice_rows(net.layers[lq], 0, kd) || !slice_rows(net.layers[lk], kd, kd) || hd < 1) return false;
    // the v slice: the third reader of x
    int lv = -1;
    for (int r : g.consumers[tx])
        if (r != lq && r != lk) lv = r;
    c->lv = lv;
    if (lv < 0 || net.layers[lv].kind != L_SLICE || !slice_rows(net.layers[lv], 2 * kd, hd) || !g.only_used_by(tx, {lq, lk, lv})) return false;
    // scale -> softmax -> transpose -> second matmul
    if (!g.sole_consumer(m1.outputs[0], &c->lsc) || net.layers[c->lsc].kind != L_SCALE || net.layers[c->lsc].op != TRTX_SCALE_UNIFORM) return false;
    const LayerDef& sc = net.layers[c->lsc];
    if (sc.w1.size() != 1 || (!sc.w0.empty() && (sc.w0.size() != 1 || sc.w0[0] != 0.f)) || (!sc.w2.empty() && (sc.w2.size() != 1 || sc.w2[0] != 1.f)))
        return false;
    c->scale = sc.w1[0];
    if (!g.sole_consumer(sc.outputs[0], &c->lsm) || net.layers[c->lsm].kind != L_SOFTMAX || net.layers[c->lsm].axis != (1 << 3)) return false;
    if (!g.sole_consumer(net.layers[c->lsm].outputs[0], &c->lat) || !transpose_only(net.layers[c->lat], {0, 1, 3, 2})) return false;
    const int t_at = net.layers[c->lat].outputs[0];
    if (!g.sole_consumer(t_at, &c->m2)) return false;
    const LayerDef& mm2 = net.layers[c->m2];
    if (!plain_matmul(mm2) || mm2.inputs[1] != t_at || mm2.inputs[0] != net.layers[lv].outputs[0]) return false;
    return g.only_used_by(m1.inputs[0], {li}) && g.only_used_by(m1.inputs[1], {li}) && g.only_used_by(net.layers[lqt].inputs[0], {lqt});
}
// Claims the core's layers and the caller's `own` ones for one OP_ATTENTION, emitted at the last of them - unless one of them is
// already claimed or produces a network output.
void claim_attention(const NetView& g, const AttentionCore& c, std::vector<int> own, AttentionFuse a, Fusions& f) {
    for (int u : {c.lq, c.lk, c.lv, c.lqt, c.m1, c.lsc, c.lsm, c.lat, c.m2}) own.push_back(u);
    for (int u : own)
        if (f.absorbed[u] || g.net.tensors[g.net.layers[u].outputs[0]].is_output) return;
    a.heads = (int)g.net.tensors[c.tx].dims.d[1];
    a.kd = (int)c.kd;
    a.hd = (int)c.hd;
    a.scale = c.scale;
    int at = 0;
    for (int u : own) {
        f.absorbed[u] = true;
        at = std::max(at, u);
    }
    f.attn_at[at] = (int)f.attns.size();
    f.attns.push_back(a);
}

// ---- YOLO11 PSA attention (yolo11/src/block.cpp:287-339): qkv -> view (B, heads, 2kd+hd, N) -> the core above -> view
// (B, heads*hd, H, W), and v viewed the same way for `pe`.  Anything else keeps the generic linear path.
// fp16 engines only (fp32 engines, the tolerance build, keep the generic path).
void match_psa_attention(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    if (!net.explicit_batch || g.dt != DT_F16) return;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        AttentionCore c;
        if (f.absorbed[li] || !match_attention_core(g, (int)li, &c)) continue;
        // the way in: one reshape-only view of the qkv image
        const int lview = g.producer(c.tx);
        if (lview < 0 || net.layers[lview].kind != L_SHUFFLE || !ident(net.layers[lview].perm1, 4) || !ident(net.layers[lview].perm2, 4)) continue;
        const int tqkv = net.layers[lview].inputs[0];
        const Dims &dx = net.tensors[c.tx].dims, &dq = net.tensors[tqkv].dims;
        if (dq.nb != 4 || dx.d[0] != dq.d[0] || dx.d[3] != dq.d[2] * dq.d[3] || dx.d[1] * dx.d[2] != dq.d[1]) continue;
        // the way out: O's only reader and v's other reader
        int lre, lvre = -1;
        if (!g.sole_consumer(net.layers[c.m2].outputs[0], &lre)) continue;
        const int tv = net.layers[c.lv].outputs[0];
        for (int r : g.consumers[tv])
            if (r != c.m2) lvre = r;
        if (lvre < 0 || !g.only_used_by(tv, {c.m2, lvre})) continue;
        auto view_bchw = [&](int l) {   // reshape (B, heads*hd, H, W) of a (B, heads, hd, N) tensor, no transposes
            const LayerDef& r = net.layers[l];
            const Dims& o = net.tensors[r.outputs[0]].dims;
            return r.kind == L_SHUFFLE && ident(r.perm1, 4) && ident(r.perm2, 4) && r.reshape.nb == 4 && o.nb == 4 && o.d[0] == dx.d[0] &&
                   o.d[1] == dx.d[1] * c.hd && o.d[2] == dq.d[2] && o.d[3] == dq.d[3];
        };
        if (!view_bchw(lre) || !view_bchw(lvre) || !psa_attention_supported((int)c.kd, (int)c.hd)) continue;
        AttentionFuse a;
        a.qkv = tqkv;
        a.out_o = net.layers[lre].outputs[0];
        a.out_v = net.layers[lvre].outputs[0];
        a.N = (int)dx.d[3];
        claim_attention(g, c, {lview, lre, lvre}, a, f);
    }
}

// ---- YOLOv12 area attention (yolov12/src/block.cpp:522-625): qkv (B, heads*96, H, W) -> [reshape (B, -1, N), transpose {0,2,1}] ->
// [reshape (B area, N / area, heads, 96), transpose {0,2,3,1}] -> the core above on q / k / v slices of 32 rows -> transpose {0,3,1,2}
// -> reshape (B, H, W, C) -> transpose {0,3,1,2}, and v through the same three shuffles for `pe`.  In NHWC that is: area a = the
// pixel range [a N/area, (a+1) N/area) of an image, head h = channels h*96 + {q | k | v}.  Anything else keeps the generic linear
// path.  fp16 explicit-batch engines only, and not with TRTX_AREA_ATTENTION=0.
void match_area_attention(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    if (!net.explicit_batch || g.dt != DT_F16 || !g.opt.area_attention) return;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        AttentionCore c;
        if (f.absorbed[li] || !match_attention_core(g, (int)li, &c)) continue;
        // the way in: the two shuffles between the qkv image and the (B area, heads, 96, N / area) tensor
        const int l2 = g.producer(c.tx);
        if (l2 < 0 || net.layers[l2].kind != L_SHUFFLE || net.layers[l2].reshape.nb != 4 || !ident(net.layers[l2].perm1, 3) ||
            !perm_is(net.layers[l2].perm2, {0, 2, 3, 1}))
            continue;
        const int tl = net.layers[l2].inputs[0];
        const int l1 = g.producer(tl);
        if (l1 < 0 || net.layers[l1].kind != L_SHUFFLE || net.layers[l1].reshape.nb != 3 || !ident(net.layers[l1].perm1, 4) ||
            !perm_is(net.layers[l1].perm2, {0, 2, 1}))
            continue;
        const int tqkv = net.layers[l1].inputs[0];
        const Dims &dx = net.tensors[c.tx].dims, &dl = net.tensors[tl].dims, &dq = net.tensors[tqkv].dims;
        if (dl.nb != 3 || dq.nb != 4) continue;
        const int64_t B = dq.d[0], C3 = dq.d[1], N = dq.d[2] * dq.d[3];
        const int64_t Ba = dx.d[0], heads = dx.d[1], rows = dx.d[2], Na = dx.d[3];
        if (dl.d[0] != B || dl.d[1] != N || dl.d[2] != C3 || B < 1 || Na < 1 || Ba % B != 0 || heads * rows != C3) continue;
        const int64_t area = Ba / B;
        if (area < 1 || Na * area != N) continue;   // the area count must divide the pixels
        if (!g.only_used_by(tl, {l2}) || !area_attention_supported((int)c.kd, (int)c.hd)) continue;
        // the way back to an image, for O and for v: transpose {0,3,1,2} -> reshape (B, H, W, heads*hd) -> transpose {0,3,1,2}
        auto image_of = [&](int t_from, int skip, int* used3, int* t_img) {
            int a = -1;
            for (int r : g.consumers[t_from])
                if (r != skip) a = r;
            if (a < 0 || net.tensors[t_from].is_output || g.consumers[t_from].size() != (skip >= 0 ? 2u : 1u) || !transpose_only(net.layers[a], {0, 3, 1, 2}))
                return false;
            int r, b2;
            if (!g.sole_consumer(net.layers[a].outputs[0], &r)) return false;
            const LayerDef& re = net.layers[r];
            const Dims& dr = net.tensors[re.outputs[0]].dims;
            if (re.kind != L_SHUFFLE || re.reshape.nb != 4 || !ident(re.perm1, 4) || !ident(re.perm2, 4) || dr.nb != 4 || dr.d[0] != B ||
                dr.d[1] != dq.d[2] || dr.d[2] != dq.d[3] || dr.d[3] != heads * c.hd)
                return false;
            if (!g.sole_consumer(re.outputs[0], &b2) || !transpose_only(net.layers[b2], {0, 3, 1, 2})) return false;
            used3[0] = a; used3[1] = r; used3[2] = b2;
            *t_img = net.layers[b2].outputs[0];
            return true;
        };
        int uo[3], uv[3];
        AttentionFuse a;
        if (!image_of(net.layers[c.m2].outputs[0], -1, uo, &a.out_o) || !image_of(net.layers[c.lv].outputs[0], c.m2, uv, &a.out_v)) continue;
        a.qkv = tqkv;
        a.N = (int)N;
        a.area = (int)area;
        claim_attention(g, c, {l1, l2, uo[0], uo[1], uo[2], uv[0], uv[1], uv[2]}, a, f);
    }
}

// ---- YOLOv13 area attention (yolov13/src/block.cpp:303-423), walked from the first matmul.  q | k come from one convolution and v from another:
//   qk (B, 2C, H, W) -> flatten {reshape (B, -1, N), second transpose {0,2,1}} -> [reshape (B', N', 2C)] -> slices [0, C) = q and [C, 2C) = k of the last axis,
//   each -> reshape (B', N', heads, hd) -> transpose {0,2,3,1}, q once more {0,1,3,2};  v (B, C, H, W) -> the same flatten -> [reshape (B', N', C)] ->
//   reshape (B', N', heads, hd) -> transpose {0,2,3,1};  matmul(q^T, k) -> uniform scale (shift 0, power 1) -> softmax over axis 3, as the five-layer chain
//   (match_exp_softmax) or one ISoftMaxLayer -> transpose {0,1,3,2} -> matmul(v, p^T) -> transpose {0,3,1,2} -> [reshape (B, N, C)] -> {reshape (B, H, W, C),
//   second transpose {0,3,1,2}}, whose output is the op's.  B' = B area, N' = N / area; the bracketed reshapes are absent where the reference has area == 1.
// Checked: every shape, permutation and slice, heads * hd == C, area_attention_split_supported, and that no tensor between the two images and the result has
// a reader outside the match or is a network output.  The qk and v images may have any other readers (v's is `pe`): the op reads them where they are.
// The scale layer becomes the op's scale.  fp16 explicit-batch engines only, not kINT8, and not with TRTX_AATTN_SPLIT=0; anything else keeps the generic ops.
bool match_aattn_split_at(const NetView& g, int li, AttentionSplitFuse* a, std::vector<int>* used) {
    const Network& net = g.net;
    auto dims = [&](int t) -> const Dims& { return net.tensors[t].dims; };
    auto is = [](const Dims& d, std::initializer_list<int64_t> want) {
        if (d.nb != (int)want.size()) return false;
        int k = 0;
        for (int64_t v : want)
            if (d.d[k++] != v) return false;
        return true;
    };
    auto reshape_only = [&](int l, int nb_out) {   // a shuffle that only reshapes, to nb_out dims
        if (l < 0 || net.layers[l].kind != L_SHUFFLE) return false;
        const LayerDef& s = net.layers[l];
        return s.reshape.nb == nb_out && ident(s.perm1, dims(s.inputs[0]).nb) && ident(s.perm2, nb_out);
    };
    auto keep = [&](int l) { used->push_back(l); return net.layers[l].inputs[0]; };   // claims layer l, returns what it reads
    const LayerDef& m1 = net.layers[li];
    if (!plain_matmul(m1)) return false;
    used->push_back(li);
    // (B', N', X) <- [reshape] <- flatten <- image (B, X, H, W): the image, or -1
    int64_t B = 0, Ba = 0, Na = 0, H = 0, W = 0;
    auto image_of = [&](int t3, int64_t X) -> int {
        int l = g.producer(t3);
        if (reshape_only(l, 3) && dims(net.layers[l].inputs[0]).nb == 3) t3 = keep(l), l = g.producer(t3);
        if (l < 0 || net.layers[l].kind != L_SHUFFLE) return -1;
        const LayerDef& fl = net.layers[l];
        const Dims& di = dims(fl.inputs[0]);
        if (fl.reshape.nb != 3 || di.nb != 4 || !ident(fl.perm1, 4) || !perm_is(fl.perm2, {0, 2, 1}) || di.d[1] != X) return -1;
        if (B == 0) B = di.d[0], H = di.d[2], W = di.d[3];
        if (di.d[0] != B || di.d[2] != H || di.d[3] != W || !is(dims(t3), {B, H * W, X})) return -1;
        return keep(l);
    };
    // (B', heads, hd, N') <- transpose {0,2,3,1} <- reshape (B', N', heads, hd) <- t3 (B', N', C): t3, or -1
    int64_t heads = 0, hd = 0;
    auto heads_of = [&](int t4) -> int {
        const int lt = g.producer(t4);
        if (lt < 0 || !transpose_only(net.layers[lt], {0, 2, 3, 1})) return -1;
        const int tr = keep(lt), lr = g.producer(tr);
        if (!reshape_only(lr, 4)) return -1;
        const Dims& d = dims(tr);
        if (heads == 0) Ba = d.d[0], Na = d.d[1], heads = d.d[2], hd = d.d[3];
        const int t3 = keep(lr);
        if (!is(d, {Ba, Na, heads, hd}) || !is(dims(t3), {Ba, Na, heads * hd})) return -1;
        return t3;
    };
    // q and k: two slices of the last axis of one (B', N', 2C) tensor
    const int lqt = g.producer(m1.inputs[0]);
    if (lqt < 0 || !transpose_only(net.layers[lqt], {0, 1, 3, 2})) return false;
    const int tq3 = heads_of(keep(lqt)), tk3 = heads_of(m1.inputs[1]);
    if (tq3 < 0 || tk3 < 0) return false;
    const int lq = g.producer(tq3), lk = g.producer(tk3);
    if (lq < 0 || lk < 0 || net.layers[lq].kind != L_SLICE || net.layers[lk].kind != L_SLICE) return false;
    const int64_t C = heads * hd;
    const int tqk3 = keep(lq);
    if (keep(lk) != tqk3 || !is(dims(tqk3), {Ba, Na, 2 * C})) return false;
    auto slice_last = [&](const LayerDef& sl, int64_t c0) {
        return is(sl.start, {0, 0, c0}) && is(sl.size, {Ba, Na, C}) && is(sl.step, {1, 1, 1});
    };
    if (!slice_last(net.layers[lq], 0) || !slice_last(net.layers[lk], C)) return false;
    a->qk = image_of(tqk3, 2 * C);
    if (a->qk < 0) return false;
    const int64_t N = H * W;
    if (B < 1 || Na < 1 || Ba % B != 0 || Ba / B * Na != N) return false;
    // scores -> uniform scale -> softmax over the keys
    int lsc, lsm;
    if (!g.sole_consumer(m1.outputs[0], &lsc) || net.layers[lsc].kind != L_SCALE || net.layers[lsc].op != TRTX_SCALE_UNIFORM) return false;
    const LayerDef& sc = net.layers[lsc];
    if (sc.w1.size() != 1 || (!sc.w0.empty() && (sc.w0.size() != 1 || sc.w0[0] != 0.f)) || (!sc.w2.empty() && (sc.w2.size() != 1 || sc.w2[0] != 1.f)))
        return false;
    used->push_back(lsc);
    int tp = -1;
    if (g.sole_consumer(sc.outputs[0], &lsm) && net.layers[lsm].kind == L_SOFTMAX) {
        if (net.layers[lsm].axis != (1 << 3)) return false;
        used->push_back(lsm);
        tp = net.layers[lsm].outputs[0];
    } else {   // the spelled-out chain: found from the scores' subtraction
        SoftmaxChainFuse c;
        for (int r : g.consumers[sc.outputs[0]]) {
            int lexp;
            if (net.layers[r].kind != L_ELEMENTWISE || net.layers[r].op != TRTX_ELEMENTWISE_SUB || !g.sole_consumer(net.layers[r].outputs[0], &lexp)) continue;
            for (int d : g.consumers[net.layers[lexp].outputs[0]]) {
                SoftmaxChainFuse at_d;
                if (match_exp_softmax(g, d, &at_d) && at_d.in == sc.outputs[0] && at_d.axis == 3) c = at_d;
            }
        }
        if (c.out < 0) return false;
        tp = c.out;
        used->insert(used->end(), c.layers.begin(), c.layers.end());
    }
    // p^T and the value product
    int lat, m2;
    if (!g.sole_consumer(tp, &lat) || !transpose_only(net.layers[lat], {0, 1, 3, 2}) || !g.sole_consumer(net.layers[lat].outputs[0], &m2)) return false;
    const LayerDef& mm2 = net.layers[m2];
    if (!plain_matmul(mm2) || mm2.inputs[1] != net.layers[lat].outputs[0]) return false;
    used->push_back(lat);
    used->push_back(m2);
    const int tv3 = heads_of(mm2.inputs[0]);
    if (tv3 < 0) return false;
    a->v = image_of(tv3, C);
    if (a->v < 0) return false;
    // the way out
    int lo, lx;
    if (!g.sole_consumer(mm2.outputs[0], &lo) || !transpose_only(net.layers[lo], {0, 3, 1, 2}) || !g.sole_consumer(net.layers[lo].outputs[0], &lx)) return false;
    used->push_back(lo);
    if (reshape_only(lx, 3)) {
        if (!is(dims(net.layers[lx].outputs[0]), {B, N, C})) return false;
        used->push_back(lx);
        if (!g.sole_consumer(net.layers[lx].outputs[0], &lx)) return false;
    }
    const LayerDef& x = net.layers[lx];
    if (x.kind != L_SHUFFLE || x.reshape.nb != 4 || !ident(x.perm1, dims(x.inputs[0]).nb) || !perm_is(x.perm2, {0, 3, 1, 2}) ||
        !is(x.reshape, {B, H, W, C}) || !is(dims(x.outputs[0]), {B, C, H, W}))
        return false;
    used->push_back(lx);
    // no claimed layer twice, the result's shuffle is the last of them, and nothing inside is read from outside or is a network output
    std::vector<int> sorted(*used);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end() || sorted.back() != lx) return false;
    for (int u : sorted) {
        if (u == lx) continue;
        const int t = net.layers[u].outputs[0];
        if (net.tensors[t].is_output) return false;
        for (int r : g.consumers[t])
            if (!std::binary_search(sorted.begin(), sorted.end(), r)) return false;
    }
    if (!area_attention_split_supported((int)hd, (int)hd)) return false;
    a->out = x.outputs[0];
    a->heads = (int)heads;
    a->N = (int)N;
    a->hd = (int)hd;
    a->area = (int)(Ba / B);
    a->scale = sc.w1[0];
    return true;
}

void match_aattn_split(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    if (!net.explicit_batch || g.dt != DT_F16 || net.int8 || !g.opt.aattn_split) return;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        AttentionSplitFuse a;
        std::vector<int> used;
        if (f.absorbed[li] || !match_aattn_split_at(g, (int)li, &a, &used)) continue;
        bool free = true;
        for (int u : used) free = free && !f.absorbed[u];
        if (!free) continue;
        for (int u : used) f.absorbed[u] = true;
        f.attn_split_at[used.back()] = (int)f.attn_splits.size();
        f.attn_splits.push_back(a);
    }
}

// ---- YOLOv13's adaptive hypergraph convolution: AdaHGComputation (yolov13/src/block.cpp:792-812) from its `tokens` shuffle
// ((B, D, H, W) -> (B, N, D)) to its `x_out` shuffle, i.e. AdaHyperedgeGen (607-700), AdaHGConv (746-790) and both GELU chains, walked
// backwards from x_out.  Checked: every reshape and permutation, both reduces of the context and their axis, the concat axis, the three
// Linear shapes and the prototype constant's, the head split (heads * head_dim == D), the scalar divisor, the mean over the heads, the
// softmax axis (the NODES: 1 << 1 on (B, N, E)), both matmul transposes, both GELU chains, that the residual is the tokens tensor,
// hgconv_supported, and that no tensor inside has a reader outside or is a network output.  Two spellings of AdaHGConv's reshapes:
//  (a) batch-correct: He (B, E, D) -> (B E, D, 1, 1) for edge_proj, x_new = matmul(A (B, N, E), He' (B, E, D)) -> (B N, D, 1, 1);
//  (b) the reference's literal ones, (E, B, D, 1) and a 2-d matmul of (N B, E) with (E, D), which are that network only at B == 1.
// fp16 explicit-batch engines only, not kINT8, and not with TRTX_HGCONV=0; anything else keeps the generic linear path.
bool match_hgconv_at(const NetView& g, int li, HgconvFuse* h, std::vector<int>* used) {
    const Network& net = g.net;
    auto dims = [&](int t) -> const Dims& { return net.tensors[t].dims; };
    auto is = [](const Dims& d, std::initializer_list<int64_t> want) {
        if (d.nb != (int)want.size()) return false;
        int k = 0;
        for (int64_t v : want)
            if (d.d[k++] != v) return false;
        return true;
    };
    auto layer_of = [&](int t, int kind) {   // the layer of `kind` that produces tensor t, or -1
        const int l = g.producer(t);
        return l >= 0 && net.layers[l].kind == kind ? l : -1;
    };
    auto view_src = [&](int t, int* l) {   // t = a reshape-only shuffle of the returned tensor, or -1
        *l = layer_of(t, L_SHUFFLE);
        if (*l < 0) return -1;
        const LayerDef& s = net.layers[*l];
        return ident(s.perm1, dims(s.inputs[0]).nb) && ident(s.perm2, dims(t).nb) ? s.inputs[0] : -1;
    };
    auto linear = [&](int l, int64_t out, int64_t in) {   // a fully connected layer out x in, with a bias of `out` values or none
        const LayerDef& fc = net.layers[l];
        return fc.nb_out == out && (int64_t)fc.w0.size() == out * in && (fc.w1.empty() || (int64_t)fc.w1.size() == out);
    };
    // x_out and the residual add
    const LayerDef& xo = net.layers[li];
    if (xo.kind != L_SHUFFLE || xo.reshape.nb != 4 || !perm_is(xo.perm1, {0, 2, 1}) || !ident(xo.perm2, 4)) return false;
    const Dims& dimg = dims(xo.outputs[0]);
    if (dimg.nb != 4) return false;
    const int64_t B = dimg.d[0], D = dimg.d[1], N = dimg.d[2] * dimg.d[3];
    const int l_add = layer_of(xo.inputs[0], L_ELEMENTWISE);
    if (l_add < 0 || net.layers[l_add].op != TRTX_ELEMENTWISE_SUM || !is(dims(xo.inputs[0]), {B, N, D})) return false;
    int l_tok = -1, t_fin = -1;
    for (int s = 0; s < 2 && l_tok < 0; ++s) {
        const int l = layer_of(net.layers[l_add].inputs[s], L_SHUFFLE);
        if (l < 0) continue;
        const LayerDef& tk = net.layers[l];
        if (ident(tk.perm1, 4) && tk.reshape.nb == 3 && perm_is(tk.perm2, {0, 2, 1}) && dims(tk.inputs[0]) == dimg) {
            l_tok = l;
            t_fin = net.layers[l_add].inputs[1 - s];
        }
    }
    if (l_tok < 0) return false;
    const int T = net.layers[l_tok].outputs[0];
    if (!is(dims(T), {B, N, D})) return false;
    // back from the residual's other operand: reshape <- GELU <- node_proj <- reshape <- x_new = matmul(A, He')
    int l_fin, l_xn4, l_a2 = -1, l_he2, l_he4, l_lgv, l_xhf, l_in4, l_po, l_ctx4;
    GeluFuse g1, g2;
    const int t_g2 = view_src(t_fin, &l_fin);
    if (t_g2 < 0 || !(is(dims(t_fin), {B, N, D}) || (B == 1 && is(dims(t_fin), {1, N, D}))) || !is(dims(t_g2), {B * N, D, 1, 1}) ||
        !match_tanh_gelu(g, g.producer(t_g2), &g2))
        return false;
    const int l_node = layer_of(g2.in, L_FULLY_CONNECTED);
    if (l_node < 0 || !linear(l_node, D, D) || !is(dims(net.layers[l_node].inputs[0]), {B * N, D, 1, 1})) return false;
    const int t_xnew = view_src(net.layers[l_node].inputs[0], &l_xn4);
    if (t_xnew < 0) return false;
    const int l_m2 = layer_of(t_xnew, L_MATMUL);
    if (l_m2 < 0 || !plain_matmul(net.layers[l_m2])) return false;
    int t_a = net.layers[l_m2].inputs[0];
    const int t_he2 = net.layers[l_m2].inputs[1];
    const bool literal = dims(t_xnew).nb == 2;   // spelling (b)
    if (literal) {
        if (B != 1 || !is(dims(t_xnew), {N, D}) || !is(dims(t_he2), {dims(t_he2).d[0], D})) return false;
        const int64_t E2 = dims(t_he2).d[0];
        if (!is(dims(t_a), {N, E2})) return false;
        t_a = view_src(t_a, &l_a2);
        if (t_a < 0) return false;
    } else if (!is(dims(t_xnew), {B, N, D})) {
        return false;
    }
    if (dims(t_a).nb != 3) return false;
    const int64_t E = dims(t_a).d[2];
    if (!is(dims(t_a), {B, N, E}) || !(literal ? is(dims(t_he2), {E, D}) : is(dims(t_he2), {B, E, D}))) return false;
    // He' = reshape <- GELU <- edge_proj <- reshape <- He = matmul(A^T, tokens)
    const int t_g1 = view_src(t_he2, &l_he2);
    if (t_g1 < 0 || !is(dims(t_g1), {B * E, D, 1, 1}) || !match_tanh_gelu(g, g.producer(t_g1), &g1)) return false;
    const int l_edge = layer_of(g1.in, L_FULLY_CONNECTED);
    if (l_edge < 0 || !linear(l_edge, D, D)) return false;
    const int t_he4 = net.layers[l_edge].inputs[0];
    if (!(is(dims(t_he4), {B * E, D, 1, 1}) || (B == 1 && is(dims(t_he4), {E, 1, D, 1})))) return false;
    const int t_he = view_src(t_he4, &l_he4);
    if (t_he < 0 || !is(dims(t_he), {B, E, D})) return false;
    const int l_m1 = layer_of(t_he, L_MATMUL);
    if (l_m1 < 0 || net.layers[l_m1].mm_op[0] != TRTX_MATMUL_TRANSPOSE || net.layers[l_m1].mm_op[1] != TRTX_MATMUL_NONE ||
        net.layers[l_m1].inputs[0] != t_a || net.layers[l_m1].inputs[1] != T)
        return false;
    // A = softmax over the nodes of the mean over the heads of (X_heads P_heads^T) / scaling
    const int l_sm = layer_of(t_a, L_SOFTMAX);
    if (l_sm < 0 || net.layers[l_sm].axis != (1 << 1)) return false;
    const int l_red = layer_of(net.layers[l_sm].inputs[0], L_REDUCE);
    if (l_red < 0 || net.layers[l_red].op != TRTX_REDUCE_AVG || net.layers[l_red].axis != (1 << 1) || net.layers[l_red].keep_dims) return false;
    const int t_lgv = net.layers[l_red].inputs[0];
    if (dims(t_lgv).nb != 4) return false;
    const int64_t heads = dims(t_lgv).d[1];
    if (heads < 1 || D % heads != 0 || !is(dims(t_lgv), {B, heads, N, E})) return false;
    const int64_t hd = D / heads;
    const int t_lgs = view_src(t_lgv, &l_lgv);
    if (t_lgs < 0 || !is(dims(t_lgs), {B * heads, N, E})) return false;
    const int l_div = layer_of(t_lgs, L_ELEMENTWISE);
    if (l_div < 0 || net.layers[l_div].op != TRTX_ELEMENTWISE_DIV) return false;
    const int l_sc = layer_of(net.layers[l_div].inputs[1], L_CONSTANT);
    if (l_sc < 0 || net.layers[l_sc].w0.size() != 1 || !(net.layers[l_sc].w0[0] > 0.f)) return false;
    const int l_m0 = layer_of(net.layers[l_div].inputs[0], L_MATMUL);
    if (l_m0 < 0 || !plain_matmul(net.layers[l_m0])) return false;
    const int t_xhf = net.layers[l_m0].inputs[0], t_phf = net.layers[l_m0].inputs[1];
    if (!is(dims(t_xhf), {B * heads, N, hd}) || !is(dims(t_phf), {B * heads, hd, E})) return false;
    // the node side: tokens -> (B N, D, 1, 1) -> pre_head_proj -> (B, N, heads, hd) -> {0, 2, 1, 3} -> (B heads, N, hd)
    const int t_xh = view_src(t_xhf, &l_xhf);
    if (t_xh < 0 || !is(dims(t_xh), {B, heads, N, hd})) return false;
    const int l_xh = layer_of(t_xh, L_SHUFFLE);
    if (l_xh < 0 || !ident(net.layers[l_xh].perm1, 4) || net.layers[l_xh].reshape.nb != 4 || !perm_is(net.layers[l_xh].perm2, {0, 2, 1, 3})) return false;
    const int l_pre = layer_of(net.layers[l_xh].inputs[0], L_FULLY_CONNECTED);
    if (l_pre < 0 || !linear(l_pre, D, D) || !is(dims(net.layers[l_pre].inputs[0]), {B * N, D, 1, 1})) return false;
    if (view_src(net.layers[l_pre].inputs[0], &l_in4) != T) return false;
    // the prototype side: (B, E, D) -> (B, E, heads, hd) -> {0, 2, 1, 3} -> (B heads, E, hd) -> {0, 2, 1}
    const int l_phf = layer_of(t_phf, L_SHUFFLE);
    if (l_phf < 0 || !ident(net.layers[l_phf].perm1, 4) || net.layers[l_phf].reshape.nb != 3 || !perm_is(net.layers[l_phf].perm2, {0, 2, 1})) return false;
    const int t_ph = net.layers[l_phf].inputs[0];
    const int l_ph = layer_of(t_ph, L_SHUFFLE);
    if (l_ph < 0 || !is(dims(t_ph), {B, heads, E, hd}) || !ident(net.layers[l_ph].perm1, 3) || net.layers[l_ph].reshape.nb != 4 ||
        !perm_is(net.layers[l_ph].perm2, {0, 2, 1, 3}))
        return false;
    const int t_protos = net.layers[l_ph].inputs[0];
    const int l_protos = layer_of(t_protos, L_ELEMENTWISE);
    if (l_protos < 0 || net.layers[l_protos].op != TRTX_ELEMENTWISE_SUM || !is(dims(t_protos), {B, E, D})) return false;
    int l_base = -1, t_po = -1;
    for (int s = 0; s < 2 && l_base < 0; ++s) {
        l_base = layer_of(net.layers[l_protos].inputs[s], L_CONSTANT);
        t_po = net.layers[l_protos].inputs[1 - s];
    }
    if (l_base < 0 || !is(dims(net.layers[l_base].outputs[0]), {1, E, D}) || !is(dims(t_po), {B, E, D})) return false;
    const int t_fcc = view_src(t_po, &l_po);
    if (t_fcc < 0 || !is(dims(t_fcc), {B, E * D, 1, 1})) return false;
    const int l_ctx = layer_of(t_fcc, L_FULLY_CONNECTED);
    if (l_ctx < 0 || !linear(l_ctx, E * D, 2 * D) || !is(dims(net.layers[l_ctx].inputs[0]), {B, 2 * D, 1, 1})) return false;
    const int t_cat = view_src(net.layers[l_ctx].inputs[0], &l_ctx4);
    if (t_cat < 0 || !is(dims(t_cat), {B, 2 * D})) return false;
    const int l_cat = layer_of(t_cat, L_CONCAT);
    if (l_cat < 0 || net.layers[l_cat].axis != 1 || net.layers[l_cat].inputs.size() != 2) return false;
    const int l_mean = layer_of(net.layers[l_cat].inputs[0], L_REDUCE), l_max = layer_of(net.layers[l_cat].inputs[1], L_REDUCE);
    auto node_reduce = [&](int l, int op) {
        return l >= 0 && net.layers[l].op == op && net.layers[l].axis == (1 << 1) && !net.layers[l].keep_dims && net.layers[l].inputs[0] == T;
    };
    if (!node_reduce(l_mean, TRTX_REDUCE_AVG) || !node_reduce(l_max, TRTX_REDUCE_MAX)) return false;
    if (!hgconv_supported((int)D, (int)E) || B * N > INT32_MAX) return false;
    // the claim: every layer once, and nothing inside is read from outside or is a network output
    *used = {l_tok, l_mean, l_max, l_cat, l_ctx4, l_ctx, l_po, l_base, l_protos, l_in4, l_pre, l_xh, l_ph, l_xhf, l_phf, l_m0, l_sc, l_div, l_lgv, l_red,
             l_sm, l_m1, l_he4, l_edge, l_he2, l_m2, l_xn4, l_node, l_fin, l_add, li};
    if (l_a2 >= 0) used->push_back(l_a2);
    for (const GeluFuse* c : {&g1, &g2}) used->insert(used->end(), c->layers.begin(), c->layers.end());
    std::vector<int> sorted(*used);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return false;
    for (int u : *used) {
        if (u == li) continue;
        const int t = net.layers[u].outputs[0];
        if (net.tensors[t].is_output) return false;
        for (int r : g.consumers[t])
            if (!std::binary_search(sorted.begin(), sorted.end(), r)) return false;
    }
    h->x = net.layers[l_tok].inputs[0];
    h->out = xo.outputs[0];
    h->N = (int)N;
    h->D = (int)D;
    h->E = (int)E;
    h->logit_scale = 1.0f / ((float)heads * net.layers[l_sc].w0[0]);
    h->l_ctx = l_ctx;
    h->l_proto = l_base;
    h->l_pre = l_pre;
    h->l_edge = l_edge;
    h->l_node = l_node;
    return true;
}

void match_hgconv(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    if (!net.explicit_batch || g.dt != DT_F16 || net.int8 || !g.opt.hgconv) return;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        HgconvFuse h;
        std::vector<int> used;
        if (f.absorbed[li] || !match_hgconv_at(g, (int)li, &h, &used)) continue;
        bool free = true;
        for (int u : used) free = free && !f.absorbed[u];
        if (!free) continue;
        for (int u : used) f.absorbed[u] = true;
        f.hgconv_at[li] = (int)f.hgconvs.size();
        f.hgconvs.push_back(h);
    }
}

// A GELU chain that no hypergraph convolution claimed becomes one activation op (ACT_GELU_TANH) at its last layer, in the layout its input has.
void match_gelu_chains(const NetView& g, Fusions& f) {
    for (size_t li = 0; li < g.net.layers.size(); ++li) {
        GeluFuse c;
        if (f.absorbed[li] || !match_tanh_gelu(g, (int)li, &c)) continue;
        bool free = true;
        for (int u : c.layers) free = free && !f.absorbed[u];
        if (!free) continue;
        for (int u : c.layers) f.absorbed[u] = true;
        f.gelu_at[li] = (int)f.gelus.size();
        f.gelus.push_back(c);
    }
}

// a + gate (.) b on images with a constant gate of one element (FullPad_Tunnel, yolov13/src/block.cpp:889-900) or one element per channel (the gamma
// residual of A2C2f, block.cpp:473-484), the product in either operand order on either side of the sum: one gated-add op at the sum instead of a broadcast
// product on the LINEAR path (two layout passes) and an element-wise sum.  The product must have no other reader and the map more than one pixel.  fp32 and fp16 engines, not kINT8, and
// not with TRTX_GATED_ADD=0.  Runs before the convolution fusion, which would otherwise take the sum as a residual epilogue.
void match_gated_add(const NetView& g, Fusions& f) {
    const Network& net = g.net;
    if (!g.opt.gated_add || net.int8) return;
    auto ew = [&](int l, int op) { return l >= 0 && !f.absorbed[l] && net.layers[l].kind == L_ELEMENTWISE && net.layers[l].op == op && net.layers[l].inputs.size() == 2; };
    for (size_t li = 0; li < net.layers.size(); ++li) {
        if (!ew((int)li, TRTX_ELEMENTWISE_SUM)) continue;
        const LayerDef& sum = net.layers[li];
        const Dims& d = net.tensors[sum.outputs[0]].dims;
        // feature maps only: a (rows, D, 1, 1) tensor is a token matrix of the linear path (the Linears of AdaHGConv and the GELU chains behind them,
        // whose x + 0.044715 x^3 has this very shape); those keep their element-wise ops
        if (d.nb != (net.explicit_batch ? 4 : 3) || d.d[d.nb - 2] * d.d[d.nb - 1] == 1) continue;
        const int ca = d.nb - 3;
        for (int s = 0; s < 2 && f.gated_at[li] < 0; ++s) {
            const int t_prod = sum.inputs[s], l_prod = g.producer(t_prod), a = sum.inputs[1 - s];
            if (!ew(l_prod, TRTX_ELEMENTWISE_PROD) || !g.only_used_by(t_prod, {(int)li}) || !(net.tensors[a].dims == d)) continue;
            for (int q = 0; q < 2; ++q) {
                const int l_gate = g.producer(net.layers[l_prod].inputs[q]), b = net.layers[l_prod].inputs[1 - q];
                if (l_gate < 0 || net.layers[l_gate].kind != L_CONSTANT || f.absorbed[l_gate] || !(net.tensors[b].dims == d)) continue;
                const Dims& cd = net.layers[l_gate].out_dims;
                bool ok = cd.nb == d.nb;
                for (int k = 0; ok && k < d.nb; ++k) ok = cd.d[k] == 1 || (k == ca && cd.d[k] == d.d[k]);
                if (!ok) continue;
                GatedAddFuse r;
                r.a = a;
                r.b = b;
                r.out = sum.outputs[0];
                r.gate_layer = l_gate;
                f.absorbed[l_prod] = f.absorbed[li] = true;
                if (g.only_used_by(net.layers[l_gate].outputs[0], {l_prod})) f.absorbed[l_gate] = true;   // (a gate with another reader stays a constant tensor)
                f.gated_at[li] = (int)f.gated_adds.size();
                f.gated_adds.push_back(r);
                break;
            }
        }
    }
}

// A spelled-out softmax that no attention claimed becomes the softmax op at its division (LINEAR fp32, like ISoftMaxLayer's).
void match_softmax_chains(const NetView& g, Fusions& f) {
    for (size_t li = 0; li < g.net.layers.size(); ++li) {
        SoftmaxChainFuse c;
        if (f.absorbed[li] || !match_exp_softmax(g, (int)li, &c)) continue;
        bool free = true;
        for (int u : c.layers) free = free && !f.absorbed[u];
        if (!free) continue;
        for (int u : c.layers) f.absorbed[u] = true;
        f.softmax_at[li] = (int)f.softmax_chains.size();
        f.softmax_chains.push_back(c);
    }
}

}  // namespace

bool match_exp_softmax(const NetView& g, int last, SoftmaxChainFuse* f) {
    const Network& net = g.net;
    auto ew = [&](int l, int op) { return l >= 0 && net.layers[l].kind == L_ELEMENTWISE && net.layers[l].op == op && net.layers[l].inputs.size() == 2; };
    // layer l = a keepDims reduction `op` of tensor `of` over exactly one axis: that axis, or -1
    auto reduce_of = [&](int l, int op, int of) {
        if (l < 0 || net.layers[l].kind != L_REDUCE || net.layers[l].op != op || !net.layers[l].keep_dims || net.layers[l].inputs[0] != of) return -1;
        const int32_t mask = net.layers[l].axis;
        const int nb = net.tensors[of].dims.nb;
        for (int k = 0; k < nb; ++k)
            if (mask == (1 << k)) return k;
        return -1;
    };
    if (!ew(last, TRTX_ELEMENTWISE_DIV)) return false;
    const int t_exp = net.layers[last].inputs[0], l_sum = g.producer(net.layers[last].inputs[1]);
    const int axis = reduce_of(l_sum, TRTX_REDUCE_SUM, t_exp);
    if (axis < 0) return false;
    const int l_exp = g.producer(t_exp);
    if (l_exp < 0 || net.layers[l_exp].kind != L_UNARY || net.layers[l_exp].op != TRTX_UNARY_EXP) return false;
    const int l_sub = g.producer(net.layers[l_exp].inputs[0]);
    if (!ew(l_sub, TRTX_ELEMENTWISE_SUB)) return false;
    const int x = net.layers[l_sub].inputs[0], l_max = g.producer(net.layers[l_sub].inputs[1]);
    if (reduce_of(l_max, TRTX_REDUCE_MAX, x) != axis) return false;
    f->layers = {l_max, l_sub, l_exp, l_sum, last};
    for (int u : f->layers) {
        if (u == last) continue;
        const int t = net.layers[u].outputs[0];
        if (net.tensors[t].is_output) return false;
        for (int r : g.consumers[t])
            if (std::find(f->layers.begin(), f->layers.end(), r) == f->layers.end()) return false;
    }
    f->in = x;
    f->out = net.layers[last].outputs[0];
    f->axis = axis;
    return true;
}

bool match_tanh_gelu(const NetView& g, int last, GeluFuse* f) {
    const Network& net = g.net;
    auto ew = [&](int l, int op) { return l >= 0 && net.layers[l].kind == L_ELEMENTWISE && net.layers[l].op == op && net.layers[l].inputs.size() == 2; };
    // layer l = `op` of a tensor and a one-element constant of value v (either order): the tensor, or -1
    auto with_const = [&](int l, int op, float v, int* cl) {
        if (!ew(l, op)) return -1;
        for (int s = 0; s < 2; ++s) {
            const int c = g.producer(net.layers[l].inputs[s]);
            if (c >= 0 && net.layers[c].kind == L_CONSTANT && net.layers[c].w0.size() == 1 && net.layers[c].w0[0] == v) {
                *cl = c;
                return net.layers[l].inputs[1 - s];
            }
        }
        return -1;
    };
    int c_half, c_one, c_sqrt, c_kappa;
    const int t_hx = with_const(last, TRTX_ELEMENTWISE_PROD, 0.5f, &c_half);
    if (t_hx < 0) return false;
    const int l_hx = g.producer(t_hx);
    if (!ew(l_hx, TRTX_ELEMENTWISE_PROD)) return false;
    int x = -1, l_add = -1, t_tanh = -1;
    for (int s = 0; s < 2 && l_add < 0; ++s) {
        const int la = g.producer(net.layers[l_hx].inputs[s]);
        const int tt = with_const(la, TRTX_ELEMENTWISE_SUM, 1.0f, &c_one);
        if (tt >= 0) {
            l_add = la;
            t_tanh = tt;
            x = net.layers[l_hx].inputs[1 - s];
        }
    }
    if (l_add < 0) return false;
    const int l_tanh = g.producer(t_tanh);
    if (l_tanh < 0 || net.layers[l_tanh].kind != L_ACTIVATION || net.layers[l_tanh].op != TRTX_ACTIVATION_TANH) return false;
    const int l_si = g.producer(net.layers[l_tanh].inputs[0]);
    const int t_inner = with_const(l_si, TRTX_ELEMENTWISE_PROD, 0.797885f, &c_sqrt);
    if (t_inner < 0) return false;
    const int l_inner = g.producer(t_inner);
    if (!ew(l_inner, TRTX_ELEMENTWISE_SUM)) return false;
    const LayerDef& in = net.layers[l_inner];
    if (in.inputs[0] != x && in.inputs[1] != x) return false;
    const int t_sx3 = in.inputs[0] == x ? in.inputs[1] : in.inputs[0];
    const int l_sx3 = g.producer(t_sx3);
    const int t_x3 = with_const(l_sx3, TRTX_ELEMENTWISE_PROD, 0.044715f, &c_kappa);
    if (t_x3 < 0) return false;
    const int l_x3 = g.producer(t_x3);
    if (!ew(l_x3, TRTX_ELEMENTWISE_PROD)) return false;
    const LayerDef& c3 = net.layers[l_x3];
    if (c3.inputs[0] != x && c3.inputs[1] != x) return false;
    const int l_x2 = g.producer(c3.inputs[0] == x ? c3.inputs[1] : c3.inputs[0]);
    if (!ew(l_x2, TRTX_ELEMENTWISE_PROD) || net.layers[l_x2].inputs[0] != x || net.layers[l_x2].inputs[1] != x) return false;
    f->layers = {l_x2, l_x3, c_kappa, l_sx3, l_inner, c_sqrt, l_si, l_tanh, c_one, l_add, l_hx, c_half, last};
    std::vector<int> sorted(f->layers);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return false;
    for (int u : f->layers) {
        if (u == last) continue;
        const int t = net.layers[u].outputs[0];
        if (net.tensors[t].is_output) return false;
        for (int r : g.consumers[t])
            if (!std::binary_search(sorted.begin(), sorted.end(), r)) return false;
    }
    f->in = x;
    f->out = net.layers[last].outputs[0];
    return true;
}

// The order is part of the behaviour - a layer belongs to the first matcher that claims it: the task head and the detection head
// and the YOLOv9 head (before conv fusion: they claim the DFL 1x1 convolutions), the anchor heads of YOLOv5 and YOLOv7 (they claim their plugin layer only), PSA attention, area
// attention, YOLOv13's area attention on separate qk and v (after the packed form, and before the hypergraph convolution, the softmax chains and the gated adds: its spelled-out softmax and its scale must still be unclaimed), the hypergraph convolution (it claims four fully connected layers and two GELU chains) and then the GELU chains left standing alone, the spelled-out softmax chains, the gated adds (before convolution fusion, which would take their sum as a residual), the ReOrg fold (slices and a concat in front of a convolution that no other matcher looks at), the RepVGGDW fold (it claims the 3x3 branch and the sum, and convolution fusion then continues the 7x7 convolution at the sum's output), convolution fusion, and last the concat-activation rewrite, which edits the convolution records.
Fusions match_fusions(const NetView& g) {
    Fusions f;
    const size_t nl = g.net.layers.size();
    f.absorbed.assign(nl, false);
    f.pad_cout.assign(nl, false);
    f.reorg_src.assign(nl, -1);
    f.repdw_at.assign(nl, -1);
    f.group_at = f.yolo_at = f.attn_at = f.attn_split_at = f.yolo5_at = f.yolo9_at = f.hgconv_at = f.gelu_at = f.softmax_at = f.gated_at = std::vector<int>(nl, -1);
    match_yolo_heads(g, true, f);
    match_yolo_heads(g, false, f);
    match_yolo9_heads(g, f);
    match_yolo5_heads(g, f);
    match_yolo7_heads(g, f);
    match_darknet_heads(g, f);
    match_psa_attention(g, f);
    match_area_attention(g, f);
    match_aattn_split(g, f);
    match_hgconv(g, f);
    match_gelu_chains(g, f);
    match_softmax_chains(g, f);
    match_gated_add(g, f);
    match_reorg_fold(g, f);
    match_repvggdw_fold(g, f);
    match_conv_fusion(g, f);
    match_concat_activation(g, f);
    return f;
}

}  // namespace trtx
