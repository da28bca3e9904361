// Network -> Plan lowering: emission of plan tensors and ops, layer by layer.  See plan.h for what this stands in for, lower_match.h for
// the fusions recognised before the walk and plan_passes.h for what happens to the op list after it.
#include <string.h>

#include <algorithm>

#include "lower_match.h"
#include "plan_passes.h"

namespace trtx {

namespace {

int ew_code(int trt_op) {
    switch (trt_op) {
        case TRTX_ELEMENTWISE_SUM: return EW_SUM;
        case TRTX_ELEMENTWISE_PROD: return EW_PROD;
        case TRTX_ELEMENTWISE_MAX: return EW_MAX;
        case TRTX_ELEMENTWISE_MIN: return EW_MIN;
        case TRTX_ELEMENTWISE_SUB: return EW_SUB;
        case TRTX_ELEMENTWISE_DIV: return EW_DIV;
        case TRTX_ELEMENTWISE_POW: return EW_POW;
        default: return -1;
    }
}

void dense_strides(const Dims& d, long* st) {   // element strides of a dense row-major tensor
    long s = 1;
    for (int k = d.nb - 1; k >= 0; --k) {
        st[k] = s;
        s *= d.d[k];
    }
}

long extent(const Dims& d, int a, int b) {   // product of the dims [a, b)
    long v = 1;
    for (int k = a; k < b; ++k) v *= d.d[k];
    return v;
}

struct Lowerer {
    const Network& net;
    Plan& plan;
    const NetView g;             // the network as the matchers read it
    const Options& opt = g.opt;
    const int dt = g.dt;         // dtype of NHWC tensors
    Fusions fu;                  // what the matchers claimed (run() asks them before it emits the first layer)
    std::vector<int> pt_of, pt_lin, pt_nhwc;
    std::vector<char> stride_folded;   // per layer: a 1x1 stride-s convolution whose producer emitted only the pixels it reads -> stride 1
    std::string err;

    Lowerer(const Network& n, Plan& p)
        : net(n), plan(p), g(n), pt_of(n.tensors.size(), -1), pt_lin(pt_of), pt_nhwc(pt_of), stride_folded(n.layers.size(), 0) {}

    bool fail(const std::string& m) {
        if (err.empty()) err = m;
        return false;
    }

    // ---- tensors ---------------------------------------------------------------------------------
    int new_tensor(int net_t, const Dims& d, int layout, bool batched) {
        PTensor t;
        t.id = (int)plan.tensors.size();
        t.net_tensor = net_t;
        t.name = net_t >= 0 ? net.tensors[net_t].name : "";
        t.dims = d;
        t.layout = layout;
        t.batched = batched;
        if (layout == LAY_NHWC) {
            t.dtype = dt;
            if (net.explicit_batch) {
                t.nfix = (int)d.d[0];
                t.C = (int)d.d[1];
                t.H = (int)d.d[2];
                t.W = (int)d.d[3];
                t.batched = false;
            } else {
                t.C = (int)d.d[d.nb - 3];
                t.H = (int)d.d[d.nb - 2];
                t.W = (int)d.d[d.nb - 1];
                if (d.nb == 4) t.nmul = (int)d.d[0];
            }
            t.Calloc = dt == DT_F16 ? (t.C + 7) / 8 * 8 : (t.C + 3) / 4 * 4;   // a pixel's channels start on a 16-byte boundary
        } else {
            t.dtype = DT_F32;
            if (net.explicit_batch) t.batched = false;
        }
        plan.tensors.push_back(t);
        return t.id;
    }
    PTensor view_of(int parent, int net_t) const {
        PTensor t = plan.tensors[parent];
        t.id = (int)plan.tensors.size();
        t.net_tensor = net_t;
        t.name = net_t >= 0 ? net.tensors[net_t].name : "";
        t.parent = parent;
        return t;
    }
    int new_view_nhwc(int parent, int coff, int C, int net_t) {
        PTensor t = view_of(parent, net_t);
        t.coff = coff;
        t.C = C;
        t.Calloc = 0;
        t.pad_zeroed = false;
        t.dims.d[t.dims.nb - 3] = C;
        plan.tensors.push_back(t);
        return t.id;
    }
    int new_view_lin(int parent, const Dims& d, int net_t) {
        PTensor t = view_of(parent, net_t);
        t.eoff = 0;
        t.dims = d;
        plan.tensors.push_back(t);
        return t.id;
    }

    POp& add_op(int kind, const std::string& name, std::vector<int> in, std::vector<int> out) {
        POp op;
        op.kind = kind;
        op.name = name;
        op.in = std::move(in);
        op.out = std::move(out);
        op.dtype = dt;
        plan.ops.push_back(std::move(op));
        return plan.ops.back();
    }

    int need_nhwc(int net_t) {
        const int p = pt_of[net_t];
        if (plan.tensors[p].layout == LAY_NHWC) return p;
        if (pt_nhwc[net_t] >= 0) return pt_nhwc[net_t];
        const int q = new_tensor(net_t, plan.tensors[p].dims, LAY_NHWC, plan.tensors[p].batched);
        plan.tensors[q].pad_zeroed = true;
        POp& op = add_op(OP_TO_NHWC, "to_nhwc:" + net.tensors[net_t].name, {p}, {q});
        op.bytes = (double)plan.tensors[p].dims.volume() * (4 + (dt == DT_F16 ? 2 : 4));
        return pt_nhwc[net_t] = q;
    }
    int need_lin(int net_t) {
        const int p = pt_of[net_t];
        if (plan.tensors[p].layout == LAY_LINEAR) return p;
        if (pt_lin[net_t] >= 0) return pt_lin[net_t];
        const int q = new_tensor(net_t, plan.tensors[p].dims, LAY_LINEAR, plan.tensors[p].batched || plan.tensors[p].nfix == 0);
        POp& op = add_op(OP_TO_LINEAR, "to_linear:" + net.tensors[net_t].name, {p}, {q});
        op.bytes = (double)plan.tensors[p].dims.volume() * (4 + (dt == DT_F16 ? 2 : 4));
        return pt_lin[net_t] = q;
    }

    // try to make tensor `child` live inside `parent` at channel `coff`
    bool try_place(int child, int parent, int coff) {
        int off = 0;
        const int top = owner_of(plan, child, &off);
        PTensor& t = plan.tensors[top];
        const PTensor& c = plan.tensors[child];
        if (t.layout != LAY_NHWC) return false;
        // only a whole, freely placeable owner may move.  Every producer writes exactly C channels (ragged channel
        // counts take the element-wise store paths), except the layout pass that zero-fills its padding.
        if (off != 0 || c.C != t.C || t.pad_zeroed || is_binding_tensor(plan, top)) return false;
        if (owner_of(plan, parent, nullptr) == top) return false;  // would create a cycle
        t.parent = parent;
        t.coff = coff;
        return true;
    }

    bool emit_attention(const AttentionFuse& f) {
        const int in = need_nhwc(f.qkv);
        const int o = new_tensor(f.out_o, net.tensors[f.out_o].dims, LAY_NHWC, true);
        const int v = new_tensor(f.out_v, net.tensors[f.out_v].dims, LAY_NHWC, true);
        POp& op = add_op(OP_ATTENTION, "attention:" + net.tensors[f.qkv].name, {in}, {o, v});
        op.i[0] = f.heads; op.i[1] = f.N; op.i[2] = f.kd; op.i[3] = f.hd;
        op.i[4] = f.area;
        op.f[0] = f.scale;
        const double B = plan.tensors[in].nfix;
        op.flops = 2.0 * B * f.heads * (double)f.N * (f.N / std::max(f.area, 1)) * (f.kd + f.hd);   // area * (N / area)^2 score and value products
        op.bytes = 2.0 * B * f.N * ((double)plan.tensors[in].C + 2.0 * f.heads * f.hd);
        pt_of[f.out_o] = o;
        pt_of[f.out_v] = v;
        return true;
    }

    // YOLOv13's area attention at its last shuffle: the qk and v convolutions' NHWC images in, O out as one NHWC image of its own (a residual epilogue or a
    // concat behind it takes it like any other); v is read where it is, no V image is written.
    bool emit_attention_split(const AttentionSplitFuse& f) {
        const int qk = need_nhwc(f.qk), v = need_nhwc(f.v);
        const int o = new_tensor(f.out, net.tensors[f.out].dims, LAY_NHWC, true);
        POp& op = add_op(OP_ATTENTION_SPLIT, "attention_split:" + net.tensors[f.qk].name, {qk, v}, {o});
        op.i[0] = f.heads; op.i[1] = f.N; op.i[2] = f.hd; op.i[3] = f.hd;   // kd == hd: q, k and v are hd channels per head
        op.i[4] = f.area;
        op.i[5] = f.heads * f.hd;   // k's first channel within the qk tensor
        op.f[0] = f.scale;
        const double B = plan.tensors[qk].nfix;
        op.flops = 2.0 * B * f.heads * (double)f.N * (f.N / f.area) * (2 * f.hd);   // as emit_attention
        op.bytes = 2.0 * B * f.N * 4.0 * f.heads * f.hd;                             // q, k, v read, O written
        pt_of[f.out] = o;
        return true;
    }

    // The hypergraph convolution at its x_out shuffle: the NHWC image AdaHGComputation read in, the NHWC image it produced out (a concat behind it
    // takes the op's output as a channel slice like any other NHWC tensor); the weights stay in their layers until pack_weights.
    bool emit_hgconv(const HgconvFuse& f) {
        const int in = need_nhwc(f.x);
        const int out = new_tensor(f.out, net.tensors[f.out].dims, LAY_NHWC, true);
        POp& op = add_op(OP_HGCONV, "hgconv:" + net.tensors[f.x].name, {in}, {out});
        op.i[0] = f.N; op.i[1] = f.D; op.i[2] = f.E;
        op.f[0] = f.logit_scale;
        op.iv = {f.l_ctx, f.l_proto, f.l_pre, f.l_edge, f.l_node};
        const int B = plan.tensors[in].nfix;
        op.ws_bytes = hgconv_workspace_bytes(B, f.N, f.D, f.E);
        if (op.ws_bytes == 0) return fail(op.name + ": no workspace size for a matched hypergraph convolution");
        const double ed = (double)f.E * f.D;
        // context_net, Q, the edge and node projections per image, and the three E-wide passes over the N x D tokens
        op.flops = 2.0 * B * (ed * 2 * f.D + 3.0 * ed * f.D + 3.0 * f.N * ed);
        op.bytes = 2.0 * B * f.N * f.D * 4;   // X read three times and written once, fp16 (pack_weights adds the weights)
        pt_of[f.out] = out;
        return true;
    }

    // A GELU chain standing alone: one activation op in the layout its input already has
    bool emit_gelu(const GeluFuse& f) {
        const int p = pt_of[f.in];
        const bool nhwc = plan.tensors[p].layout == LAY_NHWC;
        const int out = new_tensor(f.out, net.tensors[f.out].dims, nhwc ? LAY_NHWC : LAY_LINEAR, plan.tensors[p].batched);
        POp& op = add_op(nhwc ? OP_ACT_NHWC : OP_ACT_LIN, net.layers[f.layers.back()].name + " [tanh GELU chain]", {p}, {out});
        op.i[0] = ACT_GELU_TANH;
        pt_of[f.out] = out;
        return true;
    }

    // a + gate (.) b at the sum: three NHWC images; the gate stays in its constant layer until pack_weights.  A concat behind it takes the output as a channel
    // slice like any other NHWC tensor (try_place), and the op then writes at that slice's pixel stride.
    bool emit_gated_add(int li, const GatedAddFuse& f) {
        const int a = need_nhwc(f.a), b = need_nhwc(f.b);
        const int out = new_tensor(f.out, net.tensors[f.out].dims, LAY_NHWC, true);
        POp& op = add_op(OP_GATED_ADD, net.layers[li].name + " [a + gate * b]", {a, b}, {out});
        op.src_layer = f.gate_layer;
        op.bytes = 3.0 * dtype_size(dt) * net.tensors[f.out].dims.volume();
        pt_of[f.out] = out;
        return true;
    }

    bool emit_yolo_head(const YoloHeadFuse& f) {
        const LayerDef& l = net.layers[f.plugin_layer];
        std::vector<int> ins, branches;
        for (int t : f.head_tensor) ins.push_back(need_nhwc(t));
        for (int t : f.branch_tensor) branches.push_back(need_nhwc(t));
        const int out = new_tensor(l.outputs[0], net.tensors[l.outputs[0]].dims, LAY_LINEAR, true);
        const bool task = !f.branch_tensor.empty();
        const HeadOp& head = task ? *head_op(OP_YOLO_TASK_HEAD) : head_op_of(f.params.form);
        POp& op = add_op(head.kind, l.name + head.suffix, ins, {out});
        op.extra_in = branches;
        op.src_layer = f.dfl_conv_layer;
        op.i[0] = f.params.classes;
        op.i[1] = f.params.net_h;
        op.i[2] = f.params.net_w;
        op.i[3] = f.params.max_out;
        op.i[4] = (int)f.params.strides.size();
        for (size_t k = 0; k < f.params.strides.size(); ++k) op.i[5 + k] = f.params.strides[k];
        if (task) {
            op.i[9] = f.params.seg ? 1 : (f.params.pose ? 2 : 3);
            op.i[10] = f.params.pose ? f.params.nk : 0;
            op.f[0] = f.params.kpt_conf;
            for (int t : branches) op.bytes += (double)dtype_size(dt) * plan.tensors[t].dims.volume();
        }
        // explicit batch: the image count is the heads' leading dimension (op.i[11]; 0 = the enqueue's batch)
        if (net.explicit_batch) op.i[11] = plan.tensors[ins[0]].nfix;
        op.ws_bytes = head.stride_ws(net.explicit_batch ? op.i[11] : plan.max_batch, f.params.net_h, f.params.net_w, f.params.strides.data(),
                                                      (int)f.params.strides.size());
        for (int t : ins) op.bytes += (double)dtype_size(dt) * plan.tensors[t].dims.volume();
        op.bytes += 4.0 * net.tensors[l.outputs[0]].dims.volume();
        pt_of[l.outputs[0]] = out;
        return true;
    }

    // The anchor head at its plugin's layer: the detect convolutions' NHWC tensors in, the plugin's LINEAR output out.
    bool emit_yolo5_head(const Yolo5HeadFuse& f) {
        const LayerDef& l = net.layers[f.plugin_layer];
        const YoloParams& pr = f.params;
        const HeadOp& head = head_op_of(pr.form);
        std::vector<int> ins;
        for (int t : f.head_tensor) {
            if (plan.tensors[pt_of[t]].layout != LAY_NHWC) return fail(l.name + ": fused anchor head on a tensor that is not NHWC");
            ins.push_back(pt_of[t]);
        }
        const int out = new_tensor(l.outputs[0], net.tensors[l.outputs[0]].dims, LAY_LINEAR, true);
        POp& op = add_op(head.kind, l.name + head.suffix, ins, {out});
        op.i[0] = pr.classes;
        op.i[1] = pr.net_h;
        op.i[2] = pr.net_w;
        op.i[3] = pr.max_out;
        op.i[4] = (int)ins.size();
        for (size_t k = 0; k < ins.size(); ++k) {
            op.iv.push_back(pr.grid_w[k]);
            op.iv.push_back(pr.grid_h[k]);
        }
        op.fv = pr.anchors;
        // explicit batch: the image count is the heads' leading dimension (op.i[11]; 0 = the enqueue's batch)
        if (net.explicit_batch) op.i[11] = plan.tensors[ins[0]].nfix;
        op.ws_bytes = head.anchor_ws(net.explicit_batch ? op.i[11] : plan.max_batch, pr.grid_w.data(), pr.grid_h.data(), (int)ins.size());
        // what it must read: the three objectness values of every pixel (nothing else of a pixel without a candidate), and what it writes
        for (int t : ins) op.bytes += (double)dtype_size(dt) * plan.tensors[t].H * plan.tensors[t].W * 3;
        op.bytes += 4.0 * net.tensors[l.outputs[0]].dims.volume();
        pt_of[l.outputs[0]] = out;
        return true;
    }

    // The DDetect head at its plugin's layer: the box and class convolutions' NHWC tensors in (`in` = boxes, `extra_in` = classes), the
    // plugin's LINEAR output out; the DFL weights come from src_layer like OP_YOLO_HEAD's.
    bool emit_yolo9_head(const Yolo9HeadFuse& f) {
        const LayerDef& l = net.layers[f.plugin_layer];
        const YoloParams& pr = f.params;
        std::vector<int> boxes, clss;
        for (int t : f.box_tensor) boxes.push_back(need_nhwc(t));
        for (int t : f.cls_tensor) clss.push_back(need_nhwc(t));
        const int out = new_tensor(l.outputs[0], net.tensors[l.outputs[0]].dims, LAY_LINEAR, true);
        POp& op = add_op(OP_YOLO9_HEAD, l.name + head_op_of(YOLO_V9).suffix, boxes, {out});
        op.extra_in = clss;
        op.src_layer = f.dfl_conv_layer;
        op.i[0] = pr.classes;
        op.i[1] = pr.net_h;
        op.i[2] = pr.net_w;
        op.i[3] = pr.max_out;
        op.i[4] = (int)boxes.size();
        op.ws_bytes = trtx_yolov9_head_decode_workspace(plan.max_batch, pr.net_h, pr.net_w);
        // what it must read: every class logit, the box bins of the survivors only (not counted), and what it writes
        for (int t : clss) op.bytes += (double)dtype_size(dt) * plan.tensors[t].H * plan.tensors[t].W * pr.classes;
        op.bytes += 4.0 * net.tensors[l.outputs[0]].dims.volume();
        pt_of[l.outputs[0]] = out;
        return true;
    }

    // ---- per-kind emission ----------------------------------------------------------------------------
    bool emit_conv(const FusedConv& c) {
        const LayerDef& l = net.layers[c.conv_layer];
        // a folded ReOrg (match_reorg_fold): the convolution reads the slices' input with a 2k x 2k stride-2 padding-2p filter
        const int reorg = fu.reorg_src[c.conv_layer];
        const int tin = reorg >= 0 ? reorg : l.inputs[0];
        const int kmul = reorg >= 0 ? 2 : 1;
        // stem: a few-channel fp32 LINEAR input (the image) feeds conv_stem directly, no layout pass
        bool stem = false;
        {
            const PTensor& src = plan.tensors[pt_of[tin]];
            const Dims& di = net.tensors[tin].dims;
            const int cin = (int)di.d[di.nb - 3];
            const bool image = l.kind == L_CONV && di.nb == (net.explicit_batch ? 4 : 3) && src.layout == LAY_LINEAR && pt_nhwc[tin] < 0 && cin <= 4 &&
                               c.residual < 0 && c.act2 == ACT_NONE && l.groups == 1 && l.dilation[0] == 1 && l.dilation[1] == 1;
            stem = dt == DT_F16 && image && (l.nb_out == 8 || l.nb_out == 16 || l.nb_out == 32 || l.nb_out == 64) &&
                   (size_t)l.kernel[0] * kmul * l.kernel[1] * kmul * cin * l.nb_out * 4 <= 48 * 1024;
            // fp32 engines (round 5): kernels/conv_stem_f32.hip, the same idea on the vector ALU - the layer is HBM-bound and 3x padding on the MFMA path
            if (dt == DT_F32 && opt.f32_mfma) stem = image && l.nb_out % 16 == 0 && l.nb_out <= 256;
        }
        const int in = stem ? pt_of[tin] : need_nhwc(tin);
        PTensor ti = plan.tensors[in];
        if (stem) {  // geometry of the LINEAR tensor viewed as an image
            const Dims& di = net.tensors[tin].dims;
            ti.C = (int)di.d[di.nb - 3];
            ti.H = (int)di.d[di.nb - 2];
            ti.W = (int)di.d[di.nb - 1];
        }
        const int out = new_tensor(c.out_tensor, net.tensors[c.out_tensor].dims, LAY_NHWC, true);
        int res = -1;
        if (c.residual >= 0) res = need_nhwc(c.residual);
        std::vector<int> ins = {in};
        if (res >= 0) ins.push_back(res);
        POp& op = add_op(OP_CONV, l.name, ins, {out});
        op.src_layer = c.conv_layer;
        op.scale_layer = c.scale_layer;
        op.fold_layer = c.fold_conv;
        op.fold_scale = c.fold_scale;
        if (c.fold_conv >= 0) op.name += " [RepVGGDW folded]";
        op.stem = stem;
        ConvArgs& a = op.conv;
        const PTensor& to = plan.tensors[out];
        a.H = ti.H;
        a.W = ti.W;
        a.Cin = ti.C;
        a.Ho = to.H;
        a.Wo = to.W;
        a.Cout = to.C;
        // a detect convolution under the fused anchor head (its only reader, which knows the real channel count): the output channels round
        // up to the tensor's 16-byte pixel stride, with zero filter rows and biases, so that 255 channels keep the 16-byte stores
        if (fu.pad_cout[c.conv_layer] && to.Calloc > to.C && c.residual < 0) {
            op.cout_real = to.C;
            a.Cout = to.Calloc;
        }
        if (l.kind == L_FULLY_CONNECTED) {
            a.kh = ti.H;
            a.kw = ti.W;
            a.stride_h = a.stride_w = 1;
            a.pad_h = a.pad_w = 0;
            a.dil_h = a.dil_w = 1;
            a.groups = 1;
        } else {
            a.kh = l.kernel[0];
            a.kw = l.kernel[1];
            a.stride_h = l.stride[0];
            a.stride_w = l.stride[1];
            if (stride_folded[c.conv_layer]) a.stride_h = a.stride_w = 1;   // its input was emitted at the positions it reads (RoIAlign, below)
            a.pad_h = l.padding[0];
            a.pad_w = l.padding[1];
            a.dil_h = l.dilation[0];
            a.dil_w = l.dilation[1];
            a.groups = l.groups;
            if (reorg >= 0) {
                op.name += " [ReOrg folded]";
                op.reorg_cin = ti.C;
                a.kh *= 2;
                a.kw *= 2;
                a.stride_h = a.stride_w = 2;
                a.pad_h *= 2;
                a.pad_w *= 2;
            }
        }
        a.act1 = c.act1;
        a.alpha1 = c.alpha1;
        a.act2 = c.act2;
        a.alpha2 = c.alpha2;
        op.flops = 2.0 * to.nmul * a.Ho * a.Wo * to.C * (double)a.kh * a.kw * (a.Cin / a.groups);
        pt_of[c.out_tensor] = out;
        return true;
    }

    bool emit_activation(const LayerDef& l, int code, float alpha) {   // an activation op in the layout its input already has
        const int p = pt_of[l.inputs[0]];
        const bool nhwc = plan.tensors[p].layout == LAY_NHWC;
        const int out = new_tensor(l.outputs[0], net.tensors[l.outputs[0]].dims, nhwc ? LAY_NHWC : LAY_LINEAR, plan.tensors[p].batched);
        POp& op = add_op(nhwc ? OP_ACT_NHWC : OP_ACT_LIN, l.name, {p}, {out});
        op.i[0] = code;
        op.f[0] = alpha;
        pt_of[l.outputs[0]] = out;
        return true;
    }

    bool emit_softmax(const std::string& name, int t_in, int t_out, int ax) {   // the LINEAR softmax op over dim `ax` of network tensor t_in
        const Dims& di = net.tensors[t_in].dims;
        const int in = need_lin(t_in);
        const int out = new_tensor(t_out, net.tensors[t_out].dims, LAY_LINEAR, plan.tensors[in].batched);
        POp& op = add_op(OP_SOFTMAX, name, {in}, {out});
        op.i[0] = (int)extent(di, 0, ax); op.i[1] = (int)di.d[ax]; op.i[2] = (int)extent(di, ax + 1, di.nb);
        pt_of[t_out] = out;
        return true;
    }

    bool emit_layer(int li) {
        const LayerDef& l = net.layers[li];
        auto out_dims = [&](int s = 0) -> const Dims& { return net.tensors[l.outputs[s]].dims; };
        switch (l.kind) {
            case L_CONV:
            case L_FULLY_CONNECTED:
                return fail(l.name + ": convolution on a non-image tensor is not supported");
            case L_DECONV: {
                const int in = need_nhwc(l.inputs[0]);
                const PTensor ti = plan.tensors[in];
                // kernel == stride, no padding, one group (Mask R-CNN's 2x2/2 ConvTranspose over 2048 channels,
                // rcnn.cpp:209-212): every output sub-position (r, q) is its own 1x1 convolution, so the layer is one MFMA
                // implicit GEMM with Cout' = kh*kw*Cout followed by a depth-to-space shuffle (41.7 ms -> ~0.15 ms there)
                if (dt == DT_F16 && l.groups == 1 && l.kernel[0] == l.stride[0] && l.kernel[1] == l.stride[1] && l.padding[0] == 0 &&
                    l.padding[1] == 0 && l.dilation[0] == 1 && l.dilation[1] == 1 && ti.C % 8 == 0 && l.nb_out % 8 == 0 &&
                    l.kernel[0] * l.kernel[1] > 1) {
                    Dims dmid = net.tensors[l.inputs[0]].dims;
                    dmid.d[dmid.nb - 3] = (int64_t)l.nb_out * l.kernel[0] * l.kernel[1];
                    const int mid = new_tensor(-1, dmid, LAY_NHWC, true);
                    const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                    {
                        POp& op = add_op(OP_CONV, l.name + " [as 1x1]", {in}, {mid});
                        op.src_layer = li;
                        op.from_deconv = true;
                        ConvArgs& a = op.conv;
                        const PTensor& tm = plan.tensors[mid];
                        a.H = ti.H; a.W = ti.W; a.Cin = ti.C; a.Ho = ti.H; a.Wo = ti.W; a.Cout = tm.C;
                        a.kh = a.kw = 1; a.stride_h = a.stride_w = 1; a.pad_h = a.pad_w = 0; a.dil_h = a.dil_w = 1; a.groups = 1;
                        op.flops = 2.0 * tm.nmul * a.Ho * a.Wo * a.Cout * (double)a.Cin;
                    }
                    POp& d2s = add_op(OP_D2S, l.name + " [depth to space]", {mid}, {out});
                    d2s.i[0] = l.kernel[0];
                    d2s.i[1] = l.kernel[1];
                    pt_of[l.outputs[0]] = out;
                    return true;
                }
                // A depthwise transposed convolution with kernel == stride, every weight 1 and no bias copies each input pixel into its
                // k x k block: a nearest-neighbour upsample (RetinaFace's FPN spells its 2x upsample that way, retina_r50.cpp:156-172:
                // addDeconvolutionNd(256, DimsHW{2, 2}, ones) with setNbGroups(256)).  Same values, exactly; the resize kernel moves
                // 16-byte chunks where the direct transposed convolution walked scalars (253 us per launch on the 1280 x 1280 config).
                {
                    bool ones = l.groups == ti.C && l.nb_out == ti.C && l.kernel[0] == l.stride[0] && l.kernel[1] == l.stride[1] && l.kernel[0] > 1 &&
                                l.padding[0] == 0 && l.padding[1] == 0 && l.dilation[0] == 1 && l.dilation[1] == 1 &&
                                (int64_t)l.w0.size() == (int64_t)ti.C * l.kernel[0] * l.kernel[1];
                    for (size_t i = 0; ones && i < l.w0.size(); ++i) ones = l.w0[i] == 1.0f;
                    for (size_t i = 0; ones && i < l.w1.size(); ++i) ones = l.w1[i] == 0.0f;
                    if (ones) {
                        const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                        add_op(OP_RESIZE, l.name + " [all-ones depthwise deconvolution = nearest upsample]", {in}, {out});
                        pt_of[l.outputs[0]] = out;
                        return true;
                    }
                }
                const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                POp& op = add_op(OP_DECONV, l.name, {in}, {out});
                op.src_layer = li;
                ConvArgs& a = op.conv;
                const PTensor& to = plan.tensors[out];
                a.H = ti.H; a.W = ti.W; a.Cin = ti.C; a.Ho = to.H; a.Wo = to.W; a.Cout = to.C;
                a.kh = l.kernel[0]; a.kw = l.kernel[1]; a.stride_h = l.stride[0]; a.stride_w = l.stride[1];
                a.pad_h = l.padding[0]; a.pad_w = l.padding[1]; a.dil_h = l.dilation[0]; a.dil_w = l.dilation[1];
                a.groups = l.groups;
                op.flops = 2.0 * ti.H * ti.W * a.Cin * (double)a.kh * a.kw * (a.Cout / a.groups);
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_POOLING: {
                const int in = need_nhwc(l.inputs[0]);
                const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                POp& op = add_op(OP_POOL, l.name, {in}, {out});
                op.i[0] = l.op == TRTX_POOLING_MAX ? POOL_MAX : POOL_AVG;
                op.i[1] = l.kernel[0]; op.i[2] = l.kernel[1]; op.i[3] = l.stride[0]; op.i[4] = l.stride[1];
                op.i[5] = l.padding[0]; op.i[6] = l.padding[1]; op.i[7] = l.avg_exclusive;
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_PADDING: {
                // one zero-pad op, no fold into the reader: a max-pool here starts from -inf and skips its border, and yolov3-tiny's 2x2 stride-1 pool
                // behind Pad(0,0;1,1) must see the zeros (its LeakyReLU inputs are negative in places)
                if (net.int8) return fail(l.name + ": IPaddingLayer is not implemented in kINT8 networks");
                if (!g.spatial(net.tensors[l.inputs[0]].dims)) return fail(l.name + ": IPaddingLayer needs an image tensor");
                const int in = need_nhwc(l.inputs[0]);
                const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                POp& op = add_op(OP_PAD_NHWC, l.name, {in}, {out});
                op.i[0] = (int)l.start.d[0];
                op.i[1] = (int)l.start.d[1];
                op.bytes = (double)dtype_size(dt) * (net.tensors[l.inputs[0]].dims.volume() + out_dims().volume());
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_RESIZE: {
                if (l.op != TRTX_RESIZE_NEAREST) return fail(l.name + ": only nearest resize is implemented");
                const Dims& di = net.tensors[l.inputs[0]].dims;
                const Dims& dout = out_dims();
                if (!g.spatial(di) || dout.d[di.nb - 3] != di.d[di.nb - 3]) return fail(l.name + ": resize must keep channels");
                const int in = need_nhwc(l.inputs[0]);
                const int out = new_tensor(l.outputs[0], dout, LAY_NHWC, true);
                add_op(OP_RESIZE, l.name, {in}, {out});
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_ACTIVATION: {
                const int code = act_code(l.op);
                if (code < 0) return fail(l.name + ": unsupported activation type");
                return emit_activation(l, code, l.alpha);
            }
            case L_UNARY: {
                static const char* const names[] = {"kEXP", "kLOG", "kSQRT", "kRECIP", "kABS", "kNEG", "kSIN", "kCOS", "kTAN", "kSINH", "kCOSH", "kASIN",
                                                    "kACOS", "kATAN", "kASINH", "kACOSH", "kATANH", "kCEIL", "kFLOOR", "kERF", "kNOT", "kSIGN", "kROUND", "kISINF"};
                if (l.op != TRTX_UNARY_EXP)
                    return fail(l.name + ": unary operation " + (l.op > 0 && l.op <= TRTX_UNARY_LAST ? std::string(names[l.op]) : std::to_string(l.op)) +
                                " is not implemented (only kEXP is)");
                return emit_activation(l, ACT_EXP, 0.f);
            }
            case L_SCALE: {
                bool pow1 = true;
                for (float p : l.w2) pow1 = pow1 && p == 1.0f;
                const Dims& di = net.tensors[l.inputs[0]].dims;
                if (g.spatial(di) && pow1 && l.op != TRTX_SCALE_ELEMENTWISE) {
                    const int in = need_nhwc(l.inputs[0]);
                    const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                    POp& op = add_op(OP_SCALE_NHWC, l.name, {in}, {out});
                    op.src_layer = li;
                    pt_of[l.outputs[0]] = out;
                    return true;
                }
                if (l.op == TRTX_SCALE_ELEMENTWISE) return fail(l.name + ": elementwise scale is not implemented");
                const int in = need_lin(l.inputs[0]);
                const int out = new_tensor(l.outputs[0], out_dims(), LAY_LINEAR, plan.tensors[in].batched);
                POp& op = add_op(OP_SCALE_LIN, l.name, {in}, {out});
                op.src_layer = li;
                op.i[0] = l.op == TRTX_SCALE_CHANNEL ? 1 : 0;
                const int ca = (net.explicit_batch && di.nb >= 4) ? 1 : (di.nb >= 3 ? di.nb - 3 : 0);
                op.i[1] = (int)extent(di, 0, ca); op.i[2] = (int)di.d[ca]; op.i[3] = (int)extent(di, ca + 1, di.nb);
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_ELEMENTWISE: {
                const int code = ew_code(l.op);
                if (code < 0) return fail(l.name + ": unsupported elementwise op");
                const Dims &da = net.tensors[l.inputs[0]].dims, &db = net.tensors[l.inputs[1]].dims;
                const int pa = pt_of[l.inputs[0]], pb = pt_of[l.inputs[1]];
                const bool any_nhwc = plan.tensors[pa].layout == LAY_NHWC || plan.tensors[pb].layout == LAY_NHWC;
                if (g.spatial(da) && da == db && any_nhwc) {
                    const int a = need_nhwc(l.inputs[0]), b = need_nhwc(l.inputs[1]);
                    const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                    POp& op = add_op(OP_EW_NHWC, l.name, {a, b}, {out});
                    op.i[0] = code;
                    pt_of[l.outputs[0]] = out;
                    return true;
                }
                const int a = need_lin(l.inputs[0]), b = need_lin(l.inputs[1]);
                const Dims& dout = out_dims();
                const bool batched = plan.tensors[a].batched || plan.tensors[b].batched;
                const int out = new_tensor(l.outputs[0], dout, LAY_LINEAR, batched);
                POp& op = add_op(OP_EW_LIN, l.name, {a, b}, {out});
                op.i[0] = code;
                op.view.rank = dout.nb;
                long sa = 1, sb = 1;
                for (int k = dout.nb - 1; k >= 0; --k) {
                    op.view.shape[k] = dout.d[k];
                    op.view.stride_in[k] = (da.d[k] == 1 && dout.d[k] > 1) ? 0 : sa;
                    op.view.stride_in2[k] = (db.d[k] == 1 && dout.d[k] > 1) ? 0 : sb;
                    sa *= da.d[k];
                    sb *= db.d[k];
                }
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_CONCAT: return emit_concat(li);
            case L_SLICE: return emit_slice(li);
            case L_SHUFFLE: return emit_shuffle(li);
            case L_SOFTMAX: {
                const Dims& di = net.tensors[l.inputs[0]].dims;
                int ax;
                if (l.axis < 0) {
                    ax = std::max(0, di.nb - 3);
                } else {
                    ax = -1;
                    for (int k = 0; k < di.nb; ++k)
                        if ((l.axis >> k) & 1) {
                            if (ax >= 0) return fail(l.name + ": softmax over several axes");
                            ax = k;
                        }
                    if (ax < 0) return fail(l.name + ": softmax without axis");
                }
                return emit_softmax(l.name, l.inputs[0], l.outputs[0], ax);
            }
            case L_MATMUL: {
                const Dims &da = net.tensors[l.inputs[0]].dims, &db = net.tensors[l.inputs[1]].dims;
                bool lead = false;
                for (int k = 0; k < da.nb - 2; ++k) lead = lead || da.d[k] != 1 || db.d[k] != 1;
                if (l.mm_op[0] == TRTX_MATMUL_VECTOR || l.mm_op[1] == TRTX_MATMUL_VECTOR) return fail(l.name + ": kVECTOR matmul");
                const int a = need_lin(l.inputs[0]), b = need_lin(l.inputs[1]);
                if (lead && (plan.tensors[a].batched || plan.tensors[b].batched))
                    return fail(l.name + ": matmul with leading dims > 1 on a tensor that also carries the implicit batch is not implemented");
                const Dims& dout = out_dims();
                const int out = new_tensor(l.outputs[0], dout, LAY_LINEAR, plan.tensors[a].batched || plan.tensors[b].batched);
                POp& op = add_op(OP_MATMUL, l.name, {a, b}, {out});
                const int n = da.nb;
                const bool ta = l.mm_op[0] == TRTX_MATMUL_TRANSPOSE, tb = l.mm_op[1] == TRTX_MATMUL_TRANSPOSE;
                op.i[0] = (int)dout.d[n - 2]; op.i[1] = (int)dout.d[n - 1];
                op.i[2] = (int)(ta ? da.d[n - 2] : da.d[n - 1]); op.i[3] = ta; op.i[4] = tb;
                op.flops = 2.0 * op.i[0] * op.i[1] * op.i[2];
                if (lead) {
                    // batched matmul over the leading dims, a dim of 1 broadcasting against a larger one: per leading dim the element
                    // stride of A and B (0 where broadcast); adjacent dims that walk both operands contiguously merge, and the
                    // kernel takes at most two (outer, inner) - op.view holds them (rank, shape, stride_in = A, stride_in2 = B)
                    long sa = (long)da.d[n - 2] * da.d[n - 1], sb = (long)db.d[n - 2] * db.d[n - 1];
                    std::vector<long> shp, ssa, ssb;
                    for (int k = n - 3; k >= 0; --k) {
                        const long ea = da.d[k] == 1 ? 0 : sa, eb = db.d[k] == 1 ? 0 : sb;
                        sa *= da.d[k];
                        sb *= db.d[k];
                        if (dout.d[k] == 1) continue;
                        if (!shp.empty() && ssa.back() * shp.back() == ea && ssb.back() * shp.back() == eb) {
                            shp.back() *= dout.d[k];   // (merge: ea / eb continue the inner dim's walk; broadcast dims stay 0 * x == 0)
                            continue;
                        }
                        shp.push_back(dout.d[k]);
                        ssa.push_back(ea);
                        ssb.push_back(eb);
                    }
                    if (shp.size() > 2) return fail(l.name + ": matmul with more than two independent broadcast patterns in its leading dims");
                    op.view.rank = (int)shp.size();
                    for (size_t k = 0; k < shp.size(); ++k) {   // view dim 0 = outer
                        const size_t j = shp.size() - 1 - k;
                        op.view.shape[k] = shp[j];
                        op.view.stride_in[k] = ssa[j];
                        op.view.stride_in2[k] = ssb[j];
                    }
                    op.flops *= (double)dout.volume() / ((double)op.i[0] * op.i[1]);
                }
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_CONSTANT: {
                const int out = new_tensor(l.outputs[0], out_dims(), LAY_LINEAR, false);
                plan.tensors[out].batched = false;
                Storage s;
                s.kind = ST_WEIGHTS;
                s.bytes = (size_t)out_dims().volume() * 4;
                plan.tensors[out].storage = (int)plan.storages.size();
                plan.storages.push_back(s);
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_REDUCE: {
                const Dims& di = net.tensors[l.inputs[0]].dims;
                const int p = pt_of[l.inputs[0]];
                const int hw_mask = 0b110 << (di.nb - 3);
                if (g.spatial(di) && plan.tensors[p].layout == LAY_NHWC && l.op == TRTX_REDUCE_AVG && l.axis == hw_mask && l.keep_dims) {
                    const int out = new_tensor(l.outputs[0], out_dims(), LAY_NHWC, true);
                    add_op(OP_REDUCE_HW, l.name, {p}, {out});
                    pt_of[l.outputs[0]] = out;
                    return true;
                }
                // contiguous run of reduced axes in LINEAR layout
                int first = -1, last = -1;
                for (int k = 0; k < di.nb; ++k)
                    if ((l.axis >> k) & 1) {
                        if (first < 0) first = k;
                        if (last >= 0 && k != last + 1) return fail(l.name + ": non-contiguous reduce axes");
                        last = k;
                    }
                if (first < 0) return fail(l.name + ": reduce without axes");
                int rop;
                switch (l.op) {
                    case TRTX_REDUCE_SUM: rop = 0; break;
                    case TRTX_REDUCE_AVG: rop = 1; break;
                    case TRTX_REDUCE_MAX: rop = 2; break;
                    default: return fail(l.name + ": unsupported reduce op");
                }
                const int in = need_lin(l.inputs[0]);
                const int out = new_tensor(l.outputs[0], out_dims(), LAY_LINEAR, plan.tensors[in].batched);
                POp& op = add_op(OP_REDUCE_LIN, l.name, {in}, {out});
                op.i[0] = rop; op.i[1] = (int)extent(di, 0, first); op.i[2] = (int)extent(di, first, last + 1); op.i[3] = (int)extent(di, last + 1, di.nb);
                pt_of[l.outputs[0]] = out;
                return true;
            }
            case L_PLUGIN: {
                if (emit_roi_align(li)) return true;
                if (g.is_builtin_mish(li)) return emit_activation(l, ACT_MISH, 0.f);   // a Mish_TRT no convolution absorbed
                std::vector<int> ins, outs;
                for (int t : l.inputs) ins.push_back(need_lin(t));
                for (size_t s = 0; s < l.outputs.size(); ++s) {
                    const int o = new_tensor(l.outputs[s], net.tensors[l.outputs[s]].dims, LAY_LINEAR, true);
                    outs.push_back(o);
                    pt_of[l.outputs[s]] = o;
                }
                POp& op = add_op(OP_PLUGIN, l.name, ins, outs);
                op.plugin = l.plugin;
                if (net.explicit_batch && !l.inputs.empty()) op.i[0] = (int)net.tensors[l.inputs[0]].dims.d[0];   // the plugin's batchSize
                return true;
            }
            case L_IDENTITY: {
                const int p = pt_of[l.inputs[0]];
                pt_of[l.outputs[0]] = plan.tensors[p].layout == LAY_NHWC
                                              ? new_view_nhwc(p, 0, plan.tensors[p].C, l.outputs[0])
                                              : new_view_lin(p, out_dims(), l.outputs[0]);
                return true;
            }
            default: return fail(l.name + ": unknown layer kind");
        }
    }

    // "RoiAlign" (rcnn/RoiAlignPlugin.h; blob int res, float scale, int ratio, int nProp, int C, int fh, int fw) in an fp16
    // engine whose feature map already lives in NHWC fp16: run the engine-native kernel on it and emit the NHWC
    // [P][res][res][C] tensor the res5 convolutions read, instead of fp32 LINEAR in / out plus two layout passes
    // (803 MB fp32 written, re-read and re-written as fp16 per image at C5).  Same detectron2 ROIAlign(aligned=True)
    // arithmetic as the plugin (pinned on the reference's kernel in tests/test_ref_pinning.py); fp32 engines and
    // TRTX_ROIALIGN_PLUGIN=1 keep the plugin route.  Returns false (nothing emitted) where the plugin route applies.
    bool emit_roi_align(int li) {
        const LayerDef& l = net.layers[li];
        if (!opt.roialign_fused || dt != DT_F16 || net.explicit_batch || !l.plugin || l.plugin->type() != "RoiAlign" || l.plugin->version() != "1" ||
            l.inputs.size() != 2 || l.outputs.size() != 1 || plan.tensors[pt_of[l.inputs[1]]].layout != LAY_NHWC)
            return false;
        const std::vector<uint8_t> blob = l.plugin->serialize();
        const PTensor& feat = plan.tensors[pt_of[l.inputs[1]]];
        if (blob.size() != 28) return false;
        int32_t iv[7];
        memcpy(iv, blob.data(), 28);
        float scale;
        memcpy(&scale, blob.data() + 4, 4);
        const Dims& od = net.tensors[l.outputs[0]].dims;
        if (!(iv[0] > 0 && iv[3] > 0 && iv[4] == feat.C && iv[5] == feat.H && iv[6] == feat.W && feat.nmul == 1 && feat.C % 8 == 0 &&
              od.nb == 4 && od.d[0] == iv[3] && od.d[1] == iv[4] && od.d[2] == iv[0] && od.d[3] == iv[0]))
            return false;
        const int boxes = need_lin(l.inputs[0]);
        // Every reader a 1x1 stride-2 unpadded convolution (res5.0's conv1 and its shortcut, rcnn/backbone.hpp:9,110-117
        // STRIDE_IN_1X1; Faster R-CNN R50-C4): only the even bins are ever read.  Emit exactly those - [P][7][7][C]
        // instead of [P][14][14][C] - and run the readers at stride 1 over it: the same samples in the same order
        // (bit-identical), a quarter of the RoIAlign work and writes (C5 b4: 1.6 GB -> 0.4 GB per step), and the
        // convolutions read contiguous pixels.  Mask R-CNN's mask-head RoIAlign feeds a stride-1 reader and keeps
        // the full grid (rcnn/rcnn.cpp:204-233).  TRTX_ROIALIGN_FOLD_STRIDE=0 keeps the full grid (A/B, tests).
        int step = 0;
        if (opt.roialign_fold_stride && !net.tensors[l.outputs[0]].is_output && !g.consumers[l.outputs[0]].empty()) {
            step = -1;
            for (int c : g.consumers[l.outputs[0]]) {
                const LayerDef& cl = net.layers[c];
                const bool ok = cl.kind == L_CONV && cl.inputs[0] == l.outputs[0] && cl.kernel[0] == 1 && cl.kernel[1] == 1 &&
                                cl.stride[0] == cl.stride[1] && cl.stride[0] > 1 && cl.padding[0] == 0 && cl.padding[1] == 0 &&
                                cl.groups == 1 && (step < 0 || step == cl.stride[0]);
                if (!ok) { step = 0; break; }
                step = cl.stride[0];
            }
        }
        Dims od_emit = od;
        if (step > 1) {
            od_emit.d[2] = od_emit.d[3] = (iv[0] - 1) / step + 1;
            for (int c : g.consumers[l.outputs[0]]) stride_folded[c] = 1;
        } else {
            step = 1;
        }
        const int out = new_tensor(l.outputs[0], od_emit, LAY_NHWC, true);
        POp& op = add_op(OP_ROI_ALIGN, l.name + (step > 1 ? " [native NHWC, every 2nd bin]" : " [native NHWC]"), {boxes, pt_of[l.inputs[1]]}, {out});
        op.i[0] = iv[0]; op.i[1] = iv[2]; op.i[2] = iv[3]; op.i[3] = step;
        op.f[0] = scale;
        op.bytes = 2.0 * (double)od_emit.volume() + 2.0 * (double)feat.C * feat.H * feat.W;
        pt_of[l.outputs[0]] = out;
        return true;
    }

    bool emit_concat(int li) {
        const LayerDef& l = net.layers[li];
        const Dims& dout = net.tensors[l.outputs[0]].dims;
        const int cax = dout.nb - 3;
        bool all_nhwc = g.spatial(dout) && l.axis == cax;
        for (int t : l.inputs) all_nhwc = all_nhwc && plan.tensors[pt_of[t]].layout == LAY_NHWC;
        if (all_nhwc) {
            std::vector<int> ins;
            for (int t : l.inputs) ins.push_back(pt_of[t]);
            // concat of consecutive channel views of one tensor == a view of that tensor (C2F, block.cpp:134-141)
            bool consecutive = plan.tensors[ins[0]].parent >= 0;
            for (size_t k = 1; consecutive && k < ins.size(); ++k) {
                const PTensor &a = plan.tensors[ins[k - 1]], &b = plan.tensors[ins[k]];
                consecutive = b.parent == a.parent && b.coff == a.coff + a.C;
            }
            if (consecutive) {
                pt_of[l.outputs[0]] = new_view_nhwc(plan.tensors[ins[0]].parent, plan.tensors[ins[0]].coff,
                                                    (int)dout.d[cax], l.outputs[0]);
                return true;
            }
            const int out = new_tensor(l.outputs[0], dout, LAY_NHWC, true);
            int off = 0;
            for (size_t k = 0; k < ins.size(); ++k) {
                const int c = plan.tensors[ins[k]].C;
                if (!try_place(ins[k], out, off)) {
                    const int v = new_view_nhwc(out, off, c, -1);
                    add_op(OP_COPY_NHWC, l.name + ":copy" + std::to_string(k), {ins[k]}, {v});
                }
                off += c;
            }
            pt_of[l.outputs[0]] = out;
            return true;
        }
        // LINEAR: scatter every input into the dense output
        std::vector<int> ins;
        bool batched = false;
        for (int t : l.inputs) {
            ins.push_back(need_lin(t));
            batched = batched || plan.tensors[ins.back()].batched;
        }
        const int out = new_tensor(l.outputs[0], dout, LAY_LINEAR, batched);
        long ostride[8];
        dense_strides(dout, ostride);
        long pos = 0;
        for (size_t k = 0; k < ins.size(); ++k) {
            const Dims& di = net.tensors[l.inputs[k]].dims;
            POp& op = add_op(OP_SCATTER, l.name + ":in" + std::to_string(k), {ins[k]}, {out});
            op.view.rank = di.nb;
            for (int d = 0; d < di.nb; ++d) {
                op.view.shape[d] = di.d[d];
                op.view.stride_in[d] = ostride[d];
            }
            op.off0 = pos * ostride[l.axis];
            pos += di.d[l.axis];
        }
        pt_of[l.outputs[0]] = out;
        return true;
    }

    bool emit_slice(int li) {
        const LayerDef& l = net.layers[li];
        const Dims& di = net.tensors[l.inputs[0]].dims;
        const int p = pt_of[l.inputs[0]];
        const int cax = di.nb - 3;
        if (g.spatial(di) && plan.tensors[p].layout == LAY_NHWC) {
            bool chan_only = l.step.d[cax] == 1;
            for (int k = 0; k < di.nb; ++k)
                if (k != cax) chan_only = chan_only && l.start.d[k] == 0 && l.size.d[k] == di.d[k] && l.step.d[k] == 1;
            if (chan_only) {
                pt_of[l.outputs[0]] = new_view_nhwc(p, (int)l.start.d[cax], (int)l.size.d[cax], l.outputs[0]);
                return true;
            }
        }
        const int in = need_lin(l.inputs[0]);
        const int out = new_tensor(l.outputs[0], l.size, LAY_LINEAR, plan.tensors[in].batched);
        POp& op = add_op(OP_GATHER, l.name, {in}, {out});
        op.view.rank = di.nb;
        long s = 1, off = 0;
        for (int k = di.nb - 1; k >= 0; --k) {
            op.view.shape[k] = l.size.d[k];
            op.view.stride_in[k] = s * l.step.d[k];
            off += l.start.d[k] * s;
            s *= di.d[k];
        }
        op.off0 = off;
        pt_of[l.outputs[0]] = out;
        return true;
    }

    bool emit_shuffle(int li) {
        const LayerDef& l = net.layers[li];
        const Dims& di = net.tensors[l.inputs[0]].dims;
        const Dims& dout = net.tensors[l.outputs[0]].dims;
        int cur = need_lin(l.inputs[0]);
        Dims dcur = di;
        if (!ident(l.perm1, di.nb)) {
            Dims t = di;
            for (int k = 0; k < di.nb; ++k) t.d[k] = di.d[l.perm1[k]];
            const int q = new_tensor(-1, t, LAY_LINEAR, plan.tensors[cur].batched);
            POp& op = add_op(OP_GATHER, l.name + ":t1", {cur}, {q});
            long st[8];
            dense_strides(di, st);
            op.view.rank = di.nb;
            for (int k = 0; k < di.nb; ++k) {
                op.view.shape[k] = t.d[k];
                op.view.stride_in[k] = st[l.perm1[k]];
            }
            cur = q;
            dcur = t;
        }
        // reshape: a view
        Dims r = dcur;
        if (l.reshape.nb > 0) {
            // the network already validated/inferred the reshape; recover it from the output dims
            r.nb = dout.nb;
            for (int k = 0; k < dout.nb; ++k) r.d[k] = 0;
            // invert perm2: out[k] = r[perm2[k]]
            for (int k = 0; k < dout.nb; ++k) r.d[l.perm2[k]] = dout.d[k];
        }
        if (ident(l.perm2, r.nb)) {
            pt_of[l.outputs[0]] = new_view_lin(cur, dout, l.outputs[0]);
            return true;
        }
        const int rv = new_view_lin(cur, r, -1);
        const int out = new_tensor(l.outputs[0], dout, LAY_LINEAR, plan.tensors[cur].batched);
        POp& op = add_op(OP_GATHER, l.name + ":t2", {rv}, {out});
        long st[8];
        dense_strides(r, st);
        op.view.rank = r.nb;
        for (int k = 0; k < r.nb; ++k) {
            op.view.shape[k] = dout.d[k];
            op.view.stride_in[k] = st[l.perm2[k]];
        }
        pt_of[l.outputs[0]] = out;
        return true;
    }

    void apply_aliases() {
        for (auto& a : fu.aliases)
            if (pt_of[a.first] < 0 && pt_of[a.second] >= 0) pt_of[a.first] = pt_of[a.second];
    }

    // ---- driver ----------------------------------------------------------------------------------------
    void bind(int net_t, int p, bool is_input) {   // plan tensor p is the next binding: network tensor net_t
        Storage s;
        s.kind = ST_BINDING;
        s.binding = (int)plan.binding_tensor.size();
        plan.tensors[p].storage = (int)plan.storages.size();
        plan.storages.push_back(s);
        plan.binding_tensor.push_back(net_t);
        plan.binding_ptensor.push_back(p);
        plan.binding_is_input.push_back(is_input);
    }
    bool run() {
        plan.explicit_batch = net.explicit_batch;
        plan.fp16 = net.fp16;
        plan.max_batch = net.explicit_batch ? 1 : net.max_batch;
        for (int t : net.input_ids()) bind(t, pt_of[t] = new_tensor(t, net.tensors[t].dims, LAY_LINEAR, true), true);
        fu = match_fusions(g);
        for (size_t li = 0; li < net.layers.size(); ++li) {
            if (fu.yolo_at[li] >= 0) {
                if (!emit_yolo_head(fu.yolo_heads[fu.yolo_at[li]])) return false;
                continue;
            }
            if (fu.yolo5_at[li] >= 0) {
                if (!emit_yolo5_head(fu.yolo5_heads[fu.yolo5_at[li]])) return false;
                continue;
            }
            if (fu.yolo9_at[li] >= 0) {
                if (!emit_yolo9_head(fu.yolo9_heads[fu.yolo9_at[li]])) return false;
                continue;
            }
            if (fu.attn_at[li] >= 0) {
                if (!emit_attention(fu.attns[fu.attn_at[li]])) return false;
                continue;
            }
            if (fu.attn_split_at[li] >= 0) {
                if (!emit_attention_split(fu.attn_splits[fu.attn_split_at[li]])) return false;
                continue;
            }
            if (fu.hgconv_at[li] >= 0) {
                if (!emit_hgconv(fu.hgconvs[fu.hgconv_at[li]])) return false;
                continue;
            }
            if (fu.gelu_at[li] >= 0) {
                if (!emit_gelu(fu.gelus[fu.gelu_at[li]])) return false;
                apply_aliases();
                continue;
            }
            if (fu.softmax_at[li] >= 0) {   // a spelled-out softmax standing alone: the softmax op at its division
                const SoftmaxChainFuse& c = fu.softmax_chains[fu.softmax_at[li]];
                if (!emit_softmax(net.layers[li].name + " [max / sub / exp / sum / div chain]", c.in, c.out, c.axis)) return false;
                apply_aliases();
                continue;
            }
            if (fu.gated_at[li] >= 0) {
                if (!emit_gated_add((int)li, fu.gated_adds[fu.gated_at[li]])) return false;
                apply_aliases();
                continue;
            }
            if (fu.group_at[li] >= 0) {
                if (!emit_conv(fu.groups[fu.group_at[li]])) return false;
                continue;
            }
            if (fu.absorbed[li]) {
                apply_aliases();
                continue;
            }
            if (!emit_layer((int)li)) return false;
            apply_aliases();
        }
        // output bindings: LINEAR fp32
        for (int t : net.output_ids()) {
            if (pt_of[t] < 0) return fail("output tensor " + net.tensors[t].name + " is never produced");
            int p = need_lin(t);
            PTensor& pt = plan.tensors[p];
            const bool own = pt.parent < 0 && pt.storage < 0 && !is_binding_tensor(plan, p);
            if (!own) {
                const int q = new_tensor(t, pt.dims, LAY_LINEAR, pt.batched);
                POp& op = add_op(OP_COPY_LIN, "output:" + net.tensors[t].name, {p}, {q});
                op.i[0] = 0;
                p = q;
            }
            bind(t, p, false);
        }
        return finalize_plan(plan, {net.int8, net.tensor_scale, net.max_aux_streams, dt, opt}, &err);
    }
};

}  // namespace

static thread_local int g_calibration_lowering = 0;
CalibrationLowering::CalibrationLowering() { ++g_calibration_lowering; }
CalibrationLowering::~CalibrationLowering() { --g_calibration_lowering; }
bool CalibrationLowering::active() { return g_calibration_lowering > 0; }

bool lower_network(const Network& net, Plan* plan) {
    *plan = Plan();
    Lowerer L(net, *plan);
    const bool ok = L.run();
    if (!ok) plan->error = L.err.empty() ? "lowering failed" : L.err;
    return ok;
}

}  // namespace trtx
