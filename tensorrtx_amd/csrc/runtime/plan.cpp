// What a plan says about itself: op kind names and the JSON description.  See plan.h.
#include "plan.h"

#include <sstream>

namespace trtx {

const char* op_kind_name(int k) {
    static const char* n[] = {"conv",     "deconv",    "pool",      "resize",     "ew_nhwc", "act_nhwc", "scale_nhwc",
                              "copy_nhwc", "reduce_hw", "to_nhwc",   "to_linear",  "gather",  "scatter",  "ew_lin",
                              "act_lin",  "scale_lin", "softmax",   "matmul",     "reduce_lin", "plugin", "copy_lin", "yolo_head",
                              "pool_chain", "depth_to_space", "roi_align", "conv_chain", "conv_group", "attention",
                              "yolo_task_head", "yolo5_head", "yolo9_head", "yolo7_head", "hgconv", "gated_add", "attention_split",
                              "darknet_head", "pad_nhwc", "yolo10_head"};
    return (k >= 0 && k <= OP_YOLO10_HEAD) ? n[k] : "?";
}

// In YoloForm's order, the task head behind them
static const HeadOp kHeadOps[YOLO_FORMS + 1] = {
        {OP_YOLO_HEAD, " [fused DFL+decode]", 0, 8, true, {trtx_yolo_head_decode_nhwc, trtx_yolo_head_decode_nhwc_f32}, trtx_yolo_head_decode_workspace, {}, nullptr},
        {OP_YOLO5_HEAD, " [fused anchor decode]", 1, 8, false, {}, nullptr, {trtx_yolov5_head_decode_nhwc, trtx_yolov5_head_decode_nhwc_f32}, trtx_yolov5_head_decode_workspace},
        {OP_YOLO9_HEAD, " [fused DFL+decode, 38-float records]", 3, 3, true, {}, nullptr, {}, nullptr},
        {OP_YOLO7_HEAD, " [fused anchor decode, 6-float records]", 1, 8, false, {}, nullptr, {trtx_yolov7_head_decode_nhwc, trtx_yolov7_head_decode_nhwc_f32}, trtx_yolov7_head_decode_workspace},
        {OP_DARKNET_HEAD, " [fused Darknet anchor decode, 7-float records]", 1, 8, false, {}, nullptr, {trtx_darknet_head_decode_nhwc, trtx_darknet_head_decode_nhwc_f32}, trtx_darknet_head_decode_workspace},
        // the workspace is OP_YOLO_HEAD's: the same candidate lists
        {OP_YOLO10_HEAD, " [fused DFL+decode, 6-float records]", 1, 5, true, {trtx_yolov10_head_decode_nhwc, trtx_yolov10_head_decode_nhwc_f32}, trtx_yolo_head_decode_workspace, {}, nullptr},
        {OP_YOLO_TASK_HEAD, " [fused DFL+task decode]", 0, 4, true, {}, trtx_yolo_head_decode_workspace, {}, nullptr},
};
const HeadOp& head_op_of(YoloForm form) { return kHeadOps[form]; }
const HeadOp* head_op(int kind) {
    for (const HeadOp& h : kHeadOps)
        if (h.kind == kind) return &h;
    return nullptr;
}

std::string Plan::describe_json() const {
    std::ostringstream o;
    double flops = 0, bytes = 0;
    int n_conv = 0, n_igemm = 0;
    for (const auto& op : ops) {
        flops += op.flops;
        bytes += op.bytes;
        if (op.kind == OP_CONV) {
            ++n_conv;
            n_igemm += op.igemm ? 1 : 0;
        }
        n_conv += (int)op.group.size();
        n_igemm += (int)op.group.size();
    }
    o << "{\"fp16\":" << (fp16 ? "true" : "false") << ",\"max_batch\":" << max_batch << ",\"arena_bytes\":" << arena_bytes
      << ",\"weight_bytes\":" << weight_bytes << ",\"n_lanes\":" << num_lanes << ",\"n_ops\":" << ops.size() << ",\"n_conv\":" << n_conv
      << ",\"n_igemm\":" << n_igemm << ",\"flops_per_sample\":" << flops << ",\"bytes_per_sample\":" << bytes
      << ",\"ops\":[";
    for (size_t k = 0; k < ops.size(); ++k) {
        const POp& op = ops[k];
        o << (k ? "," : "") << "{\"kind\":\"" << op_kind_name(op.kind) << "\",\"name\":\"";
        for (char c : op.name) o << ((c == '"' || c == '\\' || (unsigned char)c < 0x20) ? ' ' : c);
        o << "\",\"flops\":" << op.flops << ",\"bytes\":" << op.bytes;
        auto conv_fields = [&](const POp& op) {
            const ConvArgs& a = op.conv;
            o << ",\"igemm\":" << (op.igemm ? "true" : "false") << ",\"stem\":" << (op.stem ? "true" : "false") << (op.stem_pair ? ",\"stem_pair\":true" : "")
              << (op.bneck_pair ? ",\"bneck_pair\":true" : "") << ",\"cin\":" << (a.in_i8 ? 2 * a.Cin : a.Cin) << ",\"cout\":" << a.Cout
              << ",\"k\":[" << a.kh << "," << a.kw << "],\"stride\":[" << a.stride_h << "," << a.stride_w << "],\"hw_in\":["
              << a.H << "," << a.W << "],\"hw_out\":[" << a.Ho << "," << a.Wo << "],\"act1\":" << a.act1
              << ",\"act2\":" << a.act2 << ",\"alpha1\":" << a.alpha1 << ",\"alpha2\":" << a.alpha2 << ",\"up_c\":" << a.up_C << ",\"residual\":" << (op.in.size() > 1 ? "true" : "false")
              << ",\"bn_folded\":" << (op.scale_layer >= 0 ? "true" : "false") << ",\"ld_in\":" << a.ld_in
              << ",\"ld_out\":" << a.ld_out << ",\"i8\":[" << a.in_i8 << "," << a.out_i8 << "," << a.res_i8 << "],\"nmul\":" << (op.stem ? 1 : tensors[op.in[0]].nmul) << ",\"nfix\":"
              << (op.stem ? 0 : tensors[op.in[0]].nfix);
            if (op.dw) o << ",\"dw\":true";
            if (op.grouped) o << ",\"grouped\":true";
            if (op.cout_real) o << ",\"cout_real\":" << op.cout_real;
            if (op.reorg_cin) o << ",\"reorg_cin\":" << op.reorg_cin;
            if (op.fold_layer >= 0) o << ",\"repvggdw_fold\":true";
        };
        if (op.kind == OP_CONV || op.kind == OP_DECONV) conv_fields(op);
        if (op.kind == OP_ACT_NHWC || op.kind == OP_ACT_LIN) o << ",\"act\":" << op.i[0];
        if (op.kind == OP_ATTENTION) o << ",\"heads\":" << op.i[0] << ",\"n\":" << op.i[1] << ",\"kd\":" << op.i[2] << ",\"hd\":" << op.i[3];
        if (op.kind == OP_ATTENTION && op.i[4] > 0) o << ",\"area\":" << op.i[4] << ",\"kernel\":\"mfma\"";
        if (op.kind == OP_ATTENTION_SPLIT)
            o << ",\"heads\":" << op.i[0] << ",\"n\":" << op.i[1] << ",\"kd\":" << op.i[2] << ",\"hd\":" << op.i[3] << ",\"area\":" << op.i[4] << ",\"k_offset\":" << op.i[5];
        if (op.kind == OP_HGCONV)
            o << ",\"n\":" << op.i[0] << ",\"d\":" << op.i[1] << ",\"e\":" << op.i[2] << ",\"logit_scale\":" << op.f[0] << ",\"ld\":[" << tensors[op.in[0]].ld << ","
              << tensors[op.out[0]].ld << "],\"ws_bytes\":" << op.ws_bytes;
        if (op.kind == OP_POOL || op.kind == OP_POOL_CHAIN)
            o << ",\"k\":[" << op.i[1] << "," << op.i[2] << "],\"stride\":[" << op.i[3] << "," << op.i[4] << "],\"outputs\":" << op.out.size();
        if (op.kind == OP_PAD_NHWC) o << ",\"pre\":[" << op.i[0] << "," << op.i[1] << "]";
        // the fused heads, from shared pieces
        auto list = [&](const char* key, int n, auto item) {
            o << ",\"" << key << "\":[";
            for (int j = 0; j < n; ++j) {
                o << (j ? "," : "");
                item(j);
            }
            o << "]";
        };
        auto lds = [&](const char* key, const std::vector<int>& ts) { list(key, (int)ts.size(), [&](int j) { o << tensors[ts[j]].ld; }); };
        const HeadOp* head = head_op(op.kind);
        if (op.kind == OP_YOLO_TASK_HEAD) {
            o << ",\"task\":\"" << (op.i[9] == 1 ? "seg" : (op.i[9] == 2 ? "pose" : "obb")) << "\",\"classes\":" << op.i[0] << ",\"nk\":" << op.i[10];
            lds("branch_ld", op.extra_in);
        } else if (head && op.kind != OP_YOLO_HEAD) {
            o << ",\"classes\":" << op.i[0] << ",\"levels\":" << op.i[4];
            if (head->anchor_ws) {
                o << ",\"anchor_levels\":" << op.fv.size() / 6;
                list("grids", op.i[4], [&](int j) { o << "[" << op.iv[2 * j] << "," << op.iv[2 * j + 1] << "]"; });
            }
            if (op.kind == OP_YOLO9_HEAD) {
                list("grids", op.i[4], [&](int j) { o << "[" << op.i[2] / (8 << j) << "," << op.i[1] / (8 << j) << "]"; });
                list("strides", op.i[4], [&](int j) { o << (8 << j); });
                lds("box_ld", op.in);
                lds("cls_ld", op.extra_in);
            } else {
                if (head->stride_ws) list("strides", op.i[4], [&](int j) { o << op.i[5 + j]; });
                lds("ld", op.in);
            }
        }
        if (op.kind == OP_CONV_GROUP) {
            o << ",\"members\":[";
            for (size_t j = 0; j < op.group.size(); ++j) {
                const POp& m = op.group[j];
                o << (j ? "," : "") << "{\"name\":\"";
                for (char c : m.name) o << ((c == '"' || c == '\\' || (unsigned char)c < 0x20) ? ' ' : c);
                o << "\",\"flops\":" << m.flops << ",\"bytes\":" << m.bytes;
                conv_fields(m);
                o << ",\"in\":[";
                for (size_t q = 0; q < m.in.size(); ++q) o << (q ? "," : "") << m.in[q];
                o << "],\"out\":[" << m.out[0] << "]}";
            }
            o << "]" << (op.sibling_pair ? ",\"sibling_pair\":true" : "");
        }
        o << ",\"lane\":" << op.lane << ",\"waits\":[";
        for (size_t j = 0; j < op.wait_ops.size(); ++j) o << (j ? "," : "") << op.wait_ops[j];
        o << "],\"in\":[";
        for (size_t j = 0; j < op.in.size(); ++j) o << (j ? "," : "") << op.in[j];
        o << "],\"out\":[";
        for (size_t j = 0; j < op.out.size(); ++j) o << (j ? "," : "") << op.out[j];
        o << "]}";
    }
    o << "],\"tensors\":[";
    for (size_t k = 0; k < tensors.size(); ++k) {
        const PTensor& t = tensors[k];
        o << (k ? "," : "") << "{\"id\":" << t.id << ",\"net\":" << t.net_tensor << ",\"layout\":\""
          << (t.layout == LAY_NHWC ? "nhwc" : "linear") << "\",\"dims\":[";
        for (int d = 0; d < t.dims.nb; ++d) o << (d ? "," : "") << t.dims.d[d];
        o << "],\"storage\":" << t.storage << ",\"coff\":" << t.rcoff << ",\"ld\":" << t.ld << ",\"dtype\":" << t.dtype << ",\"scale\":" << t.scale
          << ",\"view\":"
          << (t.parent >= 0 ? "true" : "false") << "}";
    }
    o << "],\"storages\":[";
    for (size_t k = 0; k < storages.size(); ++k) {
        const Storage& s = storages[k];
        o << (k ? "," : "") << "{\"kind\":" << s.kind << ",\"bytes\":" << s.bytes << ",\"offset\":" << s.offset
          << ",\"first\":" << s.first_use << ",\"last\":" << s.last_use << "}";
    }
    o << "]}";
    return o.str();
}

}  // namespace trtx
