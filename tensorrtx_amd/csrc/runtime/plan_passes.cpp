// The passes over the emitted op list, in the order finalize_plan() at the bottom runs them.  See plan_passes.h.
#include "plan_passes.h"

#include <algorithm>

namespace trtx {
namespace {

bool fail(std::string* err, const std::string& m) {
    *err = m;
    return false;
}

size_t tensor_bytes(const Plan& plan, const PTensor& t) {
    const size_t es = dtype_size(t.dtype);
    if (t.layout == LAY_NHWC) {
        const size_t n = (t.nfix ? (size_t)t.nfix : (size_t)plan.max_batch) * (size_t)t.nmul;
        return n * t.H * t.W * (size_t)t.Calloc * es;
    }
    return (t.batched ? (size_t)plan.max_batch : 1) * (size_t)t.dims.volume() * es;
}

// Which kernel runs a convolution, given the (resolved) strides / offsets and the dtypes of the tensors it touches: fills op.conv
// and sets op.igemm when the implicit-GEMM MFMA kernel takes it (the direct kernel otherwise).  ONE predicate for select_conv_kernels(),
// fold_upsample's probe and the int8 assignment, which may only put a tensor in int8 if every convolution touching it gets the MFMA path.
bool choose_conv_kernel(const Plan& plan, const PassInputs& e, POp& op) {
    ConvArgs& a = op.conv;
    const PTensor& ti = plan.tensors[op.in[0]];
    const PTensor& to = plan.tensors[op.out[0]];
    a.ld_in = ti.ld;
    a.ld_out = to.ld;
    a.ld_res = op.in.size() > 1 ? plan.tensors[op.in[1]].ld : 0;
    a.K = a.kh * a.kw * (a.Cin / a.groups);
    a.Cout_pad = a.Cout;
    a.Kpad = a.K;
    a.up_C = 0;
    if (!op.extra_in.empty()) {   // folded upsample: geometry of the half-resolution source
        const PTensor& tu = plan.tensors[op.extra_in[0]];
        a.up_C = tu.C;
        a.up_ld = tu.ld;
        a.up_H = tu.H;
        a.up_W = tu.W;
    }
    op.igemm = false;
    a.f32 = (op.stem && e.dt == DT_F32) ? 1 : 0;   // (the fp32 stem kernel; the MFMA path sets it below)
    if (op.kind == OP_CONV && !op.stem && e.dt == DT_F16 && a.groups == 1 && a.dil_h == 1 && a.dil_w == 1) {
        int cin_eff = a.Cin;
        bool ok = true;
        if (cin_eff % 8) {
            // padded channels are zero only for a freshly converted, un-aliased tensor
            const PTensor& own = plan.tensors[ti.parent >= 0 ? ti.parent : ti.id];
            ok = ti.parent < 0 && own.pad_zeroed;
            cin_eff = (a.Cin + 7) / 8 * 8;
        }
        ok = ok && ti.rcoff % 8 == 0 && ti.ld % 8 == 0;
        const bool in8 = ti.dtype == DT_I8, out8 = to.dtype == DT_I8;
        const bool res8 = op.in.size() > 1 && plan.tensors[op.in[1]].dtype == DT_I8;
        if (in8) ok = ok && a.Cin % 16 == 0 && ti.rcoff % 16 == 0 && ti.ld % 16 == 0;
        // output side: 16-byte stores when everything is a multiple of 8, element-wise stores otherwise
        bool vec_out = a.Cout % 8 == 0 && to.rcoff % 8 == 0 && to.ld % 8 == 0;
        if (op.in.size() > 1) {
            const PTensor& tr = plan.tensors[op.in[1]];
            vec_out = vec_out && tr.rcoff % 8 == 0 && tr.ld % 8 == 0;
        }
        // tiny reductions (K < 32, e.g. the DFL 1x1) stay on the direct kernel - except the square 1x1 over 16 channels (YOLOv5n's first C3
        // bottleneck, 16 -> 16 on the stride-4 map, the one such layer the builders here produce): a memory-bound layer that the
        // two-taps-per-step form (CinK = 16; its second tap lies outside the 1x1 filter and loads zeros) streams with 16-byte accesses.
        // Wider outputs over 16 channels (the qkv convolutions of the attention test graphs) keep the direct kernel: nothing measured
        // says otherwise.  Not in kINT8 engines either, where such a layer stays the fp16 island it has been.
        // The square 1x1 over 24 channels is the same case one k-step wider (CinK = 32, channels 24 .. 31 load zeros like the last channels of
        // any Cin that is no multiple of the step): the 1x1 branch of YOLOv9t's RepConvN on its 24-channel RepNCSP blocks, 18 layers.
        ok = ok && (a.kh * a.kw * cin_eff >= 32 || (!e.int8 && a.kh == 1 && a.kw == 1 && (a.Cin == 16 || a.Cin == 24) && a.Cout == a.Cin));
        if (ok) {
            ConvArgs t = a;
            t.scalar_out = vec_out ? 0 : 1;
            t.Cin = cin_eff;
            t.bn = conv_igemm_pick_bn(t.Cout);
            t.bk = conv_igemm_pick_bk(cin_eff, t.kh * t.kw);
            {   // few tiles + long K at the largest batch: keep 32-wide steps so the wave-split-K variant applies
                const long m_max = (long)(ti.nfix ? ti.nfix : plan.max_batch) * ti.nmul * t.Ho * t.Wo;
                const long tiles128 = (m_max + 127) / 128 * ((t.Cout + t.bn - 1) / t.bn);
                if (tiles128 <= 256 && (t.bn == 64 || t.bn == 80)) t.bk = 32;
            }
            t.CinK = conv_igemm_pick_cink(cin_eff, t.bk);  // a k-step never straddles a filter tap
            t.K = t.kh * t.kw * t.CinK;
            t.Kpad = (t.K + t.bk - 1) / t.bk * t.bk;
            t.bn = conv_igemm_pick_bn(t.Cout);
            t.Cout_pad = (t.Cout + t.bn - 1) / t.bn * t.bn;
            if (in8) {  // int8 operands: 64-channel k-steps; the input-side geometry is handed over in 2-byte units (ConvArgs)
                t.bk = 32;
                t.in_i8 = 1;
                t.Cin = a.Cin / 2;
                t.ld_in = ti.ld / 2;
                t.CinK = (a.Cin + 63) / 64 * 64 / 2;
                t.K = t.kh * t.kw * t.CinK;
                t.Kpad = t.K;
            }
            t.out_i8 = out8 ? 1 : 0;
            t.res_i8 = res8 ? 1 : 0;
            t.out_inv_scale = out8 ? 1.0f / to.scale : 0.f;
            t.res_scale = res8 ? plan.tensors[op.in[1]].scale : 0.f;
            // Engines for several execution contexts in flight (setMaxAuxStreams(0)) take the implicit-GEMM operands through
            // registers instead of LDS-DMA: bit-identical results, and on YOLOv8n b32 with three contexts 34.2-34.5k img/s against
            // 33.3-33.6k (same box, alternating runs) - a DMA piece costs its wave 60-185 cycles of issue, which co-scheduled
            // workgroups of other contexts cannot hide for each other; a lone context is 3 % slower with it and keeps the DMA.
            // ... and only for layers below the MFMA / HBM ridge (312 FLOP per byte): the MFMA-bound GEMMs of res5 lose with it (C5 three
            // contexts 12.1 vs 11.65 ms; tools/gemm_tactics.py: K = 4608 0.39 vs 0.42 of peak), ResNet-50 gains 2.2 %, RetinaFace is
            // indifferent (profiles/r03_rs_ab.txt).
            {
                const double flop_px = 2.0 * a.Cout * (double)a.kh * a.kw * a.Cin;
                const double byte_px = 2.0 * ((double)a.Cin * a.stride_h * a.stride_w + (double)a.Cout * (op.in.size() > 1 ? 2 : 1));
                constexpr double ridge = 312.0;   // the MFMA / HBM ridge, FLOP per byte
                t.t_rs = (e.max_aux_streams == 0 && flop_px / byte_px < ridge) ? 1 : 0;
            }
            if (conv_igemm_supported(t)) {
                a = t;
                op.igemm = true;
            }
        }
    }
    // fp32 engines: the same skeleton on the fp32 MFMA (kernels/conv_igemm_f32.hip), 16-channel k-steps; the tile shape is the launcher's
    if (op.kind == OP_CONV && !op.stem && e.dt == DT_F32 && ti.dtype == DT_F32 && to.dtype == DT_F32 && a.groups == 1 && a.dil_h == 1 && a.dil_w == 1) {
        int cin_eff = a.Cin;
        bool ok = e.opt.f32_mfma;   // (TRTX_F32_DIRECT=1: the scalar direct kernel of rounds 1-4, an A/B switch)
        if (cin_eff % 4) {
            const PTensor& own = plan.tensors[ti.parent >= 0 ? ti.parent : ti.id];
            ok = ok && ti.parent < 0 && own.pad_zeroed;
            cin_eff = (a.Cin + 3) / 4 * 4;
        }
        ok = ok && ti.rcoff % 4 == 0 && ti.ld % 4 == 0;
        bool vec_out = a.Cout % 4 == 0 && to.rcoff % 4 == 0 && to.ld % 4 == 0;
        if (op.in.size() > 1) {
            const PTensor& tr = plan.tensors[op.in[1]];
            vec_out = vec_out && tr.rcoff % 4 == 0 && tr.ld % 4 == 0;
        }
        ok = ok && a.kh * a.kw * cin_eff >= 16 && a.Cout >= 8;   // tiny reductions / single-channel outputs (the DFL 1x1) stay on the direct kernel
        if (ok) {
            ConvArgs t = a;
            t.f32 = 1;
            t.scalar_out = vec_out ? 0 : 1;
            t.Cin = cin_eff;
            t.bk = 16;
            t.bn = 0;
            t.bm = 0;
            t.CinK = conv_igemm_f32_pick_cink(cin_eff);
            t.K = t.kh * t.kw * t.CinK;
            t.Kpad = (t.K + 15) / 16 * 16;
            t.Cout_pad = (t.Cout + 15) / 16 * 16;
            if (conv_igemm_f32_supported(t)) {
                a = t;
                op.igemm = true;
            }
        }
    }
    // depthwise (YOLO11 DWConv and the PSA attention's pe): kernels/conv_dw.hip, fp16 and fp32, any channel stride
    op.dw = op.kind == OP_CONV && !op.igemm && !op.stem && !op.from_deconv && op.extra_in.empty() && ti.dtype == e.dt && to.dtype == e.dt &&
            (op.in.size() < 2 || plan.tensors[op.in[1]].dtype == e.dt) && conv_dw_supported(a);
    // grouped, not depthwise (YOLOv9's DetectBbox_Conv: 64 -> 64 with g = 4): kernels/conv_grouped.hip, fp16 engines only, 16-byte aligned channel
    // views; a.Kpad becomes the packed row length.  TRTX_CONV_GROUPED=0 leaves such layers on the direct kernel (A/B).  Not in kINT8 engines.
    op.grouped = false;
    if (op.kind == OP_CONV && !op.igemm && !op.dw && !op.stem && !op.from_deconv && op.extra_in.empty() && e.opt.conv_grouped && !e.int8 &&
        !CalibrationLowering::active() && e.dt == DT_F16 && ti.dtype == DT_F16 && to.dtype == DT_F16 && ti.rcoff % 8 == 0 && to.rcoff % 8 == 0) {
        bool ok = true;
        if (op.in.size() > 1) {
            const PTensor& tr = plan.tensors[op.in[1]];
            ok = tr.dtype == DT_F16 && tr.rcoff % 8 == 0 && tr.ld % 8 == 0 && tr.ld >= a.Cout;
        }
        if (ok && conv_grouped_supported(a)) {
            op.grouped = true;
            a.Kpad = conv_grouped_kpad(a);
        }
    }
    return op.igemm;
}

// view geometry (element units: independent of the dtypes assigned next)
void resolve_view_geometry(Plan& plan) {
    for (auto& t : plan.tensors) {
        int p = t.id, coff = 0;
        long eoff = 0;
        while (plan.tensors[p].parent >= 0) {
            coff += plan.tensors[p].coff;
            eoff += plan.tensors[p].eoff;
            p = plan.tensors[p].parent;
        }
        t.rcoff = coff;
        t.reoff = eoff;
        t.ld = plan.tensors[p].layout == LAY_NHWC ? plan.tensors[p].Calloc : 0;
    }
}

// Upsample -> Concat -> Conv1x1 without the upsampled tensor (YOLOv8 head: model.cpp:130-160, twice per network).  The nearest 2x
// resize writes the first channel slice of a concat buffer whose only reader is a 1x1 stride-1 convolution: that convolution's
// A-gather can fetch those channels from the half-resolution tensor at (h >> 1, w >> 1) itself (ConvArgs::up_in).  The resize launch,
// its write of the 4x larger tensor and the convolution's read of it disappear (YOLOv8n b32: 2 launches, 78 MB written + 78 MB read
// per step become 19.5 MB read); every product is formed from the same operands in the same order: bit-identical outputs.
// TRTX_FOLD_UPSAMPLE=0 keeps the resize (A/B, tests).  Not with kINT8 (the int8 resize requantises between two scales).
void fold_upsample(Plan& plan, const PassInputs& e) {
    if (e.int8 || CalibrationLowering::active()) return;   // (fp16 and fp32 engines: both MFMA kernels fetch the slice from the half-resolution tensor)
    if (!e.opt.fold_upsample) return;
    for (size_t k = 0; k < plan.ops.size(); ++k) {
        const POp& rz = plan.ops[k];
        if (rz.kind != OP_RESIZE) continue;
        const PTensor& src = plan.tensors[rz.in[0]];
        const PTensor& up = plan.tensors[rz.out[0]];
        if (up.parent < 0 || up.rcoff != 0 || up.layout != LAY_NHWC || src.layout != LAY_NHWC || up.H != 2 * src.H || up.W != 2 * src.W || up.C != src.C ||
            up.C % 64 || src.ld % 8 || src.rcoff % 8 || src.nmul != 1 || up.nmul != 1 || is_binding_tensor(plan, rz.out[0]))
            continue;
        const int owner = owner_of(plan, rz.out[0]);
        // every reader of the buffer: exactly one, a 1x1 stride-1 convolution over the WHOLE buffer; nobody reads the slice itself
        int reader = -1, n_readers = 0;
        for (size_t j = 0; j < plan.ops.size(); ++j)
            for (int t : plan.ops[j].in)
                if (owner_of(plan, t) == owner) {
                    // readers of OTHER channel ranges of the buffer (a skip connection also feeding elsewhere) do not matter
                    const PTensor& rt = plan.tensors[t];
                    if (rt.rcoff < up.C) {
                        reader = (int)j;
                        ++n_readers;
                    }
                }
        if (n_readers != 1 || is_binding_tensor(plan, owner)) continue;
        POp& cv = plan.ops[reader];
        const ConvArgs& a = cv.conv;
        if (cv.kind != OP_CONV || cv.stem || cv.from_deconv || cv.in[0] != owner || !cv.extra_in.empty() || a.kh != 1 || a.kw != 1 || a.stride_h != 1 ||
            a.stride_w != 1 || a.pad_h || a.pad_w || a.groups != 1 || a.Cin != plan.tensors[owner].C || up.C >= a.Cin || reader < (int)k)
            continue;
        POp probe = cv;
        probe.extra_in = {rz.in[0]};
        if (!choose_conv_kernel(plan, e, probe) || probe.conv.up_C != up.C) continue;   // the MFMA main kernel must take it
        cv.extra_in = {rz.in[0]};
        cv.name += " [+ upsample of " + rz.name + "]";
        plan.ops.erase(plan.ops.begin() + k);
        --k;
    }
}

// kINT8: which NHWC tensors live in int8.  An owning tensor (a conv output, or a concat buffer several producers write
// slices of) becomes int8 when it has a calibrated scale and EVERY op touching it can work on int8 in place: MFMA-eligible
// convolutions (as producer, consumer or residual) and nearest resizes.  Anything else (pool chains, the fused detect
// head, layout conversions, plugins, depth-to-space ...) keeps the tensor in fp16, and a convolution simply dequantises /
// requantises at that boundary in its epilogue.  The scale is a property of the OWNER, so all producers of a concat
// buffer quantise to the same scale (TensorRT reaches the same end by forcing equal scales on concat inputs).
// `veto`: owners that an earlier attempt put in int8 and the kernel choice then could not serve (see assign_int8_served()).
void assign_int8(Plan& plan, const PassInputs& e, const std::vector<char>& veto) {
    if (!e.int8 || e.dt != DT_F16) return;
    const int nt = (int)plan.tensors.size();
    std::vector<char> cand(nt, 0);
    for (const PTensor& t : plan.tensors)
        if (t.parent < 0 && t.layout == LAY_NHWC && t.dtype == DT_F16 && t.net_tensor >= 0 && t.net_tensor < (int)e.tensor_scale.size() &&
            e.tensor_scale[t.net_tensor] > 0.f && t.C % 16 == 0 && t.nmul == 1 && !is_binding_tensor(plan, t.id) && !veto[t.id])
            cand[t.id] = 1;
    auto view_ok = [&](int t) {
        int off = 0;
        owner_of(plan, t, &off);
        return off % 16 == 0 && plan.tensors[t].C % 16 == 0;
    };
    auto conv_ok = [&](const POp& op) {
        const ConvArgs& a = op.conv;
        return op.kind == OP_CONV && !op.stem && !op.from_deconv && a.groups == 1 && a.dil_h == 1 && a.dil_w == 1 && a.kh * a.kw <= 30;
    };
    for (const POp& op : plan.ops) {
        for (size_t j = 0; j < op.in.size(); ++j) {
            const PTensor& t = plan.tensors[op.in[j]];
            if (t.layout != LAY_NHWC) continue;
            bool ok = false;
            if (conv_ok(op)) ok = view_ok(op.in[j]) && (j > 0 || op.conv.kh * op.conv.kw * t.C >= 32);
            else if (op.kind == OP_RESIZE) ok = view_ok(op.in[j]);
            if (!ok) cand[owner_of(plan, op.in[j])] = 0;
        }
        for (int o : op.out) {
            if (plan.tensors[o].layout != LAY_NHWC) continue;
            const bool ok = (conv_ok(op) || op.kind == OP_RESIZE) && view_ok(o);
            if (!ok) cand[owner_of(plan, o)] = 0;
        }
    }
    for (bool changed = true; changed;) {
        changed = false;
        auto tie = [&](int a, int b) {  // both int8 or neither
            if (cand[a] != cand[b]) {
                cand[a] = cand[b] = 0;
                changed = true;
            }
        };
        for (const POp& op : plan.ops) {
            if (op.kind == OP_CONV && op.in.size() > 1) tie(owner_of(plan, op.in[1]), owner_of(plan, op.out[0]));
            if (op.kind == OP_RESIZE) tie(owner_of(plan, op.in[0]), owner_of(plan, op.out[0]));
        }
    }
    for (PTensor& t : plan.tensors) {
        if (t.layout != LAY_NHWC) continue;
        const int o = owner_of(plan, t.id);
        if (!cand[o]) continue;
        t.dtype = DT_I8;
        t.scale = e.tensor_scale[plan.tensors[o].net_tensor];
    }
}

// kINT8: assign, then ask the kernel choice itself whether every convolution that touches an int8 tensor gets the MFMA path
// (K >= 32, channel / offset / stride alignment, < 2 GB images ... - conditions the assignment's own screen does not repeat).
// A convolution that does not takes its tensors out of the race and the assignment runs again; candidates only shrink, so
// this ends, with such layers in fp16 as the builder flag promises (capi.cpp: "fall back to fp16").
void assign_int8_served(Plan& plan, const PassInputs& e) {
    if (e.int8 && e.dt == DT_F16) {
        std::vector<char> veto(plan.tensors.size(), 0);
        for (;;) {
            assign_int8(plan, e, veto);
            bool again = false;
            for (const POp& op : plan.ops) {
                if (op.kind != OP_CONV && op.kind != OP_DECONV) continue;
                bool any8 = plan.tensors[op.out[0]].dtype == DT_I8;
                for (int t : op.in) any8 = any8 || plan.tensors[t].dtype == DT_I8;
                if (!any8) continue;
                POp probe = op;
                if (op.kind == OP_CONV && choose_conv_kernel(plan, e, probe)) continue;
                for (int t : op.in)
                    if (plan.tensors[t].dtype == DT_I8) veto[owner_of(plan, t)] = 1;
                if (plan.tensors[op.out[0]].dtype == DT_I8) veto[owner_of(plan, op.out[0])] = 1;
                again = true;
            }
            if (!again) break;
            for (PTensor& t : plan.tensors)
                if (t.dtype == DT_I8) {
                    t.dtype = DT_F16;
                    t.scale = 0.f;
                }
        }
    }
}

void assign_storages(Plan& plan) {
    // storages for owners
    for (auto& t : plan.tensors) {
        if (t.parent >= 0 || t.storage >= 0) continue;
        Storage s;
        s.kind = ST_ARENA;
        s.bytes = tensor_bytes(plan, t);
        t.storage = (int)plan.storages.size();
        plan.storages.push_back(s);
    }
    // views share their owner's storage
    for (auto& t : plan.tensors) t.storage = plan.tensors[owner_of(plan, t.id)].storage;
    // binding storages take their size from the bound tensor
    for (size_t b = 0; b < plan.binding_ptensor.size(); ++b) {
        const PTensor& t = plan.tensors[plan.binding_ptensor[b]];
        plan.storages[t.storage].bytes = tensor_bytes(plan, t);
    }
}

// convolution kernel selection now that strides/offsets are known, and the bytes each convolution moves
bool select_conv_kernels(Plan& plan, const PassInputs& e, std::string* err) {
    for (auto& op : plan.ops) {
        if (op.kind != OP_CONV && op.kind != OP_DECONV) continue;
        ConvArgs& a = op.conv;
        const PTensor& ti = plan.tensors[op.in[0]];
        const PTensor& to = plan.tensors[op.out[0]];
        if (op.stem && (e.dt == DT_F16 ? (to.ld % 8 || to.rcoff % 8) : (to.ld % 4 || to.rcoff % 4))) return fail(err, op.name + ": stem convolution output is not 16-byte aligned");
        choose_conv_kernel(plan, e, op);
        if (!op.extra_in.empty() && !op.igemm) return fail(err, op.name + ": folded upsample on a convolution that cannot take the MFMA path");
        if ((ti.dtype == DT_I8 || to.dtype == DT_I8 || (op.in.size() > 1 && plan.tensors[op.in[1]].dtype == DT_I8)) && !op.igemm)
            return fail(err, op.name + ": int8 tensor on a convolution that cannot take the MFMA path");
        const double es_in = (double)dtype_size(ti.dtype), es_out = (double)dtype_size(to.dtype);
        const double cin_real = ti.dtype == DT_I8 ? 2.0 * a.Cin : (double)a.Cin;
        // (a folded upsample reads up_C of its input channels from a tensor a quarter the size)
        const double in_elems = (double)a.H * a.W * (cin_real - a.up_C) + (double)a.up_H * a.up_W * a.up_C;
        op.bytes = to.nmul * ((op.stem ? 4.0 : es_in) * in_elems + es_out * (double)a.Ho * a.Wo * a.Cout * (op.in.size() > 1 ? 2 : 1));
    }
    return true;
}

// plugins: configure + workspace
bool configure_plugins(Plan& plan, std::string* err) {
    for (size_t k = 0; k < plan.ops.size(); ++k) {
        POp& op = plan.ops[k];
        if (op.kind != OP_PLUGIN) continue;
        // explicit batch: configurePlugin / getWorkspaceSize see the dims without the leading batch dimension, and that as maxBatch
        const bool eb = plan.explicit_batch && op.i[0] > 0;
        auto strip = [&](Dims d) {
            if (eb && d.nb > 0) {
                for (int q = 1; q < d.nb; ++q) d.d[q - 1] = d.d[q];
                --d.nb;
            }
            return to_c(d);
        };
        const int mb = eb ? op.i[0] : plan.max_batch;
        std::vector<trtx_dims> din, dout;
        for (int t : op.in) din.push_back(strip(plan.tensors[t].dims));
        for (int t : op.out) dout.push_back(strip(plan.tensors[t].dims));
        if (op.plugin->v.configure &&
            op.plugin->v.configure(op.plugin->v.self, din.data(), (int)din.size(), dout.data(), (int)dout.size(), mb) != 0)
            return fail(err, op.name + ": plugin configurePlugin rejected the tensor shapes");
        op.ws_bytes = op.plugin->v.workspace_size ? op.plugin->v.workspace_size(op.plugin->v.self, mb) : 0;
        for (int t : op.in) op.bytes += 4.0 * plan.tensors[t].dims.volume();
        for (int t : op.out) op.bytes += 4.0 * plan.tensors[t].dims.volume();
    }
    return true;
}

// SPPF (yolov8/src/block.cpp:214-237): y1 = maxpool_k(x), y2 = maxpool_k(y1), y3 = maxpool_k(y2), stride 1,
// 'same' padding.  Three tiny launches (20x20 maps) become one that keeps the map in LDS.
void chain_sppf_pools(Plan& plan, const PassInputs& e) {
    for (size_t k = 0; k + 2 < plan.ops.size(); ++k) {
        auto same_max = [&](const POp& o) {
            return o.kind == OP_POOL && o.i[0] == POOL_MAX && o.i[1] == o.i[2] && (o.i[1] & 1) && o.i[3] == 1 && o.i[4] == 1 &&
                   o.i[5] == o.i[1] / 2 && o.i[6] == o.i[1] / 2;
        };
        POp &a = plan.ops[k], &b = plan.ops[k + 1], &c3 = plan.ops[k + 2];
        if (!same_max(a) || !same_max(b) || !same_max(c3) || a.i[1] != b.i[1] || a.i[1] != c3.i[1]) continue;
        if (b.in[0] != a.out[0] || c3.in[0] != b.out[0] || (e.dt != DT_F16 && e.dt != DT_F32)) continue;
        const PTensor& tx = plan.tensors[a.in[0]];
        const int cv = e.dt == DT_F16 ? 8 : 4;   // channels per 16-byte chunk (round 6: fp32 engines too)
        bool ok = tx.C % cv == 0 && tx.ld % cv == 0 && tx.rcoff % cv == 0 && (long)(tx.H + a.i[1] - 1) * (tx.W + a.i[1] - 1) * 32 <= 64 * 1024 && tx.nmul == 1;
        for (const POp* o : {&a, &b, &c3}) {
            const PTensor& ty = plan.tensors[o->out[0]];
            ok = ok && ty.ld % cv == 0 && ty.rcoff % cv == 0 && ty.H == tx.H && ty.W == tx.W && ty.C == tx.C;
        }
        if (!ok) continue;
        a.kind = OP_POOL_CHAIN;
        a.name += " [x3 chained]";
        a.out = {a.out[0], b.out[0], c3.out[0]};
        plan.ops.erase(plan.ops.begin() + k + 1, plan.ops.begin() + k + 3);
    }
}

// SPP / SPPCSPC (yolov7/src/block.cpp:140-148, model.cpp:1905-1916): y1 = maxpool_k(x), y2 = maxpool_{2k-1}(x), y3 = maxpool_{3k-2}(x),
// stride 1, 'same' padding, all three reading x.  A max-pool that skips its padding (pool_kernel: -inf start, out-of-range taps
// skipped) composes - the k-window of k-window maxima is the (2k-1)-window maximum over the in-range taps, no rounding anywhere - so
// the three are bit for bit the three outputs of the chained kernel on x.  The pools may come in any order; between the first and the
// last of them no other op may write x (or one of the three outputs: it would have to run between two of them).  The three-in-a-row
// form of chain_sppf_pools has run before this pass and has k, k, k; no network that it or this pass takes is taken by the other.
void chain_spp_parallel_pools(Plan& plan, const PassInputs& e) {
    if (!e.opt.spp_parallel_chain || e.int8 || (e.dt != DT_F16 && e.dt != DT_F32)) return;
    auto same_max = [&](const POp& o) {
        return o.kind == OP_POOL && o.i[0] == POOL_MAX && o.i[1] == o.i[2] && (o.i[1] & 1) && o.i[3] == 1 && o.i[4] == 1 &&
               o.i[5] == o.i[1] / 2 && o.i[6] == o.i[1] / 2 && o.in.size() == 1 && o.out.size() == 1;
    };
    auto overlaps = [&](int ta, int tb) {   // NHWC tensors sharing channels of one storage
        const PTensor &a = plan.tensors[ta], &b = plan.tensors[tb];
        if (ta == tb) return true;
        if (a.storage != b.storage || a.layout != LAY_NHWC || b.layout != LAY_NHWC) return a.storage == b.storage;
        return a.rcoff < b.rcoff + std::max(b.C, 1) && b.rcoff < a.rcoff + std::max(a.C, 1);
    };
    for (size_t k = 0; k + 2 < plan.ops.size(); ++k) {
        if (!same_max(plan.ops[k])) continue;
        const int x = plan.ops[k].in[0];
        // the other two pools of x, within a short window (the builders emit them back to back)
        std::vector<size_t> idx{k};
        const size_t last = std::min(plan.ops.size(), k + 8);
        for (size_t j = k + 1; j < last && idx.size() < 3; ++j)
            if (same_max(plan.ops[j]) && plan.ops[j].in[0] == x) idx.push_back(j);
        if (idx.size() != 3) continue;
        // by kernel size: k, 2k - 1, 3k - 2
        std::vector<size_t> by = idx;
        std::sort(by.begin(), by.end(), [&](size_t p, size_t q) { return plan.ops[p].i[1] < plan.ops[q].i[1]; });
        const int k1 = plan.ops[by[0]].i[1];
        if (k1 < 3 || plan.ops[by[1]].i[1] != 2 * k1 - 1 || plan.ops[by[2]].i[1] != 3 * k1 - 2) continue;
        const PTensor& tx = plan.tensors[x];
        const int cv = e.dt == DT_F16 ? 8 : 4;
        bool ok = tx.layout == LAY_NHWC && tx.dtype == e.dt && tx.C % cv == 0 && tx.ld % cv == 0 && tx.rcoff % cv == 0 &&
                  (long)(tx.H + k1 - 1) * (tx.W + k1 - 1) * 32 <= 64 * 1024 && tx.nmul == 1;
        for (size_t p : by) {
            const PTensor& ty = plan.tensors[plan.ops[p].out[0]];
            ok = ok && ty.layout == LAY_NHWC && ty.dtype == e.dt && ty.ld % cv == 0 && ty.rcoff % cv == 0 && ty.H == tx.H && ty.W == tx.W &&
                 ty.C == tx.C && !overlaps(plan.ops[p].out[0], x);
        }
        ok = ok && !overlaps(plan.ops[by[0]].out[0], plan.ops[by[1]].out[0]) && !overlaps(plan.ops[by[0]].out[0], plan.ops[by[2]].out[0]) &&
             !overlaps(plan.ops[by[1]].out[0], plan.ops[by[2]].out[0]);
        // an op between them: it must neither write x nor touch an output of the three
        for (size_t j = k + 1; ok && j < idx[2]; ++j) {
            if (j == idx[1]) continue;
            const POp& o = plan.ops[j];
            for (int t : o.out) ok = ok && !overlaps(t, x);
            for (size_t p : by) {
                const int y = plan.ops[p].out[0];
                for (int t : o.out) ok = ok && !overlaps(t, y);
                for (int t : o.in) ok = ok && !overlaps(t, y);
                for (int t : o.extra_in) ok = ok && !overlaps(t, y);
            }
        }
        if (!ok) continue;
        const int y1 = plan.ops[by[0]].out[0], y2 = plan.ops[by[1]].out[0], y3 = plan.ops[by[2]].out[0];
        POp& a = plan.ops[k];
        a.kind = OP_POOL_CHAIN;
        a.name += " [x3 parallel, chained]";
        a.i[1] = a.i[2] = k1;
        a.i[5] = a.i[6] = k1 / 2;
        a.out = {y1, y2, y3};
        plan.ops.erase(plan.ops.begin() + idx[2]);
        plan.ops.erase(plan.ops.begin() + idx[1]);
    }
}

// Per op, the earlier ops it must run after: RAW, WAR and WAW at (storage, channel / element range) granularity, sorted.
std::vector<std::vector<int>> op_dependencies(const Plan& plan) {
    const int nops = (int)plan.ops.size();
    struct Range { int storage; long lo, hi; int op; bool write; };
    auto access_of = [&](int t, int op, bool write) {
        const PTensor& pt = plan.tensors[t];
        Range a{pt.storage, 0, 0, op, write};
        if (pt.layout == LAY_NHWC) {
            a.lo = pt.rcoff;
            a.hi = pt.rcoff + (pt.parent < 0 && pt.Calloc > pt.C ? pt.Calloc : pt.C);  // the layout pass zero-fills its padding
        } else {
            a.lo = pt.reoff;
            a.hi = pt.reoff + pt.dims.volume();
        }
        return a;
    };
    std::vector<std::vector<int>> deps(nops);
    std::vector<Range> log;
    for (int k = 0; k < nops; ++k) {
        const POp& op = plan.ops[k];
        std::vector<Range> mine;
        for (int t : op.in) mine.push_back(access_of(t, k, false));
        for (int t : op.extra_in) mine.push_back(access_of(t, k, false));
        for (int t : op.out) mine.push_back(access_of(t, k, true));
        for (const Range& m : mine)
            for (const Range& o : log)
                if (o.storage == m.storage && o.lo < m.hi && m.lo < o.hi && (o.write || m.write) && o.op != k) deps[k].push_back(o.op);
        std::sort(deps[k].begin(), deps[k].end());
        deps[k].erase(std::unique(deps[k].begin(), deps[k].end()), deps[k].end());
        log.insert(log.end(), mine.begin(), mine.end());
    }
    return deps;
}

// Transitive ancestors of every op, as bit rows: over the dependency edges and, with `lane_order`, over the issue order of each lane too
// (the happens-before relation of the schedule).
struct Ancestors {
    int words;
    std::vector<uint64_t> bits;
    bool has(int a, int of) const { return (bits[(size_t)of * words + (a >> 6)] >> (a & 63)) & 1ull; }
};
Ancestors ancestors(const Plan& plan, const std::vector<std::vector<int>>& deps, bool lane_order) {
    const int n = (int)deps.size();
    Ancestors anc{(n + 63) / 64, {}};
    anc.bits.assign((size_t)n * anc.words, 0);
    std::vector<int> prev_on_lane(plan.num_lanes, -1);
    for (int k = 0; k < n; ++k) {
        uint64_t* row = &anc.bits[(size_t)k * anc.words];
        auto absorb = [&](int d) {
            for (int w = 0; w < anc.words; ++w) row[w] |= anc.bits[(size_t)d * anc.words + w];
            row[d >> 6] |= 1ull << (d & 63);
        };
        for (int d : deps[k]) absorb(d);
        if (!lane_order) continue;
        const int lane = plan.ops[k].lane;
        if (prev_on_lane[lane] >= 0) absorb(prev_on_lane[lane]);
        prev_on_lane[lane] = k;
    }
    return anc;
}

// Independent convolutions of one kernel instantiation -> one launch (OP_CONV_GROUP; kernels/conv_igemm.hip conv_igemm_group_f16_kernel).
// The YOLOv8 detect head is six chains of depth three over three pyramid levels (yolov8/src/model.cpp:188-251): cv2.{0,1,2}.0 are three
// independent 3x3 convolutions to 64 channels, cv3.{0,1,2}.0 three to 80, and so on down the chains - 18 launches, of which the 20x20 and
// 40x40 levels (100 / 400 tiles at batch 32 for 256 CUs) mostly pay the per-launch floor.  Members must be pairwise independent (no
// dependency path either way), have the same filter, stride, Cout, activation and residual-ness and sit at the same height above the
// plan's sinks (so that they are the same LAYER of sibling branches, not unrelated work that happens to fit) and pass conv_igemm_group_supported().  The ops are then re-ordered
// (a topological order of the dependency graph with each group contracted to one node; a grouping that would close a cycle between
// two groups is dropped) and every group's members are replaced by one op whose in / out are the unions.  Each member is computed
// exactly as its own launch computes it: bit-identical outputs.  TRTX_GROUP_CONVS=0 keeps one launch per convolution (A/B, tests).
void group_convs(Plan& plan, const PassInputs& e) {
    if (e.dt != DT_F16 || CalibrationLowering::active()) return;   // (INT8 plans group too since round 5: members of one storage mix - same in / out / shortcut int8 flags)
    const bool mark_only = !e.opt.group_convs;   // TRTX_GROUP_CONVS=0: one launch per convolution, but the would-be members keep the group's K order (WSK_OFF): same bits
    const int n = (int)plan.ops.size();
    if (n < 2 || n > 4096) return;
    const std::vector<std::vector<int>> deps = op_dependencies(plan);   // in the current order
    const Ancestors anc = ancestors(plan, deps, false);
    auto args_at_max_batch = [&](const POp& op) {
        ConvArgs a = op.conv;
        const PTensor& ti = plan.tensors[op.in[0]];
        a.N = (ti.nfix ? ti.nfix : plan.max_batch) * ti.nmul;
        a.M = a.N * a.Ho * a.Wo;
        a.residual = op.in.size() > 1 ? reinterpret_cast<const void*>(1) : nullptr;   // presence only (alignment rules look at ld_res)
        return a;
    };
    auto candidate = [&](const POp& op) {
        if (op.kind != OP_CONV || !op.igemm || op.stem || op.from_deconv || !op.extra_in.empty()) return false;
        ConvArgs two[2] = {args_at_max_batch(op), args_at_max_batch(op)};
        return conv_igemm_group_supported(two, 2);
    };
    auto same_layer_shape = [&](const POp& x, const POp& y) {
        const ConvArgs &a = x.conv, &b = y.conv;
        return a.kh == b.kh && a.kw == b.kw && a.stride_h == b.stride_h && a.stride_w == b.stride_w && a.pad_h == b.pad_h && a.pad_w == b.pad_w &&
               a.Cout == b.Cout && a.act1 == b.act1 && a.act2 == b.act2 && a.alpha1 == b.alpha1 && a.alpha2 == b.alpha2 && x.in.size() == y.in.size() &&
               a.in_i8 == b.in_i8 && a.out_i8 == b.out_i8 && a.res_i8 == b.res_i8;
    };
    // height = longest dependency path from an op down to a sink: sibling branches that end in the same consumer (the three levels'
    // arms into the fused head op) put their corresponding layers at equal heights; a bottleneck of the neck that merely has the same
    // shape as an arm's convolution sits higher and stays out of the arm's group
    std::vector<int> height(n, 0);
    for (int k = n - 1; k >= 0; --k)
        for (int d : deps[k]) height[d] = std::max(height[d], height[k] + 1);
    std::vector<int> group_of(n, -1);
    std::vector<std::vector<int>> groups;
    // the dependency graph with every group contracted to one node; nodes are numbered by the old position of their first member
    struct Contracted { std::vector<int> first_op, indeg; std::vector<std::vector<int>> succ; };
    auto contract = [&]() {
        Contracted c;
        std::vector<int> node(n), gnode(groups.size(), -1);
        for (int k = 0; k < n; ++k) {
            if (group_of[k] >= 0 && gnode[group_of[k]] >= 0) {
                node[k] = gnode[group_of[k]];
                continue;
            }
            if (group_of[k] >= 0) gnode[group_of[k]] = (int)c.first_op.size();
            node[k] = (int)c.first_op.size();
            c.first_op.push_back(k);
        }
        c.succ.resize(c.first_op.size());
        c.indeg.assign(c.first_op.size(), 0);
        for (int k = 0; k < n; ++k)
            for (int d : deps[k])
                if (node[d] != node[k]) {
                    c.succ[node[d]].push_back(node[k]);
                    ++c.indeg[node[k]];
                }
        return c;
    };
    auto acyclic = [&]() {
        Contracted c = contract();
        const int nn = (int)c.first_op.size();
        std::vector<int>& indeg = c.indeg;
        const std::vector<std::vector<int>>& succ = c.succ;
        std::vector<int> q;
        for (int v = 0; v < nn; ++v)
            if (!indeg[v]) q.push_back(v);
        size_t done = 0;
        while (done < q.size()) {
            const int v = q[done++];
            for (int w : succ[v])
                if (--indeg[w] == 0) q.push_back(w);
        }
        return (int)q.size() == nn;
    };
    for (int k = 0; k < n; ++k) {
        if (group_of[k] >= 0 || !candidate(plan.ops[k])) continue;
        std::vector<int> mem = {k};
        std::vector<ConvArgs> margs = {args_at_max_batch(plan.ops[k])};
        for (int j = k + 1; j < n && (int)mem.size() < kMaxConvGroup; ++j) {
            if (group_of[j] >= 0 || height[j] != height[k] || !candidate(plan.ops[j]) || !same_layer_shape(plan.ops[k], plan.ops[j])) continue;
            bool indep = true;
            for (int m : mem) indep = indep && !anc.has(m, j) && !anc.has(j, m);
            if (!indep) continue;
            margs.push_back(args_at_max_batch(plan.ops[j]));
            // the operand path (t_rs: registers or LDS-DMA, the same bits either way) is a per-layer heuristic; a group runs on the
            // path of its member with the most rows.  Checked on a COPY (a rejected candidate used to leave its t_rs on the others)
            std::vector<ConvArgs> trial = margs;
            int big = 0;
            for (size_t q = 1; q < trial.size(); ++q)
                if (trial[q].M > trial[big].M) big = (int)q;
            const int rs = trial[big].t_rs;
            for (ConvArgs& ma : trial) ma.t_rs = rs;
            if (!conv_igemm_group_supported(trial.data(), (int)trial.size())) {
                margs.pop_back();
                continue;
            }
            mem.push_back(j);
        }
        if (mem.size() < 2) continue;
        const int gi = (int)groups.size();
        groups.push_back(mem);
        for (int m : mem) group_of[m] = gi;
        if (!acyclic()) {   // (two groups each waiting for a member of the other): leave these convolutions alone
            for (int m : mem) group_of[m] = -1;
            groups.pop_back();
        }
    }
    if (groups.empty()) return;
    if (mark_only) {
        for (const auto& mem : groups)
            for (int m : mem) {
                plan.ops[m].conv.t_wsk = WSK_OFF;
                plan.ops[m].conv.k_pinned = 1;   // ... and the tuner keeps it that way (its candidates for a pinned layer all walk K as the main kernel does)
            }
        return;
    }
    // new order: Kahn over the contracted graph, ready nodes taken in the order of their first member's old position
    Contracted c = contract();
    const int nn = (int)c.first_op.size();
    std::vector<int>&indeg = c.indeg, &first_op = c.first_op;
    const std::vector<std::vector<int>>& succ = c.succ;
    std::vector<char> emitted(nn, 0);
    std::vector<POp> out;
    out.reserve(nn);
    for (int step = 0; step < nn; ++step) {
        int pick = -1;
        for (int v = 0; v < nn; ++v)
            if (!emitted[v] && indeg[v] == 0) { pick = v; break; }   // nodes are numbered by first member: the lowest ready one
        if (pick < 0) return;   // cannot happen (acyclic() held); keep the plan as it was
        emitted[pick] = 1;
        for (int w : succ[pick]) --indeg[w];
        const int k0 = first_op[pick];
        if (group_of[k0] < 0) {
            out.push_back(plan.ops[k0]);
            continue;
        }
        POp g;
        g.kind = OP_CONV_GROUP;
        g.dtype = plan.ops[k0].dtype;
        g.conv = plan.ops[k0].conv;
        int big = groups[group_of[k0]][0];
        for (int m : groups[group_of[k0]])
            if ((long)plan.ops[m].conv.Ho * plan.ops[m].conv.Wo * plan.tensors[plan.ops[m].in[0]].nmul >
                (long)plan.ops[big].conv.Ho * plan.ops[big].conv.Wo * plan.tensors[plan.ops[big].in[0]].nmul)
                big = m;
        for (int m : groups[group_of[k0]]) {
            POp mo = plan.ops[m];
            mo.conv.t_rs = plan.ops[big].conv.t_rs;
            // ONE summation order per member, grouped or not: the grouped kernel walks K as the main kernel does, so the member's own launch -
            // the fallback the executor takes at a batch where the members no longer share an instantiation, and TRTX_GROUP_CONVS=0 - must not pick
            // the wave-split-K variant (different K order: the same engine rounded differently depending on batch size and on the switch)
            mo.conv.t_wsk = WSK_OFF;
            mo.conv.k_pinned = 1;
            g.group.push_back(mo);
            g.name += (g.name.empty() ? "" : " + ") + mo.name;
            for (int t : mo.in)
                if (std::find(g.in.begin(), g.in.end(), t) == g.in.end()) g.in.push_back(t);
            g.out.push_back(mo.out[0]);
            g.flops += mo.flops;
            g.bytes += mo.bytes;
        }
        g.name = "[group of " + std::to_string(g.group.size()) + "] " + g.name;
        out.push_back(std::move(g));
    }
    plan.ops = std::move(out);
}

// The stem and the stride-2 3x3 convolution behind it in one launch (kernels/conv_stem_pair.hip): marks the convolution (POp::stem_pair); the op list, the
// tensors and the arena stay what they are - the executor issues the fused launch at the marked op and nothing at the stem, and the tensor between them
// keeps its block, unwritten.  Marked when the stem is the op right before, the tensor between them has no other reader or writer and is not a binding,
// the plan is fp16 without an int8 side, and conv_stem_pair_possible() takes the two layers at the largest batch.  Not part of the serialized network:
// re-derived wherever a plan is lowered.  TRTX_STEM_PAIR=0 marks nothing (A/B, tests): every launch is then the two-kernel form's.
void mark_stem_pair(Plan& plan, const PassInputs& e) {
    if (!e.opt.stem_pair || e.dt != DT_F16 || e.int8 || CalibrationLowering::active()) return;   // (the calibration engine's observer reads every tensor an op writes)
    const int n = (int)plan.ops.size();
    for (int k = 0; k + 1 < n; ++k) {
        const POp& st = plan.ops[k];
        POp& cv = plan.ops[k + 1];
        if (st.kind != OP_CONV || !st.stem || st.conv.f32 || st.out.size() != 1) continue;
        if (cv.kind != OP_CONV || !cv.igemm || cv.stem || cv.from_deconv || cv.in.size() != 1 || !cv.extra_in.empty() || cv.in[0] != st.out[0]) continue;
        const PTensor& mid = plan.tensors[st.out[0]];
        if (mid.storage < 0 || plan.storages[mid.storage].kind != ST_ARENA || is_binding_tensor(plan, mid.id) || is_binding_tensor(plan, owner_of(plan, mid.id))) continue;
        bool shared = false;   // any other op (or member of a grouped launch) that touches the block the intermediate lives in
        auto touches = [&](const POp& op) {
            for (const std::vector<int>* v : {&op.in, &op.out, &op.extra_in})
                for (int t : *v)
                    if (plan.tensors[t].storage == mid.storage) return true;
            return false;
        };
        for (int j = 0; j < n && !shared; ++j) {
            if (j == k || j == k + 1) continue;
            shared = touches(plan.ops[j]);
            for (const POp& m : plan.ops[j].group) shared = shared || touches(m);
        }
        if (shared) continue;
        ConvArgs a = st.conv, b = cv.conv;   // as execute_plan fills them at the largest batch (pointers unset: geometry only)
        const PTensor& t_in = plan.tensors[st.in[0]];
        a.N = plan.explicit_batch ? (int)t_in.dims.d[0] : plan.max_batch;
        a.M = a.N * a.Ho * a.Wo;
        b.N = (mid.nfix ? mid.nfix : plan.max_batch) * mid.nmul;
        b.M = b.N * b.Ho * b.Wo;
        if (!conv_stem_pair_possible(a, b)) continue;
        cv.stem_pair = true;
    }
}

// The two 3x3 convolutions of a 16-channel bottleneck in one launch (kernels/conv_bneck_pair.hip; YOLOv8n's first C2f block): marks the SECOND convolution
// (POp::bneck_pair); the op list, the tensors and the arena stay what they are - the executor issues the fused launch at the marked op and nothing at the op
// before it, and the tensor between them keeps its block, unwritten.  Marked when both are plain implicit-GEMM convolutions right behind each other, the first
// without a shortcut, the second with none or with exactly the first one's input; the tensor between them is an arena tensor of its own (no view, no binding)
// that no other op or member of a grouped launch touches; the output is not a view that overlaps the input (other workgroups still read it as halo - and
// plan_arena() keeps the output's BLOCK off the input's by counting the first op's inputs as live at the marked op); the plan is fp16
// without an int8 side; and conv_bneck_pair_possible() takes the two layers at the largest batch.  Wider pairs (32 channels and up) are not taken: their
// weights do not fit registers beside four workgroups per CU.  finalize_plan() drops a mark whose two ops ended up on different lanes.
// Not part of the serialized network: re-derived wherever a plan is lowered.  TRTX_BNECK_PAIR=0 marks nothing (A/B, tests): every launch is then the
// two-kernel form's.
void mark_bneck_pair(Plan& plan, const PassInputs& e) {
    if (!e.opt.bneck_pair || e.dt != DT_F16 || e.int8 || CalibrationLowering::active()) return;   // (the calibration engine's observer reads every tensor an op writes)
    const int n = (int)plan.ops.size();
    auto plain = [](const POp& op) { return op.kind == OP_CONV && op.igemm && !op.stem && !op.stem_pair && !op.bneck_pair && !op.from_deconv && op.extra_in.empty() && op.out.size() == 1; };
    for (int k = 0; k + 1 < n; ++k) {
        const POp& c0 = plan.ops[k];
        POp& c1 = plan.ops[k + 1];
        if (!plain(c0) || !plain(c1) || c0.in.size() != 1 || c1.in.empty() || c1.in.size() > 2 || c1.in[0] != c0.out[0]) continue;
        if (c1.in.size() == 2 && c1.in[1] != c0.in[0]) continue;   // a shortcut from anywhere else
        const PTensor& mid = plan.tensors[c0.out[0]];
        if (mid.parent >= 0 || mid.storage < 0 || plan.storages[mid.storage].kind != ST_ARENA || is_binding_tensor(plan, mid.id)) continue;
        bool shared = false;   // any other op (or member of a grouped launch) that touches the block the intermediate lives in
        auto touches = [&](const POp& op) {
            for (const std::vector<int>* v : {&op.in, &op.out, &op.extra_in})
                for (int t : *v)
                    if (plan.tensors[t].storage == mid.storage) return true;
            return false;
        };
        for (int j = 0; j < n && !shared; ++j) {
            if (j == k || j == k + 1) continue;
            shared = touches(plan.ops[j]);
            for (const POp& m : plan.ops[j].group) shared = shared || touches(m);
        }
        const PTensor &t_in = plan.tensors[c0.in[0]], &t_out = plan.tensors[c1.out[0]];
        if (shared || t_in.storage == mid.storage || t_out.storage == mid.storage) continue;
        if (t_in.layout != LAY_NHWC || t_out.layout != LAY_NHWC) continue;
        if (t_in.storage == t_out.storage && t_in.rcoff < t_out.rcoff + std::max(t_out.C, 1) && t_out.rcoff < t_in.rcoff + std::max(t_in.C, 1)) continue;
        ConvArgs a = c0.conv, b = c1.conv;   // as execute_plan fills them at the largest batch (pointers unset: geometry only)
        a.N = (t_in.nfix ? t_in.nfix : plan.max_batch) * t_in.nmul;
        a.M = a.N * a.Ho * a.Wo;
        b.N = (mid.nfix ? mid.nfix : plan.max_batch) * mid.nmul;
        b.M = b.N * b.Ho * b.Wo;
        b.residual = c1.in.size() > 1 ? reinterpret_cast<const void*>(1) : nullptr;   // presence only
        if (!conv_bneck_pair_possible(a, b)) continue;
        c1.bneck_pair = true;
        ++k;   // (the marked op starts no pair of its own)
    }
}

// Two grouped launches whose members read the same tensors in one launch (the dual tile of kernels/igemm_tile.h; YOLOv8's cv2.{0,1,2}.0 -> 64 and
// cv3.{0,1,2}.0 -> 80 read the same three pyramid levels): marks the SECOND group (POp::sibling_pair); kinds, names, members, tensors and the arena's blocks stay what
// they are - the executor issues the one launch at the marked op and nothing at the group before it.  Marked when both are OP_CONV_GROUP with the same member
// count, every member of one has a member of the other that reads the same tensor view with the same geometry (no shortcut on either), neither group depends on
// the other, no output shares channels of a block with an input or another output, and conv_dual_group_possible() takes the members at the largest batch.  A second
// group that does not directly follow the first is moved there if nothing in between is one of its ancestors (RAW, WAR or WAW: the order stays topological);
// otherwise the pair is left alone.  Only plans of ONE lane are looked at - engines built for several contexts in flight, setMaxAuxStreams(0): with auxiliary
// streams assign_lanes() puts two independent groups on different streams, where they overlap, and the pair would lose its mark again (finalize_plan() drops a
// mark whose two ops sit on different lanes or whose first op another lane waits for) after its second group was moved for nothing: such plans stay exactly
// what they were.  Not part of the serialized network.  TRTX_SIBLING_PAIR=0 marks nothing (A/B, tests).
int lane_limit(const PassInputs& e) {
    int max_lanes = e.max_aux_streams >= 0 ? 1 + e.max_aux_streams : 4;  // IBuilderConfig::setMaxAuxStreams
    if (e.opt.lanes > 0) max_lanes = std::max(1, std::min(16, e.opt.lanes));  // A/B override (TRTX_LANES)
    return max_lanes;
}
void mark_sibling_pair(Plan& plan, const PassInputs& e) {
    if (!e.opt.sibling_pair || e.dt != DT_F16 || e.int8 || CalibrationLowering::active()) return;
    if (lane_limit(e) > 1) return;   // (see above: with several lanes the plan, its op order included, stays what it was)
    const int n = (int)plan.ops.size();
    if (n < 2 || n > 4096) return;
    auto member_args = [&](const POp& m) {
        ConvArgs a = m.conv;   // as execute_plan fills them at the largest batch (pointers unset: geometry only)
        const PTensor& ti = plan.tensors[m.in[0]];
        a.N = (ti.nfix ? ti.nfix : plan.max_batch) * ti.nmul;
        a.M = a.N * a.Ho * a.Wo;
        return a;
    };
    auto shares_elements = [&](int t, int u) {
        const PTensor &x = plan.tensors[t], &y = plan.tensors[u];
        if (x.storage != y.storage) return false;
        if (x.layout != LAY_NHWC || y.layout != LAY_NHWC) return true;
        return x.rcoff < y.rcoff + std::max(y.C, 1) && y.rcoff < x.rcoff + std::max(x.C, 1);
    };
    auto mark_one = [&]() {   // (a move changes the op indices: dependencies are taken anew for every pair)
        const std::vector<std::vector<int>> deps = op_dependencies(plan);
        const Ancestors anc = ancestors(plan, deps, false);
        for (int i = 0; i + 1 < n; ++i) {
            const POp& a = plan.ops[i];
            if (a.kind != OP_CONV_GROUP || a.sibling_pair || plan.ops[i + 1].sibling_pair || a.group.empty() || (int)a.group.size() > kMaxDualGroup) continue;
            for (int j = i + 1; j < n; ++j) {
                const POp& b = plan.ops[j];
                if (b.kind != OP_CONV_GROUP || b.sibling_pair || (j + 1 < n && plan.ops[j + 1].sibling_pair) || b.group.size() != a.group.size()) continue;
                // members pairwise on the same tensor view (b's in the order of a's), the 64-wide side first
                std::vector<ConvArgs> xa, xb;
                bool ok = true;
                for (const POp& ma : a.group) {
                    const POp* mb = nullptr;
                    for (const POp& c : b.group)
                        if (c.in.size() == 1 && ma.in.size() == 1 && c.in[0] == ma.in[0]) mb = &c;
                    if (!mb || !ma.extra_in.empty() || !mb->extra_in.empty()) { ok = false; break; }
                    xa.push_back(member_args(ma));
                    xb.push_back(member_args(*mb));
                }
                if (!ok) continue;
                const int gn = (int)xa.size();
                if (!conv_dual_group_possible(xa.data(), xb.data(), gn) && !conv_dual_group_possible(xb.data(), xa.data(), gn)) continue;
                for (int t : a.out) {
                    for (int u : a.in) ok = ok && !shares_elements(t, u);
                    for (int u : b.out) ok = ok && !shares_elements(t, u);
                }
                for (int t : b.out)
                    for (int u : a.in) ok = ok && !shares_elements(t, u);
                for (int k = i; k < j; ++k) ok = ok && !anc.has(k, j);   // independent of the first group, and free to move up behind it
                if (!ok) continue;
                if (j != i + 1) std::rotate(plan.ops.begin() + i + 1, plan.ops.begin() + j, plan.ops.begin() + j + 1);
                plan.ops[i + 1].sibling_pair = true;
                return true;
            }
        }
        return false;
    };
    while (mark_one()) {}
}

// Lanes (= HIP streams at run time): an op continues the lane of a dependency that is still that lane's tail,
// otherwise it opens a free lane, otherwise it queues behind the lane that went idle first.  Independent branches
// (the six cv2/cv3 head chains of YOLOv8, model.cpp:224-291; FPN/SSH branches of RetinaFace) end up on different
// lanes and overlap on the GPU; a sequential network stays on lane 0.
// At most 4 by default: HIP multiplexes all streams of a process onto 4 hardware queues (GPU_MAX_HW_QUEUES), so further lanes
// only alias with each other and with the caller's own copy / post-processing streams.  Measured (YOLOv8n b32, same box):
// 6 lanes 1.335-1.353 ms vs 4 lanes 1.354-1.360 with resident inputs, but 2.56-2.74 vs 1.67-1.71 ms once a host-fed pipeline
// adds an H2D stream; ResNet-50 / RetinaFace / R-CNN are 0.5-1.3 % faster with 4.  (8 or 16 hardware queues: 2.2x slower.)
void assign_lanes(Plan& plan, const PassInputs& e, const std::vector<std::vector<int>>& deps) {
    const int nops = (int)plan.ops.size();
    const int max_lanes = lane_limit(e);
    std::vector<int> tail(max_lanes, -1);
    plan.num_lanes = 1;
    for (int k = 0; k < nops; ++k) {
        int lane = -1;
        for (int d : deps[k])
            if (tail[plan.ops[d].lane] == d && (lane < 0 || d > tail[lane])) lane = plan.ops[d].lane;
        if (lane < 0 && deps[k].empty()) lane = 0;  // sources (input conversions) stay on the caller's stream
        if (lane < 0) {
            for (int l = 0; l < max_lanes && lane < 0; ++l)
                if (tail[l] < 0) lane = l;
        }
        if (lane < 0) {
            lane = 0;
            for (int l = 1; l < max_lanes; ++l)
                if (tail[l] < tail[lane]) lane = l;
        }
        plan.ops[k].lane = lane;
        tail[lane] = k;
        plan.num_lanes = std::max(plan.num_lanes, lane + 1);
    }
    // cross-lane waits: a dependency on another lane needs an event unless an earlier wait already covers it
    std::vector<std::vector<int>> covered(max_lanes, std::vector<int>(max_lanes, -1));
    for (int k = 0; k < nops; ++k) {
        POp& op = plan.ops[k];
        for (int d : deps[k]) {
            const int ld = plan.ops[d].lane;
            if (ld == op.lane || covered[op.lane][ld] >= d) continue;
            op.wait_ops.push_back(d);
            plan.ops[d].signal = true;
            covered[op.lane][ld] = d;
        }
    }
}

// Which ops touch which arena storage, then arena offsets, first fit.  Two blocks may share memory only if every op touching one
// happens-before (`before`: dependency edges and lane order) every op touching the other (with one lane this is the classic
// disjoint-live-interval rule).
void plan_arena(Plan& plan, const Ancestors& anc) {
    const int nops = (int)plan.ops.size();
    auto before = [&](int a, int b) { return a == b || anc.has(a, b); };
    std::vector<std::vector<int>> touch(plan.storages.size());
    for (int k = 0; k < nops; ++k) {
        const POp& op = plan.ops[k];
        auto mark = [&](int t) {
            const int st = plan.tensors[t].storage;
            Storage& s = plan.storages[st];
            s.first_use = std::min(s.first_use, k);
            s.last_use = std::max(s.last_use, k);
            if (touch[st].empty() || touch[st].back() != k) touch[st].push_back(k);
        };
        for (int t : op.in) mark(t);
        for (int t : op.extra_in) mark(t);
        for (int t : op.out) mark(t);
        // a marked bottleneck pair is ONE launch, issued at this op, that reads the first convolution's input while it writes this op's output: that input is
        // live here too, so the output's block can never be placed on it (two launches may run in place, the fused kernel may not)
        if (op.bneck_pair && k > 0)
            for (int t : plan.ops[k - 1].in) mark(t);
        // a marked sibling pair is ONE launch, issued at this op, that also writes the first group's outputs: they are live here (and the inputs are this op's own)
        if (op.sibling_pair && k > 0)
            for (int t : plan.ops[k - 1].out) mark(t);
    }
    // plugin workspaces are short-lived arena blocks
    std::vector<std::pair<int, int>> ws_storage;  // (op, storage)
    for (int k = 0; k < nops; ++k) {
        const int kind = plan.ops[k].kind;
        if ((kind != OP_PLUGIN && !is_fused_head(kind) && kind != OP_HGCONV) || plan.ops[k].ws_bytes == 0) continue;
        Storage s;
        s.kind = ST_ARENA;
        s.bytes = plan.ops[k].ws_bytes;
        s.first_use = s.last_use = k;
        ws_storage.push_back({k, (int)plan.storages.size()});
        plan.storages.push_back(s);
        touch.push_back({k});
    }
    auto ordered = [&](int sa, int sb) {
        for (int x : touch[sa])
            for (int y : touch[sb])
                if (!before(x, y) || x == y) return false;
        return true;
    };
    std::vector<int> order;
    for (size_t si = 0; si < plan.storages.size(); ++si)
        if (plan.storages[si].kind == ST_ARENA && plan.storages[si].last_use >= 0) order.push_back((int)si);
    std::stable_sort(order.begin(), order.end(),
                     [&](int x, int y) { return plan.storages[x].first_use < plan.storages[y].first_use; });
    std::vector<int> placed;
    size_t arena = 0;
    for (int si : order) {
        Storage& st = plan.storages[si];
        const size_t need = align256(st.bytes);
        std::vector<std::pair<size_t, size_t>> busy;
        for (int pj : placed) {
            const Storage& o = plan.storages[pj];
            if (ordered(pj, si) || ordered(si, pj)) continue;
            busy.push_back({o.offset, o.offset + align256(o.bytes)});
        }
        std::sort(busy.begin(), busy.end());
        size_t off = 0;
        for (auto& bz : busy) {
            if (off + need <= bz.first) break;
            off = std::max(off, bz.second);
        }
        st.offset = off;
        arena = std::max(arena, off + need);
        placed.push_back(si);
    }
    plan.arena_bytes = arena;
    for (auto& w : ws_storage) plan.ops[w.first].ws_off = plan.storages[w.second].offset;
}

}  // namespace

bool finalize_plan(Plan& plan, const PassInputs& e, std::string* err) {
    resolve_view_geometry(plan);
    fold_upsample(plan, e);
    assign_int8_served(plan, e);
    assign_storages(plan);
    if (!select_conv_kernels(plan, e, err) || !configure_plugins(plan, err)) return false;
    chain_sppf_pools(plan, e);
    chain_spp_parallel_pools(plan, e);
    group_convs(plan, e);
    mark_sibling_pair(plan, e);
    mark_stem_pair(plan, e);
    mark_bneck_pair(plan, e);
    const std::vector<std::vector<int>> deps = op_dependencies(plan);   // (group_convs reordered and merged ops: not its list)
    assign_lanes(plan, e, deps);
    // a bottleneck pair is one launch on one stream, issued at its second op: not where the two sit on different lanes, nor where another lane waits for
    // the first op alone (its event would fire before the launch that reads its input)
    for (size_t k = 1; k < plan.ops.size(); ++k)
        if (plan.ops[k].bneck_pair && (plan.ops[k].lane != plan.ops[k - 1].lane || plan.ops[k - 1].signal)) plan.ops[k].bneck_pair = false;
    for (size_t k = 1; k < plan.ops.size(); ++k)   // ... and the same rule for the two groups of a sibling pair
        if (plan.ops[k].sibling_pair && (plan.ops[k].lane != plan.ops[k - 1].lane || plan.ops[k - 1].signal)) plan.ops[k].sibling_pair = false;
    plan_arena(plan, ancestors(plan, deps, true));
    return true;
}

}  // namespace trtx
