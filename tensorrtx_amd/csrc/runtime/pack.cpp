#include "pack.h"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "../kernels/kernels.h"
#include "plan.h"

namespace trtx {

uint16_t f32_to_f16_bits(float f) {
    const _Float16 h = (_Float16)f;  // round-to-nearest-even, same as the device conversion
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

float f16_bits_to_f32(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}

void pack_conv_weights_f16(const float* w, int cout, int cin, int kh, int kw, int cin_pad, int bk, const float* ch_scale,
                           uint16_t* packed) {
    const int bn = conv_igemm_pick_bn(cout);
    const int cout_pad = (cout + bn - 1) / bn * bn;
    const int kpad = (kh * kw * cin_pad + bk - 1) / bk * bk;  // cin_pad = per-tap K stride (CinK); rows padded to the k-step
    memset(packed, 0, sizeof(uint16_t) * (size_t)cout_pad * kpad);
    for (int co = 0; co < cout; ++co) {
        const float sc = ch_scale ? ch_scale[co] : 1.0f;
        for (int c = 0; c < cin; ++c)
            for (int r = 0; r < kh; ++r)
                for (int q = 0; q < kw; ++q) {
                    const float v = w[(((size_t)co * cin + c) * kh + r) * kw + q] * sc;
                    packed[(size_t)co * kpad + (size_t)(r * kw + q) * cin_pad + c] = f32_to_f16_bits(v);
                }
    }
}

}  // namespace trtx

// kINT8: per-output-channel symmetric quantisation of the (BN-folded) weights, rows [Cout_pad][Kpad] with k = tap * cink + c
void trtx::conv_pack_weights_i8(const float* w, int cout, int cin, int kh, int kw, int cink, const float* ch_scale, int cout_pad, int kpad,
                                int8_t* packed, float* wscale_out) {
    memset(packed, 0, (size_t)cout_pad * kpad);
    for (int co = 0; co < cout_pad; ++co) wscale_out[co] = 1.0f;
    for (int co = 0; co < cout; ++co) {
        const float sc = ch_scale ? ch_scale[co] : 1.0f;
        float amax = 0.f;
        const size_t n = (size_t)cin * kh * kw;
        for (size_t i = 0; i < n; ++i) {
            const float v = fabsf(w[(size_t)co * n + i] * sc);
            amax = v > amax ? v : amax;
        }
        const float s = amax > 0.f ? amax / 127.0f : 1.0f;
        wscale_out[co] = s;
        for (int c = 0; c < cin; ++c)
            for (int r = 0; r < kh; ++r)
                for (int q = 0; q < kw; ++q) {
                    float t = nearbyintf(w[(((size_t)co * cin + c) * kh + r) * kw + q] * sc / s);
                    t = t > 127.f ? 127.f : (t < -127.f ? -127.f : t);
                    packed[(size_t)co * kpad + (size_t)(r * kw + q) * cink + c] = (int8_t)t;
                }
    }
}

namespace trtx {

void pack_conv_weights_f32(const float* w, int cout, int cin_g, int kh, int kw, const float* ch_scale, float* packed) {
    for (int co = 0; co < cout; ++co) {
        const float sc = ch_scale ? ch_scale[co] : 1.0f;
        for (int c = 0; c < cin_g; ++c)
            for (int r = 0; r < kh; ++r)
                for (int q = 0; q < kw; ++q)
                    packed[(((size_t)co * kh + r) * kw + q) * cin_g + c] =
                            w[(((size_t)co * cin_g + c) * kh + r) * kw + q] * sc;
    }
}

void pack_conv_weights_grouped_f16(const float* w, int cout, int cin_g, int kh, int kw, int kpad, const float* ch_scale, uint16_t* packed) {
    memset(packed, 0, sizeof(uint16_t) * (size_t)cout * kpad);
    for (int co = 0; co < cout; ++co) {   // (KCRS rows are already group-major: channel co belongs to group co / Cout_g)
        const float sc = ch_scale ? ch_scale[co] : 1.0f;
        for (int c = 0; c < cin_g; ++c)
            for (int r = 0; r < kh; ++r)
                for (int q = 0; q < kw; ++q)
                    packed[(size_t)co * kpad + (size_t)(r * kw + q) * cin_g + c] = f32_to_f16_bits(w[(((size_t)co * cin_g + c) * kh + r) * kw + q] * sc);
    }
}

void pack_deconv_weights_f32(const float* w, int cin, int cout, int groups, int kh, int kw, float* packed) {
    const int cin_g = cin / groups, cout_g = cout / groups;
    for (int co = 0; co < cout; ++co) {
        const int g = co / cout_g, col = co % cout_g;
        for (int c = 0; c < cin_g; ++c) {
            const int ci = g * cin_g + c;
            for (int r = 0; r < kh; ++r)
                for (int q = 0; q < kw; ++q)
                    packed[(((size_t)co * kh + r) * kw + q) * cin_g + c] =
                            w[(((size_t)ci * cout_g + col) * kh + r) * kw + q];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// W'[o][c][2 i + dy][2 j + dx] = W[o][q cin + c][i][j], q = 2 dx + dy: the k x k filter over ReOrg's 4 cin channels as the 2kh x 2kw
// stride-2 filter over the cin channels ReOrg read (match_reorg_fold).  Every element of `out` is written once.
void reorg_fold_weights(const float* w, int cout, int cin, int kh, int kw, float* out) {
    for (int o = 0; o < cout; ++o)
        for (int q = 0; q < 4; ++q) {
            const int dy = q & 1, dx = q >> 1;
            for (int c = 0; c < cin; ++c)
                for (int i = 0; i < kh; ++i)
                    for (int j = 0; j < kw; ++j)
                        out[(((size_t)o * cin + c) * 2 * kh + 2 * i + dy) * 2 * kw + 2 * j + dx] =
                                w[(((size_t)o * 4 * cin + (size_t)q * cin + c) * kh + i) * kw + j];
        }
}

// RepVGGDW as one depthwise 7x7 filter: w[c] = scale7[c] * w7[c] with scale3[c] * w3[c] added into its 3x3 centre, shift[c] = (bias7[c] * scale7[c]
// + shift7[c]) + (bias3[c] * scale3[c] + shift3[c]); every value in double, rounded once to fp32 (what the depthwise kernel reads).
void repvggdw_fold_weights(const float* w7, const float* scale7, const float* shift7, const float* bias7, const float* w3, const float* scale3,
                           const float* shift3, const float* bias3, int channels, float* w_out, float* shift_out) {
    for (int c = 0; c < channels; ++c) {
        const double s7 = scale7[c], s3 = scale3[c];
        for (int r = 0; r < 7; ++r)
            for (int q = 0; q < 7; ++q) {
                double v = (double)w7[(size_t)c * 49 + r * 7 + q] * s7;
                if (r >= 2 && r <= 4 && q >= 2 && q <= 4) v += (double)w3[(size_t)c * 9 + (r - 2) * 3 + (q - 2)] * s3;
                w_out[(size_t)c * 49 + r * 7 + q] = (float)v;
            }
        shift_out[c] = (float)(((double)bias7[c] * s7 + (double)shift7[c]) + ((double)bias3[c] * s3 + (double)shift3[c]));
    }
}

bool pack_weights(const Network& net, Plan* plan) {
    std::vector<uint8_t>& blob = plan->weight_blob;
    blob.clear();
    auto reserve = [&](size_t bytes) {
        const size_t off = align256(blob.size());
        blob.resize(off + bytes, 0);
        return off;
    };
    // constants
    for (auto& t : plan->tensors) {
        if (t.storage < 0 || plan->storages[t.storage].kind != ST_WEIGHTS || t.parent >= 0) continue;
        const TensorDef& nt = net.tensors[t.net_tensor];
        const LayerDef& l = net.layers[nt.producer];
        const size_t off = reserve(l.w0.size() * 4);
        memcpy(blob.data() + off, l.w0.data(), l.w0.size() * 4);
        plan->storages[t.storage].offset = off;
    }
    std::vector<POp*> every;   // the members of a conv group are packed like the convolutions they are
    for (auto& op : plan->ops) {
        for (auto& m : op.group) every.push_back(&m);
        every.push_back(&op);
    }
    for (POp* pop : every) {
        POp& op = *pop;
        if (op.kind == OP_CONV || op.kind == OP_DECONV) {
            const LayerDef& l = net.layers[op.src_layer];
            const ConvArgs& a = op.conv;
            const int cout = a.Cout;
            const int cout_real = op.cout_real > 0 ? op.cout_real : cout;   // (output channels rounded up: zero filter rows and biases beyond the layer's own)
            // folded per-channel scale / shift
            std::vector<float> sc(cout, 1.f), bias(std::max(a.Cout_pad, cout), 0.f);
            for (int c = 0; c < cout_real && c < (int)l.w1.size(); ++c) bias[c] = l.w1[c];
            if (op.scale_layer >= 0) {
                const LayerDef& s = net.layers[op.scale_layer];
                for (int c = 0; c < cout_real; ++c) {
                    const float scale = s.w1.empty() ? 1.f : (s.w1.size() == 1 ? s.w1[0] : s.w1[c]);
                    const float shift = s.w0.empty() ? 0.f : (s.w0.size() == 1 ? s.w0[0] : s.w0[c]);
                    sc[c] = scale;
                    bias[c] = bias[c] * scale + shift;
                }
            }
            const TensorDef& tin = net.tensors[l.inputs[0]];
            const int cin_logical = op.reorg_cin > 0 ? op.reorg_cin : (int)tin.dims.d[tin.dims.nb - 3];
            std::vector<float> w0_padded;
            const float* w0 = l.w0.data();
            if (op.reorg_cin > 0) {   // before any packing: every branch below sees an ordinary 2k x 2k filter over the slices' input
                w0_padded.resize(l.w0.size());   // [cout][cin][2kh][2kw]: as many elements as [cout][4 cin][kh][kw]
                reorg_fold_weights(l.w0.data(), l.nb_out, op.reorg_cin, l.kernel[0], l.kernel[1], w0_padded.data());
                w0 = w0_padded.data();
            }
            if (op.fold_layer >= 0) {
                // RepVGGDW (match_repvggdw_fold): one 7x7 filter and one shift for both branches; the scale that every packer below applies is 1
                const LayerDef &l3 = net.layers[op.fold_layer], &s3 = net.layers[op.fold_scale], &s7 = net.layers[op.scale_layer];
                auto per_channel = [&](const std::vector<float>& v, float dflt) {
                    std::vector<float> o(cout, dflt);
                    for (int c = 0; c < cout && !v.empty(); ++c) o[c] = v.size() == 1 ? v[0] : v[c];
                    return o;
                };
                const auto sc7 = per_channel(s7.w1, 1.f), sh7 = per_channel(s7.w0, 0.f), sc3 = per_channel(s3.w1, 1.f), sh3 = per_channel(s3.w0, 0.f);
                const auto b7 = per_channel(l.w1, 0.f), b3 = per_channel(l3.w1, 0.f);
                w0_padded.resize((size_t)cout * 49);
                repvggdw_fold_weights(l.w0.data(), sc7.data(), sh7.data(), b7.data(), l3.w0.data(), sc3.data(), sh3.data(), b3.data(), cout, w0_padded.data(), bias.data());
                std::fill(sc.begin(), sc.end(), 1.f);
                w0 = w0_padded.data();
            }
            if (cout_real < cout) {
                if (w0_padded.empty()) w0_padded = l.w0;
                w0_padded.resize((size_t)cout * a.kh * a.kw * (cin_logical / a.groups), 0.f);
                w0 = w0_padded.data();
            }
            if (op.kind == OP_DECONV) {
                op.w_off = reserve((size_t)cout * a.kh * a.kw * (cin_logical / a.groups) * 4);
                pack_deconv_weights_f32(l.w0.data(), cin_logical, cout, a.groups, a.kh, a.kw,
                                        reinterpret_cast<float*>(blob.data() + op.w_off));
            } else if (op.stem) {
                // [tap = (c*kh + r)*kw + q][cout], BN scale folded
                op.w_off = reserve((size_t)a.kh * a.kw * cin_logical * cout * 4);
                float* dst = reinterpret_cast<float*>(blob.data() + op.w_off);
                for (int co = 0; co < cout; ++co)
                    for (int t = 0; t < cin_logical * a.kh * a.kw; ++t)
                        dst[(size_t)t * cout + co] = w0[(size_t)co * cin_logical * a.kh * a.kw + t] * sc[co];
            } else if (op.from_deconv) {
                // CKRS [Cin][Cout][kh][kw] -> KCRS of the stand-in 1x1 conv: output channel (r*kw + q)*Cout + co.  The re-layout
                // (and the per-sub-position bias) does not depend on which conv kernel runs the stand-in: the kernel choice may refuse
                // the MFMA path (kh*kw*Cin < 32, > 2 GB images) and the direct kernel must then see the same KCRS weights.
                const int taps = l.kernel[0] * l.kernel[1], dc = l.nb_out;
                std::vector<float> w2((size_t)cout * cin_logical);
                for (int ci = 0; ci < cin_logical; ++ci)
                    for (int co = 0; co < dc; ++co)
                        for (int t = 0; t < taps; ++t) w2[(size_t)(t * dc + co) * cin_logical + ci] = l.w0[((size_t)ci * dc + co) * taps + t];
                for (int c = 0; c < cout; ++c) bias[c] = l.w1.empty() ? 0.f : l.w1[c % dc];
                if (op.igemm) {
                    op.w_off = reserve((size_t)a.Cout_pad * a.Kpad * 2);
                    pack_conv_weights_f16(w2.data(), cout, cin_logical, 1, 1, a.CinK, a.bk, sc.data(),
                                          reinterpret_cast<uint16_t*>(blob.data() + op.w_off));
                } else {
                    op.w_off = reserve((size_t)cout * cin_logical * 4);
                    pack_conv_weights_f32(w2.data(), cout, cin_logical, 1, 1, sc.data(), reinterpret_cast<float*>(blob.data() + op.w_off));
                }
            } else if (op.igemm && a.in_i8) {
                // int8 weights, per-output-channel scales; cscale[c] = input tensor scale * weight scale (dequantises the int32 sums)
                const size_t kpad_bytes = (size_t)a.Kpad * 2;
                op.w_off = reserve((size_t)a.Cout_pad * kpad_bytes);
                std::vector<float> wscale(a.Cout_pad, 1.f);
                conv_pack_weights_i8(w0, cout, cin_logical, a.kh, a.kw, a.CinK * 2, sc.data(), a.Cout_pad, (int)kpad_bytes,
                                     reinterpret_cast<int8_t*>(blob.data() + op.w_off), wscale.data());
                const float s_in = plan->tensors[op.in[0]].scale;
                for (float& v : wscale) v *= s_in;
                op.s_off = reserve(wscale.size() * 4);
                memcpy(blob.data() + op.s_off, wscale.data(), wscale.size() * 4);
            } else if (op.igemm && a.f32) {
                op.w_off = reserve((size_t)a.Cout_pad * a.Kpad * 4);
                conv_pack_weights_igemm_f32(w0, cout, cin_logical, a.kh, a.kw, a.CinK, a.Kpad, a.Cout_pad, sc.data(),
                                            reinterpret_cast<float*>(blob.data() + op.w_off));
            } else if (op.igemm) {
                op.w_off = reserve((size_t)a.Cout_pad * a.Kpad * 2);
                pack_conv_weights_f16(w0, cout, cin_logical, a.kh, a.kw, a.CinK, a.bk, sc.data(),
                                      reinterpret_cast<uint16_t*>(blob.data() + op.w_off));
            } else if (op.grouped) {
                op.w_off = reserve((size_t)cout * a.Kpad * 2);
                pack_conv_weights_grouped_f16(w0, cout, cin_logical / a.groups, a.kh, a.kw, a.Kpad, sc.data(), reinterpret_cast<uint16_t*>(blob.data() + op.w_off));
            } else if (op.dw) {
                // [tap][C], BN scale folded: a lane reads its channel vector of one tap as one 16-byte load
                op.w_off = reserve((size_t)a.kh * a.kw * cout * 4);
                float* dst = reinterpret_cast<float*>(blob.data() + op.w_off);
                for (int co = 0; co < cout; ++co)
                    for (int t = 0; t < a.kh * a.kw; ++t) dst[(size_t)t * cout + co] = w0[(size_t)co * a.kh * a.kw + t] * sc[co];
            } else {
                op.w_off = reserve((size_t)cout * a.kh * a.kw * (cin_logical / a.groups) * 4);
                pack_conv_weights_f32(w0, cout, cin_logical / a.groups, a.kh, a.kw, sc.data(),
                                      reinterpret_cast<float*>(blob.data() + op.w_off));
            }
            op.b_off = reserve(bias.size() * 4);
            memcpy(blob.data() + op.b_off, bias.data(), bias.size() * 4);
            op.bytes += (double)(op.igemm ? (size_t)a.Cout_pad * a.Kpad * (a.f32 ? 4 : 2) : (op.grouped ? (size_t)cout * a.Kpad * 2 : (size_t)cout * a.K * 4));
        } else if (head_has_dfl(op.kind)) {
            const LayerDef& l = net.layers[op.src_layer];
            op.w_off = reserve(16 * 4);
            memcpy(blob.data() + op.w_off, l.w0.data(), 16 * 4);
        } else if (op.kind == OP_HGCONV) {
            // nine fp32 arrays in HgconvWeights' order, each as its layer holds it: context_net (weight, bias), the prototype constant,
            // pre_head_proj, edge_proj, node_proj (weight, bias each); a Linear without a bias gets zeros
            const size_t D = (size_t)op.i[1], ED = (size_t)op.i[2] * D;
            const LayerDef &lc = net.layers[op.iv[0]], &lp = net.layers[op.iv[1]];
            std::vector<float> all;
            auto put = [&](const std::vector<float>& v, size_t n) {
                const size_t at = all.size();
                all.resize(at + n, 0.f);
                std::copy(v.begin(), v.begin() + std::min(n, v.size()), all.begin() + at);
            };
            put(lc.w0, ED * 2 * D);
            put(lc.w1, ED);
            put(lp.w0, ED);
            for (int k = 2; k < 5; ++k) {
                put(net.layers[op.iv[k]].w0, D * D);
                put(net.layers[op.iv[k]].w1, D);
            }
            op.w_off = reserve(all.size() * 4);
            memcpy(blob.data() + op.w_off, all.data(), all.size() * 4);
            op.bytes += 4.0 * all.size();
        } else if (op.kind == OP_GATED_ADD) {
            const std::vector<float>& g = net.layers[op.src_layer].w0;   // one value, or one per channel (match_gated_add)
            const int C = plan->tensors[op.in[0]].C;
            op.w_off = reserve((size_t)C * 4);
            float* dst = reinterpret_cast<float*>(blob.data() + op.w_off);
            for (int c = 0; c < C; ++c) dst[c] = g.size() == 1 ? g[0] : g[c];
        } else if (op.kind == OP_SCALE_NHWC || op.kind == OP_SCALE_LIN) {
            const LayerDef& l = net.layers[op.src_layer];
            const int C = op.kind == OP_SCALE_NHWC ? plan->tensors[op.in[0]].C : (op.i[0] == 1 ? op.i[2] : 1);
            auto expand = [&](const std::vector<float>& w, float dflt) {
                std::vector<float> v(C, dflt);
                for (int c = 0; c < C; ++c)
                    if (!w.empty()) v[c] = w.size() == 1 ? w[0] : w[c];
                return v;
            };
            const auto shift = expand(l.w0, 0.f), scale = expand(l.w1, 1.f), power = expand(l.w2, 1.f);
            op.s_off = reserve(C * 4);
            memcpy(blob.data() + op.s_off, scale.data(), C * 4);
            op.b_off = reserve(C * 4);
            memcpy(blob.data() + op.b_off, shift.data(), C * 4);
            op.w_off = reserve(C * 4);
            memcpy(blob.data() + op.w_off, power.data(), C * 4);
        }
    }
    for (auto& op : plan->ops)   // a grouped launch moves what its members move (their packed weights were priced just above)
        if (op.kind == OP_CONV_GROUP) {
            op.bytes = 0;
            for (const POp& m : op.group) op.bytes += m.bytes;
        }
    plan->weight_bytes = align256(blob.size());
    blob.resize(plan->weight_bytes, 0);
    return true;
}

}  // namespace trtx
