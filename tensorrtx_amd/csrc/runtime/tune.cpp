// Tactic selection by measurement, the part of TensorRT's builder (IBuilder::buildSerializedNetwork, yolov8/src/model.cpp:327;
// "tactics" in its verbose log) that picks one of several kernels for a layer by timing them on the device.  As in TensorRT the
// timing runs when the plan is BUILT (trtx_build_serialized, when a GPU is present) and the choices are stored in the plan
// (Network::tactics, plan format 4): deserializeCudaEngine only applies them, so one plan file runs the same kernels - and
// returns the same bits - in every process.  A plan built on a machine without a GPU carries no choices and runs the static
// defaults (TRTX_TUNE=1 at deserialize times such a plan there, the round-2 behaviour).  How the timing works:
//
//   * every MFMA convolution of the plan has a small set of exchangeable launch configurations (conv_tactics(): column-tile
//     width, 64- / 128- / 256-row tiles, 32- or 64-wide k-steps, the wave-split-K, the weight-stationary and the 3x3 row-reuse
//     kernel where they apply);
//     they share the layer's packed weights, so nothing is re-packed;
//   * first a few whole-network "palettes" (every layer that can takes the same tile shape) are timed against the static
//     defaults: launches of different kernels back to back are expensive here, and only a whole-network move reaches a
//     configuration where long runs of layers share one kernel; the fastest becomes the baseline;
//   * then the WHOLE plan is run in place (profile mode: one stream, HIP events around every op) once per candidate index, every
//     layer using its candidate of that index: each candidate is timed behind its real producer, with the cache state of the
//     real sequence, instead of alone in a loop (a kernel timed alone keeps its weights in L2 and looks faster than it is -
//     profiles/r02_ws_per_op.txt);
//   * a layer leaves its default only for a candidate that is at least 3 % faster, and only if, with all the winners in place,
//     putting it back on the default does not make it and its neighbours faster together (second look: a kernel switch costs
//     the NEXT launch 7-10 us of cold instruction fetches); the choice is remembered per layer signature for the life of the
//     process, so that two engines built from the same plan run the same kernels;
//   * engines built for SEVERAL CONTEXTS IN FLIGHT (setMaxAuxStreams(0)) get a THIRD LOOK (round 6): the objective itself is measured - three scratch contexts run
//     the whole plan side by side, a third of a step apart, with the winners / only the winners >= 30 % faster alone / the palette alone / the launcher's own
//     choices, and the winners stay unless another set is more than 1 % faster (TRTX_TUNE=2: no third look).  YOLOv8n fp16: +1.3...+2.9 % on the three-context rate;
//     the MFMA-bound networks keep their winners by 4-27 % (profiles/r06_third_look_ab.txt).  What led to it:
//   * TRTX_TUNE_MARGIN=<percent> (round 6) replaces the 3 % for engines built for SEVERAL CONTEXTS IN FLIGHT (setMaxAuxStreams(0)).  Every candidate is timed
//     ALONE on an idle chip, and such an engine is built for the aggregate of three batches sharing it: on YOLOv8n fp16 b32, alternating on one box
//     (profiles/r06_tune_margin_ab.txt), 30 % gave kernels 5 % SLOWER alone (serialized conv time 0.239 vs 0.253 of the HBM roof) and a three-context rate 1.7 %
//     HIGHER (38.7k vs 38.0-38.2k img/s; no timing at all: 37.8-38.5k) - a candidate a few per cent faster alone has bought that with co-residency (a wider tile,
//     a deeper pipeline: more LDS per workgroup) or with work (64-row tiles re-read their weights).  NOT the default: the same 30 % cost the MFMA-bound configurations
//     what their timing had found - Faster R-CNN 503 -> 389 img/s, RetinaFace 1517 -> 1373, the fp32 engine 11.2k -> 10.6k, ResNet-50 -3 %, int8 -2.5 % - where a
//     kernel that is faster alone is faster in company too.  A switch for small-layer fp16 networks, off (3 %) unless set.
//
// Plugins, the fused detect head and RoIAlign are skipped in those runs (they would chew on uninitialised proposals); the
// convolutions do not care what the numbers are.  TRTX_TUNE=0 keeps every layer on its static default.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <map>
#include <mutex>
#include <sstream>

#include "../common.h"
#include "../options.h"
#include "engine.h"

using namespace trtx;

namespace {

constexpr int kMaxTactics = 24;

struct SigKey {
    int v[28];
    bool operator<(const SigKey& o) const { return memcmp(v, o.v, sizeof(v)) < 0; }
};

SigKey signature(const ConvArgs& a, int act_pair) {
    SigKey k{};
    const int f[] = {a.N, a.H, a.W, a.Cin, a.ld_in, a.Ho, a.Wo, a.Cout, a.Cout_pad, a.ld_out, a.residual || a.ld_res ? a.ld_res : -1, a.kh, a.kw,
                     a.stride_h, a.stride_w, a.pad_h, a.pad_w, a.CinK, a.Kpad, a.in_i8, a.out_i8, a.res_i8, a.scalar_out, a.bn, a.bk, act_pair,
                     a.up_C, a.t_rs};   //  a folded-upsample / register-staged layer has its own candidate set: its own decision
    static_assert(sizeof(f) / sizeof(int) <= 28, "signature too long");
    static_assert(sizeof(SigKey) == sizeof(Network::TacticEntry::sig), "plan tactic entries hold a whole signature");
    memcpy(k.v, f, sizeof(f));
    return k;
}

struct Choice {
    ConvTactic t;
    int32_t ns[2];  // measured: chosen, default (-1: unknown)
};
std::mutex g_mu;
std::map<SigKey, Choice> g_choice;  // process-wide: layer signature -> tactic in use (+ what it measured)

// TRTX_TACTIC_CACHE=<file>: the choices outlive the process (TensorRT's ITimingCache, IBuilderConfig::setTimingCache): read once,
// every new choice appended as one line of integers (28 signature words, 6 tactic words).  A layer found there is not timed again.
const char kCacheHeader[] = "TRTX_TACTIC_CACHE 2";
void cache_load_locked() {
    static bool done = false;
    if (done) return;
    done = true;
    const std::string path = read_options().tactic_cache;
    if (path.empty()) return;
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return;
    char head[64] = {0};
    if (!fgets(head, sizeof head, f) || strncmp(head, kCacheHeader, strlen(kCacheHeader)) != 0) {  // another format: ignored
        fclose(f);
        return;
    }
    for (;;) {
        SigKey k{};
        int t[8];
        bool ok = true;
        for (int i = 0; i < 28 && ok; ++i) ok = fscanf(f, "%d", &k.v[i]) == 1;
        for (int i = 0; i < 8 && ok; ++i) ok = fscanf(f, "%d", &t[i]) == 1;
        if (!ok) break;
        if (t[5] != 0) continue;   // the sixth word named the row-reuse kernel, which left the library: such a line matches no candidate
        g_choice[k] = Choice{ConvTactic{t[0], t[1], t[2], t[3], t[4]}, {t[6], t[7]}};
    }
    fclose(f);
}
void cache_append_locked(const SigKey& k, const Choice& c) {
    const std::string path = read_options().tactic_cache;
    if (path.empty()) return;
    FILE* f = fopen(path.c_str(), "a");
    if (!f) return;
    if (ftell(f) == 0) fprintf(f, "%s\n", kCacheHeader);
    for (int i = 0; i < 28; ++i) fprintf(f, "%d ", k.v[i]);
    fprintf(f, "%d %d %d %d %d %d %d %d\n", c.t.bn, c.t.bk, c.t.bm, c.t.wsk, c.t.ws, 0, c.ns[0], c.ns[1]);   // (the sixth word: always 0, kept by the format)
    fclose(f);
}

bool same(const ConvTactic& a, const ConvTactic& b) {
    return a.bn == b.bn && a.bk == b.bk && a.bm == b.bm && a.wsk == b.wsk && a.ws == b.ws;
}

std::string tactic_name(const ConvTactic& t) {
    std::ostringstream o;
    if (t.ws == WS_ON) {
        o << "ws";
    } else {
        o << (t.wsk == WSK_ON ? "wsk" : (t.ws == WS_PATCH ? "patch" : (t.ws == WS_RES3 ? "res3" : (t.ws == WS_RES1 ? "res1" : (t.ws == WS_F32_REGS ? "igemm/regs" : (t.ws == WS_F32_ROLES ? "igemm/roles" : "igemm")))))) << " " << (t.wsk == WSK_ON ? 64 : t.bm) << "x" << t.bn << "x" << t.bk;
    }
    return o.str();
}

}  // namespace

namespace trtx {

int32_t tune_engine(trtx_engine* e, bool time_now) {
    // TRTX_TUNE=0 (read at every build / deserialize) keeps every layer on its static default, whatever the plan carries.  Measured
    // on YOLOv8n b32 (profiles/r02_tactics.txt, same box, alternating runs): one context 1.309-1.310 ms against 1.413-1.421 untuned
    // (conv launches 19.9 against 21.6 us); three contexts in flight 0.936-0.945 against 0.945-0.950 ms.  Timing costs 0.1-2 s.
    const Options opt = read_options();
    const bool off = opt.tune == 0;
    const bool alone_only = opt.tune == 2;   // TRTX_TUNE=2: as unset, without the third look (the A/B switch of profiles/r06_third_look_ab.txt)
    const bool verbose = opt.tune_verbose;
    Plan& plan = e->plan;
    e->tactics.clear();
    // setMaxAuxStreams(0) is how a caller says "I keep several execution contexts in flight": whole batches overlap, the chip is
    // shared, and a kernel that finishes sooner by moving more bytes (narrow or short tiles) slows its neighbours down.  Measured
    // on YOLOv8n b32, 3 contexts: full candidate set 32.1k img/s against 33.6k untuned, although the same choices make a lone
    // context 5.7 % faster (profiles/r02_tactics_*.txt).  Such engines choose among the work-efficient configurations only.
    const bool throughput = e->net && e->net->max_aux_streams == 0;
    // what a candidate has to beat its default by, timed alone, to be taken (round 6: see the comment at the top of this file)
    const int margin_pct = !throughput ? 3 : (read_options().tune_margin >= 0 ? read_options().tune_margin : 3);
    const float keep = 1.0f - 0.01f * (float)std::min(margin_pct, 90);
    struct Item {
        int op;
        SigKey key;
        ConvTactic cand[kMaxTactics];
        int n = 0;
        float best_ms[kMaxTactics];
        int static_idx = 0;   // where the launcher's own choice sits after a palette has taken entry 0
    };
    std::vector<Item> items;
    for (size_t k = 0; k < plan.ops.size(); ++k) {
        POp& op = plan.ops[k];
        if (op.kind != OP_CONV || !op.igemm || op.stem) continue;
        const PTensor& t0 = plan.tensors[op.in[0]];
        ConvArgs a = op.conv;  // as execute_plan fills it at the largest batch
        a.N = (t0.nfix ? t0.nfix : plan.max_batch) * t0.nmul;
        a.M = a.N * a.Ho * a.Wo;
        a.residual = op.in.size() > 1 ? reinterpret_cast<const void*>(1) : nullptr;  // only its presence matters here
        Item it;
        it.op = (int)k;
        it.key = signature(a, a.act1 * 16 + a.act2 + (throughput ? 4096 : 0) + (a.f32 ? 8192 : 0) + (a.k_pinned ? 16384 : 0));   // (a pinned layer has its own candidate set: its own decision)
        // (fp32 engines: the tile shapes of conv_igemm_f32.hip - every one the same bits, the choice is tile balance over the 256 CUs)
        it.n = a.f32 ? conv_tactics_f32(a, it.cand, kMaxTactics) : conv_tactics(a, it.cand, kMaxTactics, throughput);
        if (it.n < 1) continue;
        for (int i = 0; i < kMaxTactics; ++i) it.best_ms[i] = 1e30f;
        items.push_back(it);
    }
    if (off || items.empty()) return TRTX_OK;
    if (!time_now) {
        // deserializeCudaEngine: the plan's own choices, no timing.  A layer the plan says nothing about keeps its default.
        const auto& stored = e->net->tactics;
        for (Item& it : items) {
            int pick = 0;
            int32_t ns[2] = {-1, -1};
            for (const Network::TacticEntry& te : stored) {
                if (memcmp(te.sig, it.key.v, sizeof(te.sig)) != 0 || te.tac[5] != 0) continue;   // (a non-zero sixth word matches no candidate)
                const ConvTactic want{te.tac[0], te.tac[1], te.tac[2], te.tac[3], te.tac[4]};
                for (int i = 0; i < it.n; ++i)
                    if (same(it.cand[i], want)) pick = i;
                ns[0] = te.ns[0];
                ns[1] = te.ns[1];
                break;
            }
            conv_apply_tactic(&plan.ops[it.op].conv, it.cand[pick]);
            trtx_engine::TacticRecord rec;
            rec.op = it.op;
            rec.chosen = tactic_name(it.cand[pick]);
            rec.dflt = tactic_name(it.cand[0]);
            rec.chosen_us = ns[0] >= 0 ? ns[0] * 1e-3f : -1.f;   // what the builder measured (carried by the plan)
            rec.default_us = ns[1] >= 0 ? ns[1] * 1e-3f : -1.f;
            rec.candidates = it.n;
            e->tactics.push_back(rec);
        }
        return TRTX_OK;
    }
    // layers this process has already decided: same kernels as before
    bool all_known = true;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        cache_load_locked();
        for (const Item& it : items)
            if (!g_choice.count(it.key)) all_known = false;
    }
    int passes = 0;
    for (const Item& it : items) passes = std::max(passes, it.n);
    if (!all_known && passes > 1) {
        // a scratch context and scratch bindings at the largest batch
        trtx_context* c = nullptr;
        if (const int32_t st0 = trtx_context_create(e, &c)) {  // e.g. no memory for a second arena: the defaults are a complete engine
            fprintf(stderr, "[trtx_hip] tactic timing skipped (%s): every layer keeps its default kernel\n", trtx_status_string(st0));
            (void)hipGetLastError();
            return TRTX_OK;
        }
        c->tuning = true;
        std::vector<void*> bindings(plan.binding_ptensor.size(), nullptr);
        hipStream_t stream = nullptr;
        int32_t st = TRTX_OK;
        auto cleanup = [&]() {
            if (stream) {
                (void)hipStreamSynchronize(stream);
                (void)hipStreamDestroy(stream);
            }
            for (void* p : bindings)
                if (p) (void)hipFree(p);
            trtx_context_destroy(c);
        };
        for (size_t b = 0; b < bindings.size() && st == TRTX_OK; ++b) {
            const PTensor& t = plan.tensors[plan.binding_ptensor[b]];
            const size_t bytes = std::max<size_t>(plan.storages[t.storage].bytes, (size_t)plan.max_batch * (size_t)std::max<int64_t>(1, t.dims.volume()) * 4) + 256;
            if (hipMalloc(&bindings[b], bytes) != hipSuccess || hipMemset(bindings[b], 0, bytes) != hipSuccess) st = TRTX_ERR_HIP;
        }
        if (st == TRTX_OK && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) st = TRTX_ERR_HIP;
        const int reps = 3;
        // Phase 0, the starting point.  Consecutive launches of DIFFERENT kernels are expensive here (cold instruction fetches:
        // +7-10 us on the launch after a switch, ~25 switches in a YOLOv8n step), and no sequence of single-layer moves gets
        // from the static defaults (widest column tile per layer: 3-4 kernels interleaved) to a configuration where long runs
        // of layers share ONE kernel.  So a few whole-network "palettes" are timed first - every layer that can takes the same
        // tile shape - and the fastest whole step becomes the baseline the per-layer search starts from.
        if (st == TRTX_OK) {
            struct Palette { int bn, bm, bk; };
            // (engines for contexts in flight have no 64-row candidates: only the first two palettes can apply to them)
            static const Palette palettes[] = {{64, 128, 32}, {64, 128, 64}, {64, 64, 32}, {64, 64, 64}, {128, 64, 32}, {32, 128, 32}};
            auto total = [&](float* out) {
                float best = 1e30f;
                for (int r = 0; r <= reps && st == TRTX_OK; ++r) {
                    std::vector<OpTiming> prof;
                    st = execute_plan(c, plan.max_batch, bindings.data(), stream, &prof);
                    if (st != TRTX_OK || r == 0) continue;
                    float sum = 0.f;
                    for (const Item& it : items) sum += prof[it.op].ms;
                    best = std::min(best, sum);
                }
                *out = best;
            };
            float base = 0.f;
            total(&base);
            int best_p = -1;
            float best_t = std::min(0.98f, keep) * base;
            for (int pi = 0; pi < (int)(sizeof(palettes) / sizeof(palettes[0])) && st == TRTX_OK; ++pi) {
                const Palette& P = palettes[pi];
                int hits = 0;
                for (const Item& it : items) {
                    int pick = 0;
                    for (int i = 1; i < it.n; ++i)
                        if (it.cand[i].bn == P.bn && it.cand[i].bm == P.bm && it.cand[i].bk == P.bk && it.cand[i].wsk == WSK_OFF && it.cand[i].ws == WS_OFF) pick = i;
                    hits += pick != 0;
                    conv_apply_tactic(&plan.ops[it.op].conv, it.cand[pick]);
                }
                if (hits < 4) continue;
                float t = 0.f;
                total(&t);
                if (verbose) fprintf(stderr, "[trtx_hip] palette %dx%dx%d on %d layers: %.1f us (static defaults %.1f us)\n", P.bm, P.bn, P.bk, hits, t * 1e3f, base * 1e3f);
                if (st == TRTX_OK && t < best_t) {
                    best_t = t;
                    best_p = pi;
                }
            }
            if (best_p >= 0) {  // the palette's tactic becomes entry 0 (the baseline) of every layer that has it
                const Palette& P = palettes[best_p];
                for (Item& it : items)
                    for (int i = 1; i < it.n; ++i)
                        if (it.cand[i].bn == P.bn && it.cand[i].bm == P.bm && it.cand[i].bk == P.bk && it.cand[i].wsk == WSK_OFF && it.cand[i].ws == WS_OFF)
                        {
                            std::swap(it.cand[0], it.cand[i]);
                            it.static_idx = i;
                        }
            }
        }
        for (int p = 0; p < passes && st == TRTX_OK; ++p) {
            for (const Item& it : items) conv_apply_tactic(&plan.ops[it.op].conv, it.cand[p < it.n ? p : 0]);
            for (int r = 0; r <= reps && st == TRTX_OK; ++r) {  // r == 0: untimed (first launch of a kernel loads its code object)
                std::vector<OpTiming> prof;
                st = execute_plan(c, plan.max_batch, bindings.data(), stream, &prof);
                if (st != TRTX_OK || r == 0) continue;
                for (Item& it : items) {
                    const int ci = p < it.n ? p : 0;
                    it.best_ms[ci] = std::min(it.best_ms[ci], prof[it.op].ms);
                }
            }
        }
        // Second look, with every layer on its winner at once.  A candidate that won while its neighbours ran THEIR candidate of
        // the same index may not win next to the kernels that were finally chosen: the first launch of a kernel after a
        // different one starts with cold instruction fetches (+7-10 us here, paid by whichever layer comes next), so a layer
        // that leaves its default can cost its successor more than it gains.  Greedy repair on the real objective: in plan order,
        // put each moved layer back on its default; keep that if the layer and its neighbours (two before, two after) together
        // got faster.
        if (st == TRTX_OK) {
            std::vector<int> win(items.size(), 0);
            for (size_t x = 0; x < items.size(); ++x) {
                const Item& it = items[x];
                for (int i = 1; i < it.n; ++i)
                    if (it.best_ms[i] < it.best_ms[win[x]] && it.best_ms[i] < keep * it.best_ms[0]) win[x] = i;
                conv_apply_tactic(&plan.ops[it.op].conv, it.cand[win[x]]);
            }
            auto measure = [&](int runs, std::vector<float>* out) {
                out->assign(items.size(), 1e30f);
                for (int r = 0; r < runs && st == TRTX_OK; ++r) {
                    std::vector<OpTiming> prof;
                    st = execute_plan(c, plan.max_batch, bindings.data(), stream, &prof);
                    if (st != TRTX_OK) return;
                    for (size_t x = 0; x < items.size(); ++x) (*out)[x] = std::min((*out)[x], prof[items[x].op].ms);
                }
            };
            std::vector<float> cur, trial;
            measure(reps, &cur);
            auto window = [&](const std::vector<float>& v, size_t x) {
                float sum = 0.f;
                for (size_t y = x >= 2 ? x - 2 : 0; y < items.size() && y <= x + 2; ++y) sum += v[y];
                return sum;
            };
            for (size_t x = 0; x < items.size() && st == TRTX_OK; ++x) {
                if (win[x] == 0) continue;
                conv_apply_tactic(&plan.ops[items[x].op].conv, items[x].cand[0]);
                measure(2, &trial);
                if (st != TRTX_OK) break;
                if (window(trial, x) < 0.985f * window(cur, x)) {
                    win[x] = 0;  // the default is better where it runs
                    cur = trial;
                } else {
                    conv_apply_tactic(&plan.ops[items[x].op].conv, items[x].cand[win[x]]);
                }
            }
            for (size_t x = 0; x < items.size() && st == TRTX_OK; ++x) {
                Item& it = items[x];
                for (int i = 1; i < it.n; ++i)
                    if (i != win[x]) it.best_ms[i] = 1e30f;   // only the surviving winner stays in the race
                if (win[x]) it.best_ms[win[x]] = std::min(cur[x], 0.989f * it.best_ms[0]);  // what it costs where it runs (kept: it paid off in its window)
            }
            // Third look (round 6), engines built for SEVERAL CONTEXTS IN FLIGHT only: everything above timed one kernel at a time on an idle chip, and such an engine
            // is for the aggregate of batches sharing it.  On YOLOv8n fp16 the winners of that timing - kernels 5 % faster alone - LOWER the three-context rate by
            // 1.7-3.7 % (they buy their speed with LDS per workgroup or with re-read weights), while on the MFMA-bound networks the same winners are worth 8-23 % in
            // company too (profiles/r06_tune_margin_ab.txt).  So the objective itself is measured: three scratch contexts run the whole plan side by side with (a) the
            // winners, (b) only the winners that are >= 30 % faster alone, (c) the defaults; the winners stay unless another set is more than 1 % faster.
            if (st == TRTX_OK && throughput && !alone_only) {
                std::vector<int> safe(win), none(win.size(), 0), stat(win.size(), 0);
                bool differ = false, any = false, palette = false;
                for (size_t x = 0; x < items.size(); ++x) {
                    if (win[x] && !(items[x].best_ms[win[x]] < 0.70f * items[x].best_ms[0])) safe[x] = 0;
                    differ = differ || safe[x] != win[x];
                    stat[x] = items[x].static_idx;   // (d) the launcher's own choices: no palette, no winner
                    palette = palette || stat[x] != 0;
                    any = any || win[x] != 0 || stat[x] != 0;
                }
                int stagger_us = 0;
                trtx_context* cx[2] = {nullptr, nullptr};
                hipStream_t sx[2] = {nullptr, nullptr};
                bool ok = any;
                for (int k = 0; k < 2 && ok; ++k) {
                    ok = trtx_context_create(e, &cx[k]) == TRTX_OK && hipStreamCreateWithFlags(&sx[k], hipStreamNonBlocking) == hipSuccess;
                    if (cx[k]) cx[k]->tuning = true;
                }
                if (!ok) {
                    (void)hipGetLastError();
                    if (verbose && any) fprintf(stderr, "[trtx_hip] three contexts in flight: no room for two more scratch contexts - the winners timed alone stay\n");
                    else if (verbose) fprintf(stderr, "[trtx_hip] three contexts in flight: every layer is on its default - nothing to compare\n");
                }
                auto rate = [&](const std::vector<int>& pick) {   // seconds per batch with three contexts in flight (best of three legs of four rounds)
                    for (size_t x = 0; x < items.size(); ++x) conv_apply_tactic(&plan.ops[items[x].op].conv, items[x].cand[pick[x]]);
                    double best = 1e30;
                    for (int leg = 0; leg < 4 && st == TRTX_OK; ++leg) {   // (leg 0: untimed)
                        (void)hipDeviceSynchronize();
                        const auto t0 = std::chrono::steady_clock::now();
                        const int rounds = 6;
                        for (int r = 0; r < rounds && st == TRTX_OK; ++r) {
                            st = execute_plan(c, plan.max_batch, bindings.data(), stream, nullptr);
                            for (int k = 0; k < 2 && st == TRTX_OK; ++k) {
                                // (first round: the three batches start a third of a step apart, as they run in steady state - in lock-step every kernel
                                // would only ever meet its own copies)
                                if (r == 0 && stagger_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(stagger_us));
                                st = execute_plan(cx[k], plan.max_batch, bindings.data(), sx[k], nullptr);
                            }
                        }
                        (void)hipDeviceSynchronize();
                        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (3.0 * rounds);
                        if (leg) best = std::min(best, dt);
                    }
                    return best;
                };
                if (ok) {
                    stagger_us = 0;
                    stagger_us = (int)(rate(win) * 1e6);   // (one batch-time of the winners per context: a third of a three-context step)
                    const double t_win = rate(win);
                    const double t_safe = differ ? rate(safe) : t_win;
                    const double t_none = rate(none);
                    const double t_stat = palette ? rate(stat) : t_none;
                    const std::vector<int>* keep_set = &win;
                    double t_keep = t_win;
                    if (st == TRTX_OK && t_safe < 0.99 * t_keep) { keep_set = &safe; t_keep = t_safe; }
                    if (st == TRTX_OK && t_none < 0.99 * t_win && t_none < t_keep) { keep_set = &none; t_keep = t_none; }
                    if (st == TRTX_OK && t_stat < 0.99 * t_win && t_stat < t_keep) { keep_set = &stat; t_keep = t_stat; }
                    if (verbose)
                        fprintf(stderr, "[trtx_hip] three contexts in flight: %.1f us per batch with the winners timed alone, %.1f with those >= 30 %% faster only, %.1f with the palette alone, %.1f with the launcher's own choices -> %s\n",
                                t_win * 1e6, t_safe * 1e6, t_none * 1e6, t_stat * 1e6,
                                keep_set == &win ? "winners" : keep_set == &safe ? "the large winners only" : keep_set == &none ? "palette" : "the launcher's own choices");
                    if (st == TRTX_OK && keep_set != &win)
                        for (size_t x = 0; x < items.size(); ++x) {
                            Item& it = items[x];
                            const int want = (*keep_set)[x];
                            if (want == win[x]) continue;
                            for (int i = 1; i < it.n; ++i) it.best_ms[i] = 1e30f;
                            if (want) it.best_ms[want] = 0.989f * it.best_ms[0];   // (the launcher's own choice under a palette: it has to win the final comparison - reported at the palette's time)
                        }
                }
                for (int k = 0; k < 2; ++k) {
                    if (sx[k]) {
                        (void)hipStreamSynchronize(sx[k]);
                        (void)hipStreamDestroy(sx[k]);
                    }
                    if (cx[k]) trtx_context_destroy(cx[k]);
                }
            }
        }
        for (const Item& it : items) conv_apply_tactic(&plan.ops[it.op].conv, it.cand[0]);
        cleanup();
        if (st != TRTX_OK) {
            (void)hipGetLastError();
            fprintf(stderr, "[trtx_hip] tactic timing failed (%s): every layer keeps its default kernel\n", trtx_status_string(st));
            return TRTX_OK;  // the defaults are a complete engine
        }
    }
    std::lock_guard<std::mutex> lock(g_mu);
    e->net->tactics.clear();
    e->net->tactics_timed = true;
    for (Item& it : items) {
        auto found = g_choice.find(it.key);
        int pick = 0;
        int32_t ns[2] = {-1, -1};
        if (found != g_choice.end()) {
            for (int i = 0; i < it.n; ++i)
                if (same(it.cand[i], found->second.t)) pick = i;
            ns[0] = found->second.ns[0];
            ns[1] = found->second.ns[1];
        } else {
            for (int i = 1; i < it.n; ++i)
                if (it.best_ms[i] < it.best_ms[pick] && it.best_ms[i] < 0.99f * it.best_ms[0]) pick = i;
            ns[0] = it.best_ms[pick] < 1e29f ? (int32_t)(it.best_ms[pick] * 1e6f) : -1;
            ns[1] = it.best_ms[0] < 1e29f ? (int32_t)(it.best_ms[0] * 1e6f) : -1;
            const Choice c{it.cand[pick], {ns[0], ns[1]}};
            g_choice[it.key] = c;
            cache_append_locked(it.key, c);
        }
        conv_apply_tactic(&plan.ops[it.op].conv, it.cand[pick]);
        {   // what goes into the plan: one entry per distinct layer signature
            Network::TacticEntry te{};
            memcpy(te.sig, it.key.v, sizeof(te.sig));
            const ConvTactic& c = it.cand[pick];
            const int32_t tv[6] = {c.bn, c.bk, c.bm, c.wsk, c.ws, 0};
            memcpy(te.tac, tv, sizeof(tv));
            te.ns[0] = ns[0];
            te.ns[1] = ns[1];
            bool dup = false;
            for (const Network::TacticEntry& o : e->net->tactics) dup = dup || memcmp(o.sig, te.sig, sizeof(te.sig)) == 0;
            if (!dup) e->net->tactics.push_back(te);
        }
        trtx_engine::TacticRecord rec;
        rec.op = it.op;
        rec.chosen = tactic_name(it.cand[pick]);
        rec.dflt = tactic_name(it.cand[0]);
        rec.chosen_us = ns[0] >= 0 ? ns[0] * 1e-3f : -1.f;
        rec.default_us = ns[1] >= 0 ? ns[1] * 1e-3f : -1.f;
        rec.candidates = it.n;
        e->tactics.push_back(rec);
        if (verbose)
            fprintf(stderr, "[trtx_hip] tactic %-40s %-18s %7.1f us (default %-18s %7.1f us, %d candidates)\n", plan.ops[it.op].name.c_str(),
                    rec.chosen.c_str(), rec.chosen_us, rec.dflt.c_str(), rec.default_us, it.n);
    }
    return TRTX_OK;
}

}  // namespace trtx

extern "C" int32_t trtx_engine_tactics(const trtx_engine* e, char** json_out) {
    if (!e || !json_out) return TRTX_ERR_INVALID;
    std::ostringstream o;
    o << "[";
    for (size_t i = 0; i < e->tactics.size(); ++i) {
        const auto& r = e->tactics[i];
        o << (i ? "," : "") << "{\"op\":" << r.op << ",\"name\":\"";
        for (char ch : e->plan.ops[r.op].name) o << ((ch == '"' || ch == '\\' || (unsigned char)ch < 0x20) ? ' ' : ch);
        o << "\",\"tactic\":\"" << r.chosen << "\",\"default\":\"" << r.dflt << "\",\"us\":" << r.chosen_us << ",\"default_us\":" << r.default_us
          << ",\"candidates\":" << r.candidates << "}";
    }
    o << "]";
    *json_out = strdup(o.str().c_str());
    return TRTX_OK;
}
