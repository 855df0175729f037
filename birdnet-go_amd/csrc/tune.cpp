// Create time, after the plan is bound to a device: which activations are stored as bf16 (mark_bf16_storage), where a plan's
// tuning comes from (tune_or_load), the tuning text format and its validator, and the four tuners that time the candidates.
#include "engine.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <sstream>

namespace bnhip {

// ================================================================================================ one definition per fact
// The geometry the fused kernel's shape helpers are asked about, exactly as launch_expand_dw builds it from its arguments: a layer
// whose phase 1 runs on the bf16 pipe has no eight-wave shapes (skw = 0).  An S_DW step (the LDS-staged form) has the plain geometry.
bool Engine::expdw_pipe16(const Step& s) const {
    return s.kind == S_EXPAND_DW && expdw_sk_pipe16(s.C, s.act, s.mode == 1, precision, s.bx && s.wbx != nullptr && bf16x3);
}
ExpDwGeo Engine::expdw_geo(const Step& s) const {
    const bool fused = s.kind == S_EXPAND_DW, stem = fused && s.mode == 1;
    return ExpDwGeo{s.kh, s.sh, s.H, s.W, s.Ho, s.Wo, s.pt, s.pl, stem, (fused && !expdw_pipe16(s)) ? expdw_skw(s.C, s.act, stem) : 0};
}
// the consumers of a step's per-tile sums index them by tile count
void Engine::set_sum_slabs(Step& s, int S) {
    s.S = S;
    for (auto& c : steps) if (&c != &s && c.in0 == s.out2) c.S = S;
}
// no tile that pads the output columns beyond 130 % of their 16-column multiple
static bool pw_padding_ok(int Co, int nt) {
    const long cols = (long)((Co + nt * 16 - 1) / (nt * 16)) * nt * 16;
    return cols * 100 <= (long)((Co + 15) / 16 * 16) * 130;
}

namespace {
// Two clocks on the engine's main stream.  Back to back: how a layer runs inside a step (the next kernel's head fills this one's
// tail); isolated: what it costs when nothing covers its tail.
struct LaunchTimer {
    hipStream_t st;
    hipEvent_t a, b;
    explicit LaunchTimer(hipStream_t s) : st(s) { hipEventCreate(&a); hipEventCreate(&b); }
    ~LaunchTimer() {
        hipStreamSynchronize(st);
        hipEventDestroy(a); hipEventDestroy(b);
        (void)hipGetLastError();
    }
    template <class F> float span(F&& go, int reps) {
        hipEventRecord(a, st);
        for (int r = 0; r < reps; r++) go();
        hipEventRecord(b, st);
        hipEventSynchronize(b);
        float ms = 0; hipEventElapsedTime(&ms, a, b);
        return ms;
    }
    template <class F> float back_to_back(F&& go) { go(); return span(go, 3) / 3; }      // one warm-up, three launches: ms per launch
    template <class F> float isolated(F&& go) {                                           // the best of three single launches
        float best = 1e30f;
        for (int r = 0; r < 3; r++) best = std::min(best, span(go, 1));
        return best;
    }
};

// Two tunings of the pointwise tiles: the batch one lane launches with (+1 % over tuning at max_batch), and max_batch for calls that
// run unsplit; the second is a copy where the two are the same batch.  tune(step index, batch, lane tuning?, nt, wm): the last two
// are that tuning's fields of the step.
template <class F> void tune_lane_then_full(Engine& e, F&& tune) {
    const int n_lane = (e.max_batch + e.n_lanes - 1) / e.n_lanes;
    for (size_t si = 0; si < e.steps.size(); si++) tune(si, n_lane, true, e.steps[si].nt, e.steps[si].wm);
    for (size_t si = 0; si < e.steps.size(); si++) {
        Step& s = e.steps[si];
        if (e.max_batch == n_lane) { s.nt_full = s.nt; s.wm_full = s.wm; }
        else tune(si, e.max_batch, false, s.nt_full, s.wm_full);
    }
}
}  // namespace

// ================================================================================================ where a tuning comes from
// Where a plan's tuning comes from, in this order (round 6: "one plan per library"):
//   1. BNHIP_TUNE_FILE          an experiment's own file (tools/profile_round.sh: bench, kernel trace and every PMC pass of one round)
//   2. the process cache        an engine of the same plan (model geometry, batch, depth, precision, switches, architecture) was
//                               already tuned in this process - the other shards of a multi-device handle, a second handle on the same
//                               model: they adopt its decisions, so a clip's bits do not depend on which engine it lands on
//   3. "tune_dir" / BNHIP_TUNE_DIR   a directory of recorded tunings named by that key (birdnet-go_amd/tune/ holds the ones the
//                               committed PMC passes ran on): the counters under profiles/ then describe the plan that is timed
//   4. the four create-time tuners (timing races: no two runs agree on every tile); recorded into 1 / 3 on request
// Switches that change what the tuners may pick (BNHIP_EXPDW_FORCE, BNHIP_DW_LDS, BNHIP_NO_DW_LDS, BNHIP_TUNE_BY_TIME) bypass 2 and 3;
// BNHIP_TUNE_CACHE=0 bypasses 2 only.
namespace {
std::mutex g_tune_mu;
std::map<std::string, std::string> g_tune_cache;
bool tune_experiment_env() {
    for (const char* n : {"BNHIP_EXPDW_FORCE", "BNHIP_DW_LDS", "BNHIP_NO_DW_LDS", "BNHIP_TUNE_BY_TIME"}) if (getenv(n)) return true;
    return false;
}
bool tune_cache_off() {                                     // BNHIP_TUNE_CACHE=0: tests of the directory path, A/B runs of the tuners themselves
    const char* e = getenv("BNHIP_TUNE_CACHE");
    return e && atoi(e) == 0;
}
bool read_text_file(const std::string& path, std::string* out) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return false;
    char buf[4096]; size_t n;
    out->clear();
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) { out->append(buf, n); if (out->size() > (1u << 22)) break; }
    fclose(f);
    return true;
}
}  // namespace

void Engine::tune_or_load() {
    const char* tf = getenv("BNHIP_TUNE_FILE");
    const bool experiment = tune_experiment_env();
    const std::string key = tune_key();
    std::string text;
    auto adopted = [&](const std::string& src) {
        tune_source = src;
        if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tuning %s: %s\n", key.c_str(), src.c_str());
    };
    if (tf && *tf && read_text_file(tf, &text) && apply_tuning_text(text)) { adopted(std::string("file:") + tf); }
    else {
        bool done = false;
        if (!experiment) {
            if (!tune_cache_off()) {
                std::lock_guard<std::mutex> lk(g_tune_mu);
                auto it = g_tune_cache.find(key);
                if (it != g_tune_cache.end()) text = it->second; else text.clear();
            }
            else text.clear();
            if (!text.empty() && apply_tuning_text(text)) { adopted("process-cache"); done = true; }
            if (!done && !tune_dir.empty() && read_text_file(tune_dir + "/" + key + ".tune", &text) && apply_tuning_text(text)) {
                adopted("dir:" + key + ".tune"); done = true;
            }
        }
        if (!done) {
            autotune_pw(); autotune_expdw(); autotune_dw(); autotune_tail();
            adopted("self-tuned");
            if (!experiment && !tune_dir.empty() && getenv("BNHIP_TUNE_RECORD")) {
                const std::string path = tune_dir + "/" + key + ".tune";
                FILE* ex = fopen(path.c_str(), "r");
                if (ex) fclose(ex); else save_tuning(path.c_str());
            }
        }
    }
    // BNHIP_TUNE_FILE records whatever this engine ended up with (timed here, or adopted from the cache / the directory) when the
    // file does not exist yet; never overwritten: another engine of the process may own it
    if (tf && *tf && tune_source.rfind("file:", 0) != 0) { FILE* ex = fopen(tf, "r"); if (ex) fclose(ex); else save_tuning(tf); }
    if (!experiment && !tune_cache_off()) {
        std::lock_guard<std::mutex> lk(g_tune_mu);
        g_tune_cache.emplace(key, tuning_text());          // (first writer wins: every later engine of this plan adopts it)
    }
}

// ================================================================================================ the tuning as text
// One line per step: what the four create-time tuners decide (tile shapes, kernel flavour, LDS-staged depthwise, slab counts).
static const char* kTuneMagic = "bnhip-tuning-2";
// what a tuning was made FOR, beyond the step names: every step's geometry, the clip length and the device architecture
// (the header of version 1 carried none of them), the device's CU count (the fill rules depend on it)
static unsigned long long tune_plan_hash(const Engine& e) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](long long v) { for (int b = 0; b < 8; b++) { h ^= (unsigned long long)(v >> (8 * b)) & 0xff; h *= 1099511628211ull; } };
    mix(e.n_samples); mix(e.n_classes);
    for (const Step& s : e.steps) { mix((int)s.kind); mix(s.H); mix(s.W); mix(s.C); mix(s.Co); mix(s.Ho); mix(s.Wo); mix(s.kh); mix(s.kw); mix(s.sh); mix(s.sw); mix(s.act); }
    hipDeviceProp_t pr{};
    if (e.device >= 0 && hipGetDeviceProperties(&pr, e.device) == hipSuccess) {
        for (const char* c = pr.gcnArchName; *c && *c != ':'; c++) mix(*c);
        mix(pr.multiProcessorCount);
    } else (void)hipGetLastError();
    return h;
}
// file name / cache key of a plan's tuning: everything the header line checks
std::string Engine::tune_key() const {
    char b[160];
    snprintf(b, sizeof b, "%016llx_b%d_d%d_h%d_p%d_x%d_l%d_s%x", tune_plan_hash(*this), max_batch, depth, host_depth, precision, bf16x3, n_lanes, (unsigned)pw_sw);
    return b;
}
std::string Engine::tuning_text() const {
    std::ostringstream os;
    char b[1024];
    snprintf(b, sizeof b, "%s %zu %d %d %d %d %d %llx\n", kTuneMagic, steps.size(), max_batch, depth, host_depth, precision, bf16x3, tune_plan_hash(*this));
    os << b;
    for (size_t i = 0; i < steps.size(); i++) {
        const Step& s = steps[i];
        snprintf(b, sizeof b, "%zu %d %d %d %d %d %d %d %d %d ", i, (int)s.kind, s.nt, s.wm, s.nt_full, s.wm_full, s.shape, s.dwl, s.bx, s.S);
        os << b << s.name << "\n";
    }
    return os.str();
}
bool Engine::save_tuning(const char* path) const {
    FILE* f = fopen(path, "w");
    if (!f) return false;
    const std::string t = tuning_text();
    fwrite(t.data(), 1, t.size(), f);
    fclose(f);
    return true;
}
bool Engine::load_tuning(const char* path) {
    std::string text;
    if (!read_text_file(path, &text) || !apply_tuning_text(text)) return false;
    if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tuning read from %s\n", path);
    return true;
}
bool Engine::apply_tuning_text(const std::string& text) {
    FILE* f = fmemopen(const_cast<char*>(text.data()), text.size(), "r");
    if (!f) return false;
    char magic[32] = {0}; size_t n = 0; int mb = 0, dp = 0, hd = 0, pr = 0, bx = 0; unsigned long long ph = 0;
    bool ok = fscanf(f, "%31s %zu %d %d %d %d %d %llx", magic, &n, &mb, &dp, &hd, &pr, &bx, &ph) == 8 && !strcmp(magic, kTuneMagic) && n == steps.size() &&
              mb == max_batch && dp == depth && hd == host_depth && pr == precision && bx == bf16x3 && ph == tune_plan_hash(*this);
    struct Row { int kind, nt, wm, ntf, wmf, shape, dwl, bx, S; };
    std::vector<Row> rows(ok ? n : 0);
    for (size_t i = 0; ok && i < n; i++) {
        size_t idx = 0; Row& r = rows[i]; char name[512] = {0};
        const Step& t = steps[i];
        ok = fscanf(f, "%zu %d %d %d %d %d %d %d %d %d %511[^\n]", &idx, &r.kind, &r.nt, &r.wm, &r.ntf, &r.wmf, &r.shape, &r.dwl, &r.bx, &r.S, name) == 11 &&
             idx == i && r.kind == (int)t.kind && t.name == name;
        if (ok && t.kind == S_PW) {                           // the fused tails (wm 13 .. 15) only where the plan marked the step and the tile holds whole clips
            auto tail_row = [&](int nt, int wm) {
                return wm < 13 || (t.tail && (nt == 4 || nt == 6 || nt == 8) && pw_tail_rows(wm) % (t.H * t.W) == 0);
            };
            ok = tail_row(r.nt, r.wm) && tail_row(r.ntf, r.wmf);
        }
        if (ok && t.kind == S_PW) ok = r.nt >= 0 && r.nt <= 8 && r.ntf >= 0 && r.ntf <= 8 && r.wm >= 0 && r.wm <= 15 && r.wmf >= 0 && r.wmf <= 15 &&
                                       (((r.wm >= 5) == (t.wm >= 5) && (r.wmf >= 5) == (t.wm_full >= 5)) || !t.wbx);       // (never switches the arithmetic family: bf16 storage was decided from it)
        if (ok && t.kind == S_DW) {                           // the staged form only where its tuner would have timed it
            const DwParams dp = dw_params(t);
            ok = r.dwl == 0 || (r.dwl == 1 && dwconv_lds_supported(dp) && (t.out2 < 0 || dwconv_sum_slabs(dp) > 0));
        }
        if (ok && (t.kind == S_EXPAND_DW || (t.kind == S_DW && r.dwl)))
            ok = r.shape >= 0 && r.shape < expdw_num_shapes() && expdw_shape_fits(r.shape, expdw_geo(t)) &&
                 (t.kind != S_EXPAND_DW || r.bx == t.bx);                          // (never switches the arithmetic)
    }
    fclose(f);
    // (a fused depthwise tail writes the register-tiled kernel's sums: its depthwise step keeps that form for the calls that run unfused)
    for (size_t i = 0; ok && i + 1 < n; i++)
        if (steps[i].kind == S_PW && steps[i].tail == 2 && (rows[i].wm >= 13 || rows[i].wmf >= 13)) ok = rows[i + 1].dwl == 0;
    if (!ok) return false;
    // A row changes what the tuners decide and nothing else; what follows from a decision (the tile count the consumers of the
    // per-tile sums index by) is recomputed from the plan, not read: a stale or edited file can pick a slower kernel, not a wrong one.
    for (size_t i = 0; i < n; i++) {
        Step& s = steps[i]; const Row& r = rows[i];
        if (s.kind == S_PW) { s.nt = r.nt; s.wm = r.wm; s.nt_full = r.ntf; s.wm_full = r.wmf; }
        const bool staged = s.kind == S_DW && r.dwl;
        if (s.kind == S_DW) s.dwl = r.dwl;
        if (s.kind != S_EXPAND_DW && !staged) continue;
        s.shape = r.shape;
        if (s.out2 >= 0) set_sum_slabs(s, expdw_shape_slabs(s.shape, expdw_geo(s)));
    }
    return true;
}

// ================================================================================================ bf16 activation storage
// bf16 activation storage ("precision":"bf16" only; BNHIP_BF16_ACT=0 keeps fp32 storage for A/B runs).  A value is kept as
// bf16 in HBM when its one producer can round on the way out and every consumer can widen on the way in: the outputs of the
// split-bf16 GEMMs (no residual), of the tiled / LDS-staged depthwise kernels and of the fused expand + depthwise kernel,
// consumed only as the A operand of split-bf16 GEMMs (which round that operand to bf16 anyway - storing it rounded changes
// nothing for them, except that a fused squeeze-excite scale is applied to the rounded value) or as the input of a tiled /
// LDS-staged depthwise convolution (fp32 taps on bf16-rounded inputs: the only place the rounding is new).  That is exactly
// the set of 6x-expanded tensors, the ones the HBM-bound layers of an MBConv stack move.  Graph inputs / outputs, residual
// and scale operands, squeeze-excite sums and everything touched by any other kernel stay fp32.  Arena offsets are
// unchanged (a bf16 value uses the first half of its block).
void Engine::mark_bf16_storage() {
    for (auto& v : vals) v.half = false;
    if (precision != 1 || device < 0) return;
    if (const char* e = getenv("BNHIP_BF16_ACT")) if (atoi(e) == 0) return;
    auto bx_pw = [&](const Step& s) { return s.kind == S_PW && s.bx && s.wbx && s.wm >= 5 && s.wm_full >= 5; };
    // bf16 residual stream (BNHIP_BF16_RESID=0: block outputs stay fp32): the narrow tensors between the blocks - projection
    // outputs, read by the next expand, by the next projection's residual add and, in ratio-1 blocks, by a depthwise kernel -
    // are what the HBM-bound early projections of a bf16 engine mostly move
    bool resid = true;
    if (const char* e = getenv("BNHIP_BF16_RESID")) resid = atoi(e) != 0;
    auto dw_ok = [&](const Step& s) { return s.kind == S_DW && !(s.C & 3) && dwconv_sum_slabs(dw_params(s)) > 0; };
    for (size_t vi = 0; vi < vals.size(); vi++) {
        Value& v = vals[vi];
        const int id = (int)vi;
        if (v.external || id == v_input || id == v_logits || id == v_emb) continue;
        int producers = 0, consumers = 0;
        bool ok = true;
        for (const Step& s : steps) {
            if (s.out == id) {
                producers++;
                bool stem_ok = false;
                if (s.kind == S_CONV_DIRECT && !s.w2) {        // the direct stem (not the MFMA one): 4-pixel kernels only
                    ConvParams cp{nullptr, nullptr, nullptr, nullptr, 1, s.H, s.W, s.C, s.Ho, s.Wo, s.Co, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.act};
                    stem_ok = conv_direct_bf16_ok(cp);
                }
                // (a projection that adds a residual may write bf16 too - the bf16 residual stream, `resid` below)
                const bool p_ok = (bx_pw(s) && (s.Co & 3) == 0 && (s.in2 < 0 || resid)) || dw_ok(s) || (s.kind == S_EXPAND_DW && (s.Co & 3) == 0) || stem_ok;
                if (!p_ok) ok = false;
            }
            if (s.out2 == id) ok = false;
            if (s.in1 == id) ok = false;
            if (s.in2 == id) {                                  // residual operand of a projection: its epilogue can widen bf16
                consumers++;
                if (!(resid && bx_pw(s) && (s.Co & 3) == 0)) ok = false;
            }
            if (s.in0 == id) {
                consumers++;
                // (the GEMM fetches 8 channels per load; the fused kernel takes bf16 input in its bf16-pipe chunk-loop form only)
                const bool c_ok = (bx_pw(s) && (s.C & 7) == 0) || dw_ok(s) || (resid && s.mode != 1 && expdw_pipe16(s));
                if (!c_ok) ok = false;
            }
        }
        if (ok && producers == 1 && consumers >= 1) v.half = true;
    }
    // accounting: the algorithmic bytes of the steps that touch a bf16 value shrink with it
    for (Step& s : steps) {
        if (s.in0 >= 0 && vals[s.in0].half) s.bytes -= 2.0 * (double)vals[s.in0].elems;
        if (s.kind == S_PW && s.in2 >= 0 && vals[s.in2].half) s.bytes -= 2.0 * (double)vals[s.in2].elems;
        if (s.out >= 0 && vals[s.out].half) s.bytes -= 2.0 * (double)vals[s.out].elems;
    }
}

// ================================================================================================ the four tuners
// Tile shape of every fused expand+depthwise layer: time each shape of the kernel's table that fits the layer (the
// pixel-count cost model picks wrongly when a shape's LDS/register footprint costs more than its smaller halo saves -
// also for a pipelined engine: choosing by fewest expanded pixels there measured -1.5 %, unlike k_pw_gemm's tiles).
void Engine::autotune_expdw() {
    LaunchTimer timer(stream);
    const int n = (max_batch + n_lanes - 1) / n_lanes;
    for (size_t si = 0; si < steps.size(); si++) {
        Step& s = steps[si];
        if (s.kind != S_EXPAND_DW) continue;
        float* in0 = vptr(s.in0, d_stage_in, d_stage_logits, nullptr);
        float* out = vptr(s.out, d_stage_in, d_stage_logits, nullptr);
        float* out2 = vptr(s.out2, d_stage_in, d_stage_logits, nullptr);
        float best = 1e30f; int best_idx = -1;
        const bool can_bx = s.wbx != nullptr && s.mode != 1 && bf16x3;
        const int bx = (can_bx && s.bx) ? 1 : 0;            // arithmetic is the planner's decision (shape rule); only the tile is timed
        const ExpDwGeo g = expdw_geo(s);
        // Two clocks per candidate: three launches back to back (how the layer runs inside a step: the next kernel's head
        // fills this one's tail) and the best of three isolated launches (what it costs when nothing covers its tail).  The
        // back-to-back time decides; the isolated one breaks near-ties (within 8 %), because a shape with few, long blocks can
        // look 7 % better back to back and be 60 % worse alone (b3 of the v2.4 stack: 8x32 tiles 201 vs 215 us back to back,
        // 329 vs 198 us isolated) while the pipelined throughput cannot tell the two apart.
        struct Cand { int idx; float b2b, iso; };
        std::vector<Cand> cands;
        for (int idx = 0; idx < expdw_num_shapes(); idx++) {
            if (!expdw_shape_fits(idx, g)) continue;
            auto go = [&]() {
                StemGeom sg{s.H2, s.W2, s.pt2, s.pl2};
                launch_expand_dw(in0, s.w0, s.w1, s.w2, s.w3, out, out2, n, s.H, s.W, s.C, s.Co, s.Ho, s.Wo, s.kh, s.sh, s.pt, s.pl,
                                 s.act, s.act2, idx, s.mode == 1 ? &sg : nullptr, stream, bx ? s.wbx : nullptr, precision,
                                 vals[s.out].half ? 1 : 0, vals[s.in0].half ? 1 : 0);          // the storage flavour the calls will run
            };
            const float b2b = timer.back_to_back(go), iso = timer.isolated(go);
            if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %-16s expand_dw shape=%d bx=%d: %.1f us back to back, %.1f us isolated\n", s.name.c_str(), idx, bx, b2b * 1e3, iso * 1e3);
            cands.push_back({idx, b2b, iso});
            if (b2b < best * 0.98f) { best = b2b; best_idx = idx; }
        }
        if (best_idx < 0) continue;
        float best_iso = 0.f;
        for (const Cand& c : cands) if (c.idx == best_idx) best_iso = c.iso;
        for (const Cand& c : cands)
            if (c.b2b <= best * 1.08f && c.iso < best_iso * 0.8f) { best_idx = c.idx; best_iso = c.iso; }
        if (const char* f = getenv("BNHIP_EXPDW_FORCE")) {          // debug / A-B: "b3/expand+dw=0,b2/expand+dw=10"
            const std::string key = s.name + "=";
            const char* q = strstr(f, key.c_str());
            if (q) { const int idx = atoi(q + key.size()); if (expdw_shape_fits(idx, g)) best_idx = idx; }
        }
        s.shape = best_idx;
        s.bx = bx;
        if (s.out2 >= 0) set_sum_slabs(s, expdw_shape_slabs(best_idx, g));
    }
}

// Plain depthwise layers: the register-tiled kernel reads its taps through L1/L2, the LDS-staged form (the fused kernel's
// second phase on a copied footprint) pays a staging pass instead; which one wins depends on the filter size, the channel
// count and the image shape, so both are timed per layer - with every tile shape / orientation of the staged form.
void Engine::autotune_dw() {
    if (getenv("BNHIP_NO_DW_LDS")) return;
    LaunchTimer timer(stream);
    const int n = (max_batch + n_lanes - 1) / n_lanes;
    for (size_t si = 0; si < steps.size(); si++) {
        Step& s = steps[si];
        if (s.kind != S_DW) continue;
        float* out2 = vptr(s.out2, d_stage_in, d_stage_logits, nullptr);
        const DwParams p = dw_params(s, vptr(s.in0, d_stage_in, d_stage_logits, nullptr), vptr(s.out, d_stage_in, d_stage_logits, nullptr), n);
        if (!dwconv_lds_supported(p)) continue;
        if (s.out2 >= 0 && dwconv_sum_slabs(p) == 0) continue;      // (sums planned for the tiled kernel only)
        const ExpDwGeo g = expdw_geo(s);
        float best = timer.back_to_back([&]() { launch_dwconv(p, out2, stream); });
        if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %-16s dwconv register-tiled: %.1f us\n", s.name.c_str(), best * 1e3);
        if (getenv("BNHIP_DW_LDS")) best = 1e30f;                   // tests: the staged form wherever it exists
        int best_idx = -1;
        for (int idx = 0; idx < expdw_num_shapes(); idx++) {
            if (!expdw_shape_fits(idx, g)) continue;
            const float ms = timer.back_to_back([&]() { launch_dwconv_lds(p, out2, idx, stream); });
            if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %-16s dwconv LDS shape=%d: %.1f us\n", s.name.c_str(), idx, ms * 1e3);
            if (ms < best * 0.97f) { best = ms; best_idx = idx; }
        }
        if (best_idx < 0) continue;
        s.dwl = 1; s.shape = best_idx;
        if (s.out2 >= 0) set_sum_slabs(s, expdw_shape_slabs(best_idx, g));
    }
}

// Per-layer choice of the pw_gemm N-tile width: the best width depends on (M, N, K) through occupancy, grid size and
// padding in ways no closed-form rule captured (late layers at batch 256 have as few as 288 blocks), so each
// pointwise/FC step is timed once at create time on its real shapes and buffers (contents are irrelevant to timing).
void Engine::autotune_pw() {
    LaunchTimer timer(stream);
    tune_lane_then_full(*this, [&](size_t si, int n, bool lane, int& nt_out, int& wm_out) {
        const Step& s = steps[si];
        if (s.kind != S_PW || (s.C & 3)) return;
        float* in0 = vptr(s.in0, d_stage_in, d_stage_logits, nullptr);
        float* in1 = vptr(s.in1, d_stage_in, d_stage_logits, nullptr);
        float* in2 = vptr(s.in2, d_stage_in, d_stage_logits, nullptr);
        float* out = vptr(s.out, d_stage_in, d_stage_logits, nullptr);
        float best = 1e30f; int best_nt = 0, best_wm = 0;
        double best_work = 1e300;
        // wm 2, 1: k_pw_gemm with 128- / 64-row tiles; 4, 3: the same tiles on the software-pipelined k_pw_pipe.
        // Selection: a serial engine takes the fastest candidate.  A pipelined one (depth > 1) is issue-bound - the other
        // context fills every stall - so there the candidate with the least padded MFMA work wins and time only breaks
        // ties: N = 80 / 112 take exact 80- / 112-column tiles although 48- / 64-column ones are 10-45 % faster alone
        // (measured: +1.2 % on the pipelined bench).
        // The full-batch tuning is what a context runs, and the host-pointer pipeline (host_depth > 1) runs its chunks on
        // contexts too; the lane tuning serves serial calls of a depth-1 engine and stays by time.
        const bool by_work = (depth > 1 || (!lane && host_depth > 1)) && !getenv("BNHIP_TUNE_BY_TIME");
        const bool arith_bx = s.bx && s.wbx && bf16x3;        // the planner's shape rule: which kernel family computes this layer
        const double flops = 2.0 * n * s.H * s.W * s.Co * s.C;
        for (int wm = arith_bx ? 0 : 4; wm >= 1; wm--) {
            for (int nt = 1; nt <= 8; nt++) {
                const long M_ = (long)n * s.H * s.W, bm = (wm == 1 || wm == 3) ? 64 : 128;
                if (!pw_padding_ok(s.Co, nt)) continue;                                 // skip absurd padding
                if (wm > 2 && !pw_pipe_ok(nt, wm - 2, s.C)) continue;
                if (nt > 4 && !by_work) continue;                                       // wide tiles never win alone (2 waves/SIMD)
                const double work = (double)((M_ + bm - 1) / bm * bm) * (double)((s.Co + nt * 16 - 1) / (nt * 16) * nt * 16);
                if (by_work && work > best_work * 1.01) continue;                       // cannot win: skip the timing
                // (not pw_params: k_pw_gemm's epilogue reads the storage flags, and these candidates are timed with fp32 storage)
                const PwParams p{in0, s.w0, s.w1, in1, in2, out, n * s.H * s.W, s.Co, s.C, s.H * s.W, s.act, nt, wm};
                const float ms = timer.back_to_back([&]() { launch_pw_gemm(p, stream); });
                if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %-16s n=%d M=%d N=%d K=%d nt=%d wm=%d: %.1f us (%.1f TF)\n", s.name.c_str(), n, p.M, s.Co, s.C, nt, wm, ms * 1e3, flops / (ms * 1e-3) / 1e12);
                const bool less_work = by_work && work < best_work * 0.99;
                if (less_work || ms < best * 0.98f) { best = ms; best_nt = nt; best_wm = wm; best_work = std::min(best_work, work); }
            }
        }
        if (arith_bx) {
            // split-bf16 candidates (wm 5 / 6 = 64- / 128-row tiles, 7 / 8 the software-pipelined form): the fastest tile
            float bbest = 1e30f;
            best_nt = 0; best_wm = 6;
            for (int wm = 12; wm >= 5; wm--)
                for (int nt = 1; nt <= 8; nt++) {
                    if (wm == 11 && precision != 1) continue;
                    if (wm != 12 && !pw_padding_ok(s.Co, nt)) continue;
                    if (wm >= 7 && wm <= 8 && !pw_bx3p_ok(nt, wm - 6, s.C)) continue;
                    if ((wm == 9 || wm == 10) && !pw_b16_ok(precision, s.C, pw_sw)) continue;
                    if (wm == 10 && precision != 0) continue;              // (64-row tiles of k_pw_b16: six-product form only)
                    PwParams p = pw_params(s, n, lane);                    // the flavour the calls will run
                    p.A = in0; p.ascale = in1; p.res = in2; p.out = out; p.nt = nt; p.wm = wm;
                    if (wm == 11) {                                        // weights-stationary form: no tile to choose
                        if (nt != 1 || !pw_b16s_ok(p)) continue;
                    }
                    if (wm == 12) {                                        // weight columns in LDS: 64-, 96- or 128-column blocks
                        // (round 6, VERDICT r5: only where a call owns the GPU - a serial engine's lane tuning.  In a pipelined
                        // engine a 512-thread block that holds a CU's LDS and registers shuts the other context out for its
                        // duration: its launches stretched 39 -> 113 us in the timed trace for +-0 on the bench.)
                        if (by_work) continue;
                        if ((nt != 4 && nt != 6 && nt != 8) || !pw_ws_ok(p) || !pw_ws_fills(p)) continue;
                        if (precision == 1 && nt != 4) continue;
                    }
                    const float ms = timer.back_to_back([&]() { launch_pw_bx3(p, s.wbx, stream); });
                    if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %-16s n=%d M=%d N=%d K=%d nt=%d wm=%d (bf16x3): %.1f us (%.1f TF fp32-equivalent)\n", s.name.c_str(), n, p.M, s.Co, s.C, nt, wm, ms * 1e3, flops / (ms * 1e-3) / 1e12);
                    if (ms < bbest * 0.98f) { bbest = ms; best_nt = nt; best_wm = wm; }
                }
        }
        nt_out = best_nt; wm_out = best_wm;
    });
}

// The folded projection (find_fold_pair) against the pair of launches it replaces, both back to back at max_batch with the tunings
// the calls will run (the projection's tile, the fused layer's shape): the form is kept only where the one launch is faster than the
// two together.  Not part of the tuning text - the verdict is one bit about two kernels that compute the same bits, timed in
// well under a millisecond, so every engine takes its own whatever its tiles came from.
void Engine::time_fold_proj() {
    fold_faster = true; fold_us[0] = fold_us[1] = 0.f;
    if (fold_pair < 0 || device < 0) return;
    const int n = max_batch;
    if (!fold_taken(fold_pair, n, false)) return;                   // (this batch would run the pair anyway: nothing to time)
    const Step& a = steps[fold_pair]; const Step& b = steps[fold_pair + 1];
    PwParams p = pw_params(a, n, false);
    p.A = vptr(a.in0, d_stage_in, d_stage_logits, nullptr); p.ascale = vptr(a.in1, d_stage_in, d_stage_logits, nullptr);
    p.out = vptr(a.out, d_stage_in, d_stage_logits, nullptr);
    float* out = vptr(b.out, d_stage_in, d_stage_logits, nullptr);
    float* out2 = vptr(b.out2, d_stage_in, d_stage_logits, nullptr);
    const ExpDwProj pj{p.A, a.w0, a.w1, p.ascale, a.C, a.Co};
    auto expdw = [&](const ExpDwProj* proj) {
        launch_expand_dw(p.out, b.w0, b.w1, b.w2, b.w3, out, out2, n, b.H, b.W, b.C, b.Co, b.Ho, b.Wo, b.kh, b.sh, b.pt, b.pl, b.act, b.act2,
                         b.shape, nullptr, stream, nullptr, precision, 0, 0, proj);
    };
    LaunchTimer timer(stream);
    const float pair = timer.back_to_back([&]() { launch_pw_gemm(p, stream); expdw(nullptr); });
    const float fold = timer.back_to_back([&]() { expdw(&pj); });
    fold_us[0] = pair * 1e3f; fold_us[1] = fold * 1e3f;
    fold_faster = fold < pair;
    if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %s + %s: pair %.1f us, one launch %.1f us -> %s\n", a.name.c_str(), b.name.c_str(), pair * 1e3, fold * 1e3, fold_faster ? "folded" : "pair");
}

// Per marked layer and per tuning (a lane's batch, max_batch): every fused candidate - row tiles of 48 / 96 / 192 rows, column
// tiles of 64 / 96 / 128 - against the SUM of the GEMM's tuned tile and the depthwise (or the two mean) launches it would replace.
void Engine::autotune_tail() {
    LaunchTimer timer(stream);
    const bool forced = (pw_sw & PW_SW_TAIL_FORCE) != 0;
    tune_lane_then_full(*this, [&](size_t si, int n, bool lane, int& nt_out, int& wm_out) {
        const Step& s = steps[si];
        if (s.kind != S_PW || !s.tail || !s.wbx) return;
        Step& c = steps[si + 1];
        PwParams p = pw_params(s, n, lane);
        if (p.wm >= 13) { p.wm = 6; p.nt = 0; }                     // (forced at plan time, no tuned tile: the default)
        p.A = vptr(s.in0, d_stage_in, d_stage_logits, nullptr);
        p.out = vptr(s.out, d_stage_in, d_stage_logits, nullptr);
        PwTail t = tail_of(s, c);
        float* mean_out = nullptr;
        DwParams dp = dw_params(c, p.out, nullptr, n);
        if (s.tail == 2) {
            t.out = dp.out = vptr(c.out, d_stage_in, d_stage_logits, nullptr);
            t.partial = vptr(c.out2, d_stage_in, d_stage_logits, nullptr);
        } else mean_out = vptr(steps[si + 2].out, d_stage_in, d_stage_logits, nullptr);
        const float pair = timer.back_to_back([&]() {
            launch_pw_bx3(p, s.wbx, stream);
            if (s.tail == 2) { if (c.dwl) launch_dwconv_lds(dp, t.partial, c.shape, stream); else launch_dwconv(dp, t.partial, stream); }
            else { launch_mean_partial(p.out, vptr(c.out, d_stage_in, d_stage_logits, nullptr), n, c.H * c.W, c.C, c.S, stream);
                   launch_mean_finish(vptr(c.out, d_stage_in, d_stage_logits, nullptr), mean_out, n, c.H * c.W, c.C, c.S, stream); }
        });
        if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %-16s n=%d unfused pair (nt=%d wm=%d): %.1f us\n", s.name.c_str(), n, p.nt, p.wm, pair * 1e3);
        float best = forced ? 1e30f : pair * 0.98f; int best_nt = 0, best_wm = 0;
        PwParams pf = p;
        if (s.tail == 1) pf.out = mean_out;
        for (int wm = 13; wm <= 15; wm++)
            for (int nt = 4; nt <= 8; nt += 2) {
                if (!pw_tail_ok(pf, t, nt, wm) || (!forced && !pw_tail_fills(pf, nt, wm))) continue;
                if (!pw_padding_ok(s.Co, nt) && !(forced && nt == 4)) continue;      // skip absurd padding
                const float ms = timer.back_to_back([&]() { launch_pw_tail(pf, t, s.wbx, nt, wm, stream); });
                if (getenv("BNHIP_DEBUG")) fprintf(stderr, "[bnhip] tune %-16s n=%d fused tail nt=%d wm=%d: %.1f us\n", s.name.c_str(), n, nt, wm, ms * 1e3);
                if (ms < best) { best = ms; best_nt = nt; best_wm = wm; }
            }
        if (!best_wm) return;
        nt_out = best_nt; wm_out = best_wm;
        if (s.tail == 2 && c.dwl) {
            // the fused form writes k_dwconv_t's sums: the calls that run this layer unfused take that kernel too
            c.dwl = 0; c.shape = -1;
            set_sum_slabs(c, dwconv_sum_slabs(dw_params(c)));
        }
    });
}

}  // namespace bnhip
