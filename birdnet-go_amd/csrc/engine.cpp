#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <sstream>

#include "../../include/bnhip.h"
#include "hostpipe.h"

namespace bnhip {

#define HIPCHK(call)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            *err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            return false;                                                                      \
        }                                                                                      \
    } while (0)

// ================================================================================================ engine
Engine::~Engine() {
    if (device >= 0) hipSetDevice(device);
    drop_graphs();
    for (auto& e : prof) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    for (auto e : ev_pool) hipEventDestroy(e);
    for (auto& p : step_ev) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (mm_scratch) hipFree(mm_scratch);
    if (d_hand) hipFree(d_hand);
    for (void* p : {(void*)act_arena, (void*)w_arena, (void*)d_stage_in, (void*)d_stage_logits, (void*)d_stage_emb,
                    (void*)d_stage_pcm, (void*)d_post_conf, (void*)d_topk_conf, (void*)d_topk_idx})
        if (p) hipFree(p);
    hostpipe_free(hostpipe);
    for (int i = 0; i < kMaxKStreams; i++) if (kstream[i]) hipStreamSynchronize(kstream[i]);
    for (int c = 0; c < kMaxDepth; c++) {
        if (c > 0 && ctx_arena[c]) hipFree(ctx_arena[c]);
        if (ev_ctx_done[c]) hipEventDestroy(ev_ctx_done[c]);
    }
    if (ev_ctx_fork) hipEventDestroy(ev_ctx_fork);
    for (int i = 0; i < kMaxLanes - 1; i++) if (ev_join[i]) hipEventDestroy(ev_join[i]);
    if (ev_fork) hipEventDestroy(ev_fork);
    release_streams();
}

// ================================================================================================ device half of build
// Arenas and staging buffers of a planned engine, the weight upload (unless another engine's copy arrives: defer_weights),
// and every step's w0..w3 / wbx and front-end spec pointed into the weight arena.
bool Engine::bind_device(const WeightPlan& wp, std::string* err, int* code) {
    *code = BNHIP_E_RUNTIME;
    HIPCHK(hipSetDevice(device));
    stream = kernel_stream(0);
    if (!stream) { *err = "hipStreamCreate failed"; return false; }
    if (n_lanes > 1) {
        HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        for (int i = 0; i < n_lanes - 1; i++) {
            lane_stream[i] = kernel_stream(1 + i);
            if (!lane_stream[i]) { *err = "hipStreamCreate failed"; return false; }
            HIPCHK(hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming));
        }
    }
    own_stream = true;
    HIPCHK(hipMalloc((void**)&w_arena, std::max<size_t>(w_bytes, 256)));
    if (!defer_weights) HIPCHK(hipMemcpy(w_arena, wp.img.data(), w_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&act_arena, std::max<size_t>(act_bytes, 256)));
    HIPCHK(hipMalloc((void**)&mm_scratch, (size_t)kMaxDepth * kMaxLanes * kMinMaxScratch * sizeof(float)));
    HIPCHK(hipMemset(mm_scratch, 0, (size_t)kMaxDepth * kMaxLanes * kMinMaxScratch * sizeof(float)));      // (arrival counters start at zero and reset themselves)
    depth = std::max(1, std::min(depth, kMaxDepth));
    host_depth = std::max(1, std::min(host_depth, kMaxDepth));
    if (depth > 1 && !ensure_contexts(depth, err)) return false;
    for (size_t si = 0; si < steps.size(); si++) {
        const float** slots[4] = {&steps[si].w0, &steps[si].w1, &steps[si].w2, &steps[si].w3};
        for (int k = 0; k < 4; k++)
            if (wp.step_w[k][si] != SIZE_MAX) *slots[k] = reinterpret_cast<const float*>(w_arena) + wp.step_w[k][si];
        if (wp.step_bx[si] != SIZE_MAX) steps[si].wbx = reinterpret_cast<const uint16_t*>(reinterpret_cast<const float*>(w_arena) + wp.step_bx[si]);
        if (steps[si].kind == S_FRONTEND) {
            specs[steps[si].spec].G = reinterpret_cast<const double*>(steps[si].w0);
            specs[steps[si].spec].window = steps[si].w1;
        }
        if (steps[si].kind == S_STFT) {
            specs[steps[si].spec].window_full = steps[si].w0;
            specs[steps[si].spec].bins = reinterpret_cast<const int*>(steps[si].w1);
            specs[steps[si].spec].stft_tw = reinterpret_cast<const double*>(steps[si].w2);
        }
    }
    HIPCHK(hipMalloc((void**)&d_stage_in, (size_t)max_batch * n_samples * 4));
    HIPCHK(hipMalloc((void**)&d_stage_logits, (size_t)max_batch * n_classes * 4));
    HIPCHK(hipMalloc((void**)&d_post_conf, (size_t)max_batch * n_classes * 4));
    if (emb_dim) HIPCHK(hipMalloc((void**)&d_stage_emb, (size_t)max_batch * emb_dim * 4));
    if (!defer_weights) mark_bf16_storage();
    if (autotune && !defer_weights) { tune_or_load(); time_fold_proj(); }
    *code = BNHIP_OK;
    return true;
}

// Streams are pooled per DEVICE, not per engine: HIP maps all streams of a process on a device onto at most four hardware
// queues, so a second engine on the same GPU (another model, or the second shard of a {"devices":[0,0]} handle) that created
// streams of its own would push everybody onto shared queues - measured 0.61-0.69x the single-engine rate for two engines
// on one GPU.  Engines on one device therefore share its (up to four) kernel streams and its one copy stream; their work
// interleaves in stream order, which is all the ordering independent clips need.
namespace {
struct DevStreams { hipStream_t k[Engine::kMaxKStreams] = {nullptr, nullptr, nullptr, nullptr}; hipStream_t xfer = nullptr; int refs = 0; };
std::mutex g_ds_mu;
std::map<int, DevStreams> g_ds;
}  // namespace

hipStream_t Engine::kernel_stream(int i) {
    if (i < 0 || i >= kMaxKStreams || device < 0) return nullptr;
    if (kstream[i]) return kstream[i];
    std::lock_guard<std::mutex> lk(g_ds_mu);
    DevStreams& ds = g_ds[device];
    if (!ds_ref) { ds.refs++; ds_ref = true; }
    if (!ds.k[i] && hipStreamCreateWithFlags(&ds.k[i], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ds.k[i] = nullptr; }
    kstream[i] = ds.k[i];
    return kstream[i];
}
hipStream_t Engine::copy_stream() {
    if (device < 0) return nullptr;
    if (xfer_stream) return xfer_stream;
    std::lock_guard<std::mutex> lk(g_ds_mu);
    DevStreams& ds = g_ds[device];
    if (!ds_ref) { ds.refs++; ds_ref = true; }
    if (!ds.xfer) {
        // highest priority: copies are what should go first (and a queue pooled by priority is less likely to be a kernel queue)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&ds.xfer, hipStreamNonBlocking, greatest) != hipSuccess) { (void)hipGetLastError(); ds.xfer = nullptr; }
    }
    xfer_stream = ds.xfer;
    return xfer_stream;
}
void Engine::release_streams() {
    for (int i = 0; i < kMaxKStreams; i++) if (kstream[i]) hipStreamSynchronize(kstream[i]);
    if (xfer_stream) hipStreamSynchronize(xfer_stream);
    std::lock_guard<std::mutex> lk(g_ds_mu);
    if (ds_ref) {
        auto it = g_ds.find(device);
        if (it != g_ds.end() && --it->second.refs == 0) {
            for (auto st : it->second.k) if (st) hipStreamDestroy(st);
            if (it->second.xfer) hipStreamDestroy(it->second.xfer);
            g_ds.erase(it);
        }
        ds_ref = false;
    }
    for (int i = 0; i < kMaxKStreams; i++) kstream[i] = nullptr;
    xfer_stream = nullptr;
}

// Contexts 0..d-1 (stream, completion event, activation arena; context 0 shares the engine's own arena).  Idempotent.
bool Engine::ensure_contexts(int d, std::string* err, bool with_streams) {
    d = std::max(1, std::min(d, kMaxDepth));
    if (device < 0) { *err = "plan-only model has no contexts"; return false; }
    hipSetDevice(device);
    if (with_streams && !ev_ctx_fork) HIPCHK(hipEventCreateWithFlags(&ev_ctx_fork, hipEventDisableTiming));
    for (int c = 0; c < d; c++) {
        if (with_streams) {
            if (!ctx_stream[c]) { ctx_stream[c] = kernel_stream(1 + c); if (!ctx_stream[c]) { *err = "hipStreamCreate failed"; return false; } }
            if (!ev_ctx_done[c]) HIPCHK(hipEventCreateWithFlags(&ev_ctx_done[c], hipEventDisableTiming));
        }
        if (!ctx_arena[c]) {
            if (c == 0) ctx_arena[c] = act_arena;
            else HIPCHK(hipMalloc((void**)&ctx_arena[c], std::max<size_t>(act_bytes, 256)));
        }
    }
    return true;
}

void Engine::finish_deferred() {
    if (device < 0) return;
    hipSetDevice(device);
    mark_bf16_storage();
    if (autotune) { tune_or_load(); time_fold_proj(); }
    defer_weights = false;
}

// ---- one step's GEMM parameters
// What a call of n clips launches step s with, on one of its two tunings, in the storage flavour the calls run: everything but the
// operand pointers.
PwParams Engine::pw_params(const Step& s, int n, bool lane_tuning) const {
    PwParams p{nullptr, s.w0, s.w1, nullptr, nullptr, nullptr, n * s.H * s.W, s.Co, s.C, s.H * s.W, s.act, lane_tuning ? s.nt : s.nt_full,
               lane_tuning ? s.wm : s.wm_full};
    p.prec = precision; p.sw = pw_sw;
    p.a_bf16 = vals[s.in0].half ? 1 : 0; p.out_bf16 = vals[s.out].half ? 1 : 0;
    p.res_bf16 = (s.in2 >= 0 && vals[s.in2].half) ? 1 : 0;
    return p;
}
// ---- fused tails (Step::tail, k_pw_b16's clip-aligned row tiles with the consumer in the epilogue)
PwTail tail_of(const Step& s, const Step& c) {
    PwTail t;
    t.kind = s.tail; t.H = s.H; t.W = s.W;
    if (s.tail == 2) { t.k = c.kh; t.pt = c.pt; t.pl = c.pl; t.act = c.act; t.w = c.w0; t.bias = c.w1; }
    return t;
}
// A call takes the fused form of step si when the tuning chose it, the launches it replaces lie in the same part of the plan (a
// two-phase host call never cuts a pair in two forms) and the clip-aligned tiles put a block on every CU; smaller calls run the
// pair - same bits.  BNHIP_PW_TAIL=2 takes it for every call.
bool Engine::tail_taken(int si, int n, bool lane_tuning) const {
    const Step& s = steps[si];
    if (s.kind != S_PW || !s.tail || !s.wbx) return false;
    const int wm = lane_tuning ? s.wm : s.wm_full, nt = lane_tuning ? s.nt : s.nt_full;
    if (wm < 13) return false;
    const int last = si + (s.tail == 1 ? 2 : 1), s_end = part_s1 < 0 ? (int)steps.size() : part_s1;
    if (si < part_s0 || last >= s_end) return false;
    if (s.tail == 2 && steps[si + 1].dwl) return false;
    const PwParams p = pw_params(s, n, lane_tuning);
    if (!pw_tail_ok(p, tail_of(s, steps[si + 1]), nt, wm)) return false;
    return (pw_sw & PW_SW_TAIL_FORCE) || pw_tail_fills(p, nt, wm);
}

// ---- min/max + normalise as one launch
// The plan keeps its two steps; a lane runs them as k_clip_norm_resident when the plan has the pair (norm_pair, find_norm_pair), the
// lane has more than 16 clips (smaller ones keep k_clip_minmax_parts, which exists for their latency), the clip fits on chip and the
// pointers are aligned to whole quads - otherwise the pair runs, same bits.  BNHIP_NORM_RESIDENT=0, read once in build(), keeps the
// pair everywhere.
void Engine::find_norm_pair() {
    norm_pair = -1; pcm_direct = false;
    if (!norm_resident || specs.empty()) return;
    for (int si = 0; si + 1 < (int)steps.size(); si++) {
        const Step& a = steps[si]; const Step& b = steps[si + 1];
        if (a.kind == S_MINMAX && b.kind == S_NORMALIZE && a.in0 == v_input && b.in0 == v_input && b.in1 == a.out) { norm_pair = si; break; }
    }
    if (norm_pair < 0 || !clip_norm_resident_fits(n_samples)) { norm_pair = -1; return; }
    // PCM straight into the launch: only when nothing else in the plan reads the float waveform
    pcm_direct = true;
    for (int si = 0; si < (int)steps.size(); si++) {
        if (si == norm_pair || si == norm_pair + 1) continue;
        const Step& s = steps[si];
        if (s.in0 == v_input || s.in1 == v_input || s.in2 == v_input) pcm_direct = false;
    }
}
bool Engine::norm_resident_taken(int n, const void* x, int bits, const float* xn) const {
    if (norm_pair < 0 || n <= 16) return false;
    const uintptr_t in_align = bits == 16 ? 8 : bits == 24 ? 4 : 16;
    return !(reinterpret_cast<uintptr_t>(x) & (in_align - 1)) && !(reinterpret_cast<uintptr_t>(xn) & 15);
}

// ---- a narrow projection inside its reader's launch
// Eligible (plan time): an fp32 engine's pointwise projection on the f32-MFMA kernel with at most 16 output channels from at most 32
// inputs, no activation, no residual, whose output is read by nothing but the next step - a fused expand+depthwise layer in the
// chunk-loop small-K form with one K slab and a 3 x 3 stride-2 filter (the instantiated shapes).  In the v2.4 stack that is
// b1/project -> b2/expand+dw; the other single-reader projections feed layers of 144+ channels and would move more bytes than they save.
// A call takes the one launch when both steps lie in the part of the plan it runs (a two-phase host call cut between them runs the
// pair), the projection's tuning is an f32-MFMA tile, and the call is large enough that the chunk loop is not cut into parts
// (expdw_proj_ok).  BNHIP_FOLD_PROJ=0, read once in build(), keeps the pair everywhere.
void Engine::find_fold_pair() {
    fold_pair = -1;
    if (!fold_proj || precision != 0) return;
    const int ns = (int)steps.size();
    for (int si = 0; si + 1 < ns; si++) {
        const Step& a = steps[si]; const Step& b = steps[si + 1];
        if (a.kind != S_PW || b.kind != S_EXPAND_DW || b.mode == 1 || b.in0 != a.out || a.out < 0) continue;
        if (a.in2 >= 0 || a.act != ACT_NONE || a.tail || (a.bx && bf16x3) || a.Co > 16 || a.C > 32 || (a.C & 3) || (a.Co & 3)) continue;
        if (a.H != b.H || a.W != b.W || a.Co != b.C || b.kh != 3 || b.sh != 2 || expdw_skw(b.C, b.act, false) != 16) continue;
        if (a.out == v_logits || a.out == v_emb || a.out == v_input || vals[a.out].external) continue;
        int readers = 0;
        for (const Step& t : steps)
            for (int v : {t.in0, t.in1, t.in2}) readers += v == a.out;
        if (readers != 1) continue;
        fold_pair = si;
        break;
    }
}
bool Engine::fold_taken(int si, int n, bool lane_tuning) const {
    if (fold_pair < 0 || si != fold_pair || !fold_faster) return false;
    const int s_end = part_s1 < 0 ? (int)steps.size() : part_s1;
    if (si < part_s0 || si + 1 >= s_end) return false;
    const Step& a = steps[si]; const Step& b = steps[si + 1];
    if (a.wbx && (lane_tuning ? a.wm : a.wm_full) >= 5) return false;             // (tuned onto the split-bf16 family: other arithmetic)
    if (vals[a.in0].half || vals[a.out].half || vals[b.out].half || expdw_pipe16(b)) return false;
    return expdw_proj_ok(b.shape, expdw_geo(b), n, b.Co);
}

// ================================================================================================ run
float* Engine::vptr(int v, const float* d_in, float* d_logits, float* d_emb, int lane) const {
    if (v < 0) return nullptr;
    if (v == v_input) return const_cast<float*>(d_in);
    if (v == v_logits) return d_logits;
    if (part_hand && v == v_hand) return part_hand;
    (void)d_emb;
    char* base = cur_arena ? cur_arena : act_arena;
    // lane >= 0: that lane's own copy of the lane layout (values are [clip][elems] from the lane's first clip)
    if (lane >= 0) return reinterpret_cast<float*>(base + (size_t)lane * lane_bytes + vals[v].offset_lane);
    return reinterpret_cast<float*>(base + vals[v].offset);
}

hipEvent_t Engine::get_event() {
    if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
    hipEvent_t e; hipEventCreate(&e); return e;
}

void Engine::drop_graphs() {
    for (auto& g : graphs) if (g.exec) hipGraphExecDestroy(g.exec);
    graphs.clear();
}

// The plan is a fixed sequence of ~60 launches; for the product's call pattern (one clip per Predict) the forward pass
// is launch-bound, so once the same (input, output, n) combination shows up a second time it is captured into a
// hipGraph and replayed from then on (the host-pointer entry points always use the same staging buffers).  Per-launch
// profiling needs real launches and bypasses the graph.
// Call i of a pipelined sequence: wait (on the GPU) for whatever the caller's stream has queued so far, then run the whole
// plan on context i % depth.  Calls on different contexts overlap; calls on the same context are ordered by its stream.
bool Engine::run_pipelined(const float* d_in, int n, float* d_logits, float* d_emb, std::string* err) {
    if (n <= 0 || n > max_batch) { *err = "batch size out of range"; return false; }
    if (depth <= 1 || (profiling && profile_filter.empty())) return run(d_in, n, d_logits, d_emb, err);
    const int c = (int)(call_idx++ % (unsigned)depth);
    if (ctx_stream[c] != stream) {              // (context 0 IS the main stream until the caller hands in its own)
        hipEventRecord(ev_ctx_fork, stream);
        hipStreamWaitEvent(ctx_stream[c], ev_ctx_fork, 0);
    }
    cur_arena = ctx_arena[c];
    cur_stream = ctx_stream[c];
    cur_ctx = c;
    bool ok = run_eager(d_in, n, d_logits, d_emb, err);
    cur_arena = nullptr;
    cur_stream = nullptr;
    cur_ctx = -1;
    return ok;
}
// One chunk of a host-pointer call in context c's arena on stream st (hostpipe.cpp orders st behind the chunk's copy and
// records its completion): the whole plan, unsplit.
bool Engine::run_on_context(int c, hipStream_t st, const float* d_in, int n, float* d_logits, float* d_emb, std::string* err, PcmSource pcm) {
    if (n <= 0 || n > max_batch) { *err = "batch size out of range"; return false; }
    if (c < 0 || c >= kMaxDepth || !st || !ctx_arena[c]) { *err = "context does not exist"; return false; }
    call_idx++;                                  // a later unsplit run() orders itself behind the contexts
    cur_arena = ctx_arena[c];
    cur_stream = st;
    cur_ctx = c;                                 // (the context's own min/max scratch)
    bool ok = run_eager(d_in, n, d_logits, d_emb, err, pcm);
    cur_ctx = -1;
    cur_arena = nullptr;
    cur_stream = nullptr;
    return ok;
}
// Steps [s0, s1) for n clips in context c's arena on stream st (hostpipe.cpp's two-phase calls); the one value that crosses the cut
// is read / written at `hand` instead of its arena slot.
bool Engine::run_part(int c, hipStream_t st, int s0, int s1, const float* d_in, int n, float* hand, float* d_logits, float* d_emb, std::string* err, PcmSource pcm) {
    if (n <= 0 || n > max_batch) { *err = "batch size out of range"; return false; }
    if (c < 0 || c >= kMaxDepth || !st || !ctx_arena[c]) { *err = "context does not exist"; return false; }
    if (v_hand < 0 || !hand || s0 < 0 || s1 > (int)steps.size() || s0 >= s1 || (s0 != 0 && s0 != split_step) || (s1 != (int)steps.size() && s1 != split_step)) {
        *err = "not a cut of this plan"; return false;
    }
    if (pcm.samples && s0 != 0) { *err = "a PCM source belongs to the part that starts the plan"; return false; }
    call_idx++;
    cur_arena = ctx_arena[c];
    cur_stream = st;
    cur_ctx = c;
    part_s0 = s0; part_s1 = s1; part_hand = hand;
    bool ok = run_eager(d_in, n, d_logits, d_emb, err, pcm);
    part_s0 = 0; part_s1 = -1; part_hand = nullptr;
    cur_ctx = -1;
    cur_arena = nullptr;
    cur_stream = nullptr;
    return ok;
}
int Engine::heatmap_pruned_step() const {
    if (steps.empty() || precision != 0) return -1;
    const Step& s = steps.back();
    if (s.kind != S_PW || s.out != v_logits || s.in1 >= 0 || s.in2 >= 0 || s.H * s.W != 1 || s.Co != n_classes) return -1;
    if (s.in0 < 0 || vals[s.in0].half || vals[s.in0].elems != (size_t)s.C) return -1;
    return (int)steps.size() - 1;
}
bool Engine::run_head(int s1, const float* d_in, int n, std::string* err) {
    if (n <= 0 || n > max_batch) { *err = "batch size out of range"; return false; }
    if (s1 < 0 || s1 > (int)steps.size()) { *err = "not a cut of this plan"; return false; }
    cur_stream = stream;                         // (a call with its own main stream runs on one lane)
    part_s1 = s1;
    bool ok = run_eager(d_in, n, nullptr, nullptr, err);
    part_s1 = -1;
    cur_stream = nullptr;
    return ok;
}
bool Engine::ensure_hand(std::string* err) {
    if (d_hand || v_hand < 0) return v_hand >= 0;
    if (hipMalloc((void**)&d_hand, std::max<size_t>((size_t)max_batch * hand_clip_bytes(), 256)) != hipSuccess) {
        (void)hipGetLastError(); d_hand = nullptr; *err = "hand-off allocation failed"; return false;
    }
    return true;
}
// Where a call that fits one batch is cut in two (run_part): the launch boundaries a single activation crosses are the block
// boundaries of the stack; of those, the first one whose crossing value has fewer than `rows_min` spatial positions per clip - from
// there on a quarter-batch chunk has too few rows to fill 256 CUs and the layers are worth running over a larger group (v2.4 stack:
// the input of b5; cuts from b4 to b7 measured within 2 % of each other, earlier and later ones lose).
// BNHIP_HOST_SPLIT=<step index> picks a boundary by hand (snapped to the next candidate), -1 disables; read once here, at plan time.
void Engine::pick_split() {
    split_step = -1; v_hand = -1; split_candidates.clear();
    const int ns = (int)steps.size();
    std::vector<int> crossing(ns, -1);
    for (int k = 1; k < ns; k++) {
        int cnt = 0, who = -1; bool bad = false;
        for (int v = 0; v < (int)vals.size(); v++) {
            const Value& V = vals[v];
            if (V.first < 0 || V.first >= k || V.last < k) continue;      // not alive across the boundary before step k
            if (v == v_input || v == v_logits || v == v_emb || V.external) { bad = true; break; }
            cnt++; who = v;
        }
        if (!bad && cnt == 1) { split_candidates.push_back(k); crossing[k] = who; }
    }
    int want = -2;
    if (const char* e = getenv("BNHIP_HOST_SPLIT")) want = atoi(e);
    if (want == -1 || split_candidates.empty()) return;
    int pick = -1;
    if (want >= 0) {
        for (int k : split_candidates) if (k >= want) { pick = k; break; }
    } else {
        const int rows_min = (int)((long)(device >= 0 ? device_cus() : 256) * 1000 / 256);      // (1000 on the 256 CUs of an MI355X)
        for (int k : split_candidates) {
            const Step& s = steps[k];                                    // the consumer's input geometry = the crossing value's
            if ((s.kind == S_PW || s.kind == S_EXPAND_DW || s.kind == S_DW) && s.H * s.W < rows_min && s.H * s.W > 0) { pick = k; break; }
        }
    }
    if (pick < 0) return;
    split_step = pick; v_hand = crossing[pick];
    if (getenv("BNHIP_DEBUG")) {
        fprintf(stderr, "[bnhip] host split: step %d (%s), value %d (%zu elems/clip%s); candidates:", split_step, steps[split_step].name.c_str(), v_hand,
                vals[v_hand].elems, vals[v_hand].half ? ", bf16" : "");
        for (int k : split_candidates) fprintf(stderr, " %d", k);
        fprintf(stderr, "\n");
    }
}
void Engine::sync_contexts() {
    for (int i = 0; i < kMaxKStreams; i++) if (kstream[i]) hipStreamSynchronize(kstream[i]);
}

bool Engine::run(const float* d_in, int n, float* d_logits, float* d_emb, std::string* err, PcmSource pcm) {
    if (n <= 0 || n > max_batch) { *err = "batch size out of range"; return false; }
    if (call_idx) {
        // an unsplit call after pipelined ones: order it (on the GPU) behind whatever the contexts still have queued -
        // context 0 shares this call's arena
        for (int c = 0; c < kMaxDepth; c++)
            if (ctx_stream[c] && ctx_stream[c] != stream) { hipEventRecord(ev_ctx_done[c], ctx_stream[c]); hipStreamWaitEvent(stream, ev_ctx_done[c], 0); }
        if (kstream[0] && kstream[0] != stream) hipStreamSynchronize(kstream[0]);      // (caller-owned main stream: the engine's own may still hold a chunk)
    }
    // (a window table moves from chunk to chunk of its call: nothing to replay)
    if (!use_graphs || profiling || pcm.win.first) return run_eager(d_in, n, d_logits, d_emb, err, pcm);
    GraphEntry* ge = nullptr;
    for (auto& g : graphs)
        if (g.in == d_in && g.logits == d_logits && g.emb == d_emb && g.n == n && g.pcm == pcm.samples && g.pcm_bits == pcm.bits) { ge = &g; break; }
    if (ge && ge->exec) {
        hipError_t e = hipGraphLaunch(ge->exec, stream);
        if (e != hipSuccess) { *err = std::string("hipGraphLaunch: ") + hipGetErrorString(e); return false; }
        return true;
    }
    if (!ge) {                                   // first sighting: run eagerly (also primes one-time function attributes)
        if (graphs.size() >= 8) { if (graphs.front().exec) hipGraphExecDestroy(graphs.front().exec); graphs.erase(graphs.begin()); }
        graphs.push_back(GraphEntry{d_in, d_logits, d_emb, n, 1, nullptr, pcm.samples, pcm.bits});
        return run_eager(d_in, n, d_logits, d_emb, err, pcm);
    }
    // second sighting: capture, instantiate, replay
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) { (void)hipGetLastError(); use_graphs = false; return run_eager(d_in, n, d_logits, d_emb, err, pcm); }
    bool ok = run_eager(d_in, n, d_logits, d_emb, err, pcm);
    e = hipStreamEndCapture(stream, &graph);
    if (!ok || e != hipSuccess || !graph) {
        if (graph) hipGraphDestroy(graph);
        (void)hipGetLastError();
        use_graphs = false;                      // capture is not available on this stream: stay eager
        return run_eager(d_in, n, d_logits, d_emb, err, pcm);
    }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess || !exec) { (void)hipGetLastError(); use_graphs = false; return run_eager(d_in, n, d_logits, d_emb, err, pcm); }
    ge->exec = exec;
    e = hipGraphLaunch(exec, stream);
    if (e != hipSuccess) { *err = std::string("hipGraphLaunch: ") + hipGetErrorString(e); return false; }
    return true;
}

// Two lanes: the batch is split into two clip ranges that run the same plan on two streams (forked/joined with
// events around the call).  Every value is laid out [clip][elems], so a lane is just a clip offset into the same
// buffers.  The lanes fill each other's gaps: the short latency-bound launches (squeeze-excite, late layers with few
// workgroups) and every kernel's tail wave overlap the other lane's work.  Launches are interleaved step by step so
// neither lane waits for the other's enqueue.
bool Engine::run_eager(const float* d_in_all, int n_all, float* d_logits_all, float* d_emb_all, std::string* err, PcmSource pcm) {
    struct Lane { const float* d_in; int n; float* d_logits; float* d_emb; hipStream_t st; int clip0; };
    Lane lanes[kMaxLanes];
    int nl = 1;
    hipStream_t main_stream = cur_stream ? cur_stream : stream;
    if (mm_dirty) {
        //  a call on this engine failed: a launch of k_clip_minmax_parts that did not run to completion leaves its arrival
        // counter non-zero, and every later small call on that (context, lane) would normalise with stale min / max without any
        // error.  Error path only: drain the engine's streams and zero the scratch before anything else is queued.
        for (int i = 0; i < kMaxKStreams; i++) if (kstream[i]) hipStreamSynchronize(kstream[i]);
        if (stream) hipStreamSynchronize(stream);
        if (mm_scratch) hipMemset(mm_scratch, 0, (size_t)kMaxDepth * kMaxLanes * kMinMaxScratch * sizeof(float));
        (void)hipGetLastError();
        mm_dirty = false;
    }
    // (an unfiltered profile wants clean per-kernel times and stays single-lane; a class-filtered one measures the
    // kernels as they run in production, overlapped)
    if (n_lanes > 1 && !cur_stream && (!profiling || !profile_filter.empty()) && n_all >= dual_lane_min) nl = std::min(n_lanes, n_all);
    for (int li = 0, c0 = 0; li < nl; li++) {
        int cnt = n_all / nl + (li < n_all % nl ? 1 : 0);
        lanes[li] = Lane{d_in_all + (size_t)c0 * n_samples, cnt, d_logits_all + (size_t)c0 * n_classes,
                         d_emb_all ? d_emb_all + (size_t)c0 * emb_dim : nullptr, li == 0 ? main_stream : lane_stream[li - 1], c0};
        c0 += cnt;
    }
    hipEvent_t st_a = nullptr, st_b = nullptr;
    if (step_timing) { hipEventCreate(&st_a); hipEventCreate(&st_b); hipEventRecord(st_a, main_stream); }
    if (nl > 1) {
        hipEventRecord(ev_fork, main_stream);
        for (int li = 1; li < nl; li++) hipStreamWaitEvent(lanes[li].st, ev_fork, 0);
    }
    const int s_end = part_s1 < 0 ? (int)steps.size() : part_s1;
    // min/max + normalise as one launch (k_clip_norm_resident): decided ONCE per lane, here - what the launch reads (the lane's float
    // clips, or its PCM samples where nothing else in the plan reads the waveform) or nullptr for the pair.  A lane of a PCM call that
    // does not convert in that launch gets its float copy first.
    // A call with a window table (file analysis): the lane's windows are read out of the recordings by that launch (its framed form:
    // nothing but the pair may read the waveform, float32 input included, and the hop must keep the quads aligned), or framed into the
    // lane's float input first.
    const void* res_x[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr};
    int res_bits[kMaxLanes] = {0, 0, 0, 0};
    bool res_framed[kMaxLanes] = {false, false, false, false};
    for (int li = 0; li < nl; li++) {
        const Lane& L = lanes[li];
        const bool pair_here = norm_pair >= part_s0 && norm_pair + 1 < s_end;
        const float* xn = pair_here ? vptr(steps[norm_pair + 1].out, L.d_in, L.d_logits, L.d_emb, nl > 1 ? li : -1) : nullptr;
        if (pcm.win.first) {
            if (pair_here && pcm_direct && clip_norm_framed_ok(pcm.samples, pcm.win) && norm_resident_taken(L.n, pcm.samples, pcm.bits, xn)) {
                res_x[li] = pcm.samples; res_bits[li] = pcm.bits; res_framed[li] = true; continue;
            }
            launch_frame_windows(pcm.samples, pcm.bits, win_at(pcm.win, L.clip0), L.n, n_samples, const_cast<float*>(L.d_in), L.st);
            if (pair_here && norm_resident_taken(L.n, L.d_in, 0, xn)) res_x[li] = L.d_in;
            continue;
        }
        const char* src = pcm.samples ? static_cast<const char*>(pcm.samples) + (size_t)L.clip0 * n_samples * (pcm.bits / 8) : nullptr;
        if (src && pair_here && pcm_direct && norm_resident_taken(L.n, src, pcm.bits, xn)) { res_x[li] = src; res_bits[li] = pcm.bits; continue; }
        if (src) launch_pcm_to_f32(src, pcm.bits, const_cast<float*>(L.d_in), (size_t)L.n * n_samples, L.st);
        if (pair_here && norm_resident_taken(L.n, L.d_in, 0, xn)) res_x[li] = L.d_in;
    }
    for (int si = part_s0; si < s_end; si++) {
      for (int li = 0; li < nl; li++) {
        const Step& s = steps[si];
        const float* d_in = lanes[li].d_in; float* d_logits = lanes[li].d_logits; float* d_emb = lanes[li].d_emb;
        const int n = lanes[li].n, clip0 = nl > 1 ? li : -1;      // arena addressing: lane index, or -1 for the unsplit layout
        hipStream_t stream = lanes[li].st;
        float* in0 = vptr(s.in0, d_in, d_logits, d_emb, clip0);
        float* in1 = vptr(s.in1, d_in, d_logits, d_emb, clip0);
        float* in2 = vptr(s.in2, d_in, d_logits, d_emb, clip0);
        float* out = vptr(s.out, d_in, d_logits, d_emb, clip0);
        float* out2 = vptr(s.out2, d_in, d_logits, d_emb, clip0);
        // a step whose work ran in the epilogue of the GEMM in front of it (fused tail)
        if (s.kind == S_DW && si > 0 && steps[si - 1].tail == 2 && tail_taken(si - 1, n, nl > 1)) continue;
        if (s.kind == S_MEAN_PARTIAL && si > 0 && steps[si - 1].tail == 1 && tail_taken(si - 1, n, nl > 1)) continue;
        if (s.kind == S_MEAN_FINISH && si > 1 && steps[si - 2].tail == 1 && tail_taken(si - 2, n, nl > 1)) continue;
        if (s.kind == S_NORMALIZE && si == norm_pair + 1 && res_x[li]) continue;      // ran inside the clip_minmax step's launch
        if (s.kind == S_PW && fold_taken(si, n, nl > 1)) continue;                    // runs inside the next step's launch (folded projection)
        ProfEntry pe{};
        // diagnostics (tools/debug): a host-side synchronize before / after every launch of one kernel class
        static const char* dbg_sync_before = getenv("BNHIP_DEBUG_SYNC_BEFORE");
        static const char* dbg_sync_after = getenv("BNHIP_DEBUG_SYNC_AFTER");
        // ... and a co-runner filter: context 1 launches only the listed kernel classes (its outputs are then garbage)
        static const char* dbg_ctx1_only = getenv("BNHIP_DEBUG_CTX1_ONLY");
        if (dbg_ctx1_only && cur_ctx == 1 && !strstr(dbg_ctx1_only, s.kclass)) continue;
        static const char* dbg_ctx1_skip = getenv("BNHIP_DEBUG_CTX1_SKIP");
        if (dbg_ctx1_skip && cur_ctx == 1 && strstr(dbg_ctx1_skip, s.kclass)) continue;
        if (dbg_sync_before && (!strcmp(dbg_sync_before, s.kclass) || s.name.rfind(dbg_sync_before, 0) == 0)) hipStreamSynchronize(stream);
        const bool prof_this = profiling && (profile_filter.empty() || profile_filter == s.kclass);
        if (prof_this) { pe.a = get_event(); pe.b = get_event(); pe.step = si; pe.n = n; hipEventRecord(pe.a, stream); }
        switch (s.kind) {
            case S_MINMAX:
                if (si == norm_pair && res_x[li]) {
                    // (launch_clip_norm_resident refuses exactly what norm_resident_taken refuses: a refusal here is a bug, not a fallback)
                    const WinView lane_win = win_at(pcm.win, lanes[li].clip0);
                    if (!launch_clip_norm_resident(res_x[li], res_bits[li], n, n_samples, specs[0].eps, specs[0].norm_sub, specs[0].norm_mul,
                                                   reinterpret_cast<float2*>(out), vptr(steps[si + 1].out, d_in, d_logits, d_emb, clip0), stream,
                                                   res_framed[li] ? &lane_win : nullptr)) {
                        *err = "k_clip_norm_resident refused a call its predicate accepted"; mm_dirty = true; return false;
                    }
                    // (profile: the launch reads x once, as float or as PCM, and writes xn - the normalize step's bytes, not the sum)
                    pe.more_bytes = steps[si + 1].bytes - s.bytes - (res_bits[li] ? (double)n_samples * (4 - res_bits[li] / 8) : 0.0);
                    break;
                }
                // (scratch of the small-call form: a buffer of its own per context and lane - the arena's full and lane layouts
                // share memory, a counter kept there would be overwritten by the other layout's activations between calls)
                launch_clip_minmax(in0, n, n_samples, specs[0].eps, reinterpret_cast<float2*>(out),
                                   mm_scratch ? mm_scratch + ((size_t)std::max(cur_ctx, 0) * kMaxLanes + (size_t)li) * kMinMaxScratch : nullptr, stream);
                break;
            case S_FRONTEND: {
                const FrontSpec& fs = specs[s.spec];
                FrontendParams p;
                p.x = in0; p.mm = reinterpret_cast<const float2*>(in1); p.G = fs.G; p.window = fs.window; p.out = out;
                p.n_samples = n_samples; p.L = fs.L; p.Lfft = fs.Lfft; p.Kp = fs.Kp; p.hop = fs.hop; p.F = fs.F; p.n_mels = fs.n_mels;
                p.NTP = fs.NTP; p.C = C_spec; p.c = fs.c; p.norm_sub = fs.norm_sub; p.norm_mul = fs.norm_mul;
                p.p1 = fs.p1; p.p2 = fs.p2; p.n_clips = n;
                launch_frontend(p, stream);
                break;
            }
            case S_NORMALIZE:
                launch_normalize(in0, reinterpret_cast<const float2*>(in1), out, n, n_samples, specs[0].norm_sub, specs[0].norm_mul, stream);
                break;
            case S_STFT: {
                const FrontSpec& fs = specs[s.spec];
                StftParams p{in0, fs.window_full, fs.bins, out, n_samples, fs.Lfft, fs.L, fs.hop, fs.F, fs.nb, fs.nbp, fs.mode, n, fs.stft_tw, fs.pad_left};
                p.zmask = fs.stft_zmask;
                if (s.mode == 1) {                           // fused mel epilogue: `out` is the spectrogram image
                    p.out = nullptr; p.img = out; p.mel = s.w3; p.mel_quads = s.S; p.n_mels = fs.n_mels; p.Ctot = C_spec; p.c0 = fs.c;
                    p.logc = fs.log_compress ? 1 : 0; p.time_major = fs.time_major ? 1 : 0; p.p1 = fs.p1; p.p2 = fs.p2;
                    p.lfloor = fs.log_floor; p.lscale = fs.log_scale;
                }
                {
                    static const bool f32_off = getenv("BNHIP_STFT_F32") && atoi(getenv("BNHIP_STFT_F32")) == 0;
                    // fp32 transform: bf16 engines whose front-end compresses with a floored log (Perch-style) - a power-law
                    // compression (v2.4: x^0.45) amplifies fp32 transform noise in near-empty bins by orders of magnitude
                    if (precision == 1 && s.mode != 1 && fs.log_compress && !f32_off) p.f32 = 1;
                }
                launch_stft_bins(p, stream);
                break;
            }
            case S_MELBAND: {
                const FrontSpec& fa = specs[s.spec];
                const FrontSpec& fb = specs[s.S == 2 ? s.op : s.spec];
                MelBandParams p{{in0, s.S == 2 ? in1 : in0}, {s.w0, s.S == 2 ? s.w2 : s.w0},
                                {reinterpret_cast<const int*>(s.w1), reinterpret_cast<const int*>(s.S == 2 ? s.w3 : s.w1)},
                                {fa.nbp, fb.nbp}, {fa.p1, fb.p1}, {fa.p2, fb.p2}, out, fa.F, fa.n_mels, C_spec, fa.c,
                                fa.log_compress ? 1 : 0, fa.log_floor, fa.log_scale, fa.time_major ? 1 : 0};
                launch_mel_banded(p, s.S, n, stream);
                break;
            }
            case S_MELFIN: {
                const FrontSpec& fa = specs[s.spec];
                const FrontSpec& fb = specs[s.S == 2 ? s.op : s.spec];
                MelFinParams p{{in0, s.S == 2 ? in1 : in0}, {fa.p1, fb.p1}, {fa.p2, fb.p2}, out, fa.F, fa.n_mels, fa.n_mels, C_spec, fa.c,
                               fa.log_compress ? 1 : 0, fa.log_floor, fa.log_scale, fa.time_major ? 1 : 0};
                launch_mel_finish(p, s.S, n, stream);
                break;
            }
            case S_CONV_DIRECT: {
                ConvParams p{in0, s.w0, s.w1, out, n, s.H, s.W, s.C, s.Ho, s.Wo, s.Co, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.act};
                p.out_bf16 = vals[s.out].half ? 1 : 0;
                if (s.w2) launch_stem_mfma(p, s.w2, s.w3, stream);
                else launch_conv_direct(p, stream);
                break;
            }
            case S_CONV_IGEMM:
                launch_conv_igemm(in0, s.w0, s.w1, out, n, s.H, s.W, s.C, s.Ho, s.Wo, s.Co, s.kh, s.kw, s.sh, s.sw, s.g.dh, s.g.dw, s.pt, s.pl,
                                  s.act, 0, 0, stream);
                break;
            case S_PW: {
                PwParams p = pw_params(s, n, nl > 1);
                p.A = in0; p.ascale = in1; p.res = in2; p.out = out;
                if (tail_taken(si, n, nl > 1)) {
                    const Step& c = steps[si + 1];
                    PwTail t = tail_of(s, c);
                    if (s.tail == 2) { t.out = vptr(c.out, d_in, d_logits, d_emb, clip0); t.partial = vptr(c.out2, d_in, d_logits, d_emb, clip0); }
                    else p.out = vptr(steps[si + 2].out, d_in, d_logits, d_emb, clip0);
                    launch_pw_tail(p, t, s.wbx, p.nt, p.wm, stream);
                    break;
                }
                if (p.wm >= 13) p.wm = 10;        // a call too small for the fused form: the same column tile on 64-row tiles, then its consumer
                if (p.wm >= 5 && s.wbx) launch_pw_bx3(p, s.wbx, stream);
                else launch_pw_gemm(p, stream);
                break;
            }
            case S_DW: {
                DwParams p = dw_params(s, in0, out, n);
                p.in_bf16 = vals[s.in0].half ? 1 : 0; p.out_bf16 = vals[s.out].half ? 1 : 0;
                if (s.dwl) launch_dwconv_lds(p, out2, s.shape, stream);
                else launch_dwconv(p, out2, stream);
                break;
            }
            case S_EXPAND_DW:
                {
                    StemGeom sg{s.H2, s.W2, s.pt2, s.pl2};
                    ExpDwProj pj{};
                    const bool fold = si > 0 && fold_taken(si - 1, n, nl > 1);
                    if (fold) {
                        const Step& a = steps[si - 1];
                        pj = ExpDwProj{vptr(a.in0, d_in, d_logits, d_emb, clip0), a.w0, a.w1, vptr(a.in1, d_in, d_logits, d_emb, clip0), a.C, a.Co};
                        // (profile: the launch reads the projection's input and gate instead of the projection's output)
                        pe.more_bytes = 4.0 * s.H * s.W * (a.C - a.Co) + (a.in1 >= 0 ? 4.0 * a.C : 0.0);
                    }
                    if (!launch_expand_dw(in0, s.w0, s.w1, s.w2, s.w3, out, out2, n, s.H, s.W, s.C, s.Co,
                                          s.Ho, s.Wo, s.kh, s.sh, s.pt, s.pl, s.act, s.act2, s.shape, s.mode == 1 ? &sg : nullptr, stream,
                                          s.bx ? s.wbx : nullptr, precision, vals[s.out].half ? 1 : 0, vals[s.in0].half ? 1 : 0, fold ? &pj : nullptr)) {
                        *err = "k_expand_dw_sk refused a folded projection its predicate accepted"; mm_dirty = true; return false;
                    }
                }
                break;
            case S_MEAN_PARTIAL:
                launch_mean_partial(in0, out, n, s.H * s.W, s.C, s.S, stream);
                break;
            case S_MEAN_FINISH:
                launch_mean_finish(in0, out, n, s.H * s.W, s.C, s.S, stream);
                break;
            case S_SE: {
                SeParams p{in0, s.S, s.H * s.W, s.w0, s.w1, s.w2, s.w3, out, n, s.C, s.Cr, s.act, s.act2};
                if (cur_stream) p.threads = 256;      // pipelined call: 4-wave workgroups slot in beside the other context's kernels
                launch_se(p, stream);
                break;
            }
            case S_UNARY:
                launch_unary(in0, out, vals[s.in0].elems * (size_t)n, s.act, stream);
                break;
            case S_BINARY:
                launch_binary(in0, s.mode == 2 ? s.w0 : in1, out, vals[s.in0].elems * (size_t)n, s.op, s.mode, s.H * s.W, s.C,
                              s.act, stream);
                break;
            case S_EW_UNARY:
                launch_unary_op(in0, out, vals[s.in0].elems * (size_t)n, s.op, s.g.alpha, stream);
                break;
            case S_EW_BINARY: {
                BcastParams p;
                p.a = s.g.a_const ? s.w0 : in0; p.b = s.g.b_const ? s.w1 : in1; p.out = out;
                for (int k = 0; k < 4; k++) { p.d[k] = s.g.d[k]; p.sa[k] = s.g.sa[k]; p.sb[k] = s.g.sb[k]; }
                p.bsa = s.g.a_const ? 0 : (long)vals[s.in0].elems; p.bsb = s.g.b_const ? 0 : (long)vals[s.in1].elems;
                p.op = s.op; p.act = s.act;
                launch_binary_bcast(p, n, stream);
                break;
            }
            case S_POOL: {
                PoolParams p{in0, out, n, s.H, s.W, s.C, s.Ho, s.Wo, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.mode, s.act};
                launch_pool2d(p, stream);
                break;
            }
            case S_COPY: {
                if (s.g.fill) launch_fill(out, vals[s.out].elems * (size_t)n, s.g.alpha, stream);
                CopyParams p;
                p.in = s.g.a_const ? s.w0 : in0; p.out = out;
                for (int k = 0; k < 4; k++) { p.d[k] = s.g.d[k]; p.si[k] = s.g.sa[k]; p.so[k] = s.g.so[k]; }
                p.offi = s.g.offa; p.offo = s.g.offo;
                p.bsi = s.g.a_const ? 0 : (long)vals[s.in0].elems; p.bso = (long)vals[s.out].elems;
                launch_copy_view(p, n, stream);
                break;
            }
            case S_SOFTMAX:
                launch_softmax_rows(in0, out, (size_t)s.H * (size_t)n, s.C, s.g.alpha, stream);
                break;
            case S_REDUCE: {
                ReduceParams p{in0, out, {s.g.d[0], s.g.d[1], s.g.d[2], s.g.d[3]}, s.g.mask, s.op};
                launch_reduce(p, n, stream);
                break;
            }
            case S_CONV_GENERIC: {
                GenConvParams p{in0, s.w0, s.w1, out, n, s.H, s.W, s.C, s.Ho, s.Wo, s.Co, s.kh, s.kw, s.sh, s.sw, s.g.dh, s.g.dw,
                                s.pt, s.pl, s.act, s.g.depthwise, s.g.mult};
                launch_conv_generic(p, stream);
                break;
            }
        }
        if (prof_this) { hipEventRecord(pe.b, stream); prof.push_back(pe); }
        if (dbg_sync_after && (!strcmp(dbg_sync_after, s.kclass) || s.name.rfind(dbg_sync_after, 0) == 0)) hipStreamSynchronize(stream);
      }
    }
    for (int li = 0; li < nl; li++) {
        const Lane& L = lanes[li];
        if (L.d_emb && v_emb >= 0 && s_end == (int)steps.size()) {
            hipError_t e = hipMemcpyAsync(L.d_emb, vptr(v_emb, L.d_in, L.d_logits, L.d_emb, nl > 1 ? li : -1), (size_t)L.n * emb_dim * 4,
                                          hipMemcpyDeviceToDevice, L.st);
            if (e != hipSuccess) { *err = std::string("emb copy: ") + hipGetErrorString(e); mm_dirty = true; return false; }
        }
    }
    for (int li = 1; li < nl; li++) {
        hipEventRecord(ev_join[li - 1], lanes[li].st);
        hipStreamWaitEvent(main_stream, ev_join[li - 1], 0);
    }
    if (step_timing) { hipEventRecord(st_b, main_stream); step_ev.emplace_back(st_a, st_b); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { *err = std::string("kernel launch: ") + hipGetErrorString(e); mm_dirty = true; return false; }
    return true;
}

int Engine::steps_read(double* start_ms, double* end_ms, int cap) {
    sync_contexts();
    if (stream) hipStreamSynchronize(stream);
    const int n = (int)step_ev.size();
    for (int i = 0; i < n; i++) {
        float a = 0, b = 0;
        hipEventElapsedTime(&a, step_ev[0].first, step_ev[i].first);
        hipEventElapsedTime(&b, step_ev[0].first, step_ev[i].second);
        if (i < cap) { if (start_ms) start_ms[i] = a; if (end_ms) end_ms[i] = b; }
    }
    for (auto& p : step_ev) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    step_ev.clear();
    (void)hipGetLastError();
    return n;
}

// ================================================================================================ describe / profile
static void jesc(std::ostringstream& os, const std::string& s) {
    for (char c : s) { if (c == '"' || c == '\\') os << '\\'; os << c; }
}

// How a step reads in describe() and the profile when the full-batch tuning fuses a tail: the GEMM carries the work of both halves
// under a name that shows it ("b13/expand+dw", "top+mean") and the bytes it really moves - its own output stays in LDS -, the steps
// it absorbed carry none.
struct StepView { std::string name; double flops, bytes; bool absorbed; };
static StepView step_view(const Engine& e, size_t i) {
    const Step& s = e.steps[i];
    StepView v{s.name, s.flops, s.bytes, false};
    auto fused = [&](size_t k) { return e.steps[k].kind == S_PW && e.steps[k].tail && e.steps[k].wm_full >= 13; };
    if (fused(i)) {
        const double mine = 4.0 * s.H * s.W * s.Co;
        if (s.tail == 2) { v.name += "+dw"; v.flops += e.steps[i + 1].flops; }
        else { v.name += "+mean"; v.flops += e.steps[i + 1].flops + e.steps[i + 2].flops; v.bytes += 4.0 * s.Co - mine; }
    } else if ((s.kind == S_DW && i > 0 && e.steps[i - 1].tail == 2 && fused(i - 1)) ||
               (s.kind == S_MEAN_PARTIAL && i > 0 && e.steps[i - 1].tail == 1 && fused(i - 1)) ||
               (s.kind == S_MEAN_FINISH && i > 1 && e.steps[i - 2].tail == 1 && fused(i - 2))) {
        v.flops = 0; v.bytes = 0; v.absorbed = true;
    }
    return v;
}

std::string Engine::describe() const {
    std::ostringstream os;
    os << "{\"tune_source\":\"";
    jesc(os, tune_source);
    os << "\",\"tune_key\":\"" << (device >= 0 ? tune_key() : std::string()) << "\",\"split_step\":" << split_step << ",\"heatmap_tail\":\"" << (heatmap_pruned_step() >= 0 ? "pruned" : "gather") << "\",\"n_samples\":" << n_samples << ",\"n_classes\":" << n_classes << ",\"emb_dim\":" << emb_dim
       << ",\"max_batch\":" << max_batch << ",\"logits_output\":" << logits_output << ",\"embedding_output\":" << embedding_output << ",\"precision\":\"" << (precision ? "bf16" : "f32") << "\",\"lanes\":" << n_lanes << ",\"lane_min_batch\":" << dual_lane_min << ",\"act_arena_bytes\":" << act_bytes << ",\"weight_bytes\":" << w_bytes
       << ",\"specs\":[";
    for (size_t i = 0; i < specs.size(); i++) {
        const FrontSpec& f = specs[i];
        os << (i ? "," : "") << "{\"frame_length\":" << f.L << ",\"fft_length\":" << f.Lfft << ",\"hop\":" << f.hop
           << ",\"frames\":" << f.F << ",\"n_mels\":" << f.n_mels << ",\"channel\":" << f.c << ",\"p1\":" << f.p1
           << ",\"p2\":" << f.p2 << "}";
    }
    os << "],\"steps\":[";
    for (size_t i = 0; i < steps.size(); i++) {
        const Step& s = steps[i];
        const StepView sv = step_view(*this, i);
        const bool absorbed = sv.absorbed;
        os << (i ? "," : "") << "{\"i\":" << i << ",\"kernel\":\"" << s.kclass << "\",\"name\":\"";
        jesc(os, sv.name);
        os << "\",\"H\":" << s.H << ",\"W\":" << s.W << ",\"C\":" << s.C << ",\"Co\":" << s.Co << ",\"k\":" << s.kh
           << ",\"stride\":" << s.sh << ",\"act\":" << s.act << ",\"fused_scale\":" << (s.kind == S_PW && s.in1 >= 0 ? 1 : 0)
           << ",\"shape\":" << s.shape << ",\"dw_lds\":" << s.dwl << ",\"bx\":" << s.bx << ",\"nt\":" << s.nt << ",\"wm\":" << s.wm << ",\"nt_full\":" << s.nt_full << ",\"wm_full\":" << s.wm_full << ",\"fused_res\":" << (s.kind == S_PW && s.in2 >= 0 ? 1 : 0) << ",\"fused_sum\":" << (s.out2 >= 0 ? 1 : 0) << ",\"flops\":" << sv.flops << ",\"bytes\":" << sv.bytes << ",\"wbytes\":" << s.wbytes
           << ",\"tail\":" << s.tail << ",\"absorbed\":" << (absorbed ? 1 : 0) << ",\"out_v\":" << s.out << ",\"out2_v\":" << s.out2 << ",\"S\":" << s.S
           << ",\"in_bf16\":" << ((s.in0 >= 0 && vals[s.in0].half) ? 1 : 0) << ",\"out_bf16\":" << ((s.out >= 0 && vals[s.out].half) ? 1 : 0) << "}";
    }
    os << "]}";
    return os.str();
}

std::string Engine::profile_read() {
    hipStreamSynchronize(stream);
    struct Agg { double ms = 0, flops = 0, bytes = 0; long launches = 0; };
    std::map<std::string, Agg> agg;
    std::vector<std::string> order;
    std::vector<Agg> per_step(steps.size());
    for (auto& e : prof) {
        float ms = 0;
        hipEventElapsedTime(&ms, e.a, e.b);
        const Step& s = steps[e.step];
        const StepView sv = step_view(*this, e.step);
        if (!agg.count(s.kclass)) order.push_back(s.kclass);
        Agg& a = agg[s.kclass];
        a.ms += ms; a.launches++; a.flops += sv.flops * e.n; a.bytes += (sv.bytes + e.more_bytes) * e.n + s.wbytes;
        Agg& ps = per_step[e.step];
        ps.ms += ms; ps.launches++; ps.flops += sv.flops * e.n; ps.bytes += (sv.bytes + e.more_bytes) * e.n + s.wbytes;
        ev_pool.push_back(e.a); ev_pool.push_back(e.b);
    }
    prof.clear();
    std::ostringstream os;
    os << "[";
    for (size_t i = 0; i < order.size(); i++) {
        const Agg& a = agg[order[i]];
        os << (i ? "," : "") << "{\"kernel\":\"" << order[i] << "\",\"launches\":" << a.launches << ",\"ms\":" << a.ms
           << ",\"flops\":" << a.flops << ",\"bytes\":" << a.bytes << "}";
    }
    for (size_t i = 0; i < steps.size(); i++) {
        const Agg& a = per_step[i];
        if (!a.launches) continue;
        os << ",{\"step\":" << i << ",\"kernel\":\"" << steps[i].kclass << "\",\"name\":\"";
        jesc(os, step_view(*this, i).name);
        os << "\",\"launches\":" << a.launches << ",\"ms\":" << a.ms << ",\"flops\":" << a.flops << ",\"bytes\":" << a.bytes << "}";
    }
    os << "]";
    return os.str();
}

}  // namespace bnhip
