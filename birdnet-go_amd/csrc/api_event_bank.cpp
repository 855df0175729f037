// C ABI of the real-time detection-event bank (events_bank.h; include/bnhip.h, "Detection events: the real-time bank").
//
// Every call is one transaction in the discipline of stream_bank.h: one H2D copy of the call's header (the sources of the call,
// ascending, with their clocks and parities; the row map; for the host form the rows), the launches, one copy back (the count and the
// first events; a second copy only for an answer beyond EVB_FIRST_FETCH events), one synchronise, and a commit that runs only once
// everything succeeded - the host flips the parities and advances the clocks there, so a failed call changes no source.  The
// bank's frames are rows, not PCM, and a call's answer is counted on the device, so bank_call itself does not fit; its buffers
// (bank_grow) and its teardown (bank_free) do.
//
// A bank created with a dynamic (include/bnhip.h, "Detection events: dynamic thresholds") also keeps the per-class learning state, a
// pair of slabs with a parity of its own that the same commit flips; its call passes an EvdCall to the launches, and the first 16
// change records come down beside the head in the same copy, in the room of as many first events.  A bank created without one
// takes exactly the path it took before.
//
// Guards (include/bnhip.h, "Detection events: dog-bark and daylight filters") are a setting like the filter: their three class
// tables are a part of the bank's tables that exists from the first set_guards on, and the daylight spans of the call's sources
// ride behind the row map in the header copy - no launch and no copy is added, and a bank that never had guards set builds the
// header it built before.  A source's dog window lives in its slab, so the commit covers it; a source that may hold one stays
// live across a flush (its freed slab is written to the other parity), since a bark counts for events that open after it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "api_events.h"
#include "events_bank.h"
#include "stream_bank.h"

using namespace bnhip;

static_assert(BNHIP_EVENT_PENDING == EVENT_PENDING, "the status of events_bank.h");
static_assert(sizeof(EvbGroup) == 32, "a group header is 32 bytes");
static_assert(sizeof(bnhip_threshold_change) == 32 && sizeof(ThresholdChange) == 32, "a change record is 32 bytes");
static_assert(BNHIP_THRESHOLD_EXPIRY == EVD_EXPIRY && BNHIP_THRESHOLD_HIGH_CONFIDENCE == EVD_HIGH_CONFIDENCE, "the reasons of events_bank.h");

struct bnhip_event_bank {
    struct Source {
        int64_t clock = 0;              // windows given since creation or reset
        int parity = 0;                 // slab read by the next call
        bool live = false;              // the slab holds state (false: every slot free, no veto window, no dog window)
        bool dog = false;               // a call under guards with a dog table has written the slab: it may hold a dog window
    };
    std::mutex mu;                      // calls on one bank are serialised
    std::mutex tick_mu;                 // ... and so are the ticks that feed it: d_rows is theirs from the first chunk to the bank's call
    int device = 0, max_sources = 0, n_classes = 0, k = 0, hold = 0, slots = 0;
    float veto_thr = 0.0f;
    int min_count = 1, flags = 0;
    bool extended = false;              // created extended: the slots carry their deadlines, the tables a third part
    int longest_wait = 0;               // ... and W of the extend it was created with: what the slots were sized for
    EventExtend x{};                    // the extend's numbers in force (max_windows 0: sliding is off)
    bool dynamic = false;               // created with a dynamic: the class state exists, the tables carry class_dynamic as their last part
    bool learning = false;              // ... and a dynamic is in force (set_dynamic(NULL): false, thr_eff = base, the state frozen)
    float trigger = 0.0f, min_threshold = 0.0f;
    int64_t valid = 1, cooldown = 0;
    int64_t now = 0;                    // bank time of the calls that follow (set_now)
    int cls_parity = 0;                 // slab of the class state read by the next call
    char* d_dyn = nullptr;              // evd_area_bytes(n_classes)
    std::vector<bnhip_threshold_change> changes;   // the records of the last successful process / flush call
    bool guarded = false;               // guards are in force (set_guards)
    bool has_guards = false;            // ... or were once: the tables carry their three parts behind the others
    bool g_dog = false, g_dog_filtered = false, g_daylight = false;      // which of the three tables the guards in force have
    float dog_thr = 0.0f;
    int dog_remember = 0;
    std::vector<int32_t> day;           // [max_sources][8][2] daylight spans from the first set_daylight on; an unused span is 0, 0
    bool tables_dirty = true;           // h_tab is newer than d_tab: the next call's header copy takes it along
    std::vector<Source> src;
    hipStream_t stream = nullptr;       // the bank's own, made at the first call that needs it: a bank fed by the tick alone runs on
                                        // the model's stream and adds none to the few hardware queues a process has (hostpipe.cpp)
    int32_t* d_state = nullptr;         // [max_sources][2][evb_slab_ints(slots, extended)]
    char* h_tab = nullptr; char* d_tab = nullptr;                                 // class_threshold [n_classes] | class_veto [n_classes]
                                                                                  // | extended: class_extended [n_classes]
                                                                                  // | dynamic: class_dynamic [n_classes]
                                                                                  // | guards: class_dog, class_dog_filtered, class_daylight
    size_t guards_tab_off() const { return (size_t)n_classes * (5 + (extended ? 1 : 0) + (dynamic ? 1 : 0)); }
    size_t tab_bytes() const { return guards_tab_off() + (has_guards ? (size_t)n_classes * 3 : 0); }
    size_t dyn_tab_off() const { return (size_t)n_classes * (extended ? 6 : 5); }
    uint8_t* h_stage = nullptr; void* d_stage = nullptr; size_t stage_cap = 0;   // groups | row map | rows
    uint8_t* h_out = nullptr; void* d_out = nullptr; size_t out_cap = 0;         // count, overflow flag | events
    void* d_work = nullptr; size_t work_cap = 0;                                 // staged events | counts and bases
    void* d_rows = nullptr; size_t rows_cap = 0;                                 // the fused tick's rows: conf [n][k] | idx [n][k]
    ~bnhip_event_bank() {               // (bank_free has drained the stream)
        if (stream) hipStreamDestroy(stream);
        for (void* p : {(void*)d_state, (void*)d_tab, (void*)d_dyn, d_stage, d_out, d_work, d_rows}) if (p) hipFree(p);
        for (void* p : {(void*)h_tab, (void*)h_stage, (void*)h_out}) if (p) hipHostFree(p);
    }
};

namespace {

constexpr const char* WHAT = "event bank";
constexpr int EVB_MAX_CLASSES = 150 * 1024 / 4;   // what the LDS top-k holds (api_events.cpp)
constexpr size_t EVB_FIRST_FETCH = 127;           // events that come down with the count: 16 + 127 * 32 = 4080 bytes
constexpr size_t EVB_HEAD = 16;
constexpr int64_t EVD_MAX_SPAN = (int64_t)1 << 61, EVD_MAX_NOW = (int64_t)1 << 62;

int evb_fail(hipError_t he) {
    (void)hipGetLastError();
    return set_err(he == hipErrorOutOfMemory ? BNHIP_E_NOMEM : BNHIP_E_RUNTIME, std::string(WHAT) + ": " + hipGetErrorString(he));
}

void evb_take_filter(bnhip_event_bank* b, const bnhip_event_filter* f) {
    memcpy(b->h_tab, f->class_threshold, (size_t)b->n_classes * 4);
    uint8_t* veto = reinterpret_cast<uint8_t*>(b->h_tab) + (size_t)b->n_classes * 4;
    if (f->class_veto) memcpy(veto, f->class_veto, (size_t)b->n_classes);
    else memset(veto, 0, (size_t)b->n_classes);
    b->veto_thr = f->veto_threshold; b->min_count = f->min_count; b->flags = f->flags;
    b->tables_dirty = true;
}

// (an extended bank) x NULL: sliding off
void evb_take_extend(bnhip_event_bank* b, const bnhip_event_extend* x) {
    uint8_t* slide = reinterpret_cast<uint8_t*>(b->h_tab) + (size_t)b->n_classes * 5;
    if (x && x->class_extended) memcpy(slide, x->class_extended, (size_t)b->n_classes);
    else memset(slide, 1, (size_t)b->n_classes);
    b->x = x ? event_extend_numbers(x) : EventExtend{};
    b->tables_dirty = true;
}

// every refusal of a dynamic itself (d NULL: refused)
int evb_dynamic_check(const bnhip_event_dynamic* d) {
    if (!d) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (!(d->trigger >= 0.0f)) return set_err(BNHIP_E_INVALID, "the dynamic's trigger must be a number >= 0");
    if (!(d->min_threshold >= 0.0f)) return set_err(BNHIP_E_INVALID, "the dynamic's min_threshold must be a number >= 0");
    if (d->valid < 1 || d->valid > EVD_MAX_SPAN) return set_err(BNHIP_E_INVALID, "the dynamic's valid must be in [1, 2^61]");
    if (d->cooldown < 0 || d->cooldown > EVD_MAX_SPAN) return set_err(BNHIP_E_INVALID, "the dynamic's cooldown must be in [0, 2^61]");
    return BNHIP_OK;
}

// (a dynamic bank) d NULL: learning off
void evb_take_dynamic(bnhip_event_bank* b, const bnhip_event_dynamic* d) {
    uint8_t* dyn = reinterpret_cast<uint8_t*>(b->h_tab) + b->dyn_tab_off();
    if (d && d->class_dynamic) memcpy(dyn, d->class_dynamic, (size_t)b->n_classes);
    else memset(dyn, d ? 1 : 0, (size_t)b->n_classes);
    b->learning = d != nullptr;
    if (d) { b->trigger = d->trigger; b->min_threshold = d->min_threshold; b->valid = d->valid; b->cooldown = d->cooldown; }
    b->tables_dirty = true;
}

int evb_dynamic_bank_check(const bnhip_event_bank* b) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (!b->dynamic) return set_err(BNHIP_E_INVALID, "the event bank was created without a dynamic");
    return BNHIP_OK;
}

// the class state of the slab the next call reads, as one host copy (the bank is locked and idle: every call ends synchronised).
// A blocking copy on the default stream: a bank fed by the tick alone has no stream of its own and is to get none for this
// (hostpipe.cpp), so the copy also waits for the process's blocking streams - include/bnhip.h says so to the caller
int evb_state_get(bnhip_event_bank* b, std::vector<char>& h) {
    h.resize(evd_slab_bytes(b->n_classes));
    hipSetDevice(b->device);
    const hipError_t he = hipMemcpy(h.data(), b->d_dyn + (size_t)b->cls_parity * h.size(), h.size(), hipMemcpyDeviceToHost);
    return he == hipSuccess ? BNHIP_OK : evb_fail(he);
}
int evb_state_put(bnhip_event_bank* b, const std::vector<char>& h) {
    hipSetDevice(b->device);
    const hipError_t he = hipMemcpy(b->d_dyn + (size_t)b->cls_parity * h.size(), h.data(), h.size(), hipMemcpyHostToDevice);
    return he == hipSuccess ? BNHIP_OK : evb_fail(he);
}
void evb_state_initial(std::vector<char>& h, int n_classes, int c0, int c1) {
    const EvdSlab S = evd_slab(h.data(), n_classes, 0);
    for (int c = c0; c < c1; c++) { S.expires[c] = 0; S.learned_at[c] = -1; S.level[c] = 0; S.count[c] = 0; }
}

// the bank's own stream (the bank is locked); NULL with the error set
hipStream_t evb_stream(bnhip_event_bank* b) {
    if (b->stream) return b->stream;
    hipSetDevice(b->device);
    const hipError_t he = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (he != hipSuccess) { b->stream = nullptr; evb_fail(he); }
    return b->stream;
}

// One call (the bank is locked).  EVB_PROCESS: rows r = 0..n_rows-1 of sources[r]; conf / idx are host rows, or with on_device rows
// on the bank's device.  EVB_FLUSH / EVB_PENDING: the live slots of `one` (or of every source: -1).  The call runs on s, or with
// own_stream on the bank's own.
int evb_call(bnhip_event_bank* b, int mode, const int32_t* sources, int n_rows, const float* conf, const int32_t* idx, bool on_device, int one,
             bnhip_event* out, size_t cap, size_t* n_out, bool own_stream, hipStream_t s) {
    const int k = b->k;
    std::vector<EvbGroup> groups;
    std::vector<int32_t> rowmap;
    size_t stage_total = 0;
    auto add_group = [&](int source, int n_windows, uint32_t row_off) {
        const bnhip_event_bank::Source& S = b->src[(size_t)source];
        const size_t room = (S.live ? (size_t)b->slots : 0) + (size_t)n_windows * (size_t)k;      // the live events and those the call opens
        EvbGroup g{};
        g.source = source; g.clock = (int32_t)S.clock; g.n_windows = n_windows; g.row_off = row_off;
        g.stage_off = (uint32_t)stage_total; g.stage_cap = (uint32_t)room;
        g.rd_parity = S.live ? S.parity : -1;
        g.wr_parity = mode == EVB_PROCESS || (mode == EVB_FLUSH && S.dog) ? (S.parity ^ 1) : -1;
        groups.push_back(g);
        stage_total += room;
    };
    if (mode == EVB_PROCESS) {
        if (n_rows < 0) return set_err(BNHIP_E_INVALID, "n_rows is negative");
        if ((unsigned long long)n_rows * (unsigned long long)k >= EVENT_MAX_ROWS) return set_err(BNHIP_E_INVALID, "n_rows * k of 2^31 or more");
        if (n_rows > 0 && (!sources || !conf || !idx)) return set_err(BNHIP_E_INVALID, "NULL argument");
        std::vector<std::pair<int32_t, int32_t>> order;                   // (source, row) of the rows that count
        order.reserve((size_t)n_rows);
        for (int r = 0; r < n_rows; r++) {
            if (sources[r] < 0) continue;                                 // (a source that was reset under the tick)
            if (sources[r] >= b->max_sources)
                return set_err(BNHIP_E_INVALID, "row " + std::to_string(r) + ": no such event bank source: " + std::to_string(sources[r]));
            if (!on_device)
                for (int i = 0; i < k; i++)
                    if (idx[(size_t)r * k + i] >= b->n_classes)
                        return set_err(BNHIP_E_INVALID, "row " + std::to_string(r) + ": class_index outside the table");
            order.emplace_back(sources[r], r);
        }
        std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& c) { return a.first < c.first; });
        rowmap.resize(order.size());
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            while (j < order.size() && order[j].first == order[i].first) { rowmap[j] = order[j].second; j++; }
            if (b->src[(size_t)order[i].first].clock + (int64_t)(j - i) > (int64_t)INT32_MAX)
                return set_err(BNHIP_E_INVALID, "source " + std::to_string(order[i].first) + ": the clock would pass 2^31 - 1 windows (reset the source)");
            add_group(order[i].first, (int)(j - i), (uint32_t)i);
            i = j;
        }
    } else {
        if (one < -1 || one >= b->max_sources) return set_err(BNHIP_E_INVALID, "no such event bank source: " + std::to_string(one));
        for (int sn = one < 0 ? 0 : one; sn < (one < 0 ? b->max_sources : one + 1); sn++)
            if (b->src[(size_t)sn].live) add_group(sn, 0, 0);
    }
    // a dynamic bank's call applies its per-class steps also with no source in it
    const bool dyn = b->learning && mode != EVB_PENDING;
    if (groups.empty() && !dyn) {
        *n_out = 0;
        if (mode != EVB_PENDING) b->changes.clear();
        return BNHIP_OK;
    }

    // ---- stage
    hipSetDevice(b->device);
    if (own_stream && !(s = evb_stream(b))) return BNHIP_E_RUNTIME;
    const size_t G = groups.size(), row_vals = on_device || mode != EVB_PROCESS ? 0 : (size_t)n_rows * (size_t)k;
    const bool marks_dog = b->guarded && b->g_dog, daylight = b->guarded && b->g_daylight && !b->day.empty() && mode != EVB_PENDING;
    const size_t o_map = G * sizeof(EvbGroup), o_conf = o_map + rowmap.size() * 4, o_idx = o_conf + row_vals * 4;
    const size_t o_day = o_idx + row_vals * 4, day_bytes = daylight ? G * EVB_DAYLIGHT_SPANS * 8 : 0;     // the sources' spans, by group
    const size_t stage_bytes = o_day + day_bytes;
    const size_t out_room = std::min(cap, stage_total);
    const size_t o_ev = EVB_HEAD + (dyn ? (size_t)EVD_FIRST_CHANGES * sizeof(ThresholdChange) : 0);   // head | dyn: the first change records | events
    const size_t o_counts = stage_total * sizeof(Event);
    if (!bank_grow((void**)&b->h_stage, &b->d_stage, &b->stage_cap, stage_bytes) ||
        !bank_grow((void**)&b->h_out, &b->d_out, &b->out_cap, o_ev + std::max<size_t>(out_room, 1) * sizeof(Event)))
        return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + WHAT + " staging)");
    if (b->work_cap < o_counts + 2 * G * 4) {
        const size_t want = o_counts + 2 * G * 4, c = std::max<size_t>(want + want / 2, 1 << 16);
        void* nd = nullptr;
        if (hipMalloc(&nd, c) != hipSuccess) { (void)hipGetLastError(); return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + WHAT + " work area)"); }
        if (b->d_work) hipFree(b->d_work);
        b->d_work = nd; b->work_cap = c;
    }
    if (o_map) memcpy(b->h_stage, groups.data(), o_map);
    if (!rowmap.empty()) memcpy(b->h_stage + o_map, rowmap.data(), rowmap.size() * 4);
    if (row_vals) {
        memcpy(b->h_stage + o_conf, conf, row_vals * 4);
        memcpy(b->h_stage + o_idx, idx, row_vals * 4);
    }
    for (size_t gi = 0; day_bytes && gi < G; gi++)
        memcpy(b->h_stage + o_day + gi * EVB_DAYLIGHT_SPANS * 8, b->day.data() + (size_t)groups[gi].source * EVB_DAYLIGHT_SPANS * 2,
               EVB_DAYLIGHT_SPANS * 8);
    hipError_t he = hipSuccess;
    if (b->tables_dirty) he = hipMemcpyAsync(b->d_tab, b->h_tab, b->tab_bytes(), hipMemcpyHostToDevice, s);
    if (he == hipSuccess && stage_bytes) he = hipMemcpyAsync(b->d_stage, b->h_stage, stage_bytes, hipMemcpyHostToDevice, s);
    if (he != hipSuccess) { hipStreamSynchronize(s); return evb_fail(he); }

    // ---- run
    const char* ds = static_cast<const char*>(b->d_stage);
    char* dw = static_cast<char*>(b->d_work);
    char* dout = static_cast<char*>(b->d_out);
    EvbCall c{};
    c.groups = reinterpret_cast<const EvbGroup*>(ds); c.n_groups = (int)G;
    c.rowmap = reinterpret_cast<const int32_t*>(ds + o_map);
    c.conf = row_vals ? reinterpret_cast<const float*>(ds + o_conf) : conf;
    c.idx = row_vals ? reinterpret_cast<const int32_t*>(ds + o_idx) : idx;
    c.k = k; c.slots = b->slots; c.mode = mode; c.extended = b->extended;
    c.day = day_bytes ? reinterpret_cast<const int32_t*>(ds + o_day) : nullptr;
    c.state = b->d_state;
    c.stage = reinterpret_cast<Event*>(dw);
    c.counts = reinterpret_cast<uint32_t*>(dw + o_counts);
    c.head = reinterpret_cast<unsigned long long*>(dout);
    c.out = reinterpret_cast<Event*>(dout + o_ev);
    c.out_cap = out_room;
    EventFilterDev fd{reinterpret_cast<const float*>(b->d_tab), reinterpret_cast<const uint8_t*>(b->d_tab) + (size_t)b->n_classes * 4,
                      b->veto_thr, b->hold, b->min_count, b->flags, b->n_classes};
    if (b->extended) { fd.slide = reinterpret_cast<const uint8_t*>(b->d_tab) + (size_t)b->n_classes * 5; fd.x = b->x; }
    if (b->guarded) {
        const uint8_t* gt = reinterpret_cast<const uint8_t*>(b->d_tab) + b->guards_tab_off();
        const size_t n = (size_t)b->n_classes;
        fd.g.dog = b->g_dog ? gt : nullptr; fd.g.dog_filtered = b->g_dog_filtered ? gt + n : nullptr;
        fd.g.daylight = b->g_daylight ? gt + 2 * n : nullptr;
        fd.g.dog_thr = b->dog_thr; fd.g.dog_remember = b->dog_remember;
    }
    if (dyn) {
        EvdCall d{};
        d.area = b->d_dyn; d.rd_parity = b->cls_parity; d.base = fd.thr;
        d.dynamic = reinterpret_cast<const uint8_t*>(b->d_tab) + b->dyn_tab_off();
        d.n_rows = (uint32_t)rowmap.size();
        d.now = b->now; d.valid = b->valid; d.cooldown = b->cooldown; d.trigger = b->trigger; d.min_threshold = b->min_threshold;
        d.first = reinterpret_cast<ThresholdChange*>(dout + EVB_HEAD);
        d.n_classes = b->n_classes;
        fd.thr = d.thr_eff();
        launch_event_bank(c, fd, s, &d);
    } else {
        launch_event_bank(c, fd, s);
    }
    he = hipGetLastError();
    // (the first change records take their room from the first events: the copy is 4080 bytes either way)
    const size_t first_n = std::min(out_room, EVB_FIRST_FETCH - (dyn ? (size_t)EVD_FIRST_CHANGES : 0));
    if (he == hipSuccess) he = hipMemcpyAsync(b->h_out, b->d_out, o_ev + first_n * sizeof(Event), hipMemcpyDeviceToHost, s);
    const hipError_t hs = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hs;
    if (he != hipSuccess) return evb_fail(he);
    unsigned long long head[2];
    memcpy(head, b->h_out, sizeof head);
    if (head[1] & 0xffffffffull) return set_err(BNHIP_E_RUNTIME, std::string(WHAT) + ": a source ran out of slots");
    const size_t n_changes = dyn ? (size_t)(head[1] >> 32) : 0;                     // (k_evd_apply counts them there)
    const size_t total = (size_t)head[0];
    if (total > cap) {
        *n_out = total;
        return set_err(BNHIP_E_INVALID, "event buffer too small: the call answers " + std::to_string(total) + " events");
    }
    std::vector<bnhip_threshold_change> changes(n_changes);
    if (total > first_n || n_changes > (size_t)EVD_FIRST_CHANGES) {
        he = hipSuccess;
        if (total > first_n)
            he = hipMemcpyAsync(b->h_out + o_ev + first_n * sizeof(Event), dout + o_ev + first_n * sizeof(Event), (total - first_n) * sizeof(Event),
                                hipMemcpyDeviceToHost, s);
        if (he == hipSuccess && n_changes > (size_t)EVD_FIRST_CHANGES) {
            EvdCall d{};
            d.area = b->d_dyn; d.n_classes = b->n_classes;
            he = hipMemcpyAsync(changes.data(), d.records(), n_changes * sizeof(ThresholdChange), hipMemcpyDeviceToHost, s);
        }
        const hipError_t hs2 = hipStreamSynchronize(s);
        if (he == hipSuccess) he = hs2;
        if (he != hipSuccess) return evb_fail(he);
    }
    if (n_changes && n_changes <= (size_t)EVD_FIRST_CHANGES) memcpy(changes.data(), b->h_out + EVB_HEAD, n_changes * sizeof(ThresholdChange));
    if (total) memcpy(out, b->h_out + o_ev, total * sizeof(Event));
    *n_out = total;

    // ---- commit: everything above succeeded
    b->tables_dirty = false;
    if (mode == EVB_PENDING) return BNHIP_OK;
    b->changes.swap(changes);
    if (dyn) b->cls_parity ^= 1;
    for (const EvbGroup& g : groups) {
        bnhip_event_bank::Source& S = b->src[(size_t)g.source];
        if (mode == EVB_FLUSH) {
            if (g.wr_parity >= 0) S.parity ^= 1;                         // (the freed slab keeps the dog window)
            else S.live = false;                                         // (no slot is live any more, and the veto windows lie behind the clock)
            continue;
        }
        S.parity ^= 1;
        S.live = true;
        S.dog = S.dog || marks_dog;
        S.clock += g.n_windows;
    }
    return BNHIP_OK;
}

// what create and set_filter refuse of the filter and the bank's shape together
int evb_shape_check(const bnhip_event_filter* f, int k) {
    if (int rc = event_filter_check(f)) return rc;
    if (k < 1) return set_err(BNHIP_E_INVALID, "k must be at least 1");
    if ((long long)k * f->hold_windows > EVB_MAX_SLOTS) return set_err(BNHIP_E_INVALID, "k * hold_windows must be at most 4096");
    return BNHIP_OK;
}

// create, with or without an extend
int evb_create(int device, int max_sources, int n_classes, int k, const bnhip_event_filter* filter, bool extended, const bnhip_event_extend* extend,
               bnhip_event_bank** out, bool dynamic = false, const bnhip_event_dynamic* dyn = nullptr) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = evb_shape_check(filter, k)) return rc;
    if (extended) if (int rc = event_extend_check(filter->hold_windows, extend, k)) return rc;
    if (dynamic) if (int rc = evb_dynamic_check(dyn)) return rc;
    if (max_sources < 1 || max_sources > 65535) return set_err(BNHIP_E_INVALID, "max_sources must be in [1, 65535]");
    if (n_classes < 1 || n_classes > EVB_MAX_CLASSES) return set_err(BNHIP_E_INVALID, "n_classes must be in [1, 38400]");
    bnhip_event_bank* b = nullptr;
    BN_GUARD_BEGIN
    if (int rc = use_device(device)) return rc;
    b = new bnhip_event_bank();
    b->device = device; b->max_sources = max_sources; b->n_classes = n_classes; b->k = k; b->hold = filter->hold_windows;
    b->extended = extended; b->dynamic = dynamic;
    b->longest_wait = extended ? ev_longest_wait(b->hold, event_extend_numbers(extend)) : b->hold;
    b->slots = std::min(k * b->longest_wait, n_classes);
    b->src.resize((size_t)max_sources);
    hipError_t he = hipMalloc((void**)&b->d_state, (size_t)max_sources * 2 * evb_slab_ints(b->slots, extended) * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&b->d_tab, b->tab_bytes());
    if (he == hipSuccess) he = hipHostMalloc((void**)&b->h_tab, b->tab_bytes(), hipHostMallocPortable);
    if (he == hipSuccess && dynamic) {
        he = hipMalloc((void**)&b->d_dyn, evd_area_bytes(n_classes));
        std::vector<char> h(evd_slab_bytes(n_classes));
        evb_state_initial(h, n_classes, 0, n_classes);
        if (he == hipSuccess) he = hipMemcpy(b->d_dyn, h.data(), h.size(), hipMemcpyHostToDevice);
    }
    if (he != hipSuccess) {
        (void)hipGetLastError();
        bank_free(b); b = nullptr;
        return set_err(he == hipErrorOutOfMemory ? BNHIP_E_NOMEM : BNHIP_E_RUNTIME, std::string(WHAT) + " create: " + hipGetErrorString(he));
    }
    evb_take_filter(b, filter);
    if (extended) evb_take_extend(b, extend);
    if (dynamic) evb_take_dynamic(b, dyn);
    *out = b;
    return BNHIP_OK;
    BN_GUARD_END(bank_free(b))
}

int evb_answer_check(const bnhip_event_bank* b, const bnhip_event* out, size_t cap, const size_t* n_out) {
    if (!b || !n_out || (cap && !out)) return set_err(BNHIP_E_INVALID, "NULL argument");
    return BNHIP_OK;
}

}  // namespace

namespace bnhip {
int event_bank_device(const bnhip_event_bank* b) { return b->device; }
int event_bank_k(const bnhip_event_bank* b) { return b->k; }
std::mutex& event_bank_tick_mutex(bnhip_event_bank* b) { return b->tick_mu; }
int event_bank_rows(bnhip_event_bank* b, size_t n_rows, float** d_conf, int32_t** d_idx) {
    std::lock_guard<std::mutex> lk(b->mu);
    const size_t half = (n_rows * (size_t)b->k * 4 + 255) / 256 * 256;
    if (b->rows_cap < 2 * half) {
        hipSetDevice(b->device);
        void* nd = nullptr;
        if (hipMalloc(&nd, 2 * half) != hipSuccess) { (void)hipGetLastError(); return set_err(BNHIP_E_NOMEM, "allocation failed (event bank rows)"); }
        if (b->d_rows) hipFree(b->d_rows);
        b->d_rows = nd; b->rows_cap = 2 * half;
    }
    *d_conf = static_cast<float*>(b->d_rows);
    *d_idx = reinterpret_cast<int32_t*>(static_cast<char*>(b->d_rows) + half);
    return BNHIP_OK;
}
}  // namespace bnhip

extern "C" {

int bnhip_event_bank_create(int device, int max_sources, int n_classes, int k, const bnhip_event_filter* filter, bnhip_event_bank** out) {
    return evb_create(device, max_sources, n_classes, k, filter, false, nullptr, out);
}

int bnhip_event_bank_create_extended(int device, int max_sources, int n_classes, int k, const bnhip_event_filter* filter,
                                     const bnhip_event_extend* extend, bnhip_event_bank** out) {
    return evb_create(device, max_sources, n_classes, k, filter, true, extend, out);
}

int bnhip_event_bank_create_dynamic(int device, int max_sources, int n_classes, int k, const bnhip_event_filter* filter,
                                    const bnhip_event_extend* extend, const bnhip_event_dynamic* dynamic, bnhip_event_bank** out) {
    return evb_create(device, max_sources, n_classes, k, filter, extend != nullptr, extend, out, true, dynamic);
}

int bnhip_event_bank_set_dynamic(bnhip_event_bank* b, const bnhip_event_dynamic* dynamic) {
    if (int rc = evb_dynamic_bank_check(b)) return rc;
    if (dynamic) if (int rc = evb_dynamic_check(dynamic)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    evb_take_dynamic(b, dynamic);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_set_now(bnhip_event_bank* b, int64_t now) {
    if (int rc = evb_dynamic_bank_check(b)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (now < 0 || now >= EVD_MAX_NOW) return set_err(BNHIP_E_INVALID, "now must be in [0, 2^62)");
    if (now < b->now) return set_err(BNHIP_E_INVALID, "bank time never decreases: " + std::to_string(now) + " after " + std::to_string(b->now));
    b->now = now;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_threshold_changes(bnhip_event_bank* b, bnhip_threshold_change* out, size_t cap, size_t* n_out) {
    if (int rc = evb_dynamic_bank_check(b)) return rc;
    if (!n_out || (cap && !out)) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    *n_out = b->changes.size();
    if (b->changes.size() > cap) return set_err(BNHIP_E_INVALID, "change buffer too small: the call left " + std::to_string(b->changes.size()) + " records");
    if (!b->changes.empty()) memcpy(out, b->changes.data(), b->changes.size() * sizeof(bnhip_threshold_change));
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_thresholds(bnhip_event_bank* b, int32_t* level, int32_t* high_count, int64_t* expires, int64_t* learned_at, float* current) {
    if (int rc = evb_dynamic_bank_check(b)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    std::vector<char> h;
    if (int rc = evb_state_get(b, h)) return rc;
    const EvdSlab S = evd_slab(h.data(), b->n_classes, 0);
    const float* base = reinterpret_cast<const float*>(b->h_tab);
    const uint8_t* dyn = reinterpret_cast<const uint8_t*>(b->h_tab) + b->dyn_tab_off();
    for (int c = 0; c < b->n_classes; c++) {
        if (level) level[c] = S.level[c];
        if (high_count) high_count[c] = S.count[c];
        if (expires) expires[c] = S.expires[c];
        if (learned_at) learned_at[c] = S.learned_at[c];
        if (current) current[c] = dyn[c] ? ev_threshold(base[c], S.level[c], b->min_threshold) : base[c];
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_set_thresholds(bnhip_event_bank* b, const int32_t* level, const int32_t* high_count, const int64_t* expires,
                                    const int64_t* learned_at) {
    if (int rc = evb_dynamic_bank_check(b)) return rc;
    if (!level || !high_count || !expires || !learned_at) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    for (int c = 0; c < b->n_classes; c++)
        if (level[c] < 0 || level[c] > 3 || high_count[c] < 0 || level[c] != std::min(high_count[c], 3) || learned_at[c] < -1 || expires[c] < 0)
            return set_err(BNHIP_E_INVALID, "class " + std::to_string(c) + ": not a threshold state (0 <= level = min(high_count, 3) <= 3, learned_at >= -1, expires >= 0)");
    std::vector<char> h(evd_slab_bytes(b->n_classes));
    const EvdSlab S = evd_slab(h.data(), b->n_classes, 0);
    for (int c = 0; c < b->n_classes; c++) { S.level[c] = level[c]; S.count[c] = high_count[c]; S.expires[c] = expires[c]; S.learned_at[c] = learned_at[c]; }
    return evb_state_put(b, h);
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_reset_thresholds(bnhip_event_bank* b, int class_index) {
    if (int rc = evb_dynamic_bank_check(b)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (class_index < -1 || class_index >= b->n_classes) return set_err(BNHIP_E_INVALID, "no such class: " + std::to_string(class_index));
    std::vector<char> h(evd_slab_bytes(b->n_classes));
    if (class_index >= 0) if (int rc = evb_state_get(b, h)) return rc;
    evb_state_initial(h, b->n_classes, class_index < 0 ? 0 : class_index, class_index < 0 ? b->n_classes : class_index + 1);
    return evb_state_put(b, h);
    BN_GUARD_END((void)0)
}

float bnhip_event_threshold(float base, int level, float min_threshold) {
    if (level < 0 || level > 3) { set_err(BNHIP_E_INVALID, "level must be in [0, 3]"); return std::nanf(""); }
    return ev_threshold(base, level, min_threshold);
}

int bnhip_event_bank_info(const bnhip_event_bank* b, int* max_sources, int* n_classes, int* k, int* hold_windows, int* slots_per_source) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (max_sources) *max_sources = b->max_sources;
    if (n_classes) *n_classes = b->n_classes;
    if (k) *k = b->k;
    if (hold_windows) *hold_windows = b->hold;
    if (slots_per_source) *slots_per_source = b->slots;
    return BNHIP_OK;
}

int bnhip_event_bank_set_filter(bnhip_event_bank* b, const bnhip_event_filter* filter) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = event_filter_check(filter)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (filter->hold_windows != b->hold)
        return set_err(BNHIP_E_INVALID, "hold_windows is fixed for the bank's life: " + std::to_string(b->hold) + ", not " + std::to_string(filter->hold_windows));
    evb_take_filter(b, filter);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_set_guards(bnhip_event_bank* b, const bnhip_event_guards* guards) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (guards) if (int rc = event_guards_check(guards)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (!guards) { b->guarded = false; return BNHIP_OK; }
    const size_t n = (size_t)b->n_classes;
    if (!b->has_guards) {               // the tables grow by the guards' three parts, once (the bank is idle: every call ends synchronised)
        hipSetDevice(b->device);
        const size_t bytes = b->guards_tab_off() + n * 3;
        char* nh = nullptr; char* nd = nullptr;
        hipError_t he = hipHostMalloc((void**)&nh, bytes, hipHostMallocPortable);
        if (he == hipSuccess) he = hipMalloc((void**)&nd, bytes);
        if (he != hipSuccess) {
            if (nh) hipHostFree(nh);
            (void)hipGetLastError();
            return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + WHAT + " guards)");
        }
        memcpy(nh, b->h_tab, b->guards_tab_off());
        hipHostFree(b->h_tab); hipFree(b->d_tab);
        b->h_tab = nh; b->d_tab = nd;
        b->has_guards = true;
    }
    uint8_t* gt = reinterpret_cast<uint8_t*>(b->h_tab) + b->guards_tab_off();
    const uint8_t* tables[3] = {guards->class_dog, guards->class_dog_filtered, guards->class_daylight};
    for (int t = 0; t < 3; t++) {
        if (tables[t]) memcpy(gt + n * t, tables[t], n);
        else memset(gt + n * t, 0, n);
    }
    b->g_dog = guards->class_dog != nullptr; b->g_dog_filtered = guards->class_dog_filtered != nullptr;
    b->g_daylight = guards->class_daylight != nullptr;
    b->dog_thr = guards->dog_threshold; b->dog_remember = guards->dog_remember_windows;
    b->guarded = true;
    b->tables_dirty = true;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_set_daylight(bnhip_event_bank* b, int source, const int32_t* spans, int n) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n < 0 || n > EVB_DAYLIGHT_SPANS) return set_err(BNHIP_E_INVALID, "a source takes 0 to 8 daylight spans");
    if (n > 0 && !spans) return set_err(BNHIP_E_INVALID, "NULL argument");
    for (int i = 0; i < n; i++) {
        if (spans[2 * i] < 0 || spans[2 * i + 1] <= spans[2 * i])
            return set_err(BNHIP_E_INVALID, "daylight span " + std::to_string(i) + ": needs 0 <= from < to");
        if (i && spans[2 * i] < spans[2 * i - 1])
            return set_err(BNHIP_E_INVALID, "daylight span " + std::to_string(i) + ": spans must ascend and not overlap");
    }
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (source < -1 || source >= b->max_sources) return set_err(BNHIP_E_INVALID, "no such event bank source: " + std::to_string(source));
    if (source < 0 && n != 0) return set_err(BNHIP_E_INVALID, "source -1 only clears: n must be 0");
    if (source < 0) { std::fill(b->day.begin(), b->day.end(), 0); return BNHIP_OK; }
    if (b->day.empty()) {
        if (n == 0) return BNHIP_OK;
        b->day.assign((size_t)b->max_sources * EVB_DAYLIGHT_SPANS * 2, 0);
    }
    int32_t* at = b->day.data() + (size_t)source * EVB_DAYLIGHT_SPANS * 2;
    std::fill_n(at, EVB_DAYLIGHT_SPANS * 2, 0);
    if (n) memcpy(at, spans, (size_t)n * 8);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_set_extend(bnhip_event_bank* b, const bnhip_event_extend* extend) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (!b->extended) return set_err(BNHIP_E_INVALID, "the event bank was created without an extend");
    if (extend) {
        if (int rc = event_extend_check(b->hold, extend)) return rc;
        const int W = ev_longest_wait(b->hold, event_extend_numbers(extend));
        if (W > b->longest_wait)
            return set_err(BNHIP_E_INVALID, "the longest wait is fixed for the bank's life: at most " + std::to_string(b->longest_wait) + ", not " + std::to_string(W));
    }
    evb_take_extend(b, extend);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_process(bnhip_event_bank* b, const int32_t* sources, int n_rows, const float* conf, const int32_t* idx, bnhip_event* out,
                             size_t cap, size_t* n_out) {
    if (int rc = evb_answer_check(b, out, cap, n_out)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    return evb_call(b, EVB_PROCESS, sources, n_rows, conf, idx, false, -1, out, cap, n_out, true, nullptr);
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_process_device(bnhip_event_bank* b, const int32_t* sources, int n_rows, const float* d_conf, const int32_t* d_idx,
                                    bnhip_event* out, size_t cap, size_t* n_out, void* stream) {
    if (int rc = evb_answer_check(b, out, cap, n_out)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    return evb_call(b, EVB_PROCESS, sources, n_rows, d_conf, d_idx, true, -1, out, cap, n_out, false, static_cast<hipStream_t>(stream));
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_flush(bnhip_event_bank* b, int source, bnhip_event* out, size_t cap, size_t* n_out) {
    if (int rc = evb_answer_check(b, out, cap, n_out)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    return evb_call(b, EVB_FLUSH, nullptr, 0, nullptr, nullptr, false, source, out, cap, n_out, true, nullptr);
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_pending(bnhip_event_bank* b, bnhip_event* out, size_t cap, size_t* n_out) {
    if (int rc = evb_answer_check(b, out, cap, n_out)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    return evb_call(b, EVB_PENDING, nullptr, 0, nullptr, nullptr, false, -1, out, cap, n_out, true, nullptr);
    BN_GUARD_END((void)0)
}

// host only: a source without state reads as "every slot free, no veto window"
int bnhip_event_bank_reset(bnhip_event_bank* b, int source) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (source < -1 || source >= b->max_sources) return set_err(BNHIP_E_INVALID, "no such event bank source: " + std::to_string(source));
    for (int sn = source < 0 ? 0 : source; sn < (source < 0 ? b->max_sources : source + 1); sn++) {
        b->src[(size_t)sn].live = false;
        b->src[(size_t)sn].dog = false;
        b->src[(size_t)sn].clock = 0;
        if (!b->day.empty()) std::fill_n(b->day.begin() + (size_t)sn * EVB_DAYLIGHT_SPANS * 2, EVB_DAYLIGHT_SPANS * 2, 0);
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_event_bank_clock(bnhip_event_bank* b, int source, int64_t* windows) {
    if (!b || !windows) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (source < 0 || source >= b->max_sources) return set_err(BNHIP_E_INVALID, "no such event bank source: " + std::to_string(source));
    *windows = b->src[(size_t)source].clock;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

void bnhip_event_bank_destroy(bnhip_event_bank* b) {
    try { bank_free(b); } catch (...) {}
}

}  // extern "C"
