// The streaming detection-event rule on the device (events_bank.h).
//
// k_evb_update  one wave per source of the call.  The source's slots come into LDS (lanes take slots 64 at a step), the wave walks the
//               source's windows of this call in order - per result a ballot on class over the live slots, the matching lane joins or
//               the lowest free slot opens; the veto window and under guards the dog window rise; the slots that are due are staged,
//               their status final (minimum count, veto, and under guards recent dog bark and daylight), and freed -
//               and the slots go out to the slab of the other parity.  Flush ("every live slot is due") and pending ("stage without
//               freeing") are modes of the same walk.
// k_evb_scan    one block: the exclusive scan of the sources' answered counts, sources ascending, and their total.
// k_evb_emit    one block per source: a staged event's rank is the number of the source's staged events with a smaller (class, first
//               window), counted against keys in LDS; it lands at base + rank.
// Integer work bound by latency: plain loads and stores, compares, ballots; nothing is accumulated in floating point.
#include "events_bank.h"

#include <climits>

#include "block_scan.h"
#include "kernels.h"

namespace bnhip {

namespace {

using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int EVB_KEY_TILE = 1024;

// a deadline as a slot stores it: no clock passes 2^31 - 1 windows, so a later one is never reached either way
__device__ __forceinline__ int evb_due(long long d) { return (int)min(d, (long long)INT_MAX); }

// EXT: the bank was created extended - a slot carries its deadline (the seventh array, behind the other six in LDS and in the slab),
// set when the slot opens and rewritten by every hit of a sliding class (ev_deadline).  Without it the deadline is first + hold
// and nothing is stored.
template <bool EXT>
__global__ __launch_bounds__(64) void k_evb_update(EvbCall c, EventFilterDev f) {
    extern __shared__ int evb_sm[];
    const int S = c.slots, lane = threadIdx.x;
    constexpr int A = EXT ? 7 : 6;
    int* cls = evb_sm;
    int* first = evb_sm + S;
    int* last = evb_sm + 2 * S;
    int* best = evb_sm + 3 * S;
    int* count = evb_sm + 4 * S;
    float* conf = reinterpret_cast<float*>(evb_sm + 5 * S);
    int* deadline = evb_sm + 6 * S;                // (EXT only)
    const EvbGroup g = c.groups[blockIdx.x];
    const size_t slab = (size_t)S * A + 4;
    const int* rd = g.rd_parity >= 0 ? c.state + ((size_t)g.source * 2 + (size_t)g.rd_parity) * slab : nullptr;
    int* wr = g.wr_parity >= 0 ? c.state + ((size_t)g.source * 2 + (size_t)g.wr_parity) * slab : nullptr;
    for (int s = lane; s < S; s += 64) {
        cls[s] = rd ? rd[s] : -1;
        first[s] = rd ? rd[S + s] : 0;
        last[s] = rd ? rd[2 * S + s] : 0;
        best[s] = rd ? rd[3 * S + s] : 0;
        count[s] = rd ? rd[4 * S + s] : 0;
        conf[s] = rd ? __int_as_float(rd[5 * S + s]) : 0.0f;
        if (EXT) deadline[s] = rd ? rd[6 * S + s] : 0;
    }
    int veto_win = rd ? rd[A * S] : -1;            // the source's largest veto-hit window so far
    int dog_win = rd ? rd[A * S + 1] : -1;         // ... and its largest dog-hit window
    const int32_t* day = c.day ? c.day + (size_t)blockIdx.x * (EVB_DAYLIGHT_SPANS * 2) : nullptr;
    __syncthreads();
    const u64 lt = (1ull << lane) - 1ull;
    u32 staged = 0;
    bool overflow = false;
    Event* stage = c.stage + g.stage_off;

    // the live slots that are due after window w (every live slot in the flush and pending modes): staged in slot order, freed
    // unless the call only looks
    auto stage_due = [&](long long w) {
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const bool live = s < S && cls[s] >= 0;
            const bool due = live && (c.mode != EVB_PROCESS || (EXT ? (long long)deadline[s] : (long long)first[s] + f.hold) <= w + 1);
            int status = EVENT_PENDING;
            if (due && c.mode != EVB_PENDING) {
                status = count[s] < f.min_count ? EVENT_FEW : veto_win >= first[s] ? EVENT_VETOED : EVENT_KEPT;
                // the guards measure from the event's final deadline, which an early flush has not reached yet
                if (status == EVENT_KEPT && f.g.dog_drops(cls[s], EXT ? (long long)deadline[s] : (long long)first[s] + f.hold, dog_win))
                    status = EVENT_DOG;
                if (status == EVENT_KEPT && day && f.g.daylight[cls[s]] != 0)
                    for (int q = 0; q < EVB_DAYLIGHT_SPANS; q++)
                        if (day[2 * q] <= first[s] && first[s] < day[2 * q + 1]) status = EVENT_DAYLIGHT;
            }
            const bool answered = due && (c.mode == EVB_PENDING || status == EVENT_KEPT || (f.flags & EVENTS_KEEP_DROPPED));
            const u64 m = __ballot(answered);
            const u32 pos = staged + (u32)__popcll(m & lt);
            if (answered) {
                if (pos < g.stage_cap) {
                    Event e;
                    e.recording = g.source; e.cls = cls[s]; e.first_window = first[s]; e.last_window = last[s];
                    e.best_window = best[s]; e.count = count[s]; e.confidence = conf[s]; e.status = status;
                    stage[pos] = e;
                } else {
                    overflow = true;
                }
            }
            if (due && c.mode != EVB_PENDING) cls[s] = -1;
            staged += (u32)__popcll(m);
        }
        __syncthreads();
    };

    if (c.mode != EVB_PROCESS) {
        stage_due(0);
    } else {
        for (int j = 0; j < g.n_windows; j++) {
            const size_t row = (size_t)c.rowmap[g.row_off + j] * (size_t)c.k;
            const int w = g.clock + j;
            for (int i = 0; i < c.k; i++) {
                const float x = c.conf[row + i];
                const int ci = c.idx[row + i];
                if ((u32)ci >= (u32)f.n_classes) continue;             // no result
                if (f.g.dog_hit(ci, x)) dog_win = w;                   // (whatever else the result is)
                if (f.veto[ci] != 0) {
                    if (x > f.veto_thr) veto_win = w;
                    continue;
                }
                if (!(x > f.thr[ci])) continue;                        // float32, strict, false for a NaN on either side
                const bool slides = EXT && f.slides(ci);
                bool placed = false;
                for (int s0 = 0; s0 < S && !placed; s0 += 64) {        // at most one live slot holds the class
                    const int s = s0 + lane;
                    const bool mine = s < S && cls[s] == ci;
                    if (__ballot(mine) == 0) continue;
                    if (mine) {
                        last[s] = w;
                        count[s] += 1;
                        if (x > conf[s]) { conf[s] = x; best[s] = w; }  // (ties: the earliest stays)
                        if (slides) deadline[s] = evb_due(ev_deadline(first[s], w, f.hold, f.x));
                    }
                    placed = true;
                }
                for (int s0 = 0; s0 < S && !placed; s0 += 64) {        // the lowest free slot opens the event
                    const int s = s0 + lane;
                    const u64 free_m = __ballot(s < S && cls[s] < 0);
                    if (free_m == 0) continue;
                    if (lane == __ffsll((long long)free_m) - 1) {
                        cls[s] = ci; first[s] = w; last[s] = w; best[s] = w; count[s] = 1; conf[s] = x;
                        if (EXT) deadline[s] = evb_due(slides ? ev_deadline(w, w, f.hold, f.x) : (long long)w + f.hold);
                    }
                    placed = true;
                }
                if (!placed) overflow = true;                          // (never: slots = min(k * hold or k * W, n_classes) is exact)
                __syncthreads();
            }
            stage_due(w);
        }
        for (int s = lane; s < S; s += 64) {
            wr[s] = cls[s];
            wr[S + s] = first[s];
            wr[2 * S + s] = last[s];
            wr[3 * S + s] = best[s];
            wr[4 * S + s] = count[s];
            wr[5 * S + s] = __float_as_int(conf[s]);
            if (EXT) wr[6 * S + s] = deadline[s];
        }
        if (lane == 0) { wr[A * S] = veto_win; wr[A * S + 1] = dog_win; }
    }
    if (c.mode == EVB_FLUSH && wr) {
        // a source that keeps a dog window stays live across its flush: every slot free, the two windows as they stand
        for (int s = lane; s < S; s += 64) wr[s] = -1;
        if (lane == 0) { wr[A * S] = veto_win; wr[A * S + 1] = dog_win; }
    }
    const bool any_overflow = __ballot(overflow) != 0;
    if (lane == 0) c.counts[blockIdx.x] = any_overflow ? 0u : staged;
    if (any_overflow && lane == 0) c.head[1] = 1ull;
}

// counts[0 .. n) -> their exclusive bases at counts[n .. 2n), 256 at a time with a running carry; the total to head[0]
__global__ __launch_bounds__(256) void k_evb_scan(u32* __restrict__ counts, u32 n, u64* __restrict__ head) {
    __shared__ u64 sh[256];
    u64 carry = 0;
    for (u32 b0 = 0; b0 < n; b0 += 256) {
        const u32 b = b0 + threadIdx.x;
        const u64 v = b < n ? (u64)counts[b] : 0ull;
        const u64 incl = block_scan(v, sh, threadIdx.x);
        if (b < n) counts[n + b] = (u32)(carry + incl - v);
        const u64 sum = sh[255];
        __syncthreads();                          // (sh is written again by the next round's scan)
        carry += sum;
    }
    if (threadIdx.x == 0) head[0] = carry;
}

__device__ __forceinline__ u64 evb_key(const Event& e) { return ((u64)(u32)e.cls << 32) | (u32)e.first_window; }

__global__ __launch_bounds__(256) void k_evb_emit(EvbCall c) {
    __shared__ u64 keys[EVB_KEY_TILE];
    const u32 tid = threadIdx.x, G = (u32)c.n_groups;
    const EvbGroup g = c.groups[blockIdx.x];
    const u32 n = min(c.counts[blockIdx.x], g.stage_cap);
    const u64 base = c.counts[G + blockIdx.x];
    const Event* stage = c.stage + g.stage_off;
    for (u32 i0 = 0; i0 < n; i0 += 256) {
        const u32 i = i0 + tid;
        const bool mine = i < n;
        Event e{};
        if (mine) e = stage[i];
        const u64 key = evb_key(e);
        u32 rank = 0;
        for (u32 t0 = 0; t0 < n; t0 += EVB_KEY_TILE) {
            const u32 m = min((u32)EVB_KEY_TILE, n - t0);
            __syncthreads();
            for (u32 q = tid; q < m; q += 256) keys[q] = evb_key(stage[t0 + q]);
            __syncthreads();
            if (mine) for (u32 q = 0; q < m; q++) rank += keys[q] < key ? 1u : 0u;
        }
        const u64 o = base + rank;
        if (mine && o < c.out_cap) c.out[o] = e;
    }
}

// ---- dynamic thresholds (events_bank.h): the per-class passes around the launches above

// the change flags of a class: bits 0-1 the level an expiry took away (0: none), bit 2 a learning changed the level, bits 3-4 from,
// bits 5-6 to
__device__ __forceinline__ u32 evd_records_of(u32 flags) { return ((flags & 3u) ? 1u : 0u) + ((flags >> 2) & 1u); }

__global__ __launch_bounds__(256) void k_evd_prepare(EvdCall d) {
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= d.n_classes) return;
    const EvdSlab rd = evd_slab(d.area, d.n_classes, d.rd_parity), wr = evd_slab(d.area, d.n_classes, d.rd_parity ^ 1);
    int L = rd.level[c], n = rd.count[c];
    long long A = rd.learned_at[c];
    const long long E = rd.expires[c];
    const bool dyn = d.dynamic[c] != 0;
    u32 flags = 0;
    if (dyn && n > 0 && d.now > E) {               // (strict: now.After(Timer))
        flags = (u32)L;
        L = 0; n = 0; A = -1;
    }
    wr.level[c] = L; wr.count[c] = n; wr.expires[c] = E; wr.learned_at[c] = A;
    d.thr_eff()[c] = dyn ? ev_threshold(d.base[c], L, d.min_threshold) : d.base[c];
    d.touch()[c] = 0u; d.best()[c] = 0u; d.flags()[c] = flags;
}

// blocks [0, n_groups): the source's staged events that were approved; the blocks behind them: the results of the call's rows
__global__ __launch_bounds__(256) void k_evd_mark(EvbCall c, EventFilterDev f, EvdCall d) {
    const u32 tid = threadIdx.x, G = (u32)c.n_groups;
    if (blockIdx.x < G) {
        const EvbGroup g = c.groups[blockIdx.x];
        const u32 n = min(c.counts[blockIdx.x], g.stage_cap);
        const Event* stage = c.stage + g.stage_off;
        for (u32 i = tid; i < n; i += 256) {
            const Event e = stage[i];
            if (e.status != EVENT_KEPT || (u32)e.cls >= (u32)d.n_classes || d.dynamic[e.cls] == 0) continue;
            // above the trigger the confidence is positive, so its bits order as it does
            if (e.confidence > d.trigger && e.confidence >= d.base[e.cls]) atomicMax(&d.best()[e.cls], __float_as_uint(e.confidence));
        }
        return;
    }
    const u64 i = (u64)(blockIdx.x - G) * 256u + tid;
    if (i >= (u64)d.n_rows * (u64)c.k) return;
    const size_t at = (size_t)c.rowmap[i / (u32)c.k] * (size_t)c.k + (size_t)(i % (u32)c.k);
    const float x = c.conf[at];
    const int ci = c.idx[at];
    if ((u32)ci >= (u32)d.n_classes || f.veto[ci] != 0 || d.dynamic[ci] == 0) return;
    if (evd_slab(d.area, d.n_classes, d.rd_parity ^ 1).count[ci] > 0 && x > f.thr[ci] && x > d.base[ci]) d.touch()[ci] = 1u;
}

__global__ __launch_bounds__(256) void k_evd_apply(EvdCall d, u64* __restrict__ head) {
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= d.n_classes || d.dynamic[c] == 0) return;
    const EvdSlab wr = evd_slab(d.area, d.n_classes, d.rd_parity ^ 1);
    u32 flags = d.flags()[c];
    const u32 best = d.best()[c];
    if (d.touch()[c] != 0u || best != 0u) wr.expires[c] = d.now + d.valid;
    if (best != 0u) {
        const long long A = wr.learned_at[c];
        if (A < 0 || d.now - A >= d.cooldown) {
            const int L = wr.level[c], n0 = wr.count[c], n = n0 == INT_MAX ? n0 : n0 + 1, L2 = min(n, 3);
            wr.count[c] = n; wr.level[c] = L2; wr.learned_at[c] = d.now;
            if (L2 != L) flags |= 4u | ((u32)L << 3) | ((u32)L2 << 5);
        }
    }
    d.flags()[c] = flags;
    const u32 nrec = evd_records_of(flags);
    if (nrec) atomicAdd(reinterpret_cast<u32*>(head) + 3, nrec);           // (the upper half of head[1]; the sum needs no order)
}

// The records, classes ascending and an expiry before a learning, 256 classes at a time with a running carry (k_evb_scan's walk).
// Changes are rare: the block leaves at once when k_evd_apply counted none.
__global__ __launch_bounds__(256) void k_evd_changes(EvdCall d, const u64* __restrict__ head) {
    __shared__ u32 sh[256];
    if ((head[1] >> 32) == 0ull) return;
    u32 carry = 0;
    for (int c0 = 0; c0 < d.n_classes; c0 += 256) {
        const int c = c0 + (int)threadIdx.x;
        const u32 flags = c < d.n_classes ? d.flags()[c] : 0u;
        const u32 v = evd_records_of(flags);
        const u32 incl = block_scan(v, sh, (int)threadIdx.x);
        u32 pos = carry + incl - v;
        if (v) {
            const float base = d.base[c];
            ThresholdChange r{};
            r.cls = c;
            if (flags & 3u) {
                r.previous_level = (int)(flags & 3u); r.new_level = 0; r.reason = EVD_EXPIRY;
                r.previous_value = ev_threshold(base, r.previous_level, d.min_threshold); r.new_value = base; r.confidence = 0.0f;
                d.records()[pos] = r;
                if (pos < (u32)EVD_FIRST_CHANGES) d.first[pos] = r;
                pos++;
            }
            if (flags & 4u) {
                r.previous_level = (int)((flags >> 3) & 3u); r.new_level = (int)((flags >> 5) & 3u); r.reason = EVD_HIGH_CONFIDENCE;
                r.previous_value = ev_threshold(base, r.previous_level, d.min_threshold);
                r.new_value = ev_threshold(base, r.new_level, d.min_threshold);
                r.confidence = __uint_as_float(d.best()[c]);
                d.records()[pos] = r;
                if (pos < (u32)EVD_FIRST_CHANGES) d.first[pos] = r;
            }
        }
        const u32 sum = sh[255];
        __syncthreads();                          // (sh is written again by the next round's scan)
        carry += sum;
    }
}

// update, scan, emit: the launches of every call that has a source in it
void evb_launch_core(const EvbCall& c, const EventFilterDev& f, hipStream_t s) {
    if (c.n_groups <= 0) return;
    const int lds = c.slots * evb_arrays(c.extended) * 4;
    if (c.extended) {
        lds_limit_once<k_evb_update<true>>(EVB_MAX_SLOTS * 7 * 4);
        hipLaunchKernelGGL(k_evb_update<true>, dim3((u32)c.n_groups), dim3(64), lds, s, c, f);
    } else {
        lds_limit_once<k_evb_update<false>>(EVB_MAX_SLOTS * 6 * 4);
        hipLaunchKernelGGL(k_evb_update<false>, dim3((u32)c.n_groups), dim3(64), lds, s, c, f);
    }
    hipLaunchKernelGGL(k_evb_scan, dim3(1), dim3(256), 0, s, c.counts, (u32)c.n_groups, c.head);
    hipLaunchKernelGGL(k_evb_emit, dim3((u32)c.n_groups), dim3(256), 0, s, c);
}

}  // namespace

void launch_event_bank(const EvbCall& c, const EventFilterDev& f, hipStream_t s, const EvdCall* d) {
    hipMemsetAsync(c.head, 0, 16, s);
    if (d) {
        const u32 cb = ((u32)d->n_classes + 255u) / 256u;
        hipLaunchKernelGGL(k_evd_prepare, dim3(cb), dim3(256), 0, s, *d);
        evb_launch_core(c, f, s);
        const u64 results = (u64)d->n_rows * (u64)c.k;
        const u32 mb = (u32)max(c.n_groups, 0) + (u32)((results + 255u) / 256u);
        if (mb) hipLaunchKernelGGL(k_evd_mark, dim3(mb), dim3(256), 0, s, c, f, *d);
        hipLaunchKernelGGL(k_evd_apply, dim3(cb), dim3(256), 0, s, *d, c.head);
        hipLaunchKernelGGL(k_evd_changes, dim3(1), dim3(256), 0, s, *d, (const u64*)c.head);
        return;
    }
    evb_launch_core(c, f, s);
}

}  // namespace bnhip
