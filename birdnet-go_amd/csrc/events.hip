// Detection events on the device (events.h): mark the hits, the veto windows and under guards the dog windows, stable-sort the hits by
// (recording, class), find the events under the greedy hold rule, reduce each, apply the minimum count, the veto and the guards,
// compact into output order.
//
// Every count that lives on the device stays there: the grids are sized from the host's bound N on the row count, and a block
// behind the real count leaves at once.  No step accumulates floating point, and no rank comes from the return value of an atomic:
// the same rows give the same bytes on every run.
#include "events.h"

#include <algorithm>

#include "block_scan.h"

namespace bnhip {

namespace {

using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int EV_TILE = 2048;                     // keys of one radix block: 8 rounds of 256
constexpr int EV_COUNTS_BYTES = 256;              // counts[0] = hits, [1] = veto hits, [2] = events, [3] = dog hits (guarded)

size_t ev_up(size_t b) { return (b + 255) / 256 * 256; }
size_t ev_nb(size_t N) { return (N + 255) / 256; }
size_t ev_nt(size_t N) { return (N + EV_TILE - 1) / EV_TILE; }

// the parts of the scratch, in order
struct EvScratch {
    u64* counts; u64* base; u32* key[2]; u32* idx[2]; u64* veto; u32* hist; u32* digits; uint8_t* start;
    u64* dog = nullptr; u64* dbase = nullptr;      // (guarded only, behind everything else: the other parts lie where they lay)
    size_t bytes;
    EvScratch(void* scratch, size_t N, bool guarded) {
        char* p = static_cast<char*>(scratch);
        size_t o = 0;
        auto take = [&](size_t b) { char* q = p ? p + o : nullptr; o += ev_up(b); return q; };
        counts = reinterpret_cast<u64*>(take(EV_COUNTS_BYTES));
        base = reinterpret_cast<u64*>(take(ev_nb(N) * 8));
        for (int a = 0; a < 2; a++) {
            key[a] = reinterpret_cast<u32*>(take(N * 4));
            idx[a] = reinterpret_cast<u32*>(take(N * 4));
        }
        veto = reinterpret_cast<u64*>(take(N * 8));
        hist = reinterpret_cast<u32*>(take(ev_nt(N) * 256 * 4));
        digits = reinterpret_cast<u32*>(take(256 * 4));
        start = reinterpret_cast<uint8_t*>(take(N));
        if (guarded) {
            dog = reinterpret_cast<u64*>(take(N * 8));
            dbase = reinterpret_cast<u64*>(take(ev_nb(N) * 8));
        }
        bytes = o;
    }
};

__device__ __forceinline__ u32 ev_rows(const u64* __restrict__ d_n, u32 N) { return (u32)min(*d_n, (u64)N); }

// ------------------------------------------------------------------------------------------ hits and veto hits
// a row's two flags, packed for one scan: bit 0 = hit, bit 32 = veto hit.  The compares are strict and false for a NaN on either
// side, so a threshold of +inf or NaN excludes its class.
__device__ __forceinline__ u64 ev_mark(const DetRow& q, const EventFilterDev& f) {
    if ((u32)q.cls >= (u32)f.n_classes) return 0;
    const bool v = f.veto && f.veto[q.cls] != 0;
    const bool hit = !v && q.confidence > f.thr[q.cls];
    const bool vh = v && q.confidence > f.veto_thr;
    return (hit ? 1ull : 0ull) | (vh ? 1ull << 32 : 0ull);
}
// a row's third flag, scanned on its own: a dog hit, whatever else the row is
__device__ __forceinline__ u64 ev_mark_dog(const DetRow& q, const EventFilterDev& f) {
    return (u32)q.cls < (u32)f.n_classes && f.g.dog_hit(q.cls, q.confidence) ? 1ull : 0ull;
}
// thread = row: the block's packed totals; DOG: also its dog hits
template <bool DOG>
__global__ __launch_bounds__(256) void k_ev_mark_count(const DetRow* __restrict__ rows, const u64* __restrict__ d_n, u32 N, EventFilterDev f,
                                                       u64* __restrict__ base, u64* __restrict__ dbase) {
    __shared__ u64 sh[256];
    const u32 n = ev_rows(d_n, N), i = blockIdx.x * 256 + threadIdx.x;
    DetRow q{0, 0, 0, 0.0f};
    if (i < n) q = rows[i];
    const u64 c = i < n ? ev_mark(q, f) : 0ull;
    const u64 incl = block_scan(c, sh, threadIdx.x);
    if (threadIdx.x == 255) base[blockIdx.x] = incl;
    if (DOG) {
        __shared__ u64 shd[256];
        const u64 dg = i < n ? ev_mark_dog(q, f) : 0ull;
        const u64 dincl = block_scan(dg, shd, threadIdx.x);
        if (threadIdx.x == 255) dbase[blockIdx.x] = dincl;
    }
}
// one block: the block totals in place -> exclusive bases, 256 at a time with a running carry.  The grand total goes to *lo, or
// with hi its two packed halves to *lo and *hi.
__global__ __launch_bounds__(256) void k_ev_bases(u64* __restrict__ base, u32 nb, u64* __restrict__ lo, u64* __restrict__ hi) {
    __shared__ u64 sh[256];
    u64 carry = 0;
    for (u32 b0 = 0; b0 < nb; b0 += 256) {
        const u32 b = b0 + threadIdx.x;
        const u64 c = b < nb ? base[b] : 0ull;
        const u64 incl = block_scan(c, sh, threadIdx.x);
        if (b < nb) base[b] = carry + incl - c;
        const u64 sum = sh[255];
        __syncthreads();                          // (sh is written again by the next round's scan)
        carry += sum;
    }
    if (threadIdx.x == 0) {
        if (hi) { *lo = carry & 0xffffffffull; *hi = carry >> 32; }
        else *lo = carry;
    }
}
// thread = row: a hit's key and row number, a veto hit's (recording, window), DOG: a dog hit's (recording, window), each in row order
template <bool DOG>
__global__ __launch_bounds__(256) void k_ev_mark_scatter(const DetRow* __restrict__ rows, const u64* __restrict__ d_n, u32 N, EventFilterDev f,
                                                         const u64* __restrict__ base, u32* __restrict__ key, u32* __restrict__ idx,
                                                         u64* __restrict__ veto, const u64* __restrict__ dbase, u64* __restrict__ dog) {
    __shared__ u64 sh[256];
    const u32 n = ev_rows(d_n, N), i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= n) return;
    DetRow q{0, 0, 0, 0.0f};
    u64 c = 0;
    if (i < n) { q = rows[i]; c = ev_mark(q, f); }
    const u64 excl = base[blockIdx.x] + block_scan(c, sh, threadIdx.x) - c;
    if (c & 1ull) {
        const u32 j = (u32)excl;
        key[j] = (u32)q.recording * (u32)f.n_classes + (u32)q.cls;
        idx[j] = i;
    }
    if (c >> 32) veto[excl >> 32] = ((u64)(u32)q.recording << 32) | (u32)q.window;
    if (DOG) {
        __shared__ u64 shd[256];
        const u64 dg = i < n ? ev_mark_dog(q, f) : 0ull;
        const u64 dexcl = dbase[blockIdx.x] + block_scan(dg, shd, threadIdx.x) - dg;
        if (dg) dog[dexcl] = ((u64)(u32)q.recording << 32) | (u32)q.window;
    }
}

// ------------------------------------------------------------------------------------------ the stable sort
// One pass of an LSD radix sort on an 8-bit digit, in three launches: per-block digit counts, a scan of every digit's counts over the
// blocks (a block per digit; the scatter adds the digits in front from the 256 digit totals), the scatter.  A block takes EV_TILE
// keys in rounds of 256.  A key's rank among the round's keys of its digit comes from wave ballots (the lanes in front with the
// same digit) and the per-wave digit counts in LDS; run[] carries each digit's count over the rounds.  SCATTER = false only counts:
// hist[digit * nt + block].
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_ev_radix(const u32* __restrict__ key_in, const u32* __restrict__ idx_in, u32* __restrict__ key_out,
                                                  u32* __restrict__ idx_out, const u64* __restrict__ counts, u32 N, int shift,
                                                  u32* __restrict__ hist, u32 nt, const u32* __restrict__ digits) {
    __shared__ u32 cnt[4][256];
    __shared__ u32 run[256];
    __shared__ u32 sh[256];
    const u32 n = ev_rows(counts, N), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 t0 = blockIdx.x * EV_TILE;
    if (t0 >= n) {
        if (!SCATTER) hist[tid * nt + blockIdx.x] = 0;
        return;
    }
    u32 first = 0;
    if (SCATTER) {                                // the keys of the digits in front, then those of this digit in the blocks in front
        const u32 d = digits[tid];
        first = block_scan(d, sh, tid) - d + hist[tid * nt + blockIdx.x];
    }
    run[tid] = first;
    for (int w = 0; w < 4; w++) cnt[w][tid] = 0;
    __syncthreads();
    const u64 lt = (1ull << lane) - 1ull;
    for (int round = 0; round < EV_TILE / 256; round++) {
        const u32 i = t0 + round * 256 + tid;
        const bool valid = i < n;
        const u32 k = valid ? key_in[i] : 0u;
        const u32 digit = (k >> shift) & 255u;
        u64 peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const u64 m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        const u32 in_front = (u32)__popcll(peers & lt);
        if (valid && in_front == 0) cnt[wave][digit] = (u32)__popcll(peers);
        __syncthreads();
        if (SCATTER && valid) {
            u32 o = run[digit] + in_front;
            for (u32 w = 0; w < wave; w++) o += cnt[w][digit];
            if (o < n) {                          // (always: a stable rank below the key count)
                key_out[o] = k;
                idx_out[o] = idx_in[i];
            }
        }
        __syncthreads();
        run[tid] += cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
        for (int w = 0; w < 4; w++) cnt[w][tid] = 0;
        __syncthreads();
    }
    if (!SCATTER) hist[tid * nt + blockIdx.x] = run[tid];
}
// block = digit: its counts hist[digit * nt .. + nt) in place -> exclusive, 2048 at a time (8 per thread) with a running carry; the
// digit's total
__global__ __launch_bounds__(256) void k_ev_hist_scan(u32* __restrict__ hist_all, u32 m, u32* __restrict__ digits) {
    __shared__ u32 sh[256];
    u32* __restrict__ hist = hist_all + (size_t)blockIdx.x * m;
    u32 carry = 0;
    for (u32 b0 = 0; b0 < m; b0 += 2048) {
        const u32 i0 = b0 + threadIdx.x * 8;
        u32 v[8], sum = 0;
        for (int e = 0; e < 8; e++) {
            const u32 t = i0 + e < m ? hist[i0 + e] : 0u;
            v[e] = sum;
            sum += t;
        }
        const u32 excl = block_scan(sum, sh, threadIdx.x) - sum;
        for (int e = 0; e < 8; e++) if (i0 + e < m) hist[i0 + e] = carry + excl + v[e];
        const u32 tot = sh[255];
        __syncthreads();
        carry += tot;
    }
    if (threadIdx.x == 0) digits[blockIdx.x] = carry;
}

// ------------------------------------------------------------------------------------------ the events
// thread = sorted hit: its window and confidence beside the key, and no event start yet
__global__ __launch_bounds__(256) void k_ev_gather(const DetRow* __restrict__ rows, const u32* __restrict__ idx, const u64* __restrict__ counts,
                                                   u32 N, int* __restrict__ win, float* __restrict__ conf, uint8_t* __restrict__ start) {
    const u32 n = ev_rows(counts, N), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const DetRow q = rows[idx[i]];
    win[i] = q.window;
    conf[i] = q.confidence;
    start[i] = 0;
}
// The greedy rule.  wave = 64 sorted hits; for every (recording, class) group that begins among them the wave walks the group from
// its first hit on, 64 hits a step: the step's event starts fall out of ballots (windows ascend inside a group, so the hits at or
// beyond b + hold are a suffix), and only the open event's first window b passes from step to step.  A species that hits in every
// window of an hour's recording is 113 steps of one wave; a serial walk would be 7 195 dependent loads.
__global__ __launch_bounds__(256) void k_ev_walk(const u32* __restrict__ key, const int* __restrict__ win, const u64* __restrict__ counts, u32 N,
                                                 int hold, uint8_t* __restrict__ start) {
    const u32 n = ev_rows(counts, N), lane = threadIdx.x & 63;
    const u32 c0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (c0 >= n) return;
    const u32 me = c0 + lane;
    const bool head = me < n && (me == 0 || key[me] != key[me - 1]);
    u64 heads = __ballot(head);
    while (heads) {
        const u32 h = (u32)__ffsll((long long)heads) - 1u;
        heads &= heads - 1ull;
        u32 pos = c0 + h;
        const u32 k = key[pos];
        long long b = 0;
        bool open = false;
        for (;;) {
            const u32 j = pos + lane;
            const bool in = j < n && key[j] == k;
            const int w = in ? win[j] : 0;
            const u64 m_in = __ballot(in);
            if (!open) {                          // the group's first hit opens its first event
                b = __shfl(w, 0);
                if (lane == 0) start[pos] = 1;
                open = true;
            }
            for (;;) {
                const u64 m = __ballot(in && (long long)w >= b + hold);
                if (!m) break;
                const int f = __ffsll((long long)m) - 1;
                b = __shfl(w, f);
                if ((int)lane == f) start[j] = 1;
            }
            if (m_in != ~0ull) break;             // the group ends inside this step
            pos += 64;
            if (pos >= n) break;
        }
    }
}

// The same walk under extended capture (events.h, ev_deadline).  A hit joins while its window lies before the deadline that its
// predecessor's window gave the open event, so with b known lane j compares against ev_deadline(b, window of lane j - 1); lane 0's
// predecessor is the last window of the step before, carried in prev.  The first lane at or beyond its deadline starts the next
// event; the lanes behind it are judged again with the new b.  A deadline may move either way, so the lanes beyond it are no
// suffix any more: todo masks the lanes that have their event.  A group of a class that does not slide keeps b + hold.
__global__ __launch_bounds__(256) void k_ev_walk_slide(const u32* __restrict__ key, const int* __restrict__ win, const u64* __restrict__ counts,
                                                       u32 N, EventFilterDev f, uint8_t* __restrict__ start) {
    const u32 n = ev_rows(counts, N), lane = threadIdx.x & 63;
    const u32 c0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (c0 >= n) return;
    const u32 me = c0 + lane;
    const bool head = me < n && (me == 0 || key[me] != key[me - 1]);
    u64 heads = __ballot(head);
    while (heads) {
        const u32 h = (u32)__ffsll((long long)heads) - 1u;
        heads &= heads - 1ull;
        u32 pos = c0 + h;
        const u32 k = key[pos];
        const bool slides = f.slides((int)(k % (u32)f.n_classes));
        long long b = 0;
        int prev = 0;
        bool open = false;
        for (;;) {
            const u32 j = pos + lane;
            const bool in = j < n && key[j] == k;
            const int w = in ? win[j] : 0;
            const u64 m_in = __ballot(in);
            u64 todo = ~0ull;
            if (!open) {                          // the group's first hit opens its first event
                b = __shfl(w, 0);
                if (lane == 0) start[pos] = 1;
                open = true;
                todo = ~1ull;
            }
            const int up = __shfl_up(w, 1);
            const long long p = lane == 0 ? prev : up;
            for (;;) {
                const long long d = slides ? ev_deadline(b, p, f.hold, f.x) : b + f.hold;
                const u64 m = __ballot(in && (long long)w >= d) & todo;
                if (!m) break;
                const int s = __ffsll((long long)m) - 1;
                b = __shfl(w, s);
                if ((int)lane == s) start[j] = 1;
                todo = (~1ull) << s;              // (s == 63: none)
            }
            if (m_in != ~0ull) break;             // the group ends inside this step
            prev = __shfl(w, 63);
            pos += 64;
            if (pos >= n) break;
        }
    }
}

// the event that begins at sorted hit i; -> whether it is answered
__device__ __forceinline__ bool ev_reduce(u32 i, u32 n, const u32* __restrict__ key, const int* __restrict__ win, const float* __restrict__ conf,
                                          const uint8_t* __restrict__ start, const u64* __restrict__ veto, u32 n_veto,
                                          const u64* __restrict__ dog, u32 n_dog, const EventFilterDev& f, Event& e) {
    const u32 k = key[i];
    float best = conf[i];
    int bw = win[i], last = bw, count = 0;
    u32 j = i;
    do {
        const float x = conf[j];
        last = win[j];
        if (x > best) { best = x; bw = last; }    // (ties: the earliest stays, as the reference replaces on > only)
        count++;
        j++;
    } while (j < n && !start[j]);
    e.recording = (int32_t)(k / (u32)f.n_classes);
    e.cls = (int32_t)(k % (u32)f.n_classes);
    e.first_window = win[i];
    e.last_window = last;
    e.best_window = bw;
    e.count = count;
    e.confidence = best;
    e.status = EVENT_KEPT;
    if (count < f.min_count) {
        e.status = EVENT_FEW;
    } else {
        // the recording's first veto window at or behind b: vetoed when it lies inside the hold - before the event's final deadline,
        // which under extended capture is the one its last hit gave it
        const u64 from = ((u64)(u32)e.recording << 32) | (u32)e.first_window;
        u64 end = from + (u64)(u32)f.hold;
        if (f.slides(e.cls))
            end = ((u64)(u32)e.recording << 32) + (u64)min(ev_deadline(e.first_window, last, f.hold, f.x), 0xffffffffll);
        u32 lo = 0, hi = n_veto;
        while (lo < hi) {
            const u32 mid = lo + (hi - lo) / 2;
            if (veto[mid] < from) lo = mid + 1; else hi = mid;
        }
        if (lo < n_veto && veto[lo] < end) e.status = EVENT_VETOED;
        if (e.status == EVENT_KEPT && n_dog && f.g.dog_filtered && f.g.dog_filtered[e.cls] != 0) {
            // the recording's last dog window before the final deadline d (end = (recording, d)): the entry in front of the first at
            // or behind end
            lo = 0, hi = n_dog;
            while (lo < hi) {
                const u32 mid = lo + (hi - lo) / 2;
                if (dog[mid] < end) lo = mid + 1; else hi = mid;
            }
            if (lo > 0 && (dog[lo - 1] >> 32) == (u64)(u32)e.recording &&
                f.g.dog_drops(e.cls, (long long)(end & 0xffffffffull), (long long)(dog[lo - 1] & 0xffffffffull)))
                e.status = EVENT_DOG;
        }
        if (e.status == EVENT_KEPT && f.g.n_spans > 0 && f.g.daylight && f.g.daylight[e.cls] != 0) {
            // the last span that begins at or before (recording, b): rows (recording, from, to), ascending and disjoint
            int slo = 0, shi = f.g.n_spans;
            while (slo < shi) {
                const int mid = slo + (shi - slo) / 2;
                const int32_t* sp = f.g.spans + (size_t)mid * 3;
                if (sp[0] < e.recording || (sp[0] == e.recording && sp[1] <= e.first_window)) slo = mid + 1; else shi = mid;
            }
            if (slo > 0) {
                const int32_t* sp = f.g.spans + (size_t)(slo - 1) * 3;
                if (sp[0] == e.recording && e.first_window < sp[2]) e.status = EVENT_DAYLIGHT;
            }
        }
    }
    return e.status == EVENT_KEPT || (f.flags & EVENTS_KEEP_DROPPED);
}
// thread = sorted hit: 1 where an answered event begins, scanned over the block; EMIT writes the events at their ranks
template <bool EMIT>
__global__ __launch_bounds__(256) void k_ev_events(const u32* __restrict__ key, const int* __restrict__ win, const float* __restrict__ conf,
                                                   const uint8_t* __restrict__ start, const u64* __restrict__ veto, const u64* __restrict__ dog,
                                                   const u64* __restrict__ counts, u32 N, EventFilterDev f, u64* __restrict__ base,
                                                   Event* __restrict__ out, u64 cap) {
    __shared__ u32 sh[256];
    const u32 n = ev_rows(counts, N), n_veto = (u32)min(counts[1], (u64)N), i = blockIdx.x * 256 + threadIdx.x;
    const u32 n_dog = dog ? (u32)min(counts[3], (u64)N) : 0u;
    if (blockIdx.x * 256 >= n) {
        if (!EMIT && threadIdx.x == 0) base[blockIdx.x] = 0;
        return;
    }
    Event e;
    const u32 c = i < n && start[i] && ev_reduce(i, n, key, win, conf, start, veto, n_veto, dog, n_dog, f, e) ? 1u : 0u;
    const u32 incl = block_scan(c, sh, threadIdx.x);
    if (!EMIT) {
        if (threadIdx.x == 255) base[blockIdx.x] = incl;
        return;
    }
    const u64 o = base[blockIdx.x] + incl - c;
    if (c && o < cap) out[o] = e;
}

}  // namespace

int events_passes(unsigned long long max_key) {
    int p = 1;
    while (p < 4 && (max_key >> (8 * p)) != 0) p++;
    return p;
}
size_t events_scratch_bytes(size_t N, bool guarded) { return EvScratch(nullptr, N, guarded).bytes; }
unsigned long long* events_total(void* scratch) { return static_cast<u64*>(scratch) + 2; }

void launch_events(const DetRow* rows, const unsigned long long* d_n, size_t N, const EventFilterDev& f, int passes, void* scratch, Event* out,
                   unsigned long long cap, hipStream_t s) {
    const bool dogs = f.g.dog != nullptr;
    const EvScratch sc(scratch, N, dogs);
    hipMemsetAsync(sc.counts, 0, EV_COUNTS_BYTES, s);
    if (N == 0) return;
    const u32 n32 = (u32)N, nb = (u32)ev_nb(N), nt = (u32)ev_nt(N);
    const dim3 rows_grid(nb), tiles_grid(nt), block(256);
    if (dogs) {
        hipLaunchKernelGGL(k_ev_mark_count<true>, rows_grid, block, 0, s, rows, d_n, n32, f, sc.base, sc.dbase);
        hipLaunchKernelGGL(k_ev_bases, dim3(1), block, 0, s, sc.base, nb, sc.counts, sc.counts + 1);
        hipLaunchKernelGGL(k_ev_bases, dim3(1), block, 0, s, sc.dbase, nb, sc.counts + 3, (u64*)nullptr);
        hipLaunchKernelGGL(k_ev_mark_scatter<true>, rows_grid, block, 0, s, rows, d_n, n32, f, sc.base, sc.key[0], sc.idx[0], sc.veto, sc.dbase,
                           sc.dog);
    } else {
        hipLaunchKernelGGL(k_ev_mark_count<false>, rows_grid, block, 0, s, rows, d_n, n32, f, sc.base, (u64*)nullptr);
        hipLaunchKernelGGL(k_ev_bases, dim3(1), block, 0, s, sc.base, nb, sc.counts, sc.counts + 1);
        hipLaunchKernelGGL(k_ev_mark_scatter<false>, rows_grid, block, 0, s, rows, d_n, n32, f, sc.base, sc.key[0], sc.idx[0], sc.veto,
                           (const u64*)nullptr, (u64*)nullptr);
    }
    int a = 0;
    for (int p = 0; p < passes; p++, a ^= 1) {
        hipLaunchKernelGGL(k_ev_radix<false>, tiles_grid, block, 0, s, sc.key[a], sc.idx[a], sc.key[a ^ 1], sc.idx[a ^ 1], sc.counts, n32, 8 * p,
                           sc.hist, nt, sc.digits);
        hipLaunchKernelGGL(k_ev_hist_scan, dim3(256), block, 0, s, sc.hist, nt, sc.digits);
        hipLaunchKernelGGL(k_ev_radix<true>, tiles_grid, block, 0, s, sc.key[a], sc.idx[a], sc.key[a ^ 1], sc.idx[a ^ 1], sc.counts, n32, 8 * p,
                           sc.hist, nt, sc.digits);
    }
    // the sorted keys and row numbers are in pair a; the other pair is free and takes the windows and confidences
    int* win = reinterpret_cast<int*>(sc.key[a ^ 1]);
    float* conf = reinterpret_cast<float*>(sc.idx[a ^ 1]);
    hipLaunchKernelGGL(k_ev_gather, rows_grid, block, 0, s, rows, sc.idx[a], sc.counts, n32, win, conf, sc.start);
    if (f.x.max_windows > 0) hipLaunchKernelGGL(k_ev_walk_slide, rows_grid, block, 0, s, sc.key[a], win, sc.counts, n32, f, sc.start);
    else hipLaunchKernelGGL(k_ev_walk, rows_grid, block, 0, s, sc.key[a], win, sc.counts, n32, f.hold, sc.start);
    hipLaunchKernelGGL(k_ev_events<false>, rows_grid, block, 0, s, sc.key[a], win, conf, sc.start, sc.veto, sc.dog, sc.counts, n32, f, sc.base, out, cap);
    hipLaunchKernelGGL(k_ev_bases, dim3(1), block, 0, s, sc.base, nb, sc.counts + 2, (u64*)nullptr);
    hipLaunchKernelGGL(k_ev_events<true>, rows_grid, block, 0, s, sc.key[a], win, conf, sc.start, sc.veto, sc.dog, sc.counts, n32, f, sc.base, out, cap);
}

}  // namespace bnhip
