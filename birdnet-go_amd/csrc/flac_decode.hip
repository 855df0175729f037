// The device FLAC decoder: flac_decode.h says what each kernel is for, flac_parse.h states the frame reader they share with the
// host.  The entropy parse and the predictor run in one lane of a wavefront against LDS; the other lanes stage the frame's bytes,
// fold its CRC-16 and store its samples.
#include "flac_decode.h"

#include <algorithm>
#include <cstring>

#include "block_scan.h"
#include "flac_parse.h"
#include "kernels.h"
#include "ragged.h"

namespace bnhip {

using u64 = unsigned long long;

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER_THREAD = FLACDEC_SCAN_TILE / SCAN_THREADS;
constexpr int WAVE = 64;

__device__ __forceinline__ FlacStreamShape shape_of(const FlacDecStream& r) { return FlacStreamShape{r.rate, r.bs, r.total, r.frames}; }

// Grid: the burst's scan tiles.  A tile's bytes and the FLACDEC_HEAD_MAX - 1 after it (as far as the stream goes) are staged in LDS;
// thread t tests positions t, t + 256, ..
__global__ __launch_bounds__(SCAN_THREADS) void k_flacdec_scan(const uint8_t* __restrict__ streams, const FlacDecStream* __restrict__ rows,
                                                               const long long* __restrict__ tile0, int n_streams,
                                                               uint32_t* __restrict__ count, FlacDecCand* __restrict__ cand,
                                                               const long long* __restrict__ cand0) {
    __shared__ uint8_t sb[FLACDEC_SCAN_TILE + FLACDEC_HEAD_MAX];
    __shared__ uint32_t sc[SCAN_THREADS];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    const int c = ragged_clip(tile0, n_streams, (long long)blockIdx.x);
    const FlacDecStream r = rows[c];
    const u64 len = r.end - r.begin;
    const u64 p0 = r.audio + (u64)((long long)blockIdx.x - tile0[c]) * FLACDEC_SCAN_TILE;       // from the stream's begin
    if (p0 >= len) return;                                                                      // (block-uniform; the host's tiles end before)
    const u64 left = len - p0;
    const int staged = (int)(left < (u64)(FLACDEC_SCAN_TILE + FLACDEC_HEAD_MAX) ? left : (u64)(FLACDEC_SCAN_TILE + FLACDEC_HEAD_MAX));
    const uint8_t* src = streams + r.begin + p0;
    for (int i = tid; i < staged; i += SCAN_THREADS) sb[i] = src[i];
    __syncthreads();
    const FlacStreamShape shape = shape_of(r);
    const int positions = staged < FLACDEC_SCAN_TILE ? staged : FLACDEC_SCAN_TILE;
    uint32_t mask = 0;
    FlacFrameHead h;
    for (int j = 0; j < SCAN_PER_THREAD; j++) {
        const int i = tid + j * SCAN_THREADS;
        if (i < positions && i + 1 < staged && sb[i] == 0xFFu && sb[i + 1] == 0xF8u && flac_frame_head(sb + i, (size_t)(staged - i), shape, &h))
            mask |= 1u << j;
    }
    const uint32_t mine = (uint32_t)__popc(mask);
    const uint32_t incl = block_scan(mine, sc, tid);
    if (tid == SCAN_THREADS - 1) s_base = incl ? atomicAdd(&count[c], incl) : 0u;
    __syncthreads();
    uint32_t slot = s_base + incl - mine;
    for (int j = 0; j < SCAN_PER_THREAD; j++) {
        if (!((mask >> j) & 1u)) continue;
        const int i = tid + j * SCAN_THREADS;
        if (slot < r.cand_cap && flac_frame_head(sb + i, (size_t)(staged - i), shape, &h))
            cand[cand0[c] + slot] = FlacDecCand{p0 + (u64)i, 0ull, h.number, h.bs, h.bytes, 0u};
        slot++;
    }
}

// The frame bytes of a candidate in LDS: min(what is left of the stream, the VERBATIM bound of the stream's block size).
__device__ __forceinline__ uint32_t stage_frame(const uint8_t* __restrict__ streams, const FlacDecStream& r, u64 start, u64 want,
                                                uint8_t* __restrict__ fb, int lane) {
    const u64 len = r.end - r.begin;
    u64 avail = start < len ? len - start : 0;
    if (avail > want) avail = want;
    const uint8_t* src = streams + r.begin + start;
    for (uint32_t i = (uint32_t)lane; i < (uint32_t)avail; i += WAVE) fb[i] = src[i];
    return (uint32_t)avail;
}

// CRC-16 of fb[0 .. n) by the wavefront: 64 chunks with zero bytes in front (a CRC that starts from 0 ignores them), folded in a
// tree as k_flac_emit folds the encoder's.  Every lane returns it.
__device__ __forceinline__ uint32_t wave_crc16(const uint8_t* __restrict__ fb, uint32_t n, uint32_t* __restrict__ cv, int lane) {
    const int C = (int)((n + WAVE - 1) / WAVE), padding = WAVE * C - (int)n;
    uint32_t crc = 0, mul = 1;
    for (int j = 0; j < C; j++) {
        const int b = lane * C + j - padding;
        if (b >= 0) crc = flac_crc16_step(crc, fb[b]);
        mul = flac_crc16_step(mul, 0);                                               // x^(8 C)
    }
    cv[lane] = crc;
    for (int s = 1; s < WAVE; s <<= 1) {
        __syncthreads();
        if ((lane & (2 * s - 1)) == 0) cv[lane] = flac_crc16_mul(cv[lane], mul) ^ cv[lane + s];
        mul = flac_crc16_mul(mul, mul);
    }
    __syncthreads();
    return cv[0];
}

// Grid: the burst's candidate slots, a wavefront each.  Dynamic LDS: flacdec_frame_cap(the burst's largest block size).
__global__ __launch_bounds__(WAVE) void k_flacdec_parse(const uint8_t* __restrict__ streams, const FlacDecStream* __restrict__ rows,
                                                        const long long* __restrict__ cand0, const long long* __restrict__ frame0,
                                                        int n_streams, const uint32_t* __restrict__ count, FlacDecCand* __restrict__ cand,
                                                        uint32_t* __restrict__ head) {
    extern __shared__ __attribute__((aligned(16))) uint8_t flacdec_sm[];
    __shared__ uint32_t cv[WAVE];
    __shared__ uint32_t s_rc, s_bytes;
    const int lane = threadIdx.x;
    const long long slot = (long long)blockIdx.x;
    const int c = ragged_clip(cand0, n_streams, slot);
    const FlacDecStream r = rows[c];
    const uint32_t have = count[c] < r.cand_cap ? count[c] : r.cand_cap;
    if (slot - cand0[c] >= (long long)have) return;                                  // (block-uniform)
    const FlacDecCand cd = cand[slot];
    if (cd.number >= r.frames) return;
    const uint32_t staged = stage_frame(streams, r, cd.start, flacdec_frame_cap(r.bs), flacdec_sm, lane);
    __syncthreads();
    if (lane == 0) {
        FlacCountSink sink;
        size_t bytes = 0;
        const uint32_t rc = cd.head_bytes <= staged && cd.bs <= r.bs ? (uint32_t)flac_parse_frame(flacdec_sm, staged, cd.head_bytes, cd.bs, sink, &bytes)
                                                                      : (uint32_t)FLACP_INVALID;
        s_rc = rc;
        s_bytes = rc == FLACP_OK ? (uint32_t)bytes : 0u;
    }
    __syncthreads();
    if (s_rc != FLACP_OK || s_bytes > staged) return;
    const uint32_t bytes = s_bytes;
    if (wave_crc16(flacdec_sm, bytes, cv, lane) != 0) return;                        // (the CRC of a frame with its CRC-16 is zero)
    if (lane == 0) {
        cand[slot].end = cd.start + bytes;
        cand[slot].next = atomicExch(&head[frame0[c] + cd.number], (uint32_t)slot + 1u);
    }
}

// Grid: the streams, a wavefront each.  Frame numbers are taken 64 at a time: lane l loads the list of number j0 + l, then the lanes
// resolve in turn which of a number's candidates starts where the chain stands.
__global__ __launch_bounds__(WAVE) void k_flacdec_link(const FlacDecStream* __restrict__ rows, const long long* __restrict__ frame0,
                                                       const uint32_t* __restrict__ count, const FlacDecCand* __restrict__ cand,
                                                       const uint32_t* __restrict__ head, uint32_t* __restrict__ chain,
                                                       bnhip_flac_decode_result* __restrict__ result) {
    const int lane = threadIdx.x, c = blockIdx.x;
    const FlacDecStream r = rows[c];
    if (r.status != BNHIP_FLAC_OK || count[c] > r.cand_cap) {
        if (lane == 0) result[c] = bnhip_flac_decode_result{r.status != BNHIP_FLAC_OK ? r.status : (int32_t)BNHIP_FLAC_UNSUPPORTED, 0, 0ull};
        return;
    }
    const long long f0 = frame0[c];
    u64 pos = r.audio;
    uint32_t done = 0;
    bool ok = true;
    for (uint32_t j0 = 0; j0 < r.frames && ok; j0 += WAVE) {
        const uint32_t j = j0 + (uint32_t)lane;
        uint32_t idx = j < r.frames ? head[f0 + j] : 0u;
        FlacDecCand cd{};
        if (idx) cd = cand[idx - 1];
        const uint32_t m = r.frames - j0 < (uint32_t)WAVE ? r.frames - j0 : (uint32_t)WAVE;
        for (uint32_t l = 0; l < m; l++) {
            int found = 0;
            if ((uint32_t)lane == l) {
                for (uint32_t steps = 0; idx && cd.start != pos && steps < r.cand_cap; steps++) {
                    idx = cd.next;
                    if (idx) cd = cand[idx - 1];
                }
                found = idx != 0 && cd.start == pos && cd.end > cd.start;
                if (found) chain[f0 + j] = idx;
            }
            found = __shfl(found, (int)l);
            if (!found) { ok = false; break; }
            const uint32_t lo = __shfl((uint32_t)cd.end, (int)l), hi = __shfl((uint32_t)(cd.end >> 32), (int)l);
            pos = ((u64)hi << 32) | lo;
            done++;
        }
    }
    if (ok && (pos != r.end - r.begin || r.frames == 0)) ok = false;                 // bytes after the last frame; a stream too short for its count
    if (lane == 0)
        result[c] = ok ? bnhip_flac_decode_result{BNHIP_FLAC_OK, (int32_t)done, 0ull} : bnhip_flac_decode_result{BNHIP_FLAC_CORRUPT, (int32_t)done, pos};
}

// Grid: the burst's frames, a wavefront each.  Dynamic LDS: the frame's bytes, then its samples int16 [the burst's largest block size].
__global__ __launch_bounds__(WAVE) void k_flacdec_restore(const uint8_t* __restrict__ streams, const FlacDecStream* __restrict__ rows,
                                                          const long long* __restrict__ frame0, int n_streams,
                                                          const FlacDecCand* __restrict__ cand, const uint32_t* __restrict__ chain,
                                                          const bnhip_flac_decode_result* __restrict__ result, uint32_t* __restrict__ bad,
                                                          int16_t* __restrict__ pcm, u64 pcm_cap, uint32_t sample_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t flacdec_sm[];
    __shared__ uint32_t s_rc;
    __shared__ int32_t s_coef[FLACDEC_MAX_ORDER];
    const int lane = threadIdx.x;
    const long long f = (long long)blockIdx.x;
    const int c = ragged_clip(frame0, n_streams, f);
    if (result[c].status != BNHIP_FLAC_OK) return;                                   // (block-uniform)
    const FlacDecStream r = rows[c];
    const uint32_t j = (uint32_t)(f - frame0[c]);
    const uint32_t idx = chain[f];
    if (!idx) return;
    const FlacDecCand cd = cand[idx - 1];
    if (cd.end <= cd.start || cd.end - cd.start > flacdec_frame_cap(r.bs) || cd.bs > r.bs || cd.number != j) return;
    int16_t* xs = reinterpret_cast<int16_t*>(flacdec_sm + sample_off);
    const uint32_t staged = stage_frame(streams, r, cd.start, cd.end - cd.start, flacdec_sm, lane);
    __syncthreads();
    if (lane == 0) {
        FlacStoreSink sink{xs, s_coef};
        size_t bytes = 0;
        s_rc = cd.head_bytes <= staged ? (uint32_t)flac_parse_frame(flacdec_sm, staged, cd.head_bytes, cd.bs, sink, &bytes) : (uint32_t)FLACP_INVALID;
    }
    __syncthreads();
    if (s_rc != FLACP_OK) {
        if (lane == 0) atomicMin(&bad[c], j);
        return;
    }
    const u64 first = (u64)j * r.bs;                                                 // of the clip
    for (uint32_t i = (uint32_t)lane; i < cd.bs; i += WAVE) {
        const u64 at = first + i;
        if (at < r.total && r.pcm0 + at < pcm_cap) pcm[r.pcm0 + at] = xs[i];
    }
}

__global__ __launch_bounds__(256) void k_flacdec_finish(const long long* __restrict__ frame0, int n_streams, const FlacDecCand* __restrict__ cand,
                                                        const uint32_t* __restrict__ chain, const uint32_t* __restrict__ bad,
                                                        bnhip_flac_decode_result* __restrict__ result) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_streams || bad[c] == 0xFFFFFFFFu || result[c].status != BNHIP_FLAC_OK) return;
    const uint32_t idx = chain[frame0[c] + bad[c]];
    result[c] = bnhip_flac_decode_result{BNHIP_FLAC_CORRUPT, (int32_t)bad[c], idx ? cand[idx - 1].start : 0ull};
}

struct Plan {
    std::vector<FlacDecStream> rows;
    std::vector<long long> tile0, cand0, frame0;
    uint32_t max_bs = 0;
    size_t pcm = 0;
};

// -> NULL, or why the burst cannot run
const char* plan(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, Plan* p) {
    if (n_streams < 1 || n_streams > 65535) return "n_streams must be in [1, 65535]";
    if (!infos || !offsets) return "NULL/empty argument";
    p->rows.resize((size_t)n_streams);
    p->tile0.assign((size_t)n_streams + 1, 0);
    p->cand0 = p->tile0;
    p->frame0 = p->tile0;
    for (int c = 0; c < n_streams; c++) {
        if (offsets[c + 1] < offsets[c]) return "offsets must ascend";
        if (offsets[c + 1] > FLACDEC_MAX_BYTES) return "the burst must be below 2^40 bytes";
        const bnhip_flac_info& in = infos[c];
        FlacDecStream& r = p->rows[(size_t)c];
        r = FlacDecStream{};
        r.begin = offsets[c];
        r.end = offsets[c + 1];
        r.pcm0 = p->pcm;
        r.status = in.status;
        long long tiles = 0;
        if (in.status == BNHIP_FLAC_OK) {
            const u64 len = r.end - r.begin;
            if (in.channels != 1 || in.bits != 16 || in.total_samples < 1 || in.total_samples > 0x7FFFFFFFull || in.max_block < FLACDEC_MIN_BLOCK ||
                in.max_block > FLACDEC_MAX_BLOCK || in.audio_offset > len)
                return "a stream's info is marked BNHIP_FLAC_OK but is not one bnhip_flac_stream_info accepts";
            r.audio = in.audio_offset;
            r.rate = in.rate;
            r.bs = in.max_block;
            r.total = (uint32_t)in.total_samples;
            r.frames = (uint32_t)((in.total_samples + r.bs - 1) / r.bs);
            if (flacdec_too_short(r.frames, len - r.audio)) {
                r.frames = 0;                                                        // (k_flacdec_link: CORRUPT at the audio offset)
            } else {
                r.cand_cap = (uint32_t)std::min<u64>(2ull * r.frames + 64, (len - r.audio) / 2 + 1);      // (a header begins FF F8: two apart at least)
                tiles = (long long)((len - r.audio + FLACDEC_SCAN_TILE - 1) / FLACDEC_SCAN_TILE);
            }
            p->max_bs = std::max(p->max_bs, r.bs);
            p->pcm += r.total;
        }
        p->tile0[(size_t)c + 1] = p->tile0[(size_t)c] + tiles;
        p->cand0[(size_t)c + 1] = p->cand0[(size_t)c] + r.cand_cap;
        p->frame0[(size_t)c + 1] = p->frame0[(size_t)c] + r.frames;
    }
    if (p->cand0[(size_t)n_streams] > FLACDEC_MAX_CANDS) return "the burst holds too many frames";
    return nullptr;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout { size_t tables, zero, zero_bytes, bad, cand, total; };
Layout layout(const Plan& p) {
    const size_t n = p.rows.size(), frames = (size_t)p.frame0[n], cands = (size_t)p.cand0[n];
    Layout l;
    l.tables = 0;
    l.zero = up256(n * sizeof(FlacDecStream) + 3 * (n + 1) * 8);
    l.zero_bytes = (n + 2 * frames) * 4;
    l.bad = l.zero + up256(l.zero_bytes);
    l.cand = l.bad + up256(n * 4);
    l.total = l.cand + up256(cands * sizeof(FlacDecCand));
    return l;
}

}  // namespace

int flacdec_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples, const char** why) {
    Plan p;
    const char* w = plan(n_streams, infos, offsets, &p);
    if (why) *why = w;
    if (w) return -1;
    if (pcm_samples) *pcm_samples = p.pcm;
    return 0;
}

size_t flacdec_workspace_bytes(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets) {
    Plan p;
    if (plan(n_streams, infos, offsets, &p)) return 0;
    return layout(p).total;
}

FlacDecWork flacdec_work(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, void* d_block) {
    FlacDecWork w;
    Plan p;
    if (plan(n_streams, infos, offsets, &p)) return w;
    const Layout l = layout(p);
    const size_t n = (size_t)n_streams;
    w.n_streams = n_streams;
    w.max_bs = p.max_bs;
    w.tiles = p.tile0[n];
    w.cands = p.cand0[n];
    w.frames = p.frame0[n];
    const size_t rows_bytes = n * sizeof(FlacDecStream), pre = (n + 1) * 8;
    w.tables.resize(rows_bytes + 3 * pre);
    std::memcpy(w.tables.data(), p.rows.data(), rows_bytes);
    std::memcpy(w.tables.data() + rows_bytes, p.tile0.data(), pre);
    std::memcpy(w.tables.data() + rows_bytes + pre, p.cand0.data(), pre);
    std::memcpy(w.tables.data() + rows_bytes + 2 * pre, p.frame0.data(), pre);
    char* base = (char*)d_block;
    w.rows = (const FlacDecStream*)base;
    w.tile0 = (const long long*)(base + rows_bytes);
    w.cand0 = w.tile0 + (n + 1);
    w.frame0 = w.cand0 + (n + 1);
    w.count = (uint32_t*)(base + l.zero);
    w.head = w.count + n;
    w.chain = w.head + (size_t)w.frames;
    w.zero_bytes = l.zero_bytes;
    w.bad = (uint32_t*)(base + l.bad);
    w.cand = (FlacDecCand*)(base + l.cand);
    return w;
}

void launch_flacdec(const uint8_t* d_streams, const FlacDecWork& w, int16_t* d_pcm, size_t pcm_cap, bnhip_flac_decode_result* d_result,
                    hipStream_t s) {
    if (w.n_streams < 1) return;
    const int n = w.n_streams;
    // (a pageable source is staged before hipMemcpyAsync returns, so the host tables need not outlive the call)
    (void)hipMemcpyAsync((void*)w.rows, w.tables.data(), w.tables.size(), hipMemcpyHostToDevice, s);
    (void)hipMemsetAsync(w.count, 0, w.zero_bytes, s);
    (void)hipMemsetAsync(w.bad, 0xFF, (size_t)n * 4, s);
    const size_t frame_lds = (flacdec_frame_cap(w.max_bs ? w.max_bs : FLACDEC_MIN_BLOCK) + 15) & ~(size_t)15;
    const size_t restore_lds = frame_lds + 2 * (size_t)(w.max_bs ? w.max_bs : FLACDEC_MIN_BLOCK);
    if (w.tiles > 0)
        hipLaunchKernelGGL(k_flacdec_scan, dim3((unsigned)w.tiles), dim3(SCAN_THREADS), 0, s, d_streams, w.rows, w.tile0, n, w.count, w.cand, w.cand0);
    if (w.cands > 0) {
        lds_limit_once<&k_flacdec_parse>(160 * 1024);
        hipLaunchKernelGGL(k_flacdec_parse, dim3((unsigned)w.cands), dim3(WAVE), frame_lds, s, d_streams, w.rows, w.cand0, w.frame0, n, w.count, w.cand,
                           w.head);
    }
    hipLaunchKernelGGL(k_flacdec_link, dim3((unsigned)n), dim3(WAVE), 0, s, w.rows, w.frame0, w.count, w.cand, w.head, w.chain, d_result);
    if (w.frames > 0) {
        lds_limit_once<&k_flacdec_restore>(160 * 1024);
        hipLaunchKernelGGL(k_flacdec_restore, dim3((unsigned)w.frames), dim3(WAVE), restore_lds, s, d_streams, w.rows, w.frame0, n, w.cand, w.chain,
                           d_result, w.bad, d_pcm, (u64)pcm_cap, (uint32_t)frame_lds);
        hipLaunchKernelGGL(k_flacdec_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.frame0, n, w.cand, w.chain, w.bad, d_result);
    }
}

}  // namespace bnhip
