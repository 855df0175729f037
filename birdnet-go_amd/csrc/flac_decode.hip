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

__device__ __forceinline__ FlacStreamShape shape_of(const FlacDecStream& r) {
    return FlacStreamShape{r.rate, r.bs, r.total, r.frames, r.channels, r.bits};
}

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

// Grid: the burst's candidate slots, a wavefront each.  Dynamic LDS: the burst's largest frame cap.  Wide: the burst holds a stream
// that is not mono 16-bit, and every frame is read as its stream's channels and depth say.
template <bool Wide>
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
    const uint32_t staged = stage_frame(streams, r, cd.start, Wide ? flacdec_frame_cap(r.bs, r.channels, r.bits) : flacdec_frame_cap(r.bs),
                                        flacdec_sm, lane);
    __syncthreads();
    if (lane == 0) {
        FlacCountSink sink;
        size_t bytes = 0;
        uint32_t rc = (uint32_t)FLACP_INVALID, assign = 0;
        if (cd.head_bytes <= staged && cd.bs <= r.bs)
            rc = Wide ? (uint32_t)flac_parse_frame_wide(flacdec_sm, staged, cd.head_bytes, cd.bs, shape_of(r), sink, &bytes, &assign)
                      : (uint32_t)flac_parse_frame(flacdec_sm, staged, cd.head_bytes, cd.bs, sink, &bytes);
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

// Byte q of a frame's interleaved PCM at `bytes` per sample, from its samples xs [channels][stride]
__device__ __forceinline__ uint32_t pcm_byte(const int32_t* __restrict__ xs, uint32_t stride, uint32_t channels, uint32_t bytes, uint32_t q) {
    const uint32_t smp = bytes == 2 ? q >> 1 : q / 3u, k = q - smp * bytes;
    const uint32_t i = channels == 2 ? smp >> 1 : smp, ch = channels == 2 ? smp & 1u : 0u;
    return ((uint32_t)xs[ch * stride + i] >> (8u * k)) & 0xFFu;
}

// Grid: the burst's frames, a wavefront each.  Dynamic LDS: the frame's bytes, then its samples: int16 [the burst's largest block
// size], or Wide int32 [channels][a stream's block size].  partial: the frames of a chain that broke are restored too.
template <bool Wide>
__global__ __launch_bounds__(WAVE) void k_flacdec_restore(const uint8_t* __restrict__ streams, const FlacDecStream* __restrict__ rows,
                                                          const long long* __restrict__ frame0, int n_streams,
                                                          const FlacDecCand* __restrict__ cand, const uint32_t* __restrict__ chain,
                                                          const bnhip_flac_decode_result* __restrict__ result, uint32_t* __restrict__ bad,
                                                          uint8_t* __restrict__ pcm, u64 pcm_cap, uint32_t sample_off, int partial) {
    extern __shared__ __attribute__((aligned(16))) uint8_t flacdec_sm[];
    __shared__ uint32_t s_rc;
    __shared__ int32_t s_coef[FLACDEC_MAX_ORDER];
    const int lane = threadIdx.x;
    const long long f = (long long)blockIdx.x;
    const int c = ragged_clip(frame0, n_streams, f);
    const int32_t status = result[c].status;
    if (status != BNHIP_FLAC_OK && !(partial && status == BNHIP_FLAC_CORRUPT)) return;       // (block-uniform)
    const FlacDecStream r = rows[c];
    const uint32_t j = (uint32_t)(f - frame0[c]);
    const uint32_t idx = chain[f];
    if (!idx) return;
    const FlacDecCand cd = cand[idx - 1];
    if (cd.end <= cd.start || cd.end - cd.start > (Wide ? flacdec_frame_cap(r.bs, r.channels, r.bits) : flacdec_frame_cap(r.bs)) || cd.bs > r.bs ||
        cd.number != j)
        return;
    const uint32_t staged = stage_frame(streams, r, cd.start, cd.end - cd.start, flacdec_sm, lane);
    __syncthreads();
    const u64 first = (u64)j * r.bs;                                                 // of the clip
    if constexpr (Wide) {
        __shared__ uint32_t s_assign;
        int32_t* xw = reinterpret_cast<int32_t*>(flacdec_sm + sample_off);
        const uint32_t stride = r.bs;
        if (lane == 0) {
            FlacWideSink sink{xw, s_coef, stride, 0u};
            size_t bytes = 0;
            uint32_t assign = 0;
            s_rc = cd.head_bytes <= staged ? (uint32_t)flac_parse_frame_wide(flacdec_sm, staged, cd.head_bytes, cd.bs, shape_of(r), sink, &bytes, &assign)
                                           : (uint32_t)FLACP_INVALID;
            s_assign = assign;
        }
        __syncthreads();
        int out_of_range = 0;
        if (s_rc == FLACP_OK && s_assign >= 8u) {
            for (uint32_t i = (uint32_t)lane; i < cd.bs; i += WAVE) {
                int32_t left, right;
                if (!flac_decorrelate(s_assign, xw[i], xw[stride + i], r.bits, &left, &right)) out_of_range = 1;
                xw[i] = left;
                xw[stride + i] = right;
            }
        }
        out_of_range = __syncthreads_or(out_of_range);
        if (s_rc != FLACP_OK || out_of_range) {
            if (lane == 0) atomicMin(&bad[c], j);
            return;
        }
        // the frame's bytes of the recording's span: single bytes up to a 4-byte line of the address and behind the last one, whole
        // words between; every byte of [o0, o1) is stored once and none outside it
        const uint32_t bytes = r.bits / 8u, pitch = bytes * r.channels;
        const u64 span = (u64)r.total * pitch;
        u64 o0 = first * pitch, o1 = o0 + (u64)cd.bs * pitch;
        if (o1 > span) o1 = span;
        if (r.pcm0 > pcm_cap || span > pcm_cap - r.pcm0 || o0 >= o1) return;
        uint8_t* dst = pcm + r.pcm0;                                                 // byte q of the span at dst[q]
        const uint32_t lead = (uint32_t)((4u - (uint32_t)((uintptr_t)(dst + o0) & 3u)) & 3u);
        const u64 a0 = o0 + lead < o1 ? o0 + lead : o1;
        const u64 a1 = a0 + ((o1 - a0) & ~(u64)3);
        for (u64 q = o0 + (u64)lane; q < a0; q += WAVE) dst[q] = (uint8_t)pcm_byte(xw, stride, r.channels, bytes, (uint32_t)(q - o0));
        for (u64 q = a0 + 4u * (u64)lane; q < a1; q += 4u * WAVE) {
            const uint32_t at = (uint32_t)(q - o0);
            const uint32_t v = pcm_byte(xw, stride, r.channels, bytes, at) | (pcm_byte(xw, stride, r.channels, bytes, at + 1) << 8) |
                               (pcm_byte(xw, stride, r.channels, bytes, at + 2) << 16) | (pcm_byte(xw, stride, r.channels, bytes, at + 3) << 24);
            *reinterpret_cast<uint32_t*>(dst + q) = v;
        }
        for (u64 q = a1 + (u64)lane; q < o1; q += WAVE) dst[q] = (uint8_t)pcm_byte(xw, stride, r.channels, bytes, (uint32_t)(q - o0));
        return;
    }
    int16_t* xs = reinterpret_cast<int16_t*>(flacdec_sm + sample_off);
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
    int16_t* pcm16 = reinterpret_cast<int16_t*>(pcm);
    const u64 s0 = r.pcm0 / 2, cap16 = pcm_cap / 2;
    for (uint32_t i = (uint32_t)lane; i < cd.bs; i += WAVE) {
        const u64 at = first + i;
        if (at < r.total && s0 + at < cap16) pcm16[s0 + at] = xs[i];
    }
}

__global__ __launch_bounds__(256) void k_flacdec_finish(const long long* __restrict__ frame0, int n_streams, const FlacDecCand* __restrict__ cand,
                                                        const uint32_t* __restrict__ chain, const uint32_t* __restrict__ bad,
                                                        bnhip_flac_decode_result* __restrict__ result) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_streams || bad[c] == 0xFFFFFFFFu) return;
    // (a chain that broke and was restored in part: a frame in front of the break that failed is the earlier failure)
    const bnhip_flac_decode_result was = result[c];
    if (was.status != BNHIP_FLAC_OK && !(was.status == BNHIP_FLAC_CORRUPT && bad[c] < (uint32_t)was.frames)) return;
    const uint32_t idx = chain[frame0[c] + bad[c]];
    result[c] = bnhip_flac_decode_result{BNHIP_FLAC_CORRUPT, (int32_t)bad[c], idx ? cand[idx - 1].start : 0ull};
}

struct Plan {
    std::vector<FlacDecStream> rows;
    std::vector<long long> tile0, cand0, frame0;
    uint32_t max_bs = 0;
    size_t pcm = 0;                                     // samples, or bytes of a recordings burst
    bool wide = false;
    size_t frame_cap = 0, sample_lds = 0;               // the largest frame of the burst: its bytes' bound, its samples in LDS
};

// -> NULL, or why the burst cannot run
const char* plan(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, bool recordings, Plan* p) {
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
        r.pcm0 = recordings ? p->pcm : 2 * p->pcm;
        r.status = in.status;
        long long tiles = 0;
        if (in.status == BNHIP_FLAC_OK) {
            const u64 len = r.end - r.begin;
            const bool clip = in.channels == 1 && in.bits == 16;
            if (!(clip || (recordings && in.channels >= 1 && in.channels <= 2 && (in.bits == 16 || in.bits == 24))) || in.total_samples < 1 ||
                in.total_samples > 0x7FFFFFFFull || in.max_block < FLACDEC_MIN_BLOCK ||
                in.max_block > (clip ? FLACDEC_MAX_BLOCK : FLACDEC_MAX_BLOCK_WIDE) || in.audio_offset > len)
                return recordings ? "a stream's info is marked BNHIP_FLAC_OK but is not one bnhip_flac_recording_info accepts"
                                  : "a stream's info is marked BNHIP_FLAC_OK but is not one bnhip_flac_stream_info accepts";
            r.channels = in.channels;
            r.bits = in.bits;
            p->wide = p->wide || !clip;
            r.audio = in.audio_offset;
            r.rate = in.rate;
            r.bs = in.max_block;
            r.total = (uint32_t)in.total_samples;
            r.frames = (uint32_t)((in.total_samples + r.bs - 1) / r.bs);
            if (clip ? flacdec_too_short(r.frames, len - r.audio) : flacdec_too_short(r.frames, len - r.audio, r.channels, r.bits)) {
                r.frames = 0;                                                        // (k_flacdec_link: CORRUPT at the audio offset)
            } else {
                r.cand_cap = (uint32_t)std::min<u64>(2ull * r.frames + 64, (len - r.audio) / 2 + 1);      // (a header begins FF F8: two apart at least)
                tiles = (long long)((len - r.audio + FLACDEC_SCAN_TILE - 1) / FLACDEC_SCAN_TILE);
            }
            p->max_bs = std::max(p->max_bs, r.bs);
            p->frame_cap = std::max(p->frame_cap, flacdec_frame_cap(r.bs, r.channels, r.bits));
            p->sample_lds = std::max(p->sample_lds, (size_t)r.bs * r.channels * 4);
            p->pcm += recordings ? flacdec_pcm_bytes(in) : (size_t)r.total;
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

int flacdec_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples, const char** why,
                  bool recordings) {
    Plan p;
    const char* w = plan(n_streams, infos, offsets, recordings, &p);
    if (why) *why = w;
    if (w) return -1;
    if (pcm_samples) *pcm_samples = p.pcm;
    return 0;
}

size_t flacdec_workspace_bytes(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, bool recordings) {
    Plan p;
    if (plan(n_streams, infos, offsets, recordings, &p)) return 0;
    return layout(p).total;
}

void flacdec_place(FlacDecWork& w, int stream, unsigned long long pcm_byte) {
    reinterpret_cast<FlacDecStream*>(w.tables.data())[stream].pcm0 = pcm_byte;
}

FlacDecWork flacdec_work(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, void* d_block, bool recordings) {
    FlacDecWork w;
    Plan p;
    if (plan(n_streams, infos, offsets, recordings, &p)) return w;
    const Layout l = layout(p);
    const size_t n = (size_t)n_streams;
    w.n_streams = n_streams;
    w.max_bs = p.max_bs;
    w.wide = p.wide;
    w.recordings = recordings;
    // (mono 16-bit bursts: the clips' sizes, 2 bs + 32 and int16 [bs])
    const uint32_t bs = p.max_bs ? p.max_bs : FLACDEC_MIN_BLOCK;
    w.frame_lds = ((p.wide ? p.frame_cap : flacdec_frame_cap(bs)) + 15) & ~(size_t)15;
    w.sample_lds = p.wide ? p.sample_lds : 2 * (size_t)bs;
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

void launch_flacdec(const uint8_t* d_streams, const FlacDecWork& w, void* d_pcm, size_t pcm_cap, bnhip_flac_decode_result* d_result,
                    hipStream_t s) {
    if (w.n_streams < 1) return;
    const int n = w.n_streams;
    // (a pageable source is staged before hipMemcpyAsync returns, so the host tables need not outlive the call)
    (void)hipMemcpyAsync((void*)w.rows, w.tables.data(), w.tables.size(), hipMemcpyHostToDevice, s);
    (void)hipMemsetAsync(w.count, 0, w.zero_bytes, s);
    (void)hipMemsetAsync(w.bad, 0xFF, (size_t)n * 4, s);
    const size_t frame_lds = w.frame_lds, restore_lds = w.frame_lds + w.sample_lds;
    uint8_t* pcm = static_cast<uint8_t*>(d_pcm);
    const int partial = w.recordings ? 1 : 0;
    if (w.tiles > 0)
        hipLaunchKernelGGL(k_flacdec_scan, dim3((unsigned)w.tiles), dim3(SCAN_THREADS), 0, s, d_streams, w.rows, w.tile0, n, w.count, w.cand, w.cand0);
    if (w.cands > 0) {
        if (w.wide) {
            lds_limit_once<&k_flacdec_parse<true>>(160 * 1024);
            hipLaunchKernelGGL(k_flacdec_parse<true>, dim3((unsigned)w.cands), dim3(WAVE), frame_lds, s, d_streams, w.rows, w.cand0, w.frame0, n,
                               w.count, w.cand, w.head);
        } else {
            lds_limit_once<&k_flacdec_parse<false>>(160 * 1024);
            hipLaunchKernelGGL(k_flacdec_parse<false>, dim3((unsigned)w.cands), dim3(WAVE), frame_lds, s, d_streams, w.rows, w.cand0, w.frame0, n,
                               w.count, w.cand, w.head);
        }
    }
    hipLaunchKernelGGL(k_flacdec_link, dim3((unsigned)n), dim3(WAVE), 0, s, w.rows, w.frame0, w.count, w.cand, w.head, w.chain, d_result);
    if (w.frames > 0) {
        if (w.wide) {
            lds_limit_once<&k_flacdec_restore<true>>(160 * 1024);
            hipLaunchKernelGGL(k_flacdec_restore<true>, dim3((unsigned)w.frames), dim3(WAVE), restore_lds, s, d_streams, w.rows, w.frame0, n, w.cand,
                               w.chain, d_result, w.bad, pcm, (u64)pcm_cap, (uint32_t)frame_lds, partial);
        } else {
            lds_limit_once<&k_flacdec_restore<false>>(160 * 1024);
            hipLaunchKernelGGL(k_flacdec_restore<false>, dim3((unsigned)w.frames), dim3(WAVE), restore_lds, s, d_streams, w.rows, w.frame0, n, w.cand,
                               w.chain, d_result, w.bad, pcm, (u64)pcm_cap, (uint32_t)frame_lds, partial);
        }
        hipLaunchKernelGGL(k_flacdec_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.frame0, n, w.cand, w.chain, w.bad, d_result);
    }
}

}  // namespace bnhip
