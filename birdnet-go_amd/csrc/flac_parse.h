// The FLAC frame reader of the device decoder (flac_decode.hip) stated once, as host and device inline code: the frame header test,
// the bit reader over a bounded byte span, the subframe and residual readers and the predictor, written from RFC 9639 for streams
// of fixed block size: mono 16-bit clips (flac_parse_frame, int16 samples and int32 products) and recordings of 1 or 2 channels
// at 16 or 24 bits (flac_parse_frame_wide, int32 samples and 64-bit products, the stereo decorrelation beside it).  The kernels
// and plain g++ builds (tests/native/flac_parse_main.cpp and flac_parse_wide_main.cpp, under ASan + UBSan) compile this one
// statement.  Nothing here reads outside the span it is given, loops longer than the block size or the span's bits allow, or
// relies on signed overflow or a negative shift: prediction sums are int64, the wasted-bit shift is a multiply.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/bnhip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FLACP_HD __host__ __device__ inline
#else
#define FLACP_HD inline
#endif

namespace bnhip {

constexpr uint32_t FLACDEC_MIN_BLOCK = 16, FLACDEC_MAX_BLOCK = 16384;     // STREAMINFO block sizes that are decoded
// ... of a wide stream (anything but mono 16-bit): its frame's bytes and its int32 samples lie side by side in LDS (flac_decode.h)
constexpr uint32_t FLACDEC_MAX_BLOCK_WIDE = 8192;
constexpr uint32_t FLACDEC_HEAD_MAX = 16;          // sync and codes 4, coded number 7, explicit block size 2, explicit rate 2, CRC-8 1
constexpr uint32_t FLACDEC_MAX_ORDER = 32;
// The bytes a frame of bs samples is read within: the VERBATIM bound.  A frame that needs more is not a frame.
FLACP_HD size_t flacdec_frame_cap(uint32_t bs) { return 2 * (size_t)bs + 32; }
// ... of a stream of `channels` at `bits`: bs x channels x bytes, a stereo frame's side channel taking one bit more per sample
FLACP_HD size_t flacdec_frame_cap(uint32_t bs, uint32_t channels, uint32_t bits) {
    return (size_t)bs * channels * (bits / 8) + (channels == 2 ? (size_t)bs / 8 + 1 : 0) + 32;
}

// No frame is shorter: a 6-byte header, a CONSTANT subframe's 3 bytes, CRC-16.  A stream whose STREAMINFO promises more frames than its
// audio bytes can hold is CORRUPT at its audio offset without a look at the bytes, so a sample count in a damaged file sizes nothing.
constexpr uint32_t FLACDEC_MIN_FRAME = 11;
FLACP_HD bool flacdec_too_short(uint64_t frames, uint64_t audio_bytes) { return frames > audio_bytes / FLACDEC_MIN_FRAME; }
// ... of a stream of `channels` at `bits`: a CONSTANT subframe per channel (independent channels: the shortest); 11 for mono 16
FLACP_HD uint32_t flacdec_min_frame(uint32_t channels, uint32_t bits) { return 6u + channels * (1u + bits / 8u) + 2u; }
FLACP_HD bool flacdec_too_short(uint64_t frames, uint64_t audio_bytes, uint32_t channels, uint32_t bits) {
    return frames > audio_bytes / flacdec_min_frame(channels, bits);
}

enum { FLACP_OK = 0, FLACP_INVALID = 1, FLACP_RANGE = 2 };     // a frame's parse: fine, not a frame, a sample outside the depth

// What a stream's STREAMINFO holds every frame header to.
struct FlacStreamShape {
    uint32_t rate, bs, total, frames;               // frames = ceil(total / bs)
    uint32_t channels = 1, bits = 16;               // 1 or 2; 16 or 24
};
struct FlacFrameHead {
    uint32_t number, bs, bytes;                     // bytes: the header's, CRC-8 included
};

FLACP_HD uint32_t flac_crc8_step(uint32_t crc, uint32_t byte) {
    crc ^= byte;
    for (int i = 0; i < 8; i++) crc = ((crc << 1) ^ ((crc & 0x80u) ? 0x07u : 0u)) & 0xffu;
    return crc;
}
FLACP_HD uint32_t flac_crc16_step(uint32_t crc, uint32_t byte) {
    crc ^= byte << 8;
    for (int i = 0; i < 8; i++) crc = ((crc << 1) ^ ((crc & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
    return crc;
}
// a * b mod x^16 + x^15 + x^2 + 1: crc(A || B) = crc(A) x^(8 |B|) ^ crc(B)
FLACP_HD uint32_t flac_crc16_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
FLACP_HD uint32_t flac_crc16(const uint8_t* p, size_t n) {
    uint32_t crc = 0;
    for (size_t i = 0; i < n; i++) crc = flac_crc16_step(crc, p[i]);
    return crc;
}

// Is p[0 .. avail) the start of a frame header of this stream?  Sync with the blocking-strategy and reserved bits clear, no reserved
// code, the stream's channel count (mono: code 0; stereo: independent 1, left/side 8, side/right 9, mid/side 10) and depth (its
// size code or "as STREAMINFO"), the stream's rate, a well-formed coded number below the frame count, the block size that
// frame must have (bs, or the remainder in the last frame), CRC-8.  avail is what is left of the stream.
FLACP_HD bool flac_frame_head(const uint8_t* p, size_t avail, const FlacStreamShape& s, FlacFrameHead* h) {
    if (avail < 6) return false;
    if (p[0] != 0xFFu || p[1] != 0xF8u) return false;
    const uint32_t bs_code = p[2] >> 4, rate_code = p[2] & 15u, channels = p[3] >> 4, size_code = (p[3] >> 1) & 7u;
    if ((p[3] & 1u) || bs_code == 0 || rate_code == 15) return false;
    if (s.channels == 1 ? channels != 0 : (channels != 1 && channels != 8 && channels != 9 && channels != 10)) return false;
    if (size_code != 0 && size_code != (s.bits == 16 ? 4u : 6u)) return false;
    const uint32_t b0 = p[4];
    uint32_t nb = 1;
    uint64_t number = b0;
    if (b0 >= 0x80u) {
        nb = 0;
        while (nb < 8 && (b0 & (0x80u >> nb))) nb++;                 // leading ones
        if (nb < 2 || nb > 7 || 4 + (size_t)nb > avail) return false;
        number = nb < 7 ? (b0 & ((1u << (7 - nb)) - 1u)) : 0u;
        for (uint32_t j = 1; j < nb; j++) {
            if ((p[4 + j] & 0xC0u) != 0x80u) return false;
            number = (number << 6) | (p[4 + j] & 0x3Fu);
        }
    }
    if (number >= s.frames) return false;
    size_t q = 4 + (size_t)nb;
    const size_t extra = (bs_code == 6 ? 1u : bs_code == 7 ? 2u : 0u) + (rate_code == 12 ? 1u : rate_code >= 13 ? 2u : 0u);
    if (q + extra + 1 > avail) return false;
    uint32_t bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576u << (bs_code - 2);
    else if (bs_code == 6) { bs = (uint32_t)p[q] + 1u; q += 1; }
    else if (bs_code == 7) { bs = (((uint32_t)p[q] << 8) | p[q + 1]) + 1u; q += 2; }
    else bs = 256u << (bs_code - 8);
    const uint64_t first = number * (uint64_t)s.bs;                  // (below total: number < frames)
    const uint64_t want = number + 1 == s.frames ? (uint64_t)s.total - first : (uint64_t)s.bs;
    if ((uint64_t)bs != want) return false;
    uint32_t rate;
    switch (rate_code) {
        case 0: rate = s.rate; break;
        case 1: rate = 88200; break;
        case 2: rate = 176400; break;
        case 3: rate = 192000; break;
        case 4: rate = 8000; break;
        case 5: rate = 16000; break;
        case 6: rate = 22050; break;
        case 7: rate = 24000; break;
        case 8: rate = 32000; break;
        case 9: rate = 44100; break;
        case 10: rate = 48000; break;
        case 11: rate = 96000; break;
        case 12: rate = (uint32_t)p[q] * 1000u; q += 1; break;
        case 13: rate = ((uint32_t)p[q] << 8) | p[q + 1]; q += 2; break;
        default: rate = (((uint32_t)p[q] << 8) | p[q + 1]) * 10u; q += 2; break;
    }
    if (rate != s.rate) return false;
    uint32_t crc = 0;
    for (size_t i = 0; i < q; i++) crc = flac_crc8_step(crc, p[i]);
    if (crc != p[q]) return false;
    h->number = (uint32_t)number;
    h->bs = bs;
    h->bytes = (uint32_t)q + 1u;
    return true;
}

// Bits of p[0 .. n), most significant first, through a 64-bit buffer whose top `cnt` bits are the next ones and whose other bits are
// zero.  A read past the span sets `fail` and returns 0; it never touches p[n].
struct FlacBits {
    const uint8_t* p;
    size_t n, pos;                                  // pos: the next byte to load
    uint64_t buf;
    int cnt;
    bool fail;
    FLACP_HD void init(const uint8_t* bytes, size_t len, size_t start) { p = bytes; n = len; pos = start < len ? start : len; buf = 0; cnt = 0; fail = false; }
    // single bytes up to a 4-byte boundary of the address (and for the span's last bytes), whole words between
    FLACP_HD void fill() {
        while (cnt <= 56 && pos < n && ((((uintptr_t)(p + pos)) & 3u) != 0 || pos + 4 > n)) { buf |= (uint64_t)p[pos++] << (56 - cnt); cnt += 8; }
        if (cnt <= 32 && pos + 4 <= n) {
            uint32_t w;
            __builtin_memcpy(&w, __builtin_assume_aligned(p + pos, 4), 4);
            buf |= (uint64_t)__builtin_bswap32(w) << (32 - cnt);
            cnt += 32;
            pos += 4;
        }
    }
    FLACP_HD uint32_t take(int k) {                 // k in 0..32
        if (k <= 0) return 0;
        if (cnt < k) {
            fill();
            if (cnt < k) { fail = true; cnt = 0; buf = 0; return 0; }
        }
        const uint32_t v = (uint32_t)(buf >> (64 - k));
        buf <<= k;
        cnt -= k;
        return v;
    }
    FLACP_HD int64_t stake(int k) {                 // k in 1..32, two's complement
        const uint32_t v = take(k);
        return (int64_t)v - (int64_t)((uint64_t)(v >> (k - 1)) << k);
    }
    // the zeros before the next one, which is consumed; a run that reaches the end of the span fails
    FLACP_HD uint32_t unary() {
        uint32_t q = 0;
        for (;;) {
            if (cnt == 0) {
                fill();
                if (cnt == 0) { fail = true; return 0; }
            }
            if (buf == 0) { q += (uint32_t)cnt; cnt = 0; continue; }
            const int z = __builtin_clzll(buf);     // (below cnt: the bits under the top cnt are zero)
            q += (uint32_t)z;
            buf <<= z;
            buf <<= 1;
            cnt -= z + 1;
            return q;
        }
    }
    FLACP_HD size_t bits_read() const { return pos * 8 - (size_t)cnt; }
};

// Where a frame's samples go.  The count-only sink parses a frame to its end without predicting; the store sink keeps the samples
// (before the wasted-bit shift, which the reader applies at the end) where the predictor reads them back.
struct FlacCountSink {
    static constexpr bool kStore = false, kWide = false;
    FLACP_HD void channel(uint32_t) {}
    FLACP_HD void put(uint32_t, int32_t) {}
    FLACP_HD int32_t get(uint32_t) const { return 0; }
    FLACP_HD void set_coef(uint32_t, int32_t) {}
    FLACP_HD int32_t coef(uint32_t) const { return 0; }
};
struct FlacStoreSink {
    static constexpr bool kStore = true, kWide = false;     // kWide: a coefficient times a sample needs 64 bits
    int16_t* x;                                     // [the block size]
    int32_t* c;                                     // [FLACDEC_MAX_ORDER] the predictor's coefficients (beside x: LDS on the device)
    FLACP_HD void put(uint32_t i, int32_t v) { x[i] = (int16_t)v; }
    FLACP_HD int32_t get(uint32_t i) const { return x[i]; }
    FLACP_HD void set_coef(uint32_t j, int32_t v) { c[j] = v; }
    FLACP_HD int32_t coef(uint32_t j) const { return c[j]; }
};
// ... of a recording's frame: int32 samples (up to 25 bits: a 24-bit stream's side channel), channel ch at x + ch * stride
struct FlacWideSink {
    static constexpr bool kStore = true, kWide = true;
    int32_t* x;                                     // [channels][stride]
    int32_t* c;                                     // [FLACDEC_MAX_ORDER]
    uint32_t stride, base;
    FLACP_HD void channel(uint32_t ch) { base = ch * stride; }
    FLACP_HD void put(uint32_t i, int32_t v) { x[base + i] = v; }
    FLACP_HD int32_t get(uint32_t i) const { return x[base + i]; }
    FLACP_HD void set_coef(uint32_t j, int32_t v) { c[j] = v; }
    FLACP_HD int32_t coef(uint32_t j) const { return c[j]; }
};

// One subframe of bs samples at `depth` bits (the stream's, or one more for a side channel) into the sink's current channel, the
// wasted-bit shift applied.  -> FLACP_OK, FLACP_INVALID for anything that is not a subframe, or FLACP_RANGE (store sinks only) when
// a predicted sample does not fit the depth.  Sink::kWide chooses the product's width at compile time: the residual loop holds no
// run-time branch on it.
template <class Sink>
FLACP_HD int flac_parse_subframe(FlacBits& b, uint32_t bs, int depth, Sink& sink) {
    if (b.take(1)) return FLACP_INVALID;
    const uint32_t kind = b.take(6);
    uint32_t wasted = 0;
    if (b.take(1)) wasted = b.unary() + 1u;
    if (b.fail || wasted >= (uint32_t)depth) return FLACP_INVALID;
    const int bps = depth - (int)wasted;
    const int64_t lim = (int64_t)1 << (bps - 1);
    if (kind == 0) {
        const int64_t v = b.stake(bps);
        if (Sink::kStore) for (uint32_t i = 0; i < bs; i++) sink.put(i, (int32_t)v);
    } else if (kind == 1) {
        for (uint32_t i = 0; i < bs && !b.fail; i++) sink.put(i, (int32_t)b.stake(bps));
    } else if ((kind >= 8 && kind <= 12) || kind >= 32) {
        const bool lpc = kind >= 32;
        const uint32_t order = lpc ? kind - 31 : kind - 8;
        if (order > bs) return FLACP_INVALID;
        for (uint32_t i = 0; i < order; i++) sink.put(i, (int32_t)b.stake(bps));
        int shift = 0;
        if (lpc) {
            const int precision = (int)b.take(4) + 1;
            if (precision == 16) return FLACP_INVALID;
            shift = (int)b.stake(5);
            if (shift < 0) return FLACP_INVALID;
            for (uint32_t j = 0; j < order; j++) sink.set_coef(j, (int32_t)b.stake(precision));
        } else {
            const int32_t fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
            for (uint32_t j = 0; j < order; j++) sink.set_coef(j, fixed[order][j]);
        }
        const uint32_t method = b.take(2);
        if (method > 1) return FLACP_INVALID;
        const int pbits = method ? 5 : 4;
        const uint32_t esc = method ? 31 : 15;
        const uint32_t porder = b.take(4);
        if (b.fail || (bs & ((1u << porder) - 1u)) != 0 || (bs >> porder) < order) return FLACP_INVALID;
        // Orders up to 8 (every FIXED predictor, and the LPC orders of this project's encoder) keep the coefficients and the last 8
        // samples in registers; longer predictors read both back from the sink.
        constexpr uint32_t kWin = 8;
        const bool window = Sink::kStore && order <= kWin;
        int32_t cw[kWin], hw[kWin];
#if defined(__clang__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < kWin; j++) {
            cw[j] = window && j < order ? sink.coef(j) : 0;
            hw[j] = window && j < order ? sink.get(order - 1 - j) : 0;
        }
        uint32_t i = order;
        for (uint32_t part = 0; part < (1u << porder); part++) {
            const uint32_t count = (bs >> porder) - (part == 0 ? order : 0u);
            const uint32_t k = b.take(pbits);
            const uint32_t width = k == esc ? b.take(5) : 0u;
            if (b.fail) return FLACP_INVALID;
            for (uint32_t c = 0; c < count; c++, i++) {
                int64_t r;
                if (k == esc) {
                    r = width ? b.stake((int)width) : 0;
                } else {
                    const uint64_t u = ((uint64_t)b.unary() << k) | b.take((int)k);
                    r = (int64_t)(u >> 1) ^ -(int64_t)(u & 1u);
                }
                if (b.fail) return FLACP_INVALID;
                if (Sink::kStore) {
                    int64_t pred = 0;
                    // (a coefficient has at most 15 bits and a kept sample 16: the product fits 32; a wide sink's samples have up
                    // to 25 bits, its products 40, a sum of 32 of them 45)
                    if (window) {
#if defined(__clang__)
#pragma unroll
#endif
                        for (uint32_t j = 0; j < kWin; j++) pred += Sink::kWide ? (int64_t)cw[j] * hw[j] : (int64_t)(cw[j] * hw[j]);
                    } else {
                        for (uint32_t j = 0; j < order; j++)
                            pred += Sink::kWide ? (int64_t)sink.coef(j) * sink.get(i - 1 - j) : (int64_t)(sink.coef(j) * sink.get(i - 1 - j));
                    }
                    const int64_t v = r + (pred >> shift);
                    if (v < -lim || v >= lim) return FLACP_RANGE;
                    sink.put(i, (int32_t)v);
#if defined(__clang__)
#pragma unroll
#endif
                    for (uint32_t j = kWin - 1; j > 0; j--) hw[j] = hw[j - 1];
                    hw[0] = (int32_t)v;
                }
            }
        }
    } else {
        return FLACP_INVALID;                       // a reserved subframe type
    }
    if (b.fail) return FLACP_INVALID;
    if (Sink::kStore && wasted)
        for (uint32_t i = 0; i < bs; i++) sink.put(i, sink.get(i) * (int32_t)(1u << wasted));
    return FLACP_OK;
}

// the zero padding to the byte behind a frame's last subframe and the room for its CRC-16 -> FLACP_OK with *frame_bytes set
FLACP_HD int flac_frame_end(FlacBits& b, size_t n, size_t* frame_bytes) {
    const int pad = (int)((8 - (b.bits_read() & 7)) & 7);
    if (b.take(pad) != 0 || b.fail) return FLACP_INVALID;
    const size_t body = b.bits_read() / 8;
    if (body + 2 > n) return FLACP_INVALID;
    *frame_bytes = body + 2;
    return FLACP_OK;
}

// The clips' reader: the mono 16-bit frame as one function of its own, beside the recordings' reader (flac_parse_subframe above,
// flac_parse_frame_wide below) and not on top of it.  Stated through the shared subframe reader the same arithmetic compiled to more scalar registers in both
// clip kernels (the restore at the register file's limit, with spills) and the clip decoder lost 13 % ("FLAC
// recordings"); a change to one reader is made to the other.
// The frame whose header (head_bytes long, already tested) starts p[0 .. n): one subframe of bs samples, zero padding to the byte.
// -> FLACP_OK with *frame_bytes = the frame's length, CRC-16 included (which the caller checks: it lies inside the span), FLACP_INVALID
// for anything that is not a frame, or FLACP_RANGE (store sink only) when a sample does not fit 16 bits.
template <class Sink>
FLACP_HD int flac_parse_frame(const uint8_t* p, size_t n, uint32_t head_bytes, uint32_t bs, Sink& sink, size_t* frame_bytes) {
    FlacBits b;
    b.init(p, n, head_bytes);
    if (b.take(1)) return FLACP_INVALID;
    const uint32_t kind = b.take(6);
    uint32_t wasted = 0;
    if (b.take(1)) wasted = b.unary() + 1u;
    if (b.fail || wasted > 15) return FLACP_INVALID;
    const int bps = 16 - (int)wasted;
    const int64_t lim = (int64_t)1 << (bps - 1);
    if (kind == 0) {
        const int64_t v = b.stake(bps);
        if (Sink::kStore) for (uint32_t i = 0; i < bs; i++) sink.put(i, (int32_t)v);
    } else if (kind == 1) {
        for (uint32_t i = 0; i < bs && !b.fail; i++) sink.put(i, (int32_t)b.stake(bps));
    } else if ((kind >= 8 && kind <= 12) || kind >= 32) {
        const bool lpc = kind >= 32;
        const uint32_t order = lpc ? kind - 31 : kind - 8;
        if (order > bs) return FLACP_INVALID;
        for (uint32_t i = 0; i < order; i++) sink.put(i, (int32_t)b.stake(bps));
        int shift = 0;
        if (lpc) {
            const int precision = (int)b.take(4) + 1;
            if (precision == 16) return FLACP_INVALID;
            shift = (int)b.stake(5);
            if (shift < 0) return FLACP_INVALID;
            for (uint32_t j = 0; j < order; j++) sink.set_coef(j, (int32_t)b.stake(precision));
        } else {
            const int32_t fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
            for (uint32_t j = 0; j < order; j++) sink.set_coef(j, fixed[order][j]);
        }
        const uint32_t method = b.take(2);
        if (method > 1) return FLACP_INVALID;
        const int pbits = method ? 5 : 4;
        const uint32_t esc = method ? 31 : 15;
        const uint32_t porder = b.take(4);
        if (b.fail || (bs & ((1u << porder) - 1u)) != 0 || (bs >> porder) < order) return FLACP_INVALID;
        // Orders up to 8 (every FIXED predictor, and the LPC orders of this project's encoder) keep the coefficients and the last 8
        // samples in registers; longer predictors read both back from the sink.
        constexpr uint32_t kWin = 8;
        const bool window = Sink::kStore && order <= kWin;
        int32_t cw[kWin], hw[kWin];
#if defined(__clang__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < kWin; j++) {
            cw[j] = window && j < order ? sink.coef(j) : 0;
            hw[j] = window && j < order ? sink.get(order - 1 - j) : 0;
        }
        uint32_t i = order;
        for (uint32_t part = 0; part < (1u << porder); part++) {
            const uint32_t count = (bs >> porder) - (part == 0 ? order : 0u);
            const uint32_t k = b.take(pbits);
            const uint32_t width = k == esc ? b.take(5) : 0u;
            if (b.fail) return FLACP_INVALID;
            for (uint32_t c = 0; c < count; c++, i++) {
                int64_t r;
                if (k == esc) {
                    r = width ? b.stake((int)width) : 0;
                } else {
                    const uint64_t u = ((uint64_t)b.unary() << k) | b.take((int)k);
                    r = (int64_t)(u >> 1) ^ -(int64_t)(u & 1u);
                }
                if (b.fail) return FLACP_INVALID;
                if (Sink::kStore) {
                    int64_t pred = 0;
                    // (a coefficient has at most 15 bits and a kept sample 16: the product fits 32)
                    if (window) {
#if defined(__clang__)
#pragma unroll
#endif
                        for (uint32_t j = 0; j < kWin; j++) pred += (int64_t)(cw[j] * hw[j]);
                    } else {
                        for (uint32_t j = 0; j < order; j++) pred += (int64_t)(sink.coef(j) * sink.get(i - 1 - j));
                    }
                    const int64_t v = r + (pred >> shift);
                    if (v < -lim || v >= lim) return FLACP_RANGE;
                    sink.put(i, (int32_t)v);
#if defined(__clang__)
#pragma unroll
#endif
                    for (uint32_t j = kWin - 1; j > 0; j--) hw[j] = hw[j - 1];
                    hw[0] = (int32_t)v;
                }
            }
        }
    } else {
        return FLACP_INVALID;                       // a reserved subframe type
    }
    if (b.fail) return FLACP_INVALID;
    const int pad = (int)((8 - (b.bits_read() & 7)) & 7);
    if (b.take(pad) != 0 || b.fail) return FLACP_INVALID;
    const size_t body = b.bits_read() / 8;
    if (body + 2 > n) return FLACP_INVALID;
    *frame_bytes = body + 2;
    if (Sink::kStore && wasted)
        for (uint32_t i = 0; i < bs; i++) sink.put(i, sink.get(i) * (int32_t)(1u << wasted));
    return FLACP_OK;
}

// A recording's frame: one subframe per channel of the stream (s.channels, which the header test held the frame to), the side
// channel of a stereo assignment read at one bit more than s.bits.  The channels are left as coded; *assign (the header's channel
// code) says how flac_decorrelate takes them to left and right.
template <class Sink>
FLACP_HD int flac_parse_frame_wide(const uint8_t* p, size_t n, uint32_t head_bytes, uint32_t bs, const FlacStreamShape& s, Sink& sink,
                                   size_t* frame_bytes, uint32_t* assign) {
    if (n < 4) return FLACP_INVALID;
    const uint32_t code = p[3] >> 4;
    if (s.channels == 1 ? code != 0 : (code != 1 && code != 8 && code != 9 && code != 10)) return FLACP_INVALID;
    *assign = code;
    FlacBits b;
    b.init(p, n, head_bytes);
    for (uint32_t ch = 0; ch < s.channels; ch++) {
        const bool side = (ch == 1 && (code == 8 || code == 10)) || (ch == 0 && code == 9);
        sink.channel(ch);
        if (const int rc = flac_parse_subframe(b, bs, (int)s.bits + (side ? 1 : 0), sink)) return rc;
    }
    return flac_frame_end(b, n, frame_bytes);
}

// One sample pair of a stereo frame as coded (a: the first subframe's, c: the second's) -> left and right, in exact integers;
// false when either falls outside the stream's depth.
FLACP_HD bool flac_decorrelate(uint32_t assign, int32_t a, int32_t c, uint32_t bits, int32_t* left, int32_t* right) {
    int64_t l = a, r = c;
    if (assign == 8) {
        r = (int64_t)a - c;                                            // left, side
    } else if (assign == 9) {
        l = (int64_t)a + c;                                            // side, right
    } else if (assign == 10) {
        const int64_t m = (int64_t)a * 2 + (c & 1);                    // mid, side: (M << 1) | (S & 1)
        l = (m + c) >> 1;
        r = (m - c) >> 1;
    }
    const int64_t lim = (int64_t)1 << (bits - 1);
    *left = (int32_t)l;
    *right = (int32_t)r;
    return l >= -lim && l < lim && r >= -lim && r < lim;
}

// The marker and the metadata blocks of stream[0 .. n_bytes), every read bounded by n_bytes: bnhip_flac_stream_info (bnhip.h) without
// its argument check, or with `recordings` bnhip_flac_recording_info, which accepts 1 or 2 channels at 16 or 24 bits (anything but
// mono 16-bit up to FLACDEC_MAX_BLOCK_WIDE).  Host only.
inline void flac_stream_info(const uint8_t* stream, size_t n_bytes, bnhip_flac_info* out, bool recordings = false) {
    *out = bnhip_flac_info{};
    out->status = BNHIP_FLAC_BAD_METADATA;
    if (n_bytes < 4 || stream[0] != 'f' || stream[1] != 'L' || stream[2] != 'a' || stream[3] != 'C') return;
    size_t pos = 4;
    bool last = false, have_info = false;
    for (size_t blocks = 0; !last; blocks++) {
        if (n_bytes - pos < 4) return;                                  // (pos <= n_bytes throughout)
        last = (stream[pos] & 0x80u) != 0;
        const uint32_t kind = stream[pos] & 0x7Fu;
        const size_t size = ((size_t)stream[pos + 1] << 16) | ((size_t)stream[pos + 2] << 8) | stream[pos + 3];
        pos += 4;
        if (n_bytes - pos < size) return;
        if ((blocks == 0) != (kind == 0) || kind == 127) return;
        const uint8_t* b = stream + pos;
        if (kind == 0) {
            if (size != 34) return;
            uint64_t v = 0;
            for (int i = 10; i < 18; i++) v = (v << 8) | b[i];
            out->min_block = ((uint32_t)b[0] << 8) | b[1];
            out->max_block = ((uint32_t)b[2] << 8) | b[3];
            out->min_frame = ((uint32_t)b[4] << 16) | ((uint32_t)b[5] << 8) | b[6];
            out->max_frame = ((uint32_t)b[7] << 16) | ((uint32_t)b[8] << 8) | b[9];
            out->rate = (uint32_t)(v >> 44);
            out->channels = (uint32_t)((v >> 41) & 7u) + 1u;
            out->bits = (uint32_t)((v >> 36) & 31u) + 1u;
            out->total_samples = v & (((uint64_t)1 << 36) - 1u);
            if (out->min_block < 16 || out->min_block > out->max_block) return;
            have_info = true;
        } else if (kind == 3) {
            out->seek_points = (uint32_t)(size / 18);
        }
        pos += size;
    }
    if (!have_info) return;
    out->audio_offset = pos;
    out->status = BNHIP_FLAC_UNSUPPORTED;
    const bool clip = out->channels == 1 && out->bits == 16;
    if (out->rate == 0 || !(clip || (recordings && out->channels <= 2 && (out->bits == 16 || out->bits == 24)))) return;
    if (out->total_samples == 0 || out->total_samples > 0x7FFFFFFFull) return;
    if (out->max_block > (clip ? FLACDEC_MAX_BLOCK : FLACDEC_MAX_BLOCK_WIDE)) return;
    if (out->min_block != out->max_block && out->total_samples > out->max_block) return;       // more than one frame
    if (n_bytes - pos >= 2 && stream[pos] == 0xFFu && stream[pos + 1] == 0xF9u) return;         // the first frame says variable block size
    out->status = BNHIP_FLAC_OK;
}

}  // namespace bnhip
