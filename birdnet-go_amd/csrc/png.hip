// PNG encoding of a batch of 8-bit index images (DESIGN.md §9 "PNG"): integer arithmetic, every band of every image independent.
//
//   analyse   one block per (image, band): the band's filtered bytes (filter 0: a zero, then the row) in LDS, their histogram by LDS
//             atomics, the all-zero test, the Adler-32 partials; then the literal code's lengths (15-bit limit) and the code-length
//             code's (7-bit limit) - the sort is a rank per thread, the tree one thread's two-queue merge, the depths a walk per
//             leaf - the block's bit count, the form (ZERO / HUFFMAN / STORED) and one record per band.
//   layout    a scan of chunk bytes per image, which also folds the bands' Adler partials in order (the last band's chunk holds the
//             Adler-32 under its CRC, so emit needs it), then of image bytes across the batch -> offsets[n_images + 1]
//   heads     signature, IHDR, PLTE (built once on the host, CRCs included) and IEND of every image
//   emit      one block per (image, band): the canonical codes from the record's lengths, a block scan of the bytes' code lengths,
//             the reversed codes ORed LSB-first into a zeroed LDS buffer that holds the whole chunk, CRC-32 folded over 256 partials
//             by crc(A || B) = crc(A) x^(8 |B|) ^ crc(B), then the chunk copied to its byte offset.
// A chunk's absolute offset is offsets[image] + rel[band].  Vector stores only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "block_scan.h"
#include "png.h"

namespace bnhip {

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr uint32_t ADLER = 65521u;
constexpr uint32_t CRC_POLY = 0xedb88320u;
// the longest chunk: length and type, the zlib header, a STORED block's five bytes, the band, the Adler-32, the CRC; in words, two spare
// (put_bits' second word and the copy's)
constexpr int CHUNK_MAX = 8 + 2 + 5 + PNG_BAND_MAX + 4 + 4;
constexpr int W_WORDS = (CHUNK_MAX + 3) / 4 + 2;

struct PngGeom { int n_images, W, H, R, bands; };
// a band's first row and its bytes
__device__ __forceinline__ int band_row0(const PngGeom& g, int band) { return band * g.R; }
__host__ __device__ inline int band_bytes(int W, int H, int R, int band) {
    const int left = H - band * R;
    return (left < R ? left : R) * (W + 1);
}

__host__ __device__ inline uint32_t crc32_byte(uint32_t c, uint32_t b) {
    c ^= b;
    for (int i = 0; i < 8; i++) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
    return c;
}

__device__ __forceinline__ void stage_band(const uint8_t* __restrict__ images, const PngGeom& g, int image, int band, int n, uint8_t* __restrict__ xs,
                                           int tid) {
    const uint8_t* img = images + ((size_t)image * (size_t)g.H + (size_t)band_row0(g, band)) * (size_t)g.W;
    const int stride = g.W + 1;
    for (int i = tid; i < n; i += THREADS) {
        const int row = i / stride, col = i - row * stride;
        xs[i] = col ? img[(size_t)row * (size_t)g.W + (size_t)(col - 1)] : (uint8_t)0;
    }
}

// What the code construction keeps in LDS.
struct HuffShared {
    uint32_t weight[2 * PNG_LIT_SYMS];
    uint16_t parent[2 * PNG_LIT_SYMS];
    uint16_t order[PNG_LIT_SYMS + 1];
    uint32_t blc[16];
    int m;
};
// Code lengths of an alphabet of nsym <= 257 symbols with at least two non-zero counts, at most `limit` bits (DESIGN.md §9 "PNG", code
// construction): cnt and len in LDS.  Called by the whole block; it ends synchronised.
__device__ __forceinline__ void huff_lengths(const uint32_t* __restrict__ cnt, int nsym, int limit, uint8_t* __restrict__ len, HuffShared& S, int tid) {
    if (tid < 16) S.blc[tid] = 0u;
    if (tid == 0) S.m = 0;
    __syncthreads();
    // the leaves in ascending (count, symbol) order: a symbol's place is the number of present symbols before it
    for (int s = tid; s < nsym; s += THREADS) {
        const uint32_t c = cnt[s];
        len[s] = 0;
        if (c) {
            int p = 0;
            for (int t = 0; t < nsym; t++) {
                const uint32_t d = cnt[t];
                p += (d != 0u && (d < c || (d == c && t < s))) ? 1 : 0;
            }
            S.order[p] = (uint16_t)s; S.weight[p] = c;
            atomicAdd(&S.m, 1);
        }
    }
    __syncthreads();
    const int m = S.m;
    if (m < 2) return;                                               // (never: end-of-block and a literal, or two lengths, are present)
    if (tid == 0) {
        // two queues: the leaves, and the internal nodes in the order they were made; a leaf before an internal node of equal weight
        int li = 0, ii = m, next = m;
        for (int k = 0; k < m - 1; k++) {
            int a, b;
            if (li < m && (ii >= next || S.weight[li] <= S.weight[ii])) a = li++; else a = ii++;
            if (li < m && (ii >= next || S.weight[li] <= S.weight[ii])) b = li++; else b = ii++;
            S.weight[next] = S.weight[a] + S.weight[b];
            S.parent[a] = S.parent[b] = (uint16_t)next;
            next++;
        }
    }
    __syncthreads();
    for (int p = tid; p < m; p += THREADS) {
        int d = 0;
        for (int node = p; node != 2 * m - 2 && d < 2 * PNG_LIT_SYMS; node = S.parent[node]) d++;     // (a depth is below m)
        atomicAdd(&S.blc[d < limit ? d : limit], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        // the depths above the limit were folded onto it; each step takes one unit 2^-limit off the Kraft sum, down to exactly 1
        uint32_t total = 0;
        for (int i = 1; i <= limit; i++) total += S.blc[i] << (limit - i);
        while (total > (1u << limit) && S.blc[limit] > 0u) {             // (a fold leaves at least two codes at the limit)
            S.blc[limit]--;
            for (int i = limit - 1; i >= 1; i--)
                if (S.blc[i]) { S.blc[i]--; S.blc[i + 1] += 2u; break; }
            total--;
        }
    }
    __syncthreads();
    // the lengths handed out again by rank: the most frequent symbol takes the shortest
    for (int p = tid; p < m; p += THREADS) {
        const uint32_t q = (uint32_t)(m - 1 - p);
        int l = 1;
        uint32_t acc = S.blc[1];
        while (acc <= q && l < limit) { l++; acc += S.blc[l]; }
        len[S.order[p]] = (uint8_t)l;
    }
    __syncthreads();
}

// the code-length code's lengths are sent in this order (RFC 1951 §3.2.7)
__device__ __forceinline__ int cl_order(int i) {
    constexpr uint8_t o[PNG_CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}
__device__ __forceinline__ int cl_sent(const uint8_t* __restrict__ cl) {
    int ncl = PNG_CL_SYMS;
    while (ncl > 4 && cl[cl_order(ncl - 1)] == 0) ncl--;
    return ncl;
}

// A match length 3..258 in the fixed code: the length symbol's index 0..28 (symbol 257 + k), its extra bits and their value.
__device__ __forceinline__ void length_symbol(int L, int* k, int* extra, int* value) {
    if (L == 258) { *k = 28; *extra = 0; *value = 0; return; }
    const int x = L - 3;
    if (x < 8) { *k = x; *extra = 0; *value = 0; return; }
    const int e = (31 - __clz(x)) - 2;
    *k = 4 + 4 * e + ((x >> e) - 4); *extra = e; *value = x & ((1 << e) - 1);
}
__device__ __forceinline__ int fixed_bits(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
// the bits of a ZERO block of n bytes: the block header, literal 0, (n - 1) / 258 matches of 258, the remainder, end-of-block
__device__ __forceinline__ uint32_t zero_bits(int n) {
    const int q = (n - 1) / 258, r = (n - 1) % 258;
    uint32_t bits = 3u + 8u + 13u * (uint32_t)q + 7u;
    if (r >= 3) {
        int k, e, v;
        length_symbol(r, &k, &e, &v);
        bits += (uint32_t)(fixed_bits(257 + k) + e + 5);
    } else bits += 8u * (uint32_t)r;
    return bits;
}
// a block's bytes in its band: the last band's block ends the stream; any other is followed by an empty stored block
__device__ __forceinline__ uint32_t closed_bytes(uint32_t bits, bool final) { return final ? (bits + 7u) / 8u : (bits + 3u + 7u) / 8u + 4u; }

// Grid: (bands, n_images).
__global__ __launch_bounds__(THREADS) void k_png_analyse(const uint8_t* __restrict__ images, PngGeom g, PngRecord* __restrict__ rec) {
    __shared__ uint8_t xs[PNG_BAND_MAX + 3];
    __shared__ uint32_t cnt[PNG_LIT_SYMS];
    __shared__ uint32_t clcnt[PNG_CL_SYMS];
    __shared__ uint8_t len[PNG_LIT_SYMS + 3], cl[PNG_CL_SYMS + 1];
    __shared__ HuffShared S;
    __shared__ u64 ad[2];
    __shared__ uint32_t bitsum;
    const int tid = threadIdx.x, band = blockIdx.x, image = blockIdx.y;
    const int n = band_bytes(g.W, g.H, g.R, band);
    const bool final = band == g.bands - 1;
    stage_band(images, g, image, band, n, xs, tid);
    cnt[tid] = 0u;
    if (tid == 0) { cnt[256] = 1u; ad[0] = ad[1] = 0ull; bitsum = 0u; }          // end-of-block occurs once
    if (tid < PNG_CL_SYMS) clcnt[tid] = 0u;
    __syncthreads();
    u64 a = 0, b = 0;
    int nz = 0;
    for (int i = tid; i < n; i += THREADS) {
        const uint32_t v = xs[i];
        atomicAdd(&cnt[v], 1u);
        a += v; b += (u64)(n - i) * v;                                             // b <= 20481^2 * 255 / 2 < 2^36
        nz |= (int)v;
    }
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
    if ((tid & 63) == 0) { atomicAdd(&ad[0], a); atomicAdd(&ad[1], b); }
    const int any = __syncthreads_or(nz);

    uint32_t form = PNG_STORED, bits = 0u, deflate = 5u + (uint32_t)n;
    if (!any) {
        form = PNG_ZERO; bits = zero_bits(n); deflate = closed_bytes(bits, final);
    } else {
        huff_lengths(cnt, PNG_LIT_SYMS, PNG_LIT_LIMIT, len, S, tid);
        // the header's 258 lengths: HLIT 0 (257 literal/length codes), HDIST 0 (one distance code, of one bit, never used)
        for (int s = tid; s < PNG_LIT_SYMS + 1; s += THREADS) atomicAdd(&clcnt[s < PNG_LIT_SYMS ? len[s] : 1], 1u);
        __syncthreads();
        huff_lengths(clcnt, PNG_CL_SYMS, PNG_CL_LIMIT, cl, S, tid);
        uint32_t part = 0;
        for (int s = tid; s < PNG_LIT_SYMS + 1; s += THREADS)
            part += s < PNG_LIT_SYMS ? (uint32_t)cl[len[s]] + cnt[s] * (uint32_t)len[s] : (uint32_t)cl[1];
        atomicAdd(&bitsum, part);
        __syncthreads();
        const uint32_t hb = 3u + 5u + 5u + 4u + 3u * (uint32_t)cl_sent(cl) + bitsum;
        const uint32_t hbytes = closed_bytes(hb, final);
        if (hbytes < deflate) { form = PNG_HUFFMAN; bits = hb; deflate = hbytes; }
    }
    PngRecord* r = rec + (size_t)image * (size_t)g.bands + (size_t)band;
    const bool coded = form == PNG_HUFFMAN;
    for (int s = tid; s < PNG_LIT_SYMS; s += THREADS) r->len[s] = coded ? len[s] : (uint8_t)0;
    if (tid < PNG_CL_SYMS) r->cl[tid] = coded ? cl[tid] : (uint8_t)0;
    if (tid == 0) {
        r->form = form; r->bits = bits;
        r->bytes = deflate + (band == 0 ? 2u : 0u) + (final ? 4u : 0u);
        r->s1 = (uint32_t)(ad[0] % ADLER); r->s2 = (uint32_t)(ad[1] % ADLER);
    }
}

// One block per image: rel[band], the image's bytes, its Adler-32.
__global__ __launch_bounds__(THREADS) void k_png_layout_image(PngGeom g, const PngRecord* __restrict__ rec, u64* __restrict__ rel,
                                                              u64* __restrict__ image_bytes, uint32_t* __restrict__ adler) {
    __shared__ u64 sh[THREADS];
    const int image = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)image * (size_t)g.bands;
    u64 carry = PNG_HEAD;
    for (int b0 = 0; b0 < g.bands; b0 += THREADS) {
        const int b = b0 + tid;
        const u64 c = b < g.bands ? 12ull + rec[base + b].bytes : 0ull;
        const u64 incl = block_scan<u64>(c, sh, tid);
        if (b < g.bands) rel[base + b] = carry + incl - c;
        carry += sh[THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) {
        image_bytes[image] = carry + PNG_IEND;
        // Adler-32 of the bands in order: s1 = 1 + all bytes; a band of n bytes adds n s1 + its own weighted sum to s2
        u64 s1 = 1, s2 = 0;
        for (int b = 0; b < g.bands; b++) {
            const u64 n = (u64)band_bytes(g.W, g.H, g.R, b);
            s2 = (s2 + n * s1 + rec[base + b].s2) % ADLER;
            s1 = (s1 + rec[base + b].s1) % ADLER;
        }
        adler[image] = (uint32_t)((s2 << 16) | s1);
    }
}

// One block: offsets[i] = the bytes of the images before i, offsets[n_images] = all of them.
__global__ __launch_bounds__(THREADS) void k_png_layout_batch(int n_images, const u64* __restrict__ image_bytes, u64* __restrict__ offsets) {
    __shared__ u64 sh[THREADS];
    const int tid = threadIdx.x;
    u64 carry = 0;
    for (int c0 = 0; c0 < n_images; c0 += THREADS) {
        const int c = c0 + tid;
        const u64 b = c < n_images ? image_bytes[c] : 0ull;
        const u64 incl = block_scan<u64>(b, sh, tid);
        if (c < n_images) offsets[c] = carry + incl - b;
        carry += sh[THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) offsets[n_images] = carry;
}

// One block per image: signature, IHDR and PLTE in front, IEND behind.
__global__ __launch_bounds__(THREADS) void k_png_heads(PngHead head, const u64* __restrict__ offsets, uint8_t* __restrict__ out, u64 out_cap) {
    const int image = blockIdx.x, tid = threadIdx.x;
    const u64 base = offsets[image], end = offsets[image + 1];
    if (end > out_cap || end < base + PNG_HEAD + PNG_IEND) return;
    for (int i = tid; i < PNG_HEAD; i += THREADS) out[base + i] = head.b[i];
    if (tid < PNG_IEND) {
        constexpr uint8_t iend[PNG_IEND] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
        out[end - PNG_IEND + tid] = iend[tid];
    }
}

// ORs the low `len` (1..32) bits of v (v < 2^len) into the LSB-first bit buffer at bit `pos`
__device__ __forceinline__ void put_bits(uint32_t* __restrict__ W, uint32_t pos, int len, uint32_t v) {
    const uint32_t w = pos >> 5;
    const int sh = (int)(pos & 31);
    if (w + 1 >= (uint32_t)W_WORDS) return;
    atomicOr(&W[w], v << sh);
    if (sh + len > 32) atomicOr(&W[w + 1], v >> (32 - sh));
}
__device__ __forceinline__ void put_byte(uint32_t* __restrict__ W, int j, uint32_t v) { put_bits(W, 8u * (uint32_t)j, 8, v & 0xffu); }
__device__ __forceinline__ uint32_t chunk_byte(const uint32_t* __restrict__ W, int j) { return (W[j >> 2] >> (8 * (j & 3))) & 0xffu; }
// a Huffman code of l bits, most significant bit first
__device__ __forceinline__ uint32_t reversed(uint32_t code, int l) { return __brev(code) >> (32 - l); }
// a symbol of the fixed literal/length code at `pos`; -> its bits
__device__ __forceinline__ int put_fixed(uint32_t* __restrict__ W, uint32_t pos, int sym) {
    const int l = fixed_bits(sym);
    const uint32_t code = sym < 144 ? 0x30u + sym : sym < 256 ? 0x190u + (sym - 144) : sym < 280 ? (uint32_t)(sym - 256) : 0xc0u + (sym - 280);
    put_bits(W, pos, l, reversed(code, l));
    return l;
}

// a * b mod the CRC-32 polynomial, bit-reflected: 0x80000000 is 1
__device__ __forceinline__ uint32_t crc32_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) r ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return r;
}

// Canonical codes (RFC 1951 §3.2.2) of the lengths in LDS, bit-reversed for the LSB-first buffer.  Called by the whole block; ends synchronised.
__device__ __forceinline__ void canonical(const uint8_t* __restrict__ len, int nsym, uint16_t* __restrict__ rc, uint32_t* __restrict__ blc,
                                          uint32_t* __restrict__ nxt, int tid) {
    if (tid < 16) blc[tid] = 0u;
    __syncthreads();
    for (int s = tid; s < nsym; s += THREADS)
        if (len[s]) atomicAdd(&blc[len[s] & 15], 1u);
    __syncthreads();
    if (tid == 0) {
        uint32_t code = 0;
        nxt[0] = 0u;
        for (int b = 1; b < 16; b++) { code = (code + blc[b - 1]) << 1; nxt[b] = code; }
    }
    __syncthreads();
    for (int s = tid; s < nsym; s += THREADS) {
        const int l = len[s] & 15;
        uint32_t k = 0;
        for (int t = 0; t < s; t++) k += len[t] == l ? 1u : 0u;
        rc[s] = l ? (uint16_t)reversed(nxt[l] + k, l) : (uint16_t)0;
    }
    __syncthreads();
}

// Grid: (bands, n_images).
__global__ __launch_bounds__(THREADS) void k_png_emit(const uint8_t* __restrict__ images, PngGeom g, const PngRecord* __restrict__ rec,
                                                      const u64* __restrict__ rel, const u64* __restrict__ offsets,
                                                      const uint32_t* __restrict__ adler, uint8_t* __restrict__ out, u64 out_cap) {
    __shared__ uint8_t xs[PNG_BAND_MAX + 3];
    __shared__ uint32_t W[W_WORDS];
    __shared__ uint32_t sc[THREADS];
    __shared__ uint32_t T[256];                                  // CRC-32 of one byte
    __shared__ uint32_t cv[THREADS];
    __shared__ uint8_t len[PNG_LIT_SYMS + 3], cl[PNG_CL_SYMS + 1];
    __shared__ uint16_t rc[PNG_LIT_SYMS + 1], rcl[PNG_CL_SYMS + 1];
    __shared__ uint32_t blc[16], nxt[16];
    __shared__ uint32_t lit0;
    const int tid = threadIdx.x, band = blockIdx.x, image = blockIdx.y;
    const int n = band_bytes(g.W, g.H, g.R, band);
    const bool first = band == 0, final = band == g.bands - 1;
    const PngRecord* r = rec + (size_t)image * (size_t)g.bands + (size_t)band;
    const uint32_t form = r->form;
    const int bytes = (int)r->bytes, chunk = 12 + bytes;
    const int data0 = 8 + (first ? 2 : 0);                       // the band's first byte of the DEFLATE stream
    const u64 off = offsets[image] + rel[(size_t)image * (size_t)g.bands + (size_t)band];
    if (form > PNG_STORED || bytes < 1 || chunk > CHUNK_MAX || bytes > (first ? 2 : 0) + 5 + n + (final ? 4 : 0) || off + (u64)chunk > out_cap)
        return;                                                  // (block-uniform)
    stage_band(images, g, image, band, n, xs, tid);
    for (int i = tid; i < W_WORDS; i += THREADS) W[i] = 0u;
    T[tid] = crc32_byte(0u, (uint32_t)tid);
    for (int s = tid; s < PNG_LIT_SYMS; s += THREADS) len[s] = r->len[s] & 15;
    if (tid < PNG_CL_SYMS) cl[tid] = r->cl[tid] & 7;
    __syncthreads();
    if (tid == 0) {
        for (int j = 0; j < 4; j++) put_byte(W, j, (uint32_t)bytes >> (8 * (3 - j)));
        put_byte(W, 4, 'I'); put_byte(W, 5, 'D'); put_byte(W, 6, 'A'); put_byte(W, 7, 'T');
        if (first) { put_byte(W, 8, 0x78); put_byte(W, 9, 0x01); }
        if (final) {
            const uint32_t ad = adler[image];
            for (int j = 0; j < 4; j++) put_byte(W, 8 + bytes - 4 + j, ad >> (8 * (3 - j)));
        }
    }
    const uint32_t p0 = 8u * (uint32_t)data0;
    if (form == PNG_STORED) {
        if (tid == 0) {
            put_byte(W, data0, final ? 1u : 0u);
            put_byte(W, data0 + 1, (uint32_t)n); put_byte(W, data0 + 2, (uint32_t)n >> 8);
            put_byte(W, data0 + 3, ~(uint32_t)n); put_byte(W, data0 + 4, ~(uint32_t)n >> 8);
        }
        for (int i = tid; i < n; i += THREADS) put_byte(W, data0 + 5 + i, xs[i]);
    } else if (form == PNG_ZERO) {
        if (tid == 0) {
            uint32_t pos = p0;
            put_bits(W, pos, 3, (final ? 1u : 0u) | (1u << 1)); pos += 3;          // BFINAL, BTYPE 01
            pos += put_fixed(W, pos, 0);
            const int q = (n - 1) / 258, rem = (n - 1) % 258;
            for (int j = 0; j < q; j++) { pos += put_fixed(W, pos, 285); pos += 5; }   // distance code 0: five zero bits
            if (rem >= 3) {
                int k, e, v;
                length_symbol(rem, &k, &e, &v);
                pos += put_fixed(W, pos, 257 + k);
                if (e) put_bits(W, pos, e, (uint32_t)v);
                pos += e + 5;
            } else
                for (int j = 0; j < rem; j++) pos += put_fixed(W, pos, 0);
            pos += put_fixed(W, pos, 256);
            lit0 = pos;
        }
    } else {
        canonical(len, PNG_LIT_SYMS, rc, blc, nxt, tid);
        canonical(cl, PNG_CL_SYMS, rcl, blc, nxt, tid);
        if (tid == 0) {
            // BFINAL, BTYPE 10, HLIT 0, HDIST 0, HCLEN, the code-length code's lengths, then the 258 lengths in it
            const int ncl = cl_sent(cl);
            uint32_t pos = p0;
            put_bits(W, pos, 3, (final ? 1u : 0u) | (2u << 1)); pos += 3 + 5 + 5;
            put_bits(W, pos, 4, (uint32_t)(ncl - 4)); pos += 4;
            for (int j = 0; j < ncl; j++) { put_bits(W, pos, 3, cl[cl_order(j)]); pos += 3; }
            for (int s = 0; s < PNG_LIT_SYMS + 1; s++) {
                const int l = s < PNG_LIT_SYMS ? len[s] : 1;
                if (cl[l]) put_bits(W, pos, cl[l], rcl[l]);
                pos += cl[l];
            }
            lit0 = pos;
        }
        // a thread's bytes are contiguous
        const int ch = (n + THREADS - 1) / THREADS;
        const int i0 = min(tid * ch, n), i1 = min(tid * ch + ch, n);
        uint32_t total = 0;
        for (int i = i0; i < i1; i++) total += len[xs[i]];
        const uint32_t incl = block_scan<uint32_t>(total, sc, tid);
        const uint32_t all = sc[THREADS - 1];
        uint32_t pos = lit0 + (incl - total);
        for (int i = i0; i < i1; i++) {
            const int v = xs[i], l = len[v];
            if (l) put_bits(W, pos, l, rc[v]);
            pos += l;
        }
        if (tid == THREADS - 1 && len[256]) put_bits(W, lit0 + all, len[256], rc[256]);
        __syncthreads();
        if (tid == 0) lit0 = lit0 + all + len[256];
    }
    __syncthreads();
    if (tid == 0 && form != PNG_STORED && !final) {
        // the empty stored block: three zero bits, the padding, 00 00 FF FF
        const int e = (int)((lit0 + 3u + 7u) / 8u);
        put_byte(W, e + 2, 0xff); put_byte(W, e + 3, 0xff);
    }
    __syncthreads();

    // CRC-32 of type and data, D bytes from byte 4.  The CRC of nothing is 0 and crc(A || B) = crc(A) x^(8 |B|) ^ crc(B): the bytes
    // are taken as 256 pieces of C bytes with the padding in front, so that every right-hand operand of the tree is whole.
    const int D = 4 + bytes;
    const int C = (D + THREADS - 1) / THREADS, padding = THREADS * C - D;
    uint32_t crc = 0xffffffffu, mul = 0x80000000u;
    for (int j = 0; j < C; j++) {
        const int b = tid * C + j - padding;
        if (b >= 0) crc = T[(crc ^ chunk_byte(W, 4 + b)) & 0xffu] ^ (crc >> 8);
        mul = T[mul & 0xffu] ^ (mul >> 8);                                            // x^(8 C)
    }
    cv[tid] = crc ^ 0xffffffffu;
    for (int s = 1; s < THREADS; s <<= 1) {
        __syncthreads();
        if ((tid & (2 * s - 1)) == 0) cv[tid] = crc32_mul(cv[tid], mul) ^ cv[tid + s];
        mul = crc32_mul(mul, mul);
    }
    if (tid == 0)
        for (int j = 0; j < 4; j++) put_byte(W, 8 + bytes + j, cv[0] >> (8 * (3 - j)));
    __syncthreads();

    // the copy: bytes up to the first 4-byte boundary of the destination, whole words, the bytes left over
    uint8_t* dst = out + off;
    int head = (int)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    head = head < chunk ? head : chunk;
    const int nw = (chunk - head) / 4, tail = chunk - head - 4 * nw;
    if (tid < head) dst[tid] = (uint8_t)chunk_byte(W, tid);
    for (int w = tid; w < nw; w += THREADS) {
        const int i = head + 4 * w, sh = 8 * (i & 3);
        const uint32_t lo = W[i >> 2], hi = W[(i >> 2) + 1];                         // (the spare word)
        *reinterpret_cast<uint32_t*>(dst + i) = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    if (tid < tail) dst[head + 4 * nw + tid] = (uint8_t)chunk_byte(W, head + 4 * nw + tid);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

uint32_t crc32_host(const uint8_t* p, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = crc32_byte(c, p[i]);
    return c ^ 0xffffffffu;
}
void store_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

}  // namespace

int png_band_rows(int width, int height) {
    const int r = (PNG_BAND_TARGET + width) / (width + 1);
    return r < 1 ? 1 : r > height ? height : r;
}

int png_bands(int width, int height) {
    const int r = png_band_rows(width, height);
    return (height + r - 1) / r;
}

size_t png_max_bytes(int n_images, int width, int height) {
    // every band STORED: the chunk's 12 bytes and the block's 5 around the band's rows; the zlib header and the Adler-32 once
    const size_t per = (size_t)PNG_HEAD + PNG_IEND + 2 + 4 + (size_t)png_bands(width, height) * (12 + 5) + (size_t)height * ((size_t)width + 1);
    return per * (size_t)n_images;
}

size_t png_workspace_bytes(int n_images, int width, int height) {
    const size_t B = (size_t)n_images * (size_t)png_bands(width, height);
    return align256(B * sizeof(PngRecord)) + align256(B * 8) + align256((size_t)n_images * 8) + align256((size_t)n_images * 4);
}

PngWork png_work(int n_images, int width, int height, const uint8_t* palette, void* d_block) {
    PngWork w;
    w.n_images = n_images; w.width = width; w.height = height;
    w.rows = png_band_rows(width, height); w.bands = png_bands(width, height);
    const size_t B = (size_t)n_images * (size_t)w.bands;
    char* p = (char*)d_block;
    w.rec = (PngRecord*)p; p += align256(B * sizeof(PngRecord));
    w.rel = (u64*)p; p += align256(B * 8);
    w.image_bytes = (u64*)p; p += align256((size_t)n_images * 8);
    w.adler = (uint32_t*)p;
    uint8_t* h = w.head.b;
    std::memset(h, 0, sizeof(w.head.b));
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::memcpy(h, sig, 8);
    // IHDR: width, height, bit depth 8, colour type 3, compression 0, filter method 0, no interlace
    store_be32(h + 8, 13); std::memcpy(h + 12, "IHDR", 4);
    store_be32(h + 16, (uint32_t)width); store_be32(h + 20, (uint32_t)height);
    h[24] = 8; h[25] = 3;
    store_be32(h + 29, crc32_host(h + 12, 17));
    store_be32(h + 33, 768); std::memcpy(h + 37, "PLTE", 4);
    std::memcpy(h + 41, palette, 768);
    store_be32(h + 809, crc32_host(h + 37, 772));
    return w;
}

void launch_png(const uint8_t* images, const PngWork& w, uint8_t* out, size_t out_cap, unsigned long long* offsets, hipStream_t s) {
    const PngGeom g{w.n_images, w.width, w.height, w.rows, w.bands};
    const dim3 grid((unsigned)w.bands, (unsigned)w.n_images);
    hipLaunchKernelGGL(k_png_analyse, grid, dim3(THREADS), 0, s, images, g, w.rec);
    hipLaunchKernelGGL(k_png_layout_image, dim3(w.n_images), dim3(THREADS), 0, s, g, (const PngRecord*)w.rec, w.rel, w.image_bytes, w.adler);
    hipLaunchKernelGGL(k_png_layout_batch, dim3(1), dim3(THREADS), 0, s, w.n_images, (const u64*)w.image_bytes, offsets);
    hipLaunchKernelGGL(k_png_heads, dim3(w.n_images), dim3(THREADS), 0, s, w.head, (const u64*)offsets, out, (u64)out_cap);
    hipLaunchKernelGGL(k_png_emit, grid, dim3(THREADS), 0, s, images, g, (const PngRecord*)w.rec, (const u64*)w.rel, (const u64*)offsets,
                       (const uint32_t*)w.adler, out, (u64)out_cap);
}

}  // namespace bnhip
