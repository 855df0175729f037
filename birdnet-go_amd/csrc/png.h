// PNG encoding of a batch of equally sized 8-bit index images on the device (png.hip, api_png.cpp bnhip_png_*): the project's own
// deterministic encoder of DESIGN.md §9 "PNG" - a valid PNG (ISO/IEC 15948) per image whose IDAT chunks hold one zlib (RFC 1950)
// DEFLATE (RFC 1951) stream cut into bands.  All arithmetic is integer, so every byte is pinned; an image's stream depends on its own
// pixels, its size and the palette alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/bnhip.h"

namespace bnhip {

constexpr int PNG_MAX_DIM = 4096;                        // width and height 1..4096
constexpr int PNG_BAND_TARGET = 16384;                   // a band is ceil(16384 / (W + 1)) rows
constexpr int PNG_BAND_MAX = 20481;                      // and less than 16384 + W + 1 bytes: at most this many
constexpr int PNG_LIT_SYMS = 257;                        // literals 0..255 and end-of-block
constexpr int PNG_CL_SYMS = 19;                          // the code-length alphabet
constexpr int PNG_LIT_LIMIT = 15, PNG_CL_LIMIT = 7;
constexpr int PNG_HEAD = 8 + 25 + 780;                   // signature, IHDR, PLTE: what precedes an image's first IDAT
constexpr int PNG_IEND = 12;

enum { PNG_ZERO = 0, PNG_HUFFMAN = 1, PNG_STORED = 2 };  // a band's form

// One band's analysis.  bits: the form's DEFLATE block (ZERO, HUFFMAN); bytes: the IDAT chunk's data - the band's piece of the
// DEFLATE stream, with the zlib header in front of the first band and the Adler-32 behind the last.
struct PngRecord {
    uint32_t form, bits, bytes;
    uint32_t s1, s2;                                     // sum of the bytes, sum of (n - i) * byte[i], both mod 65521
    uint8_t len[PNG_LIT_SYMS];                           // HUFFMAN: the literal/length code lengths
    uint8_t cl[PNG_CL_SYMS];                             // and the code-length code's
};
static_assert(sizeof(PngRecord) == 296, "PngRecord layout");

// What a call's streams open with, built on the host: signature, IHDR and PLTE with their CRCs.
struct PngHead { uint8_t b[PNG_HEAD + 3]; };

// The geometry of one call and its scratch; every array lives in one caller-supplied device block.
struct PngWork {
    int n_images = 0, width = 0, height = 0;
    int rows = 0, bands = 0;                             // rows per band, bands per image
    PngHead head;
    PngRecord* rec = nullptr;                            // [n_images * bands]
    unsigned long long* rel = nullptr;                   // [n_images * bands] byte offset of the band's chunk in its image's stream
    unsigned long long* image_bytes = nullptr;           // [n_images]
    uint32_t* adler = nullptr;                           // [n_images]
};
int png_band_rows(int width, int height);
int png_bands(int width, int height);
// the STORED bound: no stream of a width x height image is longer (per image: png_max_bytes(1, ...))
size_t png_max_bytes(int n_images, int width, int height);
size_t png_workspace_bytes(int n_images, int width, int height);
PngWork png_work(int n_images, int width, int height, const uint8_t* palette, void* d_block);

// images uint8 [n_images][height][width] on the device; out: the streams back to back, offsets uint64 [n_images + 1].  Enqueues
// analyse, the two layout scans, the stream heads and emit.  Nothing is synchronised; no kernel writes at or past out + out_cap.
void launch_png(const uint8_t* images, const PngWork& w, uint8_t* out, size_t out_cap, unsigned long long* offsets, hipStream_t s);


// api_png.cpp, for the entries that put another stage in front of the encoder: what every entry checks before any device is touched
// (-> 0 or a negative BNHIP_E_*).
int png_args_check(int n_images, int width, int height);
int png_cap_check(int n_images, int width, int height, size_t out_cap);

}  // namespace bnhip
