// The device FLAC decoder's frame reader (birdnet-go_amd/csrc/flac_parse.h) run on the host, serially, in the order of the kernels of
// flac_decode.hip: scan every byte of the audio region for frame headers, parse every candidate to its end and check CRC-16, link
// the chain from the audio offset, restore the chain's frames.  Built with plain g++ under ASan + UBSan by
// tests/test_flac_decode_asan.py; every stream is copied to a heap block of its exact size first, so a read past it is caught.
//
//   flac_parse_main corpus.bin out.bin
// corpus.bin: records of u32 length + bytes.  out.bin: per record i32 status, i32 frames, u64 fail_offset, u32 n_samples, then
// n_samples int16 (n_samples is 0 unless the status is BNHIP_FLAC_OK).  stdout: "streams N ok M".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../birdnet-go_amd/csrc/flac_parse.h"

using namespace bnhip;

namespace {

struct Cand {
    uint64_t start, end;
    FlacFrameHead head;
};

struct Result {
    int32_t status = 0, frames = 0;
    uint64_t fail_offset = 0;
    std::vector<int16_t> samples;
};

Result decode(const uint8_t* stream, size_t n_bytes) {
    Result res;
    bnhip_flac_info info;
    flac_stream_info(stream, n_bytes, &info);
    res.status = info.status;
    if (info.status != BNHIP_FLAC_OK) return res;
    FlacStreamShape shape;
    shape.rate = info.rate;
    shape.bs = info.max_block;
    shape.total = (uint32_t)info.total_samples;
    shape.frames = (uint32_t)((info.total_samples + shape.bs - 1) / shape.bs);
    if (flacdec_too_short(shape.frames, n_bytes - info.audio_offset)) {
        res.status = BNHIP_FLAC_CORRUPT;
        res.fail_offset = info.audio_offset;
        return res;
    }
    const size_t cap = 2 * (size_t)shape.frames + 64;
    // scan
    std::vector<Cand> cands;
    bool overflow = false;
    for (uint64_t pos = info.audio_offset; pos < n_bytes; pos++) {
        FlacFrameHead h;
        if (!flac_frame_head(stream + pos, n_bytes - pos, shape, &h)) continue;
        if (cands.size() >= cap) { overflow = true; break; }
        cands.push_back(Cand{pos, 0, h});
    }
    if (overflow) { res.status = BNHIP_FLAC_UNSUPPORTED; return res; }
    // parse
    for (Cand& c : cands) {
        size_t avail = n_bytes - c.start;
        if (avail > flacdec_frame_cap(shape.bs)) avail = flacdec_frame_cap(shape.bs);
        FlacCountSink sink;
        size_t bytes = 0;
        if (c.head.bs > shape.bs || c.head.bytes > avail) continue;
        if (flac_parse_frame(stream + c.start, avail, c.head.bytes, c.head.bs, sink, &bytes) != FLACP_OK) continue;
        if (flac_crc16(stream + c.start, bytes) != 0) continue;
        c.end = c.start + bytes;
    }
    // link
    uint64_t pos = info.audio_offset;
    std::vector<const Cand*> chain;
    for (uint32_t j = 0; j < shape.frames; j++) {
        const Cand* found = nullptr;
        for (const Cand& c : cands)
            if (c.end && c.start == pos && c.head.number == j) found = &c;
        if (!found) break;
        chain.push_back(found);
        pos = found->end;
    }
    res.frames = (int32_t)chain.size();
    if (chain.size() != shape.frames || pos != n_bytes) {
        res.status = BNHIP_FLAC_CORRUPT;
        res.fail_offset = pos;
        return res;
    }
    // restore
    res.samples.assign(shape.total, 0);
    std::vector<int16_t> xs(shape.bs);
    for (uint32_t j = 0; j < shape.frames; j++) {
        const Cand& c = *chain[j];
        int32_t coefs[FLACDEC_MAX_ORDER];
        FlacStoreSink sink{xs.data(), coefs};
        size_t bytes = 0;
        if (flac_parse_frame(stream + c.start, (size_t)(c.end - c.start), c.head.bytes, c.head.bs, sink, &bytes) != FLACP_OK) {
            res.status = BNHIP_FLAC_CORRUPT;
            res.frames = (int32_t)j;
            res.fail_offset = c.start;
            res.samples.clear();
            return res;
        }
        const uint64_t first = (uint64_t)j * shape.bs;
        for (uint32_t i = 0; i < c.head.bs && first + i < shape.total; i++) res.samples[first + i] = xs[i];
    }
    return res;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: flac_parse_main corpus.bin out.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    int n = 0, ok = 0;
    for (;;) {
        uint32_t len = 0;
        if (std::fread(&len, 4, 1, in) != 1) break;
        uint8_t* stream = new uint8_t[len ? len : 1];                 // (its exact size: ASan guards both ends)
        if (len && std::fread(stream, 1, len, in) != len) { std::fprintf(stderr, "truncated corpus\n"); return 2; }
        const Result r = decode(stream, len);
        delete[] stream;
        const uint32_t ns = r.status == BNHIP_FLAC_OK ? (uint32_t)r.samples.size() : 0u;
        std::fwrite(&r.status, 4, 1, out);
        std::fwrite(&r.frames, 4, 1, out);
        std::fwrite(&r.fail_offset, 8, 1, out);
        std::fwrite(&ns, 4, 1, out);
        if (ns) std::fwrite(r.samples.data(), 2, ns, out);
        n++;
        ok += r.status == BNHIP_FLAC_OK;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("streams %d ok %d\n", n, ok);
    return 0;
}
