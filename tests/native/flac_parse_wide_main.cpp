// The recording reader of the device FLAC decoder (birdnet-go_amd/csrc/flac_parse.h: flac_frame_head with a stream's channels and
// depth, flac_parse_frame_wide, flac_decorrelate) run on the host, serially, in the order of the kernels of flac_decode.hip as
// bnhip_flac_decode_recordings runs them: scan, parse + CRC-16, link, restore.  Built with plain g++ under ASan + UBSan by
// tests/test_flac_wide_ref.py; every stream is copied to a heap block of its exact size first, so a read past it is caught.
//
//   flac_parse_wide_main corpus.bin out.bin
// corpus.bin: records of u32 length + bytes.  out.bin: per record i32 status, i32 frames, u64 fail_offset, u32 n_bytes, then
// n_bytes of interleaved PCM at the stream's depth (int16, or packed little-endian 3-byte samples), zero where no frame was
// restored; n_bytes is 0 unless the metadata is accepted.  stdout: "streams N ok M".
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
    std::vector<uint8_t> pcm;
};

Result decode(const uint8_t* stream, size_t n_bytes) {
    Result res;
    bnhip_flac_info info;
    flac_stream_info(stream, n_bytes, &info, true);
    res.status = info.status;
    if (info.status != BNHIP_FLAC_OK) return res;
    FlacStreamShape shape;
    shape.rate = info.rate;
    shape.bs = info.max_block;
    shape.total = (uint32_t)info.total_samples;
    shape.frames = (uint32_t)((info.total_samples + shape.bs - 1) / shape.bs);
    shape.channels = info.channels;
    shape.bits = info.bits;
    const uint32_t bytes_per = shape.bits / 8, pitch = bytes_per * shape.channels;
    res.pcm.assign((size_t)shape.total * pitch, 0);
    if (flacdec_too_short(shape.frames, n_bytes - info.audio_offset, shape.channels, shape.bits)) {
        res.status = BNHIP_FLAC_CORRUPT;
        res.fail_offset = info.audio_offset;
        return res;
    }
    const size_t cap = 2 * (size_t)shape.frames + 64, frame_cap = flacdec_frame_cap(shape.bs, shape.channels, shape.bits);
    std::vector<Cand> cands;
    for (uint64_t pos = info.audio_offset; pos < n_bytes; pos++) {
        FlacFrameHead h;
        if (!flac_frame_head(stream + pos, n_bytes - pos, shape, &h)) continue;
        if (cands.size() >= cap) { res.status = BNHIP_FLAC_UNSUPPORTED; return res; }
        cands.push_back(Cand{pos, 0, h});
    }
    for (Cand& c : cands) {
        size_t avail = n_bytes - c.start;
        if (avail > frame_cap) avail = frame_cap;
        FlacCountSink sink;
        size_t bytes = 0;
        uint32_t assign = 0;
        if (c.head.bs > shape.bs || c.head.bytes > avail) continue;
        if (flac_parse_frame_wide(stream + c.start, avail, c.head.bytes, c.head.bs, shape, sink, &bytes, &assign) != FLACP_OK) continue;
        if (flac_crc16(stream + c.start, bytes) != 0) continue;
        c.end = c.start + bytes;
    }
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
    }
    // restore: every frame of the chain, as far as it got
    std::vector<int32_t> xs((size_t)shape.bs * shape.channels);
    uint32_t bad = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < (uint32_t)chain.size(); j++) {
        const Cand& c = *chain[j];
        int32_t coefs[FLACDEC_MAX_ORDER];
        FlacWideSink sink{xs.data(), coefs, shape.bs, 0u};
        size_t bytes = 0;
        uint32_t assign = 0;
        bool ok = flac_parse_frame_wide(stream + c.start, (size_t)(c.end - c.start), c.head.bytes, c.head.bs, shape, sink, &bytes, &assign) == FLACP_OK;
        if (ok && assign >= 8)
            for (uint32_t i = 0; i < c.head.bs; i++) {
                int32_t left, right;
                if (!flac_decorrelate(assign, xs[i], xs[shape.bs + i], shape.bits, &left, &right)) ok = false;
                xs[i] = left;
                xs[shape.bs + i] = right;
            }
        if (!ok) {
            if (j < bad) bad = j;
            continue;
        }
        const uint64_t first = (uint64_t)j * shape.bs;
        for (uint32_t i = 0; i < c.head.bs && first + i < shape.total; i++)
            for (uint32_t ch = 0; ch < shape.channels; ch++)
                for (uint32_t k = 0; k < bytes_per; k++)
                    res.pcm[(size_t)(first + i) * pitch + ch * bytes_per + k] = (uint8_t)((uint32_t)xs[(size_t)ch * shape.bs + i] >> (8 * k));
    }
    if (bad != 0xFFFFFFFFu) {                              // (a frame of the chain: in front of a break, if there is one)
        res.status = BNHIP_FLAC_CORRUPT;
        res.frames = (int32_t)bad;
        res.fail_offset = chain[bad]->start;
    }
    return res;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: flac_parse_wide_main corpus.bin out.bin\n"); return 2; }
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
        const uint32_t nb = (uint32_t)r.pcm.size();
        std::fwrite(&r.status, 4, 1, out);
        std::fwrite(&r.frames, 4, 1, out);
        std::fwrite(&r.fail_offset, 8, 1, out);
        std::fwrite(&nb, 4, 1, out);
        if (nb) std::fwrite(r.pcm.data(), 1, nb, out);
        n++;
        ok += r.status == BNHIP_FLAC_OK;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("streams %d ok %d\n", n, ok);
    return 0;
}
