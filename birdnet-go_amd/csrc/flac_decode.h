// FLAC decoding of a burst of saved clips on the device (flac_decode.hip, api_flac_decode.cpp bnhip_flac_decode_*): n_streams RFC 9639
// streams back to back, mono, 16 bits, fixed block size 16..16384 (flac_parse.h states the frame reader), to the ragged packing of
// ragged.h: int16 clips back to back, lens[c] = STREAMINFO's sample count for a stream whose metadata is accepted and 0 otherwise.
//
// Frame boundaries are found only by parsing, so a burst takes five launches whatever it holds:
//   k_flacdec_scan     every byte of every stream's audio region is tested as a frame header of that stream (flac_frame_head); the
//                      survivors go to the stream's candidate list, sized 2 F + 64 for F frames
//   k_flacdec_parse    a wavefront per candidate parses its frame to its end without predicting, checks CRC-16, and hangs a valid
//                      candidate on its frame number's list
//   k_flacdec_link     a wavefront per stream walks from the audio offset: frame j is the valid candidate numbered j that starts
//                      exactly where frame j - 1 ended, and frame F - 1 ends exactly at the stream's end
//   k_flacdec_restore  a wavefront per chain frame decodes it again with the predictor and writes its samples; no other candidate
//                      writes anything, so a CRC-valid frame image inside another frame's payload changes no sample
//   k_flacdec_finish   a stream with a sample outside int16 is CORRUPT at the first such frame
// A stream whose candidates overflow its list (an adversarial stream: more than F + 64 false headers with a valid CRC-8) is reported
// BNHIP_FLAC_UNSUPPORTED.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bnhip.h"

namespace bnhip {

constexpr int FLACDEC_SCAN_TILE = 4096;                 // byte positions a scan block tests
constexpr unsigned long long FLACDEC_MAX_BYTES = 1ull << 40;       // of a burst: keeps the scan grid inside 31 bits
constexpr long long FLACDEC_MAX_CANDS = (1ll << 31) - 1;           // of a burst: candidate slots, one wavefront each

struct FlacDecStream {                                  // a row per stream, built on the host
    unsigned long long begin, end;                      // the stream's bytes in d_streams
    unsigned long long audio;                           // the first frame header, from `begin`
    unsigned long long pcm0;                            // the clip's first sample in d_pcm
    uint32_t rate, bs, total, frames;
    uint32_t cand_cap;
    int32_t status;                                     // the metadata's: not OK = no audio region, no frames, no candidates
};
struct FlacDecCand {
    unsigned long long start, end;                      // from the stream's begin; end 0 = not a frame
    uint32_t number, bs, head_bytes, next;              // next: the following candidate (index + 1) of this number's list
};
static_assert(sizeof(FlacDecCand) == 32, "FlacDecCand layout");

// The geometry of one call and its scratch; every array lives in one caller-supplied device block, the host tables at its head.
struct FlacDecWork {
    int n_streams = 0;
    uint32_t max_bs = 0;
    long long tiles = 0, cands = 0, frames = 0;         // the three grids
    std::vector<unsigned char> tables;                  // FlacDecStream [n] | tile0, cand0, frame0 long long [n + 1] each
    const FlacDecStream* rows = nullptr;
    const long long *tile0 = nullptr, *cand0 = nullptr, *frame0 = nullptr;
    uint32_t *count = nullptr, *head = nullptr, *chain = nullptr, *bad = nullptr;      // [n], [frames], [frames], [n]
    size_t zero_bytes = 0;                              // count | head | chain, contiguous, cleared per call
    FlacDecCand* cand = nullptr;                        // [cands]
};
// What the entries check of a burst before any device is touched (offsets ascend, the totals fit the grids, every accepted
// stream's fields are ones the kernels can run on); -> 0 or -1 with *why set.  *pcm_samples: the sum of the lens.
int flacdec_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples, const char** why);
size_t flacdec_workspace_bytes(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets);
FlacDecWork flacdec_work(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, void* d_block);

// d_streams: the burst's bytes; d_pcm int16 [pcm_cap]; d_result [n_streams].  Enqueues the table copy, the clears and the five
// kernels; nothing is synchronised.  No kernel reads outside a stream's bytes or writes outside its clip's span or past pcm_cap.
void launch_flacdec(const uint8_t* d_streams, const FlacDecWork& w, int16_t* d_pcm, size_t pcm_cap, bnhip_flac_decode_result* d_result,
                    hipStream_t s);

// What an entry of another unit needs of api_flac_decode.cpp (bnhip_flac_spectrogram_png of api_spectrogram.cpp), both -> 0 or a
// negative BNHIP_E_* with the error text set:
// the metadata of a burst in host memory, read as bnhip_flac_stream_info reads one stream
int flacdec_read_infos(const uint8_t* streams, int n_streams, const uint64_t* offsets, std::vector<bnhip_flac_info>* infos);
// flacdec_check as an entry answers it
int flacdec_burst_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples);

}  // namespace bnhip
