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
//
// Recordings (bnhip_flac_decode_recordings*, bnhip_analyze_flac_*): streams of 1 or 2 channels at 16 or 24 bits, to interleaved PCM
// at each stream's own depth - int16, or packed little-endian 3-byte samples: what a WAV data chunk of the same audio holds - at
// a byte position per stream.  A burst that holds any stream but mono 16-bit ones runs the wide instantiations of the parse and
// the restore (int32 samples, 64-bit products, the stereo decorrelation and its range check by the whole wavefront); a burst of
// mono 16-bit streams runs the clips' instantiations whichever entry it came through.  A recording's restore also writes the
// frames of a chain that broke (the stream is CORRUPT there; the samples behind the break stay as the entry cleared them: zero),
// and a frame whose samples leave the depth's range leaves its own samples zero.
//
// The LDS decision for wide streams: the restore keeps a frame's bytes and its samples in LDS, as the clips' does, and the samples
// are int32 [channels][block size].  At 2 channels x 24 bits that is 6.125 + 8 bytes per sample frame, so FLACDEC_MAX_BLOCK_WIDE =
// 8192 (113 KB + slack of the 160 KB) is the cap of every stream that is not mono 16-bit; mono 16-bit stays at 16384.  Both launches
// size their LDS by the burst's largest frame, not by the cap: stereo 24-bit at 4096 takes 57 KB (two frames resident per CU),
// stereo 16-bit at 4096 49 KB (three), mono 16-bit at 4096 16 KB (nine).  A workspace scratch for the samples was not taken: the
// predictor of an order above 8 reads its history back from where the samples are kept, once per coefficient per sample.
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
    unsigned long long pcm0;                            // the byte of d_pcm the clip's first sample goes to (even for 16-bit streams)
    uint32_t rate, bs, total, frames;
    uint32_t channels, bits;
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
    bool wide = false;                                  // a stream that is not mono 16-bit: the wide instantiations run
    bool recordings = false;                            // the chain of a CORRUPT stream is restored up to its break
    size_t frame_lds = 0, sample_lds = 0;               // the burst's largest frame: its bytes (up to a 16-byte line), its samples
    long long tiles = 0, cands = 0, frames = 0;         // the three grids
    std::vector<unsigned char> tables;                  // FlacDecStream [n] | tile0, cand0, frame0 long long [n + 1] each
    const FlacDecStream* rows = nullptr;
    const long long *tile0 = nullptr, *cand0 = nullptr, *frame0 = nullptr;
    uint32_t *count = nullptr, *head = nullptr, *chain = nullptr, *bad = nullptr;      // [n], [frames], [frames], [n]
    size_t zero_bytes = 0;                              // count | head | chain, contiguous, cleared per call
    FlacDecCand* cand = nullptr;                        // [cands]
};
// What the entries check of a burst before any device is touched (offsets ascend, the totals fit the grids, every accepted
// stream's fields are ones the kernels can run on); -> 0 or -1 with *why set.  *pcm_samples: the sum of the lens.  recordings:
// the infos are bnhip_flac_recording_info's, and *pcm_samples counts bytes: the sum of total x channels x bits / 8.
int flacdec_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples, const char** why,
                  bool recordings = false);
size_t flacdec_workspace_bytes(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, bool recordings = false);
FlacDecWork flacdec_work(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, void* d_block, bool recordings = false);
// the PCM bytes of an accepted stream (0 for any other), and where a call puts them instead of back to back
inline size_t flacdec_pcm_bytes(const bnhip_flac_info& in) {
    return in.status == BNHIP_FLAC_OK ? (size_t)in.total_samples * in.channels * (in.bits / 8) : 0;
}
void flacdec_place(FlacDecWork& w, int stream, unsigned long long pcm_byte);

// d_streams: the burst's bytes; d_pcm [pcm_cap_bytes]; d_result [n_streams].  Enqueues the table copy, the clears and the five
// kernels; nothing is synchronised.  No kernel reads outside a stream's bytes or writes outside its clip's span or past the cap.
void launch_flacdec(const uint8_t* d_streams, const FlacDecWork& w, void* d_pcm, size_t pcm_cap_bytes, bnhip_flac_decode_result* d_result,
                    hipStream_t s);

// What an entry of another unit needs of api_flac_decode.cpp (bnhip_flac_spectrogram_png of api_spectrogram.cpp), both -> 0 or a
// negative BNHIP_E_* with the error text set:
// the metadata of a burst in host memory, read as bnhip_flac_stream_info reads one stream
int flacdec_read_infos(const uint8_t* streams, int n_streams, const uint64_t* offsets, std::vector<bnhip_flac_info>* infos,
                       bool recordings = false);
// flacdec_check as an entry answers it
int flacdec_burst_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples, bool recordings = false);

}  // namespace bnhip
