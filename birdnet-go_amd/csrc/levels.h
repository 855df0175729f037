// The audio level bank (include/bnhip.h, "Audio level bank"; levels.hip, api_level.cpp): the per-source input level meter of
// calculateAudioLevel (internal/analysis/buffer_consumer.go:252-332).  The device reduces every frame of a call to two integers -
// the sum of the squares of its samples and the count of its full-scale samples - and the host turns them into the 0..100 level
// (audio_level, below: the reference's float64 operations in the reference's order).
//
// The host stages every frame at a LEVEL_FRAME_ALIGN boundary of the call's PCM, so a frame of 16- or 32-bit samples is read in
// whole 16-byte lines and no line holds two frames' samples.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bnhip {

constexpr long long LEVEL_MAX_FRAME = 1ll << 23;     // samples of a measured frame: up to here the sum of squares is at most 2^53,
                                                     // so the reference's running float64 sum is exact and equals the integer
constexpr int LEVEL_LINES = 4;                       // 16-byte lines (lane steps) of one lane: a tile is 256 lanes x 4 lines = 16 KiB
                                                     // of 16- or 32-bit PCM ("Audio level")

// samples a lane takes per step, and of one tile (one block)
constexpr int level_step(int bits) { return bits == 32 ? 4 : 8; }
constexpr long long level_tile(int bits) { return 256ll * LEVEL_LINES * level_step(bits); }
constexpr long long level_tiles(long long n, int bits) { return (n + level_tile(bits) - 1) / level_tile(bits); }
// bytes a frame's first sample is aligned to in the staged PCM: a 16-byte line that is also a whole sample
constexpr size_t level_frame_align(int bits) { return bits == 24 ? 48 : 16; }

// One measured frame of a call: n samples from byte `off` of the call's PCM (a multiple of level_frame_align).
struct LevelFrame {
    long long off, n;
};
// What the device answers per frame.
struct LevelRecord {
    unsigned long long sum_squares, clipped_samples;
};

// k_frame_levels.  pcm: the call's staged PCM of pcm_bytes bytes at `bits` (16, 24 or 32), 16-byte aligned; frames: [n_frames];
// tile0: [n_frames + 1] prefix of level_tiles(n, bits), tile0[n_frames] = n_tiles <= INT_MAX; rec: [n_frames], ZEROED before
// the launch (on the same stream) - the tiles of a frame add into its record.  A sample is measured as
// sample_pcm16(frame_sample<bits>) (pcm_sample.h): what the capture ring stores, a 16-bit sample as itself.
void launch_frame_levels(const void* pcm, long long pcm_bytes, int bits, const LevelFrame* frames, const long long* tile0, int n_frames,
                         long long n_tiles, LevelRecord* rec, hipStream_t s);

// The rule of bnhip.h "Audio level bank", host only: -> the level 0..100.  n == 0 -> 0.
int audio_level(uint64_t sum_squares, int64_t n_samples, bool clipping);

}  // namespace bnhip
