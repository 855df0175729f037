// The recordings of a file-analysis call (api_analyze.cpp, api_clips.cpp, api_channels.cpp): the three forms the C ABI states them
// in taken to one description, every refusal that needs neither a handle nor a device, and the recordings on the device - the slot
// block of analyze.h that the windows are framed from, filled by one copy per recording or, for recordings at their own rates,
// depths and channel counts, by the slot launch of resample.h behind the measurement of channels.h.  A fourth form states the
// recordings as FLAC streams: it is the channels form with every field read from STREAMINFO, and the device decoder of
// flac_decode.h writes the bytes that the copies would have brought.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "analyze.h"
#include "api_oneshot.h"
#include "channels.h"
#include "flac_decode.h"
#include "resample.h"

namespace bnhip {

constexpr long long ANALYZE_MAX_SAMPLES = (1ll << 36) - 1;

// a HIP call of a host-pointer entry: made while nothing has failed, its failure kept in the DevBlocks b (api_oneshot.h)
#define AN_HIP(b, call) do { if ((b).he == hipSuccess) (b).he = (call); } while (0)

struct RatePlan { int rate; int rec; ResamplePlan p; size_t tab_off; };     // rec: the first recording at that rate (for error texts)

// A call's recordings.  `plain`: one depth and nothing to resample or pick - the bytes are copied straight into the slots (the fast
// path); else they go up as they are in their files (the raw block) and the slot launch writes float32 slots of n_out samples.
struct Recordings {
    int n = 0;
    bool plain = true;
    int bits = 0;                                 // of the slots: the one depth of a plain burst, else 0 (float32)
    const int64_t* given = nullptr;               // the bits + lengths form: the caller's lengths, checked by the caller of describe()
    std::vector<bnhip_recording> recs;            // the other two forms: [n] length (in frames), rate, depth
    int model_rate = 0;
    std::vector<int64_t> n_out;                   // [n] samples at the model's rate
    std::vector<RatePlan> plans;                  // the distinct rates that differ from the model's, ascending
    std::vector<int> plan_of;                     // [n] index into plans, -1: at the model's rate
    long long n_tiles = 0;
    // the channels form: [n] each; select: a channel, CHANNEL_MIX or CHANNEL_AUTO (channels.h).  multi: a recording has two
    // channels or more (else the call is the mixed one)
    std::vector<int> channels, select;
    bool multi = false;
    std::vector<int32_t> chosen;                  // [n] of a multi burst, filled by the call: what was read
    // the FLAC form: the recordings' bytes are compressed streams (the call's pcm argument) at flac_offsets [n + 1]; every info OK
    std::vector<bnhip_flac_info> flac_infos;
    const uint64_t* flac_offsets = nullptr;
    bool flac() const { return !flac_infos.empty(); }

    // the samples of the slots: what the windows are framed over
    const int64_t* lengths() const { return recs.empty() ? given : n_out.data(); }
    int ch(int r) const { return channels.empty() ? 1 : channels[r]; }
    // bytes of recording r as the caller packs it, and its footprint in the raw block (every recording starts on a 16-byte line)
    size_t raw_bytes(int r) const {
        return recs.empty() ? (size_t)given[r] * analyze_sample_bytes(bits)
                            : (size_t)recs[r].length * ch(r) * analyze_sample_bytes(recs[r].bits_per_sample);
    }
    size_t raw_footprint(int r) const { return (raw_bytes(r) + 15) / 16 * 16; }
    // what a channels entry answers as `chosen` (one channel: channel 0 is what auto picks, and a mix of one channel is asked for
    // and answered as a mix)
    void copy_chosen(int32_t* out) const {
        for (int r = 0; r < n; r++) out[r] = multi ? chosen[r] : select[r] == CHANNEL_AUTO ? 0 : select[r];
    }
};

// The three forms -> rec, with every refusal of the recordings themselves; -> 0 or a negative BNHIP_E_*.  bits + lengths refuses
// nothing here (its entries check the table behind their other arguments).  A mono channels burst is the mixed call, and a
// one-rate, one-depth mixed burst is the plain one.
int describe(int bits, const int64_t* lengths, int n_recordings, Recordings* rec);
int describe(const bnhip_recording* recs, int n_recordings, int model_rate, Recordings* rec);
int describe(const bnhip_channels_recording* recs, int n_recordings, int model_rate, Recordings* rec);
// FLAC streams back to back in host memory: the channels form of what each STREAMINFO says, with select [n]; a stream that
// bnhip_flac_recording_info does not accept is refused here, by name
int describe(const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings, int model_rate, Recordings* rec);
// the channels form's own part of that: every refusal of the channel fields and of the burst's size in samples; fills recs,
// channels, select, multi.  measure: the measurement entry, where a float32 recording is refused whatever its select
int channels_check(const bnhip_channels_recording* recs, int n_recordings, bool measure, Recordings* rec);
// the depth, rate and length of recording r (float32: depth 0 is allowed)
int recording_check(const bnhip_recording& q, int r, bool float32);
// the geometry of every rate of the call; a phase table that does not fit LDS is refused here, before any allocation
int rate_plans(Recordings* rec);

// The measurement's descriptors and their tile prefix [n + 1] (channels.h) for the CHANNEL_AUTO recordings of rec, or for all
struct EnergyPlan {
    std::vector<EnergyDesc> desc;
    std::vector<long long> tile0;
    long long n_tiles() const { return tile0.empty() ? 0 : tile0.back(); }
};
EnergyPlan energy_plan(const Recordings& rec, bool all);

// What a call's recordings need on the device, worked out on the host.  The slot block: recording r at slot[2 r] (analyze.h).
// Off the fast path: the raw block, a descriptor per recording and the tile prefix; multi: beside them the channel counts and the
// selection table [n] each, and the measurement of the recordings that ask for one
struct SlotPlan {
    size_t block_bytes = 0, raw_bytes = 0, rs_lds = 0;
    size_t flac_bytes = 0, flac_ws = 0, flac_res = 0;      // the FLAC form: the compressed burst, the decoder's workspace, its results
    std::vector<ResampleSlotDesc> desc;
    std::vector<long long> tile0;
    std::vector<int> chsel;
    EnergyPlan en;
};
// fills slot [n][2]
SlotPlan slot_plan(const Recordings& rec, long long* slot);

// Where a call has reserved the plan's parts, as handles of cv: the slot block (block_room bytes of it are zero-filled on the fast
// path), the raw block, the descriptors, the tile prefix, the counts and selections, the measurement's descriptors, tile prefix,
// partials and sums, and for the FLAC form the compressed burst, the decoder's workspace and its results
struct SlotDev {
    const DevCarve* cv;
    size_t block_room;
    size_t block, raw, desc, tile0, chsel, edesc, etile0, part, energy, flac_in, flac_ws, flac_res;
    template <class T = char> T* at(size_t part) const { return cv->at<T>(part); }
};
SlotDev slot_reserve(const SlotPlan& sp, DevCarve& cv);

// The recordings go up and the slot block is filled, on s: the slots' zero fill and one copy per recording into its slot, or
// one copy per recording into the raw block, the tables, the measurement where a recording asks for one, and the slot launch
// (k_resample_slots writes every slot whole, its zeros included).  The FLAC form: one copy of the compressed burst, the raw block
// (or on the fast path the slots) cleared, and the decoder's launches in place of the copies; the rest is the same.  The first
// failure is left in b.
void slot_upload(const SlotPlan& sp, const void* pcm, const Recordings& rec, const long long* slot, int device, const SlotDev& dv, hipStream_t s,
                 DevBlocks& b);

}  // namespace bnhip
