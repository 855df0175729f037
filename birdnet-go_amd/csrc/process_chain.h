// The processed-audio chain denoise -> normalise -> gain as a sequence of enqueues on the null stream (api_denoise.cpp), for the
// entries that run it: bnhip_process_pcm16, bnhip_process_ragged_pcm16 and, in front of the render and the PNG encoder,
// bnhip_process_spectrogram_png_ragged_pcm16 (api_spectrogram.cpp).  The stage sequence is stated once, for a uniform batch and a
// ragged burst alike.
//
// Denoise and normalise each read one buffer and write another; the gain works in place.  So a call needs the buffer the
// processed clips are to end in (`d_final`) and, with at least one of the two stages active, one more (`d_other`): the input goes
// where chain_input says, and the stages alternate between the two so that the last one writes d_final.
#pragma once
#include "api_oneshot.h"

namespace bnhip {

// frame 0 = no denoise; normalize 0 = no normalisation; gain_db 0 = no gain
struct ChainArgs {
    int rate = 0, frame = 0;
    double nr_db = 0.0, nf_db = 0.0;
    int normalize = 0;
    double target_lufs = 0.0, true_peak_dbtp = 0.0, gain_db = 0.0;
};

// what every chain entry checks before any device is touched: the clips' dimensions, the active stages' own arguments, the gain's
// range (IsValidGainDB, process.go:198-203), "no filter active"; -> 0 or a negative BNHIP_E_*
int chain_check(const Clips& c, const ChainArgs& a);

// the chain's parts of the call's DevCarve, besides d_final: the second clip buffer, the records, the stages' workspaces
struct ChainParts { size_t pcm_bytes = 0, res_bytes = 0, o_other = 0, o_res = 0, o_lws = 0, o_dws = 0; };
ChainParts chain_reserve(DevCarve& cv, const Clips& c, const ChainArgs& a);

// where the caller puts the unprocessed clips (d_final or the part at o_other) so that the processed ones end at d_final
int16_t* chain_input(const DevCarve& cv, const ChainParts& p, const ChainArgs& a, int16_t* d_final);

// The device (already made current) has the stages' tables looked up or uploaded and the active stages enqueued on the null
// stream: chain_input -> ... -> d_final, the records at o_res.  int16 between the stages, no gain clamp, no gate fallback.
int chain_enqueue(const char* what, int device, const DevCarve& cv, const ChainParts& p, const Clips& c, const ChainArgs& a,
                  int16_t* d_final);

}  // namespace bnhip
