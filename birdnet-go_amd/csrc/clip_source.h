// What an entry of another unit needs of api_spectrogram.cpp to put a stage of its own in front of the render and the PNG encoder
// (the processed-audio chain there, the clip export of api_clips.cpp).
#pragma once
#include "api_oneshot.h"

namespace bnhip {

// Where the int16 clips of a render come from: the host's PCM, a decode on the device, the processed-audio chain, a cut out of
// analysed recordings.  reserve() adds the source's own parts to the call's DevCarve, fill() enqueues on the null stream what puts the
// clips at d_pcm, finish() runs after the call's synchronise.
struct ClipSource {
    virtual void reserve(DevCarve&) {}
    virtual hipError_t fill(const DevCarve& cv, int16_t* d_pcm, size_t pcm_bytes) = 0;
    virtual hipError_t finish(const DevCarve&) { return hipSuccess; }
    virtual ~ClipSource() {}
};

// what every render entry checks of the image and the level rule before any device is touched; -> the transform length, or a
// negative BNHIP_E_*
int spectrogram_image_check(int width, int height, const double* window, double top_db, double range_db);
// The render fused with the PNG encode for the clips `c` of any source, after the entry's own argument checks: one DevCarve, the
// source's fill, the render (through the one-shot resampler where rate_out differs from rate_in), the encoder, the streams' fetch,
// the source's finish.
int spectrogram_png_run(const char* what, int device, ClipSource& src, const Clips& c, int rate_in, int rate_out, int width, int height,
                        const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap,
                        uint64_t* offsets);

}  // namespace bnhip
