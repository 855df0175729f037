//go:build hip

// Package hip binds libbnhip.so (the MI355X-native BirdNET engine) behind the reference's backend seam
// inference.Classifier / inference.EmbeddingExtractor (internal/inference/backend.go:8-29).
//
// Shape follows the reference's own native-accelerator precedent, the OpenVINO cgo shim
// (internal/inference/openvino/backend_openvino.go): dlopen'd library, process-global init under a
// mutex, one native handle per classifier, C-allocated input staging, sentinel "unavailable" error so
// callers fall back (internal/classifier/birdnet.go:321-335), and - because the native error text is
// thread-local - runtime.LockOSThread around every native call plus its error fetch
// (backend_openvino.go:480,581,729,805).
//
// NOTE: no Go toolchain exists in this repository's build environment.  The C preamble below is
// nevertheless compiled and executed: tests/test_cabi.py extracts it verbatim, builds it with
// `gcc -Wall -Wextra -Werror` and drives exactly the call sequence of this file through it
// (tests/native/cabi_driver.c), on the CPU for the error paths and on the GPU for the full sequence.
package hip

/*
#cgo LDFLAGS: -ldl
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct bnhip_model bnhip_model;
typedef int  (*fn_init)(int*);
typedef void (*fn_shutdown)(void);
typedef int  (*fn_model_create)(const void*, size_t, const char*, bnhip_model**);
typedef int  (*fn_model_info)(const bnhip_model*, int*, int*, int*);
typedef int  (*fn_predict)(bnhip_model*, const float*, int, float*, float*);
typedef int  (*fn_predict_topk)(bnhip_model*, const float*, int, int, double, int, float*, int32_t*);
typedef void (*fn_model_destroy)(bnhip_model*);
typedef const char* (*fn_last_error)(void);
typedef int  (*fn_predict_pcm16)(bnhip_model*, const int16_t*, int, float*, float*);
typedef int  (*fn_us_frame_cv)(int, const double*, int, int, int, int, int, int, double*, int32_t*);
typedef struct bnhip_resampler bnhip_resampler;
typedef int  (*fn_rs_create)(int, int, int, bnhip_resampler**);
typedef int  (*fn_rs_estimate)(const bnhip_resampler*, int);
typedef int  (*fn_rs_process_pcm16)(bnhip_resampler*, const int16_t*, int, int16_t*, int, int*);
typedef int  (*fn_rs_flush_pcm16)(bnhip_resampler*, int16_t*, int, int*);
typedef void (*fn_rs_destroy)(bnhip_resampler*);
typedef int  (*fn_host_alloc)(size_t, void**);
typedef int  (*fn_host_free)(void*);
typedef int  (*fn_predict_pcm_topk)(bnhip_model*, const void*, int, int, int, double, int, float*, int32_t*);
typedef struct bnhip_windows bnhip_windows;
typedef int  (*fn_win_create)(size_t, size_t, int, bnhip_windows**);
typedef int  (*fn_win_info)(const bnhip_windows*, size_t*, int*, int*, int*);
typedef int  (*fn_win_add_source)(bnhip_windows*, const char*, size_t, int*);
typedef int  (*fn_win_remove_source)(bnhip_windows*, int);
typedef int  (*fn_win_write)(bnhip_windows*, int, const void*, size_t);
typedef int  (*fn_win_collect)(bnhip_windows*, int, int*, int*, const void**);
typedef int  (*fn_win_stats)(const bnhip_windows*, int, uint64_t*, uint64_t*, size_t*);
typedef int  (*fn_win_reset)(bnhip_windows*, int);
typedef void (*fn_win_destroy)(bnhip_windows*);
typedef int  (*fn_win_predict_topk)(bnhip_windows*, bnhip_model*, int, int, double, int, int*, int*, float*, int32_t*, const void**);
typedef struct bnhip_resampler_bank bnhip_resampler_bank;
typedef int  (*fn_rb_create)(int, int, int, int, bnhip_resampler_bank**);
typedef int  (*fn_rb_add_stream)(bnhip_resampler_bank*, int*);
typedef int  (*fn_rb_remove_stream)(bnhip_resampler_bank*, int);
typedef int  (*fn_rb_estimate)(const bnhip_resampler_bank*, int);
typedef int  (*fn_rb_process_pcm16)(bnhip_resampler_bank*, int, const int*, const int16_t* const*, const int*, int16_t*, size_t, int*);
typedef int  (*fn_rb_flush_pcm16)(bnhip_resampler_bank*, int, const int*, int16_t*, size_t, int*);
typedef int  (*fn_win_write_resampled)(bnhip_windows*, bnhip_resampler_bank*, int, const int*, const int*, const int16_t* const*, const int*);
typedef void (*fn_rb_destroy)(bnhip_resampler_bank*);
typedef struct bnhip_eq_bank bnhip_eq_bank;
typedef int  (*fn_eq_create)(int, int, bnhip_eq_bank**);
typedef int  (*fn_eq_add_stream)(bnhip_eq_bank*, int*);
typedef int  (*fn_eq_remove_stream)(bnhip_eq_bank*, int);
typedef int  (*fn_eq_set_chain)(bnhip_eq_bank*, int, const double*, int, const int*, double);
typedef int  (*fn_eq_reset)(bnhip_eq_bank*, int);
typedef int  (*fn_eq_process_pcm16)(bnhip_eq_bank*, int, const int*, const int16_t* const*, const int*, int16_t*, size_t, int*);
typedef int  (*fn_win_write_equalized)(bnhip_windows*, bnhip_eq_bank*, int, const int*, const int*, const int16_t* const*, const int*);
typedef void (*fn_eq_destroy)(bnhip_eq_bank*);
typedef struct bnhip_soundlevel_bank bnhip_soundlevel_bank;
// bnhip.h's bnhip_sound_level, restated field for field (tests/test_soundlevel_bank.py compares sizeof and every offsetof)
typedef struct bnhip_sound_level {
    int stream, frame;
    int duration_s, n_bands;
    double center_hz[32], min_db[32], max_db[32], mean_db[32];
    int sample_count[32];
} bnhip_sound_level;
typedef int  (*fn_sl_bands)(int, double*, int, int*);
typedef int  (*fn_sl_create)(int, int, int, const double*, int, bnhip_soundlevel_bank**);
typedef int  (*fn_sl_add_stream)(bnhip_soundlevel_bank*, int, int*);
typedef int  (*fn_sl_remove_stream)(bnhip_soundlevel_bank*, int);
typedef int  (*fn_sl_reset)(bnhip_soundlevel_bank*, int);
typedef int  (*fn_sl_process_pcm16)(bnhip_soundlevel_bank*, int, const int*, const int16_t* const*, const int*, bnhip_sound_level*, int, int*);
typedef void (*fn_sl_destroy)(bnhip_soundlevel_bank*);
typedef int  (*fn_range_heatmap)(bnhip_model*, const float*, int, int, int, int, float*);
typedef int  (*fn_spec_size)(int, int*, int*);
typedef int  (*fn_spec_pcm16)(int, const int16_t*, int, int, int, int, int, int, const double*, double, double, uint8_t*);
// bnhip.h's bnhip_loudness, restated field for field (tests/test_loudness_ref.py compares the two declarations)
typedef struct bnhip_loudness {
    double integrated_lufs, true_peak_dbtp, true_peak;
    double target_gain_db, lift_db, planned_gain_db, gain_db, factor, output_lufs;
    int flags, reserved;
} bnhip_loudness;
typedef int  (*fn_loud_measure)(int, const int16_t*, int, int, int, bnhip_loudness*, double*);
typedef int  (*fn_loud_normalize)(int, const int16_t*, int, int, int, double, double, double, int, int16_t*, bnhip_loudness*);
typedef int  (*fn_flac_max_bytes)(int, int, int, size_t*);
typedef int  (*fn_flac_encode_pcm16)(int, const int16_t*, int, int, int, const double*, int, uint8_t*, size_t, uint64_t*);
typedef int  (*fn_png_max_bytes)(int, int, int, size_t*);
typedef int  (*fn_png_encode_u8)(int, const uint8_t*, int, int, int, const uint8_t*, uint8_t*, size_t, uint64_t*);
typedef int  (*fn_spec_png_pcm16)(int, const int16_t*, int, int, int, int, int, int, const double*, double, double, const uint8_t*, uint8_t*, size_t,
                                  uint64_t*);
typedef int  (*fn_spec_ragged_pcm16)(int, const int16_t*, int, const int*, int, int, int, int, const double*, double, double, uint8_t*);
typedef int  (*fn_spec_png_ragged_pcm16)(int, const int16_t*, int, const int*, int, int, int, int, const double*, double, double, const uint8_t*,
                                         uint8_t*, size_t, uint64_t*);
typedef int  (*fn_loud_flac_pcm16)(int, const int16_t*, int, int, int, double, double, double, int, int, bnhip_loudness*, uint8_t*, size_t, uint64_t*);
typedef int  (*fn_flac_lpc_encode_pcm16)(int, const int16_t*, int, int, int, const double*, int, uint8_t*, size_t, uint64_t*, int);
typedef int  (*fn_loud_flac_lpc_pcm16)(int, const int16_t*, int, int, int, double, double, double, int, int, bnhip_loudness*, uint8_t*, size_t, uint64_t*, int);

typedef struct {
    void* handle;
    fn_init init; fn_shutdown shutdown; fn_model_create model_create; fn_model_info model_info;
    fn_predict predict; fn_predict_topk predict_topk; fn_model_destroy model_destroy; fn_last_error last_error;
    fn_predict_pcm16 predict_pcm16; fn_us_frame_cv us_frame_cv;
    fn_rs_create rs_create; fn_rs_estimate rs_estimate; fn_rs_process_pcm16 rs_process_pcm16; fn_rs_flush_pcm16 rs_flush_pcm16;
    fn_rs_destroy rs_destroy;
    fn_host_alloc host_alloc; fn_host_free host_free;
    fn_win_create win_create; fn_win_info win_info; fn_win_add_source win_add_source; fn_win_remove_source win_remove_source;
    fn_win_write win_write; fn_win_collect win_collect; fn_win_stats win_stats; fn_win_reset win_reset; fn_win_destroy win_destroy;
    fn_predict_pcm_topk predict_pcm_topk; fn_win_predict_topk win_predict_topk;
    fn_rb_create rb_create; fn_rb_add_stream rb_add_stream; fn_rb_remove_stream rb_remove_stream; fn_rb_estimate rb_estimate;
    fn_rb_process_pcm16 rb_process_pcm16; fn_rb_flush_pcm16 rb_flush_pcm16; fn_win_write_resampled win_write_resampled;
    fn_rb_destroy rb_destroy;
    fn_eq_create eq_create; fn_eq_add_stream eq_add_stream; fn_eq_remove_stream eq_remove_stream; fn_eq_set_chain eq_set_chain;
    fn_eq_reset eq_reset; fn_eq_process_pcm16 eq_process_pcm16; fn_win_write_equalized win_write_equalized; fn_eq_destroy eq_destroy;
    fn_sl_bands sl_bands; fn_sl_create sl_create; fn_sl_add_stream sl_add_stream; fn_sl_remove_stream sl_remove_stream;
    fn_sl_reset sl_reset; fn_sl_process_pcm16 sl_process_pcm16; fn_sl_destroy sl_destroy;
    fn_range_heatmap range_heatmap;
    fn_spec_size spec_size; fn_spec_pcm16 spec_pcm16;
    fn_loud_measure loud_measure; fn_loud_normalize loud_normalize;
    fn_flac_max_bytes flac_max_bytes; fn_flac_encode_pcm16 flac_encode_pcm16; fn_loud_flac_pcm16 loud_flac_pcm16;
    fn_flac_lpc_encode_pcm16 flac_lpc_encode_pcm16; fn_loud_flac_lpc_pcm16 loud_flac_lpc_pcm16;
    fn_png_max_bytes png_max_bytes; fn_png_encode_u8 png_encode_u8; fn_spec_png_pcm16 spec_png_pcm16;
    fn_spec_ragged_pcm16 spec_ragged_pcm16; fn_spec_png_ragged_pcm16 spec_png_ragged_pcm16;
} bnbind_t;
static bnbind_t BN;
static char bnbind_errbuf[256];

// A failed resolve closes the library and clears the table: the next bnbind_load starts from scratch
// ("idempotent and retryable", backend_openvino.go:477-506) instead of returning success with NULL pointers.
static const char* bnbind_fail(const char* what, const char* detail) {
    snprintf(bnbind_errbuf, sizeof bnbind_errbuf, "%s%s", what, detail ? detail : "");
    if (BN.handle) dlclose(BN.handle);
    memset(&BN, 0, sizeof BN);
    return bnbind_errbuf;
}
#define BN_RESOLVE(field, sym) do { *(void**)(&BN.field) = dlsym(BN.handle, sym); \
    if (!BN.field) return bnbind_fail("missing symbol ", sym); } while (0)

static const char* bnbind_load(const char* path) {
    if (BN.handle) return NULL;
    BN.handle = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!BN.handle) return bnbind_fail("", dlerror());
    BN_RESOLVE(init, "bnhip_init"); BN_RESOLVE(shutdown, "bnhip_shutdown");
    BN_RESOLVE(model_create, "bnhip_model_create"); BN_RESOLVE(model_info, "bnhip_model_info");
    BN_RESOLVE(predict, "bnhip_predict"); BN_RESOLVE(predict_topk, "bnhip_predict_topk");
    BN_RESOLVE(model_destroy, "bnhip_model_destroy"); BN_RESOLVE(last_error, "bnhip_last_error");
    BN_RESOLVE(predict_pcm16, "bnhip_predict_pcm16"); BN_RESOLVE(us_frame_cv, "bnhip_us_frame_cv");
    BN_RESOLVE(rs_create, "bnhip_resampler_create"); BN_RESOLVE(rs_estimate, "bnhip_resampler_estimate");
    BN_RESOLVE(rs_process_pcm16, "bnhip_resampler_process_pcm16"); BN_RESOLVE(rs_flush_pcm16, "bnhip_resampler_flush_pcm16");
    BN_RESOLVE(rs_destroy, "bnhip_resampler_destroy");
    BN_RESOLVE(host_alloc, "bnhip_host_alloc"); BN_RESOLVE(host_free, "bnhip_host_free");
    BN_RESOLVE(win_create, "bnhip_windows_create"); BN_RESOLVE(win_info, "bnhip_windows_info");
    BN_RESOLVE(win_add_source, "bnhip_windows_add_source"); BN_RESOLVE(win_remove_source, "bnhip_windows_remove_source");
    BN_RESOLVE(win_write, "bnhip_windows_write"); BN_RESOLVE(win_collect, "bnhip_windows_collect");
    BN_RESOLVE(win_stats, "bnhip_windows_stats"); BN_RESOLVE(win_reset, "bnhip_windows_reset");
    BN_RESOLVE(win_destroy, "bnhip_windows_destroy");
    BN_RESOLVE(predict_pcm_topk, "bnhip_predict_pcm_topk"); BN_RESOLVE(win_predict_topk, "bnhip_windows_predict_topk");
    BN_RESOLVE(rb_create, "bnhip_resampler_bank_create"); BN_RESOLVE(rb_add_stream, "bnhip_resampler_bank_add_stream");
    BN_RESOLVE(rb_remove_stream, "bnhip_resampler_bank_remove_stream"); BN_RESOLVE(rb_estimate, "bnhip_resampler_bank_estimate");
    BN_RESOLVE(rb_process_pcm16, "bnhip_resampler_bank_process_pcm16"); BN_RESOLVE(rb_flush_pcm16, "bnhip_resampler_bank_flush_pcm16");
    BN_RESOLVE(win_write_resampled, "bnhip_windows_write_resampled"); BN_RESOLVE(rb_destroy, "bnhip_resampler_bank_destroy");
    BN_RESOLVE(eq_create, "bnhip_eq_bank_create"); BN_RESOLVE(eq_add_stream, "bnhip_eq_bank_add_stream");
    BN_RESOLVE(eq_remove_stream, "bnhip_eq_bank_remove_stream"); BN_RESOLVE(eq_set_chain, "bnhip_eq_bank_set_chain");
    BN_RESOLVE(eq_reset, "bnhip_eq_bank_reset"); BN_RESOLVE(eq_process_pcm16, "bnhip_eq_bank_process_pcm16");
    BN_RESOLVE(win_write_equalized, "bnhip_windows_write_equalized"); BN_RESOLVE(eq_destroy, "bnhip_eq_bank_destroy");
    BN_RESOLVE(sl_bands, "bnhip_soundlevel_bands"); BN_RESOLVE(sl_create, "bnhip_soundlevel_bank_create");
    BN_RESOLVE(sl_add_stream, "bnhip_soundlevel_bank_add_stream"); BN_RESOLVE(sl_remove_stream, "bnhip_soundlevel_bank_remove_stream");
    BN_RESOLVE(sl_reset, "bnhip_soundlevel_bank_reset"); BN_RESOLVE(sl_process_pcm16, "bnhip_soundlevel_bank_process_pcm16");
    BN_RESOLVE(sl_destroy, "bnhip_soundlevel_bank_destroy");
    BN_RESOLVE(range_heatmap, "bnhip_range_heatmap");
    BN_RESOLVE(spec_size, "bnhip_spectrogram_size"); BN_RESOLVE(spec_pcm16, "bnhip_spectrogram_pcm16");
    BN_RESOLVE(loud_measure, "bnhip_loudness_measure_pcm16"); BN_RESOLVE(loud_normalize, "bnhip_loudness_normalize_pcm16");
    BN_RESOLVE(flac_max_bytes, "bnhip_flac_max_bytes"); BN_RESOLVE(flac_encode_pcm16, "bnhip_flac_encode_pcm16");
    BN_RESOLVE(loud_flac_pcm16, "bnhip_loudness_flac_pcm16");
    BN_RESOLVE(flac_lpc_encode_pcm16, "bnhip_flac_lpc_encode_pcm16"); BN_RESOLVE(loud_flac_lpc_pcm16, "bnhip_loudness_flac_lpc_pcm16");
    BN_RESOLVE(png_max_bytes, "bnhip_png_max_bytes"); BN_RESOLVE(png_encode_u8, "bnhip_png_encode_u8");
    BN_RESOLVE(spec_png_pcm16, "bnhip_spectrogram_png_pcm16");
    BN_RESOLVE(spec_ragged_pcm16, "bnhip_spectrogram_ragged_pcm16"); BN_RESOLVE(spec_png_ragged_pcm16, "bnhip_spectrogram_png_ragged_pcm16");
    return NULL;
}
static void bnbind_unload(void) {
    if (BN.shutdown) BN.shutdown();
    if (BN.handle) dlclose(BN.handle);
    memset(&BN, 0, sizeof BN);
}
static int bnbind_win_predict_topk(bnhip_windows* w, bnhip_model* m, int bits, int act, double sens, int k, int* src, int* n,
                                   float* c, int32_t* i, const void** batch) {
    return BN.win_predict_topk(w, m, bits, act, sens, k, src, n, c, i, batch);
}
// fixed-arity wrappers (cgo cannot call function pointers directly)
static int bnbind_init(int* n) { return BN.init(n); }
static int bnbind_model_create(const void* b, size_t n, const char* o, bnhip_model** m) { return BN.model_create(b, n, o, m); }
static int bnbind_model_info(const bnhip_model* m, int* a, int* b, int* c) { return BN.model_info(m, a, b, c); }
static int bnbind_predict(bnhip_model* m, const float* s, int n, float* l, float* e) { return BN.predict(m, s, n, l, e); }
static int bnbind_predict_topk(bnhip_model* m, const float* s, int n, int act, double sens, int k, float* c, int32_t* i) {
    return BN.predict_topk(m, s, n, act, sens, k, c, i);
}
static void bnbind_model_destroy(bnhip_model* m) { BN.model_destroy(m); }
static const char* bnbind_last_error(void) { return BN.last_error ? BN.last_error() : ""; }
static int bnbind_predict_pcm16(bnhip_model* m, const int16_t* s, int n, float* l, float* e) { return BN.predict_pcm16(m, s, n, l, e); }
static int bnbind_us_frame_cv(int dev, const double* s, int n_clips, int n, int rate, int fft, int hop, int split, double* cv, int32_t* ok) {
    return BN.us_frame_cv(dev, s, n_clips, n, rate, fft, hop, split, cv, ok);
}
static int bnbind_rs_create(int dev, int from, int to, bnhip_resampler** r) { return BN.rs_create(dev, from, to, r); }
static int bnbind_rs_estimate(const bnhip_resampler* r, int n) { return BN.rs_estimate(r, n); }
static int bnbind_rs_process_pcm16(bnhip_resampler* r, const int16_t* in, int n, int16_t* out, int cap, int* n_out) {
    return BN.rs_process_pcm16(r, in, n, out, cap, n_out);
}
static int bnbind_rs_flush_pcm16(bnhip_resampler* r, int16_t* out, int cap, int* n_out) { return BN.rs_flush_pcm16(r, out, cap, n_out); }
static void bnbind_rs_destroy(bnhip_resampler* r) { BN.rs_destroy(r); }
static int bnbind_host_alloc(size_t n, void** p) { return BN.host_alloc(n, p); }
static int bnbind_host_free(void* p) { return BN.host_free ? BN.host_free(p) : 0; }
static int bnbind_win_create(size_t ov, size_t rd, int mb, bnhip_windows** w) { return BN.win_create(ov, rd, mb, w); }
static int bnbind_win_info(const bnhip_windows* w, size_t* wb, int* mb, int* pinned, int* ns) { return BN.win_info(w, wb, mb, pinned, ns); }
static int bnbind_win_add_source(bnhip_windows* w, const char* id, size_t cap, int* out) { return BN.win_add_source(w, id, cap, out); }
static int bnbind_win_remove_source(bnhip_windows* w, int s) { return BN.win_remove_source(w, s); }
static int bnbind_win_write(bnhip_windows* w, int s, const void* d, size_t n) { return BN.win_write(w, s, d, n); }
static int bnbind_win_collect(bnhip_windows* w, int cap, int* src, int* n, const void** batch) { return BN.win_collect(w, cap, src, n, batch); }
static int bnbind_win_stats(const bnhip_windows* w, int s, uint64_t* wr, uint64_t* ov, size_t* buffered) { return BN.win_stats(w, s, wr, ov, buffered); }
static int bnbind_win_reset(bnhip_windows* w, int s) { return BN.win_reset(w, s); }
static void bnbind_win_destroy(bnhip_windows* w) { if (BN.win_destroy) BN.win_destroy(w); }
static int bnbind_predict_pcm_topk(bnhip_model* m, const void* pcm, int bits, int n, int act, double sens, int k, float* c, int32_t* i) {
    return BN.predict_pcm_topk(m, pcm, bits, n, act, sens, k, c, i);
}
// resampler bank (static inline: the C test driver does not call these, and -Wunused-function spares inline ones)
static inline int bnbind_rb_create(int dev, int from, int to, int max_streams, bnhip_resampler_bank** b) {
    return BN.rb_create(dev, from, to, max_streams, b);
}
static inline int bnbind_rb_add_stream(bnhip_resampler_bank* b, int* s) { return BN.rb_add_stream(b, s); }
static inline int bnbind_rb_remove_stream(bnhip_resampler_bank* b, int s) { return BN.rb_remove_stream(b, s); }
static inline int bnbind_rb_estimate(const bnhip_resampler_bank* b, int n) { return BN.rb_estimate(b, n); }
static inline int bnbind_rb_process_pcm16(bnhip_resampler_bank* b, int n, const int* st, const int16_t* const* f, const int* n_in,
                                          int16_t* out, size_t cap, int* cnt) {
    return BN.rb_process_pcm16(b, n, st, f, n_in, out, cap, cnt);
}
static inline int bnbind_rb_flush_pcm16(bnhip_resampler_bank* b, int n, const int* st, int16_t* out, size_t cap, int* cnt) {
    return BN.rb_flush_pcm16(b, n, st, out, cap, cnt);
}
static inline int bnbind_win_write_resampled(bnhip_windows* w, bnhip_resampler_bank* b, int n, const int* st, const int* src,
                                             const int16_t* const* f, const int* n_in) {
    return BN.win_write_resampled(w, b, n, st, src, f, n_in);
}
static inline void bnbind_rb_destroy(bnhip_resampler_bank* b) { if (BN.rb_destroy) BN.rb_destroy(b); }
// equalizer bank (static inline, as the resampler bank's)
static inline int bnbind_eq_create(int dev, int max_streams, bnhip_eq_bank** b) { return BN.eq_create(dev, max_streams, b); }
static inline int bnbind_eq_add_stream(bnhip_eq_bank* b, int* s) { return BN.eq_add_stream(b, s); }
static inline int bnbind_eq_remove_stream(bnhip_eq_bank* b, int s) { return BN.eq_remove_stream(b, s); }
static inline int bnbind_eq_set_chain(bnhip_eq_bank* b, int s, const double* sec, int n, const int* passes, double gain) {
    return BN.eq_set_chain(b, s, sec, n, passes, gain);
}
static inline int bnbind_eq_reset(bnhip_eq_bank* b, int s) { return BN.eq_reset(b, s); }
static inline int bnbind_eq_process_pcm16(bnhip_eq_bank* b, int n, const int* st, const int16_t* const* f, const int* n_in,
                                          int16_t* out, size_t cap, int* cnt) {
    return BN.eq_process_pcm16(b, n, st, f, n_in, out, cap, cnt);
}
static inline int bnbind_win_write_equalized(bnhip_windows* w, bnhip_eq_bank* b, int n, const int* st, const int* src,
                                             const int16_t* const* f, const int* n_in) {
    return BN.win_write_equalized(w, b, n, st, src, f, n_in);
}
static inline void bnbind_eq_destroy(bnhip_eq_bank* b) { if (BN.eq_destroy) BN.eq_destroy(b); }
// sound level bank (static inline, as the other banks')
static inline int bnbind_sl_bands(int rate, double* bands6, int cap, int* n) { return BN.sl_bands(rate, bands6, cap, n); }
static inline int bnbind_sl_create(int dev, int rate, int max_streams, const double* bands6, int n, bnhip_soundlevel_bank** b) {
    return BN.sl_create(dev, rate, max_streams, bands6, n, b);
}
static inline int bnbind_sl_add_stream(bnhip_soundlevel_bank* b, int interval, int* s) { return BN.sl_add_stream(b, interval, s); }
static inline int bnbind_sl_remove_stream(bnhip_soundlevel_bank* b, int s) { return BN.sl_remove_stream(b, s); }
static inline int bnbind_sl_reset(bnhip_soundlevel_bank* b, int s) { return BN.sl_reset(b, s); }
static inline int bnbind_sl_process_pcm16(bnhip_soundlevel_bank* b, int n, const int* st, const int16_t* const* f, const int* n_in,
                                          bnhip_sound_level* reps, int max_reps, int* n_reps) {
    return BN.sl_process_pcm16(b, n, st, f, n_in, reps, max_reps, n_reps);
}
static inline void bnbind_sl_destroy(bnhip_soundlevel_bank* b) { if (BN.sl_destroy) BN.sl_destroy(b); }
static inline int bnbind_range_heatmap(bnhip_model* m, const float* coords, int n_cells, int species, int stride, int total_weeks,
                                       float* result) {
    return BN.range_heatmap(m, coords, n_cells, species, stride, total_weeks, result);
}
static inline int bnbind_spec_size(int width, int* height, int* fft_size) { return BN.spec_size(width, height, fft_size); }
static inline int bnbind_spec_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate_in, int rate_out, int width, int height,
                                    const double* window, double top_db, double range_db, uint8_t* image) {
    return BN.spec_pcm16(device, pcm, n_clips, n, rate_in, rate_out, width, height, window, top_db, range_db, image);
}
static inline int bnbind_loud_measure(int device, const int16_t* pcm, int n_clips, int n, int rate, bnhip_loudness* out, double* sub_energy) {
    return BN.loud_measure(device, pcm, n_clips, n, rate, out, sub_energy);
}
static inline int bnbind_loud_normalize(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs, double true_peak_dbtp,
                                        double max_gain_db, int gate_fallback, int16_t* out_pcm, bnhip_loudness* out) {
    return BN.loud_normalize(device, pcm, n_clips, n, rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, out_pcm, out);
}
static inline int bnbind_png_max_bytes(int n_images, int width, int height, size_t* bytes) { return BN.png_max_bytes(n_images, width, height, bytes); }
static inline int bnbind_png_encode_u8(int device, const uint8_t* images, int n_images, int width, int height, const uint8_t* palette, uint8_t* out,
                                       size_t out_cap, uint64_t* offsets) {
    return BN.png_encode_u8(device, images, n_images, width, height, palette, out, out_cap, offsets);
}
static inline int bnbind_spec_png_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate_in, int rate_out, int width, int height,
                                        const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap,
                                        uint64_t* offsets) {
    return BN.spec_png_pcm16(device, pcm, n_clips, n, rate_in, rate_out, width, height, window, top_db, range_db, palette, out, out_cap, offsets);
}
static inline int bnbind_spec_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out, int width,
                                           int height, const double* window, double top_db, double range_db, uint8_t* image) {
    return BN.spec_ragged_pcm16(device, pcm, n_clips, lens, rate_in, rate_out, width, height, window, top_db, range_db, image);
}
static inline int bnbind_spec_png_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out, int width,
                                               int height, const double* window, double top_db, double range_db, const uint8_t* palette,
                                               uint8_t* out, size_t out_cap, uint64_t* offsets) {
    return BN.spec_png_ragged_pcm16(device, pcm, n_clips, lens, rate_in, rate_out, width, height, window, top_db, range_db, palette, out, out_cap,
                                    offsets);
}
static inline int bnbind_flac_max_bytes(int n_clips, int n, int seek_interval, size_t* bytes) {
    return BN.flac_max_bytes(n_clips, n, seek_interval, bytes);
}
static inline int bnbind_flac_encode_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, const double* factor, int seek_interval,
                                           uint8_t* out, size_t out_cap, uint64_t* offsets) {
    return BN.flac_encode_pcm16(device, pcm, n_clips, n, rate, factor, seek_interval, out, out_cap, offsets);
}
static inline int bnbind_loud_flac_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs, double true_peak_dbtp,
                                         double max_gain_db, int gate_fallback, int seek_interval, bnhip_loudness* out, uint8_t* out_bytes,
                                         size_t out_cap, uint64_t* offsets) {
    return BN.loud_flac_pcm16(device, pcm, n_clips, n, rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, seek_interval, out,
                              out_bytes, out_cap, offsets);
}
static inline int bnbind_flac_lpc_encode_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, const double* factor,
                                               int seek_interval, uint8_t* out, size_t out_cap, uint64_t* offsets, int lpc_order) {
    return BN.flac_lpc_encode_pcm16(device, pcm, n_clips, n, rate, factor, seek_interval, out, out_cap, offsets, lpc_order);
}
static inline int bnbind_loud_flac_lpc_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs,
                                             double true_peak_dbtp, double max_gain_db, int gate_fallback, int seek_interval, bnhip_loudness* out,
                                             uint8_t* out_bytes, size_t out_cap, uint64_t* offsets, int lpc_order) {
    return BN.loud_flac_lpc_pcm16(device, pcm, n_clips, n, rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, seek_interval, out,
                                  out_bytes, out_cap, offsets, lpc_order);
}
// frames handed to the bank are staged in C memory (cgo: C may not keep or receive Go pointers inside Go memory): slot k of
// the pointer table points at byte offset off[k] of the staging block
static inline void bnbind_rb_point(const int16_t** ptrs, const char* stage, const int* off, int n) {
    for (int k = 0; k < n; k++) ptrs[k] = (const int16_t*)(const void*)(stage + off[k]);
}
*/
import "C"

import (
	"errors"
	"fmt"
	"math"
	"runtime"
	"strings"
	"sync"
	"unsafe"
)

// Supported reports whether the HIP backend is compiled in (mirrors openvino.Supported).
const Supported = true

// ErrHIPUnavailable: library missing or no gfx950 device. Callers treat it as "fall back".
var ErrHIPUnavailable = errors.New("hip: backend unavailable")

var (
	initMu   sync.Mutex
	initDone bool
)

// lastError must run on the OS thread that made the failing call (the text is thread-local in the
// library); every caller below holds runtime.LockOSThread across call + fetch.
func lastError() string { return C.GoString(C.bnbind_last_error()) }

// Init loads libbnhip.so and initialises the HIP runtime. Idempotent and retryable.
func Init(libraryPath string) error {
	initMu.Lock()
	defer initMu.Unlock()
	if initDone {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	cpath := C.CString(libraryPath)
	defer C.free(unsafe.Pointer(cpath))
	if msg := C.bnbind_load(cpath); msg != nil {
		return fmt.Errorf("%w: %s", ErrHIPUnavailable, C.GoString(msg))
	}
	var n C.int
	if rc := C.bnbind_init(&n); rc != 0 {
		err := fmt.Errorf("%w: %s", ErrHIPUnavailable, lastError())
		C.bnbind_unload() // retryable: the next Init reloads
		return err
	}
	initDone = true
	return nil
}

// Classifier implements inference.Classifier and inference.EmbeddingExtractor.
// NOT goroutine-safe (backend.go:7); BirdNET.mu serialises the whole native call.
type Classifier struct {
	h        *C.bnhip_model
	nSamples int
	nClasses int
	embDim   int
	// C-side staging, as the OpenVINO shim keeps it (backend_openvino.go:673-680): the Go slice returns to a pool right after
	// Predict (process.go:280-291) and the GC may move Go memory.  Both buffers are PAGE-LOCKED (bnhip_host_alloc), so the
	// library DMAs one clip in and the logits out without its own staging copy.
	in  *C.float // [nSamples]
	out *C.float // [nClasses + embDim]
}

// NewClassifier builds a classifier from the same in-memory model bytes the TFLite backend takes
// (tflite.NewTFLiteClassifier(modelData []byte, ...), internal/inference/tflite/classifier.go:38).
// devices: one ordinal = one GPU; several = one handle sharding every batch over them.
func NewClassifier(modelData []byte, devices ...int) (*Classifier, error) {
	return NewClassifierWithOptions(modelData, Options{Devices: devices})
}

// Options are the creation options of include/bnhip.h a host may want to set; zero values keep the library defaults.
type Options struct {
	Devices  []int // GPU ordinals (default: device 0)
	MaxBatch int   // largest PredictBatch the handle accepts (default 256)
	// Precision "bf16" rounds the MFMA operands to bf16 (fp32 accumulation): only for models that tolerate it
	// (Perch v2; never BirdNET v2.4, internal/classifier/model_openvino.go:99-103). Default "f32".
	Precision string
	// LogitsOutput / EmbeddingOutput name graph outputs explicitly (1-based here so that the zero value means "the
	// reference's per-family rule", internal/inference/onnx/detection.go:52-112).
	LogitsOutput, EmbeddingOutput int
	// StrictF32 keeps every contraction on the f32-input MFMA ("bf16x3":0) instead of letting compute-bound layers run as
	// six exact bf16 products per fp32 product (fp32-equivalent to 2^-23, include/bnhip.h): for hosts that want one kernel family.
	StrictF32 bool
	// TuneDir is a directory of recorded create-time tunings (include/bnhip.h "tune_dir": files <plan key>.tune as shipped under
	// birdnet-go_amd/tune/): an engine whose plan matches a file adopts it instead of timing its kernel candidates, which makes
	// the plan - and a clip's last bits - reproducible from process to process. Empty: the BNHIP_TUNE_DIR environment, else none.
	TuneDir string
}

// NewClassifierWithOptions is NewClassifier with explicit creation options (e.g. Perch v2 on bf16 operands).
func NewClassifierWithOptions(modelData []byte, o Options) (*Classifier, error) {
	if len(modelData) == 0 {
		return nil, errors.New("hip: empty model data")
	}
	devices := o.Devices
	if len(devices) == 0 {
		devices = []int{0}
	}
	list := ""
	for i, d := range devices {
		if i > 0 {
			list += ","
		}
		list += fmt.Sprint(d)
	}
	maxBatch := o.MaxBatch
	if maxBatch <= 0 {
		maxBatch = 256
	}
	js := fmt.Sprintf(`{"devices":[%s],"max_batch":%d`, list, maxBatch)
	if o.Precision == "bf16" || o.Precision == "f32" {
		js += fmt.Sprintf(`,"precision":"%s"`, o.Precision)
	} else if o.Precision != "" {
		return nil, fmt.Errorf("hip: unknown precision %q", o.Precision)
	}
	if o.StrictF32 {
		js += `,"bf16x3":0`
	}
	if o.LogitsOutput > 0 {
		js += fmt.Sprintf(`,"logits_output":%d`, o.LogitsOutput-1)
	}
	if o.EmbeddingOutput > 0 {
		js += fmt.Sprintf(`,"embedding_output":%d`, o.EmbeddingOutput-1)
	}
	if o.TuneDir != "" {
		if strings.ContainsAny(o.TuneDir, "\"\\") {
			return nil, fmt.Errorf("hip: tune directory %q cannot be passed (quote or backslash in the path)", o.TuneDir)
		}
		js += fmt.Sprintf(`,"tune_dir":"%s"`, o.TuneDir)
	}
	opts := C.CString(js + "}")
	defer C.free(unsafe.Pointer(opts))
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var h *C.bnhip_model
	if rc := C.bnbind_model_create(unsafe.Pointer(&modelData[0]), C.size_t(len(modelData)), opts, &h); rc != 0 {
		msg := lastError()
		if rc == -2 {
			return nil, fmt.Errorf("%w: %s", ErrHIPUnavailable, msg)
		}
		return nil, fmt.Errorf("hip: model create failed (%d): %s", int(rc), msg)
	}
	var ns, nc, ed C.int
	C.bnbind_model_info(h, &ns, &nc, &ed)
	c := &Classifier{h: h, nSamples: int(ns), nClasses: int(nc), embDim: int(ed)}
	var pin, pout unsafe.Pointer
	if rc := C.bnbind_host_alloc(C.size_t(c.nSamples)*4, &pin); rc != 0 {
		msg := lastError()
		C.bnbind_model_destroy(h)
		return nil, fmt.Errorf("hip: pinned input allocation failed (%d): %s", int(rc), msg)
	}
	if rc := C.bnbind_host_alloc(C.size_t(c.nClasses+c.embDim)*4, &pout); rc != 0 {
		msg := lastError()
		C.bnbind_host_free(pin)
		C.bnbind_model_destroy(h)
		return nil, fmt.Errorf("hip: pinned output allocation failed (%d): %s", int(rc), msg)
	}
	c.in, c.out = (*C.float)(pin), (*C.float)(pout)
	return c, nil
}

// Predict returns raw logits, one per label, in a freshly allocated slice the caller owns.
func (c *Classifier) Predict(samples []float32) ([]float32, error) {
	logits, _, err := c.predict(samples, false)
	return logits, err
}

// PredictWithEmbeddings implements inference.EmbeddingExtractor.
func (c *Classifier) PredictWithEmbeddings(samples []float32) (logits, embeddings []float32, err error) {
	return c.predict(samples, c.embDim > 0)
}

func (c *Classifier) predict(samples []float32, wantEmb bool) ([]float32, []float32, error) {
	if c.h == nil {
		return nil, nil, errors.New("hip: classifier is closed")
	}
	if len(samples) != c.nSamples {
		return nil, nil, fmt.Errorf("input size mismatch: expected %d samples, got %d", c.nSamples, len(samples))
	}
	C.memcpy(unsafe.Pointer(c.in), unsafe.Pointer(&samples[0]), C.size_t(c.nSamples)*4)
	var ep *C.float
	if wantEmb {
		ep = (*C.float)(unsafe.Add(unsafe.Pointer(c.out), c.nClasses*4))
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_predict(c.h, c.in, 1, c.out, ep); rc != 0 {
		return nil, nil, fmt.Errorf("hip: predict failed (%d): %s", int(rc), lastError())
	}
	// a freshly allocated slice the caller owns (tflite/classifier.go:115-116)
	logits := make([]float32, c.nClasses)
	copy(logits, unsafe.Slice((*float32)(unsafe.Pointer(c.out)), c.nClasses))
	var emb []float32
	if wantEmb {
		emb = make([]float32, c.embDim)
		copy(emb, unsafe.Slice((*float32)(unsafe.Pointer(ep)), c.embDim))
	}
	return logits, emb, nil
}

// PredictBatch mirrors onnx.Classifier.PredictBatch (internal/inference/onnx/classifier.go:372-430):
// flat [batchSize*nSamples] in, flat [batchSize*nClasses] out.
func (c *Classifier) PredictBatch(flat []float32, batchSize int) ([]float32, error) {
	if c.h == nil {
		return nil, errors.New("hip: classifier is closed")
	}
	if batchSize <= 0 || len(flat) != batchSize*c.nSamples {
		return nil, fmt.Errorf("input size mismatch: expected %d samples, got %d", batchSize*c.nSamples, len(flat))
	}
	out := make([]float32, batchSize*c.nClasses)
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_predict(c.h, (*C.float)(unsafe.Pointer(&flat[0])), C.int(batchSize),
		(*C.float)(unsafe.Pointer(&out[0])), nil); rc != 0 {
		return nil, fmt.Errorf("hip: predict failed (%d): %s", int(rc), lastError())
	}
	return out, nil
}

// PredictTopK runs predict + sigmoid(sensitivity) + top-k on the device ((*BirdNET).Predict's
// post-processing, classifier/analyze.go:113-115,197-253): confidences and label indices, descending.
func (c *Classifier) PredictTopK(flat []float32, batchSize, k int, sensitivity float64) ([]float32, []int32, error) {
	return c.predictTopK(flat, batchSize, k, 0, sensitivity)
}

// PredictTopKSoftmax is the Perch v2 form: softmax over the logits (perchSoftmax, classifier/perch_onnx.go:315-335:
// max-subtract, exp in float64, float32 running sum) + top-k on the device.
func (c *Classifier) PredictTopKSoftmax(flat []float32, batchSize, k int) ([]float32, []int32, error) {
	return c.predictTopK(flat, batchSize, k, 1, 1.0)
}

func (c *Classifier) predictTopK(flat []float32, batchSize, k, activation int, sensitivity float64) ([]float32, []int32, error) {
	if c.h == nil {
		return nil, nil, errors.New("hip: classifier is closed")
	}
	if batchSize <= 0 || k <= 0 || len(flat) != batchSize*c.nSamples {
		return nil, nil, fmt.Errorf("input size mismatch: expected %d samples, got %d", batchSize*c.nSamples, len(flat))
	}
	if k > c.nClasses {
		k = c.nClasses
	}
	conf := make([]float32, batchSize*k)
	idx := make([]int32, batchSize*k)
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_predict_topk(c.h, (*C.float)(unsafe.Pointer(&flat[0])), C.int(batchSize), C.int(activation), C.double(sensitivity),
		C.int(k), (*C.float)(unsafe.Pointer(&conf[0])), (*C.int32_t)(unsafe.Pointer(&idx[0]))); rc != 0 {
		return nil, nil, fmt.Errorf("hip: predict_topk failed (%d): %s", int(rc), lastError())
	}
	return conf, idx, nil
}

// NumSpecies comes from the model output, not the label list (inference/openvino.go:72-81).
func (c *Classifier) NumSpecies() int { return c.nClasses }

// Close is idempotent and frees device memory now (BirdNET.Delete, classifier/birdnet.go:972-984).
func (c *Classifier) Close() {
	if c.h != nil {
		C.bnbind_model_destroy(c.h)
		c.h = nil
	}
	if c.in != nil {
		C.bnbind_host_free(unsafe.Pointer(c.in))
		c.in = nil
	}
	if c.out != nil {
		C.bnbind_host_free(unsafe.Pointer(c.out))
		c.out = nil
	}
}

// PinnedF32 is a float32 slice over page-locked memory (bnhip_host_alloc) for batch callers: fill Data, pass it to PredictBatch /
// PredictTopK - the library recognises pinned memory per call and lets the copy engines read it directly instead of staging it.
// The memory is C-owned: Free it, do not let the slice (or a sub-slice of it) outlive Free, and do not Free it while a Predict
// call that was handed the slice is still running - nothing on the Go side tracks either.
type PinnedF32 struct {
	Data []float32
	p    unsafe.Pointer
}

// AllocPinnedF32 returns n page-locked floats (Init must have succeeded).
func AllocPinnedF32(n int) (*PinnedF32, error) {
	if n <= 0 {
		return nil, errors.New("hip: pinned allocation of zero elements")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var p unsafe.Pointer
	if rc := C.bnbind_host_alloc(C.size_t(n)*4, &p); rc != 0 {
		return nil, fmt.Errorf("hip: pinned allocation failed (%d): %s", int(rc), lastError())
	}
	return &PinnedF32{Data: unsafe.Slice((*float32)(p), n), p: p}, nil
}

// Free releases the buffer; idempotent.
func (b *PinnedF32) Free() {
	if b.p != nil {
		C.bnbind_host_free(b.p)
		b.p, b.Data = nil, nil
	}
}

// PredictPCM16 is Predict for a clip that is still 16-bit little-endian PCM: the conversion float32(s)/32768
// (internal/analysis/process.go:479-497, internal/audiocore/convert/pcm.go:226-237) runs on the device and half the bytes
// cross PCIe.  pcm holds batchSize clips of nSamples samples (2 bytes each); returns flat [batchSize*nClasses] logits.
func (c *Classifier) PredictPCM16(pcm []byte, batchSize int) ([]float32, error) {
	if c.h == nil {
		return nil, errors.New("hip: classifier is closed")
	}
	if batchSize <= 0 || len(pcm) != batchSize*c.nSamples*2 {
		return nil, fmt.Errorf("input size mismatch: expected %d bytes, got %d", batchSize*c.nSamples*2, len(pcm))
	}
	out := make([]float32, batchSize*c.nClasses)
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_predict_pcm16(c.h, (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(batchSize),
		(*C.float)(unsafe.Pointer(&out[0])), nil); rc != 0 {
		return nil, fmt.Errorf("hip: predict_pcm16 failed (%d): %s", int(rc), lastError())
	}
	return out, nil
}

// WindowAssembler holds the analysis buffers of every audio source of ONE model in the library (bnhip_windows): per source the
// ring in overwrite mode and the overlap tail of buffer.AnalysisBuffer (internal/audiocore/buffer/analysis.go:30-276), per tick
// the Read() of all of that model's poll loops (internal/analysis/buffer_manager.go:388-496) in one pass - every source with a
// window ready lands in a row of one page-locked batch buffer, which PredictWindows hands to the device as it is.  Where the
// reference queues one batch-1 Predict per window behind Orchestrator.inferenceMu (internal/classifier/orchestrator.go:531),
// a tick is one device call.  Write may be called from any capture goroutine; Collect / PredictWindows from one at a time.
//
// Lifetimes: every `windows` slice handed out below is a VIEW of the library's batch buffer (C memory): the next tick
// overwrites it and Close frees it.  Copy what must outlive the tick (the reference copies the PCM into its Results message
// too, process.go:364-372).  Close waits for a tick or a Write in flight (life) and ticks exclude each other (tick), so a
// Close racing a poll loop can neither free the buffer under a device call nor hand the C side a dead handle.
type WindowAssembler struct {
	h           *C.bnhip_windows
	windowBytes int
	maxBatch    int
	pinned      bool
	sources     []C.int      // scratch of Collect
	tick        sync.Mutex   // one Collect / PredictWindows* at a time
	life        sync.RWMutex // readers: every call that uses h; writer: Close
}

// NewWindowAssembler: overlapBytes + readBytes = the model's clip in bytes (ModelSpec.BufferDimensions, model.go:33-56).
func NewWindowAssembler(overlapBytes, readBytes, maxBatch int) (*WindowAssembler, error) {
	if overlapBytes < 0 || readBytes <= 0 || maxBatch <= 0 {
		return nil, fmt.Errorf("hip: invalid window geometry: overlap %d, read %d, max batch %d", overlapBytes, readBytes, maxBatch)
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var h *C.bnhip_windows
	if rc := C.bnbind_win_create(C.size_t(overlapBytes), C.size_t(readBytes), C.int(maxBatch), &h); rc != 0 {
		return nil, fmt.Errorf("hip: windows_create failed (%d): %s", int(rc), lastError())
	}
	var wb C.size_t
	var mb, pin C.int
	C.bnbind_win_info(h, &wb, &mb, &pin, nil)
	return &WindowAssembler{h: h, windowBytes: int(wb), maxBatch: int(mb), pinned: pin != 0, sources: make([]C.int, int(mb))}, nil
}

// AddSource = NewAnalysisBuffer(capacity, overlap, read, sourceID) for one more source; the index names it from then on.
func (w *WindowAssembler) AddSource(sourceID string, capacity int) (int, error) {
	w.life.RLock()
	defer w.life.RUnlock()
	if w.h == nil {
		return -1, errors.New("hip: window assembler is closed")
	}
	id := C.CString(sourceID)
	defer C.free(unsafe.Pointer(id))
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var idx C.int
	if capacity < 0 {
		capacity = 0
	}
	if rc := C.bnbind_win_add_source(w.h, id, C.size_t(capacity), &idx); rc != 0 {
		return -1, fmt.Errorf("hip: windows_add_source failed (%d): %s", int(rc), lastError())
	}
	return int(idx), nil
}

func (w *WindowAssembler) RemoveSource(source int) error {
	w.life.RLock()
	defer w.life.RUnlock()
	if w.h == nil {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_win_remove_source(w.h, C.int(source)); rc != 0 {
		return fmt.Errorf("hip: windows_remove_source failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// Write = AnalysisBuffer.Write (analysis.go:152-175): never blocks on the consumer, the oldest unread bytes go when the ring
// is full.  The bytes are copied before it returns.
func (w *WindowAssembler) Write(source int, data []byte) error {
	w.life.RLock()
	defer w.life.RUnlock()
	if w.h == nil {
		return errors.New("hip: window assembler is closed")
	}
	if len(data) == 0 {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_win_write(w.h, C.int(source), unsafe.Pointer(&data[0]), C.size_t(len(data))); rc != 0 {
		return fmt.Errorf("hip: windows_write failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// Collect reads every source that has a window ready (at most maxBatch; the next call resumes behind the last source looked
// at).  windows is a view of the library's batch buffer - row k belongs to sources[k] - valid until the next Collect.
func (w *WindowAssembler) Collect() (sources []int, windows []byte, err error) {
	w.tick.Lock()
	defer w.tick.Unlock()
	w.life.RLock()
	defer w.life.RUnlock()
	return w.collectLocked()
}

// collectLocked: the caller holds tick and life.
func (w *WindowAssembler) collectLocked() (sources []int, windows []byte, err error) {
	if w.h == nil {
		return nil, nil, errors.New("hip: window assembler is closed")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var n C.int
	var batch unsafe.Pointer
	if rc := C.bnbind_win_collect(w.h, C.int(w.maxBatch), &w.sources[0], &n, &batch); rc != 0 {
		return nil, nil, fmt.Errorf("hip: windows_collect failed (%d): %s", int(rc), lastError())
	}
	if n == 0 {
		return nil, nil, nil
	}
	sources = make([]int, int(n))
	for i := range sources {
		sources[i] = int(w.sources[i])
	}
	return sources, unsafe.Slice((*byte)(batch), int(n)*w.windowBytes), nil
}

// OverwriteStats: the OverwriteTracker's inputs for one source (buffer/overwrite.go) - writes and overwriting writes since
// creation or Reset.  The rate window and the notification policy stay with the caller.
func (w *WindowAssembler) OverwriteStats(source int) (writes, overwrites uint64, err error) {
	w.life.RLock()
	defer w.life.RUnlock()
	if w.h == nil {
		return 0, 0, errors.New("hip: window assembler is closed")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var wr, ov C.uint64_t
	if rc := C.bnbind_win_stats(w.h, C.int(source), &wr, &ov, nil); rc != 0 {
		return 0, 0, fmt.Errorf("hip: windows_stats failed (%d): %s", int(rc), lastError())
	}
	return uint64(wr), uint64(ov), nil
}

// Reset = AnalysisBuffer.Reset (analysis.go:270-276) for one source.
func (w *WindowAssembler) Reset(source int) error {
	w.life.RLock()
	defer w.life.RUnlock()
	if w.h == nil {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_win_reset(w.h, C.int(source)); rc != 0 {
		return fmt.Errorf("hip: windows_reset failed (%d): %s", int(rc), lastError())
	}
	return nil
}

func (w *WindowAssembler) WindowBytes() int { return w.windowBytes }
func (w *WindowAssembler) Pinned() bool     { return w.pinned }

// Close frees the rings and the batch buffer; every slice a tick handed out dangles from here on.  Waits for calls in flight.
func (w *WindowAssembler) Close() {
	w.tick.Lock()
	defer w.tick.Unlock()
	w.life.Lock()
	defer w.life.Unlock()
	if w.h != nil {
		C.bnbind_win_destroy(w.h)
		w.h = nil
	}
}

// PredictWindows is one tick of the real-time path for this classifier's model: Collect, then one device call over all ready
// windows straight from the assembler's batch buffer (16-bit capture, conf.BytesPerSample; the /32768 conversion of
// process.go:479-497 runs on the device).  Returns the source of each row and flat [len(sources)*nClasses] logits; nothing
// ready = (nil, nil, nil), the reference's "try again later".  The caller builds one Results message per row, as ProcessData
// does per window (process.go:327-420); windows is the PCM it must copy into the message before the next tick (a view of C
// memory: the next tick overwrites it, Close frees it).  On a failed device call sources still lists who gave up a window.
func (c *Classifier) PredictWindows(w *WindowAssembler) (sources []int, windows []byte, logits []float32, err error) {
	if c.h == nil {
		return nil, nil, nil, errors.New("hip: classifier is closed")
	}
	if w.windowBytes != c.nSamples*2 {
		return nil, nil, nil, fmt.Errorf("window size mismatch: assembler %d bytes, model clip %d bytes", w.windowBytes, c.nSamples*2)
	}
	w.tick.Lock()
	defer w.tick.Unlock()
	w.life.RLock()
	defer w.life.RUnlock()
	sources, windows, err = w.collectLocked()
	if err != nil || len(sources) == 0 {
		return nil, nil, nil, err
	}
	logits = make([]float32, len(sources)*c.nClasses)
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_predict_pcm16(c.h, (*C.int16_t)(unsafe.Pointer(&windows[0])), C.int(len(sources)),
		(*C.float)(unsafe.Pointer(&logits[0])), nil); rc != 0 {
		// the listed sources have given up their window all the same (their overlap tails advanced): the caller gets the list
		// with the error, as the reference's monitor has consumed its window before ProcessData fails (buffer_manager.go:494-499)
		return sources, nil, nil, fmt.Errorf("hip: predict_pcm16 failed (%d): %s", int(rc), lastError())
	}
	return sources, windows, logits, nil
}

// PredictWindowsTopK is PredictWindows with (*BirdNET).Predict's post-processing on the device as well: per ready window the
// k best confidences float32(1/(1+exp(-sensitivity*float64(x)))) and their label indices, descending (analyze.go:113-115,
// 197-208, 220-301) - the logits never reach the host.  conf / idx are flat [len(sources)*min(k, nClasses)].  On a failed device
// call sources still lists who gave up a window (everything else nil); windows is a view valid until the next tick or Close.
func (c *Classifier) PredictWindowsTopK(w *WindowAssembler, k int, sensitivity float64) (sources []int, windows []byte, conf []float32, idx []int32, err error) {
	if c.h == nil {
		return nil, nil, nil, nil, errors.New("hip: classifier is closed")
	}
	if k <= 0 {
		return nil, nil, nil, nil, errors.New("hip: k must be positive")
	}
	w.tick.Lock()
	defer w.tick.Unlock()
	w.life.RLock()
	defer w.life.RUnlock()
	if w.h == nil {
		return nil, nil, nil, nil, errors.New("hip: window assembler is closed")
	}
	kk := k
	if kk > c.nClasses {
		kk = c.nClasses
	}
	// one call: readiness pass, then the rows of chunk i+1 are assembled while chunk i is on the device
	cbuf := make([]float32, w.maxBatch*kk)
	ibuf := make([]int32, w.maxBatch*kk)
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var n C.int
	var batch unsafe.Pointer
	if rc := C.bnbind_win_predict_topk(w.h, c.h, 16, 0, C.double(sensitivity), C.int(k), &w.sources[0], &n,
		(*C.float)(unsafe.Pointer(&cbuf[0])), (*C.int32_t)(unsafe.Pointer(&ibuf[0])), &batch); rc != 0 {
		// the n listed sources have given up their window all the same (buffer_manager.go:494-499; the C call reports them
		// on failure too): the caller gets the list with the error and knows which sources lost a window
		err = fmt.Errorf("hip: windows_predict_topk failed (%d): %s", int(rc), lastError())
		if n > 0 {
			sources = make([]int, int(n))
			for i := range sources {
				sources[i] = int(w.sources[i])
			}
		}
		return sources, nil, nil, nil, err
	}
	if n == 0 {
		return nil, nil, nil, nil, nil
	}
	sources = make([]int, int(n))
	for i := range sources {
		sources[i] = int(w.sources[i]) // -1: the source was reset under the tick, skip the row
	}
	return sources, unsafe.Slice((*byte)(batch), int(n)*w.windowBytes), cbuf[:int(n)*kk], ibuf[:int(n)*kk], nil
}

// CustomClassifier implements inference.CustomClassifier (internal/inference/backend.go:31-53) for a dense head file - the
// BattyBirdNET regional heads the reference loads next to the shared embeddings backbone (internal/classifier/bat_onnx.go:282).
// PredictEmbedding returns sigmoid-applied scores with the reference's arithmetic: 1/(1+float32(exp(float64(-x)))), the
// division in float32 (internal/inference/onnx/postprocess.go:8-10, custom_classifier.go:148-174).
type CustomClassifier struct {
	c      *Classifier
	labels []string
}

// NewCustomClassifier loads the head (ONNX or TFLite bytes) and checks the label count against the model's class count
// (the reference builder does the same, custom_classifier.go:74-136).
func NewCustomClassifier(modelData []byte, labels []string, devices ...int) (*CustomClassifier, error) {
	c, err := NewClassifierWithOptions(modelData, Options{Devices: devices, MaxBatch: 64})
	if err != nil {
		return nil, err
	}
	if len(labels) != c.nClasses {
		c.Close()
		return nil, fmt.Errorf("hip: label count %d does not match the model's %d classes", len(labels), c.nClasses)
	}
	return &CustomClassifier{c: c, labels: append([]string(nil), labels...)}, nil
}

// PredictEmbedding implements inference.CustomClassifier.
func (cc *CustomClassifier) PredictEmbedding(embeddings []float32) ([]float32, error) {
	if cc.c == nil {
		return nil, errors.New("hip: classifier is closed")
	}
	if len(embeddings) != cc.c.nSamples {
		return nil, fmt.Errorf("embedding size mismatch: expected %d, got %d", cc.c.nSamples, len(embeddings))
	}
	logits, err := cc.c.Predict(embeddings)
	if err != nil {
		return nil, err
	}
	for i, x := range logits {
		logits[i] = 1.0 / (1.0 + float32(math.Exp(float64(-x))))
	}
	return logits, nil
}

// NumClasses, InputDim, Labels, Close implement the rest of inference.CustomClassifier.
func (cc *CustomClassifier) NumClasses() int { return cc.c.nClasses }
func (cc *CustomClassifier) InputDim() int   { return cc.c.nSamples }
func (cc *CustomClassifier) Labels() []string { return cc.labels }
func (cc *CustomClassifier) Close() {
	if cc.c != nil {
		cc.c.Close()
		cc.c = nil
	}
}

// RangeFilter implements inference.RangeFilter and inference.BatchRangeFilter (internal/inference/backend.go:55-76) for
// the [lat, lon, week] -> per-species occurrence meta-model: the one inference the product already batches (heat-map grids,
// internal/classifier/heatmap_service.go:17-36; internal/inference/onnx/rangefilter.go:106-153).  Scores are whatever the
// graph produces (the reference's models end in an in-graph sigmoid).
type RangeFilter struct{ c *Classifier }

// NewRangeFilter loads the meta-model bytes (TFLite - fp16 constants behind DEQUANTIZE are widened at load - or ONNX).
func NewRangeFilter(modelData []byte, devices ...int) (*RangeFilter, error) {
	c, err := NewClassifierWithOptions(modelData, Options{Devices: devices, MaxBatch: 4096})
	if err != nil {
		return nil, err
	}
	if c.nSamples != 3 {
		c.Close()
		return nil, fmt.Errorf("hip: range filter expects 3 inputs (lat, lon, week), the model takes %d", c.nSamples)
	}
	return &RangeFilter{c: c}, nil
}

// Predict implements inference.RangeFilter.
func (r *RangeFilter) Predict(latitude, longitude, week float32) ([]float32, error) {
	return r.PredictBatch([]float32{latitude, longitude, week}, 1)
}

// PredictBatch implements inference.BatchRangeFilter: len(inputs) must equal batchSize * 3; row-major [batchSize*numSpecies] out.
func (r *RangeFilter) PredictBatch(inputs []float32, batchSize int) ([]float32, error) {
	if r.c == nil {
		return nil, errors.New("hip: range filter is closed")
	}
	if batchSize <= 0 || len(inputs) != batchSize*3 {
		return nil, fmt.Errorf("input size mismatch: expected %d values, got %d", batchSize*3, len(inputs))
	}
	return r.c.PredictBatch(inputs, batchSize)
}

// ComputeGrid is HeatmapInferenceService.ComputeGridWithBinding (internal/classifier/heatmap_service.go:143-420) on the device:
// coords holds totalCells [lat, lon] pairs; result[wi*totalCells+c] receives output speciesIdx for [lat_c, lon_c, 1+wi*stride],
// wi < ceil(totalWeeks/stride).  One native call: the rows run in chunks of the handle's max batch on the GPU and only the one
// species' column comes back.  The label -> index lookup stays with the caller (GeomodelSpeciesInfo).  A range filter
// created over several devices refuses the call (a grid runs on one device).
func (r *RangeFilter) ComputeGrid(coords []float32, totalCells, speciesIdx, stride, totalWeeks int, result []float32) error {
	if r.c == nil {
		return errors.New("hip: range filter is closed")
	}
	if totalCells <= 0 || len(coords) != totalCells*2 {
		return fmt.Errorf("hip: coords length %d does not match totalCells %d * 2", len(coords), totalCells)
	}
	if stride <= 0 || totalWeeks <= 0 {
		return errors.New("hip: stride and totalWeeks must be > 0")
	}
	weeks := (totalWeeks + stride - 1) / stride
	if weeks*totalCells > math.MaxInt32 {
		return fmt.Errorf("hip: %d weeks x %d cells exceeds one call", weeks, totalCells)
	}
	if len(result) < weeks*totalCells {
		return fmt.Errorf("hip: result length %d < expected %d", len(result), weeks*totalCells)
	}
	if speciesIdx < 0 || speciesIdx >= r.c.nClasses {
		return fmt.Errorf("hip: species index %d out of range [0, %d)", speciesIdx, r.c.nClasses)
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_range_heatmap(r.c.h, (*C.float)(unsafe.Pointer(&coords[0])), C.int(totalCells), C.int(speciesIdx),
		C.int(stride), C.int(totalWeeks), (*C.float)(unsafe.Pointer(&result[0]))); rc < 0 {
		return fmt.Errorf("hip: range_heatmap failed (%d): %s", int(rc), lastError())
	}
	return nil
}

func (r *RangeFilter) NumSpecies() int { return r.c.nClasses }
func (r *RangeFilter) Close() {
	if r.c != nil {
		r.c.Close()
		r.c = nil
	}
}

// USFilterConfig carries the three geometry fields of conf.UltrasonicFilterConfig that ComputeUSFrameCV reads
// (internal/conf/config.go:1389-1395).
type USFilterConfig struct {
	FFTSize, HopSize, FrequencySplitHz int
}

// ComputeUSFrameCV is internal/audiocore/ultrasonic/filter.go:20-66 on the GPU: frame-to-frame coefficient of variation of
// the ultrasonic band power of one chunk (samples = int16/32768 as float64, convert/pcm.go:108-113); (0, false) when the
// filter's guards reject the geometry - decided before any device work, exactly as the Go code does.  Call site:
// internal/analysis/processor/processor.go:893-935.
func ComputeUSFrameCV(samples []float64, sampleRate int, cfg USFilterConfig, device int) (float64, bool, error) {
	if len(samples) == 0 {
		return 0, false, nil
	}
	var cv C.double
	var ok C.int32_t
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_us_frame_cv(C.int(device), (*C.double)(unsafe.Pointer(&samples[0])), 1, C.int(len(samples)), C.int(sampleRate),
		C.int(cfg.FFTSize), C.int(cfg.HopSize), C.int(cfg.FrequencySplitHz), &cv, &ok); rc != 0 {
		return 0, false, fmt.Errorf("hip: us_frame_cv failed (%d): %s", int(rc), lastError())
	}
	return float64(cv), ok != 0, nil
}

// SpectrogramOptions are the knobs of one render: the profile's target rate (24 000 bird / 256 000 bat, frequency_profile.go:13-16;
// 0 keeps the source rate), a window table of 2 * (height - 1) coefficients (nil = periodic Hann; the "scientific" styles pass a
// Dolph table), and the level scale (RangeDB 80 / 100 / 120, conf/config.go:262-264; 0 means 100).
type SpectrogramOptions struct {
	ResampleRate int
	Window       []float64
	TopDB        float64
	RangeDB      float64
}

// Spectrogram is the device's answer to one GenerateFromPCM (internal/spectrogram/generator.go:425): the raw image (sox's -r:
// no axes, no legend) of one mono PCM16 clip as level indices [height][width], Nyquist in row 0.  The host maps the indices
// through its style's palette (RenderSpectrogramPNGs returns the finished files instead).  Pixel values follow this engine's own rendering spec; they are not pinned
// against sox.
func Spectrogram(pcm []int16, sampleRate, width int, opts SpectrogramOptions, device int) (img []uint8, height int, err error) {
	return RenderSpectrograms(pcm, 1, sampleRate, width, opts, device)
}

// RenderSpectrograms renders nClips clips of one length (pcm = the clips back to back) in ONE device call: a burst of detections
// costs one H2D copy, the kernels and one D2H copy instead of a sox child per image.  img is [nClips][height][width].
func RenderSpectrograms(pcm []int16, nClips, sampleRate, width int, opts SpectrogramOptions, device int) (img []uint8, height int, err error) {
	if nClips <= 0 || len(pcm) == 0 || len(pcm)%nClips != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram needs nClips > 0 clips of one length, got %d samples for %d clips", len(pcm), nClips)
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var h, fft C.int
	if rc := C.bnbind_spec_size(C.int(width), &h, &fft); rc != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram_size failed (%d): %s", int(rc), lastError())
	}
	var win *C.double
	if opts.Window != nil {
		if len(opts.Window) != int(fft) {
			return nil, 0, fmt.Errorf("hip: spectrogram window must hold %d coefficients, got %d", int(fft), len(opts.Window))
		}
		win = (*C.double)(unsafe.Pointer(&opts.Window[0]))
	}
	rangeDB := opts.RangeDB
	if rangeDB == 0 {
		rangeDB = 100
	}
	img = make([]uint8, nClips*int(h)*width)
	if rc := C.bnbind_spec_pcm16(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(nClips), C.int(len(pcm)/nClips),
		C.int(sampleRate), C.int(opts.ResampleRate), C.int(width), h, win, C.double(opts.TopDB), C.double(rangeDB),
		(*C.uint8_t)(unsafe.Pointer(&img[0]))); rc != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram failed (%d): %s", int(rc), lastError())
	}
	return img, int(h), nil
}

// EncodePNG encodes nImages index images of one size (images = [nImages][height][width], back to back) as 8-bit indexed PNG streams
// in ONE device call: the file GenerateFromPCM (internal/spectrogram/generator.go:425-530) finds at its output path.  palette is
// 256 (r, g, b) entries.  The streams are the engine's own deterministic encoder (DESIGN.md section 9, "PNG"), not image/png's bytes.
func EncodePNG(images []uint8, nImages, width, height int, palette []uint8, device int) ([][]byte, error) {
	if nImages <= 0 || width <= 0 || height <= 0 || len(images) != nImages*width*height {
		return nil, fmt.Errorf("hip: png needs nImages > 0 images of width x height, got %d bytes for %d of %d x %d", len(images), nImages, width, height)
	}
	if len(palette) != 768 {
		return nil, fmt.Errorf("hip: png palette must hold 256 x 3 bytes, got %d", len(palette))
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var capBytes C.size_t
	if rc := C.bnbind_png_max_bytes(C.int(nImages), C.int(width), C.int(height), &capBytes); rc != 0 {
		return nil, fmt.Errorf("hip: png_max_bytes failed (%d): %s", int(rc), lastError())
	}
	buf := make([]byte, int(capBytes))
	offsets := make([]C.uint64_t, nImages+1)
	if rc := C.bnbind_png_encode_u8(C.int(device), (*C.uint8_t)(unsafe.Pointer(&images[0])), C.int(nImages), C.int(width), C.int(height),
		(*C.uint8_t)(unsafe.Pointer(&palette[0])), (*C.uint8_t)(unsafe.Pointer(&buf[0])), capBytes, &offsets[0]); rc != 0 {
		return nil, fmt.Errorf("hip: png_encode failed (%d): %s", int(rc), lastError())
	}
	return splitStreams(buf, offsets), nil
}

// RenderSpectrogramPNGs is RenderSpectrograms followed by EncodePNG in ONE device call: the level indices never leave the device,
// and the finished PNG files of a burst of detections return.  Each stream decodes to the image RenderSpectrograms gives.
func RenderSpectrogramPNGs(pcm []int16, nClips, sampleRate, width int, opts SpectrogramOptions, palette []uint8, device int) (files [][]byte, height int, err error) {
	if nClips <= 0 || len(pcm) == 0 || len(pcm)%nClips != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram needs nClips > 0 clips of one length, got %d samples for %d clips", len(pcm), nClips)
	}
	if len(palette) != 768 {
		return nil, 0, fmt.Errorf("hip: png palette must hold 256 x 3 bytes, got %d", len(palette))
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var h, fft C.int
	if rc := C.bnbind_spec_size(C.int(width), &h, &fft); rc != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram_size failed (%d): %s", int(rc), lastError())
	}
	var win *C.double
	if opts.Window != nil {
		if len(opts.Window) != int(fft) {
			return nil, 0, fmt.Errorf("hip: spectrogram window must hold %d coefficients, got %d", int(fft), len(opts.Window))
		}
		win = (*C.double)(unsafe.Pointer(&opts.Window[0]))
	}
	rangeDB := opts.RangeDB
	if rangeDB == 0 {
		rangeDB = 100
	}
	var capBytes C.size_t
	if rc := C.bnbind_png_max_bytes(C.int(nClips), C.int(width), h, &capBytes); rc != 0 {
		return nil, 0, fmt.Errorf("hip: png_max_bytes failed (%d): %s", int(rc), lastError())
	}
	buf := make([]byte, int(capBytes))
	offsets := make([]C.uint64_t, nClips+1)
	if rc := C.bnbind_spec_png_pcm16(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(nClips), C.int(len(pcm)/nClips),
		C.int(sampleRate), C.int(opts.ResampleRate), C.int(width), h, win, C.double(opts.TopDB), C.double(rangeDB),
		(*C.uint8_t)(unsafe.Pointer(&palette[0])), (*C.uint8_t)(unsafe.Pointer(&buf[0])), capBytes, &offsets[0]); rc != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram_png failed (%d): %s", int(rc), lastError())
	}
	return splitStreams(buf, offsets), int(h), nil
}

// raggedPack lays a burst of clips of any lengths out as the bnhip_*_ragged_* entries take it: the samples back to back and the lengths.
func raggedPack(clips [][]int16) (pcm []int16, lens []C.int, err error) {
	if len(clips) == 0 {
		return nil, nil, fmt.Errorf("hip: a ragged burst holds at least one clip")
	}
	total := 0
	for _, c := range clips {
		if len(c) == 0 {
			return nil, nil, fmt.Errorf("hip: a ragged burst holds no empty clip")
		}
		total += len(c)
	}
	pcm = make([]int16, 0, total)
	lens = make([]C.int, len(clips))
	for i, c := range clips {
		pcm = append(pcm, c...)
		lens[i] = C.int(len(c))
	}
	return pcm, lens, nil
}

// specRaggedArgs resolves what both ragged renders need of the width and the options: the height, the window pointer, the range.
func specRaggedArgs(width int, opts SpectrogramOptions) (h C.int, win *C.double, rangeDB float64, err error) {
	var fft C.int
	if rc := C.bnbind_spec_size(C.int(width), &h, &fft); rc != 0 {
		return 0, nil, 0, fmt.Errorf("hip: spectrogram_size failed (%d): %s", int(rc), lastError())
	}
	if opts.Window != nil {
		if len(opts.Window) != int(fft) {
			return 0, nil, 0, fmt.Errorf("hip: spectrogram window must hold %d coefficients, got %d", int(fft), len(opts.Window))
		}
		win = (*C.double)(unsafe.Pointer(&opts.Window[0]))
	}
	rangeDB = opts.RangeDB
	if rangeDB == 0 {
		rangeDB = 100
	}
	return h, win, rangeDB, nil
}

// RenderSpectrogramsRagged is RenderSpectrograms for clips of unequal lengths (detections under extended capture) in ONE device call:
// img is [len(clips)][height][width], image i what RenderSpectrograms gives clips[i] alone.
func RenderSpectrogramsRagged(clips [][]int16, sampleRate, width int, opts SpectrogramOptions, device int) (img []uint8, height int, err error) {
	pcm, lens, err := raggedPack(clips)
	if err != nil {
		return nil, 0, err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	h, win, rangeDB, err := specRaggedArgs(width, opts)
	if err != nil {
		return nil, 0, err
	}
	img = make([]uint8, len(clips)*int(h)*width)
	if rc := C.bnbind_spec_ragged_pcm16(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(len(clips)), &lens[0], C.int(sampleRate),
		C.int(opts.ResampleRate), C.int(width), h, win, C.double(opts.TopDB), C.double(rangeDB), (*C.uint8_t)(unsafe.Pointer(&img[0]))); rc != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram_ragged failed (%d): %s", int(rc), lastError())
	}
	return img, int(h), nil
}

// RenderSpectrogramPNGsRagged is RenderSpectrogramPNGs for clips of unequal lengths in ONE device call: file i decodes to image i of
// RenderSpectrogramsRagged.
func RenderSpectrogramPNGsRagged(clips [][]int16, sampleRate, width int, opts SpectrogramOptions, palette []uint8, device int) (files [][]byte, height int, err error) {
	if len(palette) != 768 {
		return nil, 0, fmt.Errorf("hip: png palette must hold 256 x 3 bytes, got %d", len(palette))
	}
	pcm, lens, err := raggedPack(clips)
	if err != nil {
		return nil, 0, err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	h, win, rangeDB, err := specRaggedArgs(width, opts)
	if err != nil {
		return nil, 0, err
	}
	var capBytes C.size_t
	if rc := C.bnbind_png_max_bytes(C.int(len(clips)), C.int(width), h, &capBytes); rc != 0 {
		return nil, 0, fmt.Errorf("hip: png_max_bytes failed (%d): %s", int(rc), lastError())
	}
	buf := make([]byte, int(capBytes))
	offsets := make([]C.uint64_t, len(clips)+1)
	if rc := C.bnbind_spec_png_ragged_pcm16(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(len(clips)), &lens[0], C.int(sampleRate),
		C.int(opts.ResampleRate), C.int(width), h, win, C.double(opts.TopDB), C.double(rangeDB), (*C.uint8_t)(unsafe.Pointer(&palette[0])),
		(*C.uint8_t)(unsafe.Pointer(&buf[0])), capBytes, &offsets[0]); rc != 0 {
		return nil, 0, fmt.Errorf("hip: spectrogram_png_ragged failed (%d): %s", int(rc), lastError())
	}
	return splitStreams(buf, offsets), int(h), nil
}

// Loudness is one clip's EBU R 128 measurement and gain plan (bnhip.h bnhip_loudness): what audionorm.Measurement, audionorm.Result
// and the export path's gate fallback (analysis/processor/actions_database.go:1392-1438) report, in one record.  The measurement
// follows the engine's float64 spec; the reference's meter is float32 (within 1e-3 LU / 1e-3 dBTP of it).
type Loudness struct {
	IntegratedLUFS float64 // -Inf: shorter than one 400 ms block, or under the absolute gate
	TruePeakDBTP   float64 // -Inf: digital silence
	TruePeak       float64
	TargetGainDB   float64
	LiftDB         float64 // the gate fallback's lift (GateLifted)
	PlannedGainDB  float64 // before the clamp
	GainDB         float64 // what is applied
	Factor         float64 // pcmgain.FactorFromDB(GainDB): exactly 1 at 0 dB
	OutputLUFS     float64
	PeakLimited    bool
	GateLifted     bool
	Clamped        bool
}

// LoudnessOptions are the knobs of one plan.  The reference's callers: the clip export passes MaxGainDB 60 with GateFallback
// (nativeExportMaxGainDB), the BirdWeather upload MaxGainDB 30 without (audionorm.DefaultMaxGainDB).  Zero TargetLUFS / MaxGainDB
// mean audionorm.DefaultOptions' -23 LUFS and 30 dB; a zero TruePeakDBTP is a valid ceiling, so set it (-1 by default there).
type LoudnessOptions struct {
	TargetLUFS   float64
	TruePeakDBTP float64
	MaxGainDB    float64
	GateFallback bool
	PlanOnly     bool // measure and plan, return no samples
	LPCOrder     int  // NormalizeAndEncodeFLAC only: 0, or 1..8 to try LPC subframes of that many orders (Level5LPCOrder)
}

// Level5LPCOrder is the lpcOrder that stands for the reference's CompressionLevel 5 (flac/encode.go:25,136-145,350-358).
const Level5LPCOrder = 8

const (
	loudnessPeakLimited = 1
	loudnessGateLifted  = 2
	loudnessClamped     = 4
)

func loudnessFromC(in []C.bnhip_loudness) []Loudness {
	out := make([]Loudness, len(in))
	for i := range in {
		c := &in[i]
		out[i] = Loudness{
			IntegratedLUFS: float64(c.integrated_lufs), TruePeakDBTP: float64(c.true_peak_dbtp), TruePeak: float64(c.true_peak),
			TargetGainDB: float64(c.target_gain_db), LiftDB: float64(c.lift_db), PlannedGainDB: float64(c.planned_gain_db),
			GainDB: float64(c.gain_db), Factor: float64(c.factor), OutputLUFS: float64(c.output_lufs),
			PeakLimited: int(c.flags)&loudnessPeakLimited != 0, GateLifted: int(c.flags)&loudnessGateLifted != 0,
			Clamped: int(c.flags)&loudnessClamped != 0,
		}
	}
	return out
}

// MeasureLoudness measures nClips mono PCM16 clips of one length (pcm = the clips back to back) in ONE device call
// (audionorm.MeasureInt16 per clip in the reference).
func MeasureLoudness(pcm []int16, nClips, sampleRate, device int) ([]Loudness, error) {
	if nClips <= 0 || len(pcm) == 0 || len(pcm)%nClips != 0 {
		return nil, fmt.Errorf("hip: loudness needs nClips > 0 clips of one length, got %d samples for %d clips", len(pcm), nClips)
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	res := make([]C.bnhip_loudness, nClips)
	if rc := C.bnbind_loud_measure(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(nClips), C.int(len(pcm)/nClips),
		C.int(sampleRate), &res[0], nil); rc != 0 {
		return nil, fmt.Errorf("hip: loudness_measure failed (%d): %s", int(rc), lastError())
	}
	return loudnessFromC(res), nil
}

// NormalizeClips measures, plans and gains a burst of nClips mono PCM16 clips of one length in ONE device call: what
// planNativeNormalizationGain + pcmgain.Applied do clip by clip for an export, PlanClampedGainInt16Bytes for an upload.  pcm is
// not modified; out holds the gained clips back to back (nil with PlanOnly).
func NormalizeClips(pcm []int16, nClips, sampleRate int, opts LoudnessOptions, device int) (out []int16, res []Loudness, err error) {
	if nClips <= 0 || len(pcm) == 0 || len(pcm)%nClips != 0 {
		return nil, nil, fmt.Errorf("hip: loudness needs nClips > 0 clips of one length, got %d samples for %d clips", len(pcm), nClips)
	}
	target, maxGain := opts.TargetLUFS, opts.MaxGainDB
	if target == 0 {
		target = -23
	}
	if maxGain == 0 {
		maxGain = 30
	}
	fallback := 0
	if opts.GateFallback {
		fallback = 1
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	cres := make([]C.bnhip_loudness, nClips)
	var outPtr *C.int16_t
	if !opts.PlanOnly {
		out = make([]int16, len(pcm))
		outPtr = (*C.int16_t)(unsafe.Pointer(&out[0]))
	}
	if rc := C.bnbind_loud_normalize(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(nClips), C.int(len(pcm)/nClips),
		C.int(sampleRate), C.double(target), C.double(opts.TruePeakDBTP), C.double(maxGain), C.int(fallback), outPtr, &cres[0]); rc != 0 {
		return nil, nil, fmt.Errorf("hip: loudness_normalize failed (%d): %s", int(rc), lastError())
	}
	return out, loudnessFromC(cres), nil
}

// splitStreams cuts the streams an encode entry wrote back to back at their offsets; each stream is its own copy.
func splitStreams(buf []byte, offsets []C.uint64_t) [][]byte {
	out := make([][]byte, len(offsets)-1)
	for i := range out {
		out[i] = append([]byte(nil), buf[int(offsets[i]):int(offsets[i+1])]...)
	}
	return out
}

// EncodeFLAC encodes nClips mono PCM16 clips of one length (pcm = the clips back to back) to FLAC in ONE device call: what
// flac.EncodePCMToBuffer does clip by clip (seekInterval 0), or flac.EncodePCM with its seek table (seekInterval = the sample
// rate).  gainDB: nil, or one gain per clip, applied on the device first (pcmgain.FactorFromDB, then the saturating int16 gain).
// The bytes follow the project's own encoder spec (DESIGN.md section 9): valid RFC 9639 streams, not go-flac's bytes.
func EncodeFLAC(pcm []int16, nClips, sampleRate int, gainDB []float64, seekInterval, device int) ([][]byte, error) {
	if err := flacArgs(len(pcm), nClips, gainDB); err != nil {
		return nil, err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	streams, what, rc := encodeFLACLocked(pcm, nClips, sampleRate, gainDB, seekInterval, 0, device)
	if rc != 0 {
		return nil, fmt.Errorf("hip: %s (%d): %s", what, rc, lastError())
	}
	return streams, nil
}

// EncodeFLACLPC is EncodeFLAC with LPC subframes of orders 1..lpcOrder among a frame's candidates (lpcOrder in 0..8; 0 is
// EncodeFLAC byte for byte, Level5LPCOrder the reference's level).  The spec is DESIGN.md section 9.
func EncodeFLACLPC(pcm []int16, nClips, sampleRate int, gainDB []float64, seekInterval, lpcOrder, device int) ([][]byte, error) {
	if err := flacArgs(len(pcm), nClips, gainDB); err != nil {
		return nil, err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	streams, what, rc := encodeFLACLocked(pcm, nClips, sampleRate, gainDB, seekInterval, lpcOrder, device)
	if rc != 0 {
		return nil, fmt.Errorf("hip: %s (%d): %s", what, rc, lastError())
	}
	return streams, nil
}

// flacArgs is what EncodeFLAC and EncodeFLACLPC check before the library is called.
func flacArgs(samples, nClips int, gainDB []float64) error {
	if nClips <= 0 || samples == 0 || samples%nClips != 0 {
		return fmt.Errorf("hip: flac needs nClips > 0 clips of one length, got %d samples for %d clips", samples, nClips)
	}
	if gainDB != nil && len(gainDB) != nClips {
		return fmt.Errorf("hip: flac needs one gain per clip, got %d for %d clips", len(gainDB), nClips)
	}
	return nil
}

// encodeFLACLocked is the body of EncodeFLAC and EncodeFLACLPC after flacArgs.  The caller holds the OS thread (the library's last
// error is per thread) and turns a non-zero code into an error: -> (streams, what failed, the BNHIP_E_* code).
func encodeFLACLocked(pcm []int16, nClips, sampleRate int, gainDB []float64, seekInterval, lpcOrder, device int) ([][]byte, string, int) {
	n := len(pcm) / nClips
	var capBytes C.size_t
	if rc := C.bnbind_flac_max_bytes(C.int(nClips), C.int(n), C.int(seekInterval), &capBytes); rc != 0 {
		return nil, "flac_max_bytes failed", int(rc)
	}
	var facPtr *C.double
	if gainDB != nil {
		factor := make([]C.double, nClips)
		for i, g := range gainDB {
			factor[i] = 1
			if g != 0 {
				factor[i] = C.double(math.Pow(10, g/20))
			}
		}
		facPtr = &factor[0]
	}
	buf := make([]byte, int(capBytes))
	offsets := make([]C.uint64_t, nClips+1)
	if rc := C.bnbind_flac_lpc_encode_pcm16(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(nClips), C.int(n), C.int(sampleRate),
		facPtr, C.int(seekInterval), (*C.uint8_t)(unsafe.Pointer(&buf[0])), capBytes, &offsets[0], C.int(lpcOrder)); rc != 0 {
		return nil, "flac_encode failed", int(rc)
	}
	return splitStreams(buf, offsets), "", 0
}

// NormalizeAndEncodeFLAC is NormalizeClips followed by EncodeFLAC in ONE device call (encodeFLACNative, birdweather/
// encode_native.go:28-98, for a burst; with GateFallback, MaxGainDB 60 and seekInterval = the sample rate the detection save): the
// normalised PCM never leaves the device - the loudness records and the compressed streams return.  opts.PlanOnly is ignored;
// opts.LPCOrder is EncodeFLACLPC's lpcOrder.
func NormalizeAndEncodeFLAC(pcm []int16, nClips, sampleRate int, opts LoudnessOptions, seekInterval, device int) (streams [][]byte, res []Loudness, err error) {
	if nClips <= 0 || len(pcm) == 0 || len(pcm)%nClips != 0 {
		return nil, nil, fmt.Errorf("hip: flac needs nClips > 0 clips of one length, got %d samples for %d clips", len(pcm), nClips)
	}
	target, maxGain := opts.TargetLUFS, opts.MaxGainDB
	if target == 0 {
		target = -23
	}
	if maxGain == 0 {
		maxGain = 30
	}
	fallback := 0
	if opts.GateFallback {
		fallback = 1
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	n := len(pcm) / nClips
	var capBytes C.size_t
	if rc := C.bnbind_flac_max_bytes(C.int(nClips), C.int(n), C.int(seekInterval), &capBytes); rc != 0 {
		return nil, nil, fmt.Errorf("hip: flac_max_bytes failed (%d): %s", int(rc), lastError())
	}
	cres := make([]C.bnhip_loudness, nClips)
	buf := make([]byte, int(capBytes))
	offsets := make([]C.uint64_t, nClips+1)
	if rc := C.bnbind_loud_flac_lpc_pcm16(C.int(device), (*C.int16_t)(unsafe.Pointer(&pcm[0])), C.int(nClips), C.int(n), C.int(sampleRate),
		C.double(target), C.double(opts.TruePeakDBTP), C.double(maxGain), C.int(fallback), C.int(seekInterval), &cres[0],
		(*C.uint8_t)(unsafe.Pointer(&buf[0])), capBytes, &offsets[0], C.int(opts.LPCOrder)); rc != 0 {
		return nil, nil, fmt.Errorf("hip: loudness_flac failed (%d): %s", int(rc), lastError())
	}
	return splitStreams(buf, offsets), loudnessFromC(cres), nil
}

// Resampler mirrors internal/audiocore/resample.Resampler (resample.go:44-224) method for method: a stateful PCM16 resampler
// whose filter history lives on the device between calls, so ~100 ms frames (analysis/buffer_consumer.go:118,192) resample to
// exactly the samples one call over the whole stream would give.  Not safe for concurrent use (resample.go:43).
type Resampler struct {
	h        *C.bnhip_resampler
	fromRate int
	toRate   int
	outBuf   []byte
}

const bytesPerSample = 2

// NewResampler returns nil, nil when fromRate == toRate - no resampling is required (resample.go:57-60).
func NewResampler(fromRate, toRate int, device int) (*Resampler, error) {
	if fromRate == toRate {
		return nil, nil //nolint:nilnil // as the reference: nil means "no resampling needed"
	}
	var h *C.bnhip_resampler
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_rs_create(C.int(device), C.int(fromRate), C.int(toRate), &h); rc != 0 || h == nil {
		return nil, fmt.Errorf("failed to create resampler from %d Hz to %d Hz: %s", fromRate, toRate, lastError())
	}
	return &Resampler{h: h, fromRate: fromRate, toRate: toRate}, nil
}

// EstimateOutputBytes: the maximum number of bytes ResampleTo may write for the given input length (resample.go:83-88).
func (r *Resampler) EstimateOutputBytes(inputBytes int) int {
	if inputBytes <= 0 {
		return 0
	}
	return int(C.bnbind_rs_estimate(r.h, C.int(inputBytes/bytesPerSample))) * bytesPerSample
}

// ResampleTo resamples raw 16-bit PCM into dst and returns the bytes written; a dst shorter than EstimateOutputBytes is an
// error that leaves the resampler state untouched; empty input writes nothing (resample.go:99-172).
func (r *Resampler) ResampleTo(input, dst []byte) (int, error) {
	if len(input) == 0 {
		return 0, nil
	}
	if len(input)%bytesPerSample != 0 {
		return 0, fmt.Errorf("input length %d is not a multiple of %d", len(input), bytesPerSample)
	}
	if need := r.EstimateOutputBytes(len(input)); len(dst) < need {
		return 0, fmt.Errorf("destination buffer too small: need %d bytes, have %d", need, len(dst))
	}
	var n C.int
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_rs_process_pcm16(r.h, (*C.int16_t)(unsafe.Pointer(&input[0])), C.int(len(input)/bytesPerSample),
		(*C.int16_t)(unsafe.Pointer(&dst[0])), C.int(len(dst)/bytesPerSample), &n); rc != 0 {
		return 0, fmt.Errorf("hip: resample failed (%d): %s", int(rc), lastError())
	}
	return int(n) * bytesPerSample, nil
}

// ResampleInto resamples into the resampler's own output buffer; the returned slice is valid until the next call
// (resample.go:179-196).
func (r *Resampler) ResampleInto(input []byte) ([]byte, error) {
	need := r.EstimateOutputBytes(len(input))
	if cap(r.outBuf) < need {
		r.outBuf = make([]byte, need)
	}
	r.outBuf = r.outBuf[:cap(r.outBuf)]
	n, err := r.ResampleTo(input, r.outBuf)
	if err != nil {
		return nil, err
	}
	return r.outBuf[:n], nil
}

// Flush emits the tail that needs zero-padded future input and resets the state for a new stream (the go-audio-resampler
// engine's Flush, which the reference's one-shot ResampleBytes relies on, resample.go:228-262).
func (r *Resampler) Flush() ([]byte, error) {
	out := make([]byte, r.EstimateOutputBytes(2*bytesPerSample)+64*bytesPerSample)
	var n C.int
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	for {
		rc := C.bnbind_rs_flush_pcm16(r.h, (*C.int16_t)(unsafe.Pointer(&out[0])), C.int(len(out)/bytesPerSample), &n)
		if rc == 0 {
			return out[:int(n)*bytesPerSample], nil
		}
		if rc != -1 || len(out) > 1<<26 {
			return nil, fmt.Errorf("hip: resample flush failed (%d): %s", int(rc), lastError())
		}
		out = make([]byte, 2*len(out)) // destination too small: nothing was consumed, retry larger
	}
}

func (r *Resampler) FromRate() int { return r.fromRate }
func (r *Resampler) ToRate() int   { return r.toRate }

// Close releases the device state; idempotent (resample.go:206-217).
func (r *Resampler) Close() error {
	if r != nil && r.h != nil {
		C.bnbind_rs_destroy(r.h)
		r.h = nil
	}
	return nil
}

func (r *Resampler) String() string { return fmt.Sprintf("Resampler(%d Hz -> %d Hz, hip)", r.fromRate, r.toRate) }

// ResampleBytes is the one-shot helper (resample.go:228-262): equal rates return the input unchanged; otherwise a fresh
// resampler processes the input once and an independent copy of what it emitted is returned (like the reference, without a
// flush: the last ~10 output samples, which need future input, are not produced).
func ResampleBytes(pcm []byte, fromRate, toRate int, device int) ([]byte, error) {
	if fromRate == toRate {
		return pcm, nil
	}
	r, err := NewResampler(fromRate, toRate, device)
	if err != nil {
		return nil, err
	}
	defer func() { _ = r.Close() }()
	out, err := r.ResampleInto(pcm)
	if err != nil {
		return nil, err
	}
	result := make([]byte, len(out))
	copy(result, out)
	return result, nil
}

// ResamplerBank is BufferConsumer.Write's rate fan-out (internal/analysis/buffer_consumer.go:105-210: one Resampler per
// (source, non-native rate)) for every source of ONE (fromRate, toRate) pair: a stream per source, and each call resamples
// all the frames it is given in one device call (bnhip_resampler_bank_*).  Every stream's bytes are those its own Resampler
// would return for the same frames.  Calls are serialised on the bank.
type ResamplerBank struct {
	bankStage
	h                *C.bnhip_resampler_bank
	fromRate, toRate int
}

// NewResamplerBank: nil, nil for equal rates, as NewResampler.
func NewResamplerBank(fromRate, toRate, maxStreams, device int) (*ResamplerBank, error) {
	if fromRate == toRate {
		return nil, nil //nolint:nilnil // as the reference's NewResampler: nil means "no resampling needed"
	}
	var h *C.bnhip_resampler_bank
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_rb_create(C.int(device), C.int(fromRate), C.int(toRate), C.int(maxStreams), &h); rc != 0 || h == nil {
		return nil, fmt.Errorf("failed to create resampler bank from %d Hz to %d Hz: %s", fromRate, toRate, lastError())
	}
	return &ResamplerBank{bankStage: bankStage{what: "resampler bank"}, h: h, fromRate: fromRate, toRate: toRate}, nil
}

// AddStream starts a stream (one source's Resampler); slots of removed streams are reused with fresh state.
func (b *ResamplerBank) AddStream() (int, error) {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return -1, errors.New("hip: resampler bank is closed")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var s C.int
	if rc := C.bnbind_rb_add_stream(b.h, &s); rc != 0 {
		return -1, fmt.Errorf("hip: resampler_bank_add_stream failed (%d): %s", int(rc), lastError())
	}
	return int(s), nil
}

func (b *ResamplerBank) RemoveStream(stream int) error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_rb_remove_stream(b.h, C.int(stream)); rc != 0 {
		return fmt.Errorf("hip: resampler_bank_remove_stream failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// EstimateOutputBytes = Resampler.EstimateOutputBytes for one frame (resample.go:83-88).
func (b *ResamplerBank) EstimateOutputBytes(inputBytes int) int {
	if inputBytes <= 0 || b.h == nil {
		return 0
	}
	return int(C.bnbind_rb_estimate(b.h, C.int(inputBytes/bytesPerSample))) * bytesPerSample
}

// Process resamples frames[k] of streams[k] for every k in one device call -> one slice per frame, each what that stream's
// Resampler.ResampleInto returns for it in sequence (a stream may appear several times; its frames go in slice order).  An
// unknown stream or an odd byte count fails the whole call before any stream advances.
func (b *ResamplerBank) Process(streams []int, frames [][]byte) ([][]byte, error) {
	if len(streams) != len(frames) {
		return nil, fmt.Errorf("hip: %d streams for %d frames", len(streams), len(frames))
	}
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return nil, errors.New("hip: resampler bank is closed")
	}
	if len(frames) == 0 {
		return nil, nil
	}
	ptrs, lens, err := b.stage(frames)
	if err != nil {
		return nil, err
	}
	st := make([]C.int, len(streams))
	capSamples := 0
	for k, s := range streams {
		st[k] = C.int(s)
		capSamples += int(C.bnbind_rb_estimate(b.h, lens[k]))
	}
	out := make([]int16, capSamples+1)
	counts := make([]C.int, len(frames))
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_rb_process_pcm16(b.h, C.int(len(frames)), &st[0], ptrs, &lens[0], (*C.int16_t)(unsafe.Pointer(&out[0])),
		C.size_t(capSamples), &counts[0]); rc != 0 {
		return nil, fmt.Errorf("hip: resampler bank failed (%d): %s", int(rc), lastError())
	}
	return splitPacked(out, counts), nil
}

// Flush ends each listed stream (each at most once): its tail, then the stream starts anew (Resampler.Flush).
func (b *ResamplerBank) Flush(streams []int) ([][]byte, error) {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return nil, errors.New("hip: resampler bank is closed")
	}
	if len(streams) == 0 {
		return nil, nil
	}
	st := make([]C.int, len(streams))
	for k, s := range streams {
		st[k] = C.int(s)
	}
	const tailCap = 1 << 16
	out := make([]int16, tailCap*len(streams))
	counts := make([]C.int, len(streams))
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_rb_flush_pcm16(b.h, C.int(len(streams)), &st[0], (*C.int16_t)(unsafe.Pointer(&out[0])), C.size_t(len(out)),
		&counts[0]); rc != 0 {
		return nil, fmt.Errorf("hip: resampler bank flush failed (%d): %s", int(rc), lastError())
	}
	return splitPacked(out, counts), nil
}

func (b *ResamplerBank) FromRate() int { return b.fromRate }
func (b *ResamplerBank) ToRate() int   { return b.toRate }

func (b *ResamplerBank) Close() error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h != nil {
		C.bnbind_rb_destroy(b.h)
		b.h = nil
	}
	b.release()
	return nil
}

// WriteResampled is BufferConsumer.Write's non-native rate group for every source of a tick at once: frames[k] (captured at
// the bank's fromRate) is resampled on streams[k] of bank and written into sources[k] of this assembler, one ring write per
// input frame (AnalysisBuffer.Write per frame, analysis.go:152-175), in one device call.  Every source and stream is checked
// before anything runs: an error leaves every stream and every ring as it was.
func (w *WindowAssembler) WriteResampled(bank *ResamplerBank, streams, sources []int, frames [][]byte) error {
	return w.writeFrames(&bank.bankStage, func() bool { return bank.h != nil }, streams, sources, frames,
		func(n C.int, st, src *C.int, ptrs **C.int16_t, lens *C.int) C.int {
			return C.bnbind_win_write_resampled(w.h, bank.h, n, st, src, ptrs, lens)
		})
}

// EqualizerBank is the analysis route's processing, AudioRouter.applyProcessing (internal/audiocore/router.go:1006-1080), for
// many sources: a stream per source holds its FilterChain and gainLinear, and each call converts, filters, scales and
// truncates all the frames it is given in one device call (bnhip_eq_bank_*).  Every stream's bytes are those of the
// reference's float64 arithmetic for the same sections.  Calls are serialised on the bank.
type EqualizerBank struct {
	bankStage
	h *C.bnhip_eq_bank
}

func NewEqualizerBank(maxStreams, device int) (*EqualizerBank, error) {
	var h *C.bnhip_eq_bank
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_eq_create(C.int(device), C.int(maxStreams), &h); rc != 0 || h == nil {
		return nil, fmt.Errorf("failed to create equalizer bank: %s", lastError())
	}
	return &EqualizerBank{bankStage: bankStage{what: "equalizer bank"}, h: h}, nil
}

// AddStream starts a stream with no chain and gain 1 (pass-through); slots of removed streams are reused with fresh state.
func (b *EqualizerBank) AddStream() (int, error) {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return -1, errors.New("hip: equalizer bank is closed")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var s C.int
	if rc := C.bnbind_eq_add_stream(b.h, &s); rc != 0 {
		return -1, fmt.Errorf("hip: eq_bank_add_stream failed (%d): %s", int(rc), lastError())
	}
	return int(s), nil
}

func (b *EqualizerBank) RemoveStream(stream int) error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_eq_remove_stream(b.h, C.int(stream)); rc != 0 {
		return fmt.Errorf("hip: eq_bank_remove_stream failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// SetChain installs a route's chain and gain (AddRoute / UpdateFilterChain) with zero state.  More than 16 stages (the sum
// of passes) is refused; a refused call leaves the old chain and its state.
func (b *EqualizerBank) SetChain(stream int, sections []EqualizerSection, gainLinear float64) error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return errors.New("hip: equalizer bank is closed")
	}
	coef := make([]C.double, 6*len(sections)+1)
	passes := make([]C.int, len(sections)+1)
	for k, s := range sections {
		for j, v := range s.Coef {
			coef[6*k+j] = C.double(v)
		}
		passes[k] = C.int(s.Passes)
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_eq_set_chain(b.h, C.int(stream), &coef[0], C.int(len(sections)), &passes[0], C.double(gainLinear)); rc != 0 {
		return fmt.Errorf("hip: eq_bank_set_chain failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// Reset is FilterChain.Reset: zero state, same chain.
func (b *EqualizerBank) Reset(stream int) error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return errors.New("hip: equalizer bank is closed")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_eq_reset(b.h, C.int(stream)); rc != 0 {
		return fmt.Errorf("hip: eq_bank_reset failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// Process runs frames[k] of streams[k] for every k in one device call -> one slice per frame, as long as its input (a stream
// may appear several times; its frames go in slice order).  An unknown stream or an odd byte count fails the whole call
// before any stream advances.
func (b *EqualizerBank) Process(streams []int, frames [][]byte) ([][]byte, error) {
	if len(streams) != len(frames) {
		return nil, fmt.Errorf("hip: %d streams for %d frames", len(streams), len(frames))
	}
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return nil, errors.New("hip: equalizer bank is closed")
	}
	if len(frames) == 0 {
		return nil, nil
	}
	ptrs, lens, err := b.stage(frames)
	if err != nil {
		return nil, err
	}
	st := make([]C.int, len(streams))
	total := 0
	for k, s := range streams {
		st[k] = C.int(s)
		total += int(lens[k])
	}
	out := make([]int16, total+1)
	counts := make([]C.int, len(frames))
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_eq_process_pcm16(b.h, C.int(len(frames)), &st[0], ptrs, &lens[0], (*C.int16_t)(unsafe.Pointer(&out[0])),
		C.size_t(total), &counts[0]); rc != 0 {
		return nil, fmt.Errorf("hip: equalizer bank failed (%d): %s", int(rc), lastError())
	}
	return splitPacked(out, counts), nil
}

func (b *EqualizerBank) Close() error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h != nil {
		C.bnbind_eq_destroy(b.h)
		b.h = nil
	}
	b.release()
	return nil
}

// WriteEqualized processes frames[k] on streams[k] of bank and writes the result into sources[k] of this assembler, one ring
// write per frame, in one device call.  Every source and stream is checked before anything runs: an error leaves every
// stream and every ring as it was.
func (w *WindowAssembler) WriteEqualized(bank *EqualizerBank, streams, sources []int, frames [][]byte) error {
	return w.writeFrames(&bank.bankStage, func() bool { return bank.h != nil }, streams, sources, frames,
		func(n C.int, st, src *C.int, ptrs **C.int16_t, lens *C.int) C.int {
			return C.bnbind_win_write_equalized(w.h, bank.h, n, st, src, ptrs, lens)
		})
}

// SoundLevelBank is the 1/3-octave sound level monitor, soundlevel.Processor behind one SoundLevelConsumer route per source
// (internal/analysis/audio_pipeline_service.go:685-740), for many sources of ONE sample rate: a stream per source, and each
// call runs every frame it is given as one ProcessSamples call, in one device call (bnhip_soundlevel_bank_*).  Calls are
// serialised on the bank.
type SoundLevelBank struct {
	bankStage
	h *C.bnhip_soundlevel_bank
}

// NewSoundLevelBank: bands from BuildSoundLevelBands (bit-equal to the reference's); nil = the library's own table, whose
// coefficients come from the C library's math and may differ from Go's in the last ulp.
func NewSoundLevelBank(sampleRate, maxStreams, device int, bands []SoundLevelBand) (*SoundLevelBank, error) {
	tbl := make([]C.double, 6*len(bands)+1)
	for j, b := range bands {
		for i, v := range [6]float64{b.CenterFreq, b.B0, b.B1, b.B2, b.A1, b.A2} {
			tbl[6*j+i] = C.double(v)
		}
	}
	var ptr *C.double
	if len(bands) > 0 {
		ptr = &tbl[0]
	}
	var h *C.bnhip_soundlevel_bank
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_sl_create(C.int(device), C.int(sampleRate), C.int(maxStreams), ptr, C.int(len(bands)), &h); rc != 0 || h == nil {
		return nil, fmt.Errorf("failed to create sound level bank at %d Hz: %s", sampleRate, lastError())
	}
	return &SoundLevelBank{bankStage: bankStage{what: "sound level bank"}, h: h}, nil
}

// AddStream starts a fresh Processor reporting every intervalSeconds (below 1: 1); slots of removed streams are reused.
func (b *SoundLevelBank) AddStream(intervalSeconds int) (int, error) {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return -1, errors.New("hip: sound level bank is closed")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var s C.int
	if rc := C.bnbind_sl_add_stream(b.h, C.int(intervalSeconds), &s); rc != 0 {
		return -1, fmt.Errorf("hip: soundlevel_bank_add_stream failed (%d): %s", int(rc), lastError())
	}
	return int(s), nil
}

func (b *SoundLevelBank) RemoveStream(stream int) error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_sl_remove_stream(b.h, C.int(stream)); rc != 0 {
		return fmt.Errorf("hip: soundlevel_bank_remove_stream failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// Reset is Processor.Reset: zero filter state, the partial second, the unmeasured blocks and the interval dropped.
func (b *SoundLevelBank) Reset(stream int) error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return errors.New("hip: sound level bank is closed")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_sl_reset(b.h, C.int(stream)); rc != 0 {
		return fmt.Errorf("hip: soundlevel_bank_reset failed (%d): %s", int(rc), lastError())
	}
	return nil
}

// Process runs frames[k] of streams[k] for every k as one ProcessSamples call each, in one device call -> the finished
// reports in frame order (an empty frame is not a call).  An unknown stream or an odd byte count fails the whole call before
// any stream advances.
func (b *SoundLevelBank) Process(streams []int, frames [][]byte) ([]SoundLevelReport, error) {
	if len(streams) != len(frames) {
		return nil, fmt.Errorf("hip: %d streams for %d frames", len(streams), len(frames))
	}
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h == nil {
		return nil, errors.New("hip: sound level bank is closed")
	}
	if len(frames) == 0 {
		return nil, nil
	}
	ptrs, lens, err := b.stage(frames)
	if err != nil {
		return nil, err
	}
	st := make([]C.int, len(streams))
	maxReports := 0
	for k, s := range streams {
		st[k] = C.int(s)
		if lens[k] > 0 {
			maxReports++ // at most one report per ProcessSamples call
		}
	}
	reps := (*C.bnhip_sound_level)(C.malloc(C.size_t(maxReports+1) * C.size_t(unsafe.Sizeof(C.bnhip_sound_level{}))))
	if reps == nil {
		return nil, errors.New("hip: out of host memory (sound level reports)")
	}
	defer C.free(unsafe.Pointer(reps))
	var n C.int
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.bnbind_sl_process_pcm16(b.h, C.int(len(frames)), &st[0], ptrs, &lens[0], reps, C.int(maxReports), &n); rc != 0 {
		return nil, fmt.Errorf("hip: sound level bank failed (%d): %s", int(rc), lastError())
	}
	out := make([]SoundLevelReport, int(n))
	for i, r := range unsafe.Slice(reps, int(n)) {
		rep := SoundLevelReport{Stream: int(r.stream), Frame: int(r.frame), Duration: int(r.duration_s),
			OctaveBands: make(map[string]SoundLevelBandData, int(r.n_bands))}
		for j := 0; j < int(r.n_bands); j++ {
			rep.OctaveBands[SoundLevelBandKey(float64(r.center_hz[j]))] = SoundLevelBandData{CenterFreq: float64(r.center_hz[j]),
				Min: float64(r.min_db[j]), Max: float64(r.max_db[j]), Mean: float64(r.mean_db[j]), SampleCount: int(r.sample_count[j])}
		}
		out[i] = rep
	}
	return out, nil
}

func (b *SoundLevelBank) Close() error {
	b.mu.Lock()
	defer b.mu.Unlock()
	if b.h != nil {
		C.bnbind_sl_destroy(b.h)
		b.h = nil
	}
	b.release()
	return nil
}

// bankStage is what every bank shares: the mutex that serialises calls on the bank, its name in errors, and the C memory a call
// stages its frames in (cgo: C may not keep or receive Go pointers into Go memory).
type bankStage struct {
	mu      sync.Mutex
	what    string         // "resampler bank" | "equalizer bank" | "sound level bank"
	buf     unsafe.Pointer // C memory: this call's frames back to back
	bufCap  int
	ptrs    unsafe.Pointer // C memory: one const int16_t* per frame
	ptrsCap int
}

// stage copies the frames into the C staging (the caller holds mu); -> the pointer table, the per-frame sample counts.
func (s *bankStage) stage(frames [][]byte) (**C.int16_t, []C.int, error) {
	total := 0
	for _, f := range frames {
		if len(f)%bytesPerSample != 0 {
			return nil, nil, fmt.Errorf("input length %d is not a multiple of %d", len(f), bytesPerSample)
		}
		total += len(f)
	}
	if total > s.bufCap || s.buf == nil {
		C.free(s.buf)
		s.buf, s.bufCap = C.malloc(C.size_t(total+1)), total+1
	}
	if len(frames) > s.ptrsCap || s.ptrs == nil {
		C.free(s.ptrs)
		s.ptrs, s.ptrsCap = C.malloc(C.size_t((len(frames)+1)*int(unsafe.Sizeof(uintptr(0))))), len(frames)+1
	}
	if s.buf == nil || s.ptrs == nil {
		s.release()
		return nil, nil, fmt.Errorf("hip: out of host memory (%s staging)", s.what)
	}
	lens := make([]C.int, len(frames)+1)
	offs := make([]C.int, len(frames)+1)
	buf := unsafe.Slice((*byte)(s.buf), s.bufCap)
	pos := 0
	for k, f := range frames {
		copy(buf[pos:], f)
		offs[k], lens[k] = C.int(pos), C.int(len(f)/bytesPerSample)
		pos += len(f)
	}
	C.bnbind_rb_point((**C.int16_t)(s.ptrs), (*C.char)(s.buf), &offs[0], C.int(len(frames)))
	return (**C.int16_t)(s.ptrs), lens, nil
}

// release frees the staging (the caller holds mu); the next stage allocates anew.
func (s *bankStage) release() {
	C.free(s.buf)
	C.free(s.ptrs)
	s.buf, s.bufCap, s.ptrs, s.ptrsCap = nil, 0, nil, 0
}

// splitPacked cuts a bank call's packed outputs into one slice per frame, counts[k] samples each (views of out).
func splitPacked(out []int16, counts []C.int) [][]byte {
	res := make([][]byte, len(counts))
	raw := unsafe.Slice((*byte)(unsafe.Pointer(&out[0])), len(out)*bytesPerSample)
	pos := 0
	for k, c := range counts {
		n := int(c) * bytesPerSample
		res[k] = raw[pos : pos+n : pos+n]
		pos += n
	}
	return res
}

// writeFrames is the body of WriteResampled and WriteEqualized: with the assembler and the bank locked and open, the frames staged
// in the bank's C memory and write(n, streams, sources, frame pointers, lengths) = that bank's bnhip_windows_write_* call.
func (w *WindowAssembler) writeFrames(bank *bankStage, open func() bool, streams, sources []int, frames [][]byte,
	write func(n C.int, st, src *C.int, ptrs **C.int16_t, lens *C.int) C.int) error {
	if len(streams) != len(frames) || len(sources) != len(frames) {
		return fmt.Errorf("hip: %d streams and %d sources for %d frames", len(streams), len(sources), len(frames))
	}
	w.life.RLock()
	defer w.life.RUnlock()
	if w.h == nil {
		return errors.New("hip: window assembler is closed")
	}
	bank.mu.Lock()
	defer bank.mu.Unlock()
	if !open() {
		return fmt.Errorf("hip: %s is closed", bank.what)
	}
	if len(frames) == 0 {
		return nil
	}
	ptrs, lens, err := bank.stage(frames)
	if err != nil {
		return err
	}
	st := make([]C.int, len(frames))
	src := make([]C.int, len(frames))
	for k := range frames {
		st[k], src[k] = C.int(streams[k]), C.int(sources[k])
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := write(C.int(len(frames)), &st[0], &src[0], ptrs, &lens[0]); rc != 0 {
		return fmt.Errorf("hip: writing %s frames to the windows failed (%d): %s", bank.what, int(rc), lastError())
	}
	return nil
}
