/*
 * bnhip.h — C ABI of libbnhip.so, the MI355X-native (gfx950) BirdNET inference engine.
 *
 * This is the drop-in boundary for birdnet-go's classifier backend seam
 *   internal/inference/backend.go:8-29   (inference.Classifier / EmbeddingExtractor)
 * i.e. exactly what a cgo backend `internal/inference/hip/backend_hip.go` (build tag `hip`) binds,
 * shaped after the reference's own native-accelerator precedent, the OpenVINO cgo shim
 *   internal/inference/openvino/backend_openvino.go:16-413 (C preamble), :443-832 (Go side).
 * Plain pointers and sizes only; no C++/torch types.  All functions return 0 on success or a
 * negative BNHIP_E_* code; bnhip_last_error() returns a thread-local message (the OpenVINO shim
 * keeps thread-local error strings too: backend_openvino.go:100,325).
 *
 * Threading contract (same as the reference's backends, backend.go:7 "NOT goroutine-safe; callers
 * must synchronize"): a bnhip_model may be used by one thread at a time.  Every entry point calls
 * hipSetDevice for the model's device first, so results never depend on the calling thread.  The error TEXT does:
 * bnhip_last_error() is thread-local, so a cgo caller must fetch it on the OS thread that made the failing call -
 * runtime.LockOSThread around call + fetch, exactly as the OpenVINO shim does (backend_openvino.go:480,581,729,805);
 * the Go binding in birdnet-go_amd/go does so.
 * No entry point lets a C++ exception escape: allocation failure is BNHIP_E_NOMEM, anything else BNHIP_E_RUNTIME
 * ("never panic; any failure => fall back", internal/classifier/model_openvino.go:227-230).
 *
 * Where a host-pointer clip entry below says "one device allocation": the parts of a call of 2 MiB and more (clips, streams,
 * images, workspaces) are carved from one allocation; each smaller part is a hipMalloc of its own, which the HIP runtime
 * serves from blocks it keeps, with no driver call.
 */
#ifndef BNHIP_H
#define BNHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bnhip_model bnhip_model;

enum {
    BNHIP_OK = 0,
    BNHIP_E_INVALID = -1,      /* bad argument (NULL, size mismatch) — CategoryValidation */
    BNHIP_E_NO_DEVICE = -2,    /* no usable gfx950 device / HIP runtime — maps to ErrHIPUnavailable */
    BNHIP_E_MODEL = -3,        /* model bytes are not a TFLite flatbuffer / corrupt */
    BNHIP_E_UNSUPPORTED = -4,  /* graph uses an op/pattern the engine does not implement: caller falls back */
    BNHIP_E_RUNTIME = -5,      /* HIP runtime error during alloc/launch/copy */
    BNHIP_E_NOMEM = -6
};

/* Process-global runtime init; idempotent, retryable after failure
 * (replaces InitOV, backend_openvino.go:477-506).  Returns the number of usable devices in
 * *n_devices (nullable). */
int bnhip_init(int* n_devices);

/* Releases process-global state (replaces DestroyOV, backend_openvino.go:512-536). */
void bnhip_shutdown(void);

/* Build a classifier from in-memory model bytes - the same byte slice the reference hands to
 * NewTFLiteClassifier(modelData []byte, ...) (internal/inference/tflite/classifier.go:38), or the bytes of an ONNX file
 * (the reference's ONNX backend takes a path, internal/inference/onnx/classifier.go:268-289; dense heads such as the
 * CustomClassifier / BattyBirdNET regional heads, onnx/custom_classifier.go:148-174, classifier/bat_onnx.go:252-282).  The
 * container is sniffed: "TFL3" at byte 4 = TFLite flatbuffer, otherwise ONNX ModelProto.  The blob is consumed during the
 * call and may be freed afterwards (classifier.go:37).
 * opts_json (nullable): {"device":0,"devices":[0,1,..],"replicate":"auto","max_batch":256,"plan_only":0,"debug_no_reuse":0,
 *                        "autotune":1,"graphs":0,"lanes":2,"frontend_fft":-1,"depth":1,"host_depth":2,"bf16x3":1,
 *                        "precision":"f32","logits_output":0,"embedding_output":1,"tune_dir":"/path"}
 * "devices": one handle over several GPUs: one engine per listed device, the clips of every host-
 *          pointer call are sharded index-contiguously over them and run concurrently (one worker thread per device, own
 *          streams and pinned-order staging per device).  The frozen weights are uploaded to the first device only and
 *          replicated device-to-device: "replicate":"auto" (default) = RCCL ncclBroadcast over xGMI when librccl is loadable
 *          and the devices are distinct, hipMemcpyPeer otherwise; "rccl" / "peer" force one (the same device may be listed
 *          twice with "peer": two shards on one GPU, used by the 1-GPU test of the sharding code).  The device-pointer entry
 *          bnhip_predict_device needs a single-device handle.
 * "tune_dir": directory of recorded create-time tunings (env BNHIP_TUNE_DIR; files <plan key>.tune).  The
 *          create-time tuners choose tiles by timing, so two processes need not agree on every tile; a recorded tuning makes the
 *          plan - and with it a clip's last bits - reproducible.  Inside one process every engine of the same plan (the shards
 *          of a "devices" handle, a second handle on the same model) adopts the first one's decisions whatever this option says.
 *          A file that describes another plan is ignored; BNHIP_TUNE_RECORD=1 writes a missing one after a timed tuning.
 * "plan_only": builds the kernel plan on the CPU without touching a device (info/describe work, predict is rejected).
 * "lanes": batches of >= 32 clips are split over this many concurrent streams inside one call (default 2).
 * "depth": > 1 lets successive bnhip_predict_device calls overlap on alternating contexts (own stream and activation
 *          arena each); their outputs are complete after bnhip_synchronize, not merely in the caller's stream order.
 * "host_depth": 2 (default) runs a host-pointer call of >= 128 clips as a pipeline of chunks over two contexts fed from pinned
 *          staging (csrc/hostpipe.cpp; env BNHIP_HOST_DEPTH): still blocking, outputs complete on return, results
 *          bit-identical to "host_depth":1 (one chunk at a time, round 2's behaviour).  Costs a second activation arena.
 * "frontend_fft": 0 selects the folded-GEMM mel front-end for real-part graphs instead of the FFT path.
 * "bf16x3": pointwise / dense layers on the split-bf16 MFMA path (three exact bf16 pieces per fp32 operand, six
 *          v_mfma_f32_16x16x32_bf16 products per k, fp32 accumulation: every product is reproduced to within 2^-23, see
 *          DESIGN.md): 1 (default) = the layers whose arithmetic intensity at max_batch is >= 12 flop/B (a shape rule, so the
 *          arithmetic never depends on create-time timing; the autotuner only picks tiles), 0 = f32 MFMA only (the Go shim's
 *          Options.StrictF32), 2 = every eligible layer (K >= 16, K a multiple of 4) including the fused expand + depthwise.
 * "logits_output" / "embedding_output": indices of the graph outputs returned as logits / embedding.  Default: the reference's
 *          per-family rule (internal/inference/onnx/detection.go:24-112): output 0 (+ 1 as embedding); 160000-sample graphs
 *          with 4 outputs (Perch v2) logits 3 / embedding 0; with 2 outputs (BirdNET v3.0) the 1280-wide one is the embedding.
 *          Other outputs are not computed.  "embedding_output": -1 = none.
 * "precision": "f32" (default) keeps every product fp32 (f32 MFMA or the six-product split above).  "bf16" rounds the MFMA
 *          operands of the pointwise / dense / fused-expand layers to bf16 (one product per k, fp32 accumulation) and keeps
 *          the expanded tensors between expand, depthwise and projection as bf16 in HBM (everything else fp32 storage;
 *          depthwise, squeeze-excite, front-end and head bias arithmetic stay fp32): the reduced-precision deployment the
 *          reference runs Perch v2 in (openvino f16 drift ~0.08 accepted, openvino_parity_functional_test.go:156-158;
 *          BASELINE configs[4]).  Never a default: BirdNET v2.4 is known not to survive f16 (model_openvino.go:99-103).  */
int bnhip_model_create(const void* blob, size_t n_bytes, const char* opts_json, bnhip_model** out);

/* n_samples: exact input length per clip (tflite/classifier.go:100-104); n_classes: size of the logits
 * output read from the model, not the label list (inference/openvino.go:72-81); emb_dim: 0 when the
 * graph exposes no embedding output (EmbeddingExtractor, backend.go:21-29). */
int bnhip_model_info(const bnhip_model* m, int* n_samples, int* n_classes, int* emb_dim);

/* Classifier.Predict / PredictWithEmbeddings / onnx PredictBatch (onnx/classifier.go:372-430).
 * samples: host float32 [n_clips * n_samples], copied before return (process.go:280-291 contract).
 * logits:  host float32 [n_clips * n_classes] raw pre-activation logits in label order.
 * emb:     nullable host float32 [n_clips * emb_dim].
 * Blocking. */
int bnhip_predict(bnhip_model* m, const float* samples, int n_clips, float* logits, float* emb);

/* Same, with 16-bit little-endian PCM input converted on device: float32(s)/32768
 * (internal/analysis/process.go:479-497, audiocore/convert/pcm.go:226-237). */
int bnhip_predict_pcm16(bnhip_model* m, const int16_t* pcm, int n_clips, float* logits, float* emb);

/* Same for the three bit depths of ConvertToFloat32 (internal/audiocore/convert/pcm.go:206-268): 16-bit /32768,
 * 24-bit packed little-endian with sign extension /8388608, 32-bit /2147483648.  pcm: n_clips * n_samples samples of
 * bits_per_sample / 8 bytes each.  Any other depth is BNHIP_E_INVALID (pcm.go:215-222 "supported_bit_depths 16,24,32"). */
int bnhip_predict_pcm(bnhip_model* m, const void* pcm, int bits_per_sample, int n_clips, float* logits, float* emb);

/* Window assembler: the real-time path's analysis buffers, one per audio source, read in one pass.
 * Replaces, per source, buffer.AnalysisBuffer (internal/audiocore/buffer/analysis.go:30-276: NewAnalysisBuffer :55-145, Write
 * :152-175, Read :187-252, Reset :270-276) and, per tick, the Read() of every (source, model) poll loop
 * (internal/analysis/buffer_manager.go:388-496) - the reference then makes one batch-1 Predict per window behind
 * Orchestrator.inferenceMu (internal/classifier/orchestrator.go:531); here all windows that are ready land in consecutive rows of
 * ONE batch buffer, which is what bnhip_predict_pcm takes (bits_per_sample as captured, n_clips = *n_windows).  The buffer is
 * page-locked when a device is present (*pinned), so the copy engines read the rows in place: a window's bytes move once
 * between the capture callback and the device.
 *   geometry  one assembler per model: overlap_bytes + read_bytes = the model's clip in bytes, overlap = clip / 2
 *             (internal/classifier/model.go:33-56); read_bytes >= overlap_bytes >= 0, read_bytes > 0 (analysis.go:65-90)
 *   write     any thread, any chunk size; overwrite mode - the oldest unread bytes are dropped when the data does not fit
 *             (analysis.go:119 SetOverwrite(true)), the write is counted as an overwrite when len(data) > free bytes (:154)
 *   collect   one thread at a time (writers may run beside it): every source with >= read_bytes buffered yields
 *             `previous tail (zeros the first time) || read_bytes fresh bytes`; at most min(cap, max_batch) windows per call,
 *             the next call resumes behind the last source looked at; sources[k] = source of row k; *batch = the rows, valid
 *             until the next collect / destroy.  A model that is inactive still collects (the audio is consumed, not analysed:
 *             buffer_manager.go:478-481) and simply skips the predict.
 * Needs no device and no bnhip_model.  bnhip_windows_destroy must not run beside any other call on the same assembler (stop the
 * capture callbacks first, as the reference stops its monitors first, RemoveMonitor / RemoveAllMonitors buffer_manager.go:255-292). */
typedef struct bnhip_windows bnhip_windows;
int bnhip_windows_create(size_t overlap_bytes, size_t read_bytes, int max_batch, bnhip_windows** out);
int bnhip_windows_info(const bnhip_windows* w, size_t* window_bytes, int* max_batch, int* pinned, int* n_sources);
/* capacity_bytes >= read_bytes (analysis.go:56-64,91-100); source_id non-empty (:101-109).  Slots of removed sources are reused. */
int bnhip_windows_add_source(bnhip_windows* w, const char* source_id, size_t capacity_bytes, int* out_source);
int bnhip_windows_remove_source(bnhip_windows* w, int source);
int bnhip_windows_write(bnhip_windows* w, int source, const void* data, size_t n_bytes);
int bnhip_windows_collect(bnhip_windows* w, int cap, int* sources, int* n_windows, const void** batch);
int bnhip_windows_ready(const bnhip_windows* w, int* n_ready);
/* writes / overwrites since creation or reset (the OverwriteTracker's inputs, buffer/overwrite.go; the rate window and the
 * notification policy stay with the host), bytes currently buffered.  Any output may be NULL. */
int bnhip_windows_stats(const bnhip_windows* w, int source, uint64_t* writes, uint64_t* overwrites, size_t* buffered_bytes);
int bnhip_windows_reset(bnhip_windows* w, int source);
/* One tick of the real-time path in one call: bnhip_windows_collect + bnhip_predict_pcm_topk, with the rows of chunk c + 1
 * assembled while chunk c is on the device (the host pipeline asks for them where it would otherwise stage caller memory).
 * sources: at least max_batch ints; *n_windows rows were taken (0 = "try again later", nothing is run); out_conf / out_idx:
 * at least max_batch * min(k, n_classes).  overlap_bytes + read_bytes must equal the model's clip at bits_per_sample.  A source
 * that was reset between the readiness pass and its row has sources[r] = -1 and a row of zeros: skip it.  On a device error
 * the listed sources have still given up their window, as the reference's monitor has consumed its window by the time
 * ProcessData fails (buffer_manager.go:494-499). */
int bnhip_windows_predict_topk(bnhip_windows* w, bnhip_model* m, int bits_per_sample, int activation, double sensitivity,
                               int k, int* sources, int* n_windows, float* out_conf, int32_t* out_idx, const void** batch);
void bnhip_windows_destroy(bnhip_windows* w);

/* Page-locked host buffers for the host-pointer entries above.  The reference's accelerator shim keeps a C-allocated input
 * buffer per classifier so that the native side reads memory the Go GC cannot move (backend_openvino.go:673-680); here the same
 * buffer is page-locked as well: when `samples` / `pcm` (and `logits`, `emb`) of a bnhip_predict* call lie in memory from
 * bnhip_host_alloc - detected per call, nothing to flag - the copy engines read and write the caller's buffers directly and the
 * staging pass through the library's own pinned slots is skipped.  Results are bit-identical either way.  Needs bnhip_init. */
int bnhip_host_alloc(size_t n_bytes, void** out);
int bnhip_host_free(void* p);

/* Device-resident variant: all pointers are device memory on the model's device; work is enqueued on
 * the model's stream and NOT synchronised (call bnhip_synchronize). Used by the throughput harness so
 * timing starts with inputs already in HBM.  With "depth" > 1 successive calls run on alternating contexts and may
 * overlap; the caller must not reuse an output (or overwrite an input) of an in-flight call before bnhip_synchronize. */
int bnhip_predict_device(bnhip_model* m, const float* d_samples, int n_clips, float* d_logits, float* d_emb);

/* Post-processing on device for a batch of logits already on the host:
 * conf = float32(1/(1+exp(-sensitivity*float64(x))))  (classifier/analyze.go:113-115,197-208), then
 * top-k by confidence, descending (analyze.go:220-253).  activation: 0 = sigmoid(sensitivity),
 * 1 = softmax (perch_onnx.go:315-335), 2 = plain float32-division sigmoid (onnx/postprocess.go:8-10).
 * out_conf/out_idx: [n_clips * k]. */
int bnhip_postprocess_topk(bnhip_model* m, const float* logits, int n_clips, int n_classes, int activation,
                           double sensitivity, int k, float* out_conf, int32_t* out_idx);

/* Fused convenience: predict + activation + top-k without the logits leaving the device. */
int bnhip_predict_topk(bnhip_model* m, const float* samples, int n_clips, int activation, double sensitivity,
                       int k, float* out_conf, int32_t* out_idx);

/* The same from PCM bytes as captured (bits_per_sample 16 / 24 / 32 as in bnhip_predict_pcm): what (*BirdNET).Predict does for
 * one analysis window - convert (internal/analysis/process.go:479-497) -> classifier -> sigmoid(sensitivity) -> top-10
 * (internal/classifier/analyze.go:25-110) - for n_clips windows in one call; with the rows of bnhip_windows_collect as `pcm`
 * this is one tick of the real-time path.  Neither the float samples nor the logits exist on the host. */
int bnhip_predict_pcm_topk(bnhip_model* m, const void* pcm, int bits_per_sample, int n_clips, int activation,
                           double sensitivity, int k, float* out_conf, int32_t* out_idx);

/* Species occurrence heat-map grid on a range-filter meta-model ([lat, lon, week] -> per-species occurrence): the work of
 * HeatmapInferenceService.ComputeGridWithBinding (internal/classifier/heatmap_service.go:143-420), which the API's heatmap
 * handler runs over up to 50 000 cells x 48 weeks (internal/api/v2/analytics/heatmap.go:30-36; its fallback
 * computeHeatmapGrid, :315-368, keeps one column of Orchestrator.BatchRangeFilterInference, orchestrator.go:1846-1883).
 * coords: host [n_cells][2] lat / lon pairs (cell centres, used exactly as given); result: host [weeks][n_cells] with
 * weeks = ceil(total_weeks / stride).  Row (wi, c) is [coords[2c], coords[2c+1], (float)(1 + wi * stride)] and
 * result[wi * n_cells + c] is its output `species`.  The rows run in chunks of max_batch on the device with no host round trip
 * per chunk.  When the plan ends in an fp32 dense layer that writes the outputs (its folded activation included), that layer
 * computes only column `species` ("heatmap_tail":"pruned" in bnhip_model_describe; within 1e-6 of bnhip_predict's column on
 * sigmoid outputs - a different summation order); otherwise every chunk runs the whole plan and the column is gathered
 * ("gather": bit-identical to bnhip_predict for the same chunk of rows).
 * BNHIP_E_INVALID (nothing written): NULL pointers, n_cells / stride / total_weeks <= 0, species outside [0, n_classes), a model
 * whose input width is not 3, a multi-device or plan-only handle, weeks * n_cells beyond INT_MAX.  A failed call leaves the
 * handle usable.  returns weeks computed (= ceil(total_weeks / stride)) or a negative BNHIP_E_* */
int bnhip_range_heatmap(bnhip_model* m, const float* coords, int n_cells, int species,
                        int stride, int total_weeks, float* result);

/* File analysis: whole recordings in, the result of every overlapping analysis window out, in one call - the reference's `file`
 * and `directory` commands (doc/wiki/file-analysis.md; the windowing is internal/audiocore/buffer/analysis.go:187-251; SURVEY.md
 * section 8 row f1, BASELINE config 1).  The windows are never materialised on the host: every recording goes to the device once,
 * as it is, and the plan's first launch reads each window where it lies.
 *   windows  Host only, needs no device: the framing rule in integers.  A window is n_samples long and window j of a recording
 *            starts at sample j * hop; with remain = length - j * hop it is kept when it is the recording's first, or remain >=
 *            n_samples, or remain >= min_tail, and framing stops when remain <= n_samples (a kept last window is zero-padded).
 *            first_window: [n_recordings + 1], first_window[r] = windows in front of recording r.  returns the total W (>= 1) or
 *            a negative BNHIP_E_*.
 *   pcm_topk pcm: the recordings packed back to back on the host, lengths[r] samples each; bits_per_sample 0 = float32, or 16 /
 *            24 / 32 as in bnhip_predict_pcm.  n_samples is the model's clip.  Window w of the burst (recording r, j = w -
 *            first_window[r]) gives row w of out_conf / out_idx: [W][min(k, n_classes)], what bnhip_predict_pcm_topk answers for the
 *            host-framed window, bit for bit.  One H2D copy per recording, the windows in chunks of max_batch with no host round
 *            trip per chunk, the rows down once.
 *   pcm      The same, then the detection rows: every (window, rank) with confidence >= threshold (a NaN is dropped), ordered by
 *            window, then rank.  *n_out = their total; min(cap, *n_out) rows are written (out may be NULL when cap is 0).
 *            `window` counts inside its recording: it starts at sample window * hop.
 * BNHIP_E_INVALID (nothing written, the handle stays usable): NULL pointers, an unknown bit depth, n_recordings outside 1..65535,
 * a recording without samples, a burst of 2^36 samples or more, hop outside [1, n_samples], a negative min_tail, k <= 0, an
 * unknown activation, a multi-device or plan-only handle, more than INT_MAX windows. */
typedef struct bnhip_detection {
    int32_t recording, window, class_index;
    float confidence;
} bnhip_detection;
long long bnhip_analyze_windows(const int64_t* lengths, int n_recordings, int n_samples, int hop, int64_t min_tail,
                                int64_t* first_window);
int bnhip_analyze_pcm_topk(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                           int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx);
int bnhip_analyze_pcm(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                      int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out,
                      size_t cap, size_t* n_out);

/* File analysis of recordings at their own sample rates and bit depths: a directory of field recordings (32, 44.1, 96, 192, 250,
 * 384 kHz; 16- and 24-bit files side by side) in one call.  The reference resamples file input to the model's rate before analysis
 * (internal/audiocore/resample/resample.go:57-172; call sites analysis/buffer_consumer.go:118,192) and converts the PCM depths as
 * audiocore/convert/pcm.go:206-268; here both happen on the device, between the upload and the framing, and the resampled audio
 * never exists on the host.
 *   recs     One bnhip_recording per recording: length in samples at its own `rate`, bits_per_sample 0 = float32, or 16 / 24 / 32 as
 *            in bnhip_analyze_pcm.  pcm holds recording r in length * bytes-per-sample bytes, directly after recording r - 1.
 *            Recording r becomes n_out[r] = ceil(length * L / M) samples at model_rate (L / M = model_rate / rate in lowest terms:
 *            bnhip_resample_length in 64 bits; equal rates give n_out = length), each the value bnhip_resample_f32 computes from
 *            the recording converted to float32, bit for bit.  hop, min_tail, the model's clip and every `window` of a detection
 *            row count samples at model_rate, and the window table is bnhip_analyze_windows' over n_out.
 *   windows  Host only, needs no device: that table.  n_samples is the window; resampled_length (may be NULL): [n_recordings], the
 *            n_out.  returns the total W (>= 1) or a negative BNHIP_E_*.
 *   pcm_topk / pcm  What bnhip_analyze_pcm_topk / bnhip_analyze_pcm answer for the float32 recordings at model_rate, bit for bit.
 *            One H2D copy per recording, one resample-and-convert launch for the burst, then the same chunks.  A burst whose
 *            recordings are all at model_rate and share one depth IS the bnhip_analyze_pcm call: no second block, no extra launch.
 * BNHIP_E_INVALID (nothing written, the handle stays usable): everything bnhip_analyze_pcm refuses (the 2^36-sample limit holds for
 * the recordings as they come and as they are at model_rate), a rate <= 0, model_rate <= 0, an unknown depth in any recording, a
 * length or an n_out of 2^31 or more.  BNHIP_E_UNSUPPORTED, before any allocation: a rate whose phase table does not fit LDS
 * (as bnhip_resample_f32 answers it); the error text names the recording and both rates. */
typedef struct bnhip_recording {
    int64_t length;
    int32_t rate, bits_per_sample;
} bnhip_recording;
long long bnhip_analyze_mixed_windows(const bnhip_recording* recs, int n_recordings, int model_rate, int n_samples, int hop,
                                      int64_t min_tail, int64_t* first_window, int64_t* resampled_length);
int bnhip_analyze_mixed_pcm_topk(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate,
                                 int hop, int64_t min_tail, int activation, double sensitivity, int k, float* out_conf,
                                 int32_t* out_idx);
int bnhip_analyze_mixed_pcm(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop,
                            int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out,
                            size_t cap, size_t* n_out);

/* File analysis of multichannel recordings: stereo and 4- to 8-channel files as field recorders and microphone arrays write them go
 * to the device interleaved, exactly as they are in a WAV data chunk, and the launch that converts and resamples fetches one channel
 * or the mean of the channels - no de-interleaving pass on the host.  Which one may be left to a measurement made on the device in
 * the same call: the reference's channel policy (internal/audiocore/ffmpeg/analyze.go:157-202: per-channel RMS dBFS; a channel that
 * leads by more than 6 dB is picked, both below -60 dBFS or anything else gives the downmix), restated on exact integer sums.
 *   recs     One bnhip_channels_recording per recording: length in FRAMES (samples per channel) at its own rate, the depth as in
 *            bnhip_recording, channels 1..16, and select: a channel index, BNHIP_CHANNEL_MIX or BNHIP_CHANNEL_AUTO.  pcm holds recording
 *            r as length * channels interleaved samples, directly after recording r - 1.
 *   sample   Channel c: sample n is element n * channels + c, converted as bnhip_analyze_mixed_pcm converts it.  Mix, integer depths:
 *            (float)((double)S / (double)(channels * 2^(bits - 1))), S the exact integer sum of the frame.  Mix, float32: the channels
 *            added in channel order in fp64, divided by (double)channels, rounded to float32.  The result is the recording that the
 *            mixed call then resamples and frames, bit for bit.
 *   auto     Integer depths only.  E[c] = the exact sum of squares of channel c (128 bits), Ed[c] = (double)sum_hi * 2^64 +
 *            (double)sum_lo.  A channel is quiet when Ed[c] < (1073.741824 * 4^(bits - 16)) * (double)length (-60 dBFS).  One channel
 *            gives channel 0; every channel quiet gives the mix; else the channel with the largest Ed (ties: the lower index) is
 *            picked when Ed[top] > 3.9810717055349722 * Ed[second] (6 dB in power), and the mix otherwise.
 *   windows  Host only: the table of bnhip_analyze_mixed_windows over (length, rate); the channels do not enter it.
 *   pcm_topk / pcm  As bnhip_analyze_mixed_pcm_topk / bnhip_analyze_mixed_pcm; chosen (may be NULL): [n_recordings], the channel read
 *            or BNHIP_CHANNEL_MIX.  One H2D copy per recording, the measurement (two launches, only over the recordings that ask for
 *            auto, none when no recording does), one slot launch, then the same chunks.  A burst whose recordings all have one
 *            channel IS the bnhip_analyze_mixed_* call, with that call's own fast path.
 *   bnhip_channel_energy_pcm  The measurement alone, for every recording whatever its select: out [sum of channels], recording-major:
 *            the 128-bit sum of squares of the channel's integer samples and rms_dbfs = 20 log10(rms16 / 32768) with rms16 =
 *            sqrt(E / length) / 2^(bits - 16), -96 when rms16 < 1 (computed on the host); chosen (may be NULL): what
 *            BNHIP_CHANNEL_AUTO picks.
 * BNHIP_E_INVALID (nothing written, the handle stays usable): everything bnhip_analyze_mixed_pcm refuses, channels outside 1..16,
 * select outside its range, auto (or the measurement entry) on a float32 recording, length * channels summed over the burst at 2^36
 * or more, a multi-device or plan-only handle. */
#define BNHIP_CHANNEL_MIX  (-1)
#define BNHIP_CHANNEL_AUTO (-2)
typedef struct bnhip_channels_recording {
    int64_t length;
    int32_t rate, bits_per_sample;
    int32_t channels;
    int32_t select;
} bnhip_channels_recording;
typedef struct bnhip_channel_energy {
    uint64_t sum_lo, sum_hi;
    double rms_dbfs;
} bnhip_channel_energy;
long long bnhip_analyze_channels_windows(const bnhip_channels_recording* recs, int n_recordings, int model_rate, int n_samples, int hop,
                                         int64_t min_tail, int64_t* first_window, int64_t* resampled_length);
int bnhip_analyze_channels_pcm_topk(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                    int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                    float* out_conf, int32_t* out_idx, int32_t* chosen);
int bnhip_analyze_channels_pcm(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                               int hop, int64_t min_tail, int activation, double sensitivity, int k, float threshold,
                               bnhip_detection* out, size_t cap, size_t* n_out, int32_t* chosen);
int bnhip_channel_energy_pcm(int device, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                             bnhip_channel_energy* out, int32_t* chosen);

/* Detection events: the rows of a file-analysis call merged on the device into what a user of the reference sees.  Its processor
 * (internal/analysis/processor/processor.go) tests every result against a per-species threshold (getBaseConfidenceThreshold; the
 * strict test `result.Confidence <= confidenceThreshold` at line 1046; the include / exclude lists), merges repeated hits of one
 * species from one source into a pending detection held for a fixed time (lines 713-786: the best hit is kept, on > only, and the
 * rest are counted), and at the flush discards a detection that matched fewer than minDetections times (shouldDiscardDetection,
 * lines 1485-1495; calculateMinDetectionsFromSettings, lines 1669-1729; false_positive_filter.go:42-59) or began at or before a
 * human voice was heard (lines 1497-1516; handleHumanDetection, lines 1319-1334).  Here the clock is audio time, in windows.
 *   rows     The call's top-k rows (recording r, window w, class c, confidence x), by recording, then window, then rank.
 *   hit      class_veto[c] == 0 and x > class_threshold[c]: float32, strict, false for a NaN on either side - a threshold of +inf or
 *            NaN excludes its class, which is how include / exclude lists and custom thresholds are stated.
 *   veto hit class_veto[c] != 0 and x > veto_threshold: marks window w of recording r (LastHumanDetection).  A veto class forms no
 *            event.  class_veto may be NULL: no veto class.
 *   events   The hits of one (r, c), by window (equal windows in row order; a row given twice is two hits).  The first opens an event
 *            at b = w; every following hit with w < b + hold_windows joins it; the first with w >= b + hold_windows opens the next
 *            event at its own window (FlushDeadline = created + detectionWindow: the hold is fixed from the first hit and does not
 *            slide; extended capture, where it does: "Detection events: extended capture" below).  first_window = b, last_window = the last hit that joined, count = the hits, confidence = the largest, best_window
 *            = the window of the largest (ties: the earliest).
 *   status   1 when count < min_count; else 2 when recording r has a veto hit at a window v with b <= v < b + hold_windows; else 0.
 *            Without BNHIP_EVENTS_KEEP_DROPPED in flags only status-0 events are answered; with it all are, each with its status.
 *   order    Ascending by (recording, class_index, first_window).  *n_out = the events answered; min(cap, *n_out) are written in that
 *            order (out may be NULL when cap is 0).  The same rows give the same bytes on every run.
 *   bnhip_analyze_pcm_events / _mixed_pcm_events / _channels_pcm_events  The arguments of bnhip_analyze_pcm / _mixed_pcm / _channels_pcm
 *            with the threshold replaced by the filter (its tables hold n_classes entries of the model) and the rows by the events:
 *            every non-NaN row of the call stays on the device and the tail runs behind the last chunk - no row crosses PCIe.  The
 *            fast paths of the mixed and channels calls hold as before.
 *   bnhip_detection_events  The tail alone over rows the host holds (kept from an earlier call, or of several calls joined):
 *            nondecreasing in (recording, window), checked on the host in one pass.  n_rows == 0 answers zero events.
 *   bnhip_event_min_count  Host only: calculateMinDetectionsFromSettings - 3.0 s chunk, 6.0 s reference window, segment = max(0.1, 3 -
 *            overlap), shares 0 / 0.20 / 0.30 / 0.50 / 0.60 / 0.70 for levels 0-5 (any other level: 0.30), max(1, ceil(6 / segment *
 *            share - 1e-9)); level 0 gives 1.
 * BNHIP_E_INVALID (nothing written, the handle stays usable, before any device call): everything the sibling entry refuses, a NULL
 * filter or class_threshold, hold_windows < 1, min_count < 1, unknown flag bits, windows * min(k, n_classes) of 2^31 or more; for
 * bnhip_detection_events: n_classes outside 1..38400, a recording outside 0..65534, a negative window, a class outside the table,
 * rows out of order, n_rows of 2^31 or more. */
#define BNHIP_EVENTS_KEEP_DROPPED 1
typedef struct bnhip_event_filter {
    const float* class_threshold;      /* [n_classes] */
    const uint8_t* class_veto;         /* [n_classes] or NULL */
    float veto_threshold;
    int32_t hold_windows, min_count, flags;
} bnhip_event_filter;
typedef struct bnhip_event {           /* 32 bytes */
    int32_t recording, class_index, first_window, last_window, best_window, count;
    float confidence;
    int32_t status;
} bnhip_event;
int bnhip_analyze_pcm_events(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                             int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter,
                             bnhip_event* out, size_t cap, size_t* n_out);
int bnhip_analyze_mixed_pcm_events(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate,
                                   int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                   const bnhip_event_filter* filter, bnhip_event* out, size_t cap, size_t* n_out);
int bnhip_analyze_channels_pcm_events(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                      int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                      const bnhip_event_filter* filter, bnhip_event* out, size_t cap, size_t* n_out,
                                      int32_t* chosen);
int bnhip_detection_events(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter,
                           bnhip_event* out, size_t cap, size_t* n_out);
int bnhip_event_min_count(int level, double overlap_seconds);

/* Detection events: the real-time bank.  The same rule in streaming form, for the reference's product path (processDetections and
 * flushPendingDetections, processor.go:671-804, 1485-1516, 1741-1795): a bank keeps every source's pending detections on the device
 * across calls and is fed the top-k rows of each tick; a call answers the detections that became due in it.  The filter struct, the
 * event struct, hits, veto hits, counts, ties and the statuses are those above.
 *   sources  A bank holds max_sources sources, 0..max_sources-1.  A source's clock is the number of windows the bank has been given
 *            for it since creation or reset; the j-th row of source s in a call, in row order, is window clock[s] + j.  That number is
 *            `window` of the rule above, and the source number is `recording`.
 *   rows     k results (conf, idx) as the top-k entries write them; idx < 0 is no result, and a row of k such entries only advances
 *            the clock (a window that was consumed but not analysed).
 *   events   The first hit of (s, c) with no live event opens one at b = w; a hit with w < b + hold_windows joins it.  After window w
 *            of a source is applied, every live event of it with b + hold_windows <= w + 1 is due: answered in that call, its slot
 *            freed - before window w + 1 is applied, so a hit at exactly b + hold_windows opens the next event.
 *   status   1 when count < min_count; else 2 when the source's largest veto-hit window so far is >= b (an event is flushed right
 *            after window b + hold_windows - 1, so this is b <= v < b + hold_windows of the rule above); else 0.
 *            BNHIP_EVENTS_KEEP_DROPPED as above.
 *   slots    A source has at most one live event per class and opens at most k per window, and an event opened at b is gone after
 *            window b + hold_windows - 1: while window w is applied the live events began in [w - hold_windows + 1, w].  So
 *            slots_per_source = min(k * hold_windows, n_classes) is exact.
 *   order    A call's answer ascends by (source, class_index, first_window): unique within a call, so the same calls give the same
 *            bytes on every run.
 *   bnhip_event_bank_create  Copies the filter's tables; hold_windows and k are fixed for the bank's life.
 *   bnhip_event_bank_set_filter  New thresholds, veto table, veto threshold, min_count and flags from the next call on (settings
 *            reloads; in a dynamic bank - "Detection events: dynamic thresholds" below - the thresholds are the classes' bases); a
 *            different hold_windows is refused.
 *   bnhip_event_bank_process  Rows from host memory.  sources[r] < 0 skips row r; a source may appear several times or not at all.
 *   bnhip_event_bank_process_device  The same with the rows already on the bank's device: enqueued on `stream`, synchronised before
 *            it returns.  A class index outside the table is no result here; the host form refuses it in its one checking pass.
 *   bnhip_event_bank_flush  Answers every live event of `source` (-1: of all) as if the stream had ended, statuses by the same rule;
 *            the clocks stay.  The rows of a recording fed and then flushed answer exactly bnhip_detection_events of those rows.
 *   bnhip_event_bank_reset  Drops the live events of `source` (-1: of all) unanswered, clock 0, veto memory cleared.
 *   bnhip_event_bank_pending  The live events of all sources with status BNHIP_EVENT_PENDING and the fields as they stand, ascending
 *            by (source, class_index); changes nothing (SnapshotVisiblePending, the "currently hearing" list).
 *   bnhip_windows_predict_events  bnhip_windows_predict_topk - the same tick, out_conf / out_idx filled exactly as there - with the
 *            rows also kept on the device and bnhip_event_bank_process_device run behind the last chunk on the model's stream; the
 *            bank's source numbers are the assembler's.  *n_windows == 0 runs nothing and answers no events.  An error before the
 *            bank stage leaves the bank unchanged.  The bank's k is the tick's row width min(k, n_classes); single-device handles.
 *   calls    Every bank call is one transaction: a header copy, the launches, one copy back, and a commit once everything succeeded
 *            (each source's state is a pair of slabs; a launch reads one and writes the other).  A call that fails changes no source.
 *            More events than cap is such a failure: BNHIP_E_INVALID with *n_out = the number needed, nothing written; the same call
 *            with room then succeeds.
 * BNHIP_E_INVALID (before any device call, the handle stays usable): NULL where a pointer is required, max_sources outside 1..65535,
 * n_classes outside 1..38400, k < 1, hold_windows < 1, min_count < 1, k * hold_windows > 4096, unknown flag bits, a source number
 * >= max_sources, n_rows < 0 or n_rows * k of 2^31 or more, a clock that the call would take past 2^31 - 1 (reset the source), a tick
 * whose row width differs from the bank's k, model and bank on different devices, the host form's class index >= n_classes.  In
 * the tick a source number >= max_sources can only be seen once the windows are taken: out_conf / out_idx are filled, the bank is
 * unchanged.  Allocation failure: BNHIP_E_NOMEM. */
#define BNHIP_EVENT_PENDING (-1)
typedef struct bnhip_event_bank bnhip_event_bank;
int bnhip_event_bank_create(int device, int max_sources, int n_classes, int k, const bnhip_event_filter* filter, bnhip_event_bank** out);
int bnhip_event_bank_info(const bnhip_event_bank* b, int* max_sources, int* n_classes, int* k, int* hold_windows, int* slots_per_source);
int bnhip_event_bank_set_filter(bnhip_event_bank* b, const bnhip_event_filter* filter);
int bnhip_event_bank_process(bnhip_event_bank* b, const int32_t* sources, int n_rows, const float* conf, const int32_t* idx,
                             bnhip_event* out, size_t cap, size_t* n_out);
int bnhip_event_bank_process_device(bnhip_event_bank* b, const int32_t* sources, int n_rows, const float* d_conf, const int32_t* d_idx,
                                    bnhip_event* out, size_t cap, size_t* n_out, void* stream);
int bnhip_event_bank_flush(bnhip_event_bank* b, int source, bnhip_event* out, size_t cap, size_t* n_out);
int bnhip_event_bank_reset(bnhip_event_bank* b, int source);
int bnhip_event_bank_pending(bnhip_event_bank* b, bnhip_event* out, size_t cap, size_t* n_out);
int bnhip_event_bank_clock(bnhip_event_bank* b, int source, int64_t* windows);
void bnhip_event_bank_destroy(bnhip_event_bank* b);
int bnhip_windows_predict_events(bnhip_windows* w, bnhip_model* m, bnhip_event_bank* bank, int bits_per_sample, int activation,
                                 double sensitivity, int k, int* sources, int* n_windows, float* out_conf, int32_t* out_idx,
                                 const void** batch, bnhip_event* events, size_t cap, size_t* n_events);

/* Detection events: extended capture.  For the species chosen for it the reference lets every new hit of a pending detection move
 * its flush deadline (applyExtendedCapture and calculateExtendedFlushDeadline, internal/analysis/processor/extended_capture.go:282-329,
 * applied at processor.go:788-790): now + max(normal window, 15 s) while the session is under 30 s, now + 30 s while it is under
 * 2 min, now + 60 s after that, capped at FirstDetected + MaxDuration - a detection is then as long as the bird kept calling.  Both
 * rules above take it as one more struct; the clock stays audio time in windows, and the host turns the reference's seconds into
 * windows as it does for hold_windows, with a ceiling.
 *   deadline An event opened at window b carries a deadline d.  class_extended[c] == 0: d = b + hold_windows, set once - the rule
 *            above.  Otherwise (class_extended NULL: every class) every hit of the event at window w, the one that opens it too, sets
 *            d = min(w + wait(w - b), b + max_windows), with wait(t) = max(hold_windows, short_wait) for t < medium_from,
 *            medium_wait for medium_from <= t < long_from, long_wait for t >= long_from.  The last hit's deadline stands (the
 *            reference overwrites FlushDeadline the same way), so a deadline may also move earlier; it is never before w + 1.
 *   events   A hit at window w joins the live event of its (recording or source, class) while w < d; a hit at w >= d opens the next
 *            event at its own window; equal windows join in row order.  In the bank an event is due after window w' once d <= w' + 1:
 *            answered, its slot freed, before window w' + 1 is applied.
 *   status   1 when count < min_count; else 2 for a veto hit at a window v with b <= v < d, d the event's final deadline (in the
 *            bank still "the largest veto-hit window so far is >= b" at the flush); else 0.
 *   slots    While window w is applied every live event has d >= w + 1 and d <= its last hit + W, W = max(hold_windows, short_wait,
 *            medium_wait, long_wait): its last hit lies in [w - W + 1, w], and a window brings at most k hits.  So slots_per_source =
 *            min(k * W, n_classes) is exact, by the argument of "slots" above; bnhip_event_bank_info reports it.
 *   bnhip_detection_events_extended, bnhip_analyze_channels_pcm_events_extended, bnhip_analyze_channels_pcm_clips_extended (below)
 *            Their namesakes with the extend behind the filter.  class_extended all zero answers the namesake's bytes.  With
 *            bnhip_clip_export.extended a clip then runs to the last hit of an event that may be max_windows long.
 *   bnhip_event_bank_create_extended  bnhip_event_bank_create with the extend: the bank's slots carry their deadlines, and W is
 *            fixed for the bank's life.  process, process_device, flush, pending, reset, clock, set_filter and
 *            bnhip_windows_predict_events take such a bank unchanged.  The rows of a recording fed and then flushed answer exactly
 *            bnhip_detection_events_extended of those rows.
 *   bnhip_event_bank_set_extend  A new table and new numbers from the next call on; a live event keeps its deadline until its next
 *            hit.  NULL turns sliding off (every event opened from then on is held hold_windows).  Refused: a W above the bank's
 *            own, and a bank created without an extend.
 *   bnhip_event_deadline  Host only: d of an event of a sliding class opened at first_window and last hit at window.
 * BNHIP_E_INVALID (before any device call): what the namesake refuses, a NULL extend (but for set_extend), max_windows <
 * hold_windows, a wait below 1, medium_from < 1, long_from < medium_from, k * W > 4096; for bnhip_event_deadline hold_windows < 1,
 * a negative first_window and window < first_window (it answers the negative code). */
typedef struct bnhip_event_extend {
    const uint8_t* class_extended;     /* [n_classes], non-zero: the class slides; NULL: every class does */
    int32_t max_windows;               /* MaxDuration: an event opened at b is due at b + max_windows at the latest */
    int32_t short_wait;                /* 15 s */
    int32_t medium_from, medium_wait;  /* 30 s, 30 s */
    int32_t long_from, long_wait;      /* 2 min, 60 s */
} bnhip_event_extend;
int bnhip_detection_events_extended(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter,
                                    const bnhip_event_extend* extend, bnhip_event* out, size_t cap, size_t* n_out);
int bnhip_analyze_channels_pcm_events_extended(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                               int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                               const bnhip_event_filter* filter, const bnhip_event_extend* extend, bnhip_event* out,
                                               size_t cap, size_t* n_out, int32_t* chosen);
int bnhip_event_bank_create_extended(int device, int max_sources, int n_classes, int k, const bnhip_event_filter* filter,
                                     const bnhip_event_extend* extend, bnhip_event_bank** out);
int bnhip_event_bank_set_extend(bnhip_event_bank* b, const bnhip_event_extend* extend);
int64_t bnhip_event_deadline(int32_t hold_windows, const bnhip_event_extend* extend, int64_t first_window, int64_t window);

/* Detection events: dynamic thresholds.  An approved detection above DynamicThreshold.Trigger lowers that species' threshold to 75 %,
 * 50 % and then 25 % of its base, every later hit above the base keeps the lowered threshold alive, and ValidHours without one
 * resets it (internal/analysis/processor/dynamic_threshold.go; processor.go:794, 1034-1046, 1582-1591).  The reference keys this
 * state modelID:species, so here it is per class and shared by all sources of a bank: it lives on the device beside the sources'
 * slabs, the effective thresholds are derived there at the start of every call, the learning runs behind the emit in the same
 * transaction, and the host is handed the list of threshold changes (the reference's ThresholdEvents).
 *   time     Bank time is an int64 in a unit the host chooses (milliseconds, windows), given by bnhip_event_bank_set_now: host
 *            only, it stands for the calls that follow.  0 <= now < 2^62, never decreasing.  The sources' clocks stay audio time.
 *   settings class_dynamic [n_classes] (non-zero: the class learns; NULL: every class; zero is a species with a custom threshold,
 *            which the reference never adjusts), trigger, min_threshold, valid (ValidHours in bank time, 1..2^61), cooldown
 *            (max(capture length - pre-capture, 5 s) in bank time, 0..2^61).  The base of class c is the filter's
 *            class_threshold[c]: a set_filter with new bases recalculates every effective threshold at the next call
 *            (RecalculateDynamicThresholds).
 *   state    Per class: level L in 0..3, count n >= 0, expires E, learned_at A (-1: never); initially L = n = E = 0, A = -1.  The
 *            state of a class that is not dynamic is kept and ignored.
 *   a call   process, process_device, flush or the tick at time `now`, in this order (pending changes nothing):
 *            1 expiry: a dynamic class with now > E (strict) and n > 0: a record (L -> 0, EXPIRY, confidence 0) when L != 0, then
 *              L = 0, n = 0, A = -1.
 *            2 thr_eff[c] = (float) max((double) base[c] * mult(L), (double) min_threshold) for a dynamic class with L > 0, mult =
 *              0.75 / 0.50 / 0.25; otherwise base[c] bit for bit, NaN and +inf included (they still exclude the class).
 *            3 the bank's rule with thr_eff where class_threshold stood, fixed for the whole call.
 *            4 touch (updateDynamicThreshold): every result (x, c) of the call's counted rows with class_veto[c] == 0, c dynamic,
 *              n > 0 after step 1, x > thr_eff[c] and x > base[c] sets E = now + valid.
 *            5 learn (LearnFromApprovedDetection): of the events that became due in this call with status 0 - whatever cap and
 *              BNHIP_EVENTS_KEEP_DROPPED are - class c is approved high when it is dynamic, x > trigger (strict) and x >= base[c];
 *              X is the largest such x.  Then E = now + valid, and if A < 0 or now - A >= cooldown: n = min(n + 1, INT32_MAX),
 *              A = now, L' = min(n, 3), with a record (L -> L', HIGH_CONFIDENCE, confidence X) when L' != L.  Any number of
 *              sources approving a class in one call is one learning, whatever order they are walked in.
 *            What steps 4 and 5 write is seen by the next call.  A dynamic bank runs steps 1, 2 and 4-5 also in a call that
 *            has no source in it (no counted row, no live source to flush); *n_windows == 0 of the tick stays no call at all.
 *   differs  from the reference: expiry is applied at the start of every call, not lazily at the species' next hit (the thresholds
 *            are the same, the EXPIRY record is earlier); an entry exists exactly when n > 0 (the reference keeps a level-0 entry,
 *            its base clamped to min_threshold, until its periodic clean-up); the clock is what set_now gives; one call is one
 *            instant.
 *   bnhip_event_bank_create_dynamic  bnhip_event_bank_create (extend NULL) or bnhip_event_bank_create_extended with the dynamic.
 *            process, process_device, flush, pending, reset (which leaves the class state alone), clock, set_filter, set_extend and
 *            bnhip_windows_predict_events take such a bank unchanged.  A bank created without one launches what it did before.
 *   bnhip_event_bank_set_dynamic  New settings from the next call on.  NULL turns learning off: thr_eff = base and the state is
 *            frozen, not cleared.
 *   bnhip_event_bank_threshold_changes  The records of the last successful process / flush / tick call, ascending by (class_index,
 *            EXPIRY before HIGH_CONFIDENCE); none after a call that changed nothing.  *n_out = their number; more than cap is
 *            BNHIP_E_INVALID with nothing written.  previous_value / new_value are bnhip_event_threshold at the two levels.
 *   bnhip_event_bank_thresholds  GetDynamicThresholdData: the state as the last successful call left it, dense [n_classes] arrays,
 *            any of them NULL; current = thr_eff of step 2 from that state and the filter in force (the host derives IsActive
 *            from expires and its own now).
 *   bnhip_event_bank_set_thresholds  Restores persisted state (threshold_persistence.go).  Refused unless 0 <= level <= 3, level ==
 *            min(high_count, 3), learned_at >= -1 and expires >= 0 for every class.
 *   bnhip_event_bank_reset_thresholds  ResetDynamicThreshold / ResetAll: class_index (-1: every class) back to the initial state.
 *            bnhip_event_bank_thresholds, _set_thresholds and _reset_thresholds are synchronous: each is a blocking copy of one
 *            slab of the class state (24 bytes per class; _reset_thresholds of one class a copy each way) on the default stream,
 *            which also waits for the process's blocking streams - calls for an API view or a settings change, not for every tick.
 *   bnhip_event_threshold  Host only: thr_eff of a base at a level.
 *   calls    The class state is a pair of slabs with a parity of its own, flipped in the call's commit: a call that fails - more
 *            events than cap too - changes no class, and the same call repeated with room gives the same events, state and changes.
 * BNHIP_E_INVALID (before any device call): what the namesakes refuse, a NULL dynamic at create, a NaN or negative trigger or
 * min_threshold, valid or cooldown out of range, a decreasing or out-of-range now, a level outside 0..3 for bnhip_event_threshold
 * (it answers NaN), and the entries of this section on a bank created without a dynamic. */
#define BNHIP_THRESHOLD_EXPIRY 0
#define BNHIP_THRESHOLD_HIGH_CONFIDENCE 1
typedef struct bnhip_event_dynamic {
    const uint8_t* class_dynamic;      /* [n_classes], non-zero: the class learns; NULL: every class does */
    float trigger;                     /* DynamicThreshold.Trigger */
    float min_threshold;               /* DynamicThreshold.Min */
    int64_t valid;                     /* ValidHours, in bank time */
    int64_t cooldown;                  /* max(capture length - pre-capture, 5 s), in bank time */
} bnhip_event_dynamic;
typedef struct bnhip_threshold_change {
    int32_t class_index, previous_level, new_level, reason;
    float previous_value, new_value, confidence;
    int32_t pad;
} bnhip_threshold_change;
int bnhip_event_bank_create_dynamic(int device, int max_sources, int n_classes, int k, const bnhip_event_filter* filter,
                                    const bnhip_event_extend* extend /* may be NULL */, const bnhip_event_dynamic* dynamic,
                                    bnhip_event_bank** out);
int bnhip_event_bank_set_dynamic(bnhip_event_bank* b, const bnhip_event_dynamic* dynamic);
int bnhip_event_bank_set_now(bnhip_event_bank* b, int64_t now);
int bnhip_event_bank_threshold_changes(bnhip_event_bank* b, bnhip_threshold_change* out, size_t cap, size_t* n_out);
int bnhip_event_bank_thresholds(bnhip_event_bank* b, int32_t* level, int32_t* high_count, int64_t* expires, int64_t* learned_at,
                                float* current);
int bnhip_event_bank_set_thresholds(bnhip_event_bank* b, const int32_t* level, const int32_t* high_count, const int64_t* expires,
                                    const int64_t* learned_at);
int bnhip_event_bank_reset_thresholds(bnhip_event_bank* b, int class_index);
float bnhip_event_threshold(float base, int level, float min_threshold);

/* Detection events: dog-bark and daylight filters.  The reference's shouldDiscardDetection (processor.go:1485-1566) runs four tests
 * at the flush, in this order: the minimum count, the privacy filter, the dog-bark filter (dogbarkfilter.go:15-27, marked at
 * processor.go:1302-1314) and the daylight filter (daylight_filter.go:104-160).  The first two are the rules above; the guards are
 * the other two, taken by both rules as one more struct, so that status 0 means approved by every test of the flush.  The clock
 * stays audio time in windows; the host turns DogBarkFilter.Remember (minutes) into windows as it does for hold_windows, with a
 * ceiling, and the sun times (its own suncalc: the device gets intervals, not a location) into spans of windows.
 *   dog hit  A result (x, c) with class_dog[c] != 0 and x > dog_threshold: float32, strict, false for a NaN on either side.  It marks
 *            window w of its recording or source (LastDogDetection).  Marking does not look at class_threshold and does not stop the
 *            result from being an ordinary hit - the dog class is a class like any other and may form events of its own; a class
 *            that is also a veto class still forms none.  class_dog NULL: no dog class.
 *   status 3 BNHIP_EVENT_DOG ("recent dog bark"): class_dog_filtered[c] != 0 and the recording or source has a dog hit at a window
 *            v < d with d - v <= dog_remember_windows, d the event's final deadline (b + hold_windows, or the sliding one of extended
 *            capture).  Only the largest such v matters, and it may lie before b.  A recording or source without a dog hit drops
 *            nothing.  The reference flushes at the deadline, so its time.Since(lastDogBark) is the distance from the bark to d;
 *            measuring from d - this project's choice - is also what makes an early bnhip_event_bank_flush and the file tail agree.
 *   status 4 BNHIP_EVENT_DAYLIGHT: class_daylight[c] != 0 and first_window lies in a daylight span [from, to) of its recording or
 *            source (FirstDetected in [CivilDawn + offset, CivilDusk - offset)).  No span - an inverted or unknown window of the
 *            reference - is no daylight: the filter fails open.
 *   order    1 (count), then 2 (veto), then 3, then 4: the first that applies is the status.  BNHIP_EVENTS_KEEP_DROPPED answers 3
 *            and 4 like 1 and 2; without it only status 0 is answered.
 *   spans    File tail: daylight_spans [n_spans][3] = (recording, from, to), ascending by (recording, from), disjoint within a
 *            recording, 0 <= from < to, n_spans <= 2^20.  Bank: bnhip_event_bank_set_daylight(bank, source, spans [n][2] = (from, to),
 *            n) with at most BNHIP_EVENT_DAYLIGHT_SPANS per source, in that source's clock; the struct's daylight_spans / n_spans are
 *            not read by a bank.  It is a setting, valid from the next call on and read at the flush: the spans have to cover the
 *            first windows of the events that are still live.  source -1 is allowed with n == 0 only and clears every source.
 *   bnhip_detection_events_guarded, bnhip_analyze_channels_pcm_events_guarded, bnhip_analyze_channels_pcm_clips_guarded  Their
 *            _extended namesakes with the guards behind the extend, which may be NULL here (no class slides).  Guards whose three
 *            tables are NULL or all zero, and no spans, answer the namesake's bytes.  The clip export cuts status-0 events only, as
 *            before.
 *   bnhip_event_bank_set_guards  On any bank - plain, extended or dynamic - from the next call on; NULL turns the guards off.
 *            process, process_device, flush, pending (still status -1) and bnhip_windows_predict_events carry the rule unchanged.
 *            The dog window of a source is recorded only while guards with a class_dog table are set (the reference marks only
 *            while the filter is enabled); it lives in the source's slab, so a failed call leaves it as it was, and it survives a
 *            flush and set_guards(NULL).  bnhip_event_bank_reset of a source clears its dog window and its daylight spans: its
 *            clock returns to 0.  The rows of a recording fed and then flushed answer exactly bnhip_detection_events_guarded of
 *            those rows when the source's spans are the recording's.  In a dynamic bank an event with status 3 or 4 does not learn
 *            (processApprovedDetection is never reached); the touch of rows is not affected.  A bank that never had guards set
 *            runs exactly the launches and copies it ran before.
 * BNHIP_E_INVALID (before any device call, nothing written, the handle stays usable): what the namesake refuses, NULL guards on the
 * _guarded entries, dog_remember_windows < 0, n_spans < 0 or above 2^20, NULL daylight_spans with n_spans > 0, spans out of order,
 * overlapping, empty or negative, a span's recording outside the call (outside 0..65534 for bnhip_detection_events_guarded), more
 * than BNHIP_EVENT_DAYLIGHT_SPANS spans in a bank call, a source outside the bank, source -1 with n != 0. */
#define BNHIP_EVENT_DOG 3
#define BNHIP_EVENT_DAYLIGHT 4
#define BNHIP_EVENT_DAYLIGHT_SPANS 8
typedef struct bnhip_event_guards {
    const uint8_t* class_dog;          /* [n_classes], non-zero: a dog class; NULL: none */
    const uint8_t* class_dog_filtered; /* [n_classes], non-zero: a species the bark suppresses (DogBarkFilter.Species); NULL: none */
    const uint8_t* class_daylight;     /* [n_classes], non-zero: a species dropped in daylight (DaylightFilter.Species); NULL: none */
    const int32_t* daylight_spans;     /* [n_spans][3] (recording, from, to): the file tail's; NULL with n_spans == 0 */
    float dog_threshold;               /* DogBarkFilter.Confidence: a dog result must exceed it */
    int32_t dog_remember_windows;      /* DogBarkFilter.Remember, >= 0 */
    int32_t n_spans;
    int32_t reserved;
} bnhip_event_guards;
int bnhip_detection_events_guarded(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter,
                                   const bnhip_event_extend* extend /* may be NULL */, const bnhip_event_guards* guards, bnhip_event* out,
                                   size_t cap, size_t* n_out);
int bnhip_analyze_channels_pcm_events_guarded(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                              int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                              const bnhip_event_filter* filter, const bnhip_event_extend* extend /* may be NULL */,
                                              const bnhip_event_guards* guards, bnhip_event* out, size_t cap, size_t* n_out,
                                              int32_t* chosen);
int bnhip_event_bank_set_guards(bnhip_event_bank* b, const bnhip_event_guards* guards /* NULL: off */);
int bnhip_event_bank_set_daylight(bnhip_event_bank* b, int source, const int32_t* spans /* [n][2] */, int n);

/* Detection clips: what the reference saves for every approved detection, made from the recordings of a file-analysis call while
 * they are still on the device.  Its processor takes the audio from BeginTime back by the pre-capture to the end of the capture
 * window, or under extended capture to as long as the bird kept calling (internal/analysis/processor/extended_capture.go:232-280,
 * processor.go:1105-1110, 2234-2300), loudness-normalises the clip, encodes it and renders its spectrogram.  Here the clock is
 * audio time, in samples at the model's rate.
 *   span     Of event e of recording r, N = resampled_length[r]: begin = first_window * hop - pre_samples, end = (extended ?
 *            last_window : first_window) * hop + post_samples (post_samples: captureLength - preCaptureLength), both clamped to
 *            [0, N], then end = min(end, begin + max_samples).  start = begin, length = end - begin >= 1; an event with status != 0
 *            gets length 0: no clip.
 *   bnhip_event_clip_spans  Host only: the rule over events the caller holds; spans [n_events].
 *   clip     Sample i of a span is q = clamp(rint(x * 32768), -32768, 32767), x the float32 that the windows of the call are framed
 *            from (the sample of a 16 / 24 / 32-bit recording at the model's rate, else what the device resampler and the channel
 *            fetch wrote); ties to even, a NaN gives 0.  A 16-bit recording's clip is its own samples.  Mono int16, packed back to
 *            back in span order: the layout of "Ragged bursts".
 *   bnhip_recording_clips_pcm16  The cut alone: the upload, channel fetch / measurement and slot launch of bnhip_analyze_channels_pcm
 *            (mono recordings of one depth at the model's rate are cut as they are), then one launch.  Spans of length 0 are skipped;
 *            out_pcm holds the others, the sum of their lengths in samples.
 *   bnhip_analyze_channels_pcm_clips  bnhip_analyze_channels_pcm_events, and behind it, in the same call: the spans of the events
 *            written, the cut, and on the clips where they lie bnhip_loudness_ragged_normalize_device (with normalize != 0),
 *            bnhip_flac_ragged_encode_device at lpc_order over the gained clips, and with width > 0 the render of
 *            bnhip_spectrogram_png_ragged_pcm16 (rate_in = model_rate) over them.  The recordings go up once and no PCM comes back.
 *            With normalize == 0 the streams are those of bnhip_flac_ragged_encode_pcm16 without factors and loudness is not written.
 *   out      events [event_cap]: as bnhip_analyze_channels_pcm_events writes them, n_events the total.  spans, loudness: [event_cap];
 *            flac_offsets, png_offsets: [event_cap + 1] (png, png_offsets, palette: only with width > 0).  spans[i] belongs to
 *            events[i]; clip j is the j-th span of non-zero length, its streams flac[flac_offsets[j] .. flac_offsets[j + 1]) and
 *            png[png_offsets[j] ..), its record loudness[j].
 *   n_clips  The largest n with n <= the events written, n <= 65535, bnhip_flac_ragged_max_bytes(n, lens, seek_interval) <= flac_cap
 *            and, with width > 0, bnhip_png_max_bytes(n, width, height) <= png_cap.  With n_clips == 0 nothing but events, spans,
 *            n_events and n_clips is written, and the second phase touches no device.
 * BNHIP_E_INVALID (nothing written, before any device call): everything the events entry refuses, NULL arguments, pre_samples < 0,
 * post_samples < 1, max_samples < 1, BNHIP_EVENTS_KEEP_DROPPED, what the normalise, FLAC and render entries refuse of their own
 * settings; for bnhip_event_clip_spans an event's recording outside the table; for bnhip_recording_clips_pcm16 n_spans outside
 * 1..65535, a span outside its recording, a negative length, a total of 2^36 samples or more. */
typedef struct bnhip_clip_span {       /* 16 bytes */
    int64_t start;
    int32_t length, recording;
} bnhip_clip_span;
typedef struct bnhip_clip_export {
    int32_t pre_samples, post_samples, max_samples, extended;
    int32_t normalize, gate_fallback;
    double target_lufs, true_peak_dbtp, max_gain_db;
    int32_t seek_interval, lpc_order;
    int32_t width, height, rate_out, reserved;     /* width 0: no images */
    const double* window;                          /* [2 (height - 1)] or NULL: periodic Hann */
    double top_db, range_db;
    const uint8_t* palette;                        /* [768] */
} bnhip_clip_export;
typedef struct bnhip_clips_out {
    bnhip_event* events;
    size_t event_cap, n_events;
    bnhip_clip_span* spans;
    struct bnhip_loudness* loudness;               /* (declared under "Clip loudness" below) */
    uint8_t* flac;
    size_t flac_cap;
    uint64_t* flac_offsets;
    uint8_t* png;
    size_t png_cap;
    uint64_t* png_offsets;
    size_t n_clips;
} bnhip_clips_out;
int bnhip_event_clip_spans(const bnhip_event* events, size_t n_events, const int64_t* resampled_length, int n_recordings, int hop,
                           const bnhip_clip_export* x, bnhip_clip_span* spans);
int bnhip_recording_clips_pcm16(int device, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                const bnhip_clip_span* spans, int n_spans, int16_t* out_pcm);
int bnhip_analyze_channels_pcm_clips(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                     int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                     const bnhip_event_filter* filter, int32_t* chosen, const bnhip_clip_export* x,
                                     bnhip_clips_out* out);
/* ... under extended capture ("Detection events: extended capture") */
int bnhip_analyze_channels_pcm_clips_extended(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                              int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                              const bnhip_event_filter* filter, const bnhip_event_extend* extend, int32_t* chosen,
                                              const bnhip_clip_export* x, bnhip_clips_out* out);
/* ... under the guards ("Detection events: dog-bark and daylight filters"); extend may be NULL */
int bnhip_analyze_channels_pcm_clips_guarded(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                             int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                             const bnhip_event_filter* filter, const bnhip_event_extend* extend,
                                             const bnhip_event_guards* guards, int32_t* chosen, const bnhip_clip_export* x,
                                             bnhip_clips_out* out);

/* Capture bank: the real-time path's detection clips.  The reference keeps a CaptureBuffer per source - a circular PCM buffer with a
 * monotonic byte counter, from which ReadSegment cuts a detection's audio (internal/audiocore/buffer/capture.go:60-112, 132-179,
 * 198-330).  A bank keeps every source's ring on the device: a source's audio goes up once per tick, and a due detection is answered
 * as finished FLAC and PNG bytes, as on the file path.  No PCM comes back.
 *   rings    max_sources rings of mono int16 at one sample rate, all allocated at create: max_sources * capacity * 2 bytes of device
 *            memory (2.95 GB for 256 sources of 120 s at 48 kHz).  capacity_samples is rounded up to a multiple of 1024 samples (the
 *            reference aligns to 2048 bytes: the same); bnhip_capture_bank_info answers the rounded value.
 *   clock    Audio time: written[s] is the number of samples ever given for source s since create or reset, and the sample at
 *            position P of that clock lies in the ring for as long as oldest[s] <= P < written[s], oldest[s] = max(0, written[s] -
 *            capacity, floor[s]) (floor: "a failed write" below).  A write longer than the ring counts in full although only its
 *            last `capacity` samples are stored - unlike the reference, whose counter advances by the stored tail only
 *            (capture.go:148-152, 162), so that positions behind such a write no longer are audio time there.
 *   bnhip_capture_bank_positions  written [max_sources], oldest [max_sources].
 *   bnhip_capture_bank_reset  Source `source` (-1: all) starts again: written 0, floor 0.  Host work only.
 *   bnhip_capture_bank_write  One call per tick for every source: frame f is n_samples[f] samples of bits_per_sample (16, 24 or 32,
 *            little endian, packed) for source sources[f].  A source may appear several times; its frames are appended in call order.
 *            A sample is stored as q = clamp(rint(x * 32768), -32768, 32767), x the float32 of "Detection clips" above: a 16-bit
 *            sample as itself.  If a source's frames of one call total more than the ring, its last `capacity` samples are stored.
 *            One staging copy, one launch, one synchronise, then the commit: written[s] += the source's total.
 *   a failed write  The rings are too large to keep twice, so a write that fails on the device leaves written as it was and
 *            raises floor[s] of every source of the call to written[s] + total[s] - capacity where that is positive: no later read
 *            returns a cell the failed launch may have touched.
 *   bnhip_capture_bank_read_pcm16  The cut alone.  spans: bnhip_clip_span with `recording` the source and `start` a position on its
 *            clock; every span of non-zero length must lie in [oldest, written) of its source.  Spans of length 0 are skipped;
 *            out_pcm holds the others packed back to back, as bnhip_recording_clips_pcm16 does.
 *   bnhip_capture_bank_clips  The cut, then exactly the second phase of bnhip_analyze_channels_pcm_clips over the clips where they
 *            lie: the normalise (with normalize != 0), the FLAC encode at lpc_order, and with width > 0 the render and PNG encode;
 *            rate_in is the bank's rate.  The same n_clips rule over the spans, the same records and offsets.  out->events is not
 *            used (event_cap 0 is allowed); out->spans [n_spans] receives the spans as given; loudness [n_spans], flac_offsets /
 *            png_offsets [n_spans + 1].
 *   bnhip_capture_spans  Host only, no bank: bnhip_event_clip_spans on a running clock.  hop: capture samples per window step;
 *            origins[s] (NULL: 0): the position of window 0's first sample, which may be negative - the window assembler's first
 *            window begins with its overlap of zeros, so a host that feeds both from one stream passes -overlap_samples.  For
 *            event e of source s = e.recording: P0 = origins[s] + first_window * hop - pre_samples, P1 = origins[s] + (extended ?
 *            last_window : first_window) * hop + post_samples, start = max(P0, oldest[s]), and in this order: e.status != 0 ->
 *            BNHIP_CAPTURE_DROPPED; P1 > written[s] -> BNHIP_CAPTURE_NOT_YET (the end is never cut short - capture.go:265-293:
 *            insufficient data is an error, not a shorter clip - the host asks again after a later write); start >= P1 ->
 *            BNHIP_CAPTURE_GONE; each of these with length 0.  Else length = min(P1, start + max_samples) - start, and the status
 *            is BNHIP_CAPTURE_CLAMPED when start > P0 (capture.go:222-228), else BNHIP_CAPTURE_OK.  spans, status: [n_events].
 *   calls    Every bank call holds the bank's lock and has synchronised before it returns.  The same calls give the same bytes on
 *            every run.  Single-device handles.
 * BNHIP_E_INVALID (before any device call, the handle stays usable): NULL where a pointer is required, max_sources outside 1..65535,
 * capacity_samples outside 1..2^31 - 1024, rate outside 1..1048575, bits_per_sample not 16, 24 or 32, a source outside the bank, a
 * negative frame or span length, n_spans outside 1..65535, a span outside [oldest, written), a total of 2^36 samples or more, what
 * bnhip_analyze_channels_pcm_clips refuses of its export settings; for bnhip_capture_spans what bnhip_event_clip_spans refuses and
 * an event's source outside n_sources.  Allocation failure: BNHIP_E_NOMEM. */
#define BNHIP_CAPTURE_OK 0
#define BNHIP_CAPTURE_CLAMPED 1
#define BNHIP_CAPTURE_NOT_YET 2
#define BNHIP_CAPTURE_GONE 3
#define BNHIP_CAPTURE_DROPPED 4
typedef struct bnhip_capture_bank bnhip_capture_bank;
int bnhip_capture_bank_create(int device, int max_sources, int64_t capacity_samples, int rate, bnhip_capture_bank** out);
int bnhip_capture_bank_info(const bnhip_capture_bank* b, int* max_sources, int64_t* capacity_samples, int* rate);
int bnhip_capture_bank_positions(bnhip_capture_bank* b, int64_t* written, int64_t* oldest);
int bnhip_capture_bank_reset(bnhip_capture_bank* b, int source);
int bnhip_capture_bank_write(bnhip_capture_bank* b, int n_frames, const int32_t* sources, const int64_t* n_samples,
                             const void* const* frames, int bits_per_sample);
int bnhip_capture_bank_read_pcm16(bnhip_capture_bank* b, const bnhip_clip_span* spans, int n_spans, int16_t* out_pcm);
int bnhip_capture_bank_clips(bnhip_capture_bank* b, const bnhip_clip_span* spans, int n_spans, const bnhip_clip_export* x,
                             bnhip_clips_out* out);
void bnhip_capture_bank_destroy(bnhip_capture_bank* b);
int bnhip_capture_spans(const bnhip_event* events, size_t n_events, int n_sources, const int64_t* written, const int64_t* oldest,
                        const int64_t* origins, int hop, const bnhip_clip_export* x, bnhip_clip_span* spans, int32_t* status);

/* Ultrasonic frame-CV filter (internal/audiocore/ultrasonic/filter.go:20-66), float64 throughout.
 * samples: host float64 [n_clips * n] (int16/32768 as float64, convert/pcm.go:108-113).
 * cv/ok: [n_clips]. device: HIP device ordinal. */
int bnhip_us_frame_cv(int device, const double* samples, int n_clips, int n, int sample_rate, int fft_size,
                      int hop, int split_hz, double* cv, int32_t* ok);

/* Device-resident form of the same filter for batched pipelines (BASELINE config 4: 256 kHz bat material): d_samples is
 * float64 [n_clips * n] or, with pcm16 != 0, raw int16 PCM converted in the kernel as int16 / 32768 in float64
 * (convert/pcm.go:108-113); d_scratch is float64 [n_clips * frames] (frames = 1 + (n - fft_size) / hop), d_cv float64
 * [n_clips].  Enqueued on hip_stream (NULL = default stream), not synchronised.  Returns the frame count (> 0) or a
 * negative error; geometries the filter's guards reject (filter.go:21-37) are BNHIP_E_INVALID here. */
int bnhip_us_frame_cv_device(int device, const void* d_samples, int pcm16, int n_clips, int n, int sample_rate, int fft_size,
                             int hop, int split_hz, double* d_scratch, double* d_cv, void* hip_stream);

/* Detection-clip spectrogram images: what GenerateFromPCM (internal/spectrogram/generator.go:425-530) gets from a
 * `sox ... rate 24k spectrogram -x W -y H -z R -r` child process per clip, for a batch of clips of one length in one call.
 * sox is not in the reference's tree: the pixel values follow this project's own rendering spec (restated in
 * float64 by tests/specref.py) and are NOT pinned against sox.  Raw images only (no axes, no legend), mono.
 *   N = 2 (height - 1) is the transform length; K = max(1, ceil(n / (width N))) frames are averaged per column; frame (c, k) is
 *   centred at sample floor((2 (c K + k) + 1) n / (2 K width)), zero outside the clip; x = pcm / 32768 (or the float sample);
 *   P[b] = mean over k of |sum_i w[i] x[i] e^(-2 pi i b i / N)|^2 (2 / sum w)^2 (a full-scale sine peaks at 0 dB);
 *   v = (10 log10 P - top_db + range_db) / range_db * 255; the index is 0 for v <= 0 or P = 0, 255 for v >= 255, else floor(v + 0.5).
 *   image: uint8 [n_clips][height][width], row r = bin height - 1 - r (Nyquist on top).  All arithmetic is float64.
 * window: host table of N doubles, NULL = periodic Hann 0.5 - 0.5 cos(2 pi i / N); uploaded tables are cached per (device, N, contents).
 * size:   height = fftFriendlyHeight(width) (generator.go:115-123) and fft_size = N for a width in 1..4096.
 * pcm16:  host PCM in, host image out: one device allocation, one H2D copy, the kernels, one D2H copy, one synchronise.  rate_out == 0
 *         or == rate_in renders at the source rate; otherwise the clips first pass through the one-shot resampler on the device (int16 in, float32 out,
 *         the bnhip_resample_length(n, ...) samples bnhip_resample_f32 gives) - 24 000 Hz for the bird profile, 256 000 Hz for the bat
 *         profile (frequency_profile.go:13-16) - and nothing returns to the host in between.
 * device: d_samples (int16, or float32 with f32 != 0) and d_image are device memory; enqueued on hip_stream (NULL = default
 *         stream), not synchronised.
 * BNHIP_E_INVALID: NULL / empty arguments, n < 1, n_clips > 65535, width outside 1..4096, a height that is not 2^k + 1, a non-finite
 * top_db or range_db, range_db <= 0, non-finite window coefficients or a window that sums to zero.  BNHIP_E_UNSUPPORTED: N outside
 * 64..4096, a rate pair whose resampler geometry does not fit LDS.  Argument errors are answered before any device is touched. */
int bnhip_spectrogram_size(int width, int* height, int* fft_size);
int bnhip_spectrogram_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate_in, int rate_out,
                            int width, int height, const double* window, double top_db, double range_db,
                            uint8_t* image);
int bnhip_spectrogram_device(int device, const void* d_samples, int f32, int n_clips, int n, int width, int height,
                             const double* window, double top_db, double range_db, uint8_t* d_image, void* hip_stream);

/* Spectrogram PNG files: the 8-bit indexed PNG that GenerateFromPCM (internal/spectrogram/generator.go:425-530) finds at its output path
 * after the `sox ... spectrogram -r -o <path>` child, for a batch of width x height index images of one size in one call.  The
 * streams are this project's own deterministic encoder (DESIGN.md §9 "PNG", restated by tests/pngref.py): valid PNG (ISO/IEC 15948)
 * around one zlib (RFC 1950) DEFLATE (RFC 1951) stream per image, integer arithmetic throughout, so every byte is pinned; libpng's or
 * sox's bytes are not a goal.  Per image: signature, IHDR (bit depth 8, colour type 3, no interlace), PLTE (256 entries), one IDAT
 * chunk per band of ceil(16384 / (width + 1)) rows (filter type 0 on every row), IEND.  A band is, of an all-zero band's fixed-Huffman
 * block, a literals-only dynamic-Huffman block and a stored block, the first that applies and is strictly smaller than stored.
 *   images:  uint8 [n_images][height][width]; palette: HOST table uint8 [768] = 256 x (r, g, b) in every entry, the device one included.
 *   out:     the streams back to back; offsets: uint64 [n_images + 1], image i is out[offsets[i] .. offsets[i + 1]).
 *   max_bytes: the all-stored bound of n_images streams - what out_cap must be at least; workspace_size: the device scratch of
 *            encode_device (256-byte aligned).
 * encode_device: d_images, d_out, d_offsets and d_workspace are device memory; enqueued on hip_stream (NULL = default stream), not
 *            synchronised, nothing allocated.
 * encode_u8: host images in, host streams out: one H2D copy, the kernels, a D2H copy of the offsets and then of exactly
 *            offsets[n_images] bytes; one device allocation.
 * bnhip_spectrogram_png_pcm16: bnhip_spectrogram_pcm16 and bnhip_png_encode_u8 in one call - the indices never leave the device, and
 *            each stream decodes to exactly the image bnhip_spectrogram_pcm16 returns; its arguments and limits are that entry's.
 * width and height 1..4096, n_images 1..65535.  BNHIP_E_INVALID: NULL arguments, sizes outside those ranges, out_cap below
 * bnhip_png_max_bytes, a workspace that is too small or not 256-byte aligned.  Argument errors are answered before any device is touched. */
int bnhip_png_max_bytes(int n_images, int width, int height, size_t* bytes);
int bnhip_png_workspace_size(int n_images, int width, int height, size_t* bytes);
int bnhip_png_encode_device(int device, const uint8_t* d_images, int n_images, int width, int height, const uint8_t* palette,
                            uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace, size_t workspace_bytes,
                            void* hip_stream);
int bnhip_png_encode_u8(int device, const uint8_t* images, int n_images, int width, int height, const uint8_t* palette,
                        uint8_t* out, size_t out_cap, uint64_t* offsets);
int bnhip_spectrogram_png_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate_in, int rate_out, int width, int height,
                                const double* window, double top_db, double range_db, const uint8_t* palette,
                                uint8_t* out, size_t out_cap, uint64_t* offsets);

/* Clip loudness: the EBU R 128 normalisation every exported clip and every BirdWeather upload gets (internal/audiocore/audionorm,
 * internal/audiocore/pcmgain; the export plan with its gate fallback, analysis/processor/actions_database.go:1285-1438; the upload
 * plan, birdweather/encode_native.go:25-66), for a batch of mono int16 clips of one length in one call.  The numbers follow the
 * spec of DESIGN.md §9 (restated in float64 by tests/loudref.py): the reference's float32 coefficients, its recurrence, gates,
 * true-peak taps, plan and saturating gain, evaluated in float64 with every operation rounded.
 *   x = pcm / 32768;  S = floor(0.1 rate + 0.5) samples per sub-block;  E[k] = sum of y^2 over sub-block k of the K-weighted
 *   signal y (the trailing n - floor(n / S) S samples add nothing);  z[j] = (E[j] + .. + E[j+3]) / (4 S);  absolute gate
 *   z > (float)10^(-6.9309), relative gate z > 0.1f * the absolute-gated mean;  integrated_lufs = -0.691 + 10 log10(mean of the
 *   gated z), -inf with no gated block;  true_peak = max(|x|, |4 x 32-tap polyphase interpolation of x|) over n + 16 positions;
 *   true_peak_dbtp = 20 log10(true_peak), -inf for 0.
 *   plan: target_gain_db = target_lufs - integrated_lufs, limited to true_peak_dbtp's headroom under the ceiling (PEAK_LIMITED);
 *   nothing for -inf.  With gate_fallback != 0 a clip of -inf loudness and a non-zero peak is lifted by lift_db =
 *   min(ceiling - true_peak_dbtp, target + 70) (GATE_LIFTED), the lifted int16 clip is measured on the device and planned again:
 *   planned_gain_db = lift_db + that plan's gain (target_gain_db and PEAK_LIMITED are then that plan's), or lift_db when it is
 *   still under the gate.  gain_db = planned_gain_db clamped to +-|max_gain_db| (CLAMPED; +inf = no clamp); factor = 1 exactly
 *   at 0 dB, else pow(10, gain_db / 20); output = (double)pcm * factor rounded half away from zero, saturated to int16.
 *   output_lufs = the loudness the plan used (the lifted clip's for a lifted clip) + gain_db - lift_db, -inf when that is -inf.
 *   integrated_lufs, true_peak_dbtp and true_peak always describe the clip as given.
 * The reference's callers pass (60, gate_fallback 1) for an export and (30, 0) for an upload.
 * measure:   measurements only (the plan fields are 0, factor 1, output_lufs = integrated_lufs); sub_energy (nullable) receives
 *            E as [n_clips][n / S] doubles.
 * normalize: out_pcm NULL = plan only.  pcm16: host memory in and out: one device allocation, one H2D copy, the kernels, one D2H
 *            copy of the results and of the output, one synchronise.
 * device:    d_pcm, d_out_pcm (nullable), d_out and d_workspace are device memory, d_workspace at least
 *            bnhip_loudness_workspace_size bytes and 256-byte aligned; enqueued on hip_stream (NULL = default stream), not
 *            synchronised; the workspace is in use until the enqueued work has run.
 * BNHIP_E_INVALID: NULL / empty arguments, rate < 8000, n < 1, n_clips outside 1..65535, a target that is not finite or outside
 * (-70, 0), a ceiling that is not finite or > 0, a NaN max_gain_db, a workspace that is too small.  There is no multi-channel or
 * float entry (conf.NumChannels is 1, nativeNormalizationBitDepth 16): the bindings answer BNHIP_E_UNSUPPORTED for them.  Argument errors are answered before
 * any device is touched.  Divergences: float64 where the reference's meter is float32 (distance measured in DESIGN.md §9); the
 * reference's two SIMD sums have no pinned order; libm's tan / pow / sin / log10 may differ from Go's in the last ulp. */
enum { BNHIP_LOUDNESS_PEAK_LIMITED = 1, BNHIP_LOUDNESS_GATE_LIFTED = 2, BNHIP_LOUDNESS_CLAMPED = 4 };
typedef struct bnhip_loudness {
    double integrated_lufs, true_peak_dbtp, true_peak;
    double target_gain_db, lift_db, planned_gain_db, gain_db, factor, output_lufs;
    int flags, reserved;
} bnhip_loudness;
int bnhip_loudness_measure_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, bnhip_loudness* out,
                                 double* sub_energy);
int bnhip_loudness_normalize_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs,
                                   double true_peak_dbtp, double max_gain_db, int gate_fallback, int16_t* out_pcm,
                                   bnhip_loudness* out);
int bnhip_loudness_workspace_size(int n_clips, int n, int rate, size_t* bytes);
int bnhip_loudness_normalize_device(int device, const int16_t* d_pcm, int n_clips, int n, int rate, double target_lufs,
                                    double true_peak_dbtp, double max_gain_db, int gate_fallback, int16_t* d_out_pcm,
                                    bnhip_loudness* d_out, void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* FLAC: the encoder behind every BirdWeather upload and every saved detection clip (flac.EncodePCMToBuffer / EncodePCM,
 * internal/audiocore/flac/encode.go:79-175, 320-369; birdweather/encode_native.go:28-98), for a batch of mono int16 clips of one
 * length in one call.  The bytes follow this project's own deterministic encoder spec (DESIGN.md §9 "FLAC", restated by
 * tests/flacref.py): a valid RFC 9639 stream per clip - "fLaC", STREAMINFO (MD5 zero = unknown), a SEEKTABLE when
 * seek_interval > 0 (a point for every seek_interval samples, as the reference's file path passes the sample rate), frames of 4096
 * samples with CONSTANT, FIXED (orders 0..4, partition orders 0..5, Rice parameters 0..14, the exact minimum) or VERBATIM
 * subframes.  All integer arithmetic: every byte is pinned.  Stereo, wasted bits and the MD5 are out of scope.
 *   LPC: the bnhip_*_lpc_* entries take lpc_order M in 0..8 as their last argument.  M = 0 is the encoder above, byte for byte (the
 *   entries without the argument are these called with 0).  With M > 0 LPC subframes of orders 1..min(M, bs - 1) join a frame's
 *   candidates (the reference encodes at compression level 5, an LPC level: flac/encode.go:25,136-145,350-358): a Welch-windowed
 *   integer autocorrelation, Levinson-Durbin in fp64 with a stated operation order and no contraction, 12-bit coefficients with error
 *   feedback, a shift of at most 15, the FIXED candidates' residual coding; an LPC candidate wins only by strictly fewer bits than
 *   every FIXED one, so bnhip_flac_max_bytes stands.  The spec is DESIGN.md §9 "FLAC", restated by tests/flaclpcref.py; the bytes
 *   are pinned to it, not to go-flac's.  bnhip_flac_lpc_workspace_size answers the workspace of bnhip_flac_lpc_encode_device.
 *   gain: factor (nullable, [n_clips]) is applied as the samples are read: exactly 1 is the identity, otherwise (double)pcm *
 *   factor rounded half away from zero and saturated, the rule of bnhip_loudness_*.
 *   output: the streams back to back; offsets[c] .. offsets[c + 1] is clip c's, offsets[n_clips] the bytes written.
 * max_bytes:      the worst-case output size (every frame VERBATIM); out_cap must be at least that.
 * encode_pcm16:   host memory in and out: one device allocation, one H2D copy, the kernels, a D2H copy of offsets, then of exactly
 *                 offsets[n_clips] bytes.  The fused bnhip_loudness_flac_pcm16 takes one allocation as well.
 * encode_device:  d_pcm, d_factor (nullable), d_out, d_offsets and d_workspace are device memory, d_workspace at least
 *                 bnhip_flac_workspace_size bytes and 256-byte aligned; enqueued on hip_stream (NULL = default stream), not
 *                 synchronised, nothing allocated; d_factor's values are the caller's business.
 * bnhip_loudness_flac_pcm16: bnhip_loudness_normalize_pcm16 and bnhip_flac_encode_pcm16 in one call - the normalised clips stay on
 *                 the device; the loudness records, the offsets and the compressed bytes return.
 * BNHIP_E_INVALID: NULL / empty arguments, n < 1, n_clips outside 1..65535, rate outside 1..1048575, a negative seek_interval, a
 * factor that is not finite or negative, lpc_order outside 0..8, out_cap below bnhip_flac_max_bytes, a workspace that is too small or misaligned, and for
 * the fused entry what bnhip_loudness_normalize_pcm16 rejects.  Mono int16 only: the bindings answer BNHIP_E_UNSUPPORTED for
 * anything else.  Argument errors are answered before any device is touched. */
int bnhip_flac_max_bytes(int n_clips, int n, int seek_interval, size_t* bytes);
int bnhip_flac_workspace_size(int n_clips, int n, size_t* bytes);
int bnhip_flac_encode_device(int device, const int16_t* d_pcm, int n_clips, int n, int rate, const double* d_factor,
                             int seek_interval, uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace,
                             size_t workspace_bytes, void* hip_stream);
int bnhip_flac_encode_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, const double* factor,
                            int seek_interval, uint8_t* out, size_t out_cap, uint64_t* offsets);
int bnhip_loudness_flac_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs,
                              double true_peak_dbtp, double max_gain_db, int gate_fallback, int seek_interval,
                              bnhip_loudness* out, uint8_t* out_bytes, size_t out_cap, uint64_t* offsets);
int bnhip_flac_lpc_workspace_size(int n_clips, int n, int lpc_order, size_t* bytes);
int bnhip_flac_lpc_encode_device(int device, const int16_t* d_pcm, int n_clips, int n, int rate, const double* d_factor,
                                 int seek_interval, uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace,
                                 size_t workspace_bytes, void* hip_stream, int lpc_order);
int bnhip_flac_lpc_encode_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, const double* factor,
                                int seek_interval, uint8_t* out, size_t out_cap, uint64_t* offsets, int lpc_order);
int bnhip_loudness_flac_lpc_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs,
                                  double true_peak_dbtp, double max_gain_db, int gate_fallback, int seek_interval,
                                  bnhip_loudness* out, uint8_t* out_bytes, size_t out_cap, uint64_t* offsets, int lpc_order);

/* Ragged bursts: the loudness, FLAC and spectrogram entries above for clips of unequal lengths in one call (a detection under
 * conf.ExtendedCaptureSettings is as long as the bird kept calling, so a burst of detections has as many lengths as clips).  A
 * ragged burst is n_clips mono int16 clips of lens[c] >= 1 samples packed back to back in one buffer: clip c starts at sample
 * lens[0] + .. + lens[c - 1] (64-bit), with no padding or alignment between clips; one rate, one seek_interval, one plan per call.
 * lens is a host array of n_clips ints in every entry, the device ones included, and need only stay valid until the call returns.
 * One set of kernel launches covers the burst; their number does not depend on the lengths.
 *   results: what the uniform entries give each clip on its own.  FLAC: clip c's stream is byte for byte bnhip_flac_lpc_encode_*
 *   of that clip alone (a stream depends only on its own samples, gain, rate, seek_interval and lpc_order).  Loudness: a clip with
 *   lens[c] < S has no sub-block, measures -inf and is planned as the uniform entry plans it.  The order in which a sub-block's
 *   squares are added depends on the call's split q - the largest of 8, 4, 2, 1 that divides S with q * sum(lens[c] / S) <= 2^18,
 *   for equal lengths exactly the uniform entries' q - so a ragged call and a uniform call give a clip the same bits exactly when
 *   their q are equal, and agree to rounding otherwise.
 *   output: as the uniform entries': the streams back to back with offsets[n_clips + 1], the records [n_clips], and out_pcm packed
 *   like pcm.  bnhip_flac_ragged_max_bytes is the sum over c of bnhip_flac_max_bytes(1, lens[c], seek_interval).
 *   pcm16 entries: host memory in and out; the device memory of a call is one device allocation (input, gained clips, output, offsets,
 *   records and workspaces carved from it at 256-byte alignment).  normalize: out_pcm NULL = plan only, which is also how to
 *   measure (there is no ragged measure entry).
 *   device entries: as the uniform ones; the length tables (prefix sums computed on the host) are copied into the workspace with
 *   a copy enqueued on hip_stream; nothing is allocated or synchronised.
 *   spectrogram images: bnhip_spectrogram_ragged_pcm16, bnhip_spectrogram_png_ragged_pcm16 and bnhip_spectrogram_ragged_device are
 *   bnhip_spectrogram_pcm16, bnhip_spectrogram_png_pcm16 and bnhip_spectrogram_device with lens in place of n: one width, height,
 *   window, rate pair, top_db and range_db per call, image uint8 [n_clips][height][width].  Clip c's image is byte for byte what the
 *   uniform entry gives that clip alone (its K = max(1, ceil(lens[c] / (width N))) and frame centres follow its own length; with a
 *   rate change it is rendered from its own bnhip_resample_length(lens[c], ..) floats, which the device packs like the input), and
 *   so is its PNG stream.  The PNG bound is bnhip_png_max_bytes(n_clips, width, height).  The device entry takes packed int16 or
 *   float32 at the render rate; bnhip_spectrogram_ragged_workspace_size is one 24-byte row per clip, rounded up to 256 bytes:
 *   (24 n_clips + 255) & ~255.
 * BNHIP_E_INVALID: what the uniform entries reject, lens == NULL, a lens[c] < 1, and a total length above 2^36 - 1 samples (the 36
 * bits of STREAMINFO's sample count, which also keeps every flat frame / segment / tile count inside a 31-bit grid; the spectrogram
 * entries hold the resampled lengths to the same limit), a workspace that is too small or not 256-byte aligned; answered before any
 * device is touched.
 * Not offered for ragged bursts: the sub_energy output of the measure entry, and mixed sample rates, widths or windows in one call. */
int bnhip_loudness_ragged_workspace_size(int n_clips, const int* lens, int rate, size_t* bytes);
int bnhip_loudness_ragged_normalize_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate,
                                          double target_lufs, double true_peak_dbtp, double max_gain_db, int gate_fallback,
                                          int16_t* out_pcm, bnhip_loudness* out);
int bnhip_loudness_ragged_normalize_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int rate,
                                           double target_lufs, double true_peak_dbtp, double max_gain_db, int gate_fallback,
                                           int16_t* d_out_pcm, bnhip_loudness* d_out, void* d_workspace, size_t workspace_bytes,
                                           void* hip_stream);
int bnhip_flac_ragged_max_bytes(int n_clips, const int* lens, int seek_interval, size_t* bytes);
int bnhip_flac_ragged_workspace_size(int n_clips, const int* lens, int lpc_order, size_t* bytes);
int bnhip_flac_ragged_encode_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int rate,
                                    const double* d_factor, int seek_interval, uint8_t* d_out, size_t out_cap,
                                    uint64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* hip_stream,
                                    int lpc_order);
int bnhip_flac_ragged_encode_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, const double* factor,
                                   int seek_interval, uint8_t* out, size_t out_cap, uint64_t* offsets, int lpc_order);
int bnhip_loudness_flac_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, double target_lufs,
                                     double true_peak_dbtp, double max_gain_db, int gate_fallback, int seek_interval,
                                     bnhip_loudness* out, uint8_t* out_bytes, size_t out_cap, uint64_t* offsets, int lpc_order);
int bnhip_spectrogram_ragged_workspace_size(int n_clips, const int* lens, int width, int height, size_t* bytes);
int bnhip_spectrogram_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out,
                                   int width, int height, const double* window, double top_db, double range_db, uint8_t* image);
int bnhip_spectrogram_png_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out,
                                       int width, int height, const double* window, double top_db, double range_db,
                                       const uint8_t* palette, uint8_t* out, size_t out_cap, uint64_t* offsets);
int bnhip_spectrogram_ragged_device(int device, const void* d_samples, int f32, int n_clips, const int* lens, int width,
                                    int height, const double* window, double top_db, double range_db, uint8_t* d_image,
                                    void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* FLAC decode: the read side of a saved detection clip - what the reference's pre-renderer and on-demand spectrogram requests start
 * from (GenerateFromFile, internal/spectrogram/generator.go:276-424, on a clip saved under clipenc.NativeFLAC) - for a burst of
 * streams in one call.  A burst is n_streams RFC 9639 streams back to back with host offsets[n_streams + 1], the shape
 * bnhip_flac_*_encode_* writes.  Decoded: mono, 16 bits, fixed block size 16..16384; CONSTANT, VERBATIM, FIXED 0..4 and LPC 1..32
 * subframes (precision 1..15, shift 0..15), wasted bits, both residual coding methods, escaped partitions, partition orders 0..15,
 * every block-size and sample-rate code, coded frame numbers of up to seven bytes.  Reported per stream as BNHIP_FLAC_UNSUPPORTED,
 * never guessed: more than one channel, a depth other than 16 bits, a variable-block-size stream, a STREAMINFO sample count of 0
 * (unknown) or above 2^31 - 1, min_block != max_block with more than one frame, a block size above 16384, a sample rate of 0, and a
 * stream with more than F + 64 false frame headers (F its frame count; only an adversarial stream has them).  The STREAMINFO MD5 is
 * ignored: it is NOT verified.  SEEKTABLE and every other metadata block are skipped and not trusted; a frame is accepted by its
 * CRC-8 and CRC-16, its number and its place: frame j starts exactly where frame j - 1 ended, frame 0 at audio_offset, and the last
 * frame ends at the stream's end.  A frame longer than the VERBATIM bound of its block size (2 bs + 32 bytes) is not a frame.
 *   status: BNHIP_FLAC_OK; BNHIP_FLAC_BAD_METADATA (no marker, STREAMINFO not first, repeated or not 34 bytes, a truncated block,
 *   block type 127, block bounds below 16 or inverted); BNHIP_FLAC_UNSUPPORTED (the list above); BNHIP_FLAC_CORRUPT (set by the
 *   device only: the chain of frames broke, or a sample does not fit 16 bits).
 *   stream_info:  the marker and the metadata blocks of one stream, on the host, every read bounded by n_bytes.  The return value is
 *                 an argument error only (BNHIP_E_INVALID for NULL); the stream's verdict is out->status.  audio_offset is where the
 *                 first frame header must be; seek_points the SEEKTABLE's point count.
 *   output:       the ragged packing of "Ragged bursts": int16 clips back to back, lens[c] = total_samples for a stream whose
 *                 status is OK and 0 otherwise (such a stream occupies nothing and no kernel touches it).  result[c] = {status,
 *                 frames decoded, fail_offset}: fail_offset is the byte offset from the stream's start of the first position where
 *                 the chain could not continue (for a sample outside 16 bits: that frame's start), 0 on success.  The samples of a
 *                 stream that is not OK are unspecified.
 *   decode_device: d_streams, d_pcm, d_result and d_workspace are device memory, d_workspace at least
 *                 bnhip_flac_decode_workspace_size bytes and 256-byte aligned; infos and offsets are host arrays (infos as
 *                 bnhip_flac_stream_info filled them), copied into the workspace with a copy enqueued on hip_stream; nothing is
 *                 allocated or synchronised.
 *   decode_pcm16: host memory in and out: it reads the metadata itself and fills lens; one device allocation, one H2D copy of the
 *                 streams, the kernels, a D2H copy of the results and of exactly sum(lens) samples.
 *   bnhip_flac_spectrogram_png: decode, then bnhip_spectrogram_png_ragged_pcm16 (with its resampler) in one call: the PCM never
 *                 reaches the host, rate_in is the streams' rate.  Every stream's metadata must be OK and all rates equal, else
 *                 BNHIP_E_INVALID; a stream that comes back CORRUPT still has a well-formed PNG of unspecified content.
 * BNHIP_E_INVALID: NULL / empty arguments, n_streams outside 1..65535, offsets that do not ascend, a burst above 2^40 bytes or 2^31 - 1
 * candidate slots (the sum of 2 F + 64), infos marked OK that stream_info would not accept, pcm_cap_samples or out_cap too small, a
 * workspace that is too small or misaligned, and what the render entries reject; answered before any device is touched. */
enum { BNHIP_FLAC_OK = 0, BNHIP_FLAC_BAD_METADATA = 1, BNHIP_FLAC_UNSUPPORTED = 2, BNHIP_FLAC_CORRUPT = 3 };
typedef struct bnhip_flac_info {
    uint64_t total_samples, audio_offset;
    uint32_t rate, bits, channels, min_block, max_block, min_frame, max_frame, seek_points;
    int32_t status, reserved;
} bnhip_flac_info;
typedef struct bnhip_flac_decode_result {
    int32_t status, frames;
    uint64_t fail_offset;
} bnhip_flac_decode_result;
int bnhip_flac_stream_info(const uint8_t* stream, size_t n_bytes, bnhip_flac_info* out);
int bnhip_flac_decode_workspace_size(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* bytes);
int bnhip_flac_decode_device(int device, const uint8_t* d_streams, int n_streams, const uint64_t* offsets, const bnhip_flac_info* infos,
                             int16_t* d_pcm, size_t pcm_cap_samples, bnhip_flac_decode_result* d_result, void* d_workspace,
                             size_t workspace_bytes, void* hip_stream);
int bnhip_flac_decode_pcm16(int device, const uint8_t* streams, int n_streams, const uint64_t* offsets, int16_t* pcm,
                            size_t pcm_cap_samples, int* lens, bnhip_flac_decode_result* result);
int bnhip_flac_spectrogram_png(int device, const uint8_t* streams, int n_streams, const uint64_t* offsets, int rate_out, int width,
                               int height, const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out,
                               size_t out_cap, uint64_t* png_offsets, bnhip_flac_decode_result* result);

/* FLAC recordings: what field recorders and archives write - 1 or 2 channels, 16 or 24 bits - decoded on the device by the same
 * five launches, to interleaved PCM at each stream's own depth: int16, or packed little-endian 3-byte samples; exactly the bytes of
 * a WAV data chunk of the same audio.  Stereo frames take the four channel assignments of RFC 9639 (independent, left/side,
 * side/right, mid/side), the side channel read at one bit more than the depth and decorrelated in exact integers; wasted bits are
 * per subframe; the predictor of a stream that is not mono 16-bit multiplies in 64 bits.
 *   bnhip_flac_recording_info: bnhip_flac_stream_info with the wider acceptance (host only, every read bounded by n_bytes).  OK: 1
 *                 or 2 channels, 16 or 24 bits, 1 .. 2^31 - 1 sample frames, a fixed block size of 16 .. 16384 (mono 16-bit) or
 *                 16 .. 8192 (every other shape: a frame's bytes and its int32 samples share LDS).  Anything else that parses is
 *                 BNHIP_FLAC_UNSUPPORTED - more channels, 8 / 12 / 20 / 32 bits, variable block size, a block size above the cap.
 *   bnhip_flac_decode_recordings: host memory in and out, one call for the burst.  Recording c's bytes are pcm[pcm_offsets[c] ..
 *                 pcm_offsets[c + 1]), total_samples x channels x bits / 8 of them for a stream whose metadata is accepted and none
 *                 otherwise, back to back (a later recording may start at an odd byte); pcm_offsets [n_streams + 1] is filled by
 *                 the call.  The output is cleared first: the samples of a frame that was not restored are zero.  A stream whose
 *                 chain of frames breaks is CORRUPT at that frame and keeps the frames in front of the break; a frame whose
 *                 decoded samples leave the depth's range makes the stream CORRUPT at that frame and leaves its own samples zero.
 *                 Where both happen the result names the earlier frame.
 *   ..._workspace_size / ..._device: the device-resident form, as bnhip_flac_decode_workspace_size / bnhip_flac_decode_device
 *                 are for clips; infos are bnhip_flac_recording_info's, d_pcm is cleared on hip_stream ahead of the kernels,
 *                 pcm_cap_bytes counts bytes.
 * BNHIP_E_INVALID as for the clip entries.  bnhip_flac_stream_info and the clip entries answer stereo and 24-bit streams as before:
 * BNHIP_FLAC_UNSUPPORTED.  The STREAMINFO MD5 is not verified. */
int bnhip_flac_recording_info(const uint8_t* stream, size_t n_bytes, bnhip_flac_info* out);
int bnhip_flac_decode_recordings_workspace_size(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* bytes);
int bnhip_flac_decode_recordings_device(int device, const uint8_t* d_streams, int n_streams, const uint64_t* offsets,
                                        const bnhip_flac_info* infos, void* d_pcm, size_t pcm_cap_bytes, bnhip_flac_decode_result* d_result,
                                        void* d_workspace, size_t workspace_bytes, void* hip_stream);
int bnhip_flac_decode_recordings(int device, const uint8_t* streams, int n_streams, const uint64_t* offsets, void* pcm,
                                 size_t pcm_cap_bytes, uint64_t* pcm_offsets, bnhip_flac_decode_result* result);

/* File analysis of FLAC recordings: the bnhip_analyze_channels_* calls with the recordings given as FLAC streams.  The compressed
 * bytes go to the device once; the decoder above writes each recording's interleaved PCM, at its own depth, where the channels
 * call's copies would have put it (its 16-byte line of the raw block, or its slot on the fast path), and from there the call IS the
 * channels call: the measurement, the slot launch, the framing, the model, the tail.
 *   streams  Recording r is streams[offsets[r] .. offsets[r + 1]), a whole FLAC stream; offsets [n_recordings + 1] ascend.  Rate,
 *            depth, channels and length (in frames) are what its STREAMINFO says.
 *   select   [n_recordings]: a channel index, BNHIP_CHANNEL_MIX or BNHIP_CHANNEL_AUTO, as bnhip_channels_recording.select.
 *   chosen   (may be NULL) [n_recordings], as the channels calls answer it.
 *   result   [n_recordings]: what the decoder found of each stream.  A stream found damaged on the device does not fail the call:
 *            its result is BNHIP_FLAC_CORRUPT with the frame and the offset, and its answers are those of the channels call on the
 *            PCM that bnhip_flac_decode_recordings returns for it, zeros included.  The host decides what to do with it.
 *   windows  Host only: bnhip_analyze_channels_windows over the (length, rate) of the streams.
 * BNHIP_E_INVALID (nothing written, no device work, the handle stays usable), naming the recording: a stream whose
 * bnhip_flac_recording_info status is not BNHIP_FLAC_OK, and everything the channels call refuses of the same recordings. */
long long bnhip_analyze_flac_windows(const uint8_t* streams, const uint64_t* offsets, int n_recordings, int model_rate, int n_samples,
                                     int hop, int64_t min_tail, int64_t* first_window, int64_t* resampled_length);
int bnhip_analyze_flac_topk(bnhip_model* m, const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings,
                            int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k, float* out_conf,
                            int32_t* out_idx, int32_t* chosen, bnhip_flac_decode_result* result);
int bnhip_analyze_flac(bnhip_model* m, const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings,
                       int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k, float threshold,
                       bnhip_detection* out, size_t cap, size_t* n_out, int32_t* chosen, bnhip_flac_decode_result* result);
int bnhip_analyze_flac_events(bnhip_model* m, const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings,
                              int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                              const bnhip_event_filter* filter, bnhip_event* out, size_t cap, size_t* n_out, int32_t* chosen,
                              bnhip_flac_decode_result* result);

/* Processed audio: the review UI's "re-listen with noise reduction / normalisation / gain" (ProcessAudioByID and
 * ProcessedSpectrogramByID, internal/api/v2/media/media.go:1200-1447), whose filter chain
 * internal/audiocore/ffmpeg/process.go:164-251 builds for an FFmpeg child process per clip in the fixed order
 * denoise (afftdn=nr=..:nf=..) -> normalise (loudnorm I=-23 TP=-2) -> gain (volume=..dB), for a batch of mono int16 clips of one
 * length in one call.  FFmpeg is not in the reference tree, so afftdn's arithmetic cannot be restated: the denoiser's samples
 * follow this project's own spec (DESIGN.md §9 "Denoise", restated by tests/dnref.py); the reference's two parameters, their
 * ranges, the presets light (6, -30) / medium (12, -40) / heavy (20, -50), the chain order and the validation rules are kept.
 *   denoise: frames of `frame` samples (a power of two in 64..4096) at hop frame / 4, frame m starting at (m - 3) frame / 4,
 *     zeros outside the clip; periodic Hann window w; X = real FFT of w x / 32768; P = |X|^2, smoothed within the frame as
 *     ((P[k-1] + P[k+1]) + 2 P[k]) / 4 with mirrored edges; white noise at nf_db re full scale, Nz = 10^(nf_db / 10) 3 frame / 8;
 *     g[k] = max(10^(-nr_db / 20), 1 - Nz / P[k]) (the floor alone where P = 0); y = inverse FFT of g X; output = 32768 * 2/3 * the
 *     sum of w y over the four frames that cover a sample, in frame order, rounded half away from zero and saturated to int16.
 *     All in fp64; no frame depends on another, and a clip's bytes do not depend on the batch it is in.
 *   workspace_size / device: d_pcm, d_out_pcm and d_workspace are device memory, d_workspace at least
 *     bnhip_denoise_workspace_size bytes and 256-byte aligned (the kernel keeps its frames on chip: the size is a token
 *     256 bytes, kept so that the entry has the form of the other device entries); d_out_pcm must not be d_pcm; enqueued on
 *     hip_stream (NULL = default stream), not synchronised.
 *   pcm16: host memory in and out: one H2D copy, the kernel, one D2H copy.
 *   bnhip_process_pcm16: the chain with the clips staying on the device - one H2D copy, the active stages, one D2H copy of the
 *     clips (and of the records when normalising).  frame 0 = no denoise; normalize 0 = no normalisation; gain_db 0 = no gain; a
 *     call with no stage active is BNHIP_E_INVALID (the reference hands such a request to the unprocessed endpoint instead,
 *     media.go:1338-1341: there is nothing to process).  The stages are
 *     bnhip_denoise_pcm16, then bnhip_loudness_normalize_pcm16(target_lufs, true_peak_dbtp, max_gain_db +inf, gate_fallback 0),
 *     then the saturating int16 gain at pow(10, gain_db / 20); the output is byte for byte what those give called one after
 *     another.  out (nullable when normalize is 0) receives the normalisation's records.  Divergence: each stage hands int16 to
 *     the next, where FFmpeg's chain stays in float until its output.
 * BNHIP_E_INVALID: NULL arguments, n < 1, n_clips outside 1..65535, a frame that is not a power of two in 64..4096, nr_db not
 * finite or outside [0, 97], nf_db not finite or outside [-80, -20], d_out_pcm == d_pcm, a gain_db that is not finite or outside
 * +-60 (IsValidGainDB, process.go:198-203), a workspace that is too small or misaligned, and what
 * bnhip_loudness_normalize_pcm16 rejects when normalising.  Mono int16 only: the bindings answer BNHIP_E_UNSUPPORTED for anything
 * else.  Argument errors are answered before any device is touched.
 *
 * Ragged forms ("Ragged bursts": n_clips clips of lens[c] >= 1 samples packed back to back, lens a host array; 1..65535 clips,
 * a total below 2^36 samples).  A review page of N detections of the extended capture holds about N lengths: one call instead of
 * N.  The sample values remain this project's spec, pinned to tests/dnref.py, not afftdn's; clip c's bytes are those of the
 * uniform entry called on clip c alone, whatever else the burst holds (a sample's four contributions are added in frame order
 * whatever the grouping of frames into blocks).
 *   denoise_ragged_workspace_size / _device: the workspace holds the launch's two prefix tables, the clips' starts and their
 *     tile counts: bytes = 2 * (n_clips + 1) * 8 rounded up to a multiple of 256.  The tables are copied there by a copy
 *     enqueued on hip_stream; d_out_pcm must not overlap d_pcm over the packed total; nothing is allocated or synchronised.
 *   denoise_ragged_pcm16: host memory in and out, one device allocation.
 *   bnhip_process_ragged_pcm16: bnhip_process_pcm16 of a ragged burst: the stages are bnhip_denoise_ragged_pcm16, then
 *     bnhip_loudness_ragged_normalize_pcm16(target_lufs, true_peak_dbtp, max_gain_db +inf, gate_fallback 0), then the gain; byte
 *     for byte what those give called one after another.  One device allocation.
 *   bnhip_process_spectrogram_png_ragged_pcm16: the counterpart of ProcessedSpectrogramByID (media.go:1321) -
 *     bnhip_process_ragged_pcm16, then bnhip_spectrogram_png_ragged_pcm16 at rate_in = rate (with its resampler when rate_out
 *     is neither 0 nor rate) in one call: the processed PCM never crosses to the host unless out_pcm (nullable, the packed
 *     total) asks for it.  loud (required iff normalize) receives the records; out / out_cap / png_offsets as in
 *     bnhip_spectrogram_png_ragged_pcm16.  One device allocation, one synchronising fetch.  A uniform batch is a ragged burst
 *     of equal lengths: there is no separate uniform form.
 * BNHIP_E_INVALID: what the uniform entries reject, a NULL lens, n_clips outside 1..65535, a length below 1, a total above
 * 2^36 - 1, and for the fused entry what bnhip_spectrogram_png_ragged_pcm16 rejects; answered before any device is touched. */
int bnhip_denoise_workspace_size(int n_clips, int n, int frame, size_t* bytes);
int bnhip_denoise_device(int device, const int16_t* d_pcm, int n_clips, int n, int frame, double nr_db, double nf_db,
                         int16_t* d_out_pcm, void* d_workspace, size_t workspace_bytes, void* hip_stream);
int bnhip_denoise_pcm16(int device, const int16_t* pcm, int n_clips, int n, int frame, double nr_db, double nf_db,
                        int16_t* out_pcm);
int bnhip_process_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, int frame, double nr_db, double nf_db,
                        int normalize, double target_lufs, double true_peak_dbtp, double gain_db, int16_t* out_pcm,
                        bnhip_loudness* out);
int bnhip_denoise_ragged_workspace_size(int n_clips, const int* lens, int frame, size_t* bytes);
int bnhip_denoise_ragged_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int frame, double nr_db, double nf_db,
                                int16_t* d_out_pcm, void* d_workspace, size_t workspace_bytes, void* hip_stream);
int bnhip_denoise_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int frame, double nr_db, double nf_db,
                               int16_t* out_pcm);
int bnhip_process_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, int frame, double nr_db,
                               double nf_db, int normalize, double target_lufs, double true_peak_dbtp, double gain_db,
                               int16_t* out_pcm, bnhip_loudness* out);
int bnhip_process_spectrogram_png_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, int frame,
                                               double nr_db, double nf_db, int normalize, double target_lufs, double true_peak_dbtp,
                                               double gain_db, int rate_out, int width, int height, const double* window,
                                               double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap,
                                               uint64_t* png_offsets, bnhip_loudness* loud /* required iff normalize */,
                                               int16_t* out_pcm /* nullable */);

/* Polyphase resampler for the step upstream of the classifier (Resampler.ResampleTo, internal/audiocore/resample/
 * resample.go:99-172).  Stateless per clip; n_out = ceil(n_in * rate_out / rate_in) (bnhip_resample_length); equal rates
 * pass through (NewResampler returns nil, :58-60); a too-small destination is an error before any work (:137-144).
 * The filter arithmetic of the reference lives in go-audio-resampler v1.7.0 (not in its tree, values unpinned), so the
 * filter is this project's own spec = scipy.signal.resample_poly's default Kaiser design; the _pcm16 entry keeps the
 * reference's edges: float32(int16)/32768 in, clamp +-1 and int16(f*32767) truncation out (:120-124,161-169). */
int bnhip_resample_length(int n_in, int rate_in, int rate_out);
int bnhip_resample_f32(int device, const float* in, int n_clips, int n_in, int rate_in, int rate_out, float* out,
                       int n_out_cap, int* n_out);
int bnhip_resample_pcm16(int device, const int16_t* in, int n_clips, int n_in, int rate_in, int rate_out, int16_t* out,
                         int n_out_cap, int* n_out);

/* Streaming form = the reference's stateful Resampler (internal/audiocore/resample/resample.go:44-172; call sites feed it
 * ~100 ms frames: analysis/buffer_consumer.go:118,192).  The filter history lives on the device between calls, so ANY
 * chunking of a stream yields, concatenated, exactly the samples one bnhip_resample_* call over the whole stream
 * produces (bit for bit; the flush emits the tail that needs zero-padded future input).
 *   create:   equal rates -> *out = NULL and BNHIP_OK (NewResampler returns nil, nil: resample.go:58-60).
 *   estimate: upper bound of samples one process call of n_in samples may emit (EstimateOutputBytes, :83-88).
 *   process:  empty input writes nothing (:100-102); a destination smaller than the estimate fails BEFORE the state
 *             advances (:137-144); *n_out = samples written.  PCM16 edges as in the one-shot entry (:120-124,161-169).
 *   flush:    end of stream: emits the remaining ceil(N*L/M) - emitted samples and resets the state for a new stream.
 *   destroy:  Close (:212-224); NULL is accepted. */
typedef struct bnhip_resampler bnhip_resampler;
int bnhip_resampler_create(int device, int rate_in, int rate_out, bnhip_resampler** out);
int bnhip_resampler_estimate(const bnhip_resampler* r, int n_in);
int bnhip_resampler_process_pcm16(bnhip_resampler* r, const int16_t* in, int n_in, int16_t* out, int out_cap, int* n_out);
int bnhip_resampler_process_f32(bnhip_resampler* r, const float* in, int n_in, float* out, int out_cap, int* n_out);
int bnhip_resampler_flush_pcm16(bnhip_resampler* r, int16_t* out, int out_cap, int* n_out);
int bnhip_resampler_flush_f32(bnhip_resampler* r, float* out, int out_cap, int* n_out);
void bnhip_resampler_destroy(bnhip_resampler* r);

/* Resampler bank: the rate fan-out of BufferConsumer.Write (internal/analysis/buffer_consumer.go:105-210, one stateful
 * Resampler per (source, non-native rate)) for many streams that share (rate_in, rate_out), one device call per call: the
 * frames of every stream are packed into one page-locked staging buffer with a descriptor table, resampled by one kernel
 * launch and copied back once, on one HIP stream per bank.  PCM16 in and out only (resample.go).  Each stream's output is bit
 * for bit what a bnhip_resampler of its own returns for the same frames in the same order.
 *   create:        equal rates -> *out = NULL and BNHIP_OK (as bnhip_resampler_create); max_streams fixes the slot table.
 *   add_stream:    a fresh stream; slots of removed streams are reused (with fresh state).  A full bank is BNHIP_E_INVALID.
 *   estimate:      = bnhip_resampler_estimate (upper bound for one frame of n_in samples).
 *   process:       frames f = 0..n_frames-1 (frames[f], n_in[f] samples) of streams[f]; a stream may appear several times,
 *                  its frames are consumed in call order.  out receives every frame's samples packed in call order,
 *                  out_count[f] their number (what bnhip_resampler_process_pcm16 returns for that frame).  out_cap (samples)
 *                  below the sum of estimate(n_in[f]), an unknown or removed stream, a negative length: BNHIP_E_INVALID and
 *                  no stream advances.  An empty frame emits nothing.  A device error leaves every stream as it was.
 *   flush:         end of each listed stream (each at most once): the tail, then the stream starts anew (bnhip_resampler_flush_*).
 *   windows_write_resampled: process + one bnhip_windows_write per input frame of frame f's samples into source sources[f]
 *                  of w (an empty result is a write, as AnalysisBuffer.Write of an empty slice); every source is checked
 *                  before anything runs.  Nothing leaves the library's staging.
 * Calls on one bank are serialised internally; writers of other assemblers may run at the same time. */
typedef struct bnhip_resampler_bank bnhip_resampler_bank;
int bnhip_resampler_bank_create(int device, int rate_in, int rate_out, int max_streams, bnhip_resampler_bank** out);
int bnhip_resampler_bank_add_stream(bnhip_resampler_bank* b, int* out_stream);
int bnhip_resampler_bank_remove_stream(bnhip_resampler_bank* b, int stream);
int bnhip_resampler_bank_estimate(const bnhip_resampler_bank* b, int n_in);
int bnhip_resampler_bank_process_pcm16(bnhip_resampler_bank* b, int n_frames, const int* streams, const int16_t* const* frames,
                                       const int* n_in, int16_t* out, size_t out_cap, int* out_count);
int bnhip_resampler_bank_flush_pcm16(bnhip_resampler_bank* b, int n, const int* streams, int16_t* out, size_t out_cap,
                                     int* out_count);
int bnhip_windows_write_resampled(bnhip_windows* w, bnhip_resampler_bank* b, int n_frames, const int* streams, const int* sources,
                                  const int16_t* const* frames, const int* n_in);
void bnhip_resampler_bank_destroy(bnhip_resampler_bank* b);

/* Equalizer bank: the analysis route's processing, AudioRouter.applyProcessing (internal/audiocore/router.go:1006-1080), for
 * many sources, one device call per call.  AddRoute gives the analysis BufferConsumer the source's gain (10^(dB/20)) and EQ
 * chain (internal/analysis/audio_pipeline_service.go:1005-1006); every PCM16 frame is then converted to float64
 * (x / 32768), run through every biquad of the chain `passes` times (equalizer.FilterChain.ApplyBatch), scaled by the gain,
 * clamped to [-1, 1] and truncated to int16(x * 32767) (convert.Float64ToBytesPCM16), at the source rate, before
 * BufferConsumer.Write's rate fan-out.  Output bytes equal that float64 arithmetic byte for byte (given the same sections).
 *   create:        max_streams fixes the slot table; one HIP stream per bank.  destroy: NULL-safe.
 *   add_stream:    a fresh stream (no chain, gain 1: pass-through); slots of removed streams are reused with fresh state.
 *   set_chain:     FilterChain + gainLinear of a route (router.go AddRoute / UpdateFilterChain): n_sections raw biquads
 *                  {b0, b1, b2, a0, a1, a2} (each divided by a0 as NewFilter, equalizer.go:112-136), section k run passes[k]
 *                  times.  Replaces the chain and zeroes its state.  Non-finite values, a0 == 0, passes < 1:
 *                  BNHIP_E_INVALID; more than 16 stages (sum of passes): BNHIP_E_UNSUPPORTED (a divergence: the reference has
 *                  no limit; its default chain is 2 stages).  A refused call leaves the old chain and its state.
 *   reset:         FilterChain.Reset: zero state, same chain.
 *   process:       frames f = 0..n_frames-1 (frames[f], n_in[f] samples) of streams[f]; a stream may appear several times,
 *                  its frames are consumed in call order.  out receives every frame's samples (as many as its input) packed
 *                  in call order, out_count[f] their number.  A stream with no sections and gain 1 is passed through byte for
 *                  byte without conversion (router.go:848 skips the route's processing).  out_cap (samples) below the total,
 *                  an unknown or removed stream, a negative length: BNHIP_E_INVALID and no stream advances.  A device error
 *                  leaves every stream as it was.
 *   windows_write_equalized: process + one bnhip_windows_write per frame into source sources[f] of w; every source is checked
 *                  before anything runs.
 *   design:        the RBJ biquad of equalizer.go's New* constructors (type BNHIP_EQ_*): raw section6 = {b0, b1, b2, a0, a1, a2}.
 *                  BandPass, BandReject and Peaking take width_hz (converted to octaves as hzToOctaves); the shelves and
 *                  Peaking take gain_db; q is the Q of the others.  Validation as the constructors (passes >= 1; for the
 *                  width types frequency > 0 and width_hz > 0), and non-finite results (e.g. q == 0) are BNHIP_E_INVALID.
 *                  Computed with the C library's sin / cos / pow, so a coefficient may differ from Go's in the last ulp.
 * Calls on one bank are serialised internally. */
typedef struct bnhip_eq_bank bnhip_eq_bank;
enum {
    BNHIP_EQ_LOWPASS = 0, BNHIP_EQ_HIGHPASS = 1, BNHIP_EQ_ALLPASS = 2, BNHIP_EQ_BANDPASS = 3, BNHIP_EQ_BANDREJECT = 4,
    BNHIP_EQ_LOWSHELF = 5, BNHIP_EQ_HIGHSHELF = 6, BNHIP_EQ_PEAKING = 7
};
int bnhip_eq_bank_create(int device, int max_streams, bnhip_eq_bank** out);
int bnhip_eq_bank_add_stream(bnhip_eq_bank* b, int* out_stream);
int bnhip_eq_bank_remove_stream(bnhip_eq_bank* b, int stream);
int bnhip_eq_bank_set_chain(bnhip_eq_bank* b, int stream, const double* sections, int n_sections, const int* passes, double gain_linear);
int bnhip_eq_bank_reset(bnhip_eq_bank* b, int stream);
int bnhip_eq_bank_process_pcm16(bnhip_eq_bank* b, int n_frames, const int* streams, const int16_t* const* frames, const int* n_in,
                                int16_t* out, size_t out_cap, int* out_count);
int bnhip_windows_write_equalized(bnhip_windows* w, bnhip_eq_bank* b, int n_frames, const int* streams, const int* sources,
                                  const int16_t* const* frames, const int* n_in);
int bnhip_eq_design(int type, double sample_rate, double frequency, double q, double width_hz, double gain_db, int passes,
                    double* section6);
void bnhip_eq_bank_destroy(bnhip_eq_bank* b);

/* Sound level bank: the 1/3-octave sound level monitor, soundlevel.Processor (internal/audiocore/soundlevel/processor.go) behind
 * one SoundLevelConsumer route per source (internal/analysis/sound_level_consumer.go:103-150, registered by
 * internal/analysis/audio_pipeline_service.go:685-740), for many sources of ONE sample rate, one device call per call.  Per
 * source, in float64: every PCM16 sample x / 32768 runs through the ISO 266 band-pass biquads (processAudioSample :231-250,
 * state reset when the output is NaN, +-Inf or above 100 in magnitude); every consecutive 1-second block's sum of squares gives
 * rms = sqrt(sum / fs), clamped to [1e-10, 10], and 20 * Log10(rms) dB; each call that ends with at least one unmeasured block
 * takes exactly ONE measurement (ProcessSamples :258-327: a 2.5 s frame gives one, the next frames the rest, one each); every
 * `interval` measurements give one report of per-band min / max / mean dB (generateSoundLevelData :349-412).
 *   bands:         NewProcessor's bands at sample_rate (:120-158, newOctaveBandFilter :161-225): the centres whose upper edge
 *                  c * 2^(1/6) lies below 0.95 x Nyquist (30 at 48 kHz, 29 at 44.1 kHz, 25 at 16 kHz), each
 *                  {c, b0, b1, b2, a1, a2} / a0 of the RBJ constant-0-dB band-pass with Q = max(c / (high - low), 0.5).  *n_bands
 *                  gets the count; bands6 NULL: the count only; cap (bands) below it: BNHIP_E_INVALID.  sample_rate <= 0 and
 *                  an out-of-range or unstable band are BNHIP_E_INVALID, as NewProcessor's errors.  Computed with the C
 *                  library's sin / cos / pow, so a coefficient may differ from Go's in the last ulp: a Go host passes its own.
 *   create:        one bank per sample rate; bands6 NULL: the table of `bands`, else n_bands (1..32) caller bands
 *                  {c, b0, b1, b2, a1, a2}, each finite with c > 0 and stable (|a2| < 1 and |a1| < 1 + a2, :212-214), else
 *                  BNHIP_E_INVALID.  max_streams fixes the slot table; one HIP stream per bank.  destroy: NULL-safe.
 *   add_stream:    a fresh Processor (zero filter state: the 100-sample silence warm-up leaves it at zero) reporting every
 *                  interval_s seconds (below 1: 1, :93-95); slots of removed streams are reused with fresh state.
 *   reset:         Processor.Reset (:331-346): zero filter state, the partial second and any unmeasured blocks dropped, the
 *                  interval cleared.
 *   process:       frames f = 0..n_frames-1 (frames[f], n_in[f] samples) of streams[f]; a stream may appear several times, its
 *                  frames are consumed in call order, each one ProcessSamples call; an empty frame is not a call (the
 *                  consumer returns first, sound_level_consumer.go:117).  The reports the frames complete go to reports[] in
 *                  frame order, their number to *n_reports; `frame` is the index f after which ProcessSamples returned it.
 *                  More reports than max_reports, an unknown or removed stream, a negative length: BNHIP_E_INVALID and nothing
 *                  changes.  A device error leaves every stream, its unmeasured blocks and its interval as they were.
 * Divergences: dB uses the C library's log, which may differ from Go's math.Log in the last ulp; max_streams is fixed at
 * create.  The filter outputs, block sums, measurement schedule and report count are the reference's exactly.
 * Calls on one bank are serialised internally. */
#define BNHIP_SOUNDLEVEL_MAX_BANDS 32
typedef struct bnhip_soundlevel_bank bnhip_soundlevel_bank;
typedef struct bnhip_sound_level {         /* one SoundLevelData (processor.go / soundlevel/types.go) */
    int stream, frame;                     /* frame: index in the call after which ProcessSamples returned it */
    int duration_s, n_bands;               /* Duration (the interval), bands in use */
    double center_hz[BNHIP_SOUNDLEVEL_MAX_BANDS], min_db[BNHIP_SOUNDLEVEL_MAX_BANDS], max_db[BNHIP_SOUNDLEVEL_MAX_BANDS],
        mean_db[BNHIP_SOUNDLEVEL_MAX_BANDS];
    int sample_count[BNHIP_SOUNDLEVEL_MAX_BANDS];
} bnhip_sound_level;
int bnhip_soundlevel_bands(int sample_rate, double* bands6, int cap, int* n_bands);
int bnhip_soundlevel_bank_create(int device, int sample_rate, int max_streams, const double* bands6, int n_bands,
                                 bnhip_soundlevel_bank** out);
int bnhip_soundlevel_bank_add_stream(bnhip_soundlevel_bank* b, int interval_s, int* out_stream);
int bnhip_soundlevel_bank_remove_stream(bnhip_soundlevel_bank* b, int stream);
int bnhip_soundlevel_bank_reset(bnhip_soundlevel_bank* b, int stream);
int bnhip_soundlevel_bank_process_pcm16(bnhip_soundlevel_bank* b, int n_frames, const int* streams, const int16_t* const* frames,
                                        const int* n_in, bnhip_sound_level* reports, int max_reports, int* n_reports);
void bnhip_soundlevel_bank_destroy(bnhip_soundlevel_bank* b);

/* Audio level bank: the per-source input level meter.  The reference gives every source an AudioLevelConsumer route
 * (internal/analysis/audio_level_consumer.go:65-93) whose every frame goes through calculateAudioLevel
 * (internal/analysis/buffer_consumer.go:252-332): an RMS level mapped to 0..100 and a clipping flag, which feed the level bars
 * (internal/api/v2/audio/audio_level.go), the audio_level health check (internal/health/checks/audio.go:230-298) and the
 * five-minute per-source summary (internal/analysis/audio_level_stats.go).  A bank measures every frame of a call in one device
 * call; one bank serves sources of any rate, because the level does not depend on the rate.
 *   the rule       For a frame of n int16 samples q[i]: sum = the exact integer sum of q[i]^2, clipping = any q[i] is 32767 or
 *                  -32768.  Then in float64, in this order: rms = sqrt(double(sum) / double(n)); db = 20 * log10(rms / 32768.0);
 *                  scaled = (db - (-60.0)) * (100.0 / 50.0); if clipping, scaled = max(scaled, 95.0); scaled clamped to [0, 100];
 *                  level = (int)scaled, truncating.  n == 0 gives level 0 and no clipping, and is still a measurement (the
 *                  reference publishes it); silence gives log10(0) = -Inf, which the clamp turns into 0.  The device computes the
 *                  two integers, the host the rest.  A frame holds at most 2^23 samples: up to there sum <= 2^53, so the
 *                  reference's running float64 sum is exact and equals the integer sum.
 *   24 and 32 bit  The reference meters 16-bit PCM only.  This project's own rule for 24- and 32-bit input: the meter measures
 *                  q = clamp(rint(x * 32768), -32768, 32767), x the float32 of "Detection clips" above - the sample the capture
 *                  ring stores.
 *   bnhip_audio_level  The rule from the integers on, host only, no device: *level from sum_squares, n_samples (0..2^23) and
 *                  clipping != 0.  Uses the C library's sqrt and log10; a Go host may ignore it and use its own math.
 *   create         max_streams fixes the slot table; one HIP stream per bank.  destroy: NULL-safe.
 *   add_stream     a fresh stream: never measured, empty accumulators; slots of removed streams are reused fresh.
 *   process_pcm    frames f = 0..n_frames-1: n_samples[f] samples of bits_per_sample (16, 24 or 32, little endian, packed) at
 *                  frames[f], of stream streams[f]; a stream may appear several times, and an empty frame is a measurement.
 *                  levels[f] receives frame f's record.  One transaction: every check, then the tables and the frames staged
 *                  (each frame at a 16-byte line), one H2D copy, one launch, one D2H copy of the n_frames integer records, one
 *                  synchronise, then the commit on the host: each frame's level by the rule and, per stream in call order,
 *                  `latest` and the accumulators exactly as AudioLevelStats.Record (audio_level_stats.go:42-73): sum, count,
 *                  min, max, count of level 0, count of clipping frames.  The accumulators live on the host: a failed call
 *                  changes nothing.
 *   latest         out [max_streams]: each live stream's last record; stream = -1 (the rest zero) where the slot is dead or was
 *                  never measured.
 *   stats          The accumulators of one stream and logAndReset's derived fields (audio_level_stats.go:107-134), all integer
 *                  divisions: avg_level = sum / count, zero_pct = zero_count * 100 / count, clipping_pct = clip_count * 100 /
 *                  count; count 0: all zero.  reset != 0: snapshot and start again, as logAndReset; `latest` stays.
 *   reset          Stream `stream` (-1: all live streams): latest and the accumulators cleared.  Host work only.
 *   bnhip_capture_bank_write_levels  bnhip_capture_bank_write ("Capture bank" above) with the frames also measured where the
 *                  upload has put them.  level_streams[f] names the level bank's stream for frame f; -1: the frame is stored
 *                  but not measured - levels[f].stream is -1 and the level bank does not see it.  Both banks must be on one
 *                  device; the capture bank's lock is taken first.  Both banks' checks, then one staging copy - whole frames,
 *                  each at a 16-byte line - the ring write and the level launch on the capture bank's stream, one D2H copy of
 *                  the records, one synchronise, then both commits.  A source whose frames exceed its ring is stored trimmed, as
 *                  bnhip_capture_bank_write does, but measured in full: that is why this form stages whole frames.  On a device
 *                  failure the capture bank applies "a failed write" and the level bank is unchanged.  The 2^23-sample limit
 *                  applies to measured frames only.  The rings and clocks end as after bnhip_capture_bank_write of the frames.
 * BNHIP_E_INVALID (before any device call, the handle stays usable): NULL where a pointer is required, max_streams outside
 * 1..65535, bits_per_sample not 16, 24 or 32, an unknown or removed stream, a negative length, a measured frame above 2^23 samples,
 * a NULL frame of non-zero length, a total of 2^36 samples or more, banks on different devices, and what bnhip_capture_bank_write
 * refuses.  Allocation failure: BNHIP_E_NOMEM.  Calls on one bank are serialised internally; the same call gives the same bytes
 * on every run.  Single-device handles. */
typedef struct bnhip_level_bank bnhip_level_bank;
typedef struct bnhip_audio_level_data {    /* one AudioLevelData (buffer_consumer.go:243-248) + the integers it came from */
    int32_t stream, frame;                 /* frame: index in the call */
    int32_t level, clipping;
    int64_t n_samples, clipped_samples;
    uint64_t sum_squares;
} bnhip_audio_level_data;
typedef struct bnhip_audio_level_stats {   /* audioLevelAccum + logAndReset's derived fields */
    int64_t sum, count, zero_count, clip_count;
    int32_t min, max, avg_level, zero_pct, clipping_pct;   /* count 0: all zero */
} bnhip_audio_level_stats;
int bnhip_audio_level(uint64_t sum_squares, int64_t n_samples, int clipping, int* level);
int bnhip_level_bank_create(int device, int max_streams, bnhip_level_bank** out);
int bnhip_level_bank_add_stream(bnhip_level_bank* b, int* out_stream);
int bnhip_level_bank_remove_stream(bnhip_level_bank* b, int stream);
int bnhip_level_bank_process_pcm(bnhip_level_bank* b, int n_frames, const int32_t* streams, const int64_t* n_samples,
                                 const void* const* frames, int bits_per_sample, bnhip_audio_level_data* levels);
int bnhip_level_bank_latest(bnhip_level_bank* b, bnhip_audio_level_data* out);
int bnhip_level_bank_stats(bnhip_level_bank* b, int stream, int reset, bnhip_audio_level_stats* out);
int bnhip_level_bank_reset(bnhip_level_bank* b, int stream);
void bnhip_level_bank_destroy(bnhip_level_bank* b);
int bnhip_capture_bank_write_levels(bnhip_capture_bank* capture_bank, bnhip_level_bank* level_bank, int n_frames, const int32_t* sources,
                                    const int32_t* level_streams, const int64_t* n_samples, const void* const* frames,
                                    int bits_per_sample, bnhip_audio_level_data* levels);

/* Stream plumbing for hosts that own a HIP stream (bench harness: torch's current stream). */
int bnhip_set_stream(bnhip_model* m, void* hip_stream);
int bnhip_synchronize(bnhip_model* m);

/* Per-kernel timing (the reference has no per-operator profile wired: doc/PROFILING.md:491-540).
 * When enabled every launch is bracketed by HIP events on the model stream; bnhip_profile_read
 * synchronises and writes a JSON array [{"kernel":..,"launches":..,"ms":..,"flops":..,"bytes":..},..]
 * into buf (NUL-terminated, truncated to cap) and resets the counters. Returns bytes needed. */
int bnhip_profile_enable(bnhip_model* m, int on);
/* Restrict the event bracketing to one kernel class (e.g. "expand_dw"; NULL/"" = all): bracketing every launch costs
 * ~7 % of a step (each event is a kernel boundary), bracketing only the dominant class ~1 %. */
int bnhip_profile_filter(bnhip_model* m, const char* kernel_class);
int bnhip_profile_read(bnhip_model* m, char* buf, size_t cap);

/* Whole-call timing: when enabled, every call's plan is bracketed by ONE event pair on the stream it runs on (two kernel
 * boundaries per call, cheap enough for a timed region).  bnhip_profile_steps_read synchronises, writes up to cap calls'
 * start / end times in milliseconds relative to the first call's start (either array may be NULL), clears the record and
 * returns the number of calls recorded.  Source of the per-batch median / p95 the reference's benchmarks report
 * (cmd/perch-benchmark/main.go:31-32,354-391).  Single-device handles (engine 0 of a multi-device one). */
int bnhip_profile_steps(bnhip_model* m, int on);
int bnhip_profile_steps_read(bnhip_model* m, double* start_ms, double* end_ms, int cap);

/* Plan description (JSON) for diagnostics/DESIGN tables: one entry per launch with shapes,
 * algorithmic flops and bytes. Returns bytes needed. */
int bnhip_model_describe(const bnhip_model* m, char* buf, size_t cap);

/* Diagnostics: copy the activation produced for TFLite tensor `tensor_index` by the LAST run of
 * n_clips clips to host. Only meaningful for models created with {"debug_no_reuse":1} (otherwise the
 * arena slot may already have been recycled). Returns floats per clip, or a negative error. */
int bnhip_debug_fetch(bnhip_model* m, int tensor_index, int n_clips, float* out, size_t cap_floats);

/* Devices of a handle: returns their count and writes up to cap ordinals (1 for a plain "device" handle). */
int bnhip_model_devices(const bnhip_model* m, int* devices, int cap);

/* Idempotent; frees device memory now (BirdNET.Delete, classifier/birdnet.go:972-984). */
void bnhip_model_destroy(bnhip_model* m);

const char* bnhip_last_error(void);
/* Same text copied into the caller's buffer (NUL-terminated, truncated to cap); returns the bytes needed.  For hosts that
 * prefer an out-buffer to a thread-local pointer. */
int bnhip_last_error_copy(char* buf, size_t cap);
const char* bnhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BNHIP_H */
