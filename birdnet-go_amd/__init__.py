"""birdnet-go_amd: MI355X-native BirdNET inference hot path behind birdnet-go's
`inference.Classifier` seam (reference `internal/inference/backend.go:8-29`).

Only what the hot path needs lives here: the HIP/C++ engine + C ABI (`csrc/`, built into
`lib/libbnhip.so`), the host-side mirror of the reference interface (`host.py`), the model
container tooling (`tflite_schema.py`, `tflite_build.py`, `synth_model.py`) WAV ingest and the
spectrogram image surface (`spectrogram.py`) the clip loudness surface (`loudness.py`), the FLAC clip
encoder surface (`flac.py`) and the processed-audio surface (`process.py`).
The directory name carries a hyphen (task contract); import it as `birdnet_go_amd` via the
alias module at the repo root.
"""
from . import tflite_schema, flatbuf_writer, tflite_build, synth_model, build, host, shard, wav, results, spectrogram, loudness, flac, process  # noqa: F401
from .flac import encode_clips, normalize_and_encode  # noqa: F401

__all__ = ["tflite_schema", "flatbuf_writer", "tflite_build", "synth_model", "build", "host", "shard", "wav", "results", "spectrogram", "loudness", "flac", "process", "encode_clips",
           "normalize_and_encode"]
