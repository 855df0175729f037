//go:build !hip

// Stub for builds without the `hip` tag (mirrors internal/inference/openvino/stub_noopenvino.go):
// every constructor reports ErrHIPUnavailable so callers keep their existing backend; the types exist so that code
// referring to them compiles either way.
package hip

import "errors"

const Supported = false

var ErrHIPUnavailable = errors.New("hip: backend unavailable")

type Options struct {
	Devices                       []int
	MaxBatch                      int
	Precision                     string
	LogitsOutput, EmbeddingOutput int
	StrictF32                     bool
}

type Classifier struct{}

func Init(string) error                                               { return ErrHIPUnavailable }
func NewClassifier([]byte, ...int) (*Classifier, error)               { return nil, ErrHIPUnavailable }
func NewClassifierWithOptions([]byte, Options) (*Classifier, error)   { return nil, ErrHIPUnavailable }
func (*Classifier) Predict([]float32) ([]float32, error)              { return nil, ErrHIPUnavailable }
func (*Classifier) PredictBatch([]float32, int) ([]float32, error)    { return nil, ErrHIPUnavailable }
func (*Classifier) PredictPCM16([]byte, int) ([]float32, error)       { return nil, ErrHIPUnavailable }
func (*Classifier) NumSpecies() int                                   { return 0 }
func (*Classifier) Close()                                            {}
func (*Classifier) PredictWithEmbeddings([]float32) ([]float32, []float32, error) {
	return nil, nil, ErrHIPUnavailable
}
func (*Classifier) PredictTopK([]float32, int, int, float64) ([]float32, []int32, error) {
	return nil, nil, ErrHIPUnavailable
}
func (*Classifier) PredictTopKSoftmax([]float32, int, int) ([]float32, []int32, error) {
	return nil, nil, ErrHIPUnavailable
}

type WindowAssembler struct{}

func NewWindowAssembler(int, int, int) (*WindowAssembler, error)             { return nil, ErrHIPUnavailable }
func (*WindowAssembler) AddSource(string, int) (int, error)                  { return -1, ErrHIPUnavailable }
func (*WindowAssembler) RemoveSource(int) error                              { return nil }
func (*WindowAssembler) Write(int, []byte) error                             { return ErrHIPUnavailable }
func (*WindowAssembler) Collect() ([]int, []byte, error)                     { return nil, nil, ErrHIPUnavailable }
func (*WindowAssembler) OverwriteStats(int) (uint64, uint64, error)          { return 0, 0, ErrHIPUnavailable }
func (*WindowAssembler) Reset(int) error                                     { return nil }
func (*WindowAssembler) WindowBytes() int                                    { return 0 }
func (*WindowAssembler) Pinned() bool                                        { return false }
func (*WindowAssembler) Close()                                              {}
func (*Classifier) PredictWindows(*WindowAssembler) ([]int, []byte, []float32, error) {
	return nil, nil, nil, ErrHIPUnavailable
}

func (*Classifier) PredictWindowsTopK(*WindowAssembler, int, float64) ([]int, []byte, []float32, []int32, error) {
	return nil, nil, nil, nil, ErrHIPUnavailable
}

type CustomClassifier struct{}

func NewCustomClassifier([]byte, []string, ...int) (*CustomClassifier, error) { return nil, ErrHIPUnavailable }
func (*CustomClassifier) PredictEmbedding([]float32) ([]float32, error)      { return nil, ErrHIPUnavailable }
func (*CustomClassifier) NumClasses() int                                    { return 0 }
func (*CustomClassifier) InputDim() int                                      { return 0 }
func (*CustomClassifier) Labels() []string                                   { return nil }
func (*CustomClassifier) Close()                                             {}

type RangeFilter struct{}

func NewRangeFilter([]byte, ...int) (*RangeFilter, error)                { return nil, ErrHIPUnavailable }
func (*RangeFilter) Predict(float32, float32, float32) ([]float32, error) { return nil, ErrHIPUnavailable }
func (*RangeFilter) PredictBatch([]float32, int) ([]float32, error)      { return nil, ErrHIPUnavailable }
func (*RangeFilter) NumSpecies() int                                     { return 0 }
func (*RangeFilter) ComputeGrid([]float32, int, int, int, int, []float32) error { return ErrHIPUnavailable }
func (*RangeFilter) Close()                                              {}

type USFilterConfig struct{ FFTSize, HopSize, FrequencySplitHz int }

func ComputeUSFrameCV([]float64, int, USFilterConfig, int) (float64, bool, error) {
	return 0, false, ErrHIPUnavailable
}

type SpectrogramOptions struct {
	ResampleRate int
	Window       []float64
	TopDB        float64
	RangeDB      float64
}

func Spectrogram([]int16, int, int, SpectrogramOptions, int) ([]uint8, int, error) {
	return nil, 0, ErrHIPUnavailable
}

func RenderSpectrograms([]int16, int, int, int, SpectrogramOptions, int) ([]uint8, int, error) {
	return nil, 0, ErrHIPUnavailable
}

func EncodePNG([]uint8, int, int, int, []uint8, int) ([][]byte, error) { return nil, ErrHIPUnavailable }

func RenderSpectrogramPNGs([]int16, int, int, int, SpectrogramOptions, []uint8, int) ([][]byte, int, error) {
	return nil, 0, ErrHIPUnavailable
}

func RenderSpectrogramsRagged([][]int16, int, int, SpectrogramOptions, int) ([]uint8, int, error) {
	return nil, 0, ErrHIPUnavailable
}

func RenderSpectrogramPNGsRagged([][]int16, int, int, SpectrogramOptions, []uint8, int) ([][]byte, int, error) {
	return nil, 0, ErrHIPUnavailable
}

type Loudness struct {
	IntegratedLUFS float64
	TruePeakDBTP   float64
	TruePeak       float64
	TargetGainDB   float64
	LiftDB         float64
	PlannedGainDB  float64
	GainDB         float64
	Factor         float64
	OutputLUFS     float64
	PeakLimited    bool
	GateLifted     bool
	Clamped        bool
}

type LoudnessOptions struct {
	TargetLUFS   float64
	TruePeakDBTP float64
	MaxGainDB    float64
	GateFallback bool
	PlanOnly     bool
	LPCOrder     int
}

const Level5LPCOrder = 8

func MeasureLoudness([]int16, int, int, int) ([]Loudness, error) { return nil, ErrHIPUnavailable }

func NormalizeClips([]int16, int, int, LoudnessOptions, int) ([]int16, []Loudness, error) {
	return nil, nil, ErrHIPUnavailable
}

func EncodeFLAC([]int16, int, int, []float64, int, int) ([][]byte, error) { return nil, ErrHIPUnavailable }

func EncodeFLACLPC([]int16, int, int, []float64, int, int, int) ([][]byte, error) { return nil, ErrHIPUnavailable }

func NormalizeAndEncodeFLAC([]int16, int, int, LoudnessOptions, int, int) ([][]byte, []Loudness, error) {
	return nil, nil, ErrHIPUnavailable
}

type Resampler struct{}

func NewResampler(int, int, int) (*Resampler, error)         { return nil, ErrHIPUnavailable }
func ResampleBytes([]byte, int, int, int) ([]byte, error)    { return nil, ErrHIPUnavailable }
func (*Resampler) EstimateOutputBytes(int) int               { return 0 }
func (*Resampler) ResampleTo([]byte, []byte) (int, error)    { return 0, ErrHIPUnavailable }
func (*Resampler) ResampleInto([]byte) ([]byte, error)       { return nil, ErrHIPUnavailable }
func (*Resampler) Flush() ([]byte, error)                    { return nil, ErrHIPUnavailable }
func (*Resampler) FromRate() int                             { return 0 }
func (*Resampler) ToRate() int                               { return 0 }
func (*Resampler) Close() error                              { return nil }
func (*Resampler) String() string                            { return "Resampler(hip: unavailable)" }

type ResamplerBank struct{}

func NewResamplerBank(int, int, int, int) (*ResamplerBank, error)            { return nil, ErrHIPUnavailable }
func (*ResamplerBank) AddStream() (int, error)                               { return -1, ErrHIPUnavailable }
func (*ResamplerBank) RemoveStream(int) error                                { return nil }
func (*ResamplerBank) EstimateOutputBytes(int) int                           { return 0 }
func (*ResamplerBank) Process([]int, [][]byte) ([][]byte, error)             { return nil, ErrHIPUnavailable }
func (*ResamplerBank) Flush([]int) ([][]byte, error)                         { return nil, ErrHIPUnavailable }
func (*ResamplerBank) FromRate() int                                         { return 0 }
func (*ResamplerBank) ToRate() int                                           { return 0 }
func (*ResamplerBank) Close() error                                          { return nil }
func (*WindowAssembler) WriteResampled(*ResamplerBank, []int, []int, [][]byte) error { return ErrHIPUnavailable }

type EqualizerBank struct{}

func NewEqualizerBank(int, int) (*EqualizerBank, error)                   { return nil, ErrHIPUnavailable }
func (*EqualizerBank) AddStream() (int, error)                            { return -1, ErrHIPUnavailable }
func (*EqualizerBank) RemoveStream(int) error                             { return nil }
func (*EqualizerBank) SetChain(int, []EqualizerSection, float64) error    { return ErrHIPUnavailable }
func (*EqualizerBank) Reset(int) error                                    { return ErrHIPUnavailable }
func (*EqualizerBank) Process([]int, [][]byte) ([][]byte, error)          { return nil, ErrHIPUnavailable }
func (*EqualizerBank) Close() error                                       { return nil }
func (*WindowAssembler) WriteEqualized(*EqualizerBank, []int, []int, [][]byte) error { return ErrHIPUnavailable }

type SoundLevelBank struct{}

func NewSoundLevelBank(int, int, int, []SoundLevelBand) (*SoundLevelBank, error) { return nil, ErrHIPUnavailable }
func (*SoundLevelBank) AddStream(int) (int, error)                              { return -1, ErrHIPUnavailable }
func (*SoundLevelBank) RemoveStream(int) error                                  { return nil }
func (*SoundLevelBank) Reset(int) error                                         { return ErrHIPUnavailable }
func (*SoundLevelBank) Process([]int, [][]byte) ([]SoundLevelReport, error)     { return nil, ErrHIPUnavailable }
func (*SoundLevelBank) Close() error                                            { return nil }
