package hip

import (
	"errors"
	"fmt"
	"math"
)

// SoundLevelBand is one 1/3-octave band of the sound level monitor: its centre frequency and its biquad, normalised by a0.
type SoundLevelBand struct {
	CenterFreq         float64
	B0, B1, B2, A1, A2 float64
}

// SoundLevelBandData is one band of a report (soundlevel.OctaveBandData).
type SoundLevelBandData struct {
	CenterFreq     float64
	Min, Max, Mean float64
	SampleCount    int
}

// SoundLevelReport is one soundlevel.SoundLevelData of a bank stream: Frame is the index of the frame of the Process call
// after which ProcessSamples returned it.  Timestamp, Source and Name are the host's.
type SoundLevelReport struct {
	Stream, Frame int
	Duration      int
	OctaveBands   map[string]SoundLevelBandData
}

// soundLevelCenters are the ISO 266 centres of internal/audiocore/soundlevel/processor.go:20-23.
var soundLevelCenters = []float64{
	25, 31.5, 40, 50, 63, 80, 100, 125, 160, 200, 250, 315, 400, 500, 630, 800,
	1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000, 10000, 12500, 16000, 20000,
}

// BuildSoundLevelBands is NewProcessor's band selection (processor.go:120-141) and newOctaveBandFilter (:161-225) in Go's
// math, so the coefficients are bit-equal to the reference's: pass them to NewSoundLevelBank.
func BuildSoundLevelBands(sampleRate int) ([]SoundLevelBand, error) {
	if sampleRate <= 0 {
		return nil, fmt.Errorf("invalid sample rate: %d", sampleRate)
	}
	fs := float64(sampleRate)
	nyquist := fs / 2.0
	threshold := nyquist * 0.95
	bands := make([]SoundLevelBand, 0, len(soundLevelCenters))
	for _, c := range soundLevelCenters {
		if c*math.Pow(2, 1.0/6.0) >= threshold {
			continue
		}
		low := c / math.Pow(2, 1.0/6.0)
		high := c * math.Pow(2, 1.0/6.0)
		if low <= 0 || high >= nyquist {
			return nil, fmt.Errorf("filter frequencies out of range: low=%f, high=%f, nyquist=%f", low, high, nyquist)
		}
		omega := 2.0 * math.Pi * c / fs
		sinOmega := math.Sin(omega)
		cosOmega := math.Cos(omega)
		q := c / (high - low)
		if q < 0.5 {
			q = 0.5
		}
		alpha := sinOmega / (2.0 * q)
		a0 := 1.0 + alpha
		b := SoundLevelBand{CenterFreq: c, B0: alpha / a0, B1: 0.0 / a0, B2: -alpha / a0, A1: -2.0 * cosOmega / a0, A2: (1.0 - alpha) / a0}
		if math.Abs(b.A2) >= 1.0 || math.Abs(b.A1) >= (1.0+b.A2) {
			return nil, errors.New("unstable filter coefficients")
		}
		bands = append(bands, b)
	}
	return bands, nil
}

// SoundLevelBandKey is formatBandKey (processor.go:440-445).
func SoundLevelBandKey(centerFreq float64) string {
	if centerFreq < 1000 {
		return fmt.Sprintf("%.1f_Hz", centerFreq)
	}
	return fmt.Sprintf("%.1f_kHz", centerFreq/1000)
}
