package hip

import "math"

// EqualizerSection is one raw RBJ biquad {b0, b1, b2, a0, a1, a2} and its passes (equalizer.NewFilter's arguments), the
// unit EqualizerBank.SetChain takes.
type EqualizerSection struct {
	Coef   [6]float64
	Passes int
}

// EqualizerFilter has the fields of conf.EqualizerFilter in the same order, so a host converts one with
// hip.EqualizerFilter(f) (struct conversion ignores tags).
type EqualizerFilter struct {
	Type      string
	Frequency float64
	Q         float64
	Gain      float64
	Width     float64
	Passes    int
}

// GainLinear is the route's gain factor, math.Pow(10, gainDB/20) (analysis/audio_pipeline_service.go:1005).
func GainLinear(gainDB float64) float64 { return math.Pow(10, gainDB/20) }

// BuildEqualizerSections follows equalizer.BuildFilterChain (equalizer/builder.go) with Go's math, so the sections are the
// reference's coefficients bit for bit: nil when disabled, empty, or when no filter could be built; passes < 1 becomes 1;
// unknown types and filters the constructors refuse are skipped.  Sections whose coefficients are not finite (q == 0) are
// skipped too: the bank refuses them.
func BuildEqualizerSections(enabled bool, filters []EqualizerFilter, sampleRate int) []EqualizerSection {
	if !enabled || len(filters) == 0 {
		return nil
	}
	var out []EqualizerSection
	for _, f := range filters {
		passes := max(f.Passes, 1)
		c, ok := rbjSection(f, float64(sampleRate))
		if !ok {
			continue
		}
		out = append(out, EqualizerSection{Coef: c, Passes: passes})
	}
	return out
}

func hzToOctaves(f, width float64) float64 {
	half := width / 2.0
	if half >= f-1.0 {
		half = f - 1.0
	}
	if half <= 0 {
		half = 0.01
	}
	lower := f - half
	if lower <= 0 {
		lower = 0.01
	}
	return math.Log2((f + half) / lower)
}

// rbjSection: the RBJ audio-EQ-cookbook biquad of one filter, parameterised as equalizer.go's New* constructors.
func rbjSection(f EqualizerFilter, fs float64) ([6]float64, bool) {
	var r [6]float64
	byWidth := f.Type == "BandPass" || f.Type == "BandReject" || f.Type == "Peaking"
	if byWidth && (f.Frequency <= 0 || f.Width <= 0) {
		return r, false
	}
	w0 := 2.0 * math.Pi * f.Frequency / fs
	cw, sw := math.Cos(w0), math.Sin(w0)
	alpha := sw / (2.0 * f.Q)
	if byWidth {
		alpha = sw * math.Sinh(math.Log(2.0)/2.0*hzToOctaves(f.Frequency, f.Width)*w0/sw)
	}
	a := math.Pow(10.0, f.Gain/40.0)
	switch f.Type {
	case "LowPass":
		r = [6]float64{(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0, 1.0 + alpha, -2.0 * cw, 1.0 - alpha}
	case "HighPass":
		r = [6]float64{(1.0 + cw) / 2.0, -1.0 * (1.0 + cw), (1.0 + cw) / 2.0, 1.0 + alpha, -2.0 * cw, 1.0 - alpha}
	case "AllPass":
		r = [6]float64{1.0 - alpha, -2.0 * cw, 1.0 + alpha, 1.0 + alpha, -2.0 * cw, 1.0 - alpha}
	case "BandPass":
		r = [6]float64{alpha, 0.0, -1.0 * alpha, 1.0 + alpha, -2.0 * cw, 1.0 - alpha}
	case "BandReject":
		r = [6]float64{1.0, -2.0 * cw, 1.0, 1.0 + alpha, -2.0 * cw, 1.0 - alpha}
	case "LowShelf":
		beta := math.Sqrt(a) / f.Q
		r = [6]float64{a * ((a + 1.0) - (a-1.0)*cw + beta*sw), 2.0 * a * ((a - 1.0) - (a+1.0)*cw), a * ((a + 1.0) - (a-1.0)*cw - beta*sw),
			(a + 1.0) + (a-1.0)*cw + beta*sw, -2.0 * ((a - 1.0) + (a+1.0)*cw), (a + 1.0) + (a-1.0)*cw - beta*sw}
	case "HighShelf":
		beta := math.Sqrt(a) / f.Q
		r = [6]float64{a * ((a + 1.0) + (a-1.0)*cw + beta*sw), -2.0 * a * ((a - 1.0) + (a+1.0)*cw), a * ((a + 1.0) + (a-1.0)*cw - beta*sw),
			(a + 1.0) - (a-1.0)*cw + beta*sw, 2.0 * ((a - 1.0) - (a+1.0)*cw), (a + 1.0) - (a-1.0)*cw - beta*sw}
	case "Peaking":
		r = [6]float64{1.0 + alpha*a, -2.0 * cw, 1.0 - alpha*a, 1.0 + alpha/a, -2.0 * cw, 1.0 - alpha/a}
	default:
		return r, false
	}
	for _, v := range r {
		if math.IsNaN(v) || math.IsInf(v, 0) {
			return r, false
		}
	}
	return r, r[3] != 0
}
