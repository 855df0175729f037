/* Single-thread C restatement of the float32 loudness path the reference runs per clip (audionorm's meter, true peak and plan,
 * pcmgain's gain) - the CPU leg of tools/loudness_rate.py.  A RESTATEMENT written for this project, not the reference's Go: its
 * two SIMD sums run here in sample order, the true-peak taps are applied to blocks of positions so that the compiler can use
 * vector registers across positions without reordering any sum.  Coefficients come from the caller (tests/loudref.py).
 * Build: gcc -O3 -march=native -ffp-contract=off -shared -fPIC. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TAPS 32
#define PHASES 4
#define DRAIN 16
#define TILE 1024

static double measure(const int16_t* s, int n, int S, const float* kw, const float* tp, float gate_abs, float gate_rel, float* x,
                      float* E, double* dbtp) {
    const float scale = 1.0f / 32768.0f;
    float x1 = 0, x2 = 0, u1 = 0, u2 = 0, y1 = 0, y2 = 0;
    const int Ns = n / S;
    for (int i = 0; i < TAPS - 1; i++) x[i] = 0.0f;
    for (int i = 0; i < n; i++) x[TAPS - 1 + i] = (float)s[i] * scale;
    for (int i = 0; i < DRAIN + TILE; i++) x[TAPS - 1 + n + i] = 0.0f;
    for (int k = 0; k < Ns; k++) {
        float e = 0.0f;
        for (int i = k * S; i < (k + 1) * S; i++) {
            const float v = x[TAPS - 1 + i];
            const float u = kw[0] * v + kw[1] * x1 + kw[2] * x2 - kw[3] * u1 - kw[4] * u2;
            const float y = kw[5] * u + kw[6] * u1 + kw[7] * u2 - kw[8] * y1 - kw[9] * y2;
            x2 = x1; x1 = v; u2 = u1; u1 = u; y2 = y1; y1 = y;
            e += y * y;
        }
        E[k] = e;
    }
    double L = -INFINITY;
    const int Nb = Ns - 3;
    const float den = (float)(4 * S);
    float sum = 0.0f; int cnt = 0;
    for (int j = 0; j < Nb; j++) { const float z = (E[j] + E[j + 1] + E[j + 2] + E[j + 3]) / den; if (z > gate_abs) { sum += z; cnt++; } }
    if (cnt) {
        const float rel = (sum / (float)cnt) * gate_rel;
        float sum2 = 0.0f; int cnt2 = 0;
        for (int j = 0; j < Nb; j++) { const float z = (E[j] + E[j + 1] + E[j + 2] + E[j + 3]) / den; if (z > gate_abs && z > rel) { sum2 += z; cnt2++; } }
        if (cnt2) L = -0.691 + 10.0 * log10((double)sum2 / (double)cnt2);
    }
    float peak = 0.0f;
    for (int i = 0; i < n; i++) { const float a = fabsf(x[TAPS - 1 + i]); if (a > peak) peak = a; }
    float acc[TILE];
    for (int k0 = 0; k0 < n + DRAIN; k0 += TILE) {
        const int m = n + DRAIN - k0 < TILE ? n + DRAIN - k0 : TILE;
        for (int p = 0; p < PHASES; p++) {
            for (int i = 0; i < TILE; i++) acc[i] = 0.0f;
            for (int t = TAPS - 1; t >= 0; t--) {
                const float c = tp[p * TAPS + t];
                const float* xs = x + TAPS - 1 + k0 - t;
                for (int i = 0; i < TILE; i++) acc[i] += c * xs[i];
            }
            for (int i = 0; i < m; i++) { const float a = fabsf(acc[i]); if (a > peak) peak = a; }
        }
    }
    *dbtp = peak > 0.0f ? 20.0 * log10((double)peak) : -INFINITY;
    return L;
}

static void apply_gain(const int16_t* s, int n, double factor, int16_t* out) {
    if (factor == 1.0) { memcpy(out, s, (size_t)n * 2); return; }
    for (int i = 0; i < n; i++) {
        double v = round((double)s[i] * factor);
        if (v > 32767.0) v = 32767.0;
        if (v < -32768.0) v = -32768.0;
        out[i] = (int16_t)v;
    }
}

static double plan_gain(double L, double dbtp, double T, double C) {
    if (isinf(L)) return 0.0;
    double gain = T - L;
    if (!isinf(dbtp) && gain > C - dbtp) gain = C - dbtp;
    return gain;
}

/* res[0..2] = integrated loudness, true peak (dBTP), applied gain (dB); -> 0, or -1 without memory */
int loudref_normalize(const int16_t* s, int n, int rate, const float* kw, const float* tp, float gate_abs, float gate_rel, double T,
                      double C, double max_gain, int gate_fallback, int16_t* out, double* res) {
    const int S = (int)floor(0.1 * (double)rate + 0.5);
    float* x = (float*)malloc(sizeof(float) * ((size_t)n + TAPS + DRAIN + TILE));
    float* E = (float*)malloc(sizeof(float) * ((size_t)(n / S) + 1));
    if (!x || !E) { free(x); free(E); return -1; }
    double dbtp;
    const double L = measure(s, n, S, kw, tp, gate_abs, gate_rel, x, E, &dbtp);
    double planned = plan_gain(L, dbtp, T, C);
    if (gate_fallback && isinf(L) && !isinf(dbtp)) {
        const double lift = fmin(C - dbtp, T + 70.0);
        double dbtp2;
        apply_gain(s, n, lift == 0.0 ? 1.0 : pow(10.0, lift / 20.0), out);
        const double L2 = measure(out, n, S, kw, tp, gate_abs, gate_rel, x, E, &dbtp2);
        planned = lift + plan_gain(L2, dbtp2, T, C);
    }
    double gain = planned;
    if (gain > fabs(max_gain)) gain = fabs(max_gain);
    if (gain < -fabs(max_gain)) gain = -fabs(max_gain);
    apply_gain(s, n, gain == 0.0 ? 1.0 : pow(10.0, gain / 20.0), out);
    res[0] = L; res[1] = dbtp; res[2] = gain;
    free(x); free(E);
    return 0;
}
