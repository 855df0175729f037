/* The host leg of tools/level_rate.py: calculateAudioLevel (internal/analysis/buffer_consumer.go:271-332) as a plain C loop, one
 * thread, for every source of one tick - what a host that wants level bars does today with the samples it already holds.  It stands
 * in for the Go loop (same operations per sample: abs, a float64 multiply-add, two compares); it is not the Go program.
 *
 *     cc -O2 -o level_ref tools/level_ref.c -lm && ./level_ref [sources] [samples] [ticks]
 * Prints one JSON line: p50 / p95 / min milliseconds per tick over `ticks` ticks after two warm-ups. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

static int level_of(const int16_t* q, long n, int* clipping) {
    if (n == 0) { *clipping = 0; return 0; }
    double sum = 0.0;
    int clip = 0;
    for (long i = 0; i < n; i++) {
        const double a = fabs((double)q[i]);
        sum += a * a;
        if (q[i] == 32767 || q[i] == -32768) clip = 1;
    }
    const double rms = sqrt(sum / (double)n);
    const double db = 20 * log10(rms / 32768.0);
    double scaled = (db - (-60.0)) * (100.0 / 50.0);
    if (clip) scaled = fmax(scaled, 95.0);
    if (scaled < 0) scaled = 0; else if (scaled > 100) scaled = 100;
    *clipping = clip;
    return (int)scaled;
}

static int cmp(const void* a, const void* b) { return (*(const double*)a > *(const double*)b) - (*(const double*)a < *(const double*)b); }

int main(int argc, char** argv) {
    const long sources = argc > 1 ? atol(argv[1]) : 256, n = argc > 2 ? atol(argv[2]) : 72000;
    const int ticks = argc > 3 ? atoi(argv[3]) : 40;
    if (sources < 1 || n < 1 || ticks < 1) return 2;
    int16_t* pcm = malloc((size_t)sources * n * sizeof *pcm);
    double* ms = malloc((size_t)ticks * sizeof *ms);
    if (!pcm || !ms) return 1;
    uint32_t x = 12345;
    for (long i = 0; i < sources * n; i++) { x = x * 1664525u + 1013904223u; pcm[i] = (int16_t)((int32_t)(x >> 16) - 32768) / 8; }
    long check = 0;
    for (int t = -2; t < ticks; t++) {
        struct timespec a, b;
        clock_gettime(CLOCK_MONOTONIC, &a);
        for (long s = 0; s < sources; s++) {
            int clip;
            check += level_of(pcm + s * n, n, &clip) + clip;
        }
        clock_gettime(CLOCK_MONOTONIC, &b);
        if (t >= 0) ms[t] = (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) / 1e6;
    }
    qsort(ms, (size_t)ticks, sizeof *ms, cmp);
    printf("{\"sources\": %ld, \"samples\": %ld, \"ticks\": %d, \"p50_ms\": %.3f, \"p95_ms\": %.3f, \"min_ms\": %.3f, \"check\": %ld}\n", sources, n, ticks,
           ms[ticks / 2], ms[(int)(ticks * 0.95) < ticks ? (int)(ticks * 0.95) : ticks - 1], ms[0], check);
    free(pcm); free(ms);
    return 0;
}
