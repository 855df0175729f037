/* C restatement of the sound level monitor's per-sample work (soundlevel.Processor, internal/audiocore/soundlevel/processor.go
 * :231-250 and calculateRMS's sum), in the reference's float64 operation order: the oracle of the long sound level cases in
 * tests/slref.py and leg (c) of tools/soundlevel_bank_rate.py.  A restatement, not the Go code.  Build with -ffp-contract=off.
 *
 * sl_filter runs n PCM16 samples of one stream through nb bands ({b0, b1, b2, a1, a2} each), band after band as the reference
 * does; st holds {x1, x2, y1, y2, sum} per band and *fill the samples already in the open 1-second block.  The sum of squares of
 * every block the samples complete goes to sums[k * nb + j] (at most cap blocks); returns the number of blocks. */
#include <math.h>
#include <stdint.h>

long sl_filter(const double* coef, int nb, int fs, const int16_t* x, long n, double* st, long* fill, double* sums, long cap) {
    long blocks = 0;
    for (int j = 0; j < nb; j++) {
        const double b0 = coef[5 * j], b1 = coef[5 * j + 1], b2 = coef[5 * j + 2], a1 = coef[5 * j + 3], a2 = coef[5 * j + 4];
        double x1 = st[5 * j], x2 = st[5 * j + 1], y1 = st[5 * j + 2], y2 = st[5 * j + 3], sum = st[5 * j + 4];
        long pos = *fill, k = 0;
        for (long i = 0; i < n; i++) {
            const double in = (double)x[i] / 32768.0;
            double y = b0 * in + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2;
            if (isnan(y) || isinf(y) || fabs(y) > 100.0) {
                x1 = 0.0; x2 = 0.0; y1 = 0.0; y2 = 0.0;
                y = in * 0.1;
            }
            x2 = x1; x1 = in; y2 = y1; y1 = y;
            sum += y * y;
            if (++pos == fs) {
                if (k < cap) sums[k * nb + j] = sum;
                k++;
                sum = 0.0;
                pos = 0;
            }
        }
        st[5 * j] = x1; st[5 * j + 1] = x2; st[5 * j + 2] = y1; st[5 * j + 3] = y2; st[5 * j + 4] = sum;
        blocks = k;
        if (j == nb - 1) *fill = pos;
    }
    return blocks;
}
