/* abea_events_ref.c — CPU restatement of what f5c runs per read before align(), written from the reference's lines
 * (R/benchmarks/abea/src/f5c.c:1227-1231, events.c:292-503, align.c:49-97), not from the device kernels: whole-read
 * arrays and plain loops.  Built by tests/abea_events_ref.py with -ffp-contract=off.  Test infrastructure only.
 * The one deviation (include/gbx.h): a read in which no peak is found has no events.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { uint64_t start; float length, mean, stdv; } ev_t;          /* event_t, f5c.h:104-111 */
typedef struct { float level_mean, level_stdv, level_log_stdv; } model_t;   /* f5c.h:122-136 */

/* events.c:314-363 */
static void tstat(const double *sum, const double *sumsq, size_t n, size_t w, float *out)
{
    const float eta = FLT_MIN, wf = (float)w;
    memset(out, 0, n * sizeof(float));
    if (n < 2 * w || w < 2) return;
    for (size_t i = w; i <= n - w; ++i) {
        double sum1 = sum[i], sumsq1 = sumsq[i];
        if (i > w) { sum1 -= sum[i - w]; sumsq1 -= sumsq[i - w]; }
        float sum2 = (float)(sum[i + w] - sum[i]);
        float sumsq2 = (float)(sumsq[i + w] - sumsq[i]);
        float mean1 = sum1 / wf;
        float mean2 = sum2 / wf;
        float combined_var = sumsq1 / wf - mean1 * mean1 + sumsq2 / wf - mean2 * mean2;
        combined_var = fmaxf(combined_var, eta);
        const float delta_mean = mean2 - mean1;
        out[i] = fabs(delta_mean) / sqrt(combined_var / wf);
    }
}

typedef struct { size_t masked_to, window; int peak_pos; float peak_value, threshold; int valid; const float *signal; } det_t;

/* events.c:456-472 */
static ev_t make_event(size_t start, size_t end, const double *sums, const double *sumsqs)
{
    ev_t e;
    e.start = (uint64_t)start;
    e.length = (float)(end - start);
    e.mean = (float)(sums[end] - sums[start]) / e.length;
    const float deltasqr = (sumsqs[end] - sumsqs[start]);
    const float var = deltasqr / e.length - e.mean * e.mean;
    e.stdv = sqrtf(fmaxf(var, 0.0f));
    return e;
}

/* one read: returns the number of events (0: no peak found); writes them when out != NULL (at most cap) */
static int64_t detect(const int16_t *adc, int64_t nsample, float range, float digitisation, float offset, ev_t *out, int64_t cap)
{
    if (nsample <= 0) return 0;
    const size_t n = (size_t)nsample;
    float *pa = malloc(n * sizeof(float)), *t1 = malloc(n * sizeof(float)), *t2 = malloc(n * sizeof(float));
    double *sum = malloc((n + 1) * sizeof(double)), *sumsq = malloc((n + 1) * sizeof(double));
    size_t *peaks = calloc(n, sizeof(size_t));
    const float raw_unit = range / digitisation;                             /* f5c.c:1228-1231 */
    for (size_t j = 0; j < n; ++j) pa[j] = ((float)adc[j] + offset) * raw_unit;
    sum[0] = 0.0; sumsq[0] = 0.0;                                            /* events.c:296-301 */
    for (size_t i = 0; i < n; ++i) {
        sum[i + 1] = sum[i] + pa[i];
        sumsq[i + 1] = sumsq[i] + pa[i] * pa[i];
    }
    tstat(sum, sumsq, n, 3, t1);
    tstat(sum, sumsq, n, 6, t2);
    det_t d[2] = {{0, 3, -1, FLT_MAX, 1.4f, 0, t1}, {0, 6, -1, FLT_MAX, 9.0f, 0, t2}};
    const float peak_height = 0.2f;
    size_t n_peaks = 0;
    for (size_t i = 0; i < n; ++i) {                                         /* events.c:382-439 */
        for (int k = 0; k < 2; ++k) {
            det_t *q = &d[k];
            if (q->masked_to >= i) continue;
            const float v = q->signal[i];
            if (q->peak_pos == -1) {
                if (v < q->peak_value) q->peak_value = v;
                else if (v - q->peak_value > peak_height) { q->peak_value = v; q->peak_pos = (int)i; }
            } else {
                if (v > q->peak_value) { q->peak_value = v; q->peak_pos = (int)i; }
                if (k == 0 && q->peak_value > q->threshold) {
                    d[1].masked_to = q->peak_pos + q->window;
                    d[1].peak_pos = -1; d[1].peak_value = FLT_MAX; d[1].valid = 0;
                }
                if (q->peak_value - v > peak_height && q->peak_value > q->threshold) q->valid = 1;
                if (q->valid && (i - q->peak_pos) > q->window / 2) {
                    peaks[n_peaks++] = (size_t)q->peak_pos;
                    q->peak_pos = -1; q->peak_value = v; q->valid = 0;
                }
            }
        }
    }
    size_t ne = 1;                                                           /* events.c:479-484 */
    for (size_t i = 0; i < n; ++i) if (peaks[i] > 0 && peaks[i] < n) ++ne;
    int64_t ret = 0;
    if (ne >= 2) {
        ret = (int64_t)ne;
        if (out) {
            ev_t *tmp = malloc(ne * sizeof(ev_t));
            tmp[0] = make_event(0, peaks[0], sum, sumsq);
            for (size_t e = 1; e < ne - 1; ++e) tmp[e] = make_event(peaks[e - 1], peaks[e], sum, sumsq);
            tmp[ne - 1] = make_event(peaks[ne - 2], n, sum, sumsq);
            memcpy(out, tmp, (size_t)(ret < cap ? ret : cap) * sizeof(ev_t));
            free(tmp);
        }
    }
    free(pa); free(t1); free(t2); free(sum); free(sumsq); free(peaks);
    return ret;
}

void aer_detect_many(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range, const float *digitisation,
                     const float *offset, int64_t *n_events, const int64_t *event_off, ev_t *events, int threads)
{
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t got = detect(raw + raw_off[r], raw_off[r + 1] - raw_off[r], range[r], digitisation[r], offset[r],
                                   events ? events + event_off[r] : NULL, events ? event_off[r + 1] - event_off[r] : 0);
        if (!events) n_events[r] = got;
    }
}

static uint32_t base_rank(char b) { return b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 0; }   /* align.c:10-23 */

/* align.c:49-97; a read without events or k-mers gets 0, 0 (the contract of include/gbx.h) */
void aer_scalings_many(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, const char *seq, const int64_t *event_off,
                       const ev_t *events, const model_t *model, float *scale, float *shift, int threads)
{
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (int64_t r = 0; r < n_reads; ++r) {
        const ev_t *ev = events + event_off[r];
        const size_t n = (size_t)(event_off[r + 1] - event_off[r]);
        const int32_t n_kmers = seq_len[r] - 6 + 1;
        const char *s = seq + seq_off[r];
        if (n < 1 || n_kmers < 1) { scale[r] = 0.0f; shift[r] = 0.0f; continue; }
        double event_level_sum = 0.0f;
        for (size_t i = 0; i < n; ++i) event_level_sum += ev[i].mean;
        double kmer_level_sum = 0.0f, kmer_level_sq_sum = 0.0f;
        for (int32_t i = 0; i < n_kmers; ++i) {
            uint32_t kr = 0;
            for (uint32_t j = 0; j < 6; ++j) kr += base_rank(s[i + 6 - j - 1]) << (j << 1);
            double l = model[kr].level_mean;
            kmer_level_sum += l;
            kmer_level_sq_sum += l * l;
        }
        double sh = event_level_sum / n - kmer_level_sum / n_kmers;
        double event_level_sq_sum = 0.0f;
        for (size_t i = 0; i < n; ++i) event_level_sq_sum += (ev[i].mean - sh) * (ev[i].mean - sh);
        double sc = (event_level_sq_sum / n) / (kmer_level_sq_sum / n_kmers);
        shift[r] = (float)sh;
        scale[r] = (float)sc;
    }
}
