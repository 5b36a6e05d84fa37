/* CPU statement of the contract of abea's calibration and event-alignment record entries (include/gbx.h).  Test infrastructure.
 *
 * Written from the header's contract and checked against results that only the reference's own binaries produced
 * (tests/golden/abea_calib.npz, tests/golden/abea_meth.npz); where an order of operations decides the bits, the place in the
 * reference that fixes it is named.  Everything is serial and works on the flat arrays of the entries: a map is 2 ints per
 * k-mer, a pair list 2 ints per pair, and the 'M' records of a read are two int arrays (event, k-mer code).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum { K = 6, MIN_M = 200, WINDOW = 1000 };
enum { BAD_CALIBRATION = 1, BAD_ALIGNMENT = 2, BAD_QUALITY = 4 };

typedef struct { float mean, stdv, log_stdv; } level_t;

static int base_code(char b) { return b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 0; }   /* anything else ranks as A */

static int kmer_code(const char *s)
{
    int code = 0;
    for (int i = 0; i < K; ++i) code = code * 4 + base_code(s[i]);
    return code;
}

/* One read.  pairs: (k-mer, event) x n_pairs in list order.  map: (first, last) event per k-mer, -1 -1 without events. */
void acr_calib_read(const char *bases, int32_t n_bases, const float *event_mean, const level_t *levels, const int32_t *pairs, int32_t n_pairs,
                    float *scale, float *shift, float *var, float *log_var, double *var64, int32_t *map, double *events_per_base,
                    int32_t *n_records, int32_t *n_m, int32_t *flags)
{
    const int32_t n_kmers = n_bases - K + 1;
    *n_records = 0; *n_m = 0; *events_per_base = 0; *var = 0; *log_var = 0; *var64 = 0; *flags = 0;
    for (int32_t k = 0; k < 2 * n_kmers; ++k) map[k] = -1;
    if (n_pairs <= 0) { *flags = BAD_ALIGNMENT; return; }

    /* the map: a pair counts when its event is not the event of the pair before it (align.c:576); the least event starts at
       INT32_MAX and the greatest at 0 (align.c:566-567) */
    int32_t least = INT32_MAX, greatest = 0, seen = -1;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t k = pairs[2 * p], e = pairs[2 * p + 1];
        if (e != seen) {
            if (map[2 * k] == -1) map[2 * k] = e;
            map[2 * k + 1] = e;
        }
        if (e > greatest) greatest = e;
        if (e < least) least = e;
        seen = e;
    }
    *events_per_base = (double)(greatest - least) / n_kmers;

    /* the records: one per event of every k-mer that has events, in k-mer order; a record is 'M' when the code of its k-mer
       differs from the code of the record before it (-1 before the first), and only 'M' records are kept */
    int32_t *m_event = (int32_t *)malloc(sizeof(int32_t) * (size_t)n_kmers), *m_code = (int32_t *)malloc(sizeof(int32_t) * (size_t)n_kmers);
    int32_t records = 0, ms = 0, code_before = -1;
    for (int32_t k = 0; k < n_kmers; ++k) {
        if (map[2 * k] == -1) continue;
        const int code = kmer_code(bases + k);
        for (int32_t e = map[2 * k]; e <= map[2 * k + 1]; ++e) {
            if (code != code_before) { m_event[ms] = e; m_code[ms] = code; ++ms; }
            code_before = code;
            ++records;
        }
    }
    *n_records = records;
    *n_m = ms;

    if (ms >= MIN_M) {
        /* weighted least squares event = shift + scale x level with weights 1 / stdv^2: five double sums in record order, the
           products associated as (level x level) x w and (level x event) x w (align.c:705-710), Cramer's rule as align.c:718-720 */
        double sw = 0, swl = 0, swll = 0, swe = 0, swle = 0;
        for (int32_t i = 0; i < ms; ++i) {
            const double ev = event_mean[m_event[i]], lv = levels[m_code[i]].mean, sd = levels[m_code[i]].stdv;
            const double w = 1. / (sd * sd);
            sw += w;
            swl += lv * w;
            swll += lv * lv * w;
            swe += ev * w;
            swle += lv * ev * w;
        }
        const double det = sw * swll - swl * swl;
        const double offset = -(swl * swle - swll * swe) / det;
        const double gain = (sw * swle - swl * swe) / det;
        /* the residual with the double offset and gain, not the stored floats (align.c:736-741) */
        double acc = 0.;
        for (int32_t i = 0; i < ms; ++i) {
            const double ev = event_mean[m_event[i]], lv = levels[m_code[i]].mean, sd = levels[m_code[i]].stdv;
            const double res = (ev - offset - gain * lv);
            acc += res * res / (sd * sd);
        }
        acc /= ms;
        acc = sqrt(acc);
        *shift = (float)offset;
        *scale = (float)gain;
        *var = (float)acc;
        *var64 = acc;
        *log_var = (float)log(acc);
    }
    free(m_event);
    free(m_code);
    if (ms < MIN_M || *var > 2.5) *flags = BAD_CALIBRATION;
    else if (*events_per_base > 5.0) *flags = BAD_QUALITY;
}

/* read r: bases at seq + seq_off[r], means at event_mean + event_off[r], pairs at pairs + 4 * event_off[r] (ints), map at map + 2 * seq_off[r] */
void acr_calib_many(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, const char *seq, const int64_t *event_off, const float *event_mean,
                    const level_t *levels, const int32_t *pairs, const int32_t *n_pairs, float *scale, float *shift, float *var, float *log_var,
                    double *var64, int32_t *map, double *events_per_base, int32_t *n_records, int32_t *n_m, int32_t *flags)
{
    for (int64_t r = 0; r < n_reads; ++r)
        acr_calib_read(seq + seq_off[r], seq_len[r], event_mean + event_off[r], levels, pairs + 4 * event_off[r], n_pairs[r], scale + r, shift + r, var + r,
                       log_var + r, var64 + r, map + 2 * seq_off[r], events_per_base + r, n_records + r, n_m + r, flags + r);
}

/* ---- the event-alignment record */

/* what a CIGAR operation does per base: M I D N S H P = X; -1: the reference stops there (N: meth.c:54-58, P and beyond: :65-68) */
static const signed char OP_READ[16] = {1, 1, 0, -1, 1, 0, -1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
static const signed char OP_REF[16] = {1, 0, 1, -1, 0, 0, -1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
static const signed char OP_PAIR[16] = {1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0};

/* the first event of the nearest k-mer with events: downwards from k, stopping before max(0, k - 1000); failing that upwards,
   stopping before min(k + 1000, n_kmers - 1); -1 when neither walk meets one */
static int32_t nearest_event(const int32_t *map, int32_t n_kmers, int32_t k)
{
    const int32_t down_to = k - WINDOW > 0 ? k - WINDOW : 0, up_to = k + WINDOW < n_kmers - 1 ? k + WINDOW : n_kmers - 1;
    for (int32_t i = k; i != down_to; --i)
        if (map[2 * i] != -1) return map[2 * i];
    for (int32_t i = k; i != up_to; ++i)
        if (map[2 * i] != -1) return map[2 * i];
    return -1;
}

/* The record of one read into out (2 ints per pair, room for n_bases pairs); returns its length, -1 where the reference stops.
   An aligned base at read position q is kept when 6 <= q and q + 6 < n_bases; its k-mer is q, or n_bases - q - 6 on the reverse
   strand.  A record whose first and last event are equal is empty. */
int32_t acr_record_read(const uint32_t *cigar, int64_t n_cigar, int32_t pos, int rc, int32_t n_bases, const int32_t *map, int32_t *out)
{
    const int32_t n_kmers = n_bases - K + 1;
    int64_t q = 0, ref = pos, aligned = 0;
    int32_t kept = 0;
    for (int64_t c = 0; c < n_cigar; ++c) {
        const int op = (int)(cigar[c] & 0xf);
        const int64_t len = cigar[c] >> 4;
        if (OP_READ[op] < 0) return -1;
        if (OP_PAIR[op]) {
            aligned += len;
            if (aligned > n_bases) return -1;                                   /* the assert of meth.c:135 */
            for (int64_t j = 0; j < len; ++j) {
                const int64_t at = q + j;
                if (at < K || at + K >= n_bases) continue;
                out[2 * kept] = (int32_t)(ref + j);
                out[2 * kept + 1] = nearest_event(map, n_kmers, (int32_t)(rc ? n_bases - at - K : at));
                ++kept;
            }
        }
        q += len * OP_READ[op];
        ref += len * OP_REF[op];
    }
    if (kept > 0 && out[1] == out[2 * kept - 1]) kept = 0;
    return kept;
}
