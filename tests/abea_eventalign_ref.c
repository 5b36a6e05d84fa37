/* abea_eventalign_ref.c - serial restatement of the eventalign contract of include/gbx.h over the entries' flat arrays: what
 * align_read_to_ref, profile_hmm_align, summarize_alignment and emit_event_alignment_tsv (the reference's eventalign.c:171-240,
 * 293-338, 345-911, 919-957, 1112-1179, 1263-1540, 1580-1642, 1651-1662, 1853-1938) compute.  The aligned pairs, the score
 * matrix and the backtrack matrix are materialised as the reference materialises them.  Test infrastructure, pinned by
 * tests/golden/abea_eventalign.npz. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define K 6
#define ST_ROWS 1
#define ST_UNDEFINED 2
#define ST_BOUND 4
enum { FROM_SAME_M, FROM_PREV_M, FROM_SAME_B, FROM_PREV_B, FROM_PREV_K, FROM_SOFT };
enum { PS_K, PS_B, PS_M };                                   /* the column of a state inside its block */

typedef struct { float level_mean, level_stdv, level_log_stdv; } model_t;
typedef struct { uint64_t start; float length, mean, stdv; } event_t;
typedef struct { int32_t ref_pos, event_idx, state; } rec_t;
typedef struct { int32_t num_events, num_steps, num_stays, num_skips; double sum_duration, sum_z_score; int32_t reference_span, pad_; } summary_t;

/* toupper, then the lowest base of an IUPAC code; -1 outside the alphabet */
static int base_rank(char c)
{
    if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    switch (c) {
    case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 0;
    case 'C': case 'S': case 'Y': case 'B': return 1;
    case 'G': case 'K': return 2;
    case 'T': return 3;
    }
    return -1;
}

void aer_transitions(double events_per_base, float *t)
{
    float p_stay = 1 - (1 / events_per_base);
    float p_skip = 0.0025, p_bad = 0.001, p_bad_self = p_bad, p_skip_self = 0.3;
    float p_mk = p_skip, p_mb = p_bad, p_mm_self = p_stay;
    float p_mm_next = 1.0f - p_mm_self - p_mk - p_mb;
    float p_bb = p_bad_self, p_bk, p_bm_next, p_bm_self;
    p_bk = p_bm_next = p_bm_self = (1.0f - p_bb) / 3;
    float p_kk = p_skip_self, p_km = 1.0f - p_kk;
    t[0] = logf(p_mk); t[1] = logf(p_mb); t[2] = logf(p_mm_self); t[3] = logf(p_mm_next);
    t[4] = logf(p_bb); t[5] = logf(p_bk); t[6] = logf(p_bm_next); t[7] = logf(p_bm_self);
    t[8] = logf(p_kk); t[9] = logf(p_km);
}

/* update_cell: the maximum in index order, from = the last index that equals the running maximum */
int32_t aer_pick(const float *x, float *mx_out)
{
    float mx = x[0];
    int32_t from = 0;
    for (int i = 1; i < 6; ++i) {
        mx = x[i] > mx ? x[i] : mx;
        from = mx == x[i] ? i : from;
    }
    *mx_out = mx;
    return from;
}

static int closest_event(int k_idx, const int32_t *map, int n_kmers)
{
    int stop_before = k_idx - 1000 > 0 ? k_idx - 1000 : 0;
    int stop_after = k_idx + 1000 < n_kmers - 1 ? k_idx + 1000 : n_kmers - 1;
    int before = -1, after = -1;
    for (int k = k_idx; k != stop_before; --k) if (map[2 * k] != -1) { before = map[2 * k]; break; }
    for (int k = k_idx; k != stop_after; ++k) if (map[2 * k] != -1) { after = map[2 * k]; break; }
    return before == -1 ? after : before;
}

static int end_pair(const int32_t *pairs, int64_t n, int64_t ref_max, int64_t idx)
{
    while (idx < n) {
        if (pairs[2 * idx] > ref_max) return (int)(idx - 1);
        idx += 1;
    }
    return (int)(n - 1);
}

/* One read.  -> the number of records, or -1 where the host entries refuse the CIGAR (N, P, a code above 8). */
int32_t aer_read(const uint32_t *cigar, int64_t n_cigar, int32_t pos, int rc, int32_t read_len, const int32_t *map, const float *ev_mean, int32_t n_events,
                 const model_t *model, float scale, float shift, float var, float log_var, double events_per_base, const char *ref, int32_t ref_len,
                 int32_t region_start, int32_t region_end, int32_t rows_cap, rec_t *rec, int32_t *status, int64_t *counts)
{
    *status = 0;
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    const int n_kmers = read_len - K + 1;
    if (n_kmers < 1 || n_events < 1) return 0;
    int64_t total = 0;
    for (int64_t c = 0; c < n_cigar; ++c) {
        const int op = cigar[c] & 0xf;
        if (op == 3 || op == 6 || op > 8) return -1;
        total += cigar[c] >> 4;
    }
    int32_t *pairs = malloc((size_t)(total + 1) * 8);
    int64_t np = 0;
    {
        int64_t read_pos = 0, ref_pos = pos;
        for (int64_t c = 0; c < n_cigar; ++c) {
            const int op = cigar[c] & 0xf;
            const int64_t len = cigar[c] >> 4;
            const int aligned = op == 0 || op == 7 || op == 8;
            const int rinc = aligned || op == 1 || op == 4, finc = aligned || op == 2;
            for (int64_t j = 0; j < len; ++j) {
                if (aligned) { pairs[2 * np] = (int32_t)ref_pos; pairs[2 * np + 1] = (int32_t)read_pos; ++np; }
                read_pos += rinc; ref_pos += finc;
            }
        }
    }
    if (region_start != -1 && region_end != -1) {
        int64_t m = 0;
        for (int64_t i = 0; i < np; ++i)
            if (pairs[2 * i] >= region_start && pairs[2 * i] <= region_end) { pairs[2 * m] = pairs[2 * i]; pairs[2 * m + 1] = pairs[2 * i + 1]; ++m; }
        np = m;
    }
    while (np > 0 && pairs[2 * (np - 1) + 1] > read_len - K) --np;
    int32_t n_rec = 0;
    if (np == 0) { free(pairs); return 0; }
    int k_start = pairs[1], k_end = pairs[2 * (np - 1) + 1];
    if (rc) { k_start = read_len - k_start - K; k_end = read_len - k_end - K; }
    const int first_event = closest_event(k_start, map, n_kmers), last_event = closest_event(k_end, map, n_kmers);
    if (first_event < 0 || last_event < 0 || first_event >= n_events || last_event >= n_events) { *status = ST_UNDEFINED; free(pairs); return 0; }
    const int forward = first_event < last_event;
    int cse = first_event;
    int64_t csr = pairs[0], cpi = 0;
    float t[10];
    aer_transitions(events_per_base, t);
    const float lp_mk = t[0], lp_mb = t[1], lp_mm_self = t[2], lp_mm_next = t[3], lp_bb = t[4], lp_bk = t[5], lp_bm_next = t[6], lp_bm_self = t[7],
                lp_kk = t[8], lp_km = t[9];
    const float pre0 = (float)log(1 - 0.5);
    for (int seg = 0;; ++seg) {
        if (!(forward ? cse < last_event : cse > last_event)) break;
        if (seg > n_events) { *status |= ST_BOUND; break; }
        const int epi = end_pair(pairs, np, csr + 100, cpi);
        if (epi < 0) { *status |= ST_UNDEFINED; break; }
        const int64_t end_ref = pairs[2 * epi];
        int end_read = pairs[2 * epi + 1];
        const int last_section = epi == np - 1;
        if (rc) end_read = read_len - end_read - K;
        const int64_t s = csr - pos, l = end_ref - csr + 1;
        if (l < 2 * K) break;
        if (s < 0 || s + l > ref_len || l > 101 || end_read < 0 || end_read >= n_kmers) { *status |= ST_UNDEFINED; break; }
        const int stop = closest_event(end_read, map, n_kmers);
        if (abs(cse - stop) < 2) break;
        const int stride = cse < stop ? 1 : -1;
        if (stop < 0 || stop >= n_events || (rc ? stride != -1 : stride != 1)) { *status |= ST_UNDEFINED; break; }
        const int R = abs(stop - cse) + 1, nk = (int)l - K + 1;
        if (R > rows_cap) { *status |= ST_ROWS; break; }
        const int n_emit = last_section ? R - 1 : (R - 1 < 50 ? R - 1 : 50);
        if (n_rec + n_emit > n_events) { *status |= ST_BOUND; break; }
        if (counts) { counts[0] += 1; counts[1] += 3ll * R * nk; }
        /* the fill: rows 0 .. R, blocks 0 .. nk + 1, three states each */
        const int n_rows = R + 1, n_cols = 3 * (nk + 2);
        float *vm = malloc((size_t)n_rows * n_cols * sizeof(float));
        uint8_t *bm = calloc((size_t)n_rows * n_cols, 1);
        for (int64_t i = 0; i < (int64_t)n_rows * n_cols; ++i) vm[i] = 0.0f;
        for (int c = 0; c < n_cols; ++c) vm[c] = -INFINITY;
        for (int rr = 0; rr < n_rows; ++rr) vm[rr * n_cols + PS_K] = vm[rr * n_cols + PS_B] = vm[rr * n_cols + PS_M] = -INFINITY;
        uint32_t *ranks = malloc((size_t)nk * 4);
        for (int ki = 0; ki < nk; ++ki) {
            uint32_t rk = 0;
            for (int i = 0; i < K; ++i) {
                /* rc: the k-mer of the reverse-complement string at seq_len - ki - K, i.e. the reverse complement of this k-mer */
                int b = rc ? 3 - base_rank(ref[s + ki + K - 1 - i]) : base_rank(ref[s + ki + i]);
                if (b < 0 || b > 3) b = rc ? 3 : 0;                               /* outside the alphabet: A on the forward string */
                rk = rk << 2 | (uint32_t)b;
            }
            ranks[ki] = rk;
        }
        for (int row = 1; row < n_rows; ++row) {
            const int event_idx = cse + (row - 1) * stride;
            for (int block = 1; block <= nk; ++block) {
                const int ki = block - 1, po = 3 * (block - 1), co = 3 * block;
                const float *prev = vm + (size_t)(row - 1) * n_cols;
                float *cur = vm + (size_t)row * n_cols;
                const model_t m = model[ranks[ki]];
                const float gp_mean = scale * m.level_mean + shift;
                const float gp_stdv = m.level_stdv * var;
                const float gp_log_stdv = m.level_log_stdv + log_var;
                const float a = (ev_mean[event_idx] - gp_mean) / gp_stdv;
                const float lp_emission_m = -0.918938f - gp_log_stdv + (-0.5f * a * a);
                float x[6], mx;
                x[0] = lp_mm_self + prev[co + PS_M]; x[1] = lp_mm_next + prev[po + PS_M]; x[2] = lp_bm_self + prev[co + PS_B];
                x[3] = lp_bm_next + prev[po + PS_B]; x[4] = lp_km + prev[po + PS_K];
                x[5] = (ki == 0 && event_idx == cse) ? 0.0f + pre0 : -INFINITY;
                bm[(size_t)row * n_cols + co + PS_M] = (uint8_t)aer_pick(x, &mx);
                cur[co + PS_M] = mx + lp_emission_m;
                x[0] = lp_mb + prev[co + PS_M]; x[1] = -INFINITY; x[2] = lp_bb + prev[co + PS_B]; x[3] = x[4] = x[5] = -INFINITY;
                bm[(size_t)row * n_cols + co + PS_B] = (uint8_t)aer_pick(x, &mx);
                cur[co + PS_B] = mx + 0.0f;
                x[0] = -INFINITY; x[1] = lp_mk + cur[po + PS_M]; x[2] = -INFINITY; x[3] = lp_bk + cur[po + PS_B]; x[4] = lp_kk + cur[po + PS_K]; x[5] = -INFINITY;
                bm[(size_t)row * n_cols + co + PS_K] = (uint8_t)aer_pick(x, &mx);
                cur[co + PS_K] = mx + 0.0f;
            }
        }
        /* the traceback, from M of the last k-mer in the last row */
        rec_t *path = malloc((size_t)(R + nk + 2) * sizeof(rec_t));
        int n_path = 0, row = n_rows - 1, col = 3 * nk + PS_M, ok = 1, steps = 0;
        if (!(vm[(size_t)row * n_cols + col] > -INFINITY)) ok = 0;
        while (ok && row > 0) {
            if (++steps > R + nk + 1) { ok = 0; *status |= ST_BOUND; break; }
            const int block = col / 3, ps = col % 3;
            if (block < 1) { ok = 0; break; }
            int kmer_idx = block - 1;
            path[n_path].ref_pos = kmer_idx; path[n_path].event_idx = cse + (row - 1) * stride; path[n_path].state = "KBM"[ps];
            ++n_path;
            const int mv = bm[(size_t)row * n_cols + col];
            if (mv == FROM_SOFT) break;
            int next_ps = mv == FROM_SAME_M || mv == FROM_PREV_M ? PS_M : mv == FROM_PREV_K ? PS_K : PS_B;
            if (mv == FROM_PREV_M || mv == FROM_PREV_B || mv == FROM_PREV_K) kmer_idx -= 1;
            if (ps != PS_K) row -= 1;
            col = 3 * (kmer_idx + 1) + next_ps;
        }
        if (counts) counts[2] += steps;
        if (ok && (row != 1 || n_path == 0)) ok = 0;                              /* a finite path ends by FROM_SOFT in row 1 */
        int num_output = 0, last_event_output = 0;
        int64_t last_ref_output = 0;
        if (ok) {
            for (int i = n_path - 1; i >= 0 && (num_output < 50 || last_section); --i) {       /* the reversed walk */
                if (path[i].state != 'K' && path[i].event_idx != cse) {
                    rec[n_rec].ref_pos = (int32_t)(csr + path[i].ref_pos); rec[n_rec].event_idx = path[i].event_idx; rec[n_rec].state = path[i].state;
                    ++n_rec; ++num_output;
                    last_event_output = path[i].event_idx; last_ref_output = csr + path[i].ref_pos;
                }
            }
        }
        free(path); free(ranks); free(vm); free(bm);
        if (!ok) { if (!(*status & ST_BOUND)) *status |= ST_UNDEFINED; break; }
        cse = last_event_output;
        csr = last_ref_output;
        cpi = end_pair(pairs, np, csr, cpi);
        if (cpi < 0) cpi = 0;
        if (num_output == 0) break;
    }
    free(pairs);
    return n_rec;
}

/* reads in parallel; rec: read r's records at rec + event_off[r] */
void aer_many(int64_t n_reads, const int64_t *cigar_off, const uint32_t *cigar, const int32_t *pos, const uint8_t *rc, const int64_t *seq_off,
              const int32_t *seq_len, const int32_t *map, const int64_t *event_off, const float *ev_mean, const model_t *model, const float *scale,
              const float *shift, const float *var, const float *log_var, const double *events_per_base, const int32_t *flags, const int64_t *ref_off,
              const int32_t *ref_len, const char *ref_arena, int32_t region_start, int32_t region_end, int32_t rows_cap, rec_t *rec, int32_t *n_rec,
              int32_t *status, int64_t *counts, int threads)
{
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (int64_t r = 0; r < n_reads; ++r) {
        n_rec[r] = 0; status[r] = 0;
        if (counts) counts[3 * r] = counts[3 * r + 1] = counts[3 * r + 2] = 0;
        if (flags && flags[r]) continue;
        n_rec[r] = aer_read(cigar + cigar_off[r], cigar_off[r + 1] - cigar_off[r], pos[r], rc[r], seq_len[r], map + 2 * seq_off[r], ev_mean + event_off[r],
                            (int32_t)(event_off[r + 1] - event_off[r]), model, scale[r], shift[r], var[r], log_var[r], events_per_base[r],
                            ref_arena + ref_off[r], ref_len[r], region_start, region_end, rows_cap, rec + event_off[r], status + r,
                            counts ? counts + 3 * r : NULL);
    }
}

static uint32_t kmers_of(const char *ref, int32_t pos, int rc, const rec_t *q, char *ref_kmer, char *model_kmer)
{
    const int64_t s = (int64_t)q->ref_pos - pos;
    uint32_t rank = 0;
    for (int i = 0; i < K; ++i) { int b = base_rank(ref[s + i]); ref_kmer[i] = "ACGT"[b < 0 ? 0 : b]; }
    for (int i = 0; i < K; ++i) {
        char c = 'N';
        if (q->state != 'B') { c = ref_kmer[rc ? K - 1 - i : i]; if (rc) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
        model_kmer[i] = c;
        rank = rank << 2 | (uint32_t)(c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0);
    }
    ref_kmer[K] = model_kmer[K] = 0;
    return rank;
}

void aer_summary(const event_t *ev, const model_t *model, float scale, float shift, float var, int rc, int32_t pos, const char *ref, const rec_t *rec,
                 int32_t n_rec, summary_t *out)
{
    summary_t s;
    memset(&s, 0, sizeof s);
    size_t prev = (size_t)-1;
    for (int32_t i = 0; i < n_rec; ++i) {
        s.num_events += 1;
        const size_t move = (size_t)rec[i].ref_pos - prev;
        if (move == 0) s.num_stays += 1;
        else if (i != 0 && move > 1) s.num_skips += 1;
        else if (i != 0 && move == 1) s.num_steps += 1;
        s.sum_duration += ev[rec[i].event_idx].length;
        if (rec[i].state == 'M') {
            char a[K + 1], b[K + 1];
            const uint32_t rank = kmers_of(ref, pos, rc, rec + i, a, b);
            const float gp_mean = scale * model[rank].level_mean + shift, gp_stdv = model[rank].level_stdv * var;
            const double z = (ev[rec[i].event_idx].mean - gp_mean) / gp_stdv;
            s.sum_z_score += z;
        }
        prev = (size_t)rec[i].ref_pos;
    }
    if (n_rec > 0) s.reference_span = rec[n_rec - 1].ref_pos - rec[0].ref_pos + 1;
    *out = s;
}

/* -> the bytes written (text has room for cap); the header line first when asked for */
int64_t aer_tsv(const event_t *ev, const model_t *model, float scale, float shift, float var, int rc, int32_t pos, const char *ref, const rec_t *rec,
                int32_t n_rec, int header, int print_read_names, int scale_events, int64_t read_index, const char *read_name, const char *ref_name,
                float sample_rate, char *text, int64_t cap)
{
    int64_t n = 0;
#define EMIT(...) do { n += snprintf(text + n, (size_t)(cap - n), __VA_ARGS__); if (n >= cap) return -1; } while (0)
    if (header)
        EMIT("contig\tposition\treference_kmer\t%s\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\tmodel_kmer\tmodel_mean\tmodel_stdv\tstandardized_level\n",
             print_read_names ? "read_name" : "read_index");
    for (int32_t i = 0; i < n_rec; ++i) {
        char rk[K + 1], mk[K + 1];
        const uint32_t rank = kmers_of(ref, pos, rc, rec + i, rk, mk);
        const event_t *e = ev + rec[i].event_idx;
        if (print_read_names) EMIT("%s\t%d\t%s\t%s\t%c\t", ref_name, rec[i].ref_pos, rk, read_name, 't');
        else EMIT("%s\t%d\t%s\t%ld\t%c\t", ref_name, rec[i].ref_pos, rk, (long)read_index, 't');
        float event_mean = e->mean, model_mean = 0.0f, model_stdv = 0.0f;
        const float event_duration = e->length / sample_rate;
        if (scale_events) {
            event_mean = (e->mean - shift) / scale;
            if (rec[i].state != 'B') { model_mean = model[rank].level_mean; model_stdv = model[rank].level_stdv; }
        } else if (rec[i].state != 'B') {
            model_mean = scale * model[rank].level_mean + shift;
            model_stdv = model[rank].level_stdv * var;
        }
        const float standard_level = (event_mean - model_mean) / (sqrtf(var) * model_stdv);
        EMIT("%d\t%.2lf\t%.3lf\t%.5lf\t", rec[i].event_idx, event_mean, e->stdv, event_duration);
        EMIT("%s\t%.2lf\t%.2lf\t%.2lf\n", mk, model_mean, model_stdv, standard_level);
    }
#undef EMIT
    return n;
}
