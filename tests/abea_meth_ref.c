/* CPU restatement of abea's methylation scoring stage: the profile HMM score of f5c call-methylation and the planner
 * that cuts a read into CpG site groups.  Test infrastructure: states the contract of gbx_abea_meth_* from the reference's
 * lines (R = the reference tree, R/benchmarks/abea/src/...), plain C, threaded over jobs.
 *
 *   p7_FLogsum, its table              logsum.h:44-46, 61-71
 *   get_rank / get_kmer_rank           hmm.c:21-52
 *   log_probability_match_r9           hmm.c:55-100   (CACHED_LOG, f5c.h:67)
 *   make_post_flanking / pre           hmm.c:132-205
 *   calculate_transitions              hmm.c:247-295
 *   profile_hmm_fill_generic_r9        hmm.c:305-524, update_cell / update_end hmm.c:558-572
 *   profile_hmm_score_r9               hmm.c:620-674
 *   disambiguate, methylate, reverse_complement(_meth), find_by_ref_bounds, calculate_methylation_for_read
 *                                      meth.c:261-306, 326-467, 501-658
 *
 * The reference is compiled as C++: `log` of a float argument there is the float overload, so the transition logs are logf;
 * the flank and table logs have double arguments.
 */
#include <ctype.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float level_mean, level_stdv, level_log_stdv; } model_t;                 /* f5c.h:122-136 */
typedef struct { int32_t ref_pos, read_pos; } pair_t;                                       /* AlignedPair, f5c.h:163-166 */
typedef struct { int64_t seq_off, rc_off; int32_t seq_len, read, event_start, event_stop, rc, flags; } job_t;   /* gbx_abea_meth_job */
typedef struct { int32_t read, start_position, end_position, n_cpg; int64_t ctx_off; int32_t ctx_len, pad_; } site_t; /* gbx_abea_meth_site */

#define KMER 6
#define TBL 16000
#define SCALE 1000.f
static float flogsum_lookup[TBL];

void amr_init(void)
{
    for (int i = 0; i < TBL; i++) flogsum_lookup[i] = log(1. + exp((double)-i / SCALE));    /* logsum.h:44-46 */
}

void amr_table(float *out) { memcpy(out, flogsum_lookup, sizeof flogsum_lookup); }

/* logsum.h:61-71; cnt[0]: an operand is -inf, cnt[1]: 15.7 nats or more apart, cnt[2]: table */
static inline float flogsum(float a, float b, int64_t *cnt)
{
    const float max = a > b ? a : b;
    const float min = a < b ? a : b;
    if (min == -INFINITY) { cnt[0]++; return max; }
    if ((max - min) >= 15.7f) { cnt[1]++; return max; }
    cnt[2]++;
    return max + flogsum_lookup[(int)((max - min) * SCALE)];
}

static inline uint32_t get_rank(char base)                                                  /* hmm.c:21-36, without the warning */
{
    return base == 'C' ? 1 : base == 'G' ? 2 : base == 'M' ? 3 : base == 'T' ? 4 : 0;
}

static inline uint32_t kmer_rank(const char *s)                                             /* hmm.c:40-52 */
{
    uint32_t p = 1, r = 0;
    for (int i = 0; i < KMER; ++i) { r += get_rank(s[KMER - i - 1]) * p; p *= 5; }
    return r;
}

float amr_emission(float x, float scale, float shift, float var, float log_var, const model_t *m)    /* hmm.c:55-100 */
{
    const float log_inv_sqrt_2pi = -0.918938f;
    const float gp_mean = scale * m->level_mean + shift;
    const float gp_stdv = m->level_stdv * var;
    const float gp_log_stdv = m->level_log_stdv + log_var;
    const float a = (x - gp_mean) / gp_stdv;
    return log_inv_sqrt_2pi - gp_log_stdv + (-0.5f * a * a);
}

/* hmm.c:247-295: mk mb mm_self mm_next bb bk bm_next bm_self kk km */
void amr_transitions(double events_per_base, float *t)
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

/* hmm.c:172-205: n + 1 entries */
void amr_pre_flank(int64_t n, float *pre)
{
    pre[0] = log(1 - 0.5);
    if (n >= 1) pre[1] = log(0.5) + -3.0f + log(1 - 0.9);
    for (int64_t i = 2; i <= n; ++i) pre[i] = log(0.9) + -3.0f + pre[i - 1];
}

/* hmm.c:132-168: n entries */
void amr_post_flank(int64_t n, float *post)
{
    post[n - 1] = log(1 - 0.5);
    if (n > 1) {
        post[n - 2] = log(0.5) + -3.0f + log(1 - 0.9);
        for (int64_t i = n - 3; i >= 0; --i) post[i] = log(0.9) + -3.0f + post[i + 1];
    }
}

/* hmm.c:305-524 and 620-674.  ev: the read's event means. */
float amr_score(const char *m_seq, const char *m_rc_seq, int32_t seq_len, const float *ev, float scale, float shift, float var,
                float log_var, const model_t *model, uint32_t e_start, uint32_t e_stop, int rc, double events_per_base,
                uint32_t flags, int64_t *cnt)
{
    const uint32_t n_kmers = (uint32_t)seq_len - KMER + 1;
    const uint32_t n_events = e_stop > e_start ? e_stop - e_start + 1 : e_start - e_stop + 1;
    const uint32_t n_rows = n_events + 1, n_blocks = n_kmers + 2, n_cols = 3 * n_blocks;
    const int event_stride = rc ? -1 : 1;
    const uint32_t last_kmer_idx = n_kmers - 1, last_event_row_idx = n_rows - 1;
    float t[10];
    amr_transitions(events_per_base, t);
    const float lp_mk = t[0], lp_mb = t[1], lp_mm_self = t[2], lp_mm_next = t[3], lp_bb = t[4], lp_bk = t[5], lp_bm_next = t[6],
                lp_bm_self = t[7], lp_kk = t[8], lp_km = t[9];
    uint32_t *ranks = malloc(sizeof(uint32_t) * n_kmers);
    for (uint32_t ki = 0; ki < n_kmers; ++ki)                                                /* hmm.c:382-393 */
        ranks[ki] = kmer_rank(rc == 0 ? m_seq + ki : m_rc_seq + seq_len - ki - KMER);
    float *pre = malloc(sizeof(float) * (n_events + 1)), *post = malloc(sizeof(float) * n_events);
    amr_pre_flank(n_events, pre);
    amr_post_flank(n_events, post);
    float *rows = malloc(sizeof(float) * 2 * n_cols);
    float *prev = rows, *cur = rows + n_cols;
    for (uint32_t c = 0; c < n_cols; ++c) prev[c] = cur[c] = -INFINITY;                      /* hmm.c:605-617: row 0 and block 0 */
    const float lp_sm = 0.0f, lp_ms = 0.0f;
    float lp_end = -INFINITY;
    enum { K = 0, B = 1, M = 2 };                                                            /* hmm.c:106-113 */
    for (uint32_t row = 1; row < n_rows; row++) {
        for (uint32_t block = 1; block < n_blocks - 1; block++) {
            const uint32_t kmer_idx = block - 1, po = 3 * (block - 1), co = 3 * block;
            const uint32_t event_idx = e_start + (row - 1) * event_stride;
            const float lp_emission_m = amr_emission(ev[event_idx], scale, shift, var, log_var, model + ranks[kmer_idx]);
            float x[6], sum;
            x[0] = lp_mm_self + prev[co + M];
            x[1] = lp_mm_next + prev[po + M];
            x[2] = lp_bm_self + prev[co + B];
            x[3] = lp_bm_next + prev[po + B];
            x[4] = lp_km + prev[po + K];
            x[5] = (kmer_idx == 0 && (event_idx == e_start || (flags & 1))) ? lp_sm + pre[row - 1] : -INFINITY;
            sum = x[0];
            for (int i = 1; i < 6; ++i) sum = flogsum(sum, x[i], cnt);                       /* hmm.c:558-566 */
            cur[co + M] = sum + lp_emission_m;

            x[0] = lp_mb + prev[co + M]; x[1] = -INFINITY; x[2] = lp_bb + prev[co + B]; x[3] = x[4] = x[5] = -INFINITY;
            sum = x[0];
            for (int i = 1; i < 6; ++i) sum = flogsum(sum, x[i], cnt);
            cur[co + B] = sum + 0.0f;

            x[0] = -INFINITY; x[1] = lp_mk + cur[po + M]; x[2] = -INFINITY; x[3] = lp_bk + cur[po + B]; x[4] = lp_kk + cur[po + K];
            x[5] = -INFINITY;
            sum = x[0];
            for (int i = 1; i < 6; ++i) sum = flogsum(sum, x[i], cnt);
            cur[co + K] = sum + 0.0f;

            if (kmer_idx == last_kmer_idx && ((flags & 2) || row == last_event_row_idx)) {   /* hmm.c:479-487 */
                const float lp1 = lp_ms + cur[co + M] + post[row - 1];
                const float lp2 = lp_ms + cur[co + B] + post[row - 1];
                const float lp3 = lp_ms + cur[co + K] + post[row - 1];
                lp_end = flogsum(lp_end, lp1, cnt);
                lp_end = flogsum(lp_end, lp2, cnt);
                lp_end = flogsum(lp_end, lp3, cnt);
            }
        }
        float *s = prev; prev = cur; cur = s;
    }
    free(rows); free(pre); free(post); free(ranks);
    return lp_end;
}

/* the jobs of a batch; counts[3] += the branches of p7_FLogsum taken */
void amr_score_many(int64_t n_jobs, const job_t *jobs, const char *seq_arena, const int64_t *event_off, const float *event_mean,
                    const float *scale, const float *shift, const float *var, const float *log_var, const double *events_per_base,
                    const model_t *model, float *scores, int64_t *counts, int threads)
{
    int64_t c0 = 0, c1 = 0, c2 = 0;
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads) reduction(+ : c0, c1, c2)
    for (int64_t j = 0; j < n_jobs; ++j) {
        const job_t *J = jobs + j;
        int64_t cnt[3] = {0, 0, 0};
        const int r = J->read;
        scores[j] = amr_score(seq_arena + J->seq_off, seq_arena + J->rc_off, J->seq_len, event_mean + event_off[r], scale[r], shift[r],
                              var[r], log_var[r], model, (uint32_t)J->event_start, (uint32_t)J->event_stop, J->rc, events_per_base[r],
                              (uint32_t)J->flags, cnt);
        c0 += cnt[0]; c1 += cnt[1]; c2 += cnt[2];
    }
    if (counts) { counts[0] += c0; counts[1] += c1; counts[2] += c2; }
}

/* ---------------------------------------------------------------- the planner */

static char possible0(char c)                                                               /* getPossibleSymbols(c)[0], meth.c:221-256 */
{
    switch (c) {
        case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 'A';
        case 'C': case 'S': case 'Y': case 'B': return 'C';
        case 'G': case 'K': return 'G';
        case 'T': return 'T';
        default: return 'A';                              /* not a IUPAC symbol: the reference asserts; here it ranks as A */
    }
}

void amr_disambiguate(const char *in, int64_t n, char *out)                                 /* meth.c:288-306 */
{
    for (int64_t i = 0; i < n; ++i) out[i] = possible0((char)toupper((unsigned char)in[i]));
}

static char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'T'; }   /* meth.c:261-273 */

void amr_reverse_complement(const char *s, int64_t n, char *out)                            /* meth.c:276-286 */
{
    for (int64_t i = 0; i < n; ++i) out[n - 1 - i] = complement(s[i]);
}

void amr_methylate(const char *s, int64_t n, char *out)                                     /* meth.c:359-382, 326-354 */
{
    memcpy(out, s, (size_t)n);
    int64_t i = 0;
    while (i < n) {
        if (i + 1 < n && s[i] == 'C' && s[i + 1] == 'G') { out[i] = 'M'; out[i + 1] = 'G'; i += 2; }
        else i += 1;
    }
}

void amr_reverse_complement_meth(const char *s, int64_t n, char *out)                       /* meth.c:387-420 */
{
    int64_t i = 0, j = n - 1;
    while (i < n) {
        int64_t off = 0, len = 0;
        /* match_to_site(str, i, "MG", 2): the whole string inside the site, or a prefix of the site at i */
        if (i == 0 && n <= 2 && ((n == 2 && s[0] == 'M' && s[1] == 'G') || (n == 1 && (s[0] == 'M' || s[0] == 'G')))) {
            off = (n == 1 && s[0] == 'G') ? 1 : 0; len = n;
        } else {
            const int64_t cl = n - i < 2 ? n - i : 2;
            if (s[i] == 'M' && (cl == 1 || s[i + 1] == 'G')) len = cl;
        }
        int covers = 0;
        for (int64_t k = 0; k < len; ++k) covers |= s[i + k] == 'M';
        if (len > 0 && covers) {
            for (int64_t k = off; k < off + len; ++k) { out[j--] = "GM"[k]; i += 1; }
        } else {
            out[j--] = complement(s[i++]);
        }
    }
}

static int lower_bound(const pair_t *a, int low, int high, int v)                           /* meth.c:422-431 */
{
    while (low < high) {
        const int mid = low + (high - low) / 2;
        if (a[mid].ref_pos < v) low = mid + 1; else high = mid;
    }
    return low;
}

static int find_by_ref_bounds(const pair_t *pairs, int64_t size, int ref_start, int ref_stop, int *read_start, int *read_stop)  /* meth.c:433-467 */
{
    const int start_i = lower_bound(pairs, 0, (int)size, ref_start), stop_i = lower_bound(pairs, 0, (int)size, ref_stop);
    if (start_i == size || stop_i == size) return 0;
    const int left_bounded = pairs[start_i].ref_pos <= ref_start || (start_i != 0 && pairs[start_i - 1].ref_pos <= ref_start);
    /* as written, the second operand compares against ref_start; it is only reached when the first is false, which the
       lower bound rules out, so the entry past the end is never read */
    const int right_bounded = pairs[stop_i].ref_pos >= ref_stop || (stop_i + 1 < size && pairs[stop_i + 1].ref_pos >= ref_start);
    if (left_bounded && right_bounded) { *read_start = pairs[start_i].read_pos; *read_stop = pairs[stop_i].read_pos; return 1; }
    return 0;
}

/* meth.c:501-658 for one read without the BAM record.  Appends to sites / jobs / the string arena; returns the number of
 * sites, or -1 when the record runs against the strand (the reference asserts, hmm.c:322).  With sites == NULL only counts
 * (*seq_bytes grows by the bytes the strings need). */
int64_t amr_sites_read(int32_t read, const char *ref, int64_t ref_len, int32_t ref_start_pos, int rc, const pair_t *rec, int64_t n_rec,
                       site_t *sites, job_t *jobs, char *seq_arena, int64_t *seq_bytes)
{
    if (ref_len < 2 || n_rec == 0) return 0;
    char *ref_seq = malloc((size_t)ref_len);
    amr_disambiguate(ref, ref_len, ref_seq);
    int *cpg = malloc(sizeof(int) * (size_t)ref_len);
    int64_t n_cpg = 0, n_sites = 0;
    for (int64_t i = 0; i < ref_len - 1; ++i)
        if (ref_seq[i] == 'C' && ref_seq[i + 1] == 'G') cpg[n_cpg++] = (int)i;
    const int min_separation = 10;
    int64_t curr = 0;
    while (curr < n_cpg) {
        int64_t end = curr + 1;
        while (end < n_cpg) { if (cpg[end] - cpg[end - 1] > min_separation) break; end += 1; }
        const int64_t start_idx = curr, end_idx = end;
        curr = end;
        const int sub_start_pos = cpg[start_idx] - min_separation, sub_end_pos = cpg[end_idx - 1] + min_separation;
        const int span = cpg[end_idx - 1] - cpg[start_idx];
        if (sub_start_pos <= min_separation || span > 200) continue;
        int64_t L = sub_end_pos - sub_start_pos + 1;                                          /* substr clamps at the end */
        if (L > ref_len - sub_start_pos) L = ref_len - sub_start_pos;
        const int calling_start = sub_start_pos + ref_start_pos, calling_end = sub_end_pos + ref_start_pos;
        int e1 = 0, e2 = 0;
        const int bounded = find_by_ref_bounds(rec, n_rec, calling_start, calling_end, &e1, &e2);
        if (!bounded) continue;
        const double ratio = fabs((double)(e2 - e1)) / (calling_start - calling_end);         /* negative: never above 20 */
        if (abs(e2 - e1) <= 10 || ratio > 20) continue;
        if ((e1 <= e2) == (rc != 0)) { free(ref_seq); free(cpg); return -1; }
        if (sites) {
            char *sub = seq_arena + *seq_bytes, *rcs = sub + L, *msub = rcs + L, *mrc = msub + L;
            memcpy(sub, ref_seq + sub_start_pos, (size_t)L);
            amr_reverse_complement(sub, L, rcs);
            amr_methylate(sub, L, msub);
            amr_reverse_complement_meth(msub, L, mrc);
            site_t *S = sites + n_sites;
            S->read = read; S->start_position = cpg[start_idx] + ref_start_pos; S->end_position = cpg[end_idx - 1] + ref_start_pos;
            S->n_cpg = (int32_t)(end_idx - start_idx);
            const int64_t o0 = cpg[start_idx] - KMER + 1, o1 = cpg[end_idx - 1] + KMER;
            S->ctx_off = o0; S->ctx_len = (int32_t)((o1 < ref_len ? o1 : ref_len) - o0); S->pad_ = 0;
            for (int m = 0; m < 2; ++m) {
                job_t *J = jobs + 2 * n_sites + m;
                J->seq_off = *seq_bytes + 2 * m * L; J->rc_off = J->seq_off + L; J->seq_len = (int32_t)L; J->read = read;
                J->event_start = e1; J->event_stop = e2; J->rc = rc ? 1 : 0; J->flags = 3;
            }
        }
        *seq_bytes += 4 * L;
        n_sites++;
    }
    free(ref_seq); free(cpg);
    return n_sites;
}
