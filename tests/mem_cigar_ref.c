/* C twin of tests/mem_cigar_ref.py (the rolling form of the global alignment): the rules of gbx_mem_cigar_*  for
 * inputs the Python form is too slow for.  Test infrastructure, built by mem_cigar_ref.py on first use; the CPU tests hold it
 * against the Python forms on every hand-built case. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MCR_INF (-0x40000000)

typedef struct { int32_t mat[25], o_del, e_del, o_ins, e_ins, w; } mcr_params;
typedef struct { int64_t qoff, roff; int32_t lq, rlen, qbeg, rbeg, len, pad_; } mcr_seed;
typedef struct { int32_t score, truesc, qb, qe, rb, re, w, sc0; } mcr_result;
typedef struct { int64_t pos, cigar_off; int32_t rid, is_rev, n_cigar, nm, score, w, tries, pad_; } mcr_aln;
typedef struct { uint32_t *v; int n, cap; } mcr_ops;      /* len << 4 | op, M 0, I 1, D 2 */

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

static void push(mcr_ops *o, int op, int n)
{
    if (o->n && (int)(o->v[o->n - 1] & 15) == op) { o->v[o->n - 1] += (uint32_t)n << 4; return; }
    if (o->n == o->cap) { o->cap = o->cap ? 2 * o->cap : 16; o->v = realloc(o->v, (size_t)o->cap * 4); }
    o->v[o->n++] = (uint32_t)n << 4 | (uint32_t)op;
}

static int infer_bw(int l1, int l2, int score, int a, int q, int e)
{
    if (l1 == l2 && l1 * a - score < (q + e - a) * 2) return 0;
    int w = (int)((double)(imin(l1, l2) * a - score - q) / e + 2.);
    return imax(w, abs(l1 - l2));
}

/* ksw_global2; the ops come out last to first */
static int global(const mcr_params *p, int lQ, const uint8_t *Q, int lT, const uint8_t *T, int w, mcr_ops *ops)
{
    const int oe_del = p->o_del + p->e_del, oe_ins = p->o_ins + p->e_ins, n_col = imin(lQ, 2 * w + 1);
    int32_t *H = malloc((size_t)(lQ + 1) * 4), *E = malloc((size_t)(lQ + 1) * 4);
    uint8_t *z = malloc((size_t)n_col * (size_t)lT);
    for (int j = 0; j <= lQ; ++j) { H[j] = MCR_INF; E[j] = MCR_INF; }
    H[0] = 0;
    for (int j = 1; j <= lQ && j <= w; ++j) H[j] = -(p->o_ins + p->e_ins * j);
    for (int i = 0; i < lT; ++i) {
        const int beg = imax(i - w, 0), end = imin(i + w + 1, lQ);
        int32_t h1 = beg == 0 ? -(p->o_del + p->e_del * (i + 1)) : MCR_INF, f = MCR_INF;
        uint8_t *zi = z + (size_t)i * n_col;
        for (int j = beg; j < end; ++j) {
            const int32_t m = H[j] + p->mat[T[i] * 5 + Q[j]];
            int32_t e = E[j], h, t;
            uint8_t d;
            H[j] = h1;
            d = m >= e ? 0 : 1; h = m >= e ? m : e;
            d = h >= f ? d : 2; h = h >= f ? h : f;
            h1 = h;
            t = m - oe_del; e -= p->e_del; d |= e > t ? 1 << 2 : 0; E[j] = e > t ? e : t;
            t = m - oe_ins; f -= p->e_ins; d |= f > t ? 2 << 4 : 0; f = f > t ? f : t;
            zi[j - beg] = d;
        }
        H[end] = h1; E[end] = MCR_INF;
    }
    const int score = H[lQ];
    int i = lT - 1, k = imin(i + w + 1, lQ) - 1, which = 0;
    while (i >= 0 && k >= 0) {
        which = z[(size_t)i * n_col + (k - imax(i - w, 0))] >> (which << 1) & 3;
        if (which == 0) { push(ops, 0, 1); --i; --k; }
        else if (which == 1) { push(ops, 2, 1); --i; }
        else { push(ops, 1, 1); --k; }
    }
    if (i >= 0) push(ops, 2, i + 1);
    if (k >= 0) push(ops, 1, k + 1);
    free(H); free(E); free(z);
    return score;
}

static int gen(const mcr_params *p, int lQ, const uint8_t *Q, int lT, const uint8_t *T, int w_, mcr_ops *ops)
{
    ops->n = 0;
    if (lQ == lT && w_ == 0) {
        int s = 0;
        for (int j = 0; j < lQ; ++j) s += p->mat[T[j] * 5 + Q[j]];
        push(ops, 0, lQ);
        return s;
    }
    const int a = p->mat[0];
    const int max_ins = (int)((double)(((lQ + 1) >> 1) * a - p->o_ins) / p->e_ins + 1.);
    const int max_del = (int)((double)(((lQ + 1) >> 1) * a - p->o_del) / p->e_del + 1.);
    const int g = imax(imax(max_ins, max_del), 1), d = abs(lT - lQ);
    int wb = (g + d + 1) >> 1;
    wb = imin(wb, w_);
    wb = imax(wb, d + 3);
    const int score = global(p, lQ, Q, lT, T, wb, ops);
    for (int x = 0, y = ops->n - 1; x < y; ++x, --y) { const uint32_t t = ops->v[x]; ops->v[x] = ops->v[y]; ops->v[y] = t; }
    return score;
}

/* -> the number of CIGAR words (those past cigar_cap are not written) */
int64_t mcr_run(const mcr_params *p, int64_t n, const mcr_seed *seeds, const mcr_result *res, const uint8_t *text, int64_t text_bytes,
                const uint8_t *qer, int64_t qer_bytes, int64_t L, int32_t n_contigs, const int64_t *contig_off, mcr_aln *alns,
                uint32_t *cigar, int64_t cigar_cap)
{
    int64_t total = 0;
    mcr_ops ops = {0, 0, 0};
    const int a = p->mat[0];
    for (int64_t k = 0; k < n; ++k) {
        const mcr_seed s = seeds[k];
        const mcr_result r = res[k];
        mcr_aln *o = alns + k;
        memset(o, 0, sizeof(*o));
        o->rid = -1; o->cigar_off = total;
        const int64_t rb = s.roff + r.rb, re = s.roff + r.re, tend = text_bytes < 2 * L ? text_bytes : 2 * L;
        const int qb = r.qb, qe = r.qe, lq = s.lq;
        if (qb < 0 || qe <= qb || rb >= re || (rb < L && L < re)) continue;
        if (lq < 0 || s.qoff < 0 || s.qoff + lq > qer_bytes || qe > lq || rb < 0 || re > tend) continue;
        const int lQ = qe - qb, lT = (int)(re - rb), is_rev = rb >= L;
        uint8_t *Q = malloc((size_t)lQ), *T = malloc((size_t)lT);
        for (int j = 0; j < lQ; ++j) { const uint8_t c = qer[s.qoff + (is_rev ? qe - 1 - j : qb + j)]; Q[j] = c > 4 ? 4 : c; }
        for (int i = 0; i < lT; ++i) { const uint8_t c = text[is_rev ? re - 1 - i : rb + i]; T[i] = c > 4 ? 4 : c; }
        int w2 = imax(infer_bw(lQ, lT, r.truesc, a, p->o_del, p->e_del), infer_bw(lQ, lT, r.truesc, a, p->o_ins, p->e_ins));
        if (w2 > p->w) w2 = imin(w2, r.w);
        int last = -(1 << 30), score = 0, tries = 0, used = 0;
        for (int i = 0; i < 3; ++i) {
            w2 = imin(w2, 4 * p->w);
            score = gen(p, lQ, Q, lT, T, w2, &ops);
            ++tries; used = w2;
            if (score == last || w2 == 4 * p->w) break;
            last = score;
            w2 *= 2;
            if (!(i + 1 < 3 && score < r.truesc - a)) break;
        }
        int nm = 0, x = 0, y = 0;
        for (int c = 0; c < ops.n; ++c) {
            const int op = ops.v[c] & 15, ln = (int)(ops.v[c] >> 4);
            if (op == 0) { for (int d = 0; d < ln; ++d) nm += Q[x + d] != T[y + d]; x += ln; y += ln; }
            else if (op == 1) { nm += ln; x += ln; }
            else { if (c > 0 && c < ops.n - 1) nm += ln; y += ln; }
        }
        int64_t pos = is_rev ? 2 * L - re : rb;
        int first = 0, end = ops.n;
        if ((ops.v[0] & 15) == 2) { pos += ops.v[0] >> 4; first = 1; }
        else if ((ops.v[end - 1] & 15) == 2) --end;
        int rid = 0;
        for (int c = 0; c < n_contigs; ++c) if (contig_off[c] <= pos) rid = c;
        const int clip5 = is_rev ? lq - qe : qb, clip3 = is_rev ? qb : lq - qe;
        int64_t at = total;
        if (clip5) { if (at < cigar_cap) cigar[at] = (uint32_t)clip5 << 4 | 4; ++at; }
        for (int c = first; c < end; ++c, ++at) if (at < cigar_cap) cigar[at] = ops.v[c];
        if (clip3) { if (at < cigar_cap) cigar[at] = (uint32_t)clip3 << 4 | 4; ++at; }
        o->pos = pos - contig_off[rid]; o->rid = rid; o->is_rev = is_rev; o->n_cigar = (int32_t)(at - total); o->nm = nm;
        o->score = score; o->w = used; o->tries = tries;
        total = at;
        free(Q); free(T);
    }
    free(ops.v);
    return total;
}
