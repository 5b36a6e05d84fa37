/* bsw_lane_windows.c — replays the windows of bsw_lane_kernel's lock-step rows on the CPU (scripts/bsw_lane_windows.py).
 *
 * One chunk = up to 64 pairs that a wavefront runs together.  Every pair follows oracle/bsw_oracle.c's row loop
 * (scalarBandedSWA) exactly; the rows of the chunk run in lock-step, and each row is accounted for in four ways:
 *   st[0] cells the lanes compute (sum of the windows of the lanes still running)
 *   st[1] 64 x the widest window                              (what the LDS lane kernel pays: a lane walks its own window)
 *   st[2] 64 x 2 x the column pairs from the lowest beg to the highest end   (column lock-step at pair granularity)
 *   st[3] 64 x 8 x the 8-column blocks from the lowest beg to the highest end (column lock-step at block granularity)
 *   st[4] blocks of st[3] / 512           st[5] of them, blocks some running lane covers only in part (masked variant)
 *   st[6] rows the wavefront runs         st[7] lane rows (pairs x their rows)
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline int imax(int a, int b) { return a > b ? a : b; }
static inline int imin(int a, int b) { return a < b ? a : b; }

typedef struct {
    int qlen, tlen, beg, end, w, best, best_i, best_j, h0, done;
    const uint8_t *q, *t;
    int32_t hd[1024], ev[1024];
} Lane;

void lane_windows(const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins, int zdrop, int end_bonus, int wband,
                  int64_t count, const int32_t *order, const uint8_t *ref, const uint8_t *qer, const int64_t *idr,
                  const int64_t *idq, const int32_t *len1, const int32_t *len2, const int32_t *h0v, double *st)
{
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    int mx = 0;
    for (int k = 0; k < 25; ++k) mx = imax(mx, mat[k]);
    Lane *L = (Lane *)malloc(64 * sizeof(Lane));
    for (int64_t hi = count; hi > 0; hi -= 64) {          /* chunks from the end of the sorted list, as the kernel takes them */
        const int64_t lo = hi - 64 > 0 ? hi - 64 : 0;
        const int nl = (int)(hi - lo);
        for (int l = 0; l < nl; ++l) {
            Lane *a = &L[l];
            const int k = order[lo + l];
            a->qlen = len2[k]; a->tlen = len1[k]; a->h0 = h0v[k];
            a->q = qer + idq[k]; a->t = ref + idr[k];
            memset(a->hd, 0, sizeof(int32_t) * (a->qlen + 2));
            memset(a->ev, 0, sizeof(int32_t) * (a->qlen + 2));
            a->hd[0] = a->h0;
            if (a->qlen >= 1) a->hd[1] = a->h0 > oe_ins ? a->h0 - oe_ins : 0;
            for (int j = 2; j <= a->qlen && a->hd[j - 1] > e_ins; ++j) a->hd[j] = a->hd[j - 1] - e_ins;
            int w = wband;
            int lim = (int)((double)(a->qlen * mx + end_bonus - o_ins) / e_ins + 1.);
            w = imin(w, imax(lim, 1));
            lim = (int)((double)(a->qlen * mx + end_bonus - o_del) / e_del + 1.);
            a->w = imin(w, imax(lim, 1));
            a->best = a->h0; a->best_i = -1; a->best_j = -1;
            a->beg = 0; a->end = a->qlen; a->done = a->tlen <= 0;
        }
        for (int i = 0;; ++i) {
            int running = 0, lo_b = 1 << 20, hi_e = -1, widest = 0;
            int wb[64], we[64];
            for (int l = 0; l < nl; ++l) {
                Lane *a = &L[l];
                wb[l] = 0; we[l] = 0;
                if (a->done) continue;
                ++running;
                if (a->beg < i - a->w) a->beg = i - a->w;
                if (a->end > i + a->w + 1) a->end = i + a->w + 1;
                if (a->end > a->qlen) a->end = a->qlen;
                wb[l] = a->beg; we[l] = imax(a->end, a->beg);
                if (we[l] > wb[l]) { lo_b = imin(lo_b, wb[l]); hi_e = imax(hi_e, we[l]); }
                widest = imax(widest, we[l] - wb[l]);
                st[0] += we[l] - wb[l];
            }
            if (!running) break;
            st[1] += 64.0 * widest;
            st[6] += 1; st[7] += running;
            if (hi_e > lo_b) {
                st[2] += 64.0 * 2 * (((hi_e - 1) >> 1) - (lo_b >> 1) + 1);
                const int b0 = lo_b >> 3, b1 = (hi_e - 1) >> 3;
                st[3] += 64.0 * 8 * (b1 - b0 + 1);
                st[4] += b1 - b0 + 1;
                for (int b = b0; b <= b1; ++b) {
                    int part = 0;
                    for (int l = 0; l < nl && !part; ++l)
                        if (!L[l].done && !(wb[l] <= 8 * b && we[l] >= 8 * b + 8)) part = 1;
                    st[5] += part;
                }
            }
            /* the row itself, oracle/bsw_oracle.c */
            for (int l = 0; l < nl; ++l) {
                Lane *a = &L[l];
                if (a->done) continue;
                const int8_t *srow = &mat[a->t[i] * 5];
                int f = 0, row_best = 0, row_arg = -1, left, j;
                left = a->beg == 0 ? imax(a->h0 - (o_del + e_del * (i + 1)), 0) : 0;
                for (j = a->beg; j < a->end; ++j) {
                    const int diag = a->hd[j], e = a->ev[j];
                    a->hd[j] = left;
                    const int m = diag ? diag + srow[a->q[j]] : 0;
                    const int h = imax(imax(m, e), f);
                    left = h;
                    if (h >= row_best) row_arg = j;
                    row_best = imax(row_best, h);
                    a->ev[j] = imax(e - e_del, imax(m - oe_del, 0));
                    f = imax(f - e_ins, imax(m - oe_ins, 0));
                }
                a->hd[a->end] = left; a->ev[a->end] = 0;
                int stop = row_best == 0;
                if (!stop) {
                    if (row_best > a->best) { a->best = row_best; a->best_i = i; a->best_j = row_arg; }
                    else if (zdrop > 0) {
                        const int di = i - a->best_i, dj = row_arg - a->best_j;
                        stop = di > dj ? a->best - row_best - (di - dj) * e_del > zdrop : a->best - row_best - (dj - di) * e_ins > zdrop;
                    }
                }
                if (!stop) {
                    for (j = a->beg; j < a->end && a->hd[j] == 0 && a->ev[j] == 0; ++j) {}
                    a->beg = j;
                    for (j = a->end; j >= a->beg && a->hd[j] == 0 && a->ev[j] == 0; --j) {}
                    a->end = imin(j + 2, a->qlen);
                }
                a->done = stop || i + 1 >= a->tlen;
            }
        }
    }
    free(L);
}
