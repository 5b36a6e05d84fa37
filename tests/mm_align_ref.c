/* C twin of tests/mm_align_ref.py's dp_job: one DP job of DESIGN 3.20 on full matrices, for the sizes Python cannot do in a few
 * seconds.  Sequential and plain: every cell of the (tl + 1) x (ql + 1) matrices exists, the band is a test per cell. */
#include <stdint.h>
#include <stdlib.h>

typedef struct { int32_t a, b, sc_ambi, q, e, q2, e2, bw, zdrop, end_bonus, min_ksw_len, max_ext; } mar_params;

#define NEG (-0x40000000)
static int32_t dec(int32_t x, int32_t c) { return x <= NEG / 2 ? NEG : x - c; }
static int32_t gap(const mar_params *P, int32_t l) { const int32_t a = P->q + P->e * l, b = P->q2 + P->e2 * l; return a < b ? a : b; }
static int32_t sc(const mar_params *P, int t, int c) { return t > 3 || c > 3 ? -P->sc_ambi : t == c ? P->a : -P->b; }
static int in_band(int t, int j, int w) { const int r = t + j; return ((r - w + 1) >> 1) <= t && t <= ((r + w) >> 1); }

/* T, Q: codes 0..4.  mode 0 LEFT, 1 RIGHT; ext 0 global, 1 extension.
 * out[8] = score, end_t, end_q (-1: empty), z-dropped, reach_end, consumed target, consumed query, saved-by-l.
 * ops: (op, len) pairs in the job's direction, at most cap pairs -> their number, -1: out of memory. */
int64_t mar_job(const mar_params *P, const uint8_t *T, int32_t tl, const uint8_t *Q, int32_t ql, int32_t w, int mode, int ext, int32_t *out,
                int32_t *ops, int64_t cap)
{
    const int64_t W = (int64_t)ql + 1, n = ((int64_t)tl + 1) * W;
    int32_t *H = malloc(n * 4), *G[4];
    uint8_t *D = calloc(n, 1);
    for (int k = 0; k < 4; ++k) G[k] = malloc(n * 4);
    if (!H || !D || !G[0] || !G[1] || !G[2] || !G[3]) return -1;
    if (w > tl + ql) w = tl + ql;
#define AT(t, j) (((int64_t)(t) + 1) * W + (j) + 1)
    for (int64_t i = 0; i < n; ++i) H[i] = G[0][i] = G[1][i] = G[2][i] = G[3][i] = NEG;
    H[AT(-1, -1)] = 0;
    for (int j = 0; j < ql; ++j) H[AT(-1, j)] = -gap(P, j + 1);
    for (int t = 0; t < tl; ++t) H[AT(t, -1)] = -gap(P, t + 1);
    const int32_t pq[4] = {P->q, P->q, P->q2, P->q2}, pe[4] = {P->e, P->e, P->e2, P->e2};
    int32_t mx = 0, mx_t = -1, mx_q = -1, mqe = NEG, mqe_t = -1, zdropped = 0, worst = 0;
    for (int r = 0; r < tl + ql - 1 && !zdropped; ++r) {
        int32_t best = NEG, bt = -1, any = 0;
        for (int t = r - ql + 1 > 0 ? r - ql + 1 : 0; t <= r && t < tl; ++t) {
            const int j = r - t;
            if (!in_band(t, j, w)) continue;
            int32_t st[4], fl = 0;
            for (int k = 0; k < 4; ++k) {
                const int pt = k & 1 ? t : t - 1, pj = k & 1 ? j - 1 : j;
                const int32_t opened = dec(H[AT(pt, pj)], pq[k]), cont = pt < 0 || pj < 0 ? NEG : G[k][AT(pt, pj)];
                if (pt >= 0 && pj >= 0 && (mode ? cont >= opened : cont > opened)) fl |= 1 << k;
                st[k] = dec(opened > cont ? opened : cont, pe[k]);
            }
            int32_t z = H[AT(t - 1, j - 1)] <= NEG / 2 ? NEG : H[AT(t - 1, j - 1)] + sc(P, T[t], Q[j]), d = 0;
            for (int k = 0; k < 4; ++k)
                if (mode ? st[k] >= z : st[k] > z) { z = st[k]; d = k + 1; }
            H[AT(t, j)] = z;
            for (int k = 0; k < 4; ++k) G[k][AT(t, j)] = st[k];
            D[AT(t, j)] = (uint8_t)(d | fl << 3);
            if (!any || z > best) { best = z; bt = t; any = 1; }
            if (j == ql - 1 && z > mqe) { mqe = z; mqe_t = t; }
        }
        if (!ext || !any) continue;
        if (best > mx) { mx = best; mx_t = bt; mx_q = r - bt; }
        else if (bt >= mx_t && r - bt >= mx_q) {
            const int32_t l = abs((bt - mx_t) - ((r - bt) - mx_q));
            if (P->zdrop >= 0 && (int64_t)mx - best > (int64_t)P->zdrop + (int64_t)l * P->e2) zdropped = 1;
            else if (mx - best > worst) worst = mx - best;
        }
    }
    int32_t et, eq, score, reach = 0;
    if (!ext) { et = tl - 1; eq = ql - 1; score = H[AT(et, eq)]; }
    else if (!zdropped && mqe > NEG / 2 && (int64_t)mqe + P->end_bonus > mx) { et = mqe_t; eq = ql - 1; score = mqe; reach = 1; }
    else if (mx_t >= 0) { et = mx_t; eq = mx_q; score = mx; }
    else { et = eq = -1; score = 0; }
    /* the walk, one operation a step, then reversed and merged */
    int64_t n_ops = 0, len = 0;
    uint8_t *one = malloc((size_t)tl + ql + 2);
    if (!one) return -1;
    if (et >= 0) {
        int i = et, j = eq, state = 0;
        while (i >= 0 && j >= 0) {
            const int b = D[AT(i, j)];
            if (state == 0) state = b & 7;
            if (state == 0) { one[len++] = 0; --i; --j; }
            else if (state == 1 || state == 3) { one[len++] = 2; --i; if (!(b >> (2 + state) & 1)) state = 0; }
            else { one[len++] = 1; --j; if (!(b >> (2 + state) & 1)) state = 0; }
        }
        for (; i >= 0; --i) one[len++] = 2;
        for (; j >= 0; --j) one[len++] = 1;
    }
    for (int64_t k = len - 1; k >= 0; --k) {
        if (n_ops && ops[2 * (n_ops - 1)] == one[k]) { ++ops[2 * (n_ops - 1) + 1]; continue; }
        if (n_ops < cap) { ops[2 * n_ops] = one[k]; ops[2 * n_ops + 1] = 1; }
        ++n_ops;
    }
    out[0] = score; out[1] = et; out[2] = eq; out[3] = zdropped; out[4] = reach; out[5] = et + 1; out[6] = eq + 1;
    out[7] = ext && !zdropped && P->zdrop >= 0 && worst > P->zdrop;
    free(H); free(D); free(one);
    for (int k = 0; k < 4; ++k) free(G[k]);
    return n_ops;
}
