// mm_align_rules.h — base-level alignment of minimap2's regions: the breakpoints of a region (planning), the
// two-piece affine DP of one job with its z-drop bookkeeping, the walk back, and a region's CIGAR, statistics and record.  One
// text for the device (mm_align_kernels.hip: a wavefront per job and per region) and for a plain C++ build on the host
// (shims/mm_align_cpu_twin.cpp, one thread), which the CPU tests hold against the restatement tests/mm_align_ref.py.
//
// A function takes a team T as mm_map_rules.h does: lane() of size() lanes, sync() a barrier that makes the team's stores visible
// to it, and max_key(k): the largest k any lane passed, in every lane.  On the host the team is one lane.
//
// A job's room (MmAlnJob::z_at of the caller's z bytes): eleven rows of M ints (H of three antidiagonals, E F E2 F2 of two,
// indexed by t & (M - 1), M the power of two that holds a diagonal's band and three more), then one direction byte a cell,
// antidiagonal r at r * S, S = min(w + 1, tl, ql) the most cells a diagonal has.  A neighbour is read only where the band
// rule says it exists, so what an older diagonal left in a row is never seen.  The caller may hand the DP other memory for the
// rows (the device: LDS, when M fits); the room keeps its layout either way.
#pragma once
#include <cstdint>
#include "mm_machine.h"
#include "mm_map_rules.h"
#include "../../include/gbx.h"

namespace gbx {

constexpr int32_t MMA_NEG = -0x40000000, MMA_NEG_LIM = -0x20000000;      // minus infinity, and everything below this is it
constexpr int MMA_LEFT = 0, MMA_RIGHT = 1;
constexpr int MMA_KIND_LEFT = 0, MMA_KIND_FILL = 1, MMA_KIND_RIGHT = 2;
constexpr int MMA_ROWS = 11;

struct MmAlnSolo {
    int lane() const { return 0; }
    int size() const { return 1; }
    void sync() const {}
    int64_t max_key(int64_t k) const { return k; }
};

// one job: a window of the target and of the oriented query; a left extension reads both backwards
struct MmAlnJob {
    int64_t z_at;                                  // its room in z
    int32_t reg, kind;
    int32_t t0, q0, tl, ql;                        // the windows [t0, t0 + tl) of the contig, [q0, q0 + ql) of Qs
    int32_t w, skip;                               // band; skip: the region is not aligned
    // results
    int32_t score, ct, cq;                         // consumed target and query bases
    int32_t n_ops, first_op, first_len, last_op;   // its runs in forward order
    int32_t flags;                                 // 1: z-dropped, 2: reached the query end
    int32_t end_t, end_q;                          // the end cell (-1: empty)
    int32_t w_at, merge;                           // its first word within the region's CIGAR; merge: that word is the job before's last
};

struct MmAlnSeq {                                  // a region's texts: the contig and the read as the anchors see it
    const uint8_t *t, *q;
    int32_t tlen, qlen, rev;
    GBX_MM_HD int tc(int32_t i) const { return mm_code(t[i]); }
    GBX_MM_HD int qc(int32_t j) const
    {
        if (!rev) return mm_code(q[j]);
        const int c = mm_code(q[qlen - 1 - j]);
        return c < 4 ? 3 - c : 4;
    }
};

GBX_MM_HD inline int32_t mma_gap(const gbx_mm_align_params &P, int32_t l)
{
    const int64_t a = (int64_t)P.q + (int64_t)P.e * l, b = (int64_t)P.q2 + (int64_t)P.e2 * l, m = a < b ? a : b;
    return (int32_t)(m < 0x3fffffff ? m : 0x3fffffff);
}
GBX_MM_HD inline int32_t mma_sc(const gbx_mm_align_params &P, int t, int c) { return t > 3 || c > 3 ? -P.sc_ambi : t == c ? P.a : -P.b; }
GBX_MM_HD inline int32_t mma_sub(int32_t x, int32_t c) { return x <= MMA_NEG_LIM ? MMA_NEG : x - c; }

// the band a job runs with: anything at least tl + ql wide holds every cell
GBX_MM_HD inline int32_t mma_band(int64_t w, int32_t tl, int32_t ql) { const int64_t all = (int64_t)tl + ql; return (int32_t)(w < all ? w : all); }
GBX_MM_HD inline int32_t mma_stride(int32_t w, int32_t tl, int32_t ql) { const int32_t m = tl < ql ? tl : ql; return w + 1 < m ? w + 1 : m; }
GBX_MM_HD inline int32_t mma_ring(int32_t w, int32_t tl)
{
    const int32_t need = (w + 1 < tl ? w + 1 : tl) + 3;
    int32_t m = 4;
    for (int i = 0; i < 30 && m < need; ++i) m <<= 1;
    return m;
}
// the bytes of z a job takes, a multiple of 16; tl, ql >= 1
GBX_MM_HD inline int64_t mma_job_bytes(int32_t w, int32_t tl, int32_t ql)
{
    const int64_t b = (int64_t)MMA_ROWS * 4 * mma_ring(w, tl) + ((int64_t)tl + ql - 1) * mma_stride(w, tl, ql);
    return (b + 15) & ~(int64_t)15;
}
// the cells of antidiagonal r: t in [*st, *en]
GBX_MM_HD inline void mma_diag(int32_t r, int32_t w, int32_t tl, int32_t ql, int32_t *st, int32_t *en)
{
    int32_t s = (r - w + 1) >> 1, e = (r + w) >> 1;
    if (s < 0) s = 0;
    if (s < r - ql + 1) s = r - ql + 1;
    if (e > tl - 1) e = tl - 1;
    if (e > r) e = r;
    *st = s; *en = e;
}

struct MmAlnView {                                 // a job's sequences as the DP indexes them
    MmAlnSeq S; int32_t t0, q0, tl, ql, back;
    GBX_MM_HD int tc(int32_t i) const { return S.tc(back ? t0 + tl - 1 - i : t0 + i); }
    GBX_MM_HD int qc(int32_t j) const { return S.qc(back ? q0 + ql - 1 - j : q0 + j); }
};

// ---- the DP of one job (tl, ql >= 1).  ext: extension bookkeeping and end cell, else global.  Lane 0 writes J's score, flags and
// end cell; every lane returns alike.
template <class T>
GBX_MM_HD inline void mm_aln_dp(const T &tm, const gbx_mm_align_params &P, const MmAlnView &V, int mode, bool ext, uint8_t *room, int32_t *rows,
                                MmAlnJob *J)
{
    const int32_t tl = V.tl, ql = V.ql, w = J->w, M = mma_ring(w, tl), mask = M - 1, S = mma_stride(w, tl, ql);
    uint8_t *dir = room + (size_t)MMA_ROWS * 4 * M;
    const bool right = mode == MMA_RIGHT;
    int32_t mx = 0, mx_t = -1, mx_q = -1, mqe = MMA_NEG, mqe_t = -1, zdropped = 0, last_h = MMA_NEG;
    const int32_t n_diag = tl + ql - 1;
    for (int32_t r = 0; r < n_diag; ++r) {
        int32_t st, en;
        mma_diag(r, w, tl, ql, &st, &en);
        if (st > en) break;                                            // an empty diagonal: every later one is empty too
        int32_t *Hc = rows + (r % 3) * M, *H1 = rows + ((r + 2) % 3) * M, *H2 = rows + ((r + 1) % 3) * M;
        int32_t *Gc = rows + (3 + 4 * (r & 1)) * M, *G1 = rows + (3 + 4 * ((r & 1) ^ 1)) * M;      // E, F, E2, F2 rows
        int32_t s1, e1;
        mma_diag(r - 1, w, tl, ql, &s1, &e1);                          // r - 1 < 0: never asked
        int64_t key = INT64_MIN;
        for (int32_t t = st + tm.lane(); t <= en; t += tm.size()) {
            const int32_t j = r - t;
            // neighbours: up (t - 1, j) and left (t, j - 1) on r - 1, diagonal (t - 1, j - 1) on r - 2 (always in the band)
            int32_t hd, hu, eu, e2u, hl, fl, f2l;
            const bool ub = t == 0, lb = j == 0;
            if (ub) { hu = -mma_gap(P, j + 1); eu = e2u = MMA_NEG; }
            else if (t - 1 >= s1 && t - 1 <= e1) { const int32_t k = (t - 1) & mask; hu = H1[k]; eu = G1[k]; e2u = G1[2 * M + k]; }
            else hu = eu = e2u = MMA_NEG;
            if (lb) { hl = -mma_gap(P, t + 1); fl = f2l = MMA_NEG; }
            else if (t >= s1 && t <= e1) { const int32_t k = t & mask; hl = H1[k]; fl = G1[M + k]; f2l = G1[3 * M + k]; }
            else hl = fl = f2l = MMA_NEG;
            if (ub && lb) hd = 0;
            else if (ub) hd = -mma_gap(P, j);
            else if (lb) hd = -mma_gap(P, t);
            else hd = H2[(t - 1) & mask];
            const int32_t oe = mma_sub(hu, P.q), oe2 = mma_sub(hu, P.q2), of = mma_sub(hl, P.q), of2 = mma_sub(hl, P.q2);
            const bool ce = !ub && (right ? eu >= oe : eu > oe), ce2 = !ub && (right ? e2u >= oe2 : e2u > oe2);
            const bool cf = !lb && (right ? fl >= of : fl > of), cf2 = !lb && (right ? f2l >= of2 : f2l > of2);
            const int32_t E = mma_sub(oe > eu ? oe : eu, P.e), E2 = mma_sub(oe2 > e2u ? oe2 : e2u, P.e2);
            const int32_t F = mma_sub(of > fl ? of : fl, P.e), F2 = mma_sub(of2 > f2l ? of2 : f2l, P.e2);
            int32_t z = hd <= MMA_NEG_LIM ? MMA_NEG : hd + mma_sc(P, V.tc(t), V.qc(j)), d = 0;
            if (right ? E >= z : E > z) { z = E; d = 1; }
            if (right ? F >= z : F > z) { z = F; d = 2; }
            if (right ? E2 >= z : E2 > z) { z = E2; d = 3; }
            if (right ? F2 >= z : F2 > z) { z = F2; d = 4; }
            const int32_t k = t & mask;
            Hc[k] = z; Gc[k] = E; Gc[M + k] = F; Gc[2 * M + k] = E2; Gc[3 * M + k] = F2;
            dir[(size_t)r * S + (t - st)] = (uint8_t)(d | ce << 3 | cf << 4 | ce2 << 5 | cf2 << 6);
            const int64_t kk = (int64_t)z * 4294967296ll + (0x7fffffff - t);          // the largest H, then the smallest t
            if (kk > key) key = kk;
        }
        tm.sync();
        if (ext) {
            key = tm.max_key(key);
            const int32_t bt = 0x7fffffff - (int32_t)(key & 0xffffffffll), best = (int32_t)((key - (key & 0xffffffffll)) / 4294967296ll);
            const int32_t te = r - ql + 1;
            if (te >= st && te <= en) { const int32_t h = Hc[te & mask]; if (h > mqe) { mqe = h; mqe_t = te; } }
            if (best > mx) { mx = best; mx_t = bt; mx_q = r - bt; }
            else if (bt >= mx_t && r - bt >= mx_q) {
                const int32_t dt = bt - mx_t, dq = (r - bt) - mx_q, l = dt > dq ? dt - dq : dq - dt;
                if (P.zdrop >= 0 && (int64_t)mx - best > (int64_t)P.zdrop + (int64_t)l * P.e2) { zdropped = 1; break; }
            }
        } else if (r == n_diag - 1) last_h = Hc[(tl - 1) & mask];
    }
    if (tm.lane() == 0) {
        if (!ext) { J->score = last_h; J->end_t = tl - 1; J->end_q = ql - 1; J->flags = 0; }
        else if (!zdropped && mqe > MMA_NEG_LIM && (int64_t)mqe + P.end_bonus > mx) { J->score = mqe; J->end_t = mqe_t; J->end_q = ql - 1; J->flags = 2; }
        else if (mx_t >= 0) { J->score = mx; J->end_t = mx_t; J->end_q = mx_q; J->flags = zdropped; }
        else { J->score = 0; J->end_t = J->end_q = -1; J->flags = zdropped; }
    }
    tm.sync();
}

// ---- the walk from a job's end cell: emit(op, len) a run at a time in walk order (the reverse of the job's own direction),
// equal neighbours merged.  At most tl + ql steps.
template <class Emit>
GBX_MM_HD inline void mm_aln_walk(const MmAlnJob &J, const uint8_t *room, Emit &emit)
{
    const int32_t tl = J.tl, ql = J.ql, w = J.w, M = mma_ring(w, tl), S = mma_stride(w, tl, ql);
    const uint8_t *dir = room + (size_t)MMA_ROWS * 4 * M;
    int32_t i = J.end_t, j = J.end_q, state = 0, op = -1, len = 0;
    auto put = [&](int32_t o, int32_t l) {
        if (l <= 0) return;
        if (o == op) { len += l; return; }
        if (len > 0) emit(op, len);
        op = o; len = l;
    };
    for (int64_t step = 0, most = (int64_t)tl + ql; step < most && i >= 0 && j >= 0; ++step) {
        int32_t st, en;
        mma_diag(i + j, w, tl, ql, &st, &en);
        const int b = i >= st && i <= en ? dir[(size_t)(i + j) * S + (i - st)] : 0;
        if (state == 0) state = b & 7;
        if (state < 1 || state > 4) { state = 0; put(0, 1); --i; --j; }
        else if (state == 1 || state == 3) { put(2, 1); --i; if (!(b >> (state == 1 ? 3 : 5) & 1)) state = 0; }
        else { put(1, 1); --j; if (!(b >> (state == 2 ? 4 : 6) & 1)) state = 0; }
    }
    if (j < 0) put(2, i + 1); else if (i < 0) put(1, j + 1);
    if (len > 0) emit(op, len);
}

struct MmAlnCountRuns {                            // a job's runs in walk order -> count, first and last
    int32_t n = 0, w0_op = -1, w0_len = 0, wl_op = -1, wl_len = 0;
    GBX_MM_HD void operator()(int32_t op, int32_t len) { if (!n) { w0_op = op; w0_len = len; } wl_op = op; wl_len = len; ++n; }
};

// the walk's summary into the job; lane 0 calls it after mm_aln_dp
GBX_MM_HD inline void mm_aln_job_runs(MmAlnJob *J, const uint8_t *room, bool ext)
{
    MmAlnCountRuns c;
    if (J->end_t >= 0) mm_aln_walk(*J, room, c);
    J->ct = ext ? J->end_t + 1 : J->tl;
    J->cq = ext ? J->end_q + 1 : J->ql;
    J->n_ops = c.n;
    const bool fwd = J->kind == MMA_KIND_LEFT;                         // walk order is forward order for a left extension
    J->first_op = fwd ? c.w0_op : c.wl_op; J->first_len = fwd ? c.w0_len : c.wl_len; J->last_op = fwd ? c.wl_op : c.w0_op;
}

// a job that needs no DP: an empty extension window, or a fill with an empty side
GBX_MM_HD inline void mm_aln_job_plain(const gbx_mm_align_params &P, MmAlnJob *J)
{
    const int32_t tl = J->tl, ql = J->ql;
    J->score = 0; J->flags = 0; J->end_t = J->end_q = -1; J->ct = J->cq = 0; J->n_ops = 0; J->first_op = J->last_op = -1; J->first_len = 0;
    if (J->kind != MMA_KIND_FILL || (tl == 0 && ql == 0)) return;
    const int32_t l = tl > 0 ? tl : ql;
    J->score = -mma_gap(P, l); J->ct = tl; J->cq = ql; J->n_ops = 1; J->first_op = J->last_op = tl > 0 ? 2 : 1; J->first_len = l;
}
GBX_MM_HD inline bool mm_aln_job_is_dp(const MmAlnJob &J) { return J.tl > 0 && J.ql > 0; }

// one job run to its summary (every lane calls it; room: the job's own; fast: MMA_ROWS rows of fast_m ints of the team's own, or
// null - the rows go there when the job's M fits, else into the room)
template <class T>
GBX_MM_HD inline void mm_aln_job_run(const T &tm, const gbx_mm_align_params &P, const MmAlnSeq &S, uint8_t *room, int32_t *fast, int32_t fast_m, MmAlnJob *J)
{
    if (!mm_aln_job_is_dp(*J)) { if (tm.lane() == 0) mm_aln_job_plain(P, J); tm.sync(); return; }
    const bool ext = J->kind != MMA_KIND_FILL;
    const MmAlnView V{S, J->t0, J->q0, J->tl, J->ql, J->kind == MMA_KIND_LEFT};
    int32_t *rows = fast && mma_ring(J->w, J->tl) <= fast_m ? fast : (int32_t *)room;
    mm_aln_dp(tm, P, V, J->kind == MMA_KIND_LEFT ? MMA_RIGHT : MMA_LEFT, ext, room, rows, J);
    if (tm.lane() == 0) mm_aln_job_runs(J, room, ext);
    tm.sync();
}

// the batch a call aligns over: the arguments of gbx_mm_align_device that planning reads (anchor_cap < 0: unbounded, the host twin)
struct MmAlnIn {
    int64_t n_reads; const int64_t *off; const uint64_t *cax, *cay; const int32_t *n_chained; int64_t anchor_cap;
    const uint8_t *seq; const int64_t *seq_off; int64_t n_targets; const uint8_t *tseq; const int64_t *tseq_off;
};

// the texts and anchors of region g, or false where an index or an offset is not what it must be
GBX_MM_HD inline bool mm_aln_region_view(const MmAlnIn &in, const gbx_mm_reg &g, MmAlnSeq *S, const uint64_t **x, const uint64_t **y, int32_t *n_chained)
{
    if (g.read < 0 || g.read >= in.n_reads || g.rid < 0 || g.rid >= in.n_targets) return false;
    const int64_t s0 = in.seq_off[g.read], s1 = in.seq_off[g.read + 1], t0 = in.tseq_off[g.rid], t1 = in.tseq_off[g.rid + 1];
    const int64_t a0 = in.off[g.read], a1 = in.off[g.read + 1];
    if (s0 < 0 || s1 < s0 || s1 - s0 >= (1ll << 28) || t0 < 0 || t1 < t0 || t1 - t0 >= (1ll << 28)) return false;
    if (a0 < 0 || a1 < a0 || (in.anchor_cap >= 0 && a1 > in.anchor_cap)) return false;
    const int32_t nc = in.n_chained[g.read];
    if (nc < 0 || nc > a1 - a0) return false;
    *S = MmAlnSeq{in.tseq + t0, in.seq + s0, (int32_t)(t1 - t0), (int32_t)(s1 - s0), g.rev ? 1 : 0};
    *n_chained = nc;
    const int64_t as = g.as >= 0 && g.as <= nc ? g.as : 0;             // mm_aln_valid refuses what lies outside
    *x = in.cax + a0 + as; *y = in.cay + a0 + as;
    return true;
}

// ---- planning (rules 1-5): a region's anchors -> its jobs in order (left, the fills, right) through job(kind, t0, q0, tl, ql, w).
// -> false: the region is invalid.  x, y: the region's cnt anchors.
GBX_MM_HD inline bool mm_aln_valid(const gbx_mm_reg &g, int64_t n_targets, int32_t n_chained, const uint64_t *x, const uint64_t *y, int32_t tlen, int32_t qlen)
{
    if (g.rid < 0 || g.rid >= n_targets || g.cnt < 1 || g.as < 0 || (int64_t)g.as + g.cnt > n_chained) return false;
    const int32_t sp = (int32_t)(y[0] >> 32 & 0xff);
    if ((int32_t)(uint32_t)x[0] + 1 - sp < 0 || (int32_t)(uint32_t)y[0] + 1 - sp < 0) return false;
    for (int32_t i = 0; i < g.cnt; ++i) {
        const int32_t xi = (int32_t)(uint32_t)x[i], yi = (int32_t)(uint32_t)y[i];
        if (xi < 0 || yi < 0 || xi >= tlen || yi >= qlen) return false;
    }
    return true;
}

template <class Job>
GBX_MM_HD inline void mm_aln_plan(const gbx_mm_align_params &P, int32_t cnt, const uint64_t *x, const uint64_t *y, int32_t tlen, int32_t qlen, Job &job)
{
    const int32_t sp0 = (int32_t)(y[0] >> 32 & 0xff);
    int32_t rs = (int32_t)(uint32_t)x[0] + 1 - sp0, qs = (int32_t)(uint32_t)y[0] + 1 - sp0, re = rs, qe = qs;
    {
        const int64_t lq = qs < P.max_ext ? qs : P.max_ext, lt = rs < lq + P.bw ? rs : lq + P.bw;
        const bool on = lq > 0 && lt > 0;
        job(MMA_KIND_LEFT, rs - (on ? (int32_t)lt : 0), qs - (on ? (int32_t)lq : 0), on ? (int32_t)lt : 0, on ? (int32_t)lq : 0, (int64_t)P.bw);
    }
    for (int32_t i = 1; i < cnt; ++i) {
        const int32_t sp = (int32_t)(y[i] >> 32 & 0xff), xe = (int32_t)(uint32_t)x[i] - (sp >> 1), ye = (int32_t)(uint32_t)y[i] - (sp >> 1);
        re = xe > rs ? xe : rs; qe = ye > qs ? ye : qs;
        if (i == cnt - 1 || (re - rs >= P.min_ksw_len && qe - qs >= P.min_ksw_len)) {
            const int32_t tl = re - rs, ql = qe - qs, df = tl > ql ? tl - ql : ql - tl;
            job(MMA_KIND_FILL, rs, qs, tl, ql, (int64_t)(P.bw > df + 1 ? P.bw : df + 1));
            rs = re; qs = qe;
        }
    }
    {
        const int64_t lq = qlen - qe < P.max_ext ? qlen - qe : P.max_ext, lt = tlen - re < lq + P.bw ? tlen - re : lq + P.bw;
        const bool on = lq > 0 && lt > 0;
        job(MMA_KIND_RIGHT, re, qe, on ? (int32_t)lt : 0, on ? (int32_t)lq : 0, (int64_t)P.bw);
    }
}

struct MmAlnPlanCount {                            // the jobs of a region and the bytes of z they take
    int64_t n = 0, bytes = 0;
    GBX_MM_HD void operator()(int kind, int32_t t0, int32_t q0, int32_t tl, int32_t ql, int64_t w)
    {
        (void)kind; (void)t0; (void)q0;
        ++n;
        if (tl > 0 && ql > 0) bytes += mma_job_bytes(mma_band(w, tl, ql), tl, ql);
    }
};
struct MmAlnPlanWrite {                            // the jobs into jobs[at ..) below cap, their rooms from z_at on
    MmAlnJob *jobs; int64_t at, cap, z_at; int32_t reg, skip;
    GBX_MM_HD void operator()(int kind, int32_t t0, int32_t q0, int32_t tl, int32_t ql, int64_t w)
    {
        MmAlnJob j{};
        j.reg = reg; j.kind = kind; j.t0 = t0; j.q0 = q0; j.tl = tl; j.ql = ql; j.skip = skip; j.z_at = z_at;
        j.w = tl > 0 && ql > 0 ? mma_band(w, tl, ql) : 1;
        if (tl > 0 && ql > 0) z_at += mma_job_bytes(j.w, tl, ql);
        if (at < cap) jobs[at] = j;
        ++at;
    }
};

// the record of a region that is not aligned
GBX_MM_HD inline void mm_aln_copy(const gbx_mm_reg &g, int32_t flags, gbx_mm_aln *a)
{
    a->rs = g.rs; a->re = g.re; a->qs = g.qs; a->qe = g.qe; a->mlen = g.mlen; a->blen = g.blen;
    a->n_ambi = a->nm = a->dp_score = a->dp_max = a->n_cigar = 0; a->flags = flags; a->cigar_off = 0;
}

// ---- packing, first half: the region's jobs in order -> where each job's words go and the region's word count
GBX_MM_HD inline int32_t mm_aln_place(MmAlnJob *jobs, int32_t nj)
{
    int32_t total = 0, last = -1;
    for (int32_t k = 0; k < nj; ++k) {
        MmAlnJob &j = jobs[k];
        j.merge = j.n_ops > 0 && j.first_op == last;
        j.w_at = total - j.merge;
        if (j.n_ops > 0) { total += j.n_ops - j.merge; last = j.last_op; }
    }
    return total;
}

struct MmAlnPutRuns {                              // a job's runs to their words; the merged first run is left to mm_aln_pack
    uint32_t *cig; int64_t base, cap; int32_t n_ops, fwd, merge, k;
    GBX_MM_HD void operator()(int32_t op, int32_t len)
    {
        const int32_t f = fwd ? k : n_ops - 1 - k;
        ++k;
        if (f == 0 && merge) return;
        if (base + f < cap) cig[base + f] = (uint32_t)len << 4 | (uint32_t)op;
    }
};

// ---- packing, second half (rules 6-8): the words of the region at cig[at ..) (below cap only), statistics, record.
// jobs: the region's nj jobs after mm_aln_place; z: the whole room.
template <class T>
GBX_MM_HD inline void mm_aln_pack(const T &tm, const gbx_mm_align_params &P, const gbx_mm_reg &g, const MmAlnSeq &S, const MmAlnJob *jobs, int32_t nj,
                                  int32_t n_words, const uint8_t *z, uint32_t *cig, int64_t at, int64_t cap, gbx_mm_aln *out)
{
    for (int32_t k = tm.lane(); k < nj; k += tm.size()) {
        const MmAlnJob &j = jobs[k];
        if (j.n_ops <= 0) continue;
        MmAlnPutRuns put{cig, at + j.w_at, cap, j.n_ops, j.kind == MMA_KIND_LEFT, j.merge, 0};
        if (mm_aln_job_is_dp(j)) mm_aln_walk(j, z + j.z_at, put);
        else put(j.first_op, j.first_len);
    }
    tm.sync();
    if (tm.lane() == 0) {
        for (int32_t k = 0; k < nj; ++k)
            if (jobs[k].n_ops > 0 && jobs[k].merge && at + jobs[k].w_at < cap) cig[at + jobs[k].w_at] += (uint32_t)jobs[k].first_len << 4;
        gbx_mm_aln a;
        int32_t score = 0, fl = 1;
        for (int32_t k = 0; k < nj; ++k) score += jobs[k].score;
        const MmAlnJob &L = jobs[0], &R = jobs[nj - 1];
        if (L.flags & 1) fl |= 2;
        if (R.flags & 1) fl |= 4;
        if (L.flags & 2) fl |= 8;
        if (R.flags & 2) fl |= 16;
        const int32_t rs = L.t0 + L.tl - L.ct, qs = L.q0 + L.ql - L.cq, re = R.t0 + R.ct, qe = R.q0 + R.cq;
        a.rs = rs; a.re = re;
        a.qs = S.rev ? S.qlen - qe : qs; a.qe = S.rev ? S.qlen - qs : qe;
        a.dp_score = score; a.n_cigar = n_words; a.flags = fl; a.cigar_off = at;
        int32_t mlen = 0, blen = 0, amb = 0, s = 0, mx = 0, t = rs, q = qs;
        if (at + n_words <= cap) {
            for (int32_t k = 0; k < n_words; ++k) {
                const uint32_t wd = cig[at + k];
                const int32_t op = (int32_t)(wd & 15), len = (int32_t)(wd >> 4);
                if (op == 0) {
                    for (int32_t i = 0; i < len; ++i) {
                        const int tc = S.tc(t + i), qc = S.qc(q + i);
                        if (tc > 3 || qc > 3) ++amb; else if (tc == qc) { ++mlen; ++blen; } else ++blen;
                        s += mma_sc(P, tc, qc);
                        if (s < 0) s = 0; else if (s > mx) mx = s;
                    }
                    t += len; q += len;
                } else {
                    int32_t kk = 0;
                    for (int32_t i = 0; i < len; ++i) kk += (op == 2 ? S.tc(t + i) : S.qc(q + i)) > 3;
                    blen += len - kk; amb += kk;
                    s -= mma_gap(P, len);
                    if (s < 0) s = 0;
                    if (op == 2) t += len; else q += len;
                }
            }
        }
        a.mlen = mlen; a.blen = blen; a.n_ambi = amb; a.nm = blen - mlen + amb; a.dp_max = mx;
        *out = a;
    }
    tm.sync();
}

// ---- PAF with CIGAR (rule 9): the line of an aligned region; one that is not aligned prints mm_paf_line
GBX_MM_HD inline int64_t mm_paf_cigar_line(uint8_t *out, int64_t at, int64_t cap, const gbx_mm_reg &g, const gbx_mm_aln &a, const uint32_t *cig,
                                           const uint8_t *qname, int64_t qname_len, int32_t qlen, const uint8_t *tname, int64_t tname_len, int32_t tlen,
                                           int32_t rep_len)
{
    MmPafOut o{out, at, cap, 0};
    o.bytes(qname, qname_len); o.ch('\t'); o.num(qlen); o.ch('\t'); o.num(a.qs); o.ch('\t'); o.num(a.qe); o.ch('\t');
    o.ch(g.rev ? '-' : '+'); o.ch('\t');
    if (tname) o.bytes(tname, tname_len); else o.ch('*');
    o.ch('\t'); o.num(tlen); o.ch('\t'); o.num(a.rs); o.ch('\t'); o.num(a.re); o.ch('\t');
    o.num(a.mlen); o.ch('\t'); o.num(a.blen); o.ch('\t'); o.num(g.mapq);
    o.str("\tNM:i:"); o.num(a.nm); o.str("\tms:i:"); o.num(a.dp_max); o.str("\tAS:i:"); o.num(a.dp_score); o.str("\tnn:i:"); o.num(a.n_ambi);
    o.str(g.parent == g.id ? "\ttp:A:P" : "\ttp:A:S");
    o.str("\tcm:i:"); o.num(g.cnt);
    o.str("\ts1:i:"); o.num(g.score);
    if (g.parent == g.id) { o.str("\ts2:i:"); o.num(g.subsc); }
    o.str("\trl:i:"); o.num(rep_len);
    o.str("\tcg:Z:");
    for (int32_t k = 0; k < a.n_cigar; ++k) { const uint32_t wd = cig[a.cigar_off + k]; o.num(wd >> 4); o.ch((uint8_t)"MID"[wd & 15 & 3]); }
    o.ch('\n');
    return o.n;
}

}  // namespace gbx
