// mem_rescue_kernels.hip — mate rescue between the alignment regions and the paired-end stage (bwa-mem's mem_matesw around
// ksw_align2: a full local Smith-Waterman of the mate against the window the insert-size estimate predicts) for gfx950 (MI355X).
//
// Semantics: include/gbx.h and DESIGN 3.14 (restated in tests/mem_rescue_ref.py, which pins them).
//
// Shape: the SW answer of an (anchor, direction) depends only on the anchor, the estimate and the mate; only the use of the
// answers is serial (a rescued region can make the next anchor skip, a dedup can remove the region that made one skip).  So:
//   * plan: one pair per wavefront sorts each end into dedup order (wave_sort), takes the anchors b_e and their first skip sets.  A pair in which
//     every anchor has all four directions set is done: it is copied through (the common case).  An active pair gets a task slot
//     for every (end, anchor, direction), 4 (|b_0| + |b_1|) of them at an offset from mem_scan_launch; a slot is valid when the
//     direction has not failed and has a window.  The first skip set does not filter the slots.
//   * SW: one task per wavefront, no per-task capacity.  A lane owns R consecutive query rows (R = 1, 2, 4, 8, 16: the smallest
//     with 64 R >= slen * Pw) as H and E in registers; columns are skewed one per lane, a systolic pass of n + 63 steps.  The
//     boundary H and F, the running column maximum and the target base go to the next lane by a lane shift (two packed words), so
//     the last lane sees every column's maximum in column order: it keeps gmax / te, writes the maxima into a ring in LDS and runs
//     bwa's entry rule 1100 columns behind the front, which is further than a window of +- ceil(score / a) <= 1024 reaches: an
//     entry is closed for good when it is judged, and a later te makes every closed entry eligible (best of all) - no list of
//     entries, no saved column, any window length.  Every lane keeps its first strict maximum as (value, column, striped key); a
//     wave reduction gives score, te, qe.  The same code runs the reverse pass (no entries, it stops when the last lane has seen
//     the score).  Cells are 32-bit in registers; only what crosses lanes is packed to 16 bits.
//   * replay: one active pair per wavefront applies the rules in bwa's order with the answers looked up; the lists are index lists
//     over regions that stay where they were made, in a slab of the pair's regions plus its task slots; dedup, primary marking,
//     mapq and the report are the wave-wide steps of mem_common.h that mem_regs_read_kernel runs.
//   * pack: a wavefront per pair writes the regs-shape outputs, the new seed records and the CIGAR list at offsets from scans
//     over the reads: no dependence on the scheduling.
#include <cstring>
#include "mem_common.h"

namespace gbx {
namespace {

static_assert(sizeof(gbx_mem_reg) == 88 && sizeof(gbx_mem_rescue_params) == 64 && sizeof(gbx_mem_rescue_stat) == 16 &&
              sizeof(gbx_mem_pestat) == 32 && sizeof(gbx_bsw_seed) == 40, "records");

constexpr int RS_MAX_READ = 1024;                    // the longest mate: 16 rows in each of 64 lanes
constexpr int RS_RING = 2048, RS_LAG = 1100;         // column maxima kept in LDS; how far behind the front the entry rule runs
constexpr int RS_PAD = 5, RS_OUT = 6;                // query symbols: a padded row (0 against everything), a row past the padding
constexpr int RS_MAX_WIN = 1 << 20;

struct RsTask { long long rb; int n, read, is_rev, valid; };          // window [rb, rb + n) for the mate `read`
struct RsAns { int score, te, qe, score2, te2, qb, tb, pad_; };

struct RsArgs {
    gbx_mem_rescue_params p;
    MemRescueIo io;
    long long n_pairs, pair_id0, task_cap;
    long long *tcnt;                 // [n_pairs + 1]      task slots per pair, then their exclusive scan
    long long *cnt;                  // [2][2 n_pairs + 1] regions / reported regions per read, then their scans
    long long *kcnt;                 // [2 n_pairs + 1]    surviving rescued regions per read, then their scan
    int64_t *n_tasks, *n_kept;       // the totals of tcnt and kcnt
    int *nb;                         // [2 n_pairs]        |b_e|
    int *mode;                       // [n_pairs]          0: copied through; 1: its lists are in the slab
    RsTask *tasks; RsAns *ans;       // [task_cap]
    gbx_mem_reg *st;                 // [reg_cap + task_cap] slab of a pair: its first region + its first task slot
    int *cur, *ord, *ordb, *z, *excl;   // the same slabs: the list, two index lists, the primaries, the dedup's exclusions
    RegKey *key;                     // [2 (reg_cap + task_cap)] slab at twice the pair's: the sort pads to a power of two
    int *eord;                       // [reg_cap]          an end's regions in dedup order (indices within the end)
};

struct RsSpan { long long g0, g1, g2; bool ok; };
__device__ inline RsSpan rs_span(const RsArgs &A, long long p)
{
    RsSpan s;
    const long long n = *A.io.n_regs;
    s.ok = n >= 0 && n <= A.io.reg_cap;
    const long long m = s.ok ? n : 0;
    s.g0 = clampll(A.io.reg_off[2 * p], 0, m);
    s.g1 = clampll(A.io.reg_off[2 * p + 1], s.g0, m);
    s.g2 = clampll(A.io.reg_off[2 * p + 2], s.g1, m);
    return s;
}

__device__ inline bool rs_pes_ok(const gbx_mem_pestat &pe) { return !pe.failed && pe.low >= 0 && pe.low <= pe.high && pe.high <= RS_MAX_WIN; }

// rule 2's window of direction r -> a task
__device__ inline RsTask rs_window(const RsArgs &A, const gbx_mem_pestat &pe, long long arb, int arid, int r, int read)
{
    RsTask T;
    T.rb = 0; T.n = 0; T.read = read; T.is_rev = (r >> 1) != (r & 1); T.valid = 0;
    const long long L = A.io.l_pac;
    const int l_ms = A.io.read_len[read];
    const long long qoff = A.io.read_off[read];
    if (!rs_pes_ok(pe) || l_ms < 1 || l_ms > RS_MAX_READ || qoff < 0 || qoff + l_ms > A.io.qer_bytes) return T;
    const bool larger = !(r >> 1);
    long long rb, re;
    if (!T.is_rev) {
        rb = larger ? arb + pe.low : arb - pe.high;
        re = (larger ? arb + pe.high : arb - pe.low) + l_ms;
    } else {
        rb = (larger ? arb + pe.low : arb - pe.high) - l_ms;
        re = larger ? arb + pe.high : arb - pe.low;
    }
    rb = rb > 0 ? rb : 0;
    re = re < 2 * L ? re : 2 * L;
    if (rb >= re) return T;
    const long long mid = (rb + re) >> 1;
    const bool rev = mid >= L;
    const long long fwd = rev ? 2 * L - 1 - mid : mid;
    int lo = 0, hi = A.io.n_contigs;                                             // the contig with off[c] <= fwd < off[c + 1]
    while (hi - lo > 1) {
        const int c = (lo + hi) >> 1;
        if (A.io.contig_off[c] <= fwd) lo = c; else hi = c;
    }
    const long long c0 = clampll(A.io.contig_off[lo], 0, L), c1 = clampll(A.io.contig_off[lo + 1], c0, L);
    const long long wlo = rev ? 2 * L - c1 : c0, whi = rev ? 2 * L - c0 : c1;
    rb = rb > wlo ? rb : wlo;
    re = re < whi ? re : whi;
    if (lo != arid || re - rb < A.p.min_seed_len || re - rb > RS_MAX_WIN + RS_MAX_READ) return T;
    T.rb = rb; T.n = (int)(re - rb); T.valid = 1;
    return T;
}

// rs_skip across the wavefront: lanes over the mate's list (list null: st itself in order) -> the same set in every lane
__device__ inline int rs_skip(const RsArgs &A, const gbx_mem_pestat *pes, long long rb, const gbx_mem_reg *st, const int *list, int n, int lane)
{
    int skip = 0;
    for (int r = 0; r < 4; ++r) skip |= (pes[r].failed ? 1 : 0) << r;
    for (int i = lane; i < n; i += 64) {
        long long dist;
        const int r = mem_infer_dir(A.io.l_pac, rb, st[list ? list[i] : i].rb, &dist);
        if (dist >= pes[r].low && dist <= pes[r].high) skip |= 1 << r;
    }
    for (int s = 32; s > 0; s >>= 1) skip |= __shfl_xor(skip, s);
    return skip;
}

// ---- plan, first half: one pair per wavefront: each end in dedup order, the anchors, whether the pair is active
__global__ void __launch_bounds__(64) mem_rescue_plan_kernel(RsArgs A)
{
    __shared__ gbx_mem_pestat pes[4];
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const RsSpan S = rs_span(A, p);
    if (lane < 4) pes[lane] = A.io.pes[lane];
    __syncthreads();
    int nb[2] = {0, 0};
    const long long g[3] = {S.g0, S.g1, S.g2};
    for (int e = 0; e < 2; ++e) {
        const gbx_mem_reg *const a = A.io.regs + g[e];
        const int n = (int)(g[e + 1] - g[e]);
        RegKey *const key = A.key + 2 * g[e];
        int *const ord = A.eord + g[e];
        for (int i = lane; i < n; i += 64) {                                     // (score desc, rb, qb), then the index
            RegKey v;
            v.w[0] = (unsigned long long)(0x7fffffffll - a[i].score);
            v.w[1] = (unsigned long long)a[i].rb ^ REG_SIGN;
            v.w[2] = (unsigned long long)((unsigned)a[i].qb ^ 0x80000000u) << 32 | (unsigned)i;
            key[i] = v;
        }
        __syncthreads();
        wave_sort(key, n, lane);
        for (int i = lane; i < n; i += 64) ord[i] = (int)(unsigned)key[i].w[2];
        __syncthreads();
        const int top = n > 0 ? a[ord[0]].score : 0;
        for (int b0 = 0; b0 < n && b0 < A.p.max_matesw; b0 += 64) {              // the scores fall along ord: a prefix
            const int i = b0 + lane;
            nb[e] += __builtin_popcountll(__ballot(i < n && i < A.p.max_matesw && a[ord[i]].score >= top - A.p.pen_unpaired));
        }
    }
    bool active = false;
    for (int e = 0; e < 2 && !active; ++e) {
        const gbx_mem_reg *const a = A.io.regs + g[e], *const m = A.io.regs + g[1 - e];
        for (int j = 0; j < nb[e] && !active; ++j)
            active = rs_skip(A, pes, a[A.eord[g[e] + j]].rb, m, nullptr, (int)(g[2 - e] - g[1 - e]), lane) != 15;
    }
    if (lane == 0) {
        A.nb[2 * p] = nb[0]; A.nb[2 * p + 1] = nb[1];
        A.tcnt[p] = S.ok && active ? 4ll * (nb[0] + nb[1]) : 0;
    }
}

// ---- plan, second half: the task slots of an active pair, lanes over the slots
__global__ void __launch_bounds__(64) mem_rescue_task_kernel(RsArgs A)
{
    const long long p = blockIdx.x;
    const long long t0 = A.tcnt[p], nt = A.tcnt[p + 1] - t0;
    if (nt <= 0 || t0 + nt > A.task_cap) return;
    const RsSpan S = rs_span(A, p);
    const int nb0 = A.nb[2 * p];
    for (int t = threadIdx.x; t < nt; t += 64) {
        const int e = t >= 4 * nb0, j = (e ? t - 4 * nb0 : t) >> 2, r = t & 3;
        const long long ge = e ? S.g1 : S.g0;
        const gbx_mem_reg &an = A.io.regs[ge + A.eord[ge + j]];
        A.tasks[t0 + t] = rs_window(A, A.io.pes[r], an.rb, an.rid, r, (int)(2 * p + 1 - e));
    }
}

// ---- the SW
struct RsCost { int a, b, e_del, oe_del, e_ins, oe_ins, minsc; };
struct RsPass { int score, te, qe, score2, te2; };

// One pass of ksw_align2's kernel over q[0, m) x t[0, n): q(j) = qp[j * qstep] (complemented if comp), t(i) = tp[i * tstep].
// endsc < 0: the forward pass with the entry rule; else the pass stops once the last lane has seen a column maximum >= endsc.
template <int R>
__device__ inline RsPass rs_pass(const uint8_t *qp, int qstep, bool comp, const uint8_t *tp, int tstep, int m, int n, int Pw, const RsCost &c,
                                 int endsc, unsigned short *ring, int lane)
{
    const int slen = (m + Pw - 1) / Pw, mp = slen * Pw;
    int qk[R], H[R], E[R];                                                       // qk: symbol | (1023 - striped key) << 3
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int j = lane * R + k;
        int s = RS_OUT;
        if (j < m) {
            s = qp[(long long)j * qstep];
            s = s > 3 ? 4 : comp ? 3 - s : s;
        } else if (j < mp)
            s = RS_PAD;
        const int key = j < mp ? (j % slen) * Pw + j / slen : 1023;
        qk[k] = s | (1023 - key) << 3;
        H[k] = 0; E[k] = 0;
    }
    const bool entries = endsc < 0;
    int hd = 0;                                                                  // H of the row above this lane's, one column back
    unsigned out_hf = 0, out_ct = 0;                                             // what the next lane takes: H | F << 16, colmax | base << 16
    int bv = 0, bc = 0x3fffff, bk = 0;                                           // this lane's first strict maximum
    int chunk = 4;
    // the last lane's state: gmax / te, the open entry, the best closed entry of all and of those outside te +- w
    int gmax = 0, te = -1, w = 0, last_v = 0, last_c = -2, all_v = -1, all_c = -1, cur_v = -1, cur_c = -1, done = 0;
    auto close_entry = [&]() {
        if (last_c < 0) return;
        if (last_v > all_v) { all_v = last_v; all_c = last_c; }
        if ((last_c < te - w || last_c > te + w) && last_v > cur_v) { cur_v = last_v; cur_c = last_c; }
    };
    auto consume = [&](int col) {
        const int v = ring[col & (RS_RING - 1)];
        if (v < c.minsc) return;
        if (last_c + 1 != col) { close_entry(); last_v = v; last_c = col; }
        else if (last_v < v) { last_v = v; last_c = col; }
    };
    const int steps = n + 63;
    for (int t = 0; t < steps; ++t) {
        if ((t & 63) == 0) {
            const int col = t + lane;
            chunk = col < n ? tp[(long long)col * tstep] : 4;
            chunk = chunk > 3 ? 4 : chunk;
        }
        const int ts0 = __builtin_amdgcn_readlane(chunk, t & 63);                // (t is uniform: no LDS round trip)
        const unsigned in_hf = __shfl_up(out_hf, 1), in_ct = __shfl_up(out_ct, 1);
        const int hu = lane ? (int)(in_hf & 0xffff) : 0, fu = lane ? (int)(in_hf >> 16) : 0;
        const int cm_in = lane ? (int)(in_ct & 0xffff) : 0, ts = lane ? (int)(in_ct >> 16) : ts0;
        const int i = t - lane;
        if (i >= 0 && i < n) {
            int diag = hd, f = fu, best = 0;
            hd = hu;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int q = qk[k] & 7;
                const int s = q == RS_PAD ? 0 : (q > 3 || ts > 3) ? -1 : q == ts ? c.a : -c.b;
                int h = diag + s;
                h = h > E[k] ? h : E[k];
                h = h > f ? h : f;
                h = h > 0 ? h : 0;
                if (q == RS_OUT) h = 0;
                diag = H[k];
                H[k] = h;
                int e = E[k] - c.e_del;
                e = e > h - c.oe_del ? e : h - c.oe_del;
                E[k] = e > 0 ? e : 0;
                f -= c.e_ins;
                f = f > h - c.oe_ins ? f : h - c.oe_ins;
                f = f > 0 ? f : 0;
                const int cand = h << 10 | qk[k] >> 3;
                best = best > cand ? best : cand;
            }
            const int hb = best >> 10;
            if (hb > bv) { bv = hb; bc = i; bk = best & 1023; }
            const int cm = cm_in > hb ? cm_in : hb;
            out_hf = (unsigned)H[R - 1] | (unsigned)f << 16;
            out_ct = (unsigned)cm | (unsigned)ts << 16;
            if (lane == 63) {
                if (cm > gmax) {
                    gmax = cm; te = i; w = (gmax + c.a - 1) / c.a;
                    cur_v = all_v; cur_c = all_c;                                // every closed entry lies before te - w
                    if (!entries && gmax >= endsc) done = 1;
                }
                if (entries) {
                    ring[i & (RS_RING - 1)] = (unsigned short)cm;
                    if (i >= RS_LAG) consume(i - RS_LAG);
                }
            }
        }
        if (!entries && __shfl(done, 63)) break;
    }
    if (entries && lane == 63) {
        for (int col = n > RS_LAG ? n - RS_LAG : 0; col < n; ++col) consume(col);
        close_entry();
    }
    unsigned long long v = (unsigned long long)bv << 32 | (unsigned long long)(0x3fffff - bc) << 10 | (unsigned)bk;
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o > v ? o : v;
    }
    RsPass P;
    P.score = (int)(v >> 32);
    P.te = -1; P.qe = -1;
    if (P.score > 0) {
        P.te = 0x3fffff - (int)(v >> 10 & 0x3fffff);
        const int key = 1023 - (int)(v & 1023);
        P.qe = (key % Pw) * slen + key / Pw;
        P.qe = P.qe < m ? P.qe : m - 1;                                           // (a padded row never holds the maximum)
    }
    P.score2 = __shfl(cur_v, 63);
    P.te2 = __shfl(cur_c, 63);
    return P;
}

__device__ inline RsPass rs_pass_any(const uint8_t *qp, int qstep, bool comp, const uint8_t *tp, int tstep, int m, int n, int Pw, const RsCost &c,
                                     int endsc, unsigned short *ring, int lane)
{
    const int mp = (m + Pw - 1) / Pw * Pw;
    if (mp <= 64) return rs_pass<1>(qp, qstep, comp, tp, tstep, m, n, Pw, c, endsc, ring, lane);
    if (mp <= 128) return rs_pass<2>(qp, qstep, comp, tp, tstep, m, n, Pw, c, endsc, ring, lane);
    if (mp <= 256) return rs_pass<4>(qp, qstep, comp, tp, tstep, m, n, Pw, c, endsc, ring, lane);
    if (mp <= 512) return rs_pass<8>(qp, qstep, comp, tp, tstep, m, n, Pw, c, endsc, ring, lane);
    return rs_pass<16>(qp, qstep, comp, tp, tstep, m, n, Pw, c, endsc, ring, lane);
}

__global__ void __launch_bounds__(64) mem_rescue_sw_kernel(RsArgs A)
{
    __shared__ unsigned short ring[RS_RING];
    const int lane = threadIdx.x;
    long long nt = *A.n_tasks;
    nt = nt < A.task_cap ? nt : A.task_cap;
    RsCost c;
    c.a = A.p.a; c.b = A.p.b; c.e_del = A.p.e_del; c.oe_del = A.p.o_del + A.p.e_del; c.e_ins = A.p.e_ins; c.oe_ins = A.p.o_ins + A.p.e_ins;
    c.minsc = A.p.min_seed_len * A.p.a;
    for (long long slot = blockIdx.x; slot < nt; slot += gridDim.x) {
        const RsTask T = A.tasks[slot];
        if (!T.valid) continue;
        const int m = A.io.read_len[T.read];
        const uint8_t *const mate = A.io.qer + A.io.read_off[T.read], *const win = A.io.text + T.rb;
        const int Pw = m * c.a < 250 ? 16 : 8;
        // the query is the mate, or its reverse complement read from its far end
        const RsPass F = T.is_rev ? rs_pass_any(mate + (m - 1), -1, true, win, 1, m, T.n, Pw, c, -1, ring, lane)
                                  : rs_pass_any(mate, 1, false, win, 1, m, T.n, Pw, c, -1, ring, lane);
        RsAns o;
        o.score = F.score; o.te = F.te; o.qe = F.qe; o.score2 = F.score2; o.te2 = F.te2; o.qb = -1; o.tb = -1; o.pad_ = 0;
        if (F.score >= c.minsc) {
            const RsPass B = T.is_rev ? rs_pass_any(mate + (m - 1 - F.qe), 1, true, win + F.te, -1, F.qe + 1, F.te + 1, Pw, c, F.score, ring, lane)
                                      : rs_pass_any(mate + F.qe, -1, false, win + F.te, -1, F.qe + 1, F.te + 1, Pw, c, F.score, ring, lane);
            if (B.score == F.score) { o.qb = F.qe - B.qe; o.tb = F.te - B.te; }
        }
        if (lane == 0) A.ans[slot] = o;
    }
}

// ---- replay: one active pair per wavefront applies rules 1, 2 and 4 with the SW answers looked up; dedup, primary marking
// and the report run on the pair's slab by the wave-wide steps of mem_common.h, as in mem_regs_read_kernel
__global__ void __launch_bounds__(64) mem_rescue_replay_kernel(RsArgs A)
{
    __shared__ gbx_mem_pestat pes[4];
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const RsSpan S = rs_span(A, p);
    const long long g[3] = {S.g0, S.g1, S.g2};
    long long *const cnt_reg = A.cnt + 2 * p, *const cnt_rep = A.cnt + (2 * A.n_pairs + 1) + 2 * p, *const cnt_kept = A.kcnt + 2 * p;
    if (lane < 4) pes[lane] = A.io.pes[lane];
    __syncthreads();
    gbx_mem_rescue_stat stat;
    stat.n_sw = 0; stat.n_added = 0; stat.n_kept = 0; stat.pad_ = 0;
    const long long t0 = A.tcnt[p], nt = A.tcnt[p + 1] - t0;
    const int n_in[2] = {(int)(S.g1 - S.g0), (int)(S.g2 - S.g1)};
    const int nb[2] = {A.nb[2 * p], A.nb[2 * p + 1]};
    const int cap[2] = {n_in[0] + 4 * nb[1], n_in[1] + 4 * nb[0]};                // what an end's list can grow to
    const long long base[2] = {S.g0 + t0, S.g0 + t0 + cap[0]};
    int len[2] = {n_in[0], n_in[1]}, made[2] = {n_in[0], n_in[1]};
    if (S.ok && nt > 0 && t0 + nt <= A.task_cap) {
        for (int e = 0; e < 2; ++e)                                              // the lists in dedup order; the anchors are their heads
            for (int i = lane; i < n_in[e]; i += 64) {
                A.st[base[e] + i] = A.io.regs[g[e] + A.eord[g[e] + i]];
                A.cur[base[e] + i] = i;
            }
        __syncthreads();
        const long long L = A.io.l_pac;
        for (int e = 0; e < 2; ++e) {
            const int o = 1 - e;
            gbx_mem_reg *const st = A.st + base[o];
            int *const cur = A.cur + base[o], *const ord = A.ord + base[o], *const ordb = A.ordb + base[o], *const excl = A.excl + base[o];
            RegKey *const key = A.key + 2 * base[o];
            for (int j = 0; j < nb[e]; ++j) {
                const long long arb = A.st[base[e] + j].rb;
                const int arid = A.st[base[e] + j].rid;
                const int skip = rs_skip(A, pes, arb, st, cur, len[o], lane);
                if (skip == 15) continue;
                int n = 0;
                for (int r = 0; r < 4; ++r) {
                    if (skip >> r & 1) continue;
                    const long long slot = t0 + (e ? 4 * nb[0] : 0) + 4 * j + r;
                    const RsTask T = A.tasks[slot];
                    if (T.valid) {
                        const RsAns a = A.ans[slot];
                        ++n;
                        if (a.score >= A.p.min_seed_len && a.qb >= 0 && made[o] < cap[o]) {
                            const int l_ms = A.io.read_len[T.read];
                            gbx_mem_reg B;
                            memset(&B, 0, sizeof(B));
                            B.rid = arid; B.read = T.read;
                            B.qb = T.is_rev ? l_ms - (a.qe + 1) : a.qb;
                            B.qe = T.is_rev ? l_ms - a.qb : a.qe + 1;
                            B.rb = T.is_rev ? 2 * L - (T.rb + a.te + 1) : T.rb + a.tb;
                            B.re = T.is_rev ? 2 * L - (T.rb + a.tb) : T.rb + a.te + 1;
                            B.score = a.score; B.csub = a.score2; B.secondary = -1; B.sel = -1;
                            const long long lr = B.re - B.rb, lqy = B.qe - B.qb;
                            B.seedcov = (int)((lr < lqy ? lr : lqy) >> 1);
                            B.seed = -1 - slot;                                   // until the pack pass: its task
                            // in front of the first element with a lower score: the list is in dedup order, scores falling
                            int at = 0;
                            for (int b0 = 0; b0 < len[o]; b0 += 64) {
                                const int i = b0 + lane;
                                at += __builtin_popcountll(__ballot(i < len[o] && st[cur[i]].score >= B.score));
                            }
                            for (int i = at + lane; i < len[o]; i += 64) ordb[i] = cur[i];
                            __syncthreads();
                            for (int i = at + lane; i < len[o]; i += 64) cur[i + 1] = ordb[i];
                            if (lane == 0) { st[made[o]] = B; cur[at] = made[o]; }
                            ++made[o]; ++len[o]; ++stat.n_added;
                            __syncthreads();
                        }
                    }
                    if (n > 0) {
                        len[o] = wave_reg_dedup(st, cur, len[o], ord, ordb, excl, key, A.p, lane);
                        for (int i = lane; i < len[o]; i += 64) cur[i] = ordb[i];
                        __syncthreads();
                    }
                }
                stat.n_sw += n;
            }
        }
    }
    if (stat.n_sw > 0) {
        for (int e = 0; e < 2; ++e) {
            gbx_mem_reg *const st = A.st + base[e];
            int *const cur = A.cur + base[e], *const ord = A.ord + base[e];
            for (int i = lane; i < len[e]; i += 64) { gbx_mem_reg &X = st[cur[i]]; X.sub = 0; X.sub_n = 0; X.secondary = -1; }
            __syncthreads();
            wave_reg_mark_primary(st, cur, len[e], ord, A.z + base[e], A.key + 2 * base[e], 2 * (A.pair_id0 + p) + e, A.p, lane);
            const int l_rep = A.io.l_rep[2 * p + e];
            const int n_rep = wave_reg_report(st, ord, len[e], [&](const gbx_mem_reg &R) {
                const int lq = R.seed >= 0 && R.seed < A.io.seed_cap ? A.io.seeds[R.seed].lq : 0;
                return lq > 0 ? reg_frac_rep(R, l_rep, lq) : 0.f;
            }, A.p, lane);
            __syncthreads();
            int kept = 0;
            for (int b0 = 0; b0 < len[e]; b0 += 64) {
                const int i = b0 + lane;
                kept += __builtin_popcountll(__ballot(i < len[e] && st[ord[i]].seed < 0));
            }
            for (int i = lane; i < len[e]; i += 64) cur[i] = ord[i];             // the output order, for the pack pass
            if (lane == 0) { cnt_reg[e] = len[e]; cnt_rep[e] = n_rep; cnt_kept[e] = kept; }
            stat.n_kept += kept;
        }
    } else {
        for (int e = 0; e < 2; ++e) {
            int rep = 0;
            for (long long b0 = g[e]; b0 < g[e + 1]; b0 += 64) {
                const long long t = b0 + lane;
                rep += __builtin_popcountll(__ballot(t < g[e + 1] && (A.io.regs[t].flag & 1)));
            }
            if (lane == 0) { cnt_reg[e] = S.ok ? n_in[e] : 0; cnt_rep[e] = S.ok ? rep : 0; cnt_kept[e] = 0; }
        }
    }
    if (lane == 0) {
        A.mode[p] = stat.n_sw > 0;
        A.io.stats[p] = stat;
    }
}

// ---- the records at their final places: a wavefront per pair, lanes over a read's regions in output order
__global__ void __launch_bounds__(64) mem_rescue_pack_kernel(RsArgs A)
{
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const RsSpan S = rs_span(A, p);
    if (!S.ok) return;
    const unsigned long long below = (1ull << lane) - 1;
    const int mode = A.mode[p];
    const long long t0 = A.tcnt[p], L = A.io.l_pac;
    const int n_in0 = (int)(S.g1 - S.g0);
    const long long base[2] = {S.g0 + t0, S.g0 + t0 + n_in0 + 4 * A.nb[2 * p + 1]};
    for (int e = 0; e < 2; ++e) {
        const long long r = 2 * p + e;
        const long long o0 = A.cnt[r], n = A.cnt[r + 1] - o0, s0 = A.cnt[(2 * A.n_pairs + 1) + r], k0 = A.kcnt[r];
        const long long gin = e ? S.g1 : S.g0;
        int n_rep = 0, n_kept = 0;
        for (long long b0 = 0; b0 < n; b0 += 64) {
            const long long i = b0 + lane;
            const bool act = i < n;
            gbx_mem_reg R;
            bool rep = false, fresh = false;
            if (act) {
                R = mode ? A.st[base[e] + A.cur[base[e] + i]] : A.io.regs[gin + i];
                rep = (R.flag & 1) != 0;
                fresh = mode && R.seed < 0;
            }
            const unsigned long long br = __ballot(rep), bf = __ballot(fresh);
            if (act) {
                gbx_bsw_seed s;
                memset(&s, 0, sizeof(s));
                if (fresh) {
                    const RsTask T = A.tasks[-1 - R.seed];
                    s.qoff = A.io.read_off[T.read]; s.lq = A.io.read_len[T.read];
                    s.roff = T.is_rev ? 2 * L - (T.rb + T.n) : T.rb; s.rlen = T.n;
                    s.qbeg = R.qb; s.rbeg = (int32_t)(R.rb - s.roff); s.len = 0;
                    const long long k = A.io.seed_cap + k0 + n_kept + __builtin_popcountll(bf & below);
                    R.seed = k;
                    if (k < A.io.xseed_cap) A.io.xseeds[k] = s;
                } else if (R.seed >= 0 && R.seed < A.io.seed_cap)
                    s = A.io.seeds[R.seed];
                const long long gs = s0 + n_rep + __builtin_popcountll(br & below);
                R.sel = rep ? (int32_t)gs : -1;
                if (o0 + i < A.io.xreg_cap) A.io.xregs[o0 + i] = R;
                if (rep && gs < A.io.xsel_cap) {
                    A.io.xsel_seeds[gs] = s;
                    A.io.xsel_res[gs] = reg_result(R, s);
                }
            }
            n_rep += __builtin_popcountll(br);
            n_kept += __builtin_popcountll(bf);
        }
    }
}

// the count of seed records: the caller's seed_cap and the rescued regions that survived, -1 after an upstream overflow
__global__ void mem_rescue_count_kernel(RsArgs A)
{
    const long long k = *A.n_kept;
    *A.io.n_xseeds = k < 0 ? -1 : A.io.seed_cap + k;
}

struct RsLayout {
    size_t o_tcnt, o_cnt, o_kcnt, o_bsum, o_tot, o_nb, o_mode, o_tasks, o_ans, o_st, o_cur, o_ord, o_ordb, o_z, o_excl, o_key, o_eord, total;
    int blocks_p, blocks_r;
    long long task_cap;
};
RsLayout rs_layout(int64_t n_pairs, int64_t reg_cap, int32_t max_matesw)
{
    RsLayout L;
    const size_t np = (size_t)n_pairs, nr = 2 * np;
    const long long by_anchor = 2ll * n_pairs * (max_matesw < 1 ? 1 : max_matesw);
    L.task_cap = 4 * (reg_cap < by_anchor ? reg_cap : by_anchor);
    const size_t slab = (size_t)reg_cap + (size_t)L.task_cap;
    L.blocks_p = mem_scan_blocks(n_pairs); L.blocks_r = mem_scan_blocks(2 * n_pairs);
    L.o_tcnt = 0;
    L.o_cnt = L.o_tcnt + align256((np + 1) * 8);
    L.o_kcnt = L.o_cnt + align256(2 * (nr + 1) * 8);
    L.o_bsum = L.o_kcnt + align256((nr + 1) * 8);
    L.o_tot = L.o_bsum + align256(2 * (size_t)(L.blocks_r > L.blocks_p ? L.blocks_r : L.blocks_p) * 8);
    L.o_nb = L.o_tot + 256;
    L.o_mode = L.o_nb + align256(nr * 4);
    L.o_tasks = L.o_mode + align256(np * 4);
    L.o_ans = L.o_tasks + align256((size_t)L.task_cap * sizeof(RsTask));
    L.o_st = L.o_ans + align256((size_t)L.task_cap * sizeof(RsAns));
    L.o_cur = L.o_st + align256(slab * sizeof(gbx_mem_reg));
    L.o_ord = L.o_cur + align256(slab * 4);
    L.o_ordb = L.o_ord + align256(slab * 4);
    L.o_z = L.o_ordb + align256(slab * 4);
    L.o_excl = L.o_z + align256(slab * 4);
    L.o_key = L.o_excl + align256(slab * 4);
    L.o_eord = L.o_key + align256(2 * slab * sizeof(RegKey));
    L.total = L.o_eord + align256((size_t)reg_cap * 4);
    return L;
}

}  // namespace

size_t mem_rescue_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_matesw)
{
    return rs_layout(n_pairs < 0 ? 0 : n_pairs, reg_cap < 0 ? 0 : reg_cap, max_matesw).total;
}

int mem_rescue_launch(const gbx_mem_rescue_params *p, int64_t n_pairs, int64_t pair_id0, const MemRescueIo &io, void *d_work, size_t work_bytes,
                      hipStream_t s)
{
    if (io.reg_cap >= (1ll << 28) || n_pairs >= (1ll << 28) || io.xsel_cap >= (1ll << 31) * 256) {
        set_error("mem rescue: n_pairs, reg_cap or xsel_cap too large");
        return GBX_ERR_UNSUPPORTED;
    }
    const RsLayout L = rs_layout(n_pairs, io.reg_cap, p->max_matesw);
    if (work_bytes < L.total) { set_error("mem rescue: workspace too small"); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    RsArgs A;
    A.p = *p; A.io = io; A.n_pairs = n_pairs; A.pair_id0 = pair_id0; A.task_cap = L.task_cap;
    A.tcnt = (long long *)(wb + L.o_tcnt); A.cnt = (long long *)(wb + L.o_cnt); A.kcnt = (long long *)(wb + L.o_kcnt);
    A.n_tasks = (int64_t *)(wb + L.o_tot); A.n_kept = A.n_tasks + 1;
    A.nb = (int *)(wb + L.o_nb); A.mode = (int *)(wb + L.o_mode); A.tasks = (RsTask *)(wb + L.o_tasks); A.ans = (RsAns *)(wb + L.o_ans);
    A.st = (gbx_mem_reg *)(wb + L.o_st); A.cur = (int *)(wb + L.o_cur); A.ord = (int *)(wb + L.o_ord); A.ordb = (int *)(wb + L.o_ordb);
    A.z = (int *)(wb + L.o_z); A.excl = (int *)(wb + L.o_excl); A.key = (RegKey *)(wb + L.o_key); A.eord = (int *)(wb + L.o_eord);
    long long *const bsum = (long long *)(wb + L.o_bsum);
    const MemScanGuard guard{io.n_regs, 0, io.reg_cap};                          // -1 totals when the regs stage overflowed
    const unsigned pair_blocks = (unsigned)n_pairs;                              // plan, task and replay: a wavefront per pair
    {
        Stage st("mem_rescue_plan", s);
        if (n_pairs > 0) hipLaunchKernelGGL(mem_rescue_plan_kernel, dim3(pair_blocks), dim3(64), 0, s, A);
        mem_scan_launch({A.tcnt, n_pairs, 1, bsum, L.blocks_p, {A.n_tasks, nullptr}, nullptr, {guard, {}}}, s);
        if (n_pairs > 0) hipLaunchKernelGGL(mem_rescue_task_kernel, dim3(pair_blocks), dim3(64), 0, s, A);
    }
    if (n_pairs > 0 && L.task_cap > 0) {
        Stage st("mem_rescue_sw", s);
        const long long grid = L.task_cap < 16384 ? L.task_cap : 16384;
        hipLaunchKernelGGL(mem_rescue_sw_kernel, dim3((unsigned)grid), dim3(64), 0, s, A);
    }
    if (n_pairs > 0) {
        Stage st("mem_rescue_replay", s);
        hipLaunchKernelGGL(mem_rescue_replay_kernel, dim3(pair_blocks), dim3(64), 0, s, A);
    }
    {
        Stage st("mem_rescue_scan", s);
        mem_scan_launch({A.cnt, 2 * n_pairs, 2, bsum, L.blocks_r, {io.n_xregs, io.n_xsel}, io.xreg_off, {guard, {}}}, s);
        mem_scan_launch({A.kcnt, 2 * n_pairs, 1, bsum, L.blocks_r, {A.n_kept, nullptr}, nullptr, {guard, {}}}, s);
        hipLaunchKernelGGL(mem_rescue_count_kernel, dim3(1), dim3(1), 0, s, A);
    }
    {
        Stage st("mem_rescue_pack", s);
        // the seed records: the caller's, then zeroes that the survivors' records replace
        const int64_t keep = io.seed_cap < io.xseed_cap ? io.seed_cap : io.xseed_cap;
        if (keep > 0) GBX_HIP(hipMemcpyAsync(io.xseeds, io.seeds, (size_t)keep * sizeof(gbx_bsw_seed), hipMemcpyDeviceToDevice, s));
        if (io.xseed_cap > keep) GBX_HIP(hipMemsetAsync(io.xseeds + keep, 0, (size_t)(io.xseed_cap - keep) * sizeof(gbx_bsw_seed), s));
        if (n_pairs > 0) hipLaunchKernelGGL(mem_rescue_pack_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, A);
    }
    if (io.xsel_cap > 0) {
        Stage st("mem_rescue_tail", s);
        mem_sel_tail_launch(io.xsel_seeds, io.xsel_res, io.xsel_cap, io.n_xsel, s);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("mem rescue");
    return GBX_OK;
}

}  // namespace gbx
