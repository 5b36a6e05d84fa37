// mem_pair_kernels.hip — paired-end: the insert-size estimate, pairing and the pair decision between the alignment regions and
// the CIGAR stage (bwa-mem's mem_pestat, mem_pair and the decision part of mem_sam_pe; mate rescue is the stage before it, mem_rescue_kernels.hip) for gfx950 (MI355X).
//
// Semantics: include/gbx.h and DESIGN 3.13 (restated in tests/mem_pair_ref.py, which pins them).
//
// Shape: that of mem_regs_kernels.hip and mem_chain_kernels.hip, plus one reduction across the call.
//   * estimate: a lane per pair finds each end's top region and cal_sub (short scans) and adds 1 to a 32-bit bin per direction
//     and insert size - integer counts, so the bins do not depend on the scheduling.  One block of four waves, a direction per
//     wave, then walks its bins: the total, the percentiles from running prefix counts, the integer sums of avg, and S in
//     ascending order of the value (one add per occupied bin, every lane the same chain), as the rules fix it.
//   * pairing: one pair per wavefront.  The keys of both ends' regions are sorted by wave_sort of mem_common.h: in registers with
//     shuffles up to 64 and by a bitonic network over the pair's slab (twice its first region, room for the next power of two)
//     above that.  The look-back is serial in i with lanes over k downwards; the first lane beyond `high` comes from a ballot and only the lanes below it
//     make candidates.  No candidate list is kept: a first scan leaves the best two (unique (X, Y), wave reduction) and the
//     count, a second scan of the same kind counts n_sub.  No per-pair capacity, no second path.
//   * decision: uniform over the wave; the changed regions go to d_pregs at the places they have in d_regs, the reported ones
//     numbered within their read.
//   * output: per-read counts of reported regions, a scan over the reads, a pack pass that renumbers sel and writes the seed and
//     result records at their final places, a tail pass: no dependence on the scheduling.
#include <cstring>
#include "mem_common.h"

namespace gbx {
namespace {

using MpKey = WaveKey<2>;                           // (x, y) of mem_pair: w[0] the place, w[1] score, index, strand and end
static_assert(sizeof(MpKey) == 16 && sizeof(gbx_mem_pair_params) == 56 && sizeof(gbx_mem_pestat) == 32 && sizeof(gbx_mem_pair) == 56 &&
              sizeof(gbx_mem_reg) == 88, "records");

struct MpArgs {
    gbx_mem_pair_params p;
    MemPairIo io;
    long long n_pairs, pair_id0;
    int has_pes;                     // the caller's estimate is used, none is made
    gbx_mem_pestat pes_in[4];
    const gbx_mem_pestat *d_pes_in;  // the caller's estimate on the device (gbx_mem_pair_device_pes), else pes_in holds it
    long long *cnt;                  // [2 n_pairs + 1]: reported regions per read, then their exclusive scan
    unsigned *bins;                  // [4][max_ins + 1]: pairs per direction and insert size
    MpKey *key;                      // [2 reg_cap]  slab of a pair: twice its first region
};

__device__ inline bool mp_upstream_ok(const MpArgs &A) { const long long n = *A.io.n_regs; return n >= 0 && n <= A.io.reg_cap; }

struct MpSpan { long long g0, g1, g2; bool ok; };    // the pair's regions: end 0 [g0, g1), end 1 [g1, g2)
__device__ inline MpSpan mp_span(const MpArgs &A, long long p)
{
    MpSpan s;
    s.ok = mp_upstream_ok(A);
    const long long n = s.ok ? *A.io.n_regs : 0;
    s.g0 = clampll(A.io.reg_off[2 * p], 0, n);
    s.g1 = clampll(A.io.reg_off[2 * p + 1], s.g0, n);
    s.g2 = clampll(A.io.reg_off[2 * p + 2], s.g1, n);
    return s;
}

__device__ inline bool mp_overlaps(int qb, int qe, int tb, int te, float mask_level)
{
    const int b_max = qb > tb ? qb : tb, e_min = qe < te ? qe : te;
    if (e_min <= b_max) return false;
    const int l1 = qe - qb, l2 = te - tb, min_l = l1 < l2 ? l1 : l2;
    return (float)(e_min - b_max) >= (float)min_l * mask_level;
}

__device__ inline float mp_frac_rep(const MpArgs &A, long long read, const gbx_mem_reg &R)
{
    const int lq = R.seed >= 0 && R.seed < A.io.seed_cap ? A.io.seeds[R.seed].lq : 0;
    return lq > 0 ? reg_frac_rep(R, A.io.l_rep[read], lq) : 0.f;
}

__device__ inline int mp_raw_mapq(int d, int a) { return (int)(6.02 * (double)d / (double)a + .499); }

// ---- 1a: a lane per pair; the pair's insert size into its direction's bins
__global__ void __launch_bounds__(256) mem_pair_count_kernel(MpArgs A)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.n_pairs) return;
    const MpSpan S = mp_span(A, p);
    if (S.g1 == S.g0 || S.g2 == S.g1) return;
    long long rb[2];
    int rid[2];
    for (int e = 0; e < 2; ++e) {
        const gbx_mem_reg *const a = A.io.regs + (e ? S.g1 : S.g0);
        const long long n = e ? S.g2 - S.g1 : S.g1 - S.g0;
        long long t = 0;
        for (long long i = 1; i < n; ++i) {                                      // first by (score desc, rb, qb)
            const gbx_mem_reg &X = a[i], &T = a[t];
            if (X.score != T.score ? X.score > T.score : X.rb != T.rb ? X.rb < T.rb : X.qb < T.qb) t = i;
        }
        const int tb = a[t].qb, te = a[t].qe, ts = a[t].score;
        int sub = -1;
        for (long long j = 0; j < n; ++j)
            if (j != t && mp_overlaps(a[j].qb, a[j].qe, tb, te, A.p.mask_level) && (sub < 0 || a[j].score > sub)) sub = a[j].score;
        if (sub < 0) sub = A.p.min_seed_len * A.p.a;
        if ((double)sub > 0.8 * (double)ts) return;
        rb[e] = a[t].rb; rid[e] = a[t].rid;
    }
    if (rid[0] != rid[1]) return;
    long long is;
    const int d = mem_infer_dir(A.io.l_pac, rb[0], rb[1], &is);
    if (is >= 1 && is <= A.p.max_ins) atomicAdd(A.bins + (long long)d * (A.p.max_ins + 1) + is, 1u);
}

// ---- 1b: one block, a direction per wave: the estimate from the bins
__global__ void __launch_bounds__(256) mem_pair_stat_kernel(MpArgs A)
{
    __shared__ long long n_of[4];
    const int lane = threadIdx.x & 63, d = threadIdx.x >> 6;
    if (A.has_pes) {
        if (threadIdx.x < 4) {
            gbx_mem_pestat r = A.d_pes_in ? A.d_pes_in[threadIdx.x] : A.pes_in[threadIdx.x];
            if (A.d_pes_in && r.failed == 0 && !(r.std > 0.)) r.failed = 1;       // what pes_check refuses of a host pointer
            A.io.pes[threadIdx.x] = r;
        }
        return;
    }
    const int nb = A.p.max_ins + 1;
    const unsigned *const b = A.bins + (long long)d * nb;
    long long n = 0;
    for (int v0 = 0; v0 < nb; v0 += 64) n += v0 + lane < nb ? b[v0 + lane] : 0;
    for (int s = 32; s > 0; s >>= 1) n += __shfl_xor(n, s);
    if (lane == 0) n_of[d] = n;
    gbx_mem_pestat r;
    r.low = 0; r.high = 0; r.failed = 0; r.pad_ = 0; r.avg = 0.; r.std = 0.;
    if (n < 10) r.failed = 1;
    else {
        const long long i25 = (long long)(.25 * (double)n + .499), i75 = (long long)(.75 * (double)n + .499);
        int p25 = 0, p75 = 0;
        long long run = 0;                                                       // the values below this chunk
        for (int v0 = 0; v0 < nb; v0 += 64) {
            const int v = v0 + lane;
            const long long c = v < nb ? b[v] : 0;
            const long long inc = wave_scan_incl(c, lane);
                        const long long lo = run + inc - c, hi = run + inc;                  // this bin holds sorted[lo .. hi)
            const unsigned long long b25 = __ballot(lo <= i25 && i25 < hi), b75 = __ballot(lo <= i75 && i75 < hi);
            if (b25) p25 = v0 + __builtin_ctzll(b25);
            if (b75) p75 = v0 + __builtin_ctzll(b75);
            run += __shfl(inc, 63);
        }
        int low = (int)((double)p25 - 2.0 * (double)(p75 - p25) + .499);
        low = low > 1 ? low : 1;
        int high = (int)((double)p75 + 2.0 * (double)(p75 - p25) + .499);
        const int top = high < nb - 1 ? high : nb - 1;
        long long sum = 0, x = 0;
        for (int v0 = low & ~63; v0 <= top; v0 += 64) {
            const int v = v0 + lane;
            const long long c = v >= low && v <= top ? b[v] : 0;
            sum += c * v; x += c;
        }
        for (int s = 32; s > 0; s >>= 1) { sum += __shfl_xor(sum, s); x += __shfl_xor(x, s); }
        const double avg = (double)sum / (double)x;
        double S = 0.;
        for (int v0 = low & ~63; v0 <= top; v0 += 64) {                          // ascending in v: the agreed order
            const int v = v0 + lane;
            const unsigned c = v >= low && v <= top ? b[v] : 0;
            const double term = (double)c * (((double)v - avg) * ((double)v - avg));
            unsigned long long occ = __ballot(c != 0);
            for (int k = 0; k < 64; ++k) {
                if (!occ) break;
                S += __shfl(term, __builtin_ctzll(occ));
                occ &= occ - 1;
            }
        }
        const double sd = sqrt(S / (double)x);
        low = (int)((double)p25 - 3.0 * (double)(p75 - p25) + .499);
        high = (int)((double)p75 + 3.0 * (double)(p75 - p25) + .499);
        if ((double)low > avg - 4.0 * sd) low = (int)(avg - 4.0 * sd + .499);
        if ((double)high < avg + 4.0 * sd) high = (int)(avg + 4.0 * sd + .499);
        r.low = low > 1 ? low : 1; r.high = high; r.avg = avg; r.std = sd;
    }
    __syncthreads();
    long long most = 0;
    for (int k = 0; k < 4; ++k) most = n_of[k] > most ? n_of[k] : most;
    if (!r.failed && (double)n < 0.05 * (double)most) r.failed = 1;
    if (lane == 0) A.io.pes[d] = r;
}

__device__ inline bool mp_above(unsigned long long X, unsigned long long Y, unsigned long long X2, unsigned long long Y2)
{
    return X != X2 ? X > X2 : Y > Y2;
}

struct MpBest { unsigned long long X, Y, X2, Y2; int n; };   // a lane's best two candidates (Y = 0: none) and its count

// The look-back of mem_pair over the sorted keys.  count_sub false: every lane keeps its best two candidates and their number;
// true: it counts the candidates other than (bX, bY) with sub - q <= tmp.
__device__ inline void mp_lookback(const MpKey *key, int n, const gbx_mem_pestat *pes, const gbx_mem_pair_params &p,
                                   unsigned long long id8, int lane, bool count_sub, unsigned long long bX, unsigned long long bY,
                                   int sub, int tmp, MpBest &B)
{
    int l0 = -1, l1 = -1, l2 = -1, l3 = -1;
    for (int i = 0; i < n; ++i) {
        const MpKey ki = key[i];
        for (int r = 0; r < 2; ++r) {
            const int dir = r << 1 | (int)(ki.w[1] >> 1 & 1);
            const gbx_mem_pestat pe = pes[dir];
            if (pe.failed) continue;
            const int which = r << 1 | (int)((ki.w[1] & 1) ^ 1);
            const int lw = which == 0 ? l0 : which == 1 ? l1 : which == 2 ? l2 : l3;
            for (int jb = 0; jb <= lw; jb += 64) {
                const int k = lw - jb - lane;
                MpKey kk = {{0, 0}};
                if (k >= 0) kk = key[k];
                const bool match = k >= 0 && (int)(kk.w[1] & 3) == which;
                const long long dist = (long long)(ki.w[0] - kk.w[0]);
                const unsigned long long bs = __ballot(match && dist > pe.high);
                const int first = bs ? __builtin_ctzll(bs) : 64;
                if (match && lane < first && dist >= pe.low) {
                    const double ns = ((double)dist - pe.avg) / pe.std;
                    const double qd = (double)((ki.w[1] >> 32) + (kk.w[1] >> 32)) + .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * (double)p.a + .499;
                    const int q = qd > 0. ? (int)qd : 0;                          // -inf (erfc underflowed) and NaN give 0
                    const unsigned long long Y = (unsigned long long)k << 32 | (unsigned)i;
                    const unsigned long long X = (unsigned long long)q << 32 | (hash64(Y ^ id8) & 0xffffffffull);
                    if (count_sub) {
                        if (!(X == bX && Y == bY) && sub - q <= tmp) ++B.n;
                    } else {
                        ++B.n;
                        if (mp_above(X, Y, B.X, B.Y)) { B.X2 = B.X; B.Y2 = B.Y; B.X = X; B.Y = Y; }
                        else if (mp_above(X, Y, B.X2, B.Y2)) { B.X2 = X; B.Y2 = Y; }
                    }
                }
                if (bs) break;
            }
        }
        const int w = (int)(ki.w[1] & 3);
        if (w == 0) l0 = i; else if (w == 1) l1 = i; else if (w == 2) l2 = i; else l3 = i;
    }
}

// ---- 2, 3: one pair per wavefront: pairing, the decision, the pair's regions into d_pregs (sel: the place within the read)
__global__ void __launch_bounds__(64) mem_pair_pair_kernel(MpArgs A)
{
    __shared__ gbx_mem_pestat pes[4];
    const long long pr = blockIdx.x;
    const int lane = threadIdx.x;
    const gbx_mem_pair_params p = A.p;
    const MpSpan S = mp_span(A, pr);
    if (lane < 4) pes[lane] = A.io.pes[lane];
    __syncthreads();
    gbx_mem_pair out;
    out.dist = 0; out.score = 0; out.sub = 0; out.n_sub = 0; out.n_cand = 0; out.z0 = 0; out.z1 = 0; out.q_pe = 0; out.q_se0 = 0;
    out.q_se1 = 0; out.paired = 0; out.proper = 0; out.dir = 0;
    if (!S.ok) {
        if (lane == 0) { A.io.pairs[pr] = out; A.cnt[2 * pr] = 0; A.cnt[2 * pr + 1] = 0; }
        return;
    }
    const gbx_mem_reg *const rg = A.io.regs + S.g0;
    const int n0 = (int)(S.g1 - S.g0), n1 = (int)(S.g2 - S.g1), n = n0 + n1;
    const long long L = A.io.l_pac;
    const unsigned long long below = (1ull << lane) - 1;
    int tmp = p.a + p.b;
    tmp = p.o_del + p.e_del > tmp ? p.o_del + p.e_del : tmp;
    tmp = p.o_ins + p.e_ins > tmp ? p.o_ins + p.e_ins : tmp;

    // ---- 2: pairing
    int z[2] = {-1, -1};
    if (n0 > 0 && n1 > 0 && !p.no_pairing) {
        MpKey *const key = A.key + 2 * S.g0;
        for (int t = lane; t < n; t += 64) {
            const int e = t >= n0, i = e ? t - n0 : t;
            const gbx_mem_reg &R = rg[t];
            const bool rev = R.rb >= L;
            const long long fwd = rev ? 2 * L - 1 - R.rb : R.rb;
            const long long off = R.rid >= 0 && R.rid < A.io.n_contigs ? A.io.contig_off[R.rid] : 0;
            MpKey v;
            v.w[0] = (unsigned long long)R.rid << 32 | (unsigned long long)(fwd - off);
            v.w[1] = (unsigned long long)R.score << 32 | (unsigned long long)i << 2 | (rev ? 2u : 0u) | (unsigned)e;
            key[t] = v;
        }
        __syncthreads();
        wave_sort(key, n, lane);
        const unsigned long long id8 = (unsigned long long)(A.pair_id0 + pr) << 8;
        MpBest B = {0, 0, 0, 0, 0};
        mp_lookback(key, n, pes, p, id8, lane, false, 0, 0, 0, 0, B);
        int n_cand = B.n;
        unsigned long long gX = B.X, gY = B.Y;
        for (int s = 32; s > 0; s >>= 1) {
            n_cand += __shfl_xor(n_cand, s);
            const unsigned long long oX = __shfl_xor(gX, s), oY = __shfl_xor(gY, s);
            if (mp_above(oX, oY, gX, gY)) { gX = oX; gY = oY; }
        }
        const bool mine = B.X == gX && B.Y == gY;
        unsigned long long sX = mine ? B.X2 : B.X, sY = mine ? B.Y2 : B.Y;      // the best of the rest
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long oX = __shfl_xor(sX, s), oY = __shfl_xor(sY, s);
            if (mp_above(oX, oY, sX, sY)) { sX = oX; sY = oY; }
        }
        out.n_cand = n_cand;
        if (n_cand > 0) {
            const unsigned long long y1 = key[gY >> 32].w[1], y2 = key[gY & 0xffffffffull].w[1];
            z[y1 & 1] = (int)((y1 & 0xffffffffull) >> 2);
            z[y2 & 1] = (int)((y2 & 0xffffffffull) >> 2);
            out.score = (int)(gX >> 32);
            if (n_cand > 1) {
                out.sub = (int)(sX >> 32);
                MpBest C = {0, 0, 0, 0, 0};
                mp_lookback(key, n, pes, p, id8, lane, true, gX, gY, out.sub, tmp, C);
                int n_sub = C.n;
                for (int s = 32; s > 0; s >>= 1) n_sub += __shfl_xor(n_sub, s);
                out.n_sub = n_sub;
            }
        }
    }

    // ---- 3: the decision
    bool multi = false;
    for (int e = 0; e < 2; ++e) {
        const gbx_mem_reg *const a = rg + (e ? n0 : 0);
        const int ne = e ? n1 : n0;
        for (int j0 = 1; j0 < ne; j0 += 64) {
            const int j = j0 + lane;
            if (__ballot(j < ne && a[j].secondary < 0 && a[j].score >= p.T)) { multi = true; break; }
        }
    }
    int q_se[2] = {0, 0}, c_sub[2] = {0, 0}, c_sec[2] = {0, 0};
    const bool paired = out.score > 0 && !multi && z[0] >= 0 && z[0] < n0 && z[1] >= 0 && z[1] < n1;
    if (paired) {
        const gbx_mem_reg *const a[2] = {rg, rg + n0};
        const int ne[2] = {n0, n1};
        const float fr[2] = {mp_frac_rep(A, 2 * pr, a[0][0]), mp_frac_rep(A, 2 * pr + 1, a[1][0])};
        const int score_un = a[0][0].score + a[1][0].score - p.pen_unpaired;
        const int subo = out.sub > score_un ? out.sub : score_un;
        int q_pe = mp_raw_mapq(out.score - subo, p.a);
        if (out.n_sub > 0) q_pe -= (int)(4.343 * log((double)(out.n_sub + 1)) + .499);
        q_pe = q_pe < 0 ? 0 : q_pe > 60 ? 60 : q_pe;
        q_pe = (int)((double)q_pe * (1. - .5 * (double)(fr[0] + fr[1])) + .499);
        out.q_pe = q_pe;
        if (out.score > score_un) {
            for (int e = 0; e < 2; ++e) {
                gbx_mem_reg c = a[e][z[e]];
                if (c.secondary >= 0) {
                    c.sub = a[e][c.secondary < ne[e] ? c.secondary : 0].score;
                    c.secondary = -2;
                }
                int q = approx_mapq_se(c, fr[e], p);
                q = q > q_pe ? q : q_pe < q + 40 ? q_pe : q + 40;
                const int cap = mp_raw_mapq(c.score - c.csub, p.a);
                q_se[e] = q < cap ? q : cap;
                c_sub[e] = c.sub; c_sec[e] = c.secondary;
            }
            out.proper = 1;
        } else {
            for (int e = 0; e < 2; ++e) {
                z[e] = 0;
                q_se[e] = approx_mapq_se(a[e][0], fr[e], p);
                c_sub[e] = a[e][0].sub; c_sec[e] = a[e][0].secondary;
            }
        }
        out.paired = 1;
    } else {
        z[0] = n0 > 0 && rg[0].score >= p.T ? 0 : -1;
        z[1] = n1 > 0 && rg[n0].score >= p.T ? 0 : -1;
        q_se[0] = z[0] == 0 ? rg[0].mapq : 0;
        q_se[1] = z[1] == 0 ? rg[n0].mapq : 0;
        if (!p.no_pairing && z[0] == 0 && z[1] == 0 && rg[0].rid == rg[n0].rid) {
            long long dist;
            const int d = mem_infer_dir(L, rg[0].rb, rg[n0].rb, &dist);
            out.proper = !pes[d].failed && dist >= pes[d].low && dist <= pes[d].high;
        }
    }
    out.z0 = z[0]; out.z1 = z[1]; out.q_se0 = q_se[0]; out.q_se1 = q_se[1];
    out.dir = -1;
    if (z[0] >= 0 && z[1] >= 0) {
        long long dist;
        out.dir = mem_infer_dir(L, rg[z[0]].rb, rg[n0 + z[1]].rb, &dist);
        out.dist = dist;
    }

    // ---- the pair's regions as they leave; the reported ones numbered within their read
    for (int e = 0; e < 2; ++e) {
        const gbx_mem_reg *const a = rg + (e ? n0 : 0);
        gbx_mem_reg *const o = A.io.pregs + S.g0 + (e ? n0 : 0);
        const int ne = e ? n1 : n0;
        int k = 0;
        for (int b0 = 0; b0 < ne; b0 += 64) {
            const int i = b0 + lane;
            const bool act = i < ne;
            gbx_mem_reg R;
            bool rep = false;
            if (act) {
                R = a[i];
                if (paired) {
                    rep = i == z[e];
                    R.flag = rep ? 1 : 0;
                    if (rep) { R.mapq = q_se[e]; R.sub = c_sub[e]; R.secondary = c_sec[e]; }
                } else
                    rep = (R.flag & 1) != 0;
            }
            const unsigned long long br = __ballot(rep);
            if (act) {
                R.sel = rep ? k + __builtin_popcountll(br & below) : -1;
                o[i] = R;
            }
            k += __builtin_popcountll(br);
        }
        if (lane == 0) A.cnt[2 * pr + e] = k;
    }
    if (lane == 0) A.io.pairs[pr] = out;
}

// ---- sel renumbered and the CIGAR list's records at their final places: lanes over the pair's regions
__global__ void __launch_bounds__(64) mem_pair_pack_kernel(MpArgs A)
{
    const long long pr = blockIdx.x;
    const MpSpan S = mp_span(A, pr);
    if (!S.ok) return;
    for (long long t = S.g0 + threadIdx.x; t < S.g2; t += 64) {
        gbx_mem_reg *const R = A.io.pregs + t;
        if (R->sel < 0) continue;
        const long long gs = A.cnt[2 * pr + (t >= S.g1)] + R->sel;
        R->sel = (int32_t)gs;
        if (gs >= A.io.psel_cap) continue;
        const long long old = A.io.regs[t].sel;
        gbx_bsw_seed s;
        gbx_bsw_seed_result e;
        if (old >= 0 && old < A.io.sel_cap) {                                    // a copy of the regs stage's records
            s = A.io.sel_seeds[old]; e = A.io.sel_res[old];
        } else if (R->seed >= 0 && R->seed < A.io.seed_cap) {                    // not reported there: built as that stage builds them
            s = A.io.seeds[R->seed];
            e = reg_result(*R, s);
        } else {
            memset(&s, 0, sizeof(s));
            memset(&e, 0xff, sizeof(e));
        }
        A.io.psel_seeds[gs] = s;
        A.io.psel_res[gs] = e;
    }
}

struct MpLayout { size_t o_cnt, o_bsum, o_bins, o_key, bins_bytes, total; int blocks; };
MpLayout mp_layout(int64_t n_pairs, int64_t reg_cap, int32_t max_ins)
{
    MpLayout L;
    const size_t nr = 2 * (size_t)n_pairs;
    L.blocks = mem_scan_blocks(2 * n_pairs);
    L.bins_bytes = 4 * ((size_t)max_ins + 1) * 4;
    L.o_cnt = 0;
    L.o_bsum = L.o_cnt + align256((nr + 1) * 8);
    L.o_bins = L.o_bsum + align256((size_t)L.blocks * 8);
    L.o_key = L.o_bins + align256(L.bins_bytes);
    L.total = L.o_key + align256(2 * (size_t)reg_cap * sizeof(MpKey));
    return L;
}

}  // namespace

size_t mem_pair_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_ins)
{
    return mp_layout(n_pairs < 0 ? 0 : n_pairs, reg_cap < 0 ? 0 : reg_cap, max_ins < 1 ? 1 : max_ins > (1 << 20) ? 1 << 20 : max_ins).total;
}

namespace {
// step 1 on the stream: the bins, the counts, the walk - or, with the caller's estimate, its copy into io.pes
int mp_pestat(const MpArgs &A, size_t bins_bytes, hipStream_t s)
{
    if (!A.has_pes) {
        GBX_HIP(hipMemsetAsync(A.bins, 0, bins_bytes, s));
        if (A.n_pairs > 0) hipLaunchKernelGGL(mem_pair_count_kernel, dim3((unsigned)((A.n_pairs + 255) / 256)), dim3(256), 0, s, A);
    }
    hipLaunchKernelGGL(mem_pair_stat_kernel, dim3(1), dim3(256), 0, s, A);
    return GBX_OK;
}
}  // namespace

size_t mem_pestat_workspace_bytes(int32_t max_ins)
{
    return align256(4 * ((size_t)(max_ins < 1 ? 1 : max_ins > (1 << 20) ? 1 << 20 : max_ins) + 1) * 4);
}

// step 1 alone, from the kernels of mem_pair_launch: the same bins, the same walk, so the same bytes in io.pes
int mem_pestat_launch(const gbx_mem_pair_params *p, int64_t n_pairs, const MemPairIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    if (io.reg_cap >= (1ll << 30)) { set_error("mem pestat: reg_cap too large"); return GBX_ERR_UNSUPPORTED; }
    const size_t bins_bytes = 4 * ((size_t)p->max_ins + 1) * 4;
    if (work_bytes < bins_bytes) { set_error("mem pestat: workspace too small"); return GBX_ERR_ARG; }
    MpArgs A;
    A.p = *p; A.io = io; A.n_pairs = n_pairs; A.pair_id0 = 0; A.has_pes = 0; A.d_pes_in = nullptr;
    for (int d = 0; d < 4; ++d) A.pes_in[d] = gbx_mem_pestat{0, 0, 1, 0, 0., 0.};
    A.cnt = nullptr; A.bins = (unsigned *)d_work; A.key = nullptr;
    Stage st("mem_pestat", s);
    const int rc = mp_pestat(A, bins_bytes, s);
    if (rc) return rc;
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

int mem_pair_launch(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0, const MemPairIo &io, const gbx_mem_pestat *pes_in,
                    void *d_work, size_t work_bytes, hipStream_t s, const gbx_mem_pestat *d_pes_in)
{
    if (io.reg_cap >= (1ll << 30) || io.psel_cap >= (1ll << 31) * 256) { set_error("mem pair: reg_cap or psel_cap too large"); return GBX_ERR_UNSUPPORTED; }
    const MpLayout L = mp_layout(n_pairs, io.reg_cap, p->max_ins);
    if (work_bytes < L.total) { set_error("mem pair: workspace too small"); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    MpArgs A;
    A.p = *p; A.io = io; A.n_pairs = n_pairs; A.pair_id0 = pair_id0;
    A.has_pes = pes_in != nullptr || d_pes_in != nullptr;
    A.d_pes_in = d_pes_in;
    for (int d = 0; d < 4; ++d) A.pes_in[d] = pes_in ? pes_in[d] : gbx_mem_pestat{0, 0, 1, 0, 0., 0.};
    A.cnt = (long long *)(wb + L.o_cnt); A.bins = (unsigned *)(wb + L.o_bins);
    A.key = (MpKey *)(wb + L.o_key);
    {
        Stage st("mem_pair_pestat", s);
        const int rc = mp_pestat(A, L.bins_bytes, s);
        if (rc) return rc;
    }
    if (n_pairs > 0) {
        Stage st("mem_pair_pair", s);
        hipLaunchKernelGGL(mem_pair_pair_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, A);
    }
    {
        Stage st("mem_pair_scan", s);
        // the total is -1 when the regs stage overflowed: the condition of mp_upstream_ok
        mem_scan_launch({A.cnt, 2 * n_pairs, 1, (long long *)(wb + L.o_bsum), L.blocks, {io.n_psel, nullptr}, nullptr,
                         {{io.n_regs, 0, io.reg_cap}, {}}}, s);
    }
    if (n_pairs > 0) {
        Stage st("mem_pair_pack", s);
        hipLaunchKernelGGL(mem_pair_pack_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, A);
    }
    if (io.psel_cap > 0) {
        Stage st("mem_pair_tail", s);
        mem_sel_tail_launch(io.psel_seeds, io.psel_res, io.psel_cap, io.n_psel, s);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("mem pair");
    return GBX_OK;
}

}  // namespace gbx
