// mem_common.h — what the bwa-mem stage files (mem_chain / mem_cigar / mem_regs / mem_pair / mem_rescue / mem_sam _kernels.hip) share on the device
// and nobody else uses: the small helpers, the mapq formula, the one-wave key sort, the wave-wide steps on a read's regions and
// the CIGAR-list record.  The helpers that are not bwa-mem's (align256, the pieces of the exclusive scan) are in dev_prims.h,
// which this includes; the CIGAR list's tail kernel is in mem_scan.hip (mem_sel_tail_launch: gbx_internal.h).
#pragma once
#include "dev_prims.h"

namespace gbx {

__device__ inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ inline unsigned long long hash64(unsigned long long k)
{
    k += ~(k << 32); k ^= k >> 22; k += ~(k << 13); k ^= k >> 8; k += k << 3; k ^= k >> 15; k += ~(k << 27); k ^= k >> 31;
    return k;
}

// bwa's cal_max_gap for a query stretch of q bases; P has a, o_del, e_del, o_ins, e_ins, w
template <class P>
__device__ inline long long max_gap(long long q, const P &p)
{
    const long long gd = (long long)((double)(q * p.a - p.o_del) / p.e_del + 1.);
    const long long gi = (long long)((double)(q * p.a - p.o_ins) / p.e_ins + 1.);
    long long g = gd > gi ? gd : gi;
    g = g > 1 ? g : 1;
    const long long w2 = 2ll * p.w;
    return g < w2 ? g : w2;
}

// bwa's mem_infer_dir: the direction (0 FF, 1 FR, 2 RF, 3 RR) and the distance of two places on the 2 L text
__device__ inline int mem_infer_dir(long long L, long long b1, long long b2, long long *dist)
{
    const bool r1 = b1 >= L, r2 = b2 >= L;
    const long long p2 = r1 == r2 ? b2 : 2 * L - 1 - b2;
    *dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// a region's frac_rep: l_rep of its read over its seed's lq; 0 for a region without a seed (mate rescue: seedlen0 == 0)
__device__ inline float reg_frac_rep(const gbx_mem_reg &R, int l_rep, int lq)
{
    return R.seedlen0 == 0 ? 0.f : (float)l_rep / (float)lq;
}

// mem_approx_mapq_se on the region's sub, sub_n and csub (0 but for a rescued region); everything in double but frac_rep.
// P has a, b, min_seed_len, mapq_coef_len, mapq_coef_fac
template <class P>
__device__ inline int approx_mapq_se(const gbx_mem_reg &R, float frac_rep, const P &p)
{
    int sub = R.sub ? R.sub : p.min_seed_len * p.a;
    sub = sub > R.csub ? sub : R.csub;
    if (sub >= R.score) return 0;
    const long long lr = R.re - R.rb;
    const int l = R.qe - R.qb > lr ? R.qe - R.qb : (int)lr;
    if (l < 1 || R.score == 0) return 0;
    const double identity = 1. - (double)(l * p.a - R.score) / (double)(p.a + p.b) / (double)l;
    double t = l < p.mapq_coef_len ? 1. : (double)p.mapq_coef_fac / log((double)l);
    t *= identity * identity;
    int mapq = (int)(6.02 * (double)(R.score - sub) / (double)p.a * t * t + .499);
    if (R.sub_n > 0) mapq -= (int)(4.343 * log((double)(R.sub_n + 1)) + .499);
    mapq = mapq > 60 ? 60 : mapq;
    mapq = mapq < 0 ? 0 : mapq;
    return (int)((double)mapq * (1. - (double)frac_rep) + .499);
}

// ---- sort of one wavefront: keys of W 64-bit words, compared word by word
template <int W> struct WaveKey { unsigned long long w[W]; };

template <int W>
__device__ inline bool key_less(const WaveKey<W> &x, const WaveKey<W> &y)
{
#pragma unroll
    for (int i = 0; i < W - 1; ++i)
        if (x.w[i] != y.w[i]) return x.w[i] < y.w[i];
    return x.w[W - 1] < y.w[W - 1];
}

// ascending sort of key[0 .. n) in place: in registers with shuffles up to 64 keys, a bitonic network over the slab above that
// (the slab has room for the next power of two, padded with all-ones keys).  The caller's stores to key are ordered before it
// by a barrier, and it ends in one.
template <int W>
__device__ inline void wave_sort(WaveKey<W> *key, int n, int lane)
{
    WaveKey<W> pad;
#pragma unroll
    for (int i = 0; i < W; ++i) pad.w[i] = ~0ull;
    if (n <= 64) {
        WaveKey<W> v = lane < n ? key[lane] : pad;
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                WaveKey<W> o;
#pragma unroll
                for (int i = 0; i < W; ++i) o.w[i] = __shfl_xor(v.w[i], j);
                const bool up = (lane & k) == 0, lower = (lane & j) == 0;
                if ((lower == up) ? key_less(o, v) : key_less(v, o)) v = o;
            }
        if (lane < n) key[lane] = v;
    } else {
        int P = 64;
        for (int it = 0; it < 25; ++it) { if (P >= n) break; P <<= 1; }
        for (int i = n + lane; i < P; i += 64) key[i] = pad;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;
                    const WaveKey<W> x = key[i], y = key[o];
                    const bool up = (i & k) == 0;
                    if (key_less(y, x) == up && (key_less(y, x) || key_less(x, y))) { key[i] = y; key[o] = x; }
                }
                __syncthreads();
            }
    }
    __syncthreads();
}

// ---- the wave-wide steps on a read's regions that the regs stage and the rescue stage share.  One wavefront, uniform control
// flow; the regions stay where they are in rg and the orders are index lists; lane 0 (or the one lane a ballot picks) stores, and
// a barrier (free for a one-wave block) orders the store before the next step's loads.  key: room for the next power of two
// above n.  P has max_chain_gap, mask_level_redun (dedup), a, b, the gap costs, mask_level (primary), T and approx_mapq_se's.
using RegKey = WaveKey<3>;                          // the low 32 bits of the last word: the element's index
constexpr unsigned long long REG_SIGN = 1ull << 63;

// mem_sort_dedup_patch without the patch on the list in[0, n) (null: 0 .. n - 1), ties of re by the position in the list; the
// survivors end up in ordb by (score desc, rb, qb) -> their number.  excl is indexed as rg is
template <class P>
__device__ inline int wave_reg_dedup(const gbx_mem_reg *rg, const int *in, int n, int *ord, int *ordb, int *excl, RegKey *key, const P &p,
                                     int lane)
{
    const unsigned long long below = (1ull << lane) - 1;
    if (n < 2) {
        if (n == 1 && lane == 0) ordb[0] = in ? in[0] : 0;
        __syncthreads();
        return n;
    }
    for (int i = lane; i < n; i += 64) {
        const int c = in ? in[i] : i;
        RegKey v;
        v.w[0] = (unsigned long long)rg[c].re ^ REG_SIGN; v.w[1] = 0; v.w[2] = (unsigned)i;
        key[i] = v;
        excl[c] = 0;
    }
    __syncthreads();
    wave_sort(key, n, lane);
    for (int i = lane; i < n; i += 64) { const int k = (int)(unsigned)key[i].w[2]; ord[i] = in ? in[k] : k; }
    __syncthreads();
    for (int i = 1; i < n; ++i) {
        const int ci = ord[i];
        const gbx_mem_reg P_ = rg[ci];
        for (int jb = 0; jb < i; jb += 64) {
            const int j = i - 1 - jb - lane;
            bool wstop = false, pstop = false, qex = false;
            int cj = 0;
            if (j >= 0) {
                cj = ord[j];
                const gbx_mem_reg Q = rg[cj];
                if (!(Q.rid == P_.rid && P_.rb < Q.re + p.max_chain_gap)) wstop = true;
                else if (!excl[cj]) {
                    const long long orr = Q.re - P_.rb;
                    const long long oq = Q.qb < P_.qb ? Q.qe - P_.qb : P_.qe - Q.qb;
                    const long long lrq = Q.re - Q.rb, lrp = P_.re - P_.rb, mr = lrq < lrp ? lrq : lrp;
                    const long long lqq = Q.qe - Q.qb, lqp = P_.qe - P_.qb, mq = lqq < lqp ? lqq : lqp;
                    if ((float)orr > p.mask_level_redun * (float)mr && (float)oq > p.mask_level_redun * (float)mq) {
                        if (P_.score < Q.score) pstop = true; else qex = true;
                    }
                }
            }
            const unsigned long long bs = __ballot(wstop || pstop);
            const int first = bs ? __builtin_ctzll(bs) : 64;
            if (qex && lane < first) excl[cj] = 1;
            if (bs) {
                if (lane == first && pstop) excl[ci] = 1;
                break;
            }
        }
        __syncthreads();
    }
    int n2 = 0;
    for (int b0 = 0; b0 < n; b0 += 64) {
        const int i = b0 + lane;
        const int c = i < n ? ord[i] : 0;
        const bool keep = i < n && !excl[c];
        const unsigned long long bk = __ballot(keep);
        if (keep) ordb[n2 + __builtin_popcountll(bk & below)] = c;
        n2 += __builtin_popcountll(bk);
    }
    __syncthreads();
    for (int i = lane; i < n2; i += 64) {
        const gbx_mem_reg &Q = rg[ordb[i]];
        RegKey v;
        v.w[0] = (unsigned long long)(0x7fffffffll - Q.score);
        v.w[1] = (unsigned long long)Q.rb ^ REG_SIGN;
        v.w[2] = (unsigned long long)((unsigned)Q.qb ^ 0x80000000u) << 32 | (unsigned)i;
        key[i] = v;
    }
    __syncthreads();
    wave_sort(key, n2, lane);
    for (int i = lane; i < n2; i += 64) ord[i] = ordb[(unsigned)key[i].w[2]];
    __syncthreads();
    int n3 = 0;                                                                   // a hit identical to the one before it goes
    for (int b0 = 0; b0 < n2; b0 += 64) {
        const int i = b0 + lane;
        bool keep = i < n2;
        const int c = keep ? ord[i] : 0;
        if (keep && i > 0) {
            const gbx_mem_reg &X = rg[c], &Y = rg[ord[i - 1]];
            keep = !(X.score == Y.score && X.rb == Y.rb && X.qb == Y.qb);
        }
        const unsigned long long bk = __ballot(keep);
        __builtin_amdgcn_wave_barrier();
        if (keep) ordb[n3 + __builtin_popcountll(bk & below)] = c;
        n3 += __builtin_popcountll(bk);
    }
    __syncthreads();
    return n3;
}

// mem_mark_primary_se on the list ordb[0, n) whose regions have sub = sub_n = 0 and secondary = -1: ord becomes the output order
// by (score desc, hash_64(read_id + i), i), z holds the primaries' places in it
template <class P>
__device__ inline void wave_reg_mark_primary(gbx_mem_reg *rg, const int *ordb, int n, int *ord, int *z, RegKey *key, long long read_id,
                                             const P &p, int lane)
{
    for (int i = lane; i < n; i += 64) {
        RegKey v;
        v.w[0] = (unsigned long long)(0x7fffffffll - rg[ordb[i]].score);
        v.w[1] = hash64((unsigned long long)(read_id + i));
        v.w[2] = (unsigned)i;
        key[i] = v;
    }
    __syncthreads();
    wave_sort(key, n, lane);
    for (int i = lane; i < n; i += 64) ord[i] = ordb[(unsigned)key[i].w[2]];
    if (n > 0 && lane == 0) z[0] = 0;
    __syncthreads();
    int tmp = p.a + p.b;
    tmp = p.o_del + p.e_del > tmp ? p.o_del + p.e_del : tmp;
    tmp = p.o_ins + p.e_ins > tmp ? p.o_ins + p.e_ins : tmp;
    int nz = n > 0 ? 1 : 0;
    for (int i = 1; i < n; ++i) {
        const int ci = ord[i];
        const int bi = rg[ci].qb, ei = rg[ci].qe, sci = rg[ci].score;
        bool hit = false;
        for (int kb = 0; kb < nz; kb += 64) {
            const int k = kb + lane;
            bool stop = false;
            int j = 0, cj = 0;
            if (k < nz) {
                j = z[k];
                cj = ord[j];
                const int bj = rg[cj].qb, ej = rg[cj].qe;
                const int b_max = bj > bi ? bj : bi, e_min = ej < ei ? ej : ei;
                if (e_min > b_max) {
                    const int li = ei - bi, lj = ej - bj, min_l = li < lj ? li : lj;
                    stop = (float)(e_min - b_max) >= (float)min_l * p.mask_level;
                }
            }
            const unsigned long long bs = __ballot(stop);
            if (bs) {
                if (lane == __builtin_ctzll(bs)) {
                    if (rg[cj].sub == 0) rg[cj].sub = sci;
                    if (rg[cj].score - sci <= tmp) ++rg[cj].sub_n;
                    rg[ci].secondary = j;
                }
                hit = true;
                break;
            }
        }
        if (!hit) {
            if (lane == 0) z[nz] = i;
            ++nz;
        }
        __syncthreads();
    }
}

// mapq and the report rule on the output order ord[0, n): mapq, flag and sel (the place among the read's reported regions) of
// every region -> the number reported.  frac_of(R): the region's frac_rep.  (bwa's drop_ratio test of a reported
// region is dead behind `secondary < 0` and is left out.)
template <class P, class FR>
__device__ inline int wave_reg_report(gbx_mem_reg *rg, const int *ord, int n, FR frac_of, const P &p, int lane)
{
    const unsigned long long below = (1ull << lane) - 1;
    int n_rep = 0, first_mapq = 0;
    for (int b0 = 0; b0 < n; b0 += 64) {
        const int i = b0 + lane;
        const bool act = i < n;
        const int c = act ? ord[i] : 0;
        int mq = 0;
        bool rep = false;
        if (act) {
            const gbx_mem_reg R = rg[c];
            if (R.secondary < 0) mq = approx_mapq_se(R, frac_of(R), p);
            rep = R.score >= p.T && R.secondary < 0;
        }
        const unsigned long long br = __ballot(rep);
        if (n_rep == 0 && br) first_mapq = __shfl(mq, __builtin_ctzll(br));
        const int my = n_rep + __builtin_popcountll(br & below);
        if (act) {
            int flag = 0, sel = -1;
            if (rep) {
                flag = 1; sel = my;
                if (my > 0) { flag |= 0x800; mq = mq < first_mapq ? mq : first_mapq; }
            }
            rg[c].mapq = mq; rg[c].flag = flag; rg[c].sel = sel;
        }
        n_rep += __builtin_popcountll(br);
    }
    return n_rep;
}

// ---- the CIGAR list's result record of a region: what the extension would have answered for it on the region's seed
__device__ inline gbx_bsw_seed_result reg_result(const gbx_mem_reg &R, const gbx_bsw_seed &s)
{
    gbx_bsw_seed_result e;
    e.score = R.score; e.truesc = R.truesc; e.qb = R.qb; e.qe = R.qe;
    e.rb = (int32_t)(R.rb - s.roff); e.re = (int32_t)(R.re - s.roff); e.w = R.w; e.sc0 = 0;
    return e;
}

}  // namespace gbx
