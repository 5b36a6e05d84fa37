// mem_common.h — what the bwa-mem stage files (mem_chain / mem_cigar / mem_regs / mem_pair _kernels.hip) share on the device:
// the small helpers, the mapq formula, the one-wave key sort, the CIGAR-list record and the pieces of the exclusive scan over
// per-unit counts.  fmi_kernels.hip and fmi_sal_kernels.hip use the scan's pieces inside their fused kernels.  The scan's own
// kernels and the CIGAR list's tail kernel are in mem_scan.hip (mem_scan_launch, mem_sel_tail_launch: gbx_internal.h).
#pragma once
#include "gbx_internal.h"

namespace gbx {

constexpr int MEM_SCAN = 1024;                      // entries a block of the scan takes
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int mem_scan_blocks(int64_t n) { return (int)((n + 1 + MEM_SCAN - 1) / MEM_SCAN); }     // n counts make n + 1 offsets

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

// mem_approx_mapq_se with csub = 0 on the region's sub and sub_n; everything in double but frac_rep.  P has a, b,
// min_seed_len, mapq_coef_len, mapq_coef_fac
template <class P>
__device__ inline int approx_mapq_se(const gbx_mem_reg &R, float frac_rep, const P &p)
{
    const int sub = R.sub ? R.sub : p.min_seed_len * p.a;
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

// ---- the CIGAR list's result record of a region: what the extension would have answered for it on the region's seed
__device__ inline gbx_bsw_seed_result reg_result(const gbx_mem_reg &R, const gbx_bsw_seed &s)
{
    gbx_bsw_seed_result e;
    e.score = R.score; e.truesc = R.truesc; e.qb = R.qb; e.qe = R.qe;
    e.rb = (int32_t)(R.rb - s.roff); e.re = (int32_t)(R.re - s.roff); e.w = R.w; e.sc0 = 0;
    return e;
}

// ---- exclusive scan, the pieces.  A block scans its entries (block_scan_excl) and leaves its sum; one block scans the sums
// (scan_block_sums); an offset pass adds a block's scanned sum to its entries.
template <class T>
__device__ inline T wave_scan_incl(T v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) { const T u = __shfl_up(v, d); if (lane >= d) v += u; }
    return v;
}

// every thread of the block calls it with its count c; -> the sum of the counts of the threads before it.  sh: a long long per
// wavefront of the block.  *block_total: the sum up to and including this thread - in the block's last thread, the block's sum.
__device__ inline long long block_scan_excl(long long c, long long *sh, long long *block_total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long v = wave_scan_incl(c, lane);
    if (lane == 63) sh[wv] = v;
    __syncthreads();
    long long before = 0;
    for (int w = 0; w < wv; ++w) before += sh[w];
    *block_total = before + v;
    return before + v - c;
}

// one block of 1024 threads: bsum[0 .. blocks) becomes its exclusive scan; -> the total (in every thread)
__device__ inline long long scan_block_sums(long long *bsum, int blocks)
{
    __shared__ long long sh[1024];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < blocks; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const long long v = i < blocks ? bsum[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const long long u = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += u;
            __syncthreads();
        }
        if (i < blocks) bsum[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    return carry;
}

}  // namespace gbx
