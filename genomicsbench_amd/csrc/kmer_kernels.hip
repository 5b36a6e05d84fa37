// kmer_kernels.hip — canonical k-mer counting of long reads (Flye's KmerCounter::count) for gfx950 (MI355X).
//
// Semantics (include/gbx.h, kmer section): read r contributes the k-mers at positions 0 .. len - k - 1 (R/kmer.h:185-197:
// the last window is not counted), each as min(code, revcomp(code)) with the first base most significant
// (R/kmer.h:39-63); the count of a k-mer is how often its canonical form occurs.  The result is exact and does not depend
// on the scheduling.
//
// Layout: a direct-address table of 32-bit counters over the code space, 4^k counters, processed in slices of at most
// 2^30 counters (4 GB): one slice for k <= 15, 4 for k = 16, 16 for k = 17.  Per slice:
//   count    every lane takes units of KC_CHUNK consecutive positions of one read (the unit's read by a binary search of
//            the units' prefix sum), reads its bases with aligned 16-byte loads, rolls the forward and reverse codes and
//            issues one no-return atomicAdd of 1 for each canonical k-mer that falls in the slice.  No compare-and-swap.
//   summary  each workgroup sweeps a contiguous range of the slice with 16-byte loads: distinct, >= 16 and largest counts
//            (one atomic per workgroup), the histogram (in LDS, then one add per non-empty bin) and its selected count.
//   select   (only with a selection and an output) a scan of the workgroups' selected counts gives each workgroup's first
//            output slot behind everything earlier slices selected; the workgroup sweeps its range again and writes
//            (k-mer, count) at block-scan offsets, so the output is in ascending canonical code.
// What bounds it: the count pass's scattered 4-byte atomics into HBM (profiles/atomic_peak.json).
//
// Every loop is counted: the unit loop by the unit total, the base loop by (KC_CHUNK + k - 1) / 16 + 2 words, the sweeps
// by the slice size.  Base codes are masked with & 3, so a table index never leaves the slice whatever the input bytes.
//
// The unit size, the sweeps' split and the slice rule are in kmer_split.h, which the plain host compiler takes as well:
// tests/hostcheck/kmer_split_check.cpp holds the tests' boundary cases (tests/kmer_cases.py) against it.
#include <algorithm>
#include "dev_prims.h"
#include "kmer_split.h"

namespace gbx {
namespace {

constexpr int KC_COUNT_BLOCKS = 256 * 8;           // count pass grid: eight workgroups of four wavefronts per CU
constexpr long long KC_TOO_MANY = 1ll << 32;       // n_positions from which nothing is counted (32-bit counters)

struct KmerLayout {
    long long slice_n, n_slices;
    size_t o_blk, o_base, o_table, total;
};

KmerLayout kmer_layout(int k, long long n_reads)
{
    KmerLayout L;
    L.slice_n = kmer_slice_n(k);
    L.n_slices = kmer_n_slices(k);
    L.o_blk = align256((size_t)(n_reads + 1) * 8);                     // unit prefix sum: n_reads + 1 int64
    L.o_base = L.o_blk + align256((size_t)KC_MAX_BLOCKS * 2 * 8);      // per-workgroup selected count and first slot
    L.o_table = L.o_base + 256;                                        // the selection's running total
    L.total = L.o_table + (size_t)L.slice_n * 4 + 64;
    return L;
}

// One workgroup: unit_off[r] = units of reads 0 .. r-1 (KC_CHUNK positions each, max(0, len - k) positions per read),
// unit_off[n_reads] = the total; st->n_positions = the position total.
__global__ void __launch_bounds__(1024) kmer_units_kernel(const int32_t *read_len, long long n_reads, int k, long long *unit_off,
                                                          gbx_kmer_stats *st)
{
    __shared__ long long sh_u[1024], sh_p[1024];
    const int t = threadIdx.x;
    const long long per = (n_reads + 1023) / 1024, r0 = std::min(n_reads, t * per), r1 = std::min(n_reads, r0 + per);
    long long u = 0, p = 0;
    for (long long r = r0; r < r1; ++r) {
        u += kmer_read_units(read_len[r], k);
        p += std::max(0ll, (long long)read_len[r] - k);
    }
    sh_u[t] = u; sh_p[t] = p;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long a = t >= d ? sh_u[t - d] : 0, b = t >= d ? sh_p[t - d] : 0;
        __syncthreads();
        sh_u[t] += a; sh_p[t] += b;
        __syncthreads();
    }
    long long run = sh_u[t] - u;
    for (long long r = r0; r < r1; ++r) {
        unit_off[r] = run;
        run += kmer_read_units(read_len[r], k);
    }
    if (t == 1023) {
        unit_off[n_reads] = sh_u[1023];
        st->n_positions = sh_p[1023];
    }
}

struct CountArgs {
    const uint8_t *enc;
    const int64_t *read_off;
    const int32_t *read_len;
    const long long *unit_off;
    long long n_reads;
    const gbx_kmer_stats *st;
    unsigned *table;
    unsigned long long lo, n_slice;
    int k;
};

__global__ void __launch_bounds__(KC_THREADS) kmer_count_kernel(CountArgs A)
{
    if (A.st->n_positions >= KC_TOO_MANY) return;
    const long long total = A.unit_off[A.n_reads];
    const int k = A.k;
    const unsigned long long mask = (1ull << (2 * k)) - 1;
    const int rs = 2 * (k - 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += stride) {
        // the read of unit u: the largest r with unit_off[r] <= u (reads without units share their offset with the next)
        long long a = 0, b = A.n_reads;            // unit_off[a] <= u < unit_off[b]
        while (b - a > 1) {
            const long long m = (a + b) >> 1;
            if (A.unit_off[m] <= u) a = m; else b = m;
        }
        const long long npos = (long long)A.read_len[a] - k;
        const long long p0 = (u - A.unit_off[a]) * KC_CHUNK;
        const long long n = std::min<long long>(KC_CHUNK, npos - p0);
        // bases p0 .. p0 + n + k - 2 (the k-mers at positions p0 .. p0 + n - 1), read as the aligned 16-byte words that
        // hold them: a word with one byte of the read in it lies inside the allocation's pages
        const uint8_t *first = A.enc + A.read_off[a] + p0, *end = first + n + k - 1;
        const uintptr_t w0 = (uintptr_t)first & ~(uintptr_t)15;
        const int n_words = (int)(((uintptr_t)end - w0 + 15) >> 4);
        unsigned long long fwd = 0, rev = 0;
        int have = 0;
        for (int w = 0; w < n_words; ++w) {
            const uintptr_t wa = w0 + ((uintptr_t)w << 4);
            const uint4 v = *(const uint4 *)wa;
            const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uintptr_t ba = wa + j;
                if (ba < (uintptr_t)first || ba >= (uintptr_t)end) continue;
                const unsigned c = (wv[j >> 2] >> (8 * (j & 3))) & 3u;
                fwd = ((fwd << 2) | c) & mask;
                rev = (rev >> 2) | ((unsigned long long)(3u - c) << rs);
                if (++have >= k) {
                    const unsigned long long key = (fwd < rev ? fwd : rev) - A.lo;
                    if (key < A.n_slice) atomicAdd(&A.table[key], 1u);
                }
            }
        }
    }
}

struct SweepArgs {
    const unsigned *table;
    unsigned long long lo;
    long long n_slice, per;
    int n_hist;
    unsigned min_freq, max_freq;
    gbx_kmer_stats *st;
    int64_t *hist;
    long long *blk_sel, *blk_off;
    uint64_t *sel_kmer;
    uint32_t *sel_count;
    long long sel_cap;
};

__device__ inline bool kmer_selected(unsigned c, unsigned min_freq, unsigned max_freq)
{
    return min_freq != 0 && c >= min_freq && (max_freq == 0 || c <= max_freq);
}

__device__ inline long long wave_sum(long long v)
{
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ void __launch_bounds__(KC_THREADS) kmer_summary_kernel(SweepArgs A)
{
    extern __shared__ unsigned sh_hist[];
    __shared__ long long sh_red[4][KC_THREADS / 64];
    __shared__ unsigned sh_max[KC_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int f = t; f < A.n_hist; f += KC_THREADS) sh_hist[f] = 0;
    __syncthreads();
    const long long b0 = (long long)blockIdx.x * A.per, b1 = std::min(A.n_slice, b0 + A.per);
    long long distinct = 0, ge16 = 0, sel = 0, ones = 0;
    unsigned mx = 0;
    const unsigned top = A.n_hist > 0 ? (unsigned)A.n_hist - 1 : 0;
    for (long long i = b0 + 4 * t; i < b1; i += KC_SWEEP) {
        const uint4 v = *(const uint4 *)(A.table + i);
        const unsigned cs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned c = cs[j];
            if (c == 0) continue;
            ++distinct;
            ge16 += c >= 16;
            mx = c > mx ? c : mx;
            sel += kmer_selected(c, A.min_freq, A.max_freq);
            if (A.n_hist > 0) {
                const unsigned f = c < top ? c : top;
                if (f == 1) ++ones;                  // the crowded bin: counted in a register
                else atomicAdd(&sh_hist[f], 1u);
            }
        }
    }
    distinct = wave_sum(distinct); ge16 = wave_sum(ge16); sel = wave_sum(sel); ones = wave_sum(ones);
    for (int d = 32; d; d >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)mx, d); mx = o > mx ? o : mx; }
    if (lane == 0) { sh_red[0][wv] = distinct; sh_red[1][wv] = ge16; sh_red[2][wv] = sel; sh_red[3][wv] = ones; sh_max[wv] = mx; }
    __syncthreads();
    if (t == 0) {
        long long s[4] = {0, 0, 0, 0};
        unsigned m = 0;
        for (int w = 0; w < KC_THREADS / 64; ++w) {
            for (int q = 0; q < 4; ++q) s[q] += sh_red[q][w];
            m = sh_max[w] > m ? sh_max[w] : m;
        }
        if (s[0]) atomicAdd((unsigned long long *)&A.st->n_distinct, (unsigned long long)s[0]);
        if (s[1]) atomicAdd((unsigned long long *)&A.st->n_ge16, (unsigned long long)s[1]);
        if (m) atomicMax((unsigned long long *)&A.st->max_count, (unsigned long long)m);
        A.blk_sel[blockIdx.x] = s[2];
        if (s[3]) sh_hist[1] += (unsigned)s[3];
    }
    __syncthreads();
    for (int f = t; f < A.n_hist; f += KC_THREADS)
        if (sh_hist[f]) atomicAdd((unsigned long long *)&A.hist[f], (unsigned long long)sh_hist[f]);
}

// One workgroup: blk_off[b] = *base + the selected counts of workgroups 0 .. b-1; *base and st->n_selected += the slice's
// selected total.
__global__ void __launch_bounds__(1024) kmer_sel_scan_kernel(const long long *blk_sel, long long *blk_off, int nb, long long *base,
                                                             gbx_kmer_stats *st)
{
    __shared__ long long sh[1024];
    __shared__ long long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = *base;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + t;
        const long long v = i < nb ? blk_sel[i] : 0;
        sh[t] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const long long u = t >= d ? sh[t - d] : 0;
            __syncthreads();
            sh[t] += u;
            __syncthreads();
        }
        if (i < nb) blk_off[i] = carry + sh[t] - v;
        __syncthreads();
        if (t == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (t == 0) {
        *base = carry;
        st->n_selected = carry;
    }
}

__global__ void __launch_bounds__(KC_THREADS) kmer_select_kernel(SweepArgs A)
{
    __shared__ long long sh_w[KC_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long long b0 = (long long)blockIdx.x * A.per, b1 = std::min(A.n_slice, b0 + A.per);
    long long slot = A.blk_off[blockIdx.x];
    if (A.blk_sel[blockIdx.x] == 0 || slot >= A.sel_cap) return;      // the whole workgroup leaves together
    for (long long r = b0; r < b1; r += KC_SWEEP) {
        const long long i = r + 4 * t;
        unsigned cs[4] = {0, 0, 0, 0};
        if (i < b1) {
            const uint4 v = *(const uint4 *)(A.table + i);
            cs[0] = v.x; cs[1] = v.y; cs[2] = v.z; cs[3] = v.w;
        }
        long long mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) mine += kmer_selected(cs[j], A.min_freq, A.max_freq);
        long long inc = mine;                                         // inclusive scan over the wavefront
        for (int d = 1; d < 64; d <<= 1) { const long long u = __shfl_up(inc, d); if (lane >= d) inc += u; }
        if (lane == 63) sh_w[wv] = inc;
        __syncthreads();
        long long before = 0, all = 0;
        for (int w = 0; w < KC_THREADS / 64; ++w) { before += w < wv ? sh_w[w] : 0; all += sh_w[w]; }
        long long o = slot + before + inc - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (kmer_selected(cs[j], A.min_freq, A.max_freq)) {
                if (o < A.sel_cap) {
                    A.sel_kmer[o] = A.lo + (unsigned long long)(i + j);
                    A.sel_count[o] = cs[j];
                }
                ++o;
            }
        slot += all;
        __syncthreads();
    }
}

__global__ void kmer_finish_kernel(gbx_kmer_stats *st)
{
    if (st->n_positions >= KC_TOO_MANY) { st->n_distinct = -1; st->n_ge16 = -1; st->max_count = -1; st->n_selected = -1; }
}

}  // namespace

size_t kmer_workspace_bytes(int32_t k, int64_t n_reads) { return kmer_layout(k, n_reads).total; }

int kmer_launch(const gbx_kmer_params *p, int64_t n_reads, const uint8_t *d_enc, const int64_t *d_read_off, const int32_t *d_read_len,
                gbx_kmer_stats *d_stats, int64_t *d_hist, uint64_t *d_sel_kmer, uint32_t *d_sel_count, int64_t sel_cap, void *d_work,
                size_t work_bytes, hipStream_t s)
{
    const KmerLayout L = kmer_layout(p->k, n_reads);
    if (work_bytes < L.total) {
        set_error("kmer: workspace of %zu bytes, k = %d and %lld reads need %zu", work_bytes, p->k, (long long)n_reads, L.total);
        return GBX_ERR_ARG;
    }
    char *wb = (char *)d_work;
    long long *unit_off = (long long *)wb, *blk_sel = (long long *)(wb + L.o_blk), *blk_off = blk_sel + KC_MAX_BLOCKS;
    long long *base = (long long *)(wb + L.o_base);
    unsigned *table = (unsigned *)(wb + L.o_table);
    GBX_HIP(hipMemsetAsync(d_stats, 0, sizeof(gbx_kmer_stats), s));
    if (p->n_hist > 0) GBX_HIP(hipMemsetAsync(d_hist, 0, (size_t)p->n_hist * 8, s));
    GBX_HIP(hipMemsetAsync(base, 0, 8, s));
    {
        Stage st("kmer_units", s);
        hipLaunchKernelGGL(kmer_units_kernel, dim3(1), dim3(1024), 0, s, d_read_len, (long long)n_reads, p->k, unit_off, d_stats);
    }
    int nb = 0;
    long long per = 0;
    sweep_split(L.slice_n, &nb, &per);
    const bool select = p->min_freq != 0;
    for (long long sl = 0; sl < L.n_slices; ++sl) {
        const unsigned long long lo = (unsigned long long)(sl * L.slice_n);
        GBX_HIP(hipMemsetAsync(table, 0, (size_t)L.slice_n * 4, s));
        if (n_reads > 0) {
            CountArgs A{d_enc, d_read_off, d_read_len, unit_off, (long long)n_reads, d_stats, table, lo, (unsigned long long)L.slice_n, p->k};
            Stage st("kmer_count", s);
            hipLaunchKernelGGL(kmer_count_kernel, dim3(KC_COUNT_BLOCKS), dim3(KC_THREADS), 0, s, A);
        }
        SweepArgs B{table, lo, L.slice_n, per, p->n_hist, p->min_freq, p->max_freq, d_stats, d_hist, blk_sel, blk_off,
                    d_sel_kmer, d_sel_count, (long long)sel_cap};
        {
            Stage st("kmer_summary", s);
            hipLaunchKernelGGL(kmer_summary_kernel, dim3(nb), dim3(KC_THREADS), (size_t)std::max(p->n_hist, 1) * 4, s, B);
        }
        if (select) {
            Stage st("kmer_select", s);
            hipLaunchKernelGGL(kmer_sel_scan_kernel, dim3(1), dim3(1024), 0, s, (const long long *)blk_sel, blk_off, nb, base, d_stats);
            if (sel_cap > 0) hipLaunchKernelGGL(kmer_select_kernel, dim3(nb), dim3(KC_THREADS), 0, s, B);
        }
    }
    hipLaunchKernelGGL(kmer_finish_kernel, dim3(1), dim3(1), 0, s, d_stats);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
