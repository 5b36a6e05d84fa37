// pileup_kernels.hip — medaka's pileup feature counts (calculate_pileup, R/benchmarks/pileup/medaka_counts.c:298-478) for
// gfx950 (MI355X).
//
// Semantics: include/gbx.h, pileup section.  Two steps over the reads of a region [S, E):
//   prep     one lane per read walks its CIGAR once: the reference position and query position at which every op starts,
//            the indel of the op's last position (htslib's resolve_cigar2 rule: the next op decides) and the read's end.
//            For the layout it also adds +1 / -1 at the ends of the read's span (clipped to the region), takes an atomicMax
//            of every positive indel at its position, counts the aligned bases and records reads without a valid dtype.
//   scan     tiles of 8192 positions: depth = prefix of the +1 / -1 marks, columns = depth > 0 ? 1 + max_ins : 0, pos_col =
//            exclusive prefix of the columns (per-tile sums, one workgroup scans those, the tiles then finish).
//   count    a workgroup owns a window of W consecutive positions and accumulates every counter of the window's columns in
//            LDS, two 16-bit counters a dword (a counter is bounded by the reads that overlap the window, and a window with
//            65 535 of them or more uses 32-bit counters instead), then writes each counter once with coalesced stores.
//            The reads that overlap the window are a contiguous range of the sorted reads: from the first whose prefix
//            maximum of ends passes the window to the first that starts after it (two binary searches).  A task is one
//            read and one 32-position piece of the window; it finds its first op by a binary search over the read's op
//            start positions and walks the ops from there.  A window whose columns do not fit LDS is done in rounds of
//            what fits (a long insertion), each round walking the reads again.
// Counting is additions of 1 into integers, so the result is bit-identical whatever the schedule, the slicing or the
// device count.  What bounds it: DESIGN 3.8 (profiles/pileup_time_large.json).
//
// Every loop is bounded: the op walks by the read's op count, the P-then-I scan by the ops after it, the position walks by
// the op span clipped to the 32-position piece, the binary searches by log2 of their range, the scans by the tile.  In the
// GBX_LOOP_GUARD build the op walks count down from the read's op count as well.  Query positions outside [0, l_seq) and
// unknown ops are skipped on the device; the host entries refuse such reads before uploading them.
#include <algorithm>
#include "dev_prims.h"

namespace gbx {
namespace {

constexpr int PT_THREADS = 1024;                   // scan tiles: 1024 lanes x 8 positions
constexpr int PT_PER = 8;
constexpr int PT_TILE = PT_THREADS * PT_PER;
constexpr int PC_THREADS = 256;                    // count pass
constexpr int PC_LDS_WORDS = 16384;                // 64 KiB of counters per workgroup
constexpr int PC_SUB = 32;                         // positions per task
constexpr int PR_THREADS = 256;                    // prep

enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8 };
__host__ __device__ inline bool op_ref(int op) { return op == OP_M || op == OP_D || op == OP_N || op == OP_EQ || op == OP_X; }
__host__ __device__ inline bool op_query(int op) { return op == OP_M || op == OP_I || op == OP_S || op == OP_EQ || op == OP_X; }

// nt16 (+16 on the reverse strand) -> index in "acgtACGTdD", -1 for IUPAC codes (medaka_counts.h: num2countbase)
__constant__ int8_t c_countbase[32] = {-1, 4, 5, -1, 6, -1, -1, -1, 7, -1, -1, -1, -1, -1, -1, -1,
                                       -1, 0, 1, -1, 2, -1, -1, -1, 3, -1, -1, -1, -1, -1, -1, -1};

struct PlpOp {                                     // per CIGAR op: reference and query position of its start, the indel of its
    int32_t r, q, ind;                             // last position
};

// The workspace: per read and per position arrays first, the per-op array last, so that its offsets do not depend on
// the op count (the device entries cannot read it without a synchronisation).
struct PlpWork {
    size_t o_rend, o_pmax, o_diff, o_maxins, o_tsum, o_csum, o_misc, o_ops;
};

PlpWork plp_work(long long n_reads, long long n_pos)
{
    PlpWork w;
    const long long tiles = (n_pos + PT_TILE - 1) / PT_TILE + 1;
    w.o_rend = 0;
    w.o_pmax = w.o_rend + align256((size_t)n_reads * 4);
    w.o_diff = w.o_pmax + align256((size_t)n_reads * 4);
    w.o_maxins = w.o_diff + align256((size_t)(n_pos + 1) * 4);
    w.o_tsum = w.o_maxins + align256((size_t)(n_pos + 1) * 4);
    w.o_csum = w.o_tsum + align256((size_t)tiles * 8);
    w.o_misc = w.o_csum + align256((size_t)tiles * 8);   // the bad-read word (unsigned long long)
    w.o_ops = w.o_misc + 256;
    return w;
}

struct ReadsDev {
    const int32_t *pos;
    const int64_t *cigar_off;
    const uint32_t *cigar;
    const int64_t *seq_off, *seq_boff;
    const uint8_t *seq, *qual, *rev;
    const int8_t *dtype;
    long long n_reads;
};

ReadsDev reads_dev(const gbx_pileup_reads *d)
{
    return ReadsDev{d->pos, d->cigar_off, d->cigar, d->seq_off, d->seq_boff, d->seq, d->qual, d->rev, d->dtype, (long long)d->n_reads};
}

struct OpArrays {
    PlpOp *ops;
    int32_t *rend, *pmax;
};

__device__ inline int read_dtype(const ReadsDev &R, long long r, int nd)
{
    if (nd <= 1) return 0;
    const int dt = R.dtype ? (int)R.dtype[r] : -1;
    return dt >= 0 && dt < nd ? dt : -1;
}

__global__ void plp_init_kernel(gbx_pileup_layout_stats *st, unsigned long long *bad)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (st) {
            st->n_cols = 0; st->n_positions = 0; st->max_ins = 0; st->max_depth = 0; st->aligned_bases = 0; st->bad_read = -1;
        }
        *bad = ~0ull;
    }
}

// One lane per read: op starts, last-position indels, the read's end; with `layout` the span marks, insertion maxima,
// aligned bases and reads without a dtype.
__global__ void __launch_bounds__(PR_THREADS) plp_prep_kernel(ReadsDev R, OpArrays A, long long S, long long E, int nd, int layout,
                                                              int32_t *diff, int32_t *maxins, gbx_pileup_layout_stats *st,
                                                              unsigned long long *bad)
{
    const long long r = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (r >= R.n_reads) return;
    const long long k0 = R.cigar_off[r], k1 = R.cigar_off[r + 1];
    long long rp = R.pos[r], qp = 0, aligned = 0;
    bool entry_in_region = false;
    GBX_GUARD(gd_ops, k1 - k0);
    for (long long k = k0; k < k1; ++k) {
        if (GBX_GUARD_TRIP(gd_ops, GBX_GK_PILEUP, 1, r)) break;
        const uint32_t w = R.cigar[k];
        const int op = (int)(w & 15u);
        const long long len = (long long)(w >> 4);
        int ind = 0;
        if (k + 1 < k1) {
            const int op2 = (int)(R.cigar[k + 1] & 15u);
            const int l2 = (int)(R.cigar[k + 1] >> 4);
            if (op2 == OP_D && op != OP_D) ind = -l2;
            else if (op2 == OP_I) ind = l2;
            else if (op2 == OP_P && k + 2 < k1) {
                long long l3 = 0;
                GBX_GUARD(gd_pad, k1 - k);
                for (long long kk = k + 2; kk < k1; ++kk) {
                    if (GBX_GUARD_TRIP(gd_pad, GBX_GK_PILEUP, 2, r)) break;
                    const int op3 = (int)(R.cigar[kk] & 15u);
                    if (op3 == OP_I) l3 += (long long)(R.cigar[kk] >> 4);
                    else if (op_ref(op3)) break;
                }
                if (l3 > 0) ind = (int)std::min(l3, (long long)INT32_MAX);
            }
        }
        A.ops[k] = PlpOp{(int32_t)rp, (int32_t)std::min(qp, (long long)INT32_MAX), ind};
        if (op_ref(op)) {
            if (layout && len > 0) {
                const long long last = rp + len - 1;
                if (ind > 0 && last >= S && last < E) atomicMax(&maxins[last - S], ind);
                const long long lo = std::max(rp, S), hi = std::min(rp + len, E);
                if (lo < hi) {
                    if (op != OP_D && op != OP_N) aligned += hi - lo;
                    if (op != OP_N) entry_in_region = true;
                }
            }
            rp += len;
        }
        if (op_query(op)) qp += len;
    }
    const long long re = std::min(rp, (long long)INT32_MAX);
    A.rend[r] = (int32_t)re;
    if (!layout) return;
    const long long lo = std::max((long long)R.pos[r], S), hi = std::min(re, E);
    if (lo < hi) {
        atomicAdd(&diff[lo - S], 1);
        atomicAdd(&diff[hi - S], -1);
    }
    if (aligned) atomicAdd((unsigned long long *)&st->aligned_bases, (unsigned long long)aligned);
    if (entry_in_region && nd > 1 && read_dtype(R, r, nd) < 0) atomicMin(bad, (unsigned long long)r);
}

// pmax[r] = max(rend[0 .. r]): one workgroup, contiguous chunks per lane
__global__ void __launch_bounds__(1024) plp_pmax_kernel(const int32_t *rend, long long n, int32_t *pmax)
{
    __shared__ int32_t sh[1024];
    const int t = threadIdx.x;
    const long long per = (n + 1023) / 1024, r0 = std::min(n, t * per), r1 = std::min(n, r0 + per);
    int32_t m = INT32_MIN;
    for (long long r = r0; r < r1; ++r) m = std::max(m, rend[r]);
    sh[t] = m;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int32_t x = t >= off ? sh[t - off] : INT32_MIN;
        __syncthreads();
        sh[t] = std::max(sh[t], x);
        __syncthreads();
    }
    m = t > 0 ? sh[t - 1] : INT32_MIN;
    for (long long r = r0; r < r1; ++r) { m = std::max(m, rend[r]); pmax[r] = m; }
}

// exclusive scan of v over the workgroup (PT_THREADS lanes); *total = the sum
__device__ long long block_excl_scan(long long v, long long *sh, long long *total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < PT_THREADS; off <<= 1) {
        const long long x = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const long long incl = sh[t];
    *total = sh[PT_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(PT_THREADS) plp_tile_sum_kernel(const int32_t *v, long long n, long long *tsum)
{
    __shared__ long long sh[PT_THREADS];
    const long long i0 = (long long)blockIdx.x * PT_TILE + (long long)threadIdx.x * PT_PER;
    long long s = 0;
    for (int j = 0; j < PT_PER; ++j) if (i0 + j < n) s += v[i0 + j];
    long long tot;
    (void)block_excl_scan(s, sh, &tot);
    if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}

// exclusive scan of n tile sums in place, one workgroup
__global__ void __launch_bounds__(PT_THREADS) plp_scan_tiles_kernel(long long *a, long long n)
{
    __shared__ long long sh[PT_THREADS];
    const int t = threadIdx.x;
    const long long per = (n + PT_THREADS - 1) / PT_THREADS, r0 = std::min(n, t * per), r1 = std::min(n, r0 + per);
    long long s = 0;
    for (long long r = r0; r < r1; ++r) s += a[r];
    long long tot;
    long long run = block_excl_scan(s, sh, &tot);
    for (long long r = r0; r < r1; ++r) { const long long x = a[r]; a[r] = run; run += x; }
}

// depth from the marks, columns per position (written over the marks), the tile's column sum and the statistics
__global__ void __launch_bounds__(PT_THREADS) plp_tile_cols_kernel(int32_t *diff, const int32_t *maxins, long long n, const long long *toff,
                                                                   long long *csum, gbx_pileup_layout_stats *st)
{
    __shared__ long long sh[PT_THREADS];
    __shared__ unsigned long long s_pos;
    __shared__ int s_depth, s_ins;
    if (threadIdx.x == 0) { s_pos = 0; s_depth = 0; s_ins = 0; }
    const long long i0 = (long long)blockIdx.x * PT_TILE + (long long)threadIdx.x * PT_PER;
    int d[PT_PER];
    long long s = 0;
    for (int j = 0; j < PT_PER; ++j) { d[j] = i0 + j < n ? diff[i0 + j] : 0; s += d[j]; }
    long long tot;
    long long depth = block_excl_scan(s, sh, &tot) + toff[blockIdx.x];
    long long cols = 0, npos = 0;
    int dmax = 0, imax = 0;
    for (int j = 0; j < PT_PER; ++j) {
        if (i0 + j >= n) break;
        depth += d[j];
        int c = 0;
        if (depth > 0) {
            const int mi = std::max(maxins[i0 + j], 0);
            c = 1 + mi;
            ++npos;
            imax = std::max(imax, mi);
            dmax = std::max(dmax, (int)std::min(depth, (long long)INT32_MAX));
        }
        diff[i0 + j] = c;
        cols += c;
    }
    if (npos) { atomicAdd(&s_pos, (unsigned long long)npos); atomicMax(&s_depth, dmax); atomicMax(&s_ins, imax); }
    (void)block_excl_scan(cols, sh, &tot);
    if (threadIdx.x == 0) {
        csum[blockIdx.x] = tot;
        if (s_pos) {
            atomicAdd((unsigned long long *)&st->n_positions, s_pos);
            atomicMax((unsigned long long *)&st->max_depth, (unsigned long long)s_depth);
            atomicMax((unsigned long long *)&st->max_ins, (unsigned long long)s_ins);
        }
    }
}

__global__ void __launch_bounds__(PT_THREADS) plp_tile_poscol_kernel(const int32_t *cols, long long n, const long long *coff,
                                                                     int64_t *pos_col, gbx_pileup_layout_stats *st,
                                                                     const unsigned long long *bad)
{
    __shared__ long long sh[PT_THREADS];
    const long long i0 = (long long)blockIdx.x * PT_TILE + (long long)threadIdx.x * PT_PER;
    int c[PT_PER];
    long long s = 0;
    for (int j = 0; j < PT_PER; ++j) { c[j] = i0 + j < n ? cols[i0 + j] : 0; s += c[j]; }
    long long tot;
    long long run = block_excl_scan(s, sh, &tot) + coff[blockIdx.x];
    for (int j = 0; j < PT_PER; ++j) {
        if (i0 + j >= n) break;
        pos_col[i0 + j] = run;
        run += c[j];
        if (i0 + j == n - 1) {
            pos_col[n] = run;
            st->n_cols = run;
            st->bad_read = *bad == ~0ull ? -1 : (int64_t)*bad;
        }
    }
}

struct CountArgs {
    ReadsDev R;
    const PlpOp *ops;
    const int32_t *rend, *pmax;
    const int64_t *pos_col;        // index p - S
    long long S, p0, p1;
    int W, nd, nh, F, vec_ok;
    int32_t *major, *minor;
    uint32_t *counts;
    unsigned long long *bad;
};

__global__ void __launch_bounds__(PC_THREADS) plp_count_kernel(CountArgs a)
{
    __shared__ uint32_t lds[PC_LDS_WORDS];
    const int t = threadIdx.x;
    const long long w0 = a.p0 + (long long)blockIdx.x * a.W, w1 = std::min(w0 + a.W, a.p1);
    if (w0 >= w1) return;
    const long long c_lo = a.pos_col[w0 - a.S], c_hi = a.pos_col[w1 - a.S], col_base = a.pos_col[a.p0 - a.S];
    if (c_lo >= c_hi) return;
    for (long long p = w0 + t; p < w1; p += PC_THREADS) {
        const long long c0 = a.pos_col[p - a.S], c1 = a.pos_col[p + 1 - a.S];
        for (long long c = c0; c < c1; ++c) {
            a.major[c - col_base] = (int32_t)p;
            a.minor[c - col_base] = (int32_t)(c - c0);
        }
    }
    // the reads overlapping [w0, w1): from the first whose prefix maximum of ends passes w0 to the first starting at w1
    long long lo = 0, hi = a.R.n_reads;
    while (lo < hi) { const long long m = (lo + hi) >> 1; if (a.R.pos[m] < w1) lo = m + 1; else hi = m; }
    const long long r_hi = lo;
    lo = 0; hi = r_hi;
    while (lo < hi) { const long long m = (lo + hi) >> 1; if (a.pmax[m] <= w0) lo = m + 1; else hi = m; }
    const long long r_lo = lo, ncand = r_hi - r_lo;
    const bool wide = ncand >= 65535;
    const long long cap_cols = (wide ? PC_LDS_WORDS : 2 * PC_LDS_WORDS) / a.F;
    const int nsub = (int)((w1 - w0 + PC_SUB - 1) / PC_SUB);
    const int F = a.F, nh = a.nh;
    for (long long rc0 = c_lo; rc0 < c_hi; rc0 += cap_cols) {
        const long long rc1 = std::min(rc0 + cap_cols, c_hi);
        const int ncells = (int)((rc1 - rc0) * F);
        const int nwords = wide ? ncells : (ncells + 1) / 2;
        for (int w = t; w < nwords; w += PC_THREADS) lds[w] = 0;
        __syncthreads();
        for (long long task = t; task < ncand * nsub; task += PC_THREADS) {
            const long long r = r_lo + task / nsub;
            const int sub = (int)(task % nsub);
            long long s0 = w0 + (long long)sub * PC_SUB, s1 = std::min(s0 + PC_SUB, w1);
            s0 = std::max(s0, (long long)a.R.pos[r]);
            s1 = std::min(s1, (long long)a.rend[r]);
            if (s0 >= s1) continue;
            const int dt = read_dtype(a.R, r, a.nd);
            const long long k0 = a.R.cigar_off[r], k1 = a.R.cigar_off[r + 1];
            // last op starting at or before s0
            long long blo = k0, bhi = k1;
            while (blo < bhi) { const long long m = (blo + bhi) >> 1; if (a.ops[m].r <= s0) blo = m + 1; else bhi = m; }
            long long k = blo > k0 ? blo - 1 : k0;
            const long long q_base = a.R.seq_off[r], l_seq = a.R.seq_off[r + 1] - q_base;
            const uint8_t *sq = a.R.seq + a.R.seq_boff[r];
            const uint8_t *ql = a.R.qual + q_base;
            const int strand = a.R.rev[r] ? 16 : 0;
            bool skipped = false;
            long long p = s0;
            GBX_GUARD(gd_walk, k1 - k0);
            for (; k < k1 && p < s1; ++k) {
                if (GBX_GUARD_TRIP(gd_walk, GBX_GK_PILEUP, 3, r)) break;
                const uint32_t cw = a.R.cigar[k];
                const int op = (int)(cw & 15u);
                if (!op_ref(op)) continue;
                const PlpOp o = a.ops[k];
                const long long ob = o.r, oe = ob + (long long)(cw >> 4);
                const long long e = std::min(oe, s1);
                for (p = std::max(p, ob); p < e; ++p) {
                    if (op == OP_N) continue;
                    if (dt < 0) { skipped = true; continue; }
                    const long long col0 = a.pos_col[p - a.S];
                    if (op == OP_D) {
                        const long long cell = (col0 - rc0) * F + (long long)dt * nh * 10 + (strand ? 8 : 9);
                        if (col0 >= rc0 && col0 < rc1) {
                            if (wide) atomicAdd(&lds[cell], 1u);
                            else atomicAdd(&lds[cell >> 1], 1u << ((cell & 1) * 16));
                        }
                        continue;
                    }
                    const long long qpos = (long long)o.q + (p - ob);
                    const int ind = p == oe - 1 ? o.ind : 0;
                    const long long jmax = ind > 0 ? ind : 0;
                    // the position's columns col0 .. col0 + jmax: only those inside this round
                    const long long jlo = std::max(0ll, rc0 - col0), jhi = std::min(jmax, rc1 - 1 - col0);
                    for (long long j = jlo; j <= jhi; ++j) {
                        const long long q = qpos + j;
                        if (q < 0 || q >= l_seq) break;
                        const int nib = (sq[q >> 1] >> ((q & 1) ? 0 : 4)) & 15;
                        const int bi = c_countbase[nib + strand];
                        if (bi < 0) continue;
                        int strat = 0;
                        if (nh > 1) strat = std::max(0, std::min((int)ql[q], nh) - 1);
                        const long long cell = (col0 + j - rc0) * F + ((long long)dt * nh + strat) * 10 + bi;
                        if (wide) atomicAdd(&lds[cell], 1u);
                        else atomicAdd(&lds[cell >> 1], 1u << ((cell & 1) * 16));
                    }
                }
            }
            if (skipped) atomicMin(a.bad, (unsigned long long)r);
        }
        __syncthreads();
        uint32_t *out = a.counts + (rc0 - col_base) * F;
        if (wide) {
            for (int w = t; w < ncells; w += PC_THREADS) out[w] = lds[w];
        } else if (a.vec_ok) {
            for (int w = t; w < nwords; w += PC_THREADS) {
                const uint32_t v = lds[w];
                if (2 * w + 1 < ncells) *(uint2 *)(out + 2 * w) = make_uint2(v & 0xffffu, v >> 16);
                else out[2 * w] = v & 0xffffu;
            }
        } else {
            for (int w = t; w < nwords; w += PC_THREADS) {
                const uint32_t v = lds[w];
                out[2 * w] = v & 0xffffu;
                if (2 * w + 1 < ncells) out[2 * w + 1] = v >> 16;
            }
        }
        __syncthreads();
    }
}

OpArrays op_arrays(void *d_work, const PlpWork &W)
{
    char *b = (char *)d_work;
    return OpArrays{(PlpOp *)(b + W.o_ops), (int32_t *)(b + W.o_rend), (int32_t *)(b + W.o_pmax)};
}

int plp_work_check(const gbx_pileup_params *p, const gbx_pileup_reads *d, size_t work_bytes, PlpWork *W, const char *who)
{
    *W = plp_work(d->n_reads, p->end - p->start);
    if (W->o_ops > work_bytes) {
        set_error("%s: a workspace of %zu bytes; gbx_pileup_workspace_bytes asks for at least %zu before the CIGAR ops", who, work_bytes,
                  W->o_ops);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

}  // namespace

size_t pileup_workspace_bytes(int64_t n_reads, int64_t n_cigar, int64_t n_pos)
{
    return plp_work(n_reads, n_pos).o_ops + (size_t)n_cigar * sizeof(PlpOp) + 256;
}

int pileup_layout_launch(const gbx_pileup_params *p, const gbx_pileup_reads *d, int64_t *d_pos_col, gbx_pileup_layout_stats *d_stats,
                         void *d_work, size_t work_bytes, hipStream_t s)
{
    PlpWork W;
    int rc = plp_work_check(p, d, work_bytes, &W, "gbx_pileup_layout_device");
    if (rc) return rc;
    const long long S = p->start, E = p->end, n = E - S;
    char *b = (char *)d_work;
    unsigned long long *bad = (unsigned long long *)(b + W.o_misc);
    int32_t *diff = (int32_t *)(b + W.o_diff), *maxins = (int32_t *)(b + W.o_maxins);
    {
        Stage st_("pileup_init", s);
        plp_init_kernel<<<1, 64, 0, s>>>(d_stats, bad);
        GBX_HIP(hipGetLastError());
    }
    GBX_HIP(hipMemsetAsync(d_pos_col, 0, 8, s));
    if (n == 0) return GBX_OK;
    GBX_HIP(hipMemsetAsync(diff, 0, (size_t)(n + 1) * 4, s));
    GBX_HIP(hipMemsetAsync(maxins, 0, (size_t)(n + 1) * 4, s));
    const ReadsDev R = reads_dev(d);
    if (R.n_reads > 0) {
        Stage st_("pileup_prep", s);
        plp_prep_kernel<<<(unsigned)((R.n_reads + PR_THREADS - 1) / PR_THREADS), PR_THREADS, 0, s>>>(R, op_arrays(d_work, W), S, E, p->num_dtypes, 1,
                                                                                                   diff, maxins, d_stats, bad);
        GBX_HIP(hipGetLastError());
    }
    const long long tiles = (n + PT_TILE - 1) / PT_TILE;
    long long *tsum = (long long *)(b + W.o_tsum), *csum = (long long *)(b + W.o_csum);
    {
        Stage st_("pileup_scan", s);
        plp_tile_sum_kernel<<<(unsigned)tiles, PT_THREADS, 0, s>>>(diff, n, tsum);
        plp_scan_tiles_kernel<<<1, PT_THREADS, 0, s>>>(tsum, tiles);
        plp_tile_cols_kernel<<<(unsigned)tiles, PT_THREADS, 0, s>>>(diff, maxins, n, tsum, csum, d_stats);
        plp_scan_tiles_kernel<<<1, PT_THREADS, 0, s>>>(csum, tiles);
        plp_tile_poscol_kernel<<<(unsigned)tiles, PT_THREADS, 0, s>>>(diff, n, csum, d_pos_col, d_stats, bad);
        GBX_HIP(hipGetLastError());
    }
    GBX_GUARD_CHECK("gbx_pileup_layout");
    return GBX_OK;
}

int pileup_count_launch(const gbx_pileup_params *p, const gbx_pileup_reads *d, const int64_t *d_pos_col, int64_t p0, int64_t p1,
                        int32_t *d_major, int32_t *d_minor, uint32_t *d_counts, void *d_work, size_t work_bytes, hipStream_t s)
{
    PlpWork W;
    int rc = plp_work_check(p, d, work_bytes, &W, "gbx_pileup_count_device");
    if (rc) return rc;
    char *b = (char *)d_work;
    unsigned long long *bad = (unsigned long long *)(b + W.o_misc);
    {
        Stage st_("pileup_init", s);
        plp_init_kernel<<<1, 64, 0, s>>>(nullptr, bad);
        GBX_HIP(hipGetLastError());
    }
    if (p1 <= p0) return GBX_OK;
    const ReadsDev R = reads_dev(d);
    const OpArrays A = op_arrays(d_work, W);
    if (R.n_reads > 0) {                                   // (without reads every column of [p0, p1) is written as zeros)
        Stage st_("pileup_prep", s);
        plp_prep_kernel<<<(unsigned)((R.n_reads + PR_THREADS - 1) / PR_THREADS), PR_THREADS, 0, s>>>(R, A, p->start, p->end, p->num_dtypes, 0,
                                                                                                   nullptr, nullptr, nullptr, bad);
        plp_pmax_kernel<<<1, 1024, 0, s>>>(A.rend, R.n_reads, A.pmax);
        GBX_HIP(hipGetLastError());
    }
    const int F = GBX_PILEUP_FEATLEN * p->num_dtypes * p->num_homop;
    const long long cap16 = 2ll * PC_LDS_WORDS / F;
    const int Wn = (int)std::max<long long>(PC_SUB, std::min<long long>(512, cap16 / 2 / PC_SUB * PC_SUB));
    CountArgs a;
    a.R = R;
    a.ops = A.ops; a.rend = A.rend; a.pmax = A.pmax;
    a.pos_col = d_pos_col;
    a.S = p->start; a.p0 = p0; a.p1 = p1;
    a.W = Wn; a.nd = p->num_dtypes; a.nh = p->num_homop; a.F = F;
    a.major = d_major; a.minor = d_minor; a.counts = d_counts;
    a.vec_ok = ((uintptr_t)d_counts & 7) == 0;
    a.bad = bad;
    const long long nwin = (p1 - p0 + Wn - 1) / Wn;
    {
        Stage st_("pileup_count", s);
        plp_count_kernel<<<(unsigned)nwin, PC_THREADS, 0, s>>>(a);
        GBX_HIP(hipGetLastError());
    }
    GBX_GUARD_CHECK("gbx_pileup_count");
    return GBX_OK;
}

int pileup_read_bad(const gbx_pileup_params *p, const gbx_pileup_reads *d, const void *d_work, int64_t *bad, hipStream_t s)
{
    const PlpWork W = plp_work(d->n_reads, p->end - p->start);
    unsigned long long v = 0;
    GBX_HIP(hipMemcpyAsync(&v, (const char *)d_work + W.o_misc, 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    *bad = v == ~0ull ? -1 : (int64_t)v;
    return GBX_OK;
}

}  // namespace gbx
