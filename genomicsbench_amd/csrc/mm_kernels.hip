// mm_kernels.hip — minimap2's seeding stage in front of chain: the minimizer sketch, the minimizer index and seed
// collection with the occurrence filter.  The rules are minimap2's (mm_sketch, mm_idx_*, collect_matches / collect_seed_hits),
// restated in tests/mm_ref.py; the machine itself is in mm_machine.h, shared with a host build.
//
//   sketch   a lane takes one piece of GBX_MM_SKETCH_CHUNK bases of the concatenated text (the stretches of every sequence that
//            fall in it), warm-started w + k steps ahead; a count pass, the shared scan (mem_scan_launch), a fill pass.  The ring
//            of w slots and the HPC queue are per lane, lane-interleaved: in LDS up to w = 16 (sized by w), in the workspace above.  Even k:
//            a lane takes a whole sequence.
//   sort     LSD radix sort of 128-bit items (hi, lo) on a list of 8-bit digits: radix_sort of dev_sort.hip with the element
//            count read on the device, the grid covering the capacity.  Stable, so equal keys keep their order.
//   index    sketch (rid = ordinal) -> sort on the digits of x >> 8 (the values keep their ascending y) -> head flags, scan ->
//            sorted distinct keys + CSR; the keys' counts are sorted for mid_occ.  Lookup: binary search over the keys.
//   seeding  sketch (rid 0) -> lookup (read, key range, count per minimizer) -> scan -> per-read record (one wavefront a read)
//            -> fill -> sort on the significant digits of (read, x, y) -> unpack.
// No kernel here waits for another block, and no entry synchronises with the host.
#include "dev_prims.h"
#include "mm_machine.h"

namespace gbx {
namespace {

using u32 = unsigned;
using u64 = uint64_t;

constexpr int LDS_W = 16;                                        // the widest ring kept in LDS
constexpr int READ_SHIFT = 43;                                   // the read's place in an anchor's sort word
constexpr u64 Y_MASK = (1ull << READ_SHIFT) - 1;

inline int bits_of(long long v) { int b = 0; while (v > 0) { ++b; v >>= 1; } return b; }

// ------------------------------------------------------------------------------------------------ sketch
struct SketchJob {
    const uint8_t *seq; const int64_t *off; long long n_seqs, n_units;
    int w, k, hpc, whole, rid_ordinal;
    long long *cnt;                                  // [n_units + 1]: the units' counts, then their offsets
    u64 *mx, *my; long long cap; int64_t *mini_off;
    u64 *gring;                                      // w > LDS_W: 64 (2 w + MM_TQ / 2) words a block
};

struct LaneRing {                                    // lane-interleaved: element j of a lane is 64 entries behind element j - 1
    u64 *bx, *by; int *bq;
    __device__ u64 &x(int j) { return bx[j * 64]; }
    __device__ u64 &y(int j) { return by[j * 64]; }
    __device__ int &q(int j) { return bq[j * 64]; }
};

template <bool FILL>
struct Emit {
    u64 *mx, *my; long long at, cap;
    __device__ void operator()(u64 x, u64 y)
    {
        if (FILL && at < cap) { mx[at] = x; my[at] = y; }
        ++at;
    }
};

template <bool LDS, bool FILL>
__global__ void __launch_bounds__(64) mm_sketch_kernel(SketchJob J)
{
    extern __shared__ u64 lds_ring[];                 // LDS: 64 (2 w) words, and 64 MM_TQ ints behind them under HPC (sketch_lds_bytes)
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= J.n_units) return;
    LaneRing ring;
    if (LDS) { ring.bx = lds_ring + threadIdx.x; ring.by = lds_ring + 64 * J.w + threadIdx.x; ring.bq = (int *)(lds_ring + 128 * J.w) + threadIdx.x; }
    else {
        u64 *const base = J.gring + (long long)blockIdx.x * 64 * (2 * J.w + MM_TQ / 2);
        ring.bx = base + threadIdx.x; ring.by = base + 64 * J.w + threadIdx.x;
        ring.bq = (int *)(base + 128 * J.w) + threadIdx.x;
    }
    Emit<FILL> emit{J.mx, J.my, FILL ? J.cnt[g] : 0, J.cap};
    auto piece = [&](long long s, long long lo, long long hi) {
        const long long o = J.off[s], len = J.off[s + 1] - o;
        mm_sketch_piece(J.seq + o, len, J.w, J.k, J.rid_ordinal ? (uint32_t)s : 0u, J.hpc != 0, lo, hi, ring, emit);
    };
    if (J.whole) {
        if (FILL) J.mini_off[g] = emit.at;
        if (J.off[g + 1] > J.off[g]) piece(g, 0, J.off[g + 1] - J.off[g]);
    } else {
        const long long lo_g = g * MM_CHUNK, hi_g = lo_g + MM_CHUNK;
        long long a = 0, b = J.n_seqs;                                       // the first sequence that starts at or behind lo_g
        while (a < b) { const long long m = (a + b) >> 1; if (J.off[m] < lo_g) a = m + 1; else b = m; }
        long long s = a;
        if (s > 0 && J.off[s] > lo_g) {                                      // the sequence before it reaches into this piece
            const long long o = J.off[s - 1], e = J.off[s] < hi_g ? J.off[s] : hi_g;
            piece(s - 1, lo_g - o, e - o);
        }
        for (; s < J.n_seqs && J.off[s] < hi_g; ++s) {
            if (FILL) J.mini_off[s] = emit.at;
            const long long o = J.off[s], e = J.off[s + 1] < hi_g ? J.off[s + 1] : hi_g;
            if (e > o) piece(s, 0, e - o);
        }
    }
    if (!FILL) J.cnt[g] = emit.at;
    else if (g == 0) J.mini_off[J.n_seqs] = J.cnt[J.n_units];
}

// the LDS of a block whose ring fits there: the queue only where it is used, so that w = 10 without HPC takes 10 KB and not 24
inline unsigned sketch_lds_bytes(const gbx_mm_params *p) { return p->w <= LDS_W ? 64u * (16u * (unsigned)p->w + (p->is_hpc ? 4u * MM_TQ : 0u)) : 0u; }

struct SketchLayout { size_t o_cnt, o_bsum, o_ring, total; long long n_units, blocks; };

SketchLayout sketch_layout(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len)
{
    SketchLayout L;
    L.n_units = (p->k & 1) ? total_len / MM_CHUNK + 1 : (n_seqs > 0 ? n_seqs : 1);
    L.blocks = (L.n_units + 63) / 64;
    Carver take;
    L.o_cnt = take((size_t)(L.n_units + 1) * 8);
    L.o_bsum = take((size_t)mem_scan_blocks(L.n_units) * 8);
    L.o_ring = take(p->w > LDS_W ? (size_t)L.blocks * 64 * (2 * (size_t)p->w + MM_TQ / 2) * 8 : 0);
    L.total = take.at;
    return L;
}

// ------------------------------------------------------------------------------------------------ index
struct IndexJob {
    MmIndexView v; long long cap;
    const u64 *hi, *lo;                              // the sorted minimizers
    long long *cnt;                                  // [cap + 1] head flags, then ranks
    u64 *chi;                                        // the keys' counts, to be sorted
    float frac; int mid_occ, k, w, hpc;
};

__global__ void __launch_bounds__(MM_EL) mm_idx_head_kernel(IndexJob J)
{
    const long long i = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (i >= J.cap) return;
    const long long m = clip_count(J.v.hdr, J.cap);
    J.cnt[i] = i < m && (i == 0 || J.hi[i] >> 8 != J.hi[i - 1] >> 8) ? 1 : 0;
}

// cnt has become the ranks of the heads; cnt[cap] = hdr[1] = the number of keys
__global__ void __launch_bounds__(MM_EL) mm_idx_write_kernel(IndexJob J)
{
    const long long i = (long long)blockIdx.x * MM_EL + threadIdx.x;
    const long long m = clip_count(J.v.hdr, J.cap);
    if (i == 0) J.v.koff[J.cnt[J.cap]] = m;
    if (i >= m) return;
    J.v.vals[i] = J.lo[i];
    if (i == 0 || J.hi[i] >> 8 != J.hi[i - 1] >> 8) { const long long r = J.cnt[i]; J.v.keys[r] = J.hi[i] >> 8; J.v.koff[r] = i; }
}

__global__ void __launch_bounds__(MM_EL) mm_idx_count_kernel(IndexJob J)
{
    const long long j = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (j < clip_count(J.v.hdr + 1, J.cap)) J.chi[j] = (u64)(J.v.koff[j + 1] - J.v.koff[j]);
}

// hi: the counts in ascending order
__global__ void mm_idx_mid_occ_kernel(IndexJob J)
{
    const long long N = clip_count(J.v.hdr + 1, J.cap);
    long long mo = 0x7fffffffll;
    if (J.mid_occ > 0) mo = J.mid_occ;
    else if (J.frac > 0.f && N > 0) {
        long long rank = (long long)(u32)((1. - (double)J.frac) * (double)N);
        if (rank >= N) rank = N - 1;
        const long long c = (long long)J.hi[rank] + 1;
        mo = c < mo ? c : mo;
    }
    J.v.hdr[2] = mo; J.v.hdr[3] = J.k; J.v.hdr[4] = J.w; J.v.hdr[5] = J.hpc;
}

struct IndexLayout { size_t o_sketch, o_moff, o_cnt, o_bsum, total; SortLayout sort; };

IndexLayout index_layout(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len, int64_t cap)
{
    IndexLayout L;
    Carver take;
    L.o_sketch = take(sketch_layout(p, n_seqs, total_len).total);
    L.o_moff = take((size_t)(n_seqs + 1) * 8);
    L.sort = sort_layout(cap, take);
    L.o_cnt = take((size_t)(cap + 2) * 8);
    L.o_bsum = take((size_t)mem_scan_blocks(cap > 0 ? cap : 1) * 8);
    L.total = take.at;
    return L;
}

// ------------------------------------------------------------------------------------------------ seeding
struct SeedJob {
    MmIndexView v; long long idx_cap;
    const uint8_t *seq; const int64_t *seq_off; long long n_reads;
    const u64 *mx, *my; long long mini_cap; const int64_t *mini_off;
    int32_t *mread; long long *kst; int32_t *mt;     // per minimizer: its read, where its key's values start, the key's count
    long long *acnt;                                 // [mini_cap + 1]: anchors per minimizer, then their offsets
    u64 *hi, *lo; long long anchor_cap;              // the fill's target (sort buffer 0)
    int64_t *off; gbx_chain_call *hdr; int32_t *rep_len, *n_mini; const int64_t *counts;
    u64 *ax, *ay;
    int max_gap, bw;
};

__global__ void __launch_bounds__(MM_EL) mm_seed_lookup_kernel(SeedJob J)
{
    const long long j = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (j >= J.mini_cap) return;
    const long long n = clip_count(J.counts, J.mini_cap);
    if (j >= n) { J.acnt[j] = 0; return; }
    long long a = 0, b = J.n_reads;                                          // the last read whose minimizers start at or before j
    while (a < b) { const long long m = (a + b + 1) >> 1; if (J.mini_off[m] <= j) a = m; else b = m - 1; }
    if (a >= J.n_reads) a = J.n_reads - 1;
    J.mread[j] = (int32_t)a;
    const u64 key = J.mx[j] >> 8;
    const long long nk = clip_count(J.v.hdr + 1, J.idx_cap);
    long long lo = 0, hi = nk;
    while (lo < hi) { const long long m = (lo + hi) >> 1; if (J.v.keys[m] < key) lo = m + 1; else hi = m; }
    long long t = 0, st = 0;
    if (lo < nk && J.v.keys[lo] == key) { st = J.v.koff[lo]; t = J.v.koff[lo + 1] - st; }
    J.kst[j] = st;
    J.mt[j] = (int32_t)(t < 0x7fffffffll ? t : 0x7fffffffll);
    J.acnt[j] = t < J.v.hdr[2] ? t : 0;
}

// one wavefront a read: off, n_mini, rep_len and the call's header
__global__ void __launch_bounds__(64) mm_seed_read_kernel(SeedJob J)
{
    const long long r = blockIdx.x;
    const int lane = threadIdx.x;
    const long long clip0 = J.mini_off[r] < J.mini_cap ? J.mini_off[r] : J.mini_cap;
    const long long clip1 = J.mini_off[r + 1] < J.mini_cap ? J.mini_off[r + 1] : J.mini_cap;
    const long long n_all = clip_count(J.counts, J.mini_cap);
    const long long m0 = clip0 < n_all ? clip0 : n_all, m1 = clip1 < n_all ? clip1 : n_all;
    const long long mid_occ = J.v.hdr[2];
    long long sum_span = 0;
    int rep_st = 0, rep_en = 0, rep = 0;
    for (long long b0 = m0; b0 < m1; b0 += 64) {
        const long long j = b0 + lane;
        bool is_rep = false;
        int st = 0, en = 0;
        if (j < m1) {
            const int span = (int)(J.mx[j] & 0xff);
            sum_span += (J.acnt[j + 1] - J.acnt[j]) * span;
            is_rep = J.mt[j] >= mid_occ;
            en = (int)((u32)J.my[j] >> 1) + 1;
            st = en - span;
        }
        u64 bal = __ballot(is_rep);
        while (bal) {                                                        // the repetitive ones in order, every lane alike
            const int b = __builtin_ctzll(bal);
            bal &= bal - 1;
            const int s_ = __shfl(st, b), e_ = __shfl(en, b);
            if (s_ > rep_en) { rep += rep_en - rep_st; rep_st = s_; rep_en = e_; }
            else rep_en = e_;
        }
    }
    rep += rep_en - rep_st;
    for (int d = 32; d > 0; d >>= 1) sum_span += __shfl_xor(sum_span, d);
    if (lane != 0) return;
    const long long a0 = J.acnt[m0], n = J.acnt[m1] - a0;
    J.off[r] = a0;
    if (r == J.n_reads - 1) J.off[J.n_reads] = J.acnt[m1];
    J.n_mini[r] = (int32_t)(J.mini_off[r + 1] - J.mini_off[r]);
    J.rep_len[r] = rep;
    gbx_chain_call h;
    h.avg_qspan = n > 0 ? (float)sum_span / (float)n : 0.f;
    h.max_dist_x = h.max_dist_y = J.max_gap; h.bw = J.bw; h.n_segs = 1;
    J.hdr[r] = h;
}

__global__ void __launch_bounds__(MM_EL) mm_seed_fill_kernel(SeedJob J)
{
    const long long j = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (j >= clip_count(J.counts, J.mini_cap)) return;
    const long long a0 = J.acnt[j], cnt = J.acnt[j + 1] - a0;
    if (cnt <= 0) return;
    const long long r = J.mread[j];
    const u64 x = J.mx[j], y = J.my[j], key = x >> 8;
    const u64 q_span = x & 0xff, q_pos = (u32)y;
    const u64 qlen = (u64)(J.seq_off[r + 1] - J.seq_off[r]);
    const long long m_lo = J.mini_off[r], m_hi = J.mini_off[r + 1] < J.mini_cap ? J.mini_off[r + 1] : J.mini_cap;
    const bool tandem = (j > m_lo && J.mx[j - 1] >> 8 == key) || (j + 1 < m_hi && J.mx[j + 1] >> 8 == key);
    const u64 y_fwd = q_span << 32 | q_pos >> 1, y_rev = q_span << 32 | (u64)(u32)(qlen - ((q_pos >> 1) + 1 - q_span) - 1);
    const u64 tag = (u64)r << READ_SHIFT | (tandem ? GBX_MM_SEED_TANDEM : 0);
    const long long st = J.kst[j];
    for (long long v = 0; v < cnt; ++v) {
        const long long dst = a0 + v;
        if (dst >= J.anchor_cap) break;
        const u64 rv = J.v.vals[st + v];
        const u64 rpos = (u32)rv >> 1;
        const bool same = ((rv ^ q_pos) & 1) == 0;
        J.hi[dst] = (same ? 0 : 1ull << 63) | (rv & 0xffffffff00000000ull) | rpos;
        J.lo[dst] = tag | (same ? y_fwd : y_rev);
    }
}

__global__ void __launch_bounds__(MM_EL) mm_seed_unpack_kernel(const u64 *hi, const u64 *lo, const int64_t *d_m, long long cap, u64 *ax, u64 *ay)
{
    const long long i = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (i >= clip_count(d_m, cap)) return;
    ax[i] = hi[i]; ay[i] = lo[i] & Y_MASK;
}

struct SeedLayout { size_t o_sketch, o_mread, o_kst, o_mt, o_acnt, o_bsum, total; SortLayout sort; };

SeedLayout seed_layout(const gbx_mm_params *p, int64_t n_reads, int64_t total_len, int64_t mini_cap, int64_t anchor_cap)
{
    SeedLayout L;
    Carver take;
    const size_t mc = (size_t)(mini_cap > 0 ? mini_cap : 1);
    L.o_sketch = take(sketch_layout(p, n_reads, total_len).total);
    L.o_mread = take(mc * 4);
    L.o_kst = take(mc * 8);
    L.o_mt = take(mc * 4);
    L.o_acnt = take((mc + 1) * 8);
    L.o_bsum = take((size_t)mem_scan_blocks((long long)mc) * 8);
    L.sort = sort_layout(anchor_cap, take);
    L.total = take.at;
    return L;
}

}  // namespace

MmIndexView mm_index_view(void *d_index, int64_t mini_cap)
{
    char *b = (char *)d_index;
    const size_t c = (size_t)(mini_cap > 0 ? mini_cap : 1);
    MmIndexView v;
    v.hdr = (int64_t *)b; b += 256;
    v.keys = (uint64_t *)b; b += align256(c * 8);
    v.koff = (int64_t *)b; b += align256((c + 1) * 8);
    v.vals = (uint64_t *)b;
    return v;
}

size_t mm_index_bytes(int64_t mini_cap)
{
    const size_t c = (size_t)(mini_cap > 0 ? mini_cap : 1);
    return 256 + align256(c * 8) + align256((c + 1) * 8) + align256(c * 8);
}

size_t mm_sketch_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len) { return sketch_layout(p, n_seqs, total_len).total; }

int mm_sketch_launch(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len, int rid_ordinal,
                     uint64_t *d_mx, uint64_t *d_my, int64_t mini_cap, int64_t *d_mini_off, int64_t *d_n_mini, void *d_work, size_t work_bytes,
                     hipStream_t s)
{
    const SketchLayout L = sketch_layout(p, n_seqs, total_len);
    if (work_bytes < L.total) { set_error("mm sketch: workspace too small (%zu bytes, %zu needed)", work_bytes, L.total); return GBX_ERR_ARG; }
    if (L.blocks >= (1ll << 31)) { set_error("mm sketch: too many pieces"); return GBX_ERR_UNSUPPORTED; }
    char *wb = (char *)d_work;
    SketchJob J;
    J.seq = d_seq; J.off = d_seq_off; J.n_seqs = n_seqs; J.n_units = n_seqs > 0 ? L.n_units : 0;
    J.w = p->w; J.k = p->k; J.hpc = p->is_hpc; J.whole = (p->k & 1) ? 0 : 1; J.rid_ordinal = rid_ordinal;
    J.cnt = (long long *)(wb + L.o_cnt); J.mx = (u64 *)d_mx; J.my = (u64 *)d_my; J.cap = mini_cap; J.mini_off = d_mini_off;
    J.gring = (u64 *)(wb + L.o_ring);
    const bool lds = p->w <= LDS_W;
    const dim3 grid((unsigned)L.blocks), block(64);
    if (n_seqs == 0) GBX_HIP(hipMemsetAsync(d_mini_off, 0, 8, s));
    {
        Stage st("mm_sketch_count", s);
        if (lds) hipLaunchKernelGGL((mm_sketch_kernel<true, false>), grid, block, sketch_lds_bytes(p), s, J);
        else hipLaunchKernelGGL((mm_sketch_kernel<false, false>), grid, block, 0, s, J);
    }
    {
        Stage st("mm_sketch_scan", s);
        scan_launch1(J.cnt, J.n_units, (long long *)(wb + L.o_bsum), d_n_mini, MemScanGuard{}, s);
    }
    {
        Stage st("mm_sketch_fill", s);
        if (lds) hipLaunchKernelGGL((mm_sketch_kernel<true, true>), grid, block, sketch_lds_bytes(p), s, J);
        else hipLaunchKernelGGL((mm_sketch_kernel<false, true>), grid, block, 0, s, J);
    }
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

size_t mm_index_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len, int64_t mini_cap)
{
    return index_layout(p, n_seqs, total_len, mini_cap).total;
}

int mm_index_launch(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len, void *d_index,
                    int64_t mini_cap, void *d_work, size_t work_bytes, hipStream_t s)
{
    const IndexLayout L = index_layout(p, n_seqs, total_len, mini_cap);
    if (work_bytes < L.total) { set_error("mm index: workspace too small (%zu bytes, %zu needed)", work_bytes, L.total); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    const SortBufs<u64> B = sort_bufs(wb, L.sort);
    IndexJob J;
    J.v = mm_index_view(d_index, mini_cap); J.cap = mini_cap > 0 ? mini_cap : 1;
    J.cnt = (long long *)(wb + L.o_cnt);
    J.frac = p->mid_occ_frac; J.mid_occ = p->mid_occ; J.k = p->k; J.w = p->w; J.hpc = p->is_hpc;
    // the minimizers land in sort buffer 0; their offsets per sequence are not kept
    int rc = mm_sketch_launch(p, n_seqs, d_seq, d_seq_off, total_len, 1, B.a[0], B.b[0], mini_cap, (int64_t *)(wb + L.o_moff), J.v.hdr, wb + L.o_sketch,
                              sketch_layout(p, n_seqs, total_len).total, s);
    if (rc) return rc;
    SortPass pass[8];
    int np = 0;
    for (int sh = 8; sh < 8 + 2 * p->k; sh += 8) pass[np++] = SortPass{0, sh, 255u};
    int cur;
    {
        Stage st("mm_index_sort", s);
        cur = radix_sort(B, SortCount{J.v.hdr, J.cap}, pass, np, s);
    }
    J.hi = B.a[cur]; J.lo = B.b[cur]; J.chi = B.a[cur ^ 1];
    {
        Stage st("mm_index_group", s);
        hipLaunchKernelGGL(mm_idx_head_kernel, dim3(mm_el_blocks(J.cap)), dim3(MM_EL), 0, s, J);
        scan_launch1(J.cnt, J.cap, (long long *)(wb + L.o_bsum), J.v.hdr + 1, MemScanGuard{}, s);
        hipLaunchKernelGGL(mm_idx_write_kernel, dim3(mm_el_blocks(J.cap)), dim3(MM_EL), 0, s, J);
        hipLaunchKernelGGL(mm_idx_count_kernel, dim3(mm_el_blocks(J.cap)), dim3(MM_EL), 0, s, J);
    }
    {
        Stage st("mm_index_mid_occ", s);
        // the counts sit in the buffer the sorted minimizers do not use; the sort starts from buffer 0
        SortBufs<u64> C = B;
        if (cur == 0) { std::swap(C.a[0], C.a[1]); std::swap(C.b[0], C.b[1]); }
        np = 0;
        for (int sh = 0; sh < bits_of(J.cap) && sh < 32; sh += 8) pass[np++] = SortPass{0, sh, 255u};
        const int c2 = radix_sort(C, SortCount{J.v.hdr + 1, J.cap}, pass, np, s);
        J.hi = C.a[c2];
        hipLaunchKernelGGL(mm_idx_mid_occ_kernel, dim3(1), dim3(1), 0, s, J);
    }
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

size_t mm_seed_workspace_bytes(const gbx_mm_params *p, int64_t n_reads, int64_t total_len, int64_t mini_cap, int64_t anchor_cap)
{
    return seed_layout(p, n_reads, total_len, mini_cap, anchor_cap).total;
}

int mm_seed_launch(const gbx_mm_params *p, const MmSeedIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    const SeedLayout L = seed_layout(p, io.n_reads, io.total_len, io.mini_cap, io.anchor_cap);
    if (work_bytes < L.total) { set_error("mm seed: workspace too small (%zu bytes, %zu needed)", work_bytes, L.total); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    if (io.n_reads == 0) {
        GBX_HIP(hipMemsetAsync(io.off, 0, 8, s));
        GBX_HIP(hipMemsetAsync(io.mini_off, 0, 8, s));
        GBX_HIP(hipMemsetAsync(io.counts, 0, 16, s));
        return GBX_OK;
    }
    int rc = mm_sketch_launch(p, io.n_reads, io.seq, io.seq_off, io.total_len, 0, io.mini_x, io.mini_y, io.mini_cap, io.mini_off, io.counts,
                              wb + L.o_sketch, sketch_layout(p, io.n_reads, io.total_len).total, s);
    if (rc) return rc;
    const SortBufs<u64> B = sort_bufs(wb, L.sort);
    const long long sort_cap = io.anchor_cap > 0 ? io.anchor_cap : 1;
    SeedJob J;
    J.v = mm_index_view(const_cast<void *>(io.index), io.index_mini_cap); J.idx_cap = io.index_mini_cap > 0 ? io.index_mini_cap : 1;
    J.seq = io.seq; J.seq_off = io.seq_off; J.n_reads = io.n_reads;
    J.mx = (const u64 *)io.mini_x; J.my = (const u64 *)io.mini_y; J.mini_cap = io.mini_cap; J.mini_off = io.mini_off;
    J.mread = (int32_t *)(wb + L.o_mread); J.kst = (long long *)(wb + L.o_kst); J.mt = (int32_t *)(wb + L.o_mt);
    J.acnt = (long long *)(wb + L.o_acnt);
    J.hi = B.a[0]; J.lo = B.b[0]; J.anchor_cap = io.anchor_cap;
    J.off = io.off; J.hdr = io.hdr; J.rep_len = io.rep_len; J.n_mini = io.n_mini; J.counts = io.counts;
    J.ax = (u64 *)io.ax; J.ay = (u64 *)io.ay; J.max_gap = p->max_gap; J.bw = p->bw;
    {
        Stage st("mm_seed_lookup", s);
        if (io.mini_cap > 0) hipLaunchKernelGGL(mm_seed_lookup_kernel, dim3(mm_el_blocks(io.mini_cap)), dim3(MM_EL), 0, s, J);
        else GBX_HIP(hipMemsetAsync(J.acnt, 0, 16, s));
        scan_launch1(J.acnt, io.mini_cap, (long long *)(wb + L.o_bsum), io.counts + 1, MemScanGuard{io.counts, 0, io.mini_cap}, s);
        hipLaunchKernelGGL(mm_seed_read_kernel, dim3((unsigned)io.n_reads), dim3(64), 0, s, J);
    }
    {
        Stage st("mm_seed_fill", s);
        if (io.mini_cap > 0) hipLaunchKernelGGL(mm_seed_fill_kernel, dim3(mm_el_blocks(io.mini_cap)), dim3(MM_EL), 0, s, J);
    }
    SortPass pass[24];
    int np = 0;
    for (int sh = 0; sh < bits_of(io.total_len) && sh < 32; sh += 8) pass[np++] = SortPass{1, sh, 255u};          // y: the query position,
    pass[np++] = SortPass{1, 32, 255u};                                                                           // the span,
    pass[np++] = SortPass{1, 42, 1u};                                                                             // the tandem flag
    for (int sh = 0; sh < bits_of(io.ref_max_len) && sh < 32; sh += 8) pass[np++] = SortPass{0, sh, 255u};        // x: the reference position,
    for (int sh = 32; sh < 32 + bits_of(io.ref_n_seqs) && sh < 56; sh += 8) pass[np++] = SortPass{0, sh, 255u};   // the sequence,
    pass[np++] = SortPass{0, 56, 255u};                                                                           // its top bits and the strand
    for (int sh = READ_SHIFT; sh < READ_SHIFT + bits_of(io.n_reads - 1); sh += 8) pass[np++] = SortPass{1, sh, 255u};      // the read
    {
        Stage st("mm_seed_sort", s);
        const int cur = radix_sort(B, SortCount{io.counts + 1, sort_cap}, pass, np, s);
        hipLaunchKernelGGL(mm_seed_unpack_kernel, dim3(mm_el_blocks(sort_cap)), dim3(MM_EL), 0, s, B.a[cur], B.b[cur], io.counts + 1, (long long)io.anchor_cap,
                           J.ax, J.ay);
    }
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
