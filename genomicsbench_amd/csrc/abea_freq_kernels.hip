// abea_freq_kernels.hip — f5c meth-freq (freq.c) on the device: the per-read methylation calls become one row per genomic site.
// The rules are abea_freq_rules.h, compiled here for the device.
//
// Expand: a thread per record, as count and fill over the shared scan (mem_scan_launch).  A called record makes one item, or in
// split mode one per "CG" of its own bytes (the scan stops one byte before the record's end, so a C that ends one record never
// pairs with the G that begins the next in the arena).  An item is a 128-bit sort item - a = start << 32 | end, b = contig << 32
// | its index - and a 24-byte FreqItem {sequence reference, group size, weight, methylated weight} that stays where it was
// written; the merge makes one item per site of its two tables the same way.
// Sort: the shared stable LSD radix sort (dev_sort.hip) over the bits the caller says are in use: end, start, contig.  Items of a
// key stay in input order, so the first item of a segment is the first the reference's hash table saw.
// Reduce: a head flag per sorted item and its two weights; one scan over (weight, methylated weight) and one over the heads
// turn a segment's sums into the difference of two prefix sums, 64-bit integers, whatever the segment's length and wherever it
// lies among blocks, tiles and wavefronts.  A thread per segment then decides (called_sites > 0, the sum inside int), a scan over
// (kept, sequence bytes) places the rows, and the fill writes each row and copies its head item's sequence into the table's
// own arena.
// Text: a length per line, the scan, a thread per line writes its bytes.
// Every loop is counted from a length in the record, site or name it was handed; the only atomics are integer atomicOr on the
// flag word.  Nothing waits for another block inside a kernel.
#include "dev_prims.h"
#include "abea_freq_rules.h"

namespace gbx {

namespace {

namespace R = abea_freq_rules;
using u32 = uint32_t;
using u64 = unsigned long long;

constexpr int FQ_EL = 256;
constexpr int64_t ARENA_B = 1ll << 62;                        // the item's sequence lies in the second arena (merge)

struct FreqItem { int64_t seq_off; int32_t seq_len, group_size, w, mw; };
static_assert(sizeof(FreqItem) == 24, "FreqItem");

inline unsigned fq_blocks(long long n) { const long long b = (n + FQ_EL - 1) / FQ_EL; return (unsigned)(b > 0 ? b : 1); }

struct FreqLayout { size_t o_bsum; SortLayout sort; size_t o_item, o_wm, o_wm_bsum, o_head, o_head_bsum, o_seg, o_kb, o_kb_bsum, bytes; };

FreqLayout freq_layout(int64_t n_in, int64_t n_items)
{
    FreqLayout L;
    Carver carve;
    const size_t c = (size_t)(n_items > 0 ? n_items : 1);
    const size_t sb = (size_t)mem_scan_blocks(n_items > 0 ? n_items : 0);
    L.o_bsum = carve((size_t)mem_scan_blocks(n_in > 0 ? n_in : 0) * 8);
    L.sort = sort_layout(n_items, carve);
    L.o_item = carve(c * sizeof(FreqItem));
    L.o_wm = carve(2 * (c + 1) * 8); L.o_wm_bsum = carve(2 * sb * 8);
    L.o_head = carve((c + 1) * 8); L.o_head_bsum = carve(sb * 8);
    L.o_seg = carve((c + 1) * 8);
    L.o_kb = carve(2 * (c + 1) * 8); L.o_kb_bsum = carve(2 * sb * 8);
    L.bytes = carve.at;
    return L;
}

__device__ inline void raise(int64_t *counts, int flag) { atomicOr((u64 *)(counts + 4), (u64)flag); }

__global__ void __launch_bounds__(64) freq_init_kernel(int64_t *counts, long long n_items)
{
    if (threadIdx.x < GBX_ABEA_FREQ_NCOUNTS) counts[threadIdx.x] = threadIdx.x == 0 ? n_items : 0;
}

struct ExpandArgs {
    long long n; const gbx_abea_freq_record *rec; const char *arena; double thr; int split, pos_bits, contig_bits;
    long long n_items; long long *item_off; uint64_t *ka, *kb; FreqItem *items; int64_t *counts;
};

__device__ inline void put_item(const ExpandArgs &A, long long at, int32_t contig, int32_t start, int32_t end, const FreqItem &it)
{
    if (contig < 0 || ((u32)contig >> A.contig_bits) || ((u32)start >> A.pos_bits) || ((u32)end >> A.pos_bits)) raise(A.counts, GBX_ABEA_FREQ_KEY_BITS);
    A.ka[at] = ((uint64_t)(u32)start << 32) | (u32)end;
    A.kb[at] = ((uint64_t)(u32)contig << 32) | (u32)at;
    A.items[at] = it;
}

template <bool FILL>
__global__ void __launch_bounds__(FQ_EL) freq_expand_kernel(ExpandArgs A)
{
    const long long r = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (FILL && r == 0 && A.item_off[A.n] != A.n_items) raise(A.counts, GBX_ABEA_FREQ_ITEMS);
    if (r >= A.n) return;
    const gbx_abea_freq_record c = A.rec[r];
    const bool call = R::called(c.llr, A.thr), sp = R::splits(A.split, c.n_cpg);
    const char *const seq = A.arena + c.seq_off;
    const long long len = c.seq_len;
    if (!FILL) {
        long long cnt = 0;
        if (call && !sp) cnt = 1;
        else if (call)
            for (long long i = 0; i + 1 < len; ++i) cnt += R::cg_at(seq, len, i) ? 1 : 0;
        A.item_off[r] = cnt;
        return;
    }
    if (!call) return;
    long long at = A.item_off[r];
    const long long end = A.item_off[r + 1];
    if (at < 0 || end < at || end > A.n_items) { raise(A.counts, GBX_ABEA_FREQ_ITEMS); return; }
    const int32_t mw = R::methylated(c.llr) ? 1 : 0;
    if (!sp) {
        if (end - at != 1) { raise(A.counts, GBX_ABEA_FREQ_ITEMS); return; }
        put_item(A, at, c.contig, c.start, c.end, FreqItem{c.seq_off, c.seq_len < 0 ? 0 : c.seq_len, c.n_cpg, c.n_cpg, mw ? c.n_cpg : 0});
        return;
    }
    long long first = -1;
    for (long long i = 0; i + 1 < len && at < end; ++i) {
        if (!R::cg_at(seq, len, i)) continue;
        if (first < 0) first = i;
        long long pos = (long long)c.start + i - first;
        if (pos > 0x7fffffffLL) { raise(A.counts, GBX_ABEA_FREQ_POS_OVERFLOW); pos = 0x7fffffffLL; }
        put_item(A, at++, c.contig, (int32_t)pos, (int32_t)pos, FreqItem{0, -1, 1, 1, mw});
    }
    if (at != end) raise(A.counts, GBX_ABEA_FREQ_ITEMS);
}

// the merge: site i of table A, then of table B, is item i
__global__ void __launch_bounds__(FQ_EL) freq_table_items_kernel(long long n_a, const gbx_abea_freq_site *sa, long long n_b, const gbx_abea_freq_site *sb,
                                                                 int pos_bits, int contig_bits, uint64_t *ka, uint64_t *kb, FreqItem *items, int64_t *counts)
{
    const long long i = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (i >= n_a + n_b) return;
    const bool second = i >= n_a;
    const gbx_abea_freq_site S = second ? sb[i - n_a] : sa[i];
    if (S.contig < 0 || ((u32)S.contig >> contig_bits) || ((u32)S.start >> pos_bits) || ((u32)S.end >> pos_bits)) raise(counts, GBX_ABEA_FREQ_KEY_BITS);
    ka[i] = ((uint64_t)(u32)S.start << 32) | (u32)S.end;
    kb[i] = ((uint64_t)(u32)S.contig << 32) | (u32)i;
    const bool lit = S.seq_len < 0;
    items[i] = FreqItem{lit ? 0 : (S.seq_off | (second ? ARENA_B : 0)), lit ? -1 : S.seq_len, S.group_size, S.called_sites, S.called_sites_methylated};
}

struct ReduceArgs {
    long long n;                                             // items
    const uint64_t *ka, *kb; const FreqItem *items;
    long long *wm, *head, *seg, *kept;                       // wm: [2][n + 1]; head, seg: [n + 1]; kept: [2][n + 1] (rows, bytes)
    int64_t *counts;
    const char *arena_a, *arena_b;
    long long site_cap; gbx_abea_freq_site *sites; long long seq_cap; char *seq_arena;
};

// the item a sorted slot names; a slot nothing wrote (GBX_ABEA_FREQ_ITEMS is up then) counts as an item of no weight
__device__ inline FreqItem item_of(const ReduceArgs &A, long long i)
{
    const u32 idx = (u32)A.kb[i];
    return idx < A.n ? A.items[idx] : FreqItem{0, 0, 0, 0, 0};
}

__device__ inline bool is_head(const ReduceArgs &A, long long i)
{
    return i == 0 || A.ka[i] != A.ka[i - 1] || (A.kb[i] >> 32) != (A.kb[i - 1] >> 32);
}

__global__ void __launch_bounds__(FQ_EL) freq_weights_kernel(ReduceArgs A)
{
    const long long i = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (i >= A.n) return;
    const FreqItem it = item_of(A, i);
    A.wm[i] = it.w;
    A.wm[A.n + 1 + i] = it.mw;
    A.head[i] = is_head(A, i) ? 1 : 0;
}

// head has become the segment index of every head; entry n the number of segments
__global__ void __launch_bounds__(FQ_EL) freq_segments_kernel(ReduceArgs A)
{
    const long long i = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (i >= A.n) return;
    if (is_head(A, i)) A.seg[A.head[i]] = i;
    if (i == 0) A.seg[A.head[A.n]] = A.n;
}

__global__ void __launch_bounds__(FQ_EL) freq_decide_kernel(ReduceArgs A)
{
    const long long s = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (s >= A.n) return;
    long long keep = 0, bytes = 0;
    if (s < A.head[A.n]) {
        const long long lo = A.seg[s], hi = A.seg[s + 1];
        const long long called = A.wm[hi] - A.wm[lo], meth = A.wm[A.n + 1 + hi] - A.wm[A.n + 1 + lo];
        if (called > 0x7fffffffLL || meth > 0x7fffffffLL) raise(A.counts, GBX_ABEA_FREQ_SUM_OVERFLOW);
        else if (called > 0) {
            const FreqItem it = item_of(A, lo);
            keep = 1;
            bytes = it.seq_len > 0 ? it.seq_len : 0;
        }
    }
    A.kept[s] = keep;
    A.kept[A.n + 1 + s] = bytes;
}

__global__ void __launch_bounds__(FQ_EL) freq_fill_kernel(ReduceArgs A)
{
    const long long s = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (s >= A.n || s >= A.head[A.n] || (A.counts[4] & GBX_ABEA_FREQ_ITEMS)) return;      // (items nothing wrote: no sequence reference is followed)
    const long long row = A.kept[s];
    if (A.kept[s + 1] == row || row >= A.site_cap) return;
    const long long lo = A.seg[s], hi = A.seg[s + 1];
    const FreqItem it = item_of(A, lo);
    const long long boff = A.kept[A.n + 1 + s];
    gbx_abea_freq_site S;
    S.contig = (int32_t)(A.kb[lo] >> 32); S.start = (int32_t)(A.ka[lo] >> 32); S.end = (int32_t)(u32)A.ka[lo];
    S.group_size = it.group_size;
    S.called_sites = (int32_t)(A.wm[hi] - A.wm[lo]);
    S.called_sites_methylated = (int32_t)(A.wm[A.n + 1 + hi] - A.wm[A.n + 1 + lo]);
    S.seq_off = it.seq_len < 0 ? 0 : boff;
    S.seq_len = it.seq_len; S.pad_ = 0;
    A.sites[row] = S;
    if (it.seq_len > 0 && boff + it.seq_len <= A.seq_cap) {
        const char *src = ((it.seq_off & ARENA_B) ? A.arena_b : A.arena_a) + (it.seq_off & ~ARENA_B);
        for (int32_t k = 0; k < it.seq_len; ++k) A.seq_arena[boff + k] = src[k];
    }
}

// ---- call-methylation's sites -> records
struct RecordsArgs {
    long long n; const gbx_abea_meth_site *sites; const float *scores; long long n_reads; const int32_t *contig; const int64_t *ref_off;
    const int32_t *ref_len; const char *ref; int32_t clip_start, clip_end; long long *off;
    long long rec_cap; gbx_abea_freq_record *rec; long long seq_cap; char *arena;
};

template <bool FILL>
__global__ void __launch_bounds__(FQ_EL) freq_records_kernel(RecordsArgs A)
{
    const long long s = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (s >= A.n) return;
    const gbx_abea_meth_site S = A.sites[s];
    const bool read_ok = S.read >= 0 && S.read < A.n_reads;
    const bool keep = read_ok && !((A.clip_start != -1 && S.start_position < A.clip_start) || (A.clip_end != -1 && S.end_position >= A.clip_end));
    const bool ctx_ok = read_ok && S.ctx_len > 0 && S.ctx_off >= 0 && S.ctx_off + S.ctx_len <= A.ref_len[S.read];
    const int32_t len = keep && ctx_ok ? S.ctx_len : 0;
    if (!FILL) { A.off[s] = keep ? 1 : 0; A.off[A.n + 1 + s] = len; return; }
    if (!keep) return;
    const long long at = A.off[s], boff = A.off[A.n + 1 + s];
    if (at >= A.rec_cap) return;
    gbx_abea_freq_record r;
    r.contig = A.contig[S.read]; r.start = S.start_position; r.end = S.end_position; r.n_cpg = S.n_cpg;
    r.llr = R::llr_as_printed((double)A.scores[2 * s + 1] - (double)A.scores[2 * s]);
    r.seq_off = boff; r.seq_len = len; r.pad_ = 0;
    A.rec[at] = r;
    if (len > 0 && boff + len <= A.seq_cap) {
        const char *src = A.ref + A.ref_off[S.read] + S.ctx_off;
        for (int32_t k = 0; k < len; ++k) A.arena[boff + k] = R::site_byte(src[k]);
    }
}

// ---- text
#define FREQ_HEADER(what) "chromosome\tstart\tend\tnum_" what "_in_group\tcalled_sites\tcalled_sites_methylated\tmethylated_frequency\tgroup_sequence\n"
__host__ __device__ inline const char *freq_header(int kind) { return kind == GBX_ABEA_FREQ_MOTIFS ? FREQ_HEADER("motifs") : FREQ_HEADER("cpgs"); }

struct TsvArgs {
    long long n; const gbx_abea_freq_site *sites; const char *arena; long long n_contigs; const int64_t *name_off; const char *names;
    int kind; long long header_len; long long *line_off; long long cap; char *out;
};

__device__ inline long long name_len_of(const TsvArgs &A, int32_t c) { return c >= 0 && c < A.n_contigs ? A.name_off[c + 1] - A.name_off[c] : 0; }

// line_off[0]: the header's bytes, line_off[s + 1]: site s's
__global__ void __launch_bounds__(FQ_EL) freq_tsv_len_kernel(TsvArgs A)
{
    const long long s = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (s == 0) A.line_off[0] = A.header_len;
    if (s >= A.n) return;
    const gbx_abea_freq_site S = A.sites[s];
    const long long nl = name_len_of(A, S.contig);
    A.line_off[s + 1] = (nl > 0 ? nl : 0) + R::line_tail_len(S.start, S.end, S.group_size, S.called_sites, S.called_sites_methylated, S.seq_len);
}

__global__ void __launch_bounds__(FQ_EL) freq_tsv_fill_kernel(TsvArgs A)
{
    const long long s = (long long)blockIdx.x * FQ_EL + threadIdx.x;
    if (s == 0 && A.header_len > 0 && A.line_off[1] <= A.cap) {
        const char *h = freq_header(A.kind);
        for (long long k = 0; k < A.header_len; ++k) A.out[k] = h[k];
    }
    if (s >= A.n || A.line_off[s + 2] > A.cap) return;
    const gbx_abea_freq_site S = A.sites[s];
    char *o = A.out + A.line_off[s + 1];
    const long long nl = name_len_of(A, S.contig);
    if (nl > 0) {
        const char *nm = A.names + A.name_off[S.contig];
        for (long long k = 0; k < nl; ++k) o[k] = nm[k];
        o += nl;
    }
    *o++ = '\t'; o += R::dec_put(o, S.start);
    *o++ = '\t'; o += R::dec_put(o, S.end);
    *o++ = '\t'; o += R::dec_put(o, S.group_size);
    *o++ = '\t'; o += R::dec_put(o, S.called_sites);
    *o++ = '\t'; o += R::dec_put(o, S.called_sites_methylated);
    *o++ = '\t';
    R::freq_put(o, S.called_sites > 0 ? R::freq_milli(S.called_sites_methylated, S.called_sites) : 0);
    o += R::FREQ_LEN;
    *o++ = '\t';
    if (S.seq_len < 0) {
        const char *lit = "split-group";
        for (int k = 0; k < R::SPLIT_LEN; ++k) o[k] = lit[k];
        o += R::SPLIT_LEN;
    } else {
        const char *src = A.arena + S.seq_off;
        for (int32_t k = 0; k < S.seq_len; ++k) o[k] = src[k];
        o += S.seq_len;
    }
    *o = '\n';
}

void scan2(long long *cnt, long long n, long long *bsum, int64_t *total0, int64_t *total1, hipStream_t s)
{
    MemScanJob J{};
    J.cnt = cnt; J.n = n; J.nq = 2; J.bsum = bsum; J.blocks = mem_scan_blocks(n);
    J.total[0] = total0; J.total[1] = total1;
    mem_scan_launch(J, s);
}

// FILL after a REDUCE of an earlier call: the sorted items lie in the buffer the pass count says
ReduceArgs reduce_args(const FreqLayout &L, char *wb, long long n, int pos_bits, int contig_bits, int64_t *counts)
{
    const int n_pass = 2 * ((pos_bits + 7) / 8) + (contig_bits + 7) / 8;
    SortBufs<uint64_t> B = sort_bufs(wb, L.sort);
    const int cur = n_pass & 1;
    ReduceArgs A{};
    A.n = n; A.ka = B.a[cur]; A.kb = B.b[cur]; A.items = (const FreqItem *)(wb + L.o_item);
    A.wm = (long long *)(wb + L.o_wm); A.head = (long long *)(wb + L.o_head); A.seg = (long long *)(wb + L.o_seg); A.kept = (long long *)(wb + L.o_kb);
    A.counts = counts;
    return A;
}

// the items stand in buffer 0 of the sort: sort, segments, sums, sizes
int freq_reduce(const FreqLayout &L, char *wb, long long n, int pos_bits, int contig_bits, int64_t *counts, hipStream_t s)
{
    SortBufs<uint64_t> B = sort_bufs(wb, L.sort);
    SortPass pass[12];
    int n_pass = 0;
    const auto digit = [](int bits, int b) { return (uint32_t)((1u << (bits - b < 8 ? bits - b : 8)) - 1); };
    for (int b = 0; b < pos_bits; b += 8) pass[n_pass++] = SortPass{0, b, digit(pos_bits, b)};
    for (int b = 0; b < pos_bits; b += 8) pass[n_pass++] = SortPass{0, 32 + b, digit(pos_bits, b)};
    for (int b = 0; b < contig_bits; b += 8) pass[n_pass++] = SortPass{1, 32 + b, digit(contig_bits, b)};
    {
        Stage st("abea_freq_sort", s);
        radix_sort(B, SortCount{nullptr, n}, pass, n_pass, s);       // -> buffer n_pass & 1, where reduce_args looks
    }
    GBX_HIP(hipGetLastError());
    const ReduceArgs A = reduce_args(L, wb, n, pos_bits, contig_bits, counts);
    {
        Stage st("abea_freq_reduce", s);
        hipLaunchKernelGGL(freq_weights_kernel, dim3(fq_blocks(n)), dim3(FQ_EL), 0, s, A);
        scan2(A.wm, n, (long long *)(wb + L.o_wm_bsum), nullptr, nullptr, s);
        scan_launch1(A.head, n, (long long *)(wb + L.o_head_bsum), counts + 1, MemScanGuard{}, s);
        hipLaunchKernelGGL(freq_segments_kernel, dim3(fq_blocks(n)), dim3(FQ_EL), 0, s, A);
        hipLaunchKernelGGL(freq_decide_kernel, dim3(fq_blocks(n)), dim3(FQ_EL), 0, s, A);
        scan2(A.kept, n, (long long *)(wb + L.o_kb_bsum), counts + 2, counts + 3, s);
    }
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

int freq_fill(ReduceArgs A, const char *arena_a, const char *arena_b, int64_t site_cap, gbx_abea_freq_site *sites, int64_t seq_cap, char *seq_arena, hipStream_t s)
{
    A.arena_a = arena_a; A.arena_b = arena_b; A.site_cap = site_cap; A.sites = sites; A.seq_cap = seq_cap; A.seq_arena = seq_arena;
    Stage st("abea_freq_fill", s);
    hipLaunchKernelGGL(freq_fill_kernel, dim3(fq_blocks(A.n)), dim3(FQ_EL), 0, s, A);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace

size_t abea_freq_work_bytes(int64_t n_in, int64_t n_items) { return freq_layout(n_in, n_items).bytes; }

int abea_freq_launch(int pass, int64_t n_records, const gbx_abea_freq_record *d_records, const char *d_rec_arena, double threshold, int split_groups,
                     int pos_bits, int contig_bits, int64_t n_items, void *d_work, int64_t *d_item_off, int64_t *d_counts, int64_t site_cap,
                     gbx_abea_freq_site *d_sites, int64_t seq_cap, char *d_seq_arena, hipStream_t s)
{
    if (n_records > 0x7fffffffLL - 1024 || n_items > 0x7fffffffLL - 1024) { set_error("abea freq: more than 2^31 records or items in one call"); return GBX_ERR_UNSUPPORTED; }
    char *const wb = (char *)d_work;
    const FreqLayout L = freq_layout(n_records, n_items);
    ExpandArgs E{(long long)n_records, d_records, d_rec_arena, threshold, split_groups, pos_bits, contig_bits, (long long)n_items, (long long *)d_item_off,
                 nullptr, nullptr, nullptr, d_counts};
    if (pass & GBX_ABEA_FREQ_COUNT) {
        Stage st("abea_freq_count", s);
        if (n_records > 0) hipLaunchKernelGGL(freq_expand_kernel<false>, dim3(fq_blocks(n_records)), dim3(FQ_EL), 0, s, E);
        scan_launch1((long long *)d_item_off, n_records, (long long *)(wb + L.o_bsum), d_counts, MemScanGuard{}, s);
        GBX_HIP(hipGetLastError());
    }
    if (pass & GBX_ABEA_FREQ_REDUCE) {
        hipLaunchKernelGGL(freq_init_kernel, dim3(1), dim3(64), 0, s, d_counts, (long long)n_items);
        GBX_HIP(hipGetLastError());
        const SortBufs<uint64_t> B = sort_bufs(wb, L.sort);
        E.ka = B.a[0]; E.kb = B.b[0]; E.items = (FreqItem *)(wb + L.o_item);
        {
            Stage st("abea_freq_expand", s);
            hipLaunchKernelGGL(freq_expand_kernel<true>, dim3(fq_blocks(n_records)), dim3(FQ_EL), 0, s, E);
        }
        GBX_HIP(hipGetLastError());
        if (n_items > 0)
            if (int rc = freq_reduce(L, wb, n_items, pos_bits, contig_bits, d_counts, s)) return rc;
    }
    if ((pass & GBX_ABEA_FREQ_FILL) && n_items > 0)
        return freq_fill(reduce_args(L, wb, n_items, pos_bits, contig_bits, d_counts), d_rec_arena, d_rec_arena, site_cap, d_sites, seq_cap, d_seq_arena, s);
    return GBX_OK;
}

int abea_freq_merge_launch(int pass, int64_t n_a, const gbx_abea_freq_site *d_sites_a, const char *d_arena_a, int64_t n_b, const gbx_abea_freq_site *d_sites_b,
                           const char *d_arena_b, int pos_bits, int contig_bits, void *d_work, int64_t *d_counts, int64_t site_cap,
                           gbx_abea_freq_site *d_sites, int64_t seq_cap, char *d_seq_arena, hipStream_t s)
{
    const int64_t n = n_a + n_b;
    if (n > 0x7fffffffLL - 1024) { set_error("abea freq merge: more than 2^31 sites in one call"); return GBX_ERR_UNSUPPORTED; }
    char *const wb = (char *)d_work;
    const FreqLayout L = freq_layout(n, n);
    if (pass & GBX_ABEA_FREQ_REDUCE) {
        hipLaunchKernelGGL(freq_init_kernel, dim3(1), dim3(64), 0, s, d_counts, (long long)n);
        GBX_HIP(hipGetLastError());
        if (n > 0) {
            const SortBufs<uint64_t> B = sort_bufs(wb, L.sort);
            {
                Stage st("abea_freq_table_items", s);
                hipLaunchKernelGGL(freq_table_items_kernel, dim3(fq_blocks(n)), dim3(FQ_EL), 0, s, (long long)n_a, d_sites_a, (long long)n_b, d_sites_b, pos_bits,
                                   contig_bits, B.a[0], B.b[0], (FreqItem *)(wb + L.o_item), d_counts);
            }
            GBX_HIP(hipGetLastError());
            if (int rc = freq_reduce(L, wb, n, pos_bits, contig_bits, d_counts, s)) return rc;
        }
    }
    if ((pass & GBX_ABEA_FREQ_FILL) && n > 0)
        return freq_fill(reduce_args(L, wb, n, pos_bits, contig_bits, d_counts), d_arena_a, d_arena_b, site_cap, d_sites, seq_cap, d_seq_arena, s);
    return GBX_OK;
}

size_t abea_freq_records_work_bytes(int64_t n_sites) { return align256(2 * (size_t)mem_scan_blocks(n_sites > 0 ? n_sites : 0) * 8); }

int abea_freq_records_launch(int pass, int64_t n_sites, const gbx_abea_meth_site *d_sites, const float *d_scores, int64_t n_reads, const int32_t *d_contig,
                             const int64_t *d_ref_off, const int32_t *d_ref_len, const char *d_ref, int32_t clip_start, int32_t clip_end, void *d_work,
                             int64_t *d_off, int64_t rec_cap, gbx_abea_freq_record *d_records, int64_t seq_cap, char *d_seq_arena, hipStream_t s)
{
    if (n_sites > 0x7fffffffLL - 1024) { set_error("abea freq records: more than 2^31 sites in one call"); return GBX_ERR_UNSUPPORTED; }
    const RecordsArgs A{(long long)n_sites, d_sites, d_scores, (long long)n_reads, d_contig, d_ref_off, d_ref_len, d_ref, clip_start, clip_end, (long long *)d_off,
                        (long long)rec_cap, d_records, (long long)seq_cap, d_seq_arena};
    if (pass & GBX_ABEA_FREQ_COUNT) {
        Stage st("abea_freq_records_count", s);
        if (n_sites > 0) hipLaunchKernelGGL(freq_records_kernel<false>, dim3(fq_blocks(n_sites)), dim3(FQ_EL), 0, s, A);
        scan2((long long *)d_off, n_sites, (long long *)d_work, nullptr, nullptr, s);
        GBX_HIP(hipGetLastError());
    }
    if ((pass & GBX_ABEA_FREQ_FILL) && n_sites > 0) {
        Stage st("abea_freq_records_fill", s);
        hipLaunchKernelGGL(freq_records_kernel<true>, dim3(fq_blocks(n_sites)), dim3(FQ_EL), 0, s, A);
        GBX_HIP(hipGetLastError());
    }
    return GBX_OK;
}

size_t abea_freq_tsv_work_bytes(int64_t n_sites) { return align256((size_t)mem_scan_blocks((n_sites > 0 ? n_sites : 0) + 1) * 8); }

int abea_freq_tsv_launch(int pass, int64_t n_sites, const gbx_abea_freq_site *d_sites, const char *d_seq_arena, int64_t n_contigs, const int64_t *d_name_off,
                         const char *d_names, int header_kind, int with_header, void *d_work, int64_t *d_line_off, int64_t cap, char *d_out, hipStream_t s)
{
    if (n_sites > 0x7fffffffLL - 1024) { set_error("abea freq tsv: more than 2^31 sites in one call"); return GBX_ERR_UNSUPPORTED; }
    const long long header_len = with_header ? (long long)strlen(freq_header(header_kind)) : 0;
    const TsvArgs A{(long long)n_sites, d_sites, d_seq_arena, (long long)n_contigs, d_name_off, d_names, header_kind, header_len, (long long *)d_line_off,
                    (long long)cap, d_out};
    if (pass & GBX_ABEA_FREQ_COUNT) {
        Stage st("abea_freq_tsv_count", s);
        hipLaunchKernelGGL(freq_tsv_len_kernel, dim3(fq_blocks(n_sites)), dim3(FQ_EL), 0, s, A);
        scan_launch1((long long *)d_line_off, n_sites + 1, (long long *)d_work, nullptr, MemScanGuard{}, s);
        GBX_HIP(hipGetLastError());
    }
    if (pass & GBX_ABEA_FREQ_FILL) {
        Stage st("abea_freq_tsv_fill", s);
        hipLaunchKernelGGL(freq_tsv_fill_kernel, dim3(fq_blocks(n_sites)), dim3(FQ_EL), 0, s, A);
        GBX_HIP(hipGetLastError());
    }
    return GBX_OK;
}

}  // namespace gbx
