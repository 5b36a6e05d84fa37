// abea_meth_plan_kernels.hip — the middle of call-methylation on the device: the site planner (calculate_methylation_for_read,
// meth.c:500-658) behind the event-alignment record, and the order and checks of the jobs it emits in front of the score kernel.
// The rules are abea_meth_rules.h, compiled here for the device.
//
// Planner: a wavefront per read walks the reference segment 64 bases a trip.  A ballot gives the trip's CpG mask; mask arithmetic
// gives every CpG its predecessor, hence the group starts; the lane of a group start closes the group before it (the one carried
// in from earlier trips, or the one the previous start of this trip opened) and decides it on the spot: the skips and the two
// lower bounds over the read's record.  A closed group never leaves the registers, so the planner needs no candidate list: the
// count pass adds up the kept groups and their string bytes, the fill pass walks again, ranks the kept groups of a trip with a
// ballot and an in-wavefront scan, and the whole wavefront writes each kept site's 4 L string bytes with consecutive stores.
// Between the two, the shared exclusive scan (mem_scan_launch) turns the per-read counts into offsets.  Every loop is counted
// from ref_len, the kept groups of a trip (at most 64) or L; the lower bounds carry the 32-step bound; no wavefront waits for
// another; the only atomic is the order stage's atomicMin.
//
// Order: a key per job, (class, max_rows - rows), the shared stable radix sort (dev_sort.hip) with as many 8-bit passes as the key
// has bits, and class_off from the class boundaries of the sorted keys (a class's count is the distance between two of them).
#include "dev_prims.h"
#include "abea_meth_rules.h"

namespace gbx {

namespace {

namespace R = abea_meth_rules;
using u32 = uint32_t;
using u64 = unsigned long long;

constexpr int ORDER_EL = 256;

__device__ inline int top_bit(u64 m) { return 63 - __clzll((long long)m); }              // m != 0

struct SitesArgs {
    long long n_reads;
    const int64_t *ref_off; const int32_t *ref_len; const char *ref; const int32_t *ref_start_pos; const uint8_t *rc;
    const int64_t *rec_off; const gbx_abea_pair *rec;
    int64_t *site_off, *byte_off; uint8_t *bad;
    long long site_cap; gbx_abea_meth_site *sites; gbx_abea_meth_job *jobs; long long seq_cap; char *seq_arena;
};

// what a wavefront carries from trip to trip, the same in every lane
struct Walk {
    long long n_kept, n_bytes;                               // of the groups closed so far
    int any_bad;
    // fill: where the read's sites and bytes go and how many there are
    long long site0, n_site, byte0, byte1;
};

// `active` lanes hold a closed group each, in ascending lane order
template <bool FILL>
__device__ inline void close_groups(const SitesArgs &A, Walk &w, long long r, const char *ref, long long len, int32_t rsp, bool rev,
                                    const gbx_abea_pair *rp, int n_rec, bool active, const R::Group &g, int lane)
{
    R::Kept k{0, 0, 0, 0};
    int d = R::GROUP_SKIP;
    if (active) d = R::group_decide(g, len, rsp, rev, rp, n_rec, &k);
    const u64 km = __ballot(d == R::GROUP_KEEP);
    if (__ballot(d == R::GROUP_AGAINST_STRAND)) w.any_bad = 1;
    if (km == 0) return;
    const long long mine = d == R::GROUP_KEEP ? 4ll * k.L : 0;
    const long long incl = wave_scan_incl(mine, lane);
    const long long total = __shfl(incl, 63);
    if (FILL) {
        const u64 below = (1ull << lane) - 1;
        const long long excl = incl - mine, rank = w.n_kept + __builtin_popcountll(km & below);
        const long long at = w.byte0 + w.n_bytes + excl;
        const bool fits = rank < w.n_site && at + mine <= w.byte1;                        // (a fill always agrees with its count)
        if (d == R::GROUP_KEEP && fits) {
            A.sites[w.site0 + rank] = R::site_of((int32_t)r, g, len, rsp);
            A.jobs[2 * (w.site0 + rank)] = R::job_of((int32_t)r, k, rev, at, 0);
            A.jobs[2 * (w.site0 + rank) + 1] = R::job_of((int32_t)r, k, rev, at, 1);
        }
        // the strings of each kept group of this trip, the whole wavefront on one group at a time
        u64 m = km;
        for (int it = 0; it < 64 && m; ++it) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int ss = __shfl(k.sub_start, src), L = __shfl(k.L, src);
            const long long o = __shfl(at, src);
            if (!__shfl((int)fits, src)) continue;
            for (int t = lane; t < 4 * L; t += 64) {
                const int which = t / L;
                A.seq_arena[o + t] = R::site_byte(ref, ss, L, which, t - which * L);
            }
        }
    }
    w.n_kept += __builtin_popcountll(km);
    w.n_bytes += total;
}

template <bool FILL>
__global__ void __launch_bounds__(64) abea_meth_sites_kernel(SitesArgs A)
{
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    if (r >= A.n_reads) return;
    const long long len = A.ref_len[r], n_rec_ll = A.rec_off[r + 1] - A.rec_off[r];
    Walk w{0, 0, 0, 0, 0, 0, 0};
    if (FILL) {
        w.site0 = A.site_off[r]; w.n_site = A.site_off[r + 1] - w.site0; w.byte0 = A.byte_off[r]; w.byte1 = A.byte_off[r + 1];
        // nothing to write, or a read whose sites or strings would end past the room: left unwritten
        if (w.n_site <= 0 || w.site0 < 0 || w.byte0 < 0 || w.byte1 < w.byte0 || w.site0 + w.n_site > A.site_cap || w.byte1 > A.seq_cap) return;
    }
    if (len >= 2 && n_rec_ll > 0) {                                                       // (else: an empty record bounds nothing)
        const char *ref = A.ref + A.ref_off[r];
        const gbx_abea_pair *rp = A.rec + A.rec_off[r];
        const int n_rec = (int)(n_rec_ll < 0x7fffffffLL ? n_rec_ll : 0x7fffffffLL);
        const int32_t rsp = A.ref_start_pos[r];
        const bool rev = A.rc[r] != 0;
        const u64 below = (1ull << lane) - 1;
        bool open = false;                                                                // the group the walk is inside
        int c_first = 0, c_last = 0, c_n = 0;
        for (long long b = 0; b + 1 < len; b += 64) {
            const long long pos = b + lane;
            const bool cpg = R::cpg_at(ref, len, pos);
            const u64 mask = __ballot(cpg), mb = mask & below;
            const bool has_prev = mb != 0 || open;
            const int prev = mb ? (int)b + top_bit(mb) : c_last;
            const bool st = cpg && R::group_starts(has_prev, prev, (int)pos);
            const u64 S = __ballot(st), sb = S & below;
            // a start closes the group before it
            const bool closes = st && (sb != 0 || open);
            R::Group g{0, 0, 0};
            if (closes) {
                if (sb) { const int ps = top_bit(sb); g.first = (int)b + ps; g.last = prev; g.n_cpg = __builtin_popcountll(mb >> ps); }
                else { g.first = c_first; g.last = prev; g.n_cpg = c_n + __builtin_popcountll(mb); }
            }
            close_groups<FILL>(A, w, r, ref, len, rsp, rev, rp, n_rec, closes, g, lane);
            if (S) { const int hs = top_bit(S); c_first = (int)b + hs; c_n = __builtin_popcountll(mask >> hs); c_last = (int)b + top_bit(mask); open = true; }
            else if (mask) { c_last = (int)b + top_bit(mask); c_n += __builtin_popcountll(mask); }
        }
        const R::Group last{c_first, c_last, c_n};
        close_groups<FILL>(A, w, r, ref, len, rsp, rev, rp, n_rec, open && lane == 0, last, lane);
    }
    if (!FILL && lane == 0) { A.site_off[r] = w.n_kept; A.byte_off[r] = w.n_bytes; A.bad[r] = (uint8_t)w.any_bad; }
}

// ---- order
__global__ void __launch_bounds__(64) abea_meth_order_init_kernel(int64_t *class_off, int64_t *first_bad)
{
    if (threadIdx.x <= GBX_ABEA_METH_NCLASS) class_off[threadIdx.x] = 0;
    if (threadIdx.x == 0) *first_bad = INT64_MAX;
}

__global__ void __launch_bounds__(ORDER_EL) abea_meth_order_key_kernel(long long n_jobs, const gbx_abea_meth_job *__restrict__ jobs, long long seq_bytes,
                                                                      long long n_reads, const int64_t *__restrict__ event_off, long long flank_len,
                                                                      int bits, uint64_t *__restrict__ key, u32 *__restrict__ val, int64_t *first_bad)
{
    const long long j = (long long)blockIdx.x * ORDER_EL + threadIdx.x;
    if (j >= n_jobs) return;
    const gbx_abea_meth_job J = jobs[j];
    if (R::job_check(J, seq_bytes, n_reads, event_off, flank_len) != R::JOB_OK) atomicMin((u64 *)first_bad, (u64)j);
    const long long max_rows = (1ll << bits) - 1;
    long long rows = R::job_rows(J);
    rows = rows < 1 ? 1 : rows > max_rows ? max_rows : rows;                               // (a job out of range is a bad job: no score follows)
    key[j] = ((uint64_t)R::job_class((int64_t)J.seq_len - GBX_ABEA_KMER + 1) << bits) | (uint64_t)(max_rows - rows);
    val[j] = (u32)j;
}

// the sorted payloads are the order; class c starts where the first key of a class >= c stands
__global__ void __launch_bounds__(ORDER_EL) abea_meth_order_out_kernel(long long n_jobs, const uint64_t *__restrict__ key, const u32 *__restrict__ val, int bits,
                                                                      int32_t *__restrict__ order, int64_t *__restrict__ class_off)
{
    const long long j = (long long)blockIdx.x * ORDER_EL + threadIdx.x;
    if (j >= n_jobs) return;
    order[j] = (int32_t)val[j];
    const int c = (int)(key[j] >> bits), pc = j ? (int)(key[j - 1] >> bits) : -1;
    for (int k = pc + 1; k <= c && k <= GBX_ABEA_METH_NCLASS; ++k) class_off[k] = j;
    if (j == n_jobs - 1)
        for (int k = c + 1; k <= GBX_ABEA_METH_NCLASS; ++k) class_off[k] = n_jobs;
}

struct OrderLayout { size_t o_a[2], o_b[2], o_hist, o_hsum, bytes; };

OrderLayout order_layout(int64_t n_jobs)
{
    OrderLayout L;
    Carver carve;
    const size_t c = (size_t)(n_jobs > 0 ? n_jobs : 1);
    for (int i = 0; i < 2; ++i) { L.o_a[i] = carve(c * 8); L.o_b[i] = carve(c * 4); }
    const long long he = 256 * sort_blocks(n_jobs);
    L.o_hist = carve((size_t)(he + 1) * 8);
    L.o_hsum = carve((size_t)mem_scan_blocks(he) * 8);
    L.bytes = carve.at;
    return L;
}

}  // namespace

size_t abea_meth_sites_work_bytes(int64_t n_reads)
{
    return 2 * align256((size_t)mem_scan_blocks(n_reads > 0 ? n_reads : 0) * 8);          // the block sums of the two scans
}

int abea_meth_sites_launch(int pass, int64_t n_reads, const int64_t *d_ref_off, const int32_t *d_ref_len, const char *d_ref, const int32_t *d_ref_start_pos,
                           const uint8_t *d_rc, const int64_t *d_rec_off, const gbx_abea_pair *d_rec, void *d_work, int64_t *d_site_off, int64_t *d_byte_off,
                           uint8_t *d_bad, int64_t site_cap, gbx_abea_meth_site *d_sites, gbx_abea_meth_job *d_jobs, int64_t seq_cap, char *d_seq_arena,
                           hipStream_t s)
{
    if (n_reads == 0) return GBX_OK;
    if (n_reads > 0x7fffffffLL - 1024) { set_error("abea meth sites: more than 2^31 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    const SitesArgs A{(long long)n_reads, d_ref_off, d_ref_len, d_ref, d_ref_start_pos, d_rc, d_rec_off, d_rec, d_site_off, d_byte_off, d_bad,
                      (long long)site_cap, d_sites, d_jobs, (long long)seq_cap, d_seq_arena};
    if (pass & GBX_ABEA_METH_SITES_COUNT) {
        {
            Stage st("abea_meth_sites_count", s);
            hipLaunchKernelGGL(abea_meth_sites_kernel<false>, dim3((unsigned)n_reads), dim3(64), 0, s, A);
        }
        GBX_HIP(hipGetLastError());
        {
            Stage st("abea_meth_sites_scan", s);
            long long *const bsum = (long long *)d_work;
            scan_launch1((long long *)d_site_off, n_reads, bsum, nullptr, MemScanGuard{}, s);
            scan_launch1((long long *)d_byte_off, n_reads, (long long *)((char *)d_work + align256((size_t)mem_scan_blocks(n_reads) * 8)), nullptr,
                         MemScanGuard{}, s);
        }
        GBX_HIP(hipGetLastError());
    }
    if (pass & GBX_ABEA_METH_SITES_FILL) {
        Stage st("abea_meth_sites_fill", s);
        hipLaunchKernelGGL(abea_meth_sites_kernel<true>, dim3((unsigned)n_reads), dim3(64), 0, s, A);
        GBX_HIP(hipGetLastError());
    }
    return GBX_OK;
}

size_t abea_meth_order_work_bytes(int64_t n_jobs) { return order_layout(n_jobs).bytes; }

int abea_meth_order_launch(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, int64_t seq_bytes, int64_t n_reads, const int64_t *d_event_off, int64_t flank_len,
                           int max_rows_bits, void *d_work, int32_t *d_order, int64_t *d_class_off, int64_t *d_first_bad, hipStream_t s)
{
    if (n_jobs > 0x7fffffffLL - 1024) { set_error("abea meth order: more than 2^31 jobs in one call"); return GBX_ERR_UNSUPPORTED; }
    Stage st("abea_meth_order", s);
    hipLaunchKernelGGL(abea_meth_order_init_kernel, dim3(1), dim3(64), 0, s, d_class_off, d_first_bad);
    GBX_HIP(hipGetLastError());
    if (n_jobs == 0) return GBX_OK;
    const OrderLayout L = order_layout(n_jobs);
    char *const wb = (char *)d_work;
    SortBufs<u32> B;
    for (int i = 0; i < 2; ++i) { B.a[i] = (uint64_t *)(wb + L.o_a[i]); B.b[i] = (u32 *)(wb + L.o_b[i]); }
    B.hist = (long long *)(wb + L.o_hist); B.hsum = (long long *)(wb + L.o_hsum);
    const unsigned blocks = (unsigned)((n_jobs + ORDER_EL - 1) / ORDER_EL);
    hipLaunchKernelGGL(abea_meth_order_key_kernel, dim3(blocks), dim3(ORDER_EL), 0, s, (long long)n_jobs, d_jobs, (long long)seq_bytes, (long long)n_reads,
                       d_event_off, (long long)flank_len, max_rows_bits, B.a[0], B.b[0], d_first_bad);
    GBX_HIP(hipGetLastError());
    SortPass pass[4];
    const int n_pass = (max_rows_bits + 2 + 7) / 8;                                        // the class takes two bits above the rows
    for (int p = 0; p < n_pass; ++p) pass[p] = SortPass{0, 8 * p, 255u};
    const int cur = radix_sort(B, SortCount{nullptr, (long long)n_jobs}, pass, n_pass, s);
    GBX_HIP(hipGetLastError());
    hipLaunchKernelGGL(abea_meth_order_out_kernel, dim3(blocks), dim3(ORDER_EL), 0, s, (long long)n_jobs, (const uint64_t *)B.a[cur], (const u32 *)B.b[cur],
                       max_rows_bits, d_order, d_class_off);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
