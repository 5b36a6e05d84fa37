// abea_calib_kernels.hip — what f5c runs per read between align() and the methylation score: postalign (align.c:550-650),
// recalibrate_model (align.c:655-762) with the QC rules of scaling_single (f5c.c:1262-1330), and get_event_alignment_record
// (meth.c:15-185).  A wavefront per read; every loop is counted from seq_len, n_pairs or n_cigar.
#include "abea_dev.h"

namespace gbx {

namespace {

using abea_dev::base_rank;
using abea_dev::rec_scan_incl;
using abea_dev::rec_closest;

constexpr int CAL_MIN_M_STATES = 200;      // minNumEventsToRescale, align.c:679

__device__ inline double cal_lane(double v, int j)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// acc + v(lane 0) + v(lane 1) + ... in that order, the same in every lane (lanes that carry no term hold 0.0: x + 0.0 = x)
__device__ inline double cal_ordered_add(double acc, double v)
{
#pragma unroll
    for (int j = 0; j < 64; ++j) acc += cal_lane(v, j);
    return acc;
}

__device__ inline int cal_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the first of the n pairs whose ref_pos is at least k (the pairs never decrease in either field, align.c:476-487)
__device__ inline int cal_lower_kmer(const gbx_abea_pair *p, int n, int k)
{
    int lo = 0, hi = n;
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p[mid].ref_pos < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the first pair of [lo, hi) whose read_pos is above e
__device__ inline int cal_upper_event(const gbx_abea_pair *p, int lo, int hi, int e)
{
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p[mid].read_pos <= e) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Of the k-mers with events in this chunk of 64 (lane l: k-mer b + l, `has`, rank kr): is lane l's the first record of an 'M'
// state?  It is when its rank differs from the rank of the previous k-mer that has events (align.c:633, 643); `prev_rank`
// carries that rank from chunk to chunk (-1 before the first, align.c:596).
__device__ inline bool cal_m_state(bool has, unsigned kr, int lane, int &prev_rank)
{
    const unsigned long long hm = __ballot(has);
    const unsigned long long below = hm & ((1ull << lane) - 1ull);
    const int from_lane = __shfl((int)kr, below ? 63 - __clzll((long long)below) : 0);
    const int pr = below ? from_lane : prev_rank;
    const int last = __shfl((int)kr, hm ? 63 - __clzll((long long)hm) : 0);
    if (hm) prev_rank = last;
    return has && pr != (int)kr;
}

// postalign + recalibrate_model + the QC of scaling_single.  The event_alignment_t array is never written: a k-mer with events
// contributes stop - start + 1 records, the first of them 'M' (its event: start) when the rank changed, every other one 'E'.
__global__ void __launch_bounds__(64) abea_calib_kernel(long long n_reads, const int64_t *__restrict__ seq_off, const int32_t *__restrict__ seq_len,
                                                        const char *__restrict__ seq, const int64_t *__restrict__ event_off,
                                                        const float *__restrict__ event_mean, const gbx_abea_model *__restrict__ models,
                                                        const gbx_abea_pair *__restrict__ pairs, const int32_t *__restrict__ n_pairs,
                                                        float *__restrict__ scale, float *__restrict__ shift, float *__restrict__ var,
                                                        double *__restrict__ var64, int32_t *__restrict__ map, double *__restrict__ events_per_base,
                                                        int32_t *__restrict__ n_event_alignment, int32_t *__restrict__ n_m_state,
                                                        int32_t *__restrict__ flags)
{
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    if (r >= n_reads) return;
    const long long so = seq_off[r];
    const int n_kmers = seq_len[r] - GBX_ABEA_KMER + 1;
    const long long e0 = event_off[r], ne = event_off[r + 1] - e0;
    const int np = (int)min((long long)n_pairs[r], 2 * ne);                    // the read's room: 2 x n_events pairs
    int2 *mp = reinterpret_cast<int2 *>(map) + so;
    if (np <= 0 || ne < 1 || n_kmers < 1) {                                   // f5c.c:1310-1317: could not align
        for (int k = lane; k < n_kmers; k += 64) mp[k] = make_int2(-1, -1);
        if (lane == 0) {
            events_per_base[r] = 0.0; n_event_alignment[r] = 0; n_m_state[r] = 0; var[r] = 0.0f; var64[r] = 0.0;
            flags[r] = GBX_ABEA_FAILED_ALIGNMENT;
        }
        return;
    }
    const gbx_abea_pair *p = pairs + 2 * e0;
    const char *s = seq + so;
    const float *ev = event_mean + e0;
    const int last_event = (int)ne - 1;
    int prev_rank = -1, n_m = 0, n_ea = 0;
    double A00 = 0.0, A01 = 0.0, A11 = 0.0, b0 = 0.0, b1 = 0.0;
    for (int b = 0; b < n_kmers; b += 64) {
        const int k = b + lane;
        int start = -1, stop = -1;
        unsigned kr = 0;
        if (k < n_kmers) {
            // align.c:571-585 with monotone pairs: the pairs of k-mer k are one run, and a pair counts when its event differs
            // from the event of the pair before it; start and stop are the events of the first and the last such pair
            const int i0 = cal_lower_kmer(p, np, k), i1 = cal_lower_kmer(p, np, k + 1);
            if (i0 < i1) {
                const int first = p[i0].read_pos, before = i0 > 0 ? p[i0 - 1].read_pos : -1;
                const int f = first != before ? i0 : cal_upper_event(p, i0, i1, first);
                if (f < i1) { start = p[f].read_pos; stop = p[i1 - 1].read_pos; }
            }
            mp[k] = make_int2(start, stop);
            for (int q = 0; q < GBX_ABEA_KMER; ++q) kr = kr << 2 | base_rank(s[k + q]);
        }
        const bool has = start != -1;
        const bool is_m = cal_m_state(has, kr, lane, prev_rank);
        n_m += __popcll(__ballot(is_m));
        n_ea += cal_wave_sum(has ? stop - start + 1 : 0);
        double t00 = 0.0, t01 = 0.0, t11 = 0.0, tb0 = 0.0, tb1 = 0.0;
        if (is_m) {                                                           // align.c:695-710
            const double e = (double)ev[min(max(start, 0), last_event)];
            const double mu = (double)models[kr].level_mean, sd = (double)models[kr].level_stdv;
            const double inv_var = 1. / (sd * sd);
            t00 = inv_var; t01 = mu * inv_var; t11 = (mu * mu) * inv_var;
            tb0 = e * inv_var; tb1 = (mu * e) * inv_var;
        }
        if (__ballot(is_m)) {
#pragma unroll
            for (int j = 0; j < 64; ++j) {                                    // five sums, each in k-mer order
                A00 += cal_lane(t00, j); A01 += cal_lane(t01, j); A11 += cal_lane(t11, j);
                b0 += cal_lane(tb0, j); b1 += cal_lane(tb1, j);
            }
        }
    }
    // align.c:566-591: min_event starts at INT32_MAX, max_event at 0; the first pair holds the least event, the last the greatest
    const int max_event = max(0, p[np - 1].read_pos), min_event = min(0x7fffffff, p[0].read_pos);
    const double epb = (double)(max_event - min_event) / n_kmers;
    int fl = 0;
    float var_f = 0.0f;
    double var_d = 0.0;
    if (n_m >= CAL_MIN_M_STATES) {
        const double A10 = A01;
        const double div = A00 * A11 - A01 * A10;                             // align.c:718-720
        const double sh = -(A01 * b1 - A11 * b0) / div;
        const double sc = (A00 * b1 - A10 * b0) / div;
        __syncthreads();                                                      // the map is read back: one wavefront, its own stores
        double v = 0.0;
        prev_rank = -1;
        for (int b = 0; b < n_kmers; b += 64) {                               // align.c:729-741
            const int k = b + lane;
            int start = -1;
            unsigned kr = 0;
            if (k < n_kmers) {
                start = mp[k].x;
                for (int q = 0; q < GBX_ABEA_KMER; ++q) kr = kr << 2 | base_rank(s[k + q]);
            }
            const bool is_m = cal_m_state(start != -1, kr, lane, prev_rank);
            double t = 0.0;
            if (is_m) {
                const double e = (double)ev[min(max(start, 0), last_event)];
                const double mu = (double)models[kr].level_mean, sd = (double)models[kr].level_stdv;
                const double yi = (e - sh - sc * mu);
                t = yi * yi / (sd * sd);
            }
            if (__ballot(is_m)) v = cal_ordered_add(v, t);
        }
        v /= n_m;
        v = sqrt(v);
        var_d = v;
        var_f = (float)v;
        if (lane == 0) { shift[r] = (float)sh; scale[r] = (float)sc; }
        if (var_f > 2.5) fl = GBX_ABEA_FAILED_CALIBRATION;                    // MIN_CALIBRATION_VAR, f5cmisc.h:9; f5c.c:1300
    } else {
        fl = GBX_ABEA_FAILED_CALIBRATION;
    }
    if (!fl && epb > 5.0) fl = GBX_ABEA_FAILED_QUALITY_CHK;                   // f5c.c:1321
    if (lane == 0) {
        events_per_base[r] = epb; n_event_alignment[r] = n_ea; n_m_state[r] = n_m; var[r] = var_f; var64[r] = var_d;
        flags[r] = fl;
    }
}

// ---- get_event_alignment_record

// near[k] = (the largest k' <= k whose k-mer has events or -1, the smallest k' >= k or n_kmers): get_next_event's two walks
// (meth.c:92-102) as a max-scan and a min-scan over the map
__device__ inline void rec_near_scan(const int2 *mp, int2 *nr, int n_kmers, int lane)
{
    int carry = -1;
    for (int b = 0; b < n_kmers; b += 64) {
        const int k = b + lane;
        const unsigned long long hm = __ballot(k < n_kmers && mp[k].x != -1);
        const unsigned long long upto = hm & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);
        if (k < n_kmers) nr[k].x = upto ? b + 63 - __clzll((long long)upto) : carry;
        if (hm) carry = b + 63 - __clzll((long long)hm);
    }
    carry = n_kmers;
    for (int b = (n_kmers - 1) / 64 * 64; b >= 0; b -= 64) {
        const int k = b + lane;
        const unsigned long long hm = __ballot(k < n_kmers && mp[k].x != -1);
        const unsigned long long from = hm & (~0ull << lane);
        if (k < n_kmers) nr[k].y = from ? b + __ffsll((long long)from) - 1 : carry;
        if (hm) carry = b + __ffsll((long long)hm) - 1;
    }
}

// One chunk of 64 CIGAR operations of get_aligned_segments (meth.c:36-85), lane l: operation c + l.  The pairs an operation
// emits and the record keeps (meth.c:148-154: 6 <= read_pos, read_pos + 6 < read_length) are read_pos lo .. lo + cnt - 1;
// ref0 is the reference position of the first of them, excl the kept pairs of this chunk before the operation.
struct RecChunk { int lo, cnt, excl, total; long long ref0; };

__device__ inline RecChunk rec_chunk(const uint32_t *cig, long long n_cigar, long long c, int lane, int read_len, long long pos,
                                     long long &read_pos, long long &ref_adv)
{
    const bool live = c + lane < n_cigar;
    const uint32_t w = live ? cig[c + lane] : 0u;
    const long long len = live ? (long long)(w >> 4) : 0;
    const int op = (int)(w & 0xf);
    const bool aligned = op == 0 || op == 7 || op == 8;                       // M, =, X
    const long long rinc = (aligned || op == 1 || op == 4) ? len : 0;         // I and S advance the read
    const long long finc = (aligned || op == 2) ? len : 0;                    // D advances the reference; H advances nothing
    const long long ri = rec_scan_incl(rinc, lane), fi = rec_scan_incl(finc, lane);
    const long long rp = read_pos + ri - rinc, fp = ref_adv + fi - finc;
    const long long lo = max(rp, (long long)GBX_ABEA_KMER), hi = min(rp + len, (long long)read_len - GBX_ABEA_KMER);
    RecChunk ch;
    ch.cnt = aligned && hi > lo ? (int)(hi - lo) : 0;
    ch.lo = ch.cnt ? (int)lo : 0;
    ch.ref0 = pos + fp + (lo - rp);
    const long long ki = rec_scan_incl(ch.cnt, lane);
    ch.excl = (int)(ki - ch.cnt);
    ch.total = (int)__shfl(ki, 63);
    read_pos += __shfl(ri, 63);
    ref_adv += __shfl(fi, 63);
    return ch;
}

// count pass: the nearest-k-mer table of every read and the length of its record (0 for a flagged read, meth_single,
// f5c.c:1376, and for a degenerate record, meth.c:169-178)
__global__ void __launch_bounds__(64) abea_record_count_kernel(long long n_reads, const int64_t *__restrict__ cigar_off, const uint32_t *__restrict__ cigar,
                                                               const int32_t *__restrict__ pos, const uint8_t *__restrict__ rc,
                                                               const int64_t *__restrict__ seq_off, const int32_t *__restrict__ seq_len,
                                                               const int32_t *__restrict__ map, const int32_t *__restrict__ flags,
                                                               int32_t *__restrict__ near, int64_t *__restrict__ n_rec)
{
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    if (r >= n_reads) return;
    const int read_len = seq_len[r], n_kmers = read_len - GBX_ABEA_KMER + 1;
    if ((flags && flags[r] != 0) || n_kmers < 1) {
        if (lane == 0) n_rec[r] = 0;
        return;
    }
    const int2 *mp = reinterpret_cast<const int2 *>(map) + seq_off[r];
    int2 *nr = reinterpret_cast<int2 *>(near) + seq_off[r];
    rec_near_scan(mp, nr, n_kmers, lane);
    // lane 0 reads entries of near[] below that other lanes of this wavefront have just stored: the barrier of this one-wavefront
    // block orders them, and no entry is read anywhere above this line - keep it so, or fence, if near[] is ever read earlier
    __threadfence_block();
    __syncthreads();
    const uint32_t *cig = cigar + cigar_off[r];
    const long long n_cigar = cigar_off[r + 1] - cigar_off[r];
    long long read_pos = 0, ref_adv = 0, kept = 0;
    int first = 0x7fffffff, last = -1;
    for (long long c = 0; c < n_cigar; c += 64) {
        const RecChunk ch = rec_chunk(cig, n_cigar, c, lane, read_len, pos[r], read_pos, ref_adv);
        if (ch.cnt) { first = min(first, ch.lo); last = max(last, ch.lo + ch.cnt - 1); }
        kept += ch.total;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) { first = min(first, __shfl_xor(first, d)); last = max(last, __shfl_xor(last, d)); }
    if (lane != 0) return;
    if (kept > 0) {
        const bool rev = rc[r] != 0;
        const int ef = rec_closest(mp, nr, rev ? read_len - first - GBX_ABEA_KMER : first, n_kmers);
        const int el = rec_closest(mp, nr, rev ? read_len - last - GBX_ABEA_KMER : last, n_kmers);
        if (ef == el) kept = 0;
    }
    n_rec[r] = kept;
}

// rec_off = exclusive scan of the counts, in place (one wavefront: lane l sums reads [l c, (l + 1) c), the wavefront scans the sums)
__global__ void __launch_bounds__(64) abea_record_scan_kernel(long long n_reads, int64_t *__restrict__ rec_off)
{
    const int lane = threadIdx.x;
    const long long c = (n_reads + 63) / 64, a = min(n_reads, lane * c), b = min(n_reads, a + c);
    long long mine = 0;
    for (long long r = a; r < b; ++r) mine += rec_off[r];
    const long long incl = rec_scan_incl(mine, lane);
    const long long total = __shfl(incl, 63);
    __syncthreads();
    long long run = incl - mine;
    for (long long r = a; r < b; ++r) { const long long n = rec_off[r]; rec_off[r] = run; run += n; }
    if (lane == 63) rec_off[n_reads] = total;
}

// fill pass: the kept pairs of a read are a contiguous run of its segment list; output slot t of a chunk belongs to the
// operation with the largest excl <= t
__global__ void __launch_bounds__(64) abea_record_fill_kernel(long long n_reads, const int64_t *__restrict__ cigar_off, const uint32_t *__restrict__ cigar,
                                                              const int32_t *__restrict__ pos, const uint8_t *__restrict__ rc,
                                                              const int64_t *__restrict__ seq_off, const int32_t *__restrict__ seq_len,
                                                              const int32_t *__restrict__ map, const int32_t *__restrict__ near,
                                                              const int64_t *__restrict__ rec_off, gbx_abea_pair *__restrict__ rec, long long rec_cap)
{
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    if (r >= n_reads) return;
    const long long out0 = rec_off[r], n_out = rec_off[r + 1] - out0;
    if (n_out <= 0 || out0 < 0 || out0 + n_out > rec_cap) return;
    const int read_len = seq_len[r], n_kmers = read_len - GBX_ABEA_KMER + 1;
    const int2 *mp = reinterpret_cast<const int2 *>(map) + seq_off[r];
    const int2 *nr = reinterpret_cast<const int2 *>(near) + seq_off[r];
    const uint32_t *cig = cigar + cigar_off[r];
    const long long n_cigar = cigar_off[r + 1] - cigar_off[r];
    const bool rev = rc[r] != 0;
    long long read_pos = 0, ref_adv = 0, kept = 0;
    for (long long c = 0; c < n_cigar; c += 64) {
        const RecChunk ch = rec_chunk(cig, n_cigar, c, lane, read_len, pos[r], read_pos, ref_adv);
        for (int t0 = 0; t0 < ch.total; t0 += 64) {
            const int t = t0 + lane;
            int o = 0;
#pragma unroll
            for (int step = 32; step; step >>= 1) {
                const int ex = __shfl(ch.excl, (o + step) & 63);
                if (o + step < 64 && ex <= t) o += step;
            }
            const int j = t - __shfl(ch.excl, o);
            const int rp = __shfl(ch.lo, o) + j;
            const long long ref = __shfl(ch.ref0, o) + j;
            if (t < ch.total && kept + t < n_out) {
                gbx_abea_pair q;
                q.ref_pos = (int32_t)ref;
                q.read_pos = rec_closest(mp, nr, rev ? read_len - rp - GBX_ABEA_KMER : rp, n_kmers);
                rec[out0 + kept + t] = q;
            }
        }
        kept += ch.total;
    }
}

}  // namespace

int abea_calib_launch(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq, const int64_t *d_event_off,
                      const float *d_event_mean, const gbx_abea_model *d_models, const gbx_abea_pair *d_pairs, const int32_t *d_n_pairs,
                      float *d_scale, float *d_shift, float *d_var, double *d_var64, int32_t *d_map, double *d_events_per_base,
                      int32_t *d_n_event_alignment, int32_t *d_n_m_state, int32_t *d_flags, hipStream_t s)
{
    if (n_reads == 0) return GBX_OK;
    if (n_reads > 0x7fffffffLL - 1024) { set_error("abea calib: more than 2^31 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    Stage st("abea_calib", s);
    hipLaunchKernelGGL(abea_calib_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, (long long)n_reads, d_seq_off, d_seq_len, d_seq, d_event_off,
                       d_event_mean, d_models, d_pairs, d_n_pairs, d_scale, d_shift, d_var, d_var64, d_map, d_events_per_base, d_n_event_alignment,
                       d_n_m_state, d_flags);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

int abea_record_launch(int pass, int64_t n_reads, const int64_t *d_cigar_off, const uint32_t *d_cigar, const int32_t *d_pos, const uint8_t *d_rc,
                       const int64_t *d_seq_off, const int32_t *d_seq_len, const int32_t *d_map, const int32_t *d_flags, int32_t *d_near,
                       int64_t *d_rec_off, gbx_abea_pair *d_rec, int64_t rec_cap, hipStream_t s)
{
    if (n_reads == 0) return GBX_OK;
    if (n_reads > 0x7fffffffLL - 1024) { set_error("abea record: more than 2^31 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    if (pass & GBX_ABEA_RECORD_COUNT) {
        {
            Stage st("abea_record_count", s);
            hipLaunchKernelGGL(abea_record_count_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, (long long)n_reads, d_cigar_off, d_cigar, d_pos, d_rc,
                               d_seq_off, d_seq_len, d_map, d_flags, d_near, d_rec_off);
        }
        GBX_HIP(hipGetLastError());
        {
            Stage st("abea_record_scan", s);
            hipLaunchKernelGGL(abea_record_scan_kernel, dim3(1), dim3(64), 0, s, (long long)n_reads, d_rec_off);
        }
        GBX_HIP(hipGetLastError());
    }
    if (pass & GBX_ABEA_RECORD_FILL) {
        Stage st("abea_record_fill", s);
        hipLaunchKernelGGL(abea_record_fill_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, (long long)n_reads, d_cigar_off, d_cigar, d_pos, d_rc, d_seq_off,
                           d_seq_len, d_map, (const int32_t *)d_near, (const int64_t *)d_rec_off, d_rec, (long long)rec_cap);
        GBX_HIP(hipGetLastError());
    }
    return GBX_OK;
}

}  // namespace gbx
