// abea_events_kernels.hip — what f5c runs per read before align(): ADC counts -> pA, scrappie's event detector and the
// method-of-moments scalings (R/benchmarks/abea/src/f5c.c:1219-1242 event_single, events.c:292-549, align.c:49-97).
// gfx950 only.  Bit-exact to the reference's order of operations; the file is compiled with
// -ffp-contract=off like the rest of the library, and every mixed float / double expression below is written with
// the conversions the C expression implies.
//
// One wavefront (= one block) per read, the samples in tiles of 64:
//   1. the tile's 64 samples become pA and join the cumulative sums S (sum) and Q (sum of float squares), doubles, kept
//      for the last 256 positions in LDS.  Reads that pass the exactness predicate (abea_events_exact) take a
//      wavefront scan, the others one lane adding in index order.
//   2. every lane computes the two windowed t-statistics of one position (6 positions behind the newest sample, the
//      longer window's look-ahead).
//   3. lane 0 walks the short / long peak detector over the tile's 64 positions.  The next tile's samples are
//      already in flight.
// The kernel runs twice: a count pass (events per read, status), and after an exclusive scan over the reads a fill
// pass that writes the packed event records and means.
#include "abea_dev.h"
#include <cfloat>

namespace gbx {

namespace {

constexpr int EV_TILE = 64, EV_RING = 256, EV_LOOK = 6;
constexpr int EV_W1 = 3, EV_W2 = 6;                         // event_detection_defaults, events.c:42-46
constexpr float EV_THR1 = 1.4f, EV_THR2 = 9.0f, EV_PEAK_HEIGHT = 0.2f;

// events.c:337-360 for one position w <= i <= n - w (the caller has checked that); S[k], Q[k] at ring[k & 255]
__device__ inline float ev_tstat(const double *rs, const double *rq, long long i, int w)
{
    const float wf = (float)w;
    double sum1 = rs[i & (EV_RING - 1)], sumsq1 = rq[i & (EV_RING - 1)];
    if (i > w) {
        sum1 -= rs[(i - w) & (EV_RING - 1)];
        sumsq1 -= rq[(i - w) & (EV_RING - 1)];
    }
    const float sum2 = (float)(rs[(i + w) & (EV_RING - 1)] - rs[i & (EV_RING - 1)]);
    const float sumsq2 = (float)(rq[(i + w) & (EV_RING - 1)] - rq[i & (EV_RING - 1)]);
    const float mean1 = (float)(sum1 / (double)wf);
    const float mean2 = sum2 / wf;
    const float m1sq = mean1 * mean1, m2sq = mean2 * mean2, q2 = sumsq2 / wf;
    float combined_var = (float)(((sumsq1 / (double)wf - (double)m1sq) + (double)q2) - (double)m2sq);
    combined_var = fmaxf(combined_var, FLT_MIN);
    const float delta_mean = mean2 - mean1;
    const float cw = combined_var / wf;
    return (float)(fabs((double)delta_mean) / sqrt((double)cw));
}

// create_event, events.c:456-472
__device__ inline gbx_abea_event ev_create(unsigned long long start, unsigned long long end, double s0, double q0, double s1, double q1)
{
    gbx_abea_event e;
    e.start = start;
    e.length = (float)(end - start);
    e.mean = (float)(s1 - s0) / e.length;
    const float deltasqr = (float)(q1 - q0);
    const float msq = e.mean * e.mean;
    const float var = deltasqr / e.length - msq;
    e.stdv = sqrtf(fmaxf(var, 0.0f));
    return e;
}

struct EvDet {                      // Detector, events.c:268-279 (DEF_PEAK_POS -1, DEF_PEAK_VAL FLT_MAX)
    long long masked_to, peak_pos;
    float peak_value;
    bool valid;
    double ps, pq;                  // S, Q at peak_pos once its tile has gone by (fill pass)
};

// Every partial sum of the read's pA values and of their float squares is exactly representable in a double, so any
// summation order gives the in-order bits: the non-zero |pA| lie in [2^emin, 2^emax), squares are multiples of
// 2^(2 emin - 23) below 2^(2 emax), n of them stay below 2^(ceil(log2 n) + 2 emax).  e_lo / e_hi: the smallest and the
// largest biased exponent field seen (e_lo > e_hi: no non-zero sample).
__device__ inline bool abea_events_exact(long long n, int e_lo, int e_hi)
{
    if (e_lo > e_hi) return true;
    if (e_lo == 0 || e_hi == 255) return false;            // denormals, infinities, NaN
    const int lg = n <= 1 ? 0 : 64 - __clzll((unsigned long long)(n - 1));
    return lg + 2 * (e_hi + 1) + 2 - 2 * e_lo + 23 <= 53;
}

template <bool FILL>
__global__ void __launch_bounds__(EV_TILE) abea_events_kernel(long long n_reads, const int16_t *__restrict__ raw, const int64_t *__restrict__ raw_off,
                                                              const float *__restrict__ range, const float *__restrict__ digitisation,
                                                              const float *__restrict__ offset, int64_t *__restrict__ n_events,
                                                              const int64_t *__restrict__ event_off, gbx_abea_event *__restrict__ events,
                                                              float *__restrict__ event_mean, long long event_cap, int32_t *__restrict__ status)
{
    __shared__ double rs[EV_RING], rq[EV_RING];
    __shared__ float ts1[EV_TILE], ts2[EV_TILE];
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    if (r >= n_reads) return;
    const long long o = raw_off[r], n = raw_off[r + 1] - o;
    const float raw_unit = range[r] / digitisation[r], off = offset[r];     // f5c.c:1228
    const int16_t *x = raw + o;

    bool inorder;
    if (!FILL) {
        int e_lo = 256, e_hi = -1;
        for (long long k = lane; k < n; k += EV_TILE) {
            const float p = ((float)x[k] + off) * raw_unit;
            const unsigned b = __float_as_uint(p) & 0x7fffffffu;
            if (b) { const int e = (int)(b >> 23); e_lo = min(e_lo, e); e_hi = max(e_hi, e); }
        }
        for (int d = 32; d; d >>= 1) { e_lo = min(e_lo, __shfl_xor(e_lo, d)); e_hi = max(e_hi, __shfl_xor(e_hi, d)); }
        inorder = !abea_events_exact(n, e_lo, e_hi);
    } else {
        inorder = (status[r] & GBX_ABEA_EV_INORDER) != 0;
    }

    const long long ev0 = FILL ? event_off[r] : 0, ev1 = FILL ? event_off[r + 1] : 0;
    const bool writes = FILL && ev1 <= event_cap;
    EvDet ds = {0, -1, FLT_MAX, false, 0.0, 0.0}, dl = ds;
    long long n_peaks = 0, prev_pos = 0;
    double prev_s = 0.0, prev_q = 0.0, carry_s = 0.0, carry_q = 0.0;
    if (lane == 0) { rs[0] = 0.0; rq[0] = 0.0; }

    const long long n_tiles = (n + EV_LOOK + EV_TILE - 1) / EV_TILE;         // positions [64 t - 6, 64 t + 58) in tile t
    GBX_GUARD(guard, n / EV_TILE + 2);
    int16_t nxt = lane < n ? x[lane] : (int16_t)0;
    for (long long t = 0; t < n_tiles; ++t) {
        if (GBX_GUARD_TRIP(guard, GBX_GK_ABEA, 10, r)) break;
        const long long k = t * EV_TILE + lane, kn = k + EV_TILE;
        const int16_t cur = nxt;
        nxt = kn < n ? x[kn] : (int16_t)0;
        const float p = k < n ? ((float)cur + off) * raw_unit : 0.0f;          // f5c.c:1230
        const float psq = p * p;                                              // events.c:300: a float product, widened by the sum
        double vs = (double)p, vq = (double)psq;
        if (!inorder) {
            for (int d = 1; d < EV_TILE; d <<= 1) {
                const double us = __shfl_up(vs, d), uq = __shfl_up(vq, d);
                if (lane >= d) { vs += us; vq += uq; }
            }
            vs += carry_s; vq += carry_q;
            rs[(k + 1) & (EV_RING - 1)] = vs; rq[(k + 1) & (EV_RING - 1)] = vq;
            carry_s = __shfl(vs, EV_TILE - 1); carry_q = __shfl(vq, EV_TILE - 1);
            __syncthreads();
        } else {
            rs[(k + 1) & (EV_RING - 1)] = vs; rq[(k + 1) & (EV_RING - 1)] = vq;
            __syncthreads();
            if (lane == 0) {
                double as = carry_s, aq = carry_q;
                for (int j = 1; j <= EV_TILE; ++j) {                          // events.c:298-301, in index order
                    const int at = (int)((t * EV_TILE + j) & (EV_RING - 1));
                    as += rs[at]; aq += rq[at];
                    rs[at] = as; rq[at] = aq;
                }
            }
            __syncthreads();
            carry_s = rs[(t * EV_TILE + EV_TILE) & (EV_RING - 1)]; carry_q = rq[(t * EV_TILE + EV_TILE) & (EV_RING - 1)];
        }
        // the t-statistics of position i: zero outside [w, n - w] and for reads shorter than 2 w (events.c:327-334)
        const long long lo = t * EV_TILE - EV_LOOK, i = lo + lane;
        float t1 = 0.0f, t2 = 0.0f;
        if (i >= EV_W1 && i <= n - EV_W1) t1 = ev_tstat(rs, rq, i, EV_W1);
        if (i >= EV_W2 && i <= n - EV_W2) t2 = ev_tstat(rs, rq, i, EV_W2);
        ts1[lane] = t1; ts2[lane] = t2;
        __syncthreads();
        if (lane == 0) {
            const int j0 = lo < 0 ? (int)-lo : 0;
            const int j1 = n - lo < EV_TILE ? (int)(n - lo) : EV_TILE;
            for (int j = j0; j < j1; ++j) {                                   // short_long_peak_detector, events.c:382-439
                const long long pos = lo + j;
#pragma unroll
                for (int kd = 0; kd < 2; ++kd) {
                    EvDet &d = kd == 0 ? ds : dl;
                    const float thr = kd == 0 ? EV_THR1 : EV_THR2;
                    const int w = kd == 0 ? EV_W1 : EV_W2;
                    if (d.masked_to >= pos) continue;
                    const float v = kd == 0 ? ts1[j] : ts2[j];
                    if (d.peak_pos == -1) {
                        if (v < d.peak_value) d.peak_value = v;
                        else if (v - d.peak_value > EV_PEAK_HEIGHT) { d.peak_value = v; d.peak_pos = pos; }
                    } else {
                        if (v > d.peak_value) { d.peak_value = v; d.peak_pos = pos; }
                        if (kd == 0 && d.peak_value > thr) {
                            dl.masked_to = d.peak_pos + w;
                            dl.peak_pos = -1; dl.peak_value = FLT_MAX; dl.valid = false;
                        }
                        if (d.peak_value - v > EV_PEAK_HEIGHT && d.peak_value > thr) d.valid = true;
                        if (d.valid && (pos - d.peak_pos) > w / 2) {
                            if (FILL) {                                       // create_events: the event that ends at this peak
                                const bool here = d.peak_pos >= lo;
                                const double s1 = here ? rs[d.peak_pos & (EV_RING - 1)] : d.ps, q1 = here ? rq[d.peak_pos & (EV_RING - 1)] : d.pq;
                                const long long at = ev0 + n_peaks;
                                if (writes && at < ev1) {
                                    const gbx_abea_event e = ev_create((unsigned long long)prev_pos, (unsigned long long)d.peak_pos, prev_s, prev_q, s1, q1);
                                    events[at] = e;
                                    event_mean[at] = e.mean;
                                }
                                prev_pos = d.peak_pos; prev_s = s1; prev_q = q1;
                            }
                            ++n_peaks;
                            d.peak_pos = -1; d.peak_value = v; d.valid = false;
                        }
                    }
                }
            }
            if (FILL) {                                                       // a pending peak of this tile: its sums leave the ring later
                if (ds.peak_pos >= lo) { ds.ps = rs[ds.peak_pos & (EV_RING - 1)]; ds.pq = rq[ds.peak_pos & (EV_RING - 1)]; }
                if (dl.peak_pos >= lo) { dl.ps = rs[dl.peak_pos & (EV_RING - 1)]; dl.pq = rq[dl.peak_pos & (EV_RING - 1)]; }
            }
        }
        __syncthreads();
    }
    if (lane != 0) return;
    if (!FILL) {
        // no peak: the reference reads peaks[-1] (events.c:499); here the read has no events and a status bit
        n_events[r] = n_peaks ? n_peaks + 1 : 0;
        status[r] = (inorder ? GBX_ABEA_EV_INORDER : 0) | (n_peaks ? 0 : GBX_ABEA_EV_NONE);
    } else if (!writes) {
        if (ev1 > ev0) status[r] |= GBX_ABEA_EV_OVERFLOW;
    } else if (n_peaks) {
        const long long at = ev0 + n_peaks;                                   // the last event ends at nsample (carry = S[n], Q[n])
        if (at < ev1) {
            const gbx_abea_event e = ev_create((unsigned long long)prev_pos, (unsigned long long)n, prev_s, prev_q, carry_s, carry_q);
            events[at] = e;
            event_mean[at] = e.mean;
        }
    }
}

// event_off = exclusive scan of n_events (one wavefront: lane l sums reads [l c, (l+1) c), the wavefront scans the 64 sums)
__global__ void __launch_bounds__(64) abea_events_scan_kernel(long long n_reads, const int64_t *__restrict__ n_events, int64_t *__restrict__ event_off)
{
    const int lane = threadIdx.x;
    const long long c = (n_reads + 63) / 64, a = min(n_reads, lane * c), b = min(n_reads, a + c);
    long long mine = 0;
    for (long long r = a; r < b; ++r) mine += n_events[r];
    long long incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    long long run = incl - mine;
    for (long long r = a; r < b; ++r) { event_off[r] = run; run += n_events[r]; }
    if (lane == 63) event_off[n_reads] = incl;
}

// acc + v(lane 0) + v(lane 1) + ... in that order, the same in every lane (lanes past the data hold 0.0: x + 0.0 = x)
__device__ inline double ev_ordered_add(double acc, double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
#pragma unroll
    for (int j = 0; j < 64; ++j)
        acc += __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
    return acc;
}

// estimate_scalings_using_mom, align.c:49-97: a wavefront per read; the terms are formed 64 at a time, the double sums
// run in index order.  A read without events or without a k-mer gets scale = shift = 0.
__global__ void __launch_bounds__(64) abea_scalings_kernel(long long n_reads, const int64_t *__restrict__ seq_off, const int32_t *__restrict__ seq_len,
                                                           const char *__restrict__ seq, const int64_t *__restrict__ event_off,
                                                           const float *__restrict__ event_mean, const gbx_abea_model *__restrict__ models,
                                                           float *__restrict__ scale, float *__restrict__ shift)
{
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    if (r >= n_reads) return;
    const long long e0 = event_off[r], ne = event_off[r + 1] - e0;
    const long long n_kmers = (long long)seq_len[r] - GBX_ABEA_KMER + 1;
    if (ne < 1 || n_kmers < 1) {
        if (lane == 0) { scale[r] = 0.0f; shift[r] = 0.0f; }
        return;
    }
    const float *ev = event_mean + e0;
    double event_level_sum = 0.0;
    for (long long b = 0; b < ne; b += 64)
        event_level_sum = ev_ordered_add(event_level_sum, b + lane < ne ? (double)ev[b + lane] : 0.0);
    const char *s = seq + seq_off[r];
    double kmer_level_sum = 0.0, kmer_level_sq_sum = 0.0;
    for (long long b = 0; b < n_kmers; b += 64) {
        double l = 0.0;
        if (b + lane < n_kmers) {
            unsigned kr = 0;
            for (int q = 0; q < GBX_ABEA_KMER; ++q) kr = kr << 2 | abea_dev::base_rank(s[b + lane + q]);
            l = (double)models[kr].level_mean;
        }
        kmer_level_sum = ev_ordered_add(kmer_level_sum, l);
        kmer_level_sq_sum = ev_ordered_add(kmer_level_sq_sum, l * l);
    }
    const double sh = event_level_sum / (double)(unsigned long long)ne - kmer_level_sum / (double)(int)n_kmers;
    double event_level_sq_sum = 0.0;
    for (long long b = 0; b < ne; b += 64) {
        double d = 0.0;
        if (b + lane < ne) { d = (double)ev[b + lane] - sh; d = d * d; }
        event_level_sq_sum = ev_ordered_add(event_level_sq_sum, d);
    }
    const double sc = (event_level_sq_sum / (double)(unsigned long long)ne) / (kmer_level_sq_sum / (double)(int)n_kmers);
    if (lane == 0) { shift[r] = (float)sh; scale[r] = (float)sc; }
}

}  // namespace

int abea_events_launch(int pass, int64_t n_reads, const int16_t *d_raw, const int64_t *d_raw_off, const float *d_range,
                       const float *d_digitisation, const float *d_offset, int64_t *d_n_events, int64_t *d_event_off,
                       gbx_abea_event *d_events, float *d_event_mean, int64_t event_cap, int32_t *d_status, hipStream_t s)
{
    if (n_reads == 0) return GBX_OK;
    if (n_reads > 0x7fffffffLL - 1024) { set_error("abea events: more than 2^31 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    if (pass & GBX_ABEA_EVENTS_COUNT) {
        {
            Stage st("abea_events_count", s);
            hipLaunchKernelGGL(abea_events_kernel<false>, dim3((unsigned)n_reads), dim3(EV_TILE), 0, s, (long long)n_reads, d_raw, d_raw_off, d_range,
                               d_digitisation, d_offset, d_n_events, (const int64_t *)nullptr, (gbx_abea_event *)nullptr, (float *)nullptr, 0LL, d_status);
        }
        GBX_HIP(hipGetLastError());
        {
            Stage st("abea_events_scan", s);
            hipLaunchKernelGGL(abea_events_scan_kernel, dim3(1), dim3(64), 0, s, (long long)n_reads, d_n_events, d_event_off);
        }
        GBX_HIP(hipGetLastError());
    }
    if (pass & GBX_ABEA_EVENTS_FILL) {
        Stage st("abea_events_fill", s);
        hipLaunchKernelGGL(abea_events_kernel<true>, dim3((unsigned)n_reads), dim3(EV_TILE), 0, s, (long long)n_reads, d_raw, d_raw_off, d_range,
                           d_digitisation, d_offset, d_n_events, (const int64_t *)d_event_off, d_events, d_event_mean, (long long)event_cap, d_status);
        GBX_HIP(hipGetLastError());
    }
    GBX_GUARD_CHECK("abea events");
    return GBX_OK;
}

int abea_scalings_launch(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq, const int64_t *d_event_off,
                         const float *d_event_mean, const gbx_abea_model *d_models, float *d_scale, float *d_shift, hipStream_t s)
{
    if (n_reads == 0) return GBX_OK;
    if (n_reads > 0x7fffffffLL - 1024) { set_error("abea scalings: more than 2^31 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    Stage st("abea_scalings", s);
    hipLaunchKernelGGL(abea_scalings_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, (long long)n_reads, d_seq_off, d_seq_len, d_seq, d_event_off,
                       d_event_mean, d_models, d_scale, d_shift);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
