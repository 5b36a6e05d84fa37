// host_abea.h — what the abea entries (capi_abea / _events / _calib / _meth / _eventalign .hip) share on the host: the argument checks
// with their error texts, the rebased offsets and the compact event means, the
// transition logarithms, the eventalign kernel's arguments, the calibration behind align() and the score plan.  Every check sets the
// error text and returns GBX_ERR_ARG (event_count_check, a CIGAR past 2^30: GBX_ERR_UNSUPPORTED), or returns GBX_OK.
#pragma once

namespace gbx {

// ---- the checks of read r; `base` = index of read 0 in the caller's job (error texts only)
inline int read_check(const int64_t *seq_off, const int32_t *seq_len, int64_t seq_bytes, int64_t r, const char *who, int64_t base = 0)
{
    if (seq_off[r] >= 0 && seq_len[r] >= 0 && seq_off[r] + seq_len[r] <= seq_bytes) return GBX_OK;
    set_error("%s: read %lld lies outside the arena", who, (long long)(base + r));
    return GBX_ERR_ARG;
}
inline int kmer_check(const int32_t *seq_len, int64_t r, const char *who)
{
    if (seq_len[r] < GBX_ABEA_KMER) { set_error("%s: read %lld needs at least %d bases", who, (long long)r, GBX_ABEA_KMER); return GBX_ERR_ARG; }
    return GBX_OK;
}
inline int event_off_check(const int64_t *event_off, int64_t r, const char *who, int64_t base = 0)
{
    if (event_off[r] >= 0 && event_off[r + 1] >= event_off[r]) return GBX_OK;
    set_error("%s: event_off not monotone at read %lld", who, (long long)(base + r));
    return GBX_ERR_ARG;
}
inline int event_count_check(const int64_t *event_off, int64_t r, const char *who)           // the kernels index a read's events with 32 bits
{
    if (event_off[r + 1] - event_off[r] > 0x3fffffffLL) { set_error("%s: read %lld has too many events", who, (long long)r); return GBX_ERR_UNSUPPORTED; }
    return GBX_OK;
}
inline int ref_segment_check(const int64_t *ref_off, const int32_t *ref_len, int64_t r, const char *who)
{
    if (ref_off[r] < 0 || ref_len[r] < 0) { set_error("%s: bad reference segment at read %lld", who, (long long)r); return GBX_ERR_ARG; }
    return GBX_OK;
}

// where the reference exits or asserts (meth.c:54-58, 65-68, 135), before any device work
inline int check_cigars(const char *who, int64_t n_reads, const int64_t *cigar_off, const uint32_t *cigar, const int32_t *seq_len)
{
    if (cigar_off[0] < 0) { set_error("%s: cigar_off below 0", who); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n_reads; ++r) {
        if (cigar_off[r + 1] < cigar_off[r]) { set_error("%s: cigar_off not monotone at read %lld", who, (long long)r); return GBX_ERR_ARG; }
        if (cigar_off[r + 1] > cigar_off[r] && !cigar) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
        if (int rc = kmer_check(seq_len, r, who)) return rc;
        int64_t aligned = 0, advance = 0;
        for (int64_t c = cigar_off[r]; c < cigar_off[r + 1]; ++c) {
            const int op = (int)(cigar[c] & 0xf);
            const int64_t len = cigar[c] >> 4;
            if (op == 3) { set_error("%s: read %lld: a spliced alignment (operation N)", who, (long long)r); return GBX_ERR_ARG; }
            if (op == 6 || op > 8) { set_error("%s: read %lld: unhandled CIGAR operation %d", who, (long long)r, op); return GBX_ERR_ARG; }
            if (op == 0 || op == 7 || op == 8) aligned += len;
            if (op != 5) advance += len;
        }
        if (aligned > seq_len[r]) {
            set_error("%s: read %lld: %lld aligned bases, the read has %d", who, (long long)r, (long long)aligned, seq_len[r]);
            return GBX_ERR_ARG;
        }
        if (advance > 0x3fffffffLL) { set_error("%s: read %lld: its CIGAR spans more than 2^30 positions", who, (long long)r); return GBX_ERR_UNSUPPORTED; }
    }
    return GBX_OK;
}

// off[0 .. n] relative to off[0]: what the device gets beside an array uploaded from its first used entry
inline std::vector<int64_t> rebased0(const int64_t *off, int64_t n)
{
    std::vector<int64_t> r((size_t)n + 1);
    for (int64_t j = 0; j <= n; ++j) r[(size_t)j] = off[j] - off[0];
    return r;
}

// The means of events[e0 .. e0 + n_ev), compact (one spare entry: never empty).  For the entries that upload with plain copies;
// the entries that run a HostPipe gather the same field on the way up (stage_field4) and make no host copy.
inline std::vector<float> event_means(const gbx_abea_event *events, int64_t e0, int64_t n_ev)
{
    std::vector<float> m((size_t)n_ev + 1);
    for (int64_t i = 0; i < n_ev; ++i) m[(size_t)i] = events[e0 + i].mean;
    return m;
}

// calculate_transitions (hmm.c:212-295, eventalign.c:171-240; the two are the same lines) for a read: lp_mk mb mm_self mm_next bb
// bk bm_next bm_self kk km.  Host C library, so that the logarithms carry the reference's bits.
inline void abea_transitions(double events_per_base, float *t)
{
    float p_stay = 1 - (1 / events_per_base);
    float p_skip = 0.0025, p_bad = 0.001, p_bad_self = p_bad, p_skip_self = 0.3;
    float p_mk = p_skip, p_mb = p_bad, p_mm_self = p_stay;
    float p_mm_next = 1.0f - p_mm_self - p_mk - p_mb;
    float p_bb = p_bad_self, p_bk, p_bm_next, p_bm_self;
    p_bk = p_bm_next = p_bm_self = (1.0f - p_bb) / 3;
    float p_kk = p_skip_self, p_km = 1.0f - p_kk;
    /* the reference's `log` has a float argument in C++: the float overload */
    t[0] = logf(p_mk); t[1] = logf(p_mb); t[2] = logf(p_mm_self); t[3] = logf(p_mm_next);
    t[4] = logf(p_bb); t[5] = logf(p_bk); t[6] = logf(p_bm_next); t[7] = logf(p_bm_self);
    t[8] = logf(p_kk); t[9] = logf(p_km);
}

// The eventalign kernel's arguments from the device pointers, in the order of gbx_abea_eventalign_device (pre0 is the launch's).
inline AbeaEventalignArgs abea_eventalign_args(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, const int64_t *event_off,
                                               const float *event_mean, const gbx_abea_model *models, const float *scale, const float *shift,
                                               const float *var, const float *log_var, const float *trans, const int32_t *map, const int32_t *near,
                                               const int32_t *flags, const int64_t *cigar_off, const uint32_t *cigar, const int32_t *pos,
                                               const uint8_t *rc, const int64_t *ref_off, const int32_t *ref_len, const char *ref, int32_t region_start,
                                               int32_t region_end, const int32_t *order, gbx_abea_eventalign_rec *rec, int32_t *n_rec, int32_t *status,
                                               int64_t *counts, int64_t n_cigar_total, int64_t rows_cap, void *work)
{
    return AbeaEventalignArgs{n_reads, seq_off, seq_len, event_off, event_mean, models, scale, shift, var, log_var, trans, map, near, flags, cigar_off, cigar,
                              pos, rc, ref_off, ref_len, ref, region_start, region_end, order, rec, n_rec, status, counts, n_cigar_total, rows_cap, work, 0.0f};
}

// abea from raw signal, continued on the device (capi_abea_events.hip): what events -> scalings -> align() leave there for all
// n_reads reads, handed to `tail` (a closure over its entry's arguments) on the lane's compute stream once align() is queued.
// Absolute indexing throughout; a read without events has n_pairs 0.  The event records and the pairs are not downloaded.
struct AbeaAligned {
    Lane *L;
    int64_t n_reads, seq_bytes;
    const int64_t *event_off;                 // host, n_reads + 1
    const int32_t *n_pairs;                   // host, n_reads
    const int64_t *d_seq_off; const int32_t *d_seq_len; const char *d_seq;
    const int64_t *d_event_off; const float *d_event_mean; const gbx_abea_model *d_models;
    float *d_scale, *d_shift;
    const gbx_abea_pair *d_pairs;
    const gbx_abea_event *d_events;           // the 24-byte records, beside the means
};
typedef std::function<int(const AbeaAligned &)> abea_tail_fn;
int abea_signal_align_tail(const char *who, int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range, const float *digitisation,
                           const float *offset, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                           const gbx_abea_model *models, int32_t *status, float *scale, float *shift, const abea_tail_fn &tail);

// The calibration behind align(), for the tails of the two one-call entries.  queue() uploads the pair counts and the alignments,
// calibrates and queues the per-read results down to the caller's arrays; finish() drains the stream, takes the logarithm on the
// host (h_log_var may be null) and queues its upload.  The pointers are the device arrays the tail goes on with (scale and shift
// stay where align() left them).  Declare it after every host array the tail queues copies on: its guard drains the stream
// before they die, and before its own.
struct AbeaCalibrated {
    float *var = nullptr, *log_var = nullptr;
    int32_t *map = nullptr, *flags = nullptr, *pos = nullptr;
    int64_t *cigar_off = nullptr, n_cigar = 0; uint32_t *cigar = nullptr; uint8_t *rc = nullptr;
    explicit AbeaCalibrated(Lane *L) : per_read(L), dmap(L), dcg(L), drain{L->compute} {}
    int queue(const AbeaAligned &a, const int64_t *h_cigar_off, const uint32_t *h_cigar, const int32_t *h_pos, const uint8_t *h_rc, float *scale,
              float *shift, float *h_var, double *events_per_base, int32_t *h_flags)
    {
        const hipStream_t cs = a.L->compute;
        const int64_t n = a.n_reads;
        int e;
        n_cigar = h_cigar_off[n] - h_cigar_off[0];
        for (size_t b : {n * 4, n * 4, n * 8, n * 8, n * 4, n * 4, n * 4, n * 4, (n + 1) * 8, n * 4, n}) per_read.want(b);
        if ((e = per_read.alloc()) || (e = dmap.alloc((size_t)a.seq_bytes * 8 + 16)) || (e = dcg.alloc((size_t)n_cigar * 4 + 16))) return e;
        int32_t *dnp = per_read.take<int32_t>(n * 4);
        var = per_read.take<float>(n * 4);
        double *dv64 = per_read.take<double>(n * 8), *depb = per_read.take<double>(n * 8);
        int32_t *dnea = per_read.take<int32_t>(n * 4), *dnm = per_read.take<int32_t>(n * 4);
        flags = per_read.take<int32_t>(n * 4); log_var = per_read.take<float>(n * 4); cigar_off = per_read.take<int64_t>((n + 1) * 8);
        pos = per_read.take<int32_t>(n * 4); rc = per_read.take<uint8_t>(n); map = dmap.as<int32_t>(); cigar = dcg.as<uint32_t>();
        coff = rebased0(h_cigar_off, n);
        v64.resize((size_t)n); nm.resize((size_t)n); lv.resize((size_t)n);
        GBX_HIP(hipMemcpyAsync(dnp, a.n_pairs, (size_t)n * 4, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(cigar_off, coff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, cs));
        if (n_cigar) GBX_HIP(hipMemcpyAsync(cigar, h_cigar + h_cigar_off[0], (size_t)n_cigar * 4, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(pos, h_pos, (size_t)n * 4, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(rc, h_rc, (size_t)n, hipMemcpyHostToDevice, cs));
        if ((e = abea_calib_launch(n, a.d_seq_off, a.d_seq_len, a.d_seq, a.d_event_off, a.d_event_mean, a.d_models, a.d_pairs, dnp, a.d_scale, a.d_shift, var,
                                   dv64, map, depb, dnea, dnm, flags, cs)))
            return e;
        // the per-read calibration comes down: the caller's outputs, and var64 with the M-state counts for the host logarithm
        GBX_HIP(hipMemcpyAsync(scale, a.d_scale, (size_t)n * 4, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(shift, a.d_shift, (size_t)n * 4, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(h_var, var, (size_t)n * 4, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(v64.data(), dv64, (size_t)n * 8, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(events_per_base, depb, (size_t)n * 8, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(nm.data(), dnm, (size_t)n * 4, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(h_flags, flags, (size_t)n * 4, hipMemcpyDeviceToHost, cs));
        return GBX_OK;
    }
    int finish(float *h_log_var)
    {
        GBX_HIP(hipStreamSynchronize(drain.s));
        if (int e = gbx_abea_calib_logvar_host((int64_t)lv.size(), v64.data(), nm.data(), lv.data())) return e;
        if (h_log_var) memcpy(h_log_var, lv.data(), lv.size() * 4);
        GBX_HIP(hipMemcpyAsync(log_var, lv.data(), lv.size() * 4, hipMemcpyHostToDevice, drain.s));
        return GBX_OK;
    }
private:
    Carve per_read;
    DevBuf dmap, dcg;
    std::vector<int64_t> coff; std::vector<double> v64; std::vector<int32_t> nm; std::vector<float> lv;
    StreamDrain drain;
};

using abea_meth_rules::job_rows;

// The per-job checks of the score plan (abea_meth_rules.h: job_check, what the device order stage runs too) with the error texts
// of gbx_abea_meth_plan_host, which both it and the one call give for job j.
inline int abea_meth_job_refuse(int64_t j, const gbx_abea_meth_job &J, int64_t seq_bytes, int64_t n_reads, const int64_t *event_off, int64_t flank_len)
{
    const char *who = "gbx_abea_meth_plan_host";
    const int64_t nk = (int64_t)J.seq_len - GBX_ABEA_KMER + 1;
    switch (abea_meth_rules::job_check(J, seq_bytes, n_reads, event_off, flank_len)) {
        case abea_meth_rules::JOB_OK: return GBX_OK;
        case abea_meth_rules::JOB_STRINGS: set_error("%s: job %lld: its strings need %d bases inside the arena", who, (long long)j, GBX_ABEA_KMER); return GBX_ERR_ARG;
        case abea_meth_rules::JOB_TOO_LONG:
            set_error("%s: job %lld has %lld k-mers (at most %d)", who, (long long)j, (long long)nk, GBX_ABEA_METH_MAX_KMERS);
            return GBX_ERR_UNSUPPORTED;
        case abea_meth_rules::JOB_READ: set_error("%s: job %lld names read %d", who, (long long)j, J.read); return GBX_ERR_ARG;
        case abea_meth_rules::JOB_EVENTS:
            set_error("%s: job %lld: events %d..%d (rc %d) of a read with %lld", who, (long long)j, J.event_start, J.event_stop, J.rc,
                      (long long)(event_off[J.read + 1] - event_off[J.read]));
            return GBX_ERR_ARG;
        default:
            set_error("%s: job %lld has %lld rows, the flank tables %lld entries", who, (long long)j, (long long)job_rows(J), (long long)flank_len);
            return GBX_ERR_ARG;
    }
}

// What the score kernel needs beside the jobs: the flank tables sized by the longest job, the flogsum and transition tables, the
// jobs' order and the class bounds.  build() runs gbx_abea_meth_plan_host and returns its code.
struct AbeaMethPlan {
    int64_t flank_len = 1, class_off[GBX_ABEA_METH_NCLASS + 1];
    std::vector<float> flogsum, trans, pre, post;
    std::vector<int32_t> order;
    int build(int64_t n_jobs, const gbx_abea_meth_job *jobs, int64_t seq_bytes, int64_t n_reads, const int64_t *event_off, const double *events_per_base)
    {
        for (int64_t j = 0; j < n_jobs; ++j) flank_len = std::max(flank_len, job_rows(jobs[j]));
        flank_len += 1;                                      // the longest job's rows, and one
        flogsum.resize(GBX_ABEA_FLOGSUM_TBL); trans.resize((size_t)n_reads * GBX_ABEA_METH_NTRANS); pre.resize((size_t)flank_len); post.resize((size_t)flank_len);
        order.resize((size_t)n_jobs);
        return gbx_abea_meth_plan_host(n_jobs, jobs, seq_bytes, n_reads, event_off, events_per_base, flogsum.data(), trans.data(), flank_len, pre.data(),
                                       post.data(), order.data(), class_off);
    }
};

}  // namespace gbx
