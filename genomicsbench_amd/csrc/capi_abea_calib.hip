// capi_abea_calib.hip — abea between align() and the methylation score: the calibration and event-alignment record entries of
// the C-ABI (include/gbx.h), and call-methylation from raw signal in one call.
#include "capi_common.h"

using namespace gbx;

namespace {

// COUNT, the total (rec_off != nullptr: all the offsets) to the host, FILL.  The record stays on the device, in drec at droff.
// rec_cap < 0: whatever the count says.
int record_on_device(const char *who, Lane *L, int64_t n_reads, const int64_t *d_cigar_off, const uint32_t *d_cigar, const int32_t *d_pos,
                     const uint8_t *d_rc, const int64_t *d_seq_off, const int32_t *d_seq_len, const int32_t *d_map, const int32_t *d_flags,
                     int64_t seq_bytes, int64_t *rec_off, int64_t rec_cap, DevBuf &droff, DevBuf &drec, int64_t *n_rec)
{
    const hipStream_t cs = L->compute;
    DevBuf dnear(L);
    int rc;
    if ((rc = dnear.alloc((size_t)seq_bytes * 8 + 16)) || (rc = droff.alloc((size_t)(n_reads + 1) * 8))) return rc;
    if ((rc = abea_record_launch(GBX_ABEA_RECORD_COUNT, n_reads, d_cigar_off, d_cigar, d_pos, d_rc, d_seq_off, d_seq_len, d_map, d_flags,
                                 dnear.as<int32_t>(), droff.as<int64_t>(), nullptr, 0, cs)))
        return rc;
    int64_t total = 0;
    if (rec_off) GBX_HIP(hipMemcpyAsync(rec_off, droff.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, cs));
    else GBX_HIP(hipMemcpyAsync(&total, droff.as<int64_t>() + n_reads, 8, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipStreamSynchronize(cs));
    if (rec_off) total = rec_off[n_reads];
    *n_rec = total;
    if (rec_cap >= 0 && total > rec_cap) { set_error("%s: %lld record pairs, room for %lld", who, (long long)total, (long long)rec_cap); return GBX_ERR_ARG; }
    if ((rc = drec.alloc((size_t)std::max<int64_t>(total, 1) * sizeof(gbx_abea_pair)))) return rc;
    if (total == 0) return GBX_OK;
    rc = abea_record_launch(GBX_ABEA_RECORD_FILL, n_reads, d_cigar_off, d_cigar, d_pos, d_rc, d_seq_off, d_seq_len, d_map, d_flags, dnear.as<int32_t>(),
                            droff.as<int64_t>(), drec.as<gbx_abea_pair>(), total, cs);
    if (rc) return rc;
    GBX_HIP(hipStreamSynchronize(cs));                          // dnear dies with this scope
    return GBX_OK;
}

// the same, and the record to the host
int record_to_host(const char *who, Lane *L, int64_t n_reads, const int64_t *d_cigar_off, const uint32_t *d_cigar, const int32_t *d_pos,
                   const uint8_t *d_rc, const int64_t *d_seq_off, const int32_t *d_seq_len, const int32_t *d_map, const int32_t *d_flags,
                   int64_t seq_bytes, int64_t *rec_off, int64_t rec_cap, gbx_abea_pair *rec, int64_t *n_rec)
{
    DevBuf droff(L), drec(L);
    int rc = record_on_device(who, L, n_reads, d_cigar_off, d_cigar, d_pos, d_rc, d_seq_off, d_seq_len, d_map, d_flags, seq_bytes, rec_off, rec_cap, droff,
                              drec, n_rec);
    if (rc || *n_rec == 0) return rc;
    GBX_HIP(hipMemcpyAsync(rec, drec.p, (size_t)*n_rec * sizeof(gbx_abea_pair), hipMemcpyDeviceToHost, L->compute));
    GBX_HIP(hipStreamSynchronize(L->compute));
    return GBX_OK;
}

}  // namespace

extern "C" {

int gbx_abea_calib_device(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq_arena, const int64_t *d_event_off,
                          const float *d_event_mean, const gbx_abea_model *d_models, const gbx_abea_pair *d_pairs, const int32_t *d_n_pairs,
                          float *d_scale, float *d_shift, float *d_var, double *d_var64, int32_t *d_map, double *d_events_per_base,
                          int32_t *d_n_event_alignment, int32_t *d_n_m_state, int32_t *d_flags, void *stream)
{
    if (n_reads < 0) { set_error("gbx_abea_calib_device: bad argument"); return GBX_ERR_ARG; }
    if (n_reads == 0) return GBX_OK;
    if (!d_seq_off || !d_seq_len || !d_seq_arena || !d_event_off || !d_event_mean || !d_models || !d_pairs || !d_n_pairs || !d_scale || !d_shift ||
        !d_var || !d_var64 || !d_map || !d_events_per_base || !d_n_event_alignment || !d_n_m_state || !d_flags) {
        set_error("gbx_abea_calib_device: null pointer");
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_calib_launch(n_reads, d_seq_off, d_seq_len, d_seq_arena, d_event_off, d_event_mean, d_models, d_pairs, d_n_pairs, d_scale, d_shift, d_var,
                             d_var64, d_map, d_events_per_base, d_n_event_alignment, d_n_m_state, d_flags, (hipStream_t)stream);
}

int gbx_abea_calib_logvar_host(int64_t n_reads, const double *var64, const int32_t *n_m_state, float *log_var)
{
    if (n_reads < 0 || (n_reads > 0 && (!var64 || !n_m_state || !log_var))) { set_error("gbx_abea_calib_logvar_host: bad argument"); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n_reads; ++r) log_var[r] = n_m_state[r] >= 200 ? (float)log(var64[r]) : 0.0f;       /* align.c:749 */
    return GBX_OK;
}

int gbx_abea_calib_host(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                        const int64_t *event_off, const gbx_abea_event *events, const gbx_abea_model *models, const gbx_abea_pair *pairs,
                        const int32_t *n_pairs, float *scale, float *shift, float *var, float *log_var, double *var64, int32_t *map,
                        double *events_per_base, int32_t *n_event_alignment, int32_t *n_m_state, int32_t *flags)
{
    const char *who = "gbx_abea_calib_host";
    RoctxRange range_(who);
    if (n_reads < 0 || seq_bytes < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_reads == 0) return GBX_OK;
    if (!seq_off || !seq_len || !seq_arena || !event_off || !models || !n_pairs || !scale || !shift || !var || !log_var || !var64 || !map ||
        !events_per_base || !n_event_alignment || !n_m_state || !flags) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if (event_off[0] < 0) { set_error("%s: event_off below 0", who); return GBX_ERR_ARG; }
    if (event_off[n_reads] > event_off[0] && !events) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc;
    for (int64_t r = 0; r < n_reads; ++r) {
        if ((rc = read_check(seq_off, seq_len, seq_bytes, r, who)) || (rc = kmer_check(seq_len, r, who)) || (rc = event_off_check(event_off, r, who)) ||
            (rc = event_count_check(event_off, r, who)))
            return rc;
        const int64_t ne = event_off[r + 1] - event_off[r], nk = (int64_t)seq_len[r] - GBX_ABEA_KMER + 1;
        if (n_pairs[r] < 0 || n_pairs[r] > 2 * ne) { set_error("%s: read %lld: %d pairs, room for %lld", who, (long long)r, n_pairs[r], (long long)(2 * ne)); return GBX_ERR_ARG; }
        if (n_pairs[r] > 0 && !pairs) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
        const gbx_abea_pair *p = pairs + 2 * event_off[r];
        for (int32_t i = 0; i < n_pairs[r]; ++i) {
            if (p[i].ref_pos < 0 || p[i].ref_pos >= nk || p[i].read_pos < 0 || p[i].read_pos >= ne) {
                set_error("%s: read %lld: pair %d lies outside its k-mers or events", who, (long long)r, i);
                return GBX_ERR_ARG;
            }
            if (i > 0 && (p[i].ref_pos < p[i - 1].ref_pos || p[i].read_pos < p[i - 1].read_pos)) {
                set_error("%s: read %lld: pair %d lies below the pair before it", who, (long long)r, i);
                return GBX_ERR_ARG;
            }
        }
    }
    if ((rc = require_device())) return rc;
    const int64_t e0 = event_off[0], n_ev = event_off[n_reads] - e0;
    const std::vector<int64_t> eoff = rebased0(event_off, n_reads);
    const std::vector<float> means = event_means(events, e0, n_ev);                                            // only the mean is read (align.c:697)
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    const hipStream_t cs = L->compute;
    DevBuf dso(L), dsl(L), dsq(L), deo(L), dem(L), dmo(L), dpr(L), dnp(L), dsc(L), dsh(L), dvar(L), dv64(L), dmap(L), depb(L), dnea(L), dnm(L), dfl(L);
    if ((rc = dso.alloc(n_reads * 8)) || (rc = dsl.alloc(n_reads * 4)) || (rc = dsq.alloc((size_t)seq_bytes + 16)) || (rc = deo.alloc((n_reads + 1) * 8)) ||
        (rc = dem.alloc((size_t)n_ev * 4 + 16)) || (rc = dmo.alloc(GBX_ABEA_NMODEL * sizeof(gbx_abea_model))) ||
        (rc = dpr.alloc((size_t)n_ev * 2 * sizeof(gbx_abea_pair) + 16)) || (rc = dnp.alloc(n_reads * 4)) || (rc = dsc.alloc(n_reads * 4)) ||
        (rc = dsh.alloc(n_reads * 4)) || (rc = dvar.alloc(n_reads * 4)) || (rc = dv64.alloc(n_reads * 8)) || (rc = dmap.alloc((size_t)seq_bytes * 8 + 16)) ||
        (rc = depb.alloc(n_reads * 8)) || (rc = dnea.alloc(n_reads * 4)) || (rc = dnm.alloc(n_reads * 4)) || (rc = dfl.alloc(n_reads * 4)))
        return rc;
    GBX_HIP(hipMemcpyAsync(dso.p, seq_off, (size_t)n_reads * 8, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dsl.p, seq_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, cs));
    if (seq_bytes) GBX_HIP(hipMemcpyAsync(dsq.p, seq_arena, (size_t)seq_bytes, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(deo.p, eoff.data(), (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, cs));
    if (n_ev) GBX_HIP(hipMemcpyAsync(dem.p, means.data(), (size_t)n_ev * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dmo.p, models, GBX_ABEA_NMODEL * sizeof(gbx_abea_model), hipMemcpyHostToDevice, cs));
    if (n_ev && pairs) GBX_HIP(hipMemcpyAsync(dpr.p, pairs + 2 * e0, (size_t)n_ev * 2 * sizeof(gbx_abea_pair), hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dnp.p, n_pairs, (size_t)n_reads * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dsc.p, scale, (size_t)n_reads * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dsh.p, shift, (size_t)n_reads * 4, hipMemcpyHostToDevice, cs));
    if ((rc = abea_calib_launch(n_reads, dso.as<int64_t>(), dsl.as<int32_t>(), dsq.as<char>(), deo.as<int64_t>(), dem.as<float>(), dmo.as<gbx_abea_model>(),
                                dpr.as<gbx_abea_pair>(), dnp.as<int32_t>(), dsc.as<float>(), dsh.as<float>(), dvar.as<float>(), dv64.as<double>(),
                                dmap.as<int32_t>(), depb.as<double>(), dnea.as<int32_t>(), dnm.as<int32_t>(), dfl.as<int32_t>(), cs)))
        return rc;
    GBX_HIP(hipMemcpyAsync(scale, dsc.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(shift, dsh.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(var, dvar.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(var64, dv64.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(events_per_base, depb.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(n_event_alignment, dnea.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(n_m_state, dnm.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(flags, dfl.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    std::vector<int32_t> whole((size_t)seq_bytes * 2);
    if (seq_bytes) GBX_HIP(hipMemcpyAsync(whole.data(), dmap.p, (size_t)seq_bytes * 8, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipStreamSynchronize(cs));
    for (int64_t r = 0; r < n_reads; ++r)                                     // a read's entries only: the slots between reads are not written
        memcpy(map + 2 * seq_off[r], whole.data() + 2 * seq_off[r], ((size_t)seq_len[r] - GBX_ABEA_KMER + 1) * 8);
    return gbx_abea_calib_logvar_host(n_reads, var64, n_m_state, log_var);
}

int gbx_abea_event_record_device(int pass, int64_t n_reads, const int64_t *d_cigar_off, const uint32_t *d_cigar, const int32_t *d_pos, const uint8_t *d_rc,
                                 const int64_t *d_seq_off, const int32_t *d_seq_len, const int32_t *d_map, const int32_t *d_flags, int32_t *d_near,
                                 int64_t *d_rec_off, gbx_abea_pair *d_rec, int64_t rec_cap, void *stream)
{
    if (n_reads < 0 || rec_cap < 0 || pass < 1 || pass > (GBX_ABEA_RECORD_COUNT | GBX_ABEA_RECORD_FILL)) {
        set_error("gbx_abea_event_record_device: bad argument");
        return GBX_ERR_ARG;
    }
    if (n_reads == 0) return GBX_OK;
    if (!d_cigar_off || !d_cigar || !d_pos || !d_rc || !d_seq_off || !d_seq_len || !d_map || !d_near || !d_rec_off ||
        ((pass & GBX_ABEA_RECORD_FILL) && rec_cap > 0 && !d_rec)) {
        set_error("gbx_abea_event_record_device: null pointer");
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_record_launch(pass, n_reads, d_cigar_off, d_cigar, d_pos, d_rc, d_seq_off, d_seq_len, d_map, d_flags, d_near, d_rec_off, d_rec, rec_cap,
                              (hipStream_t)stream);
}

int gbx_abea_event_record_host(int64_t n_reads, const int64_t *cigar_off, const uint32_t *cigar, const int32_t *pos, const uint8_t *rc_flag,
                               const int64_t *seq_off, const int32_t *seq_len, int64_t seq_bytes, const int32_t *map, const int32_t *flags,
                               int64_t *rec_off, int64_t rec_cap, gbx_abea_pair *rec, int64_t *n_rec)
{
    const char *who = "gbx_abea_event_record_host";
    RoctxRange range_(who);
    if (n_reads < 0 || seq_bytes < 0 || rec_cap < 0 || !n_rec) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    *n_rec = 0;
    if (n_reads == 0) { if (rec_off) rec_off[0] = 0; return GBX_OK; }
    if (!cigar_off || !pos || !rc_flag || !seq_off || !seq_len || !map || !rec_off || (rec_cap > 0 && !rec)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc;
    for (int64_t r = 0; r < n_reads; ++r)
        if ((rc = read_check(seq_off, seq_len, seq_bytes, r, who))) return rc;
    if ((rc = check_cigars(who, n_reads, cigar_off, cigar, seq_len))) return rc;
    if ((rc = require_device())) return rc;
    const int64_t c0 = cigar_off[0], n_cig = cigar_off[n_reads] - c0;
    const std::vector<int64_t> coff = rebased0(cigar_off, n_reads);
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    const hipStream_t cs = L->compute;
    DevBuf dco(L), dcg(L), dpos(L), drc(L), dso(L), dsl(L), dmap(L), dfl(L);
    if ((rc = dco.alloc((n_reads + 1) * 8)) || (rc = dcg.alloc((size_t)n_cig * 4 + 16)) || (rc = dpos.alloc(n_reads * 4)) || (rc = drc.alloc(n_reads)) ||
        (rc = dso.alloc(n_reads * 8)) || (rc = dsl.alloc(n_reads * 4)) || (rc = dmap.alloc((size_t)seq_bytes * 8 + 16)) || (rc = dfl.alloc(n_reads * 4)))
        return rc;
    GBX_HIP(hipMemcpyAsync(dco.p, coff.data(), (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, cs));
    if (n_cig) GBX_HIP(hipMemcpyAsync(dcg.p, cigar + c0, (size_t)n_cig * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dpos.p, pos, (size_t)n_reads * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(drc.p, rc_flag, (size_t)n_reads, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dso.p, seq_off, (size_t)n_reads * 8, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dsl.p, seq_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, cs));
    if (seq_bytes) GBX_HIP(hipMemcpyAsync(dmap.p, map, (size_t)seq_bytes * 8, hipMemcpyHostToDevice, cs));
    if (flags) GBX_HIP(hipMemcpyAsync(dfl.p, flags, (size_t)n_reads * 4, hipMemcpyHostToDevice, cs));
    return record_to_host(who, L, n_reads, dco.as<int64_t>(), dcg.as<uint32_t>(), dpos.as<int32_t>(), drc.as<uint8_t>(), dso.as<int64_t>(),
                          dsl.as<int32_t>(), dmap.as<int32_t>(), flags ? dfl.as<int32_t>() : nullptr, seq_bytes, rec_off, rec_cap, rec, n_rec);
}

int gbx_abea_call_methylation_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range, const float *digitisation,
                                   const float *offset, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                                   const gbx_abea_model *models, const gbx_abea_model *cpg_model, const int64_t *cigar_off, const uint32_t *cigar,
                                   const int32_t *pos, const uint8_t *rc_flag, const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena,
                                   int32_t *flags, int32_t *status, float *scale, float *shift, float *var, double *events_per_base, int64_t site_cap,
                                   gbx_abea_meth_site *sites, float *scores, int64_t *n_sites)
{
    const char *who = "gbx_abea_call_methylation_host";
    RoctxRange range_(who);
    if (n_reads < 0 || seq_bytes < 0 || site_cap < 0 || !n_sites) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    *n_sites = 0;
    if (n_reads == 0) return GBX_OK;
    if (!seq_len || !cpg_model || !cigar_off || !pos || !rc_flag || !ref_off || !ref_len || !ref_arena || !flags || !status || !scale || !shift || !var ||
        !events_per_base || (site_cap > 0 && (!sites || !scores))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc;
    for (int64_t r = 0; r < n_reads; ++r)
        if ((rc = ref_segment_check(ref_off, ref_len, r, who))) return rc;
    if ((rc = check_cigars(who, n_reads, cigar_off, cigar, seq_len))) return rc;
    // a batch in which no read has events never reaches the tail
    for (int64_t r = 0; r < n_reads; ++r) { flags[r] = GBX_ABEA_FAILED_ALIGNMENT; var[r] = 0.0f; events_per_base[r] = 0.0; }
    // behind align(), on the buffers it left: calibration, record, the site planner, the order and the score.  The record, the jobs
    // and the strings never leave the device; the site table and the scores come down.
    const abea_tail_fn call_meth_tail = [&](const AbeaAligned &a) -> int {
        Lane *L = a.L;
        const hipStream_t cs = L->compute;
        const int64_t n = a.n_reads;
        std::vector<uint8_t> bad((size_t)n);
        std::vector<float> flogsum(GBX_ABEA_FLOGSUM_TBL), trans((size_t)n * GBX_ABEA_METH_NTRANS), pre, post;
        int64_t totals[2] = {0, 0}, tail[GBX_ABEA_METH_NCLASS + 2];
        gbx_abea_meth_job bad_job;
        AbeaCalibrated cal(L);                                   // behind every host array a queued copy uses: it drains the stream before they die
        if ((rc = cal.queue(a, cigar_off, cigar, pos, rc_flag, scale, shift, var, events_per_base, flags))) return rc;
        // the record of the unflagged reads (the flags are on the device; the count pass is queued behind the calibration)
        int64_t n_rec = 0;
        DevBuf droff(L), drec(L);
        if ((rc = record_on_device(who, L, n, cal.cigar_off, cal.cigar, cal.pos, cal.rc, a.d_seq_off, a.d_seq_len, cal.map, cal.flags, a.seq_bytes, nullptr, -1,
                                   droff, drec, &n_rec)))
            return rc;
        if ((rc = cal.finish(nullptr))) return rc;
        // the reference segments go up; planner COUNT; the two totals and the strand flags come down
        int64_t ref_bytes = 0, flank_len = 2;
        for (int64_t r = 0; r < n; ++r) {
            ref_bytes = std::max<int64_t>(ref_bytes, ref_off[r] + ref_len[r]);
            flank_len = std::max<int64_t>(flank_len, a.event_off[r + 1] - a.event_off[r] + 1);      // a job's rows are events of one read
        }
        int bits = 1;
        while (bits < 30 && (1ll << bits) < flank_len) bits++;
        Carve per_read(L);
        DevBuf dref(L);
        const size_t sites_work = abea_meth_sites_work_bytes(n);
        for (size_t b : {(size_t)n * 8, (size_t)n * 4, (size_t)(n + 1) * 8, (size_t)(n + 1) * 8, (size_t)n, sites_work, sizeof tail}) per_read.want(b);
        if ((rc = per_read.alloc()) || (rc = dref.alloc((size_t)ref_bytes + 16))) return rc;
        int64_t *d_ref_off = per_read.take<int64_t>((size_t)n * 8);
        int32_t *d_ref_len = per_read.take<int32_t>((size_t)n * 4);
        int64_t *d_site_off = per_read.take<int64_t>((size_t)(n + 1) * 8), *d_byte_off = per_read.take<int64_t>((size_t)(n + 1) * 8);
        uint8_t *d_bad = per_read.take<uint8_t>((size_t)n);
        void *d_swork = per_read.take<char>(sites_work);
        int64_t *d_tail = per_read.take<int64_t>(sizeof tail);                                       // class_off, then first_bad
        GBX_HIP(hipMemcpyAsync(d_ref_off, ref_off, (size_t)n * 8, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(d_ref_len, ref_len, (size_t)n * 4, hipMemcpyHostToDevice, cs));
        if (ref_bytes) GBX_HIP(hipMemcpyAsync(dref.p, ref_arena, (size_t)ref_bytes, hipMemcpyHostToDevice, cs));
        if ((rc = abea_meth_sites_launch(GBX_ABEA_METH_SITES_COUNT, n, d_ref_off, d_ref_len, dref.as<char>(), cal.pos, cal.rc, droff.as<int64_t>(),
                                         drec.as<gbx_abea_pair>(), d_swork, d_site_off, d_byte_off, d_bad, 0, nullptr, nullptr, 0, nullptr, cs)))
            return rc;
        GBX_HIP(hipMemcpyAsync(&totals[0], d_site_off + n, 8, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(&totals[1], d_byte_off + n, 8, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(bad.data(), d_bad, (size_t)n, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipStreamSynchronize(cs));
        for (int64_t r = 0; r < n; ++r)
            if (bad[(size_t)r]) { set_error("gbx_abea_meth_sites_host: the record of read %lld runs against its strand", (long long)r); return GBX_ERR_ARG; }
        const int64_t ns = totals[0], nb = totals[1];
        *n_sites = ns;
        if (ns > site_cap) { set_error("%s: %lld sites, room for %lld", who, (long long)ns, (long long)site_cap); return GBX_ERR_ARG; }
        if (ns == 0) return GBX_OK;
        const int64_t n_jobs = 2 * ns;
        if (n_jobs > 0x7fffffffLL - 1024) { set_error("gbx_abea_meth_plan_host: more than 2^31 jobs in one call"); return GBX_ERR_UNSUPPORTED; }
        // the tables that need the host C library, planner FILL, the order and its checks
        pre.resize((size_t)flank_len); post.resize((size_t)flank_len);
        if ((rc = gbx_abea_meth_tables_host(n, events_per_base, flogsum.data(), trans.data(), flank_len, pre.data(), post.data()))) return rc;
        DevBuf dst(L), djb(L), dsq(L), dor(L), dout(L), dow(L);
        Carve tables(L);
        const size_t job_bytes = (size_t)n_jobs * sizeof(gbx_abea_meth_job), model_bytes = GBX_ABEA_NMODEL_CPG * sizeof(gbx_abea_model);
        const size_t flank_bytes = (size_t)flank_len * 4, site_bytes = (size_t)ns * sizeof(gbx_abea_meth_site);
        for (size_t b : {model_bytes, (size_t)GBX_ABEA_FLOGSUM_TBL * 4, trans.size() * 4, flank_bytes, flank_bytes}) tables.want(b);
        if ((rc = dst.alloc(site_bytes)) || (rc = djb.alloc(job_bytes)) || (rc = dsq.alloc((size_t)nb + 16)) || (rc = tables.alloc()) ||
            (rc = dor.alloc((size_t)n_jobs * 4)) || (rc = dout.alloc((size_t)n_jobs * 4)) || (rc = dow.alloc(abea_meth_order_work_bytes(n_jobs))))
            return rc;
        gbx_abea_model *dmo = tables.take<gbx_abea_model>(model_bytes);
        float *dflg = tables.take<float>(GBX_ABEA_FLOGSUM_TBL * 4), *dtr = tables.take<float>(trans.size() * 4);
        float *dpr = tables.take<float>(flank_bytes), *dpo = tables.take<float>(flank_bytes);
        GBX_HIP(hipMemcpyAsync(dmo, cpg_model, model_bytes, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(dflg, flogsum.data(), GBX_ABEA_FLOGSUM_TBL * 4, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(dtr, trans.data(), trans.size() * 4, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(dpr, pre.data(), flank_bytes, hipMemcpyHostToDevice, cs));
        GBX_HIP(hipMemcpyAsync(dpo, post.data(), flank_bytes, hipMemcpyHostToDevice, cs));
        if ((rc = abea_meth_sites_launch(GBX_ABEA_METH_SITES_FILL, n, d_ref_off, d_ref_len, dref.as<char>(), cal.pos, cal.rc, droff.as<int64_t>(),
                                         drec.as<gbx_abea_pair>(), d_swork, d_site_off, d_byte_off, d_bad, ns, dst.as<gbx_abea_meth_site>(),
                                         djb.as<gbx_abea_meth_job>(), nb, dsq.as<char>(), cs)))
            return rc;
        if ((rc = abea_meth_order_launch(n_jobs, djb.as<gbx_abea_meth_job>(), nb, n, a.d_event_off, flank_len, bits, dow.p, dor.as<int32_t>(), d_tail,
                                         d_tail + GBX_ABEA_METH_NCLASS + 1, cs)))
            return rc;
        GBX_HIP(hipMemcpyAsync(tail, d_tail, sizeof tail, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipStreamSynchronize(cs));
        const int64_t first_bad = tail[GBX_ABEA_METH_NCLASS + 1];
        if (first_bad != INT64_MAX) {                            // the score indexes events with what the jobs say: it is not launched
            if (first_bad < 0 || first_bad >= n_jobs) { set_error("%s: the order stage names job %lld of %lld", who, (long long)first_bad, (long long)n_jobs); return GBX_ERR_HIP; }
            GBX_HIP(hipMemcpyAsync(&bad_job, djb.as<gbx_abea_meth_job>() + first_bad, sizeof bad_job, hipMemcpyDeviceToHost, cs));
            GBX_HIP(hipStreamSynchronize(cs));
            if ((rc = abea_meth_job_refuse(first_bad, bad_job, nb, n, a.event_off, flank_len))) return rc;
            set_error("%s: the order stage refuses job %lld, the host check does not", who, (long long)first_bad);
            return GBX_ERR_HIP;
        }
        if ((rc = abea_meth_launch(n_jobs, djb.as<gbx_abea_meth_job>(), dsq.as<char>(), a.d_event_off, a.d_event_mean, a.d_scale, a.d_shift, cal.var, cal.log_var,
                                   dmo, dflg, dtr, dpr, dpo, dor.as<int32_t>(), tail, dout.as<float>(), cs)))
            return rc;
        GBX_HIP(hipMemcpyAsync(sites, dst.p, site_bytes, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipMemcpyAsync(scores, dout.p, (size_t)n_jobs * 4, hipMemcpyDeviceToHost, cs));
        GBX_HIP(hipStreamSynchronize(cs));
        return GBX_OK;
    };
    return abea_signal_align_tail(who, n_reads, raw, raw_off, range, digitisation, offset, seq_off, seq_len, seq_arena, seq_bytes, models, status, scale,
                                  shift, call_meth_tail);
}

}  // extern "C"
