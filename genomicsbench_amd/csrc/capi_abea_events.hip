// capi_abea_events.hip — abea from raw signal: the event detection, scalings and chained entries of the C-ABI (include/gbx.h).
#include "capi_common.h"

using namespace gbx;

// One device (the calling thread's current one): detection, and with `align` the scalings and align() behind it.
static int abea_signal_host(const char *who, bool align, int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range,
                            const float *digitisation, const float *offset, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena,
                            int64_t seq_bytes, const gbx_abea_model *models, int64_t *n_events, int64_t *event_off, gbx_abea_event *events,
                            int64_t event_cap, int64_t *n_events_total, float *scale, float *shift, int32_t *status, gbx_abea_pair *out,
                            int32_t *n_pairs, const abea_tail_fn &tail = nullptr)
{
    RoctxRange range_(who);
    if (n_reads < 0 || event_cap < 0 || (align && seq_bytes < 0)) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_events_total) *n_events_total = 0;
    if (n_reads == 0) { if (event_off) event_off[0] = 0; return GBX_OK; }
    if (!raw || !raw_off || !range || !digitisation || !offset || !event_off || (!events && event_cap > 0) || !n_events_total || !status ||
        (align && (!seq_off || !seq_len || !seq_arena || !models || !scale || !shift || (!out && !tail) || !n_pairs))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (raw_off[r] < 0 || raw_off[r + 1] < raw_off[r]) { set_error("%s: raw_off not monotone at read %lld", who, (long long)r); return GBX_ERR_ARG; }
        if (raw_off[r + 1] - raw_off[r] > 0x3fffffff) { set_error("%s: read %lld is too long", who, (long long)r); return GBX_ERR_UNSUPPORTED; }
        if (!align) continue;
        if ((rc = read_check(seq_off, seq_len, seq_bytes, r, who)) || (rc = kmer_check(seq_len, r, who))) return rc;
    }
    if ((rc = require_device())) return rc;
    const int64_t s0 = raw_off[0], n_samples = raw_off[n_reads] - s0;
    const std::vector<int64_t> roff = rebased0(raw_off, n_reads);
    std::vector<int64_t> nev_own;
    if (!n_events) { nev_own.resize((size_t)n_reads); n_events = nev_own.data(); }

    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    const hipStream_t cs = L->compute;
    DevBuf draw(L), dro(L), drg(L), ddg(L), dof(L), dne(L), deo(L), dst(L), dev(L), dem(L);                     // detection
    DevBuf dso(L), dsl(L), dsq(L), dmo(L), dsc(L), dsh(L);                                                        // scalings
    DevBuf dcso(L), dcsl(L), dceo(L), dcsc(L), dcsh(L), dbo(L), dor(L), dlp(L), dout(L), dnp(L), dw(L), dpre(L);  // align
    if ((rc = draw.alloc((size_t)n_samples * 2)) || (rc = dro.alloc((n_reads + 1) * 8)) || (rc = drg.alloc(n_reads * 4)) || (rc = ddg.alloc(n_reads * 4)) ||
        (rc = dof.alloc(n_reads * 4)) || (rc = dne.alloc(n_reads * 8)) || (rc = deo.alloc((n_reads + 1) * 8)) || (rc = dst.alloc(n_reads * 4)))
        return rc;
    if (align && ((rc = dso.alloc(n_reads * 8)) || (rc = dsl.alloc(n_reads * 4)) || (rc = dsq.alloc((size_t)seq_bytes)) ||
                  (rc = dmo.alloc(GBX_ABEA_NMODEL * sizeof(gbx_abea_model))) || (rc = dsc.alloc(n_reads * 4)) || (rc = dsh.alloc(n_reads * 4))))
        return rc;
    HostPipe pipe(L, (size_t)n_samples * 2 + (align ? (size_t)seq_bytes : 0) + (size_t)n_reads * 32, false);
    if ((rc = pipe.prepare(1))) return rc;
#define EV_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return pipe.finish(hip_fail(e_, #call)); } while (0)
    if (n_samples) pipe.stage(0, draw.p, raw + s0, (size_t)n_samples * 2);
    pipe.stage(0, dro.p, roff.data(), (n_reads + 1) * 8);
    pipe.stage(0, drg.p, range, n_reads * 4); pipe.stage(0, ddg.p, digitisation, n_reads * 4); pipe.stage(0, dof.p, offset, n_reads * 4);
    if (align) {
        pipe.stage(0, dso.p, seq_off, n_reads * 8); pipe.stage(0, dsl.p, seq_len, n_reads * 4);
        if (seq_bytes) pipe.stage(0, dsq.p, seq_arena, (size_t)seq_bytes);
        pipe.stage(0, dmo.p, models, GBX_ABEA_NMODEL * sizeof(gbx_abea_model));
    }
    pipe.start();
    if ((rc = pipe.wait_stage(0))) return pipe.finish(rc);
    if ((rc = abea_events_launch(GBX_ABEA_EVENTS_COUNT, n_reads, draw.as<int16_t>(), dro.as<int64_t>(), drg.as<float>(), ddg.as<float>(), dof.as<float>(),
                                 dne.as<int64_t>(), deo.as<int64_t>(), nullptr, nullptr, 0, dst.as<int32_t>(), cs)))
        return pipe.finish(rc);
    if ((rc = pipe.chunk_launched(0))) return pipe.finish(rc);
    // the event counts come back (8 bytes per read): the caller's arrays and align's band plan are sized by them
    EV_HIP(hipMemcpyAsync(n_events, dne.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, cs));
    EV_HIP(hipMemcpyAsync(status, dst.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    EV_HIP(hipStreamSynchronize(cs));
    event_off[0] = 0;
    for (int64_t r = 0; r < n_reads; ++r) event_off[r + 1] = event_off[r] + n_events[r];
    const int64_t total = event_off[n_reads];
    *n_events_total = total;
    if (total > event_cap && !tail) {                                         // with a tail the records stay on the device
        set_error("%s: %lld events, room for %lld", who, (long long)total, (long long)event_cap);
        return pipe.finish(GBX_ERR_ARG);
    }
    if ((rc = dev.alloc((size_t)total * sizeof(gbx_abea_event))) || (rc = dem.alloc((size_t)total * 4 + 16))) return pipe.finish(rc);
    if ((rc = abea_events_launch(GBX_ABEA_EVENTS_FILL, n_reads, draw.as<int16_t>(), dro.as<int64_t>(), drg.as<float>(), ddg.as<float>(), dof.as<float>(),
                                 dne.as<int64_t>(), deo.as<int64_t>(), dev.as<gbx_abea_event>(), dem.as<float>(), total, dst.as<int32_t>(), cs)))
        return pipe.finish(rc);
    if (total && !tail) EV_HIP(hipMemcpyAsync(events, dev.p, (size_t)total * sizeof(gbx_abea_event), hipMemcpyDeviceToHost, cs));
    if (!align) {
        EV_HIP(hipStreamSynchronize(cs));
        return pipe.finish();
    }
    if ((rc = abea_scalings_launch(n_reads, dso.as<int64_t>(), dsl.as<int32_t>(), dsq.as<char>(), deo.as<int64_t>(), dem.as<float>(),
                                   dmo.as<gbx_abea_model>(), dsc.as<float>(), dsh.as<float>(), cs)))
        return pipe.finish(rc);
    EV_HIP(hipMemcpyAsync(scale, dsc.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    EV_HIP(hipMemcpyAsync(shift, dsh.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, cs));
    EV_HIP(hipStreamSynchronize(cs));
    // align() takes the reads that have events; a read without any reports no pairs.  Reads without events take no room in
    // the event array, so the kept reads' offsets (absolute indexing) still delimit their events.
    std::vector<int64_t> keep, cso, ceo;
    std::vector<int32_t> csl;
    std::vector<float> csc, csh;
    int64_t n_kmers_total = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        n_pairs[r] = 0;
        if (n_events[r] < 1) continue;
        keep.push_back(r); cso.push_back(seq_off[r]); csl.push_back(seq_len[r]); ceo.push_back(event_off[r]);
        csc.push_back(scale[r]); csh.push_back(shift[r]);
        n_kmers_total += (int64_t)seq_len[r] - GBX_ABEA_KMER + 1;
    }
    const int64_t m = (int64_t)keep.size();
    if (m == 0) return pipe.finish();
    ceo.push_back(total);
    std::vector<int64_t> band_off((size_t)m + 1), prefix((size_t)m + 1);
    std::vector<int32_t> order((size_t)m), cnp((size_t)m);
    std::vector<double> lp((size_t)m * 2);
    if ((rc = gbx_abea_plan_host(m, csl.data(), ceo.data(), band_off.data(), order.data(), lp.data()))) return pipe.finish(rc);
    const size_t wb = abea_workspace_bytes(m, n_kmers_total, band_off[(size_t)m]);
    if ((rc = dcso.alloc(m * 8)) || (rc = dcsl.alloc(m * 4)) || (rc = dceo.alloc((m + 1) * 8)) || (rc = dcsc.alloc(m * 4)) || (rc = dcsh.alloc(m * 4)) ||
        (rc = dbo.alloc((m + 1) * 8)) || (rc = dor.alloc(m * 4)) || (rc = dlp.alloc(m * 16)) || (rc = dout.alloc((size_t)total * 2 * sizeof(gbx_abea_pair) + 16)) ||
        (rc = dnp.alloc(m * 4)) || (rc = dw.alloc(wb)) || (rc = dpre.alloc((m + 1) * 8)))
        return pipe.finish(rc);
    EV_HIP(hipMemcpyAsync(dcso.p, cso.data(), (size_t)m * 8, hipMemcpyHostToDevice, cs));
    EV_HIP(hipMemcpyAsync(dcsl.p, csl.data(), (size_t)m * 4, hipMemcpyHostToDevice, cs));
    EV_HIP(hipMemcpyAsync(dceo.p, ceo.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, cs));
    EV_HIP(hipMemcpyAsync(dcsc.p, csc.data(), (size_t)m * 4, hipMemcpyHostToDevice, cs));
    EV_HIP(hipMemcpyAsync(dcsh.p, csh.data(), (size_t)m * 4, hipMemcpyHostToDevice, cs));
    EV_HIP(hipMemcpyAsync(dbo.p, band_off.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, cs));
    EV_HIP(hipMemcpyAsync(dor.p, order.data(), (size_t)m * 4, hipMemcpyHostToDevice, cs));
    EV_HIP(hipMemcpyAsync(dlp.p, lp.data(), (size_t)m * 16, hipMemcpyHostToDevice, cs));
    if ((rc = abea_launch(m, dcso.as<int64_t>(), dcsl.as<int32_t>(), dsq.as<char>(), dceo.as<int64_t>(), dem.as<float>(), dmo.as<gbx_abea_model>(),
                          dcsc.as<float>(), dcsh.as<float>(), dbo.as<int64_t>(), dor.as<int32_t>(), dlp.as<double>(), n_kmers_total,
                          band_off[(size_t)m], dout.as<gbx_abea_pair>(), dnp.as<int32_t>(), dw.p, wb, cs)))
        return pipe.finish(rc);
    EV_HIP(hipMemcpyAsync(cnp.data(), dnp.p, (size_t)m * 4, hipMemcpyDeviceToHost, cs));
    EV_HIP(hipStreamSynchronize(cs));
    if (tail) {
        for (int64_t k = 0; k < m; ++k) n_pairs[keep[(size_t)k]] = cnp[(size_t)k];
        const AbeaAligned a{L, n_reads, seq_bytes, event_off, n_pairs, dso.as<int64_t>(), dsl.as<int32_t>(), dsq.as<char>(), deo.as<int64_t>(),
                            dem.as<float>(), dmo.as<gbx_abea_model>(), dsc.as<float>(), dsh.as<float>(), dout.as<gbx_abea_pair>(), dev.as<gbx_abea_event>()};
        return pipe.finish(tail(a));
    }
    // half of the 2 x n_events slots are slack: the pairs are packed on the device, come back in one piece and go to
    // the reads' places from there
    int64_t tot = 0;
    for (int64_t k = 0; k < m; ++k) { prefix[(size_t)k] = tot; tot += cnp[(size_t)k] > 0 ? cnp[(size_t)k] : 0; }
    prefix[(size_t)m] = tot;
    if (tot) {
        gbx_abea_pair *packed = nullptr;
        EV_HIP(hipMemcpyAsync(dpre.p, prefix.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, cs));
        if ((rc = abea_pack_pairs(m, dceo.as<int64_t>(), dout.as<gbx_abea_pair>(), dnp.as<int32_t>(), dpre.as<int64_t>(), dw.p, n_kmers_total, &packed, cs)))
            return pipe.finish(rc);
        std::vector<gbx_abea_pair> flat((size_t)tot);
        EV_HIP(hipMemcpyAsync(flat.data(), packed, (size_t)tot * sizeof(gbx_abea_pair), hipMemcpyDeviceToHost, cs));
        EV_HIP(hipStreamSynchronize(cs));
        parallel_ranges(m, host_workers(), [&](int, int64_t lo, int64_t hi) {
            for (int64_t k = lo; k < hi; ++k)
                if (cnp[(size_t)k] > 0)
                    memcpy(out + 2 * ceo[(size_t)k], flat.data() + prefix[(size_t)k], (size_t)cnp[(size_t)k] * sizeof(gbx_abea_pair));
        });
    }
    for (int64_t k = 0; k < m; ++k) n_pairs[keep[(size_t)k]] = cnp[(size_t)k];
    return pipe.finish();
#undef EV_HIP
}

namespace gbx {
int abea_signal_align_tail(const char *who, int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range, const float *digitisation,
                           const float *offset, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                           const gbx_abea_model *models, int32_t *status, float *scale, float *shift, const abea_tail_fn &tail)
{
    std::vector<int64_t> event_off((size_t)(n_reads > 0 ? n_reads : 0) + 1);
    std::vector<int32_t> n_pairs((size_t)(n_reads > 0 ? n_reads : 0) + 1);
    int64_t total = 0;
    return abea_signal_host(who, true, n_reads, raw, raw_off, range, digitisation, offset, seq_off, seq_len, seq_arena, seq_bytes, models, nullptr,
                            event_off.data(), nullptr, 0, &total, scale, shift, status, nullptr, n_pairs.data(), tail);
}
}  // namespace gbx

extern "C" {

int gbx_abea_events_device(int pass, int64_t n_reads, const int16_t *d_raw, const int64_t *d_raw_off, const float *d_range,
                           const float *d_digitisation, const float *d_offset, int64_t *d_n_events, int64_t *d_event_off,
                           gbx_abea_event *d_events, float *d_event_mean, int64_t event_cap, int32_t *d_status, void *stream)
{
    if (n_reads < 0 || event_cap < 0 || pass < 1 || pass > (GBX_ABEA_EVENTS_COUNT | GBX_ABEA_EVENTS_FILL)) {
        set_error("gbx_abea_events_device: bad argument");
        return GBX_ERR_ARG;
    }
    if (n_reads == 0) return GBX_OK;
    if (!d_raw || !d_raw_off || !d_range || !d_digitisation || !d_offset || !d_n_events || !d_event_off || !d_status ||
        ((pass & GBX_ABEA_EVENTS_FILL) && (!d_events || !d_event_mean))) {
        set_error("gbx_abea_events_device: null pointer");
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_events_launch(pass, n_reads, d_raw, d_raw_off, d_range, d_digitisation, d_offset, d_n_events, d_event_off, d_events, d_event_mean,
                              event_cap, d_status, (hipStream_t)stream);
}

int gbx_abea_scalings_device(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq_arena,
                             const int64_t *d_event_off, const float *d_event_mean, const gbx_abea_model *d_models,
                             float *d_scale, float *d_shift, void *stream)
{
    if (n_reads < 0) { set_error("gbx_abea_scalings_device: bad argument"); return GBX_ERR_ARG; }
    if (n_reads == 0) return GBX_OK;
    if (!d_seq_off || !d_seq_len || !d_seq_arena || !d_event_off || !d_event_mean || !d_models || !d_scale || !d_shift) {
        set_error("gbx_abea_scalings_device: null pointer");
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_scalings_launch(n_reads, d_seq_off, d_seq_len, d_seq_arena, d_event_off, d_event_mean, d_models, d_scale, d_shift, (hipStream_t)stream);
}

int gbx_abea_events_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range,
                         const float *digitisation, const float *offset, int64_t *n_events, int64_t *event_off,
                         gbx_abea_event *events, int64_t event_cap, int64_t *n_events_total, int32_t *status)
{
    return abea_signal_host("gbx_abea_events_host", false, n_reads, raw, raw_off, range, digitisation, offset, nullptr, nullptr, nullptr, 0, nullptr,
                            n_events, event_off, events, event_cap, n_events_total, nullptr, nullptr, status, nullptr, nullptr);
}

int gbx_abea_signal_align_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range,
                               const float *digitisation, const float *offset, const int64_t *seq_off, const int32_t *seq_len,
                               const char *seq_arena, int64_t seq_bytes, const gbx_abea_model *models, int64_t *event_off,
                               gbx_abea_event *events, int64_t event_cap, int64_t *n_events_total, float *scale, float *shift,
                               int32_t *status, gbx_abea_pair *out, int32_t *n_pairs)
{
    return abea_signal_host("gbx_abea_signal_align_host", true, n_reads, raw, raw_off, range, digitisation, offset, seq_off, seq_len, seq_arena, seq_bytes,
                            models, nullptr, event_off, events, event_cap, n_events_total, scale, shift, status, out, n_pairs);
}

}  // extern "C"
