// capi_abea_eventalign.hip — f5c eventalign behind the calibration: the device and host entries of realign_read, the summary and
// TSV emitters (host only) and eventalign from raw signal in one call (include/gbx.h).
#include "capi_common.h"

using namespace gbx;

namespace {

// toupper and disambiguate (eventalign.c:1054-1109, 1294): the lowest base of an IUPAC code; -1 where the reference asserts
int ea_host_rank(char c)
{
    if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    switch (c) {
    case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 0;
    case 'C': case 'S': case 'Y': case 'B': return 1;
    case 'G': case 'K': return 2;
    case 'T': return 3;
    default: return -1;
    }
}

// ref_kmer and model_kmer of a record (eventalign.c:1474-1503) and the rank of model_kmer (get_kmer_rank: N ranks as A);
// false when the six bases do not lie inside the reference segment
bool ea_kmers(const char *ref, int32_t ref_len, int32_t pos, int rc, const gbx_abea_eventalign_rec &q, char *ref_kmer, char *model_kmer, uint32_t *rank)
{
    const int64_t s = (int64_t)q.ref_pos - pos;
    if (s < 0 || s + GBX_ABEA_KMER > ref_len) return false;
    int rk[GBX_ABEA_KMER];
    for (int i = 0; i < GBX_ABEA_KMER; ++i) { rk[i] = std::max(ea_host_rank(ref[s + i]), 0); ref_kmer[i] = "ACGT"[rk[i]]; }
    uint32_t r = 0;
    for (int i = 0; i < GBX_ABEA_KMER; ++i) {
        const int b = q.state == 'B' ? -1 : rc ? 3 - rk[GBX_ABEA_KMER - 1 - i] : rk[i];
        model_kmer[i] = b < 0 ? 'N' : "ACGT"[b];
        r = r << 2 | (uint32_t)std::max(b, 0);
    }
    ref_kmer[GBX_ABEA_KMER] = model_kmer[GBX_ABEA_KMER] = 0;
    *rank = r;
    return true;
}

// What both host paths share once the reads, the calibration and the CIGARs are on the device: the near table (the record's
// count pass), the transitions and the order from the host, the reference segments up, the kernel, the records down.
// event_off: host, absolute into d_event_mean as d_event_off; rec receives event_off[n] - event_off[0] records.
struct EaOnDevice {
    const int64_t *d_seq_off; const int32_t *d_seq_len; const int64_t *d_event_off; const float *d_event_mean; const gbx_abea_model *d_models;
    const float *d_scale, *d_shift, *d_var, *d_log_var; const int32_t *d_map, *d_flags;
    const int64_t *d_cigar_off; const uint32_t *d_cigar; const int32_t *d_pos; const uint8_t *d_rc;
};

int eventalign_on_lane(Lane *L, int64_t n, int64_t seq_bytes, const EaOnDevice &d, const int64_t *event_off, const double *events_per_base,
                       int64_t n_cig, const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena, int32_t region_start, int32_t region_end,
                       gbx_abea_eventalign_rec *rec, int32_t *n_rec, int32_t *status)
{
    const hipStream_t cs = L->compute;
    const int64_t e0 = event_off[0], n_ev = event_off[n] - e0;
    int rc;
    std::vector<float> trans((size_t)n * GBX_ABEA_METH_NTRANS);
    std::vector<int32_t> order((size_t)n);
    std::vector<int64_t> roff((size_t)n);
    std::vector<char> refs;
    if ((rc = gbx_abea_eventalign_trans_host(n, events_per_base, trans.data()))) return rc;
    for (int64_t r = 0; r < n; ++r) order[(size_t)r] = (int32_t)r;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return event_off[a + 1] - event_off[a] > event_off[b + 1] - event_off[b]; });
    for (int64_t r = 0; r < n; ++r) {
        roff[(size_t)r] = (int64_t)refs.size();
        refs.insert(refs.end(), ref_arena + ref_off[r], ref_arena + ref_off[r] + ref_len[r]);
    }
    const size_t wb = abea_eventalign_workspace_bytes(n, n_cig, GBX_ABEA_EVENTALIGN_ROWS);
    DevBuf dnear(L), dref(L), dw(L), drec(L);
    Carve small(L);
    for (size_t b : {trans.size() * 4, (size_t)n * 4, (size_t)n * 8, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)(n + 1) * 8}) small.want(b);
    if ((rc = small.alloc()) || (rc = dnear.alloc((size_t)seq_bytes * 8 + 16)) || (rc = dref.alloc(refs.size() + 16)) || (rc = dw.alloc(wb)) ||
        (rc = drec.alloc((size_t)n_ev * sizeof(gbx_abea_eventalign_rec) + 16)))
        return rc;
    float *dtr = small.take<float>(trans.size() * 4);
    int32_t *dord = small.take<int32_t>(n * 4);
    int64_t *droff = small.take<int64_t>(n * 8);
    int32_t *drl = small.take<int32_t>(n * 4), *dnr = small.take<int32_t>(n * 4), *dst = small.take<int32_t>(n * 4);
    int64_t *drecoff = small.take<int64_t>((n + 1) * 8);
    StreamDrain drain{cs};                                                      // the host vectors above outlive the queued copies
    GBX_HIP(hipMemcpyAsync(dtr, trans.data(), trans.size() * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dord, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(droff, roff.data(), (size_t)n * 8, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(drl, ref_len, (size_t)n * 4, hipMemcpyHostToDevice, cs));
    if (!refs.empty()) GBX_HIP(hipMemcpyAsync(dref.p, refs.data(), refs.size(), hipMemcpyHostToDevice, cs));
    if ((rc = abea_record_launch(GBX_ABEA_RECORD_COUNT, n, d.d_cigar_off, d.d_cigar, d.d_pos, d.d_rc, d.d_seq_off, d.d_seq_len, d.d_map, d.d_flags,
                                 dnear.as<int32_t>(), drecoff, nullptr, 0, cs)))
        return rc;
    // the kernel indexes records as it indexes events: absolutely
    const AbeaEventalignArgs a = abea_eventalign_args(n, d.d_seq_off, d.d_seq_len, d.d_event_off, d.d_event_mean, d.d_models, d.d_scale, d.d_shift, d.d_var,
                                                      d.d_log_var, dtr, d.d_map, dnear.as<int32_t>(), d.d_flags, d.d_cigar_off, d.d_cigar, d.d_pos, d.d_rc, droff,
                                                      drl, dref.as<char>(), region_start, region_end, dord, drec.as<gbx_abea_eventalign_rec>() - e0, dnr, dst,
                                                      nullptr, n_cig, GBX_ABEA_EVENTALIGN_ROWS, dw.p);
    if ((rc = abea_eventalign_launch(a, wb, cs))) return rc;
    GBX_HIP(hipMemcpyAsync(n_rec, dnr, (size_t)n * 4, hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipMemcpyAsync(status, dst, (size_t)n * 4, hipMemcpyDeviceToHost, cs));
    if (n_ev) GBX_HIP(hipMemcpyAsync(rec, drec.p, (size_t)n_ev * sizeof(gbx_abea_eventalign_rec), hipMemcpyDeviceToHost, cs));
    GBX_HIP(hipStreamSynchronize(cs));
    return GBX_OK;
}

// the checks of the reference segments and the region shared by the host entry and the one call
int check_refs(const char *who, int64_t n_reads, const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena, int32_t region_start, int32_t region_end)
{
    if (!((region_start == -1 && region_end == -1) || region_start <= region_end)) {          // eventalign.c:1275
        set_error("%s: region %d .. %d", who, region_start, region_end);
        return GBX_ERR_ARG;
    }
    for (int64_t r = 0; r < n_reads; ++r) {
        if (int rc = ref_segment_check(ref_off, ref_len, r, who)) return rc;
        for (int32_t i = 0; i < ref_len[r]; ++i)
            if (ea_host_rank(ref_arena[ref_off[r] + i]) < 0) {
                set_error("%s: read %lld: reference base %d is outside the IUPAC alphabet", who, (long long)r, i);
                return GBX_ERR_ARG;
            }
    }
    return GBX_OK;
}

}  // namespace

extern "C" {

int gbx_abea_eventalign_trans_host(int64_t n_reads, const double *events_per_base, float *trans)
{
    if (n_reads < 0 || (n_reads > 0 && (!events_per_base || !trans))) { set_error("gbx_abea_eventalign_trans_host: bad argument"); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n_reads; ++r) abea_transitions(events_per_base[r], trans + r * GBX_ABEA_METH_NTRANS);
    return GBX_OK;
}

size_t gbx_abea_eventalign_workspace_bytes(int64_t n_reads, int64_t n_cigar_total, int64_t rows_cap)
{
    return abea_eventalign_workspace_bytes(n_reads, n_cigar_total, rows_cap);
}

int gbx_abea_eventalign_device(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const int64_t *d_event_off, const float *d_event_mean,
                               const gbx_abea_model *d_models, const float *d_scale, const float *d_shift, const float *d_var, const float *d_log_var,
                               const float *d_trans, const int32_t *d_map, const int32_t *d_near, const int32_t *d_flags, const int64_t *d_cigar_off,
                               const uint32_t *d_cigar, const int32_t *d_pos, const uint8_t *d_rc, const int64_t *d_ref_off, const int32_t *d_ref_len,
                               const char *d_ref_arena, int32_t region_start, int32_t region_end, const int32_t *d_order, gbx_abea_eventalign_rec *d_rec,
                               int32_t *d_n_rec, int32_t *d_status, int64_t *d_counts, int64_t n_cigar_total, int64_t rows_cap, void *d_work,
                               size_t work_bytes, void *stream)
{
    const char *who = "gbx_abea_eventalign_device";
    if (n_reads < 0 || n_cigar_total < 0 || rows_cap < 1) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_reads == 0) return GBX_OK;
    if (!d_seq_off || !d_seq_len || !d_event_off || !d_event_mean || !d_models || !d_scale || !d_shift || !d_var || !d_log_var || !d_trans || !d_map ||
        !d_near || !d_cigar_off || !d_cigar || !d_pos || !d_rc || !d_ref_off || !d_ref_len || !d_ref_arena || !d_rec || !d_n_rec || !d_status || !d_work) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    const AbeaEventalignArgs a = abea_eventalign_args(n_reads, d_seq_off, d_seq_len, d_event_off, d_event_mean, d_models, d_scale, d_shift, d_var, d_log_var,
                                                      d_trans, d_map, d_near, d_flags, d_cigar_off, d_cigar, d_pos, d_rc, d_ref_off, d_ref_len, d_ref_arena,
                                                      region_start, region_end, d_order, d_rec, d_n_rec, d_status, d_counts, n_cigar_total, rows_cap, d_work);
    return abea_eventalign_launch(a, work_bytes, (hipStream_t)stream);
}

int gbx_abea_eventalign_host(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, int64_t seq_bytes, const int64_t *event_off,
                             const gbx_abea_event *events, const gbx_abea_model *models, const float *scale, const float *shift, const float *var,
                             const float *log_var, const double *events_per_base, const int32_t *map, const int32_t *flags, const int64_t *cigar_off,
                             const uint32_t *cigar, const int32_t *pos, const uint8_t *rc_flag, const int64_t *ref_off, const int32_t *ref_len,
                             const char *ref_arena, int32_t region_start, int32_t region_end, gbx_abea_eventalign_rec *rec, int32_t *n_rec, int32_t *status)
{
    const char *who = "gbx_abea_eventalign_host";
    RoctxRange range_(who);
    if (n_reads < 0 || seq_bytes < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_reads == 0) return GBX_OK;
    if (!seq_off || !seq_len || !event_off || !models || !scale || !shift || !var || !log_var || !events_per_base || !map || !cigar_off || !pos || !rc_flag ||
        !ref_off || !ref_len || !ref_arena || !n_rec || !status) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if (event_off[0] < 0) { set_error("%s: event_off below 0", who); return GBX_ERR_ARG; }
    int rc;
    for (int64_t r = 0; r < n_reads; ++r)
        if ((rc = read_check(seq_off, seq_len, seq_bytes, r, who)) || (rc = event_off_check(event_off, r, who)) || (rc = event_count_check(event_off, r, who)))
            return rc;
    if (event_off[n_reads] > event_off[0] && (!events || !rec)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = check_cigars(who, n_reads, cigar_off, cigar, seq_len))) return rc;
    if ((rc = check_refs(who, n_reads, ref_off, ref_len, ref_arena, region_start, region_end))) return rc;
    if ((rc = require_device())) return rc;
    const int64_t e0 = event_off[0], n_ev = event_off[n_reads] - e0, c0 = cigar_off[0], n_cig = cigar_off[n_reads] - c0;
    const std::vector<int64_t> eoff = rebased0(event_off, n_reads), coff = rebased0(cigar_off, n_reads);
    const std::vector<float> means = event_means(events, e0, n_ev);                                            // only the mean is read (eventalign.c:314)
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    const hipStream_t cs = L->compute;
    DevBuf dem(L), dmo(L), dmap(L), dcg(L);
    Carve small(L);
    const size_t n4 = (size_t)n_reads * 4, n8 = (size_t)n_reads * 8;
    for (size_t b : {n8, n4, n8 + 8, n4, n4, n4, n4, n4, n8 + 8, n4, (size_t)n_reads}) small.want(b);
    if ((rc = small.alloc()) || (rc = dem.alloc((size_t)n_ev * 4 + 16)) || (rc = dmo.alloc(GBX_ABEA_NMODEL * sizeof(gbx_abea_model))) ||
        (rc = dmap.alloc((size_t)seq_bytes * 8 + 16)) || (rc = dcg.alloc((size_t)n_cig * 4 + 16)))
        return rc;
    int64_t *dso = small.take<int64_t>(n8);
    int32_t *dsl = small.take<int32_t>(n4);
    int64_t *deo = small.take<int64_t>(n8 + 8);
    float *dsc = small.take<float>(n4), *dsh = small.take<float>(n4), *dvar = small.take<float>(n4), *dlv = small.take<float>(n4);
    int32_t *dfl = small.take<int32_t>(n4);
    int64_t *dco = small.take<int64_t>(n8 + 8);
    int32_t *dpos = small.take<int32_t>(n4);
    uint8_t *drc = small.take<uint8_t>((size_t)n_reads);
    StreamDrain drain{cs};
    GBX_HIP(hipMemcpyAsync(dso, seq_off, n8, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dsl, seq_len, n4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(deo, eoff.data(), n8 + 8, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dsc, scale, n4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dsh, shift, n4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dvar, var, n4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dlv, log_var, n4, hipMemcpyHostToDevice, cs));
    if (flags) GBX_HIP(hipMemcpyAsync(dfl, flags, n4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dco, coff.data(), n8 + 8, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dpos, pos, n4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(drc, rc_flag, (size_t)n_reads, hipMemcpyHostToDevice, cs));
    if (n_ev) GBX_HIP(hipMemcpyAsync(dem.p, means.data(), (size_t)n_ev * 4, hipMemcpyHostToDevice, cs));
    GBX_HIP(hipMemcpyAsync(dmo.p, models, GBX_ABEA_NMODEL * sizeof(gbx_abea_model), hipMemcpyHostToDevice, cs));
    if (seq_bytes) GBX_HIP(hipMemcpyAsync(dmap.p, map, (size_t)seq_bytes * 8, hipMemcpyHostToDevice, cs));
    if (n_cig) GBX_HIP(hipMemcpyAsync(dcg.p, cigar + c0, (size_t)n_cig * 4, hipMemcpyHostToDevice, cs));
    const EaOnDevice d{dso, dsl, deo, dem.as<float>(), dmo.as<gbx_abea_model>(), dsc, dsh, dvar, dlv, dmap.as<int32_t>(), flags ? dfl : nullptr,
                       dco, dcg.as<uint32_t>(), dpos, drc};
    return eventalign_on_lane(L, n_reads, seq_bytes, d, eoff.data(), events_per_base, n_cig, ref_off, ref_len, ref_arena, region_start, region_end, rec,
                              n_rec, status);
}

int gbx_abea_eventalign_summary_host(int64_t n_reads, const int64_t *event_off, const gbx_abea_event *events, const gbx_abea_model *models,
                                     const float *scale, const float *shift, const float *var, const uint8_t *rc_flag, const int32_t *pos,
                                     const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena, const gbx_abea_eventalign_rec *rec,
                                     const int32_t *n_rec, gbx_abea_eventalign_summary *out)
{
    const char *who = "gbx_abea_eventalign_summary_host";
    if (n_reads < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_reads == 0) return GBX_OK;
    if (!event_off || !models || !scale || !shift || !var || !rc_flag || !pos || !ref_off || !ref_len || !ref_arena || !n_rec || !out) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t ne = event_off[r + 1] - event_off[r];
        if (ne < 0 || n_rec[r] < 0 || n_rec[r] > ne) { set_error("%s: read %lld: %d records, %lld events", who, (long long)r, n_rec[r], (long long)ne); return GBX_ERR_ARG; }
        if (n_rec[r] > 0 && (!rec || !events)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
        gbx_abea_eventalign_summary s{};
        const gbx_abea_eventalign_rec *q = rec + (event_off[r] - event_off[0]);
        const gbx_abea_event *ev = events + event_off[r];
        uint64_t prev_ref_pos = ~(uint64_t)0;                                                  /* std::string::npos, eventalign.c:1600 */
        for (int32_t i = 0; i < n_rec[r]; ++i) {
            if (q[i].event_idx < 0 || q[i].event_idx >= ne) { set_error("%s: read %lld: record %d names event %d", who, (long long)r, i, q[i].event_idx); return GBX_ERR_ARG; }
            s.num_events += 1;
            const uint64_t ref_move = (uint64_t)(int64_t)q[i].ref_pos - prev_ref_pos;
            if (ref_move == 0) s.num_stays += 1;
            else if (i != 0 && ref_move > 1) s.num_skips += 1;
            else if (i != 0 && ref_move == 1) s.num_steps += 1;
            s.sum_duration += ev[q[i].event_idx].length;
            if (q[i].state == 'M') {
                char rk[GBX_ABEA_KMER + 1], mk[GBX_ABEA_KMER + 1];
                uint32_t rank = 0;
                if (!ea_kmers(ref_arena + ref_off[r], ref_len[r], pos[r], rc_flag[r], q[i], rk, mk, &rank)) {
                    set_error("%s: read %lld: record %d lies outside the reference segment", who, (long long)r, i);
                    return GBX_ERR_ARG;
                }
                const float level = ev[q[i].event_idx].mean;                                  /* z_score, eventalign.c:1561-1577 */
                const float gp_mean = scale[r] * models[rank].level_mean + shift[r];
                const float gp_stdv = models[rank].level_stdv * var[r];
                const double z = (level - gp_mean) / gp_stdv;
                s.sum_z_score += z;
            }
            prev_ref_pos = (uint64_t)(int64_t)q[i].ref_pos;
        }
        if (n_rec[r] > 0) s.reference_span = q[n_rec[r] - 1].ref_pos - q[0].ref_pos + 1;
        out[r] = s;
    }
    return GBX_OK;
}

int gbx_abea_eventalign_tsv_host(const gbx_abea_event *events, int64_t n_events, const gbx_abea_model *models, float scale, float shift, float var, int rc_flag,
                                 int32_t pos, const char *ref, int32_t ref_len, const gbx_abea_eventalign_rec *rec, int32_t n_rec, int header,
                                 int print_read_names, int scale_events, int write_samples, int64_t read_index, const char *read_name, const char *ref_name,
                                 float sample_rate, char *text, int64_t cap, int64_t *need)
{
    const char *who = "gbx_abea_eventalign_tsv_host";
    if (!need || n_rec < 0 || n_events < 0 || cap < 0 || ref_len < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    *need = 0;
    if (write_samples) { set_error("%s: write_samples is not implemented (the reference asserts)", who); return GBX_ERR_UNSUPPORTED; }
    if (!models || !ref_name || (print_read_names && !read_name) || (n_rec > 0 && (!events || !rec || !ref))) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    std::string out;
    char line[512];
    if (header) {                                                                              /* eventalign.c:1651-1662 */
        snprintf(line, sizeof line, "%s\t%s\t%s\t%s\t%s\t", "contig", "position", "reference_kmer", (print_read_names ? "read_name" : "read_index"), "strand");
        out += line;
        snprintf(line, sizeof line, "%s\t%s\t%s\t%s\t", "event_index", "event_level_mean", "event_stdv", "event_length");
        out += line;
        snprintf(line, sizeof line, "%s\t%s\t%s\t%s", "model_kmer", "model_mean", "model_stdv", "standardized_level");
        out += line;
        out += "\n";
    }
    for (int32_t i = 0; i < n_rec; ++i) {                                                      /* eventalign.c:1863-1937 */
        const gbx_abea_eventalign_rec &q = rec[i];
        char rk[GBX_ABEA_KMER + 1], mk[GBX_ABEA_KMER + 1];
        uint32_t rank = 0;
        if (q.event_idx < 0 || q.event_idx >= n_events) { set_error("%s: record %d names event %d", who, i, q.event_idx); return GBX_ERR_ARG; }
        if (!ea_kmers(ref, ref_len, pos, rc_flag, q, rk, mk, &rank)) { set_error("%s: record %d lies outside the reference segment", who, i); return GBX_ERR_ARG; }
        out += ref_name; out += "\t";
        snprintf(line, sizeof line, "%d\t%s\t", q.ref_pos, rk);
        out += line;
        if (!print_read_names) { snprintf(line, sizeof line, "%ld", (long)read_index); out += line; }
        else out += read_name;
        out += "\tt\t";
        float event_mean = events[q.event_idx].mean;
        const float event_stdv = events[q.event_idx].stdv;
        const float event_duration = events[q.event_idx].length / sample_rate;
        float model_mean = 0.0, model_stdv = 0.0;
        if (scale_events) {
            event_mean = (events[q.event_idx].mean - shift) / scale;                            /* get_fully_scaled_level */
            if (q.state != 'B') { model_mean = models[rank].level_mean; model_stdv = models[rank].level_stdv; }
        } else if (q.state != 'B') {
            model_mean = scale * models[rank].level_mean + shift;                               /* get_scaled_gaussian_from_pore_model_state */
            model_stdv = models[rank].level_stdv * var;
        }
        const float standard_level = (event_mean - model_mean) / (sqrtf(var) * model_stdv);     /* sqrt of a float in C++: the float overload */
        snprintf(line, sizeof line, "%d\t%.2lf\t%.3lf\t%.5lf\t", q.event_idx, event_mean, event_stdv, event_duration);
        out += line;
        snprintf(line, sizeof line, "%s\t%.2lf\t%.2lf\t%.2lf", mk, model_mean, model_stdv, standard_level);
        out += line;
        out += "\n";
    }
    *need = (int64_t)out.size();
    if ((int64_t)out.size() > cap) { set_error("%s: %lld bytes of text, room for %lld", who, (long long)out.size(), (long long)cap); return GBX_ERR_ARG; }
    if (!out.empty()) { if (!text) { set_error("%s: null pointer", who); return GBX_ERR_ARG; } memcpy(text, out.data(), out.size()); }
    return GBX_OK;
}

int gbx_abea_eventalign_from_signal_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range, const float *digitisation,
                                         const float *offset, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                                         const gbx_abea_model *models, const int64_t *cigar_off, const uint32_t *cigar, const int32_t *pos,
                                         const uint8_t *rc_flag, const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena, int32_t region_start,
                                         int32_t region_end, int32_t *flags, int32_t *status, float *scale, float *shift, float *var, float *log_var,
                                         double *events_per_base, int64_t *event_off, gbx_abea_event *events, int64_t event_cap, int64_t *n_events_total,
                                         gbx_abea_eventalign_rec *rec, int32_t *n_rec, int32_t *ea_status)
{
    const char *who = "gbx_abea_eventalign_from_signal_host";
    RoctxRange range_(who);
    if (n_reads < 0 || seq_bytes < 0 || event_cap < 0 || !n_events_total) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    *n_events_total = 0;
    if (n_reads == 0) return GBX_OK;
    if (!seq_len || !cigar_off || !pos || !rc_flag || !ref_off || !ref_len || !ref_arena || !flags || !status || !scale || !shift || !var || !log_var ||
        !events_per_base || !event_off || !n_rec || !ea_status || (event_cap > 0 && (!events || !rec))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = check_cigars(who, n_reads, cigar_off, cigar, seq_len);
    if (rc) return rc;
    if ((rc = check_refs(who, n_reads, ref_off, ref_len, ref_arena, region_start, region_end))) return rc;
    // a batch in which no read has events never reaches the tail
    for (int64_t r = 0; r < n_reads; ++r) {
        flags[r] = GBX_ABEA_FAILED_ALIGNMENT; var[r] = 0.0f; log_var[r] = 0.0f; events_per_base[r] = 0.0; n_rec[r] = 0; ea_status[r] = 0; event_off[r] = 0;
    }
    event_off[n_reads] = 0;
    // behind align(), on the buffers it left: calibration, the logarithm on the host, eventalign, the event records down
    const abea_tail_fn eventalign_tail = [&](const AbeaAligned &a) -> int {
        Lane *L = a.L;
        const hipStream_t cs = L->compute;
        const int64_t n = a.n_reads, total = a.event_off[n];
        for (int64_t r = 0; r <= n; ++r) event_off[r] = a.event_off[r];
        *n_events_total = total;
        if (total > event_cap) { set_error("%s: %lld events, room for %lld", who, (long long)total, (long long)event_cap); return GBX_ERR_ARG; }
        AbeaCalibrated cal(L);                                   // its guard drains the stream however this function is left
        if ((rc = cal.queue(a, cigar_off, cigar, pos, rc_flag, scale, shift, var, events_per_base, flags))) return rc;
        if (total) GBX_HIP(hipMemcpyAsync(events, a.d_events, (size_t)total * sizeof(gbx_abea_event), hipMemcpyDeviceToHost, cs));
        if ((rc = cal.finish(log_var))) return rc;
        const EaOnDevice d{a.d_seq_off, a.d_seq_len, a.d_event_off, a.d_event_mean, a.d_models, a.d_scale, a.d_shift, cal.var, cal.log_var, cal.map, cal.flags,
                           cal.cigar_off, cal.cigar, cal.pos, cal.rc};
        return eventalign_on_lane(L, n, a.seq_bytes, d, a.event_off, events_per_base, cal.n_cigar, ref_off, ref_len, ref_arena, region_start,
                                  region_end, rec, n_rec, ea_status);
    };
    return abea_signal_align_tail(who, n_reads, raw, raw_off, range, digitisation, offset, seq_off, seq_len, seq_arena, seq_bytes, models, status, scale,
                                  shift, eventalign_tail);
}

}  // extern "C"
