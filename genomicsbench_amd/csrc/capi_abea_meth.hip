// capi_abea_meth.hip — abea methylation scoring: the plan (tables, order), the site planner on the host and the entries of the one on the
// device, the score entries and the call-methylation TSV writer of the C-ABI (include/gbx.h).
#include "capi_common.h"
#include <cctype>

using namespace gbx;

namespace {

using abea_meth_rules::job_class;

// ---- the string functions of meth.c
char possible0(char c)                                       // getPossibleSymbols(c)[0], meth.c:221-256
{
    switch (c) {
        case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 'A';
        case 'C': case 'S': case 'Y': case 'B': return 'C';
        case 'G': case 'K': return 'G';
        case 'T': return 'T';
        default: return 'A';                                 // not a IUPAC symbol (the reference asserts): ranks as A
    }
}
char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'T'; }     // meth.c:261-273

void reverse_complement(const char *s, int64_t n, char *out)                                 // meth.c:276-286
{
    for (int64_t i = 0; i < n; ++i) out[n - 1 - i] = complement(s[i]);
}

void methylate(const char *s, int64_t n, char *out)                                          // meth.c:359-382: every whole "CG" becomes "MG"
{
    memcpy(out, s, (size_t)n);
    for (int64_t i = 0; i < n;) {
        if (i + 1 < n && s[i] == 'C' && s[i + 1] == 'G') { out[i] = 'M'; out[i + 1] = 'G'; i += 2; }
        else i += 1;
    }
}

void reverse_complement_meth(const char *s, int64_t n, char *out)                            // meth.c:387-420
{
    int64_t i = 0, j = n - 1;
    while (i < n) {
        int64_t off = 0, len = 0;
        // match_to_site(str, i, "MG", 2), meth.c:326-354: the whole string inside the site, or a prefix of the site at i
        if (i == 0 && n <= 2 && ((n == 2 && s[0] == 'M' && s[1] == 'G') || (n == 1 && (s[0] == 'M' || s[0] == 'G')))) {
            off = (n == 1 && s[0] == 'G') ? 1 : 0; len = n;
        } else {
            const int64_t cl = n - i < 2 ? n - i : 2;
            if (s[i] == 'M' && (cl == 1 || s[i + 1] == 'G')) len = cl;
        }
        bool covers = false;
        for (int64_t k = 0; k < len; ++k) covers |= s[i + k] == 'M';
        if (len > 0 && covers) {
            for (int64_t k = off; k < off + len; ++k) { out[j--] = "GM"[k]; i += 1; }
        } else {
            out[j--] = complement(s[i++]);
        }
    }
}

int pair_lower_bound(const gbx_abea_pair *a, int low, int high, int v)                       // meth.c:422-431
{
    while (low < high) {
        const int mid = low + (high - low) / 2;
        if (a[mid].ref_pos < v) low = mid + 1; else high = mid;
    }
    return low;
}

bool find_by_ref_bounds(const gbx_abea_pair *pairs, int64_t size, int ref_start, int ref_stop, int &read_start, int &read_stop)   // meth.c:433-467
{
    const int start_i = pair_lower_bound(pairs, 0, (int)size, ref_start), stop_i = pair_lower_bound(pairs, 0, (int)size, ref_stop);
    if (start_i == size || stop_i == size) return false;
    const bool left_bounded = pairs[start_i].ref_pos <= ref_start || (start_i != 0 && pairs[start_i - 1].ref_pos <= ref_start);
    // as written, the second operand compares against ref_start (meth.c:448-450); the lower bound makes the first one true
    // whenever stop_i is inside the record, so the entry past the end is never read
    const bool right_bounded = pairs[stop_i].ref_pos >= ref_stop || (stop_i + 1 < size && pairs[stop_i + 1].ref_pos >= ref_start);
    if (!(left_bounded && right_bounded)) return false;
    read_start = pairs[start_i].read_pos;
    read_stop = pairs[stop_i].read_pos;
    return true;
}

// calculate_methylation_for_read (meth.c:501-658) for one read.  sites == nullptr: counts only.  The read's sites go to
// sites[0..], its jobs to jobs[0..], its strings to arena + seq_base.  Returns false when the record runs against rc.
bool sites_of_read(int32_t read, const char *ref, int64_t ref_len, int32_t ref_start_pos, bool rc, const gbx_abea_pair *rec, int64_t n_rec,
                   gbx_abea_meth_site *sites, gbx_abea_meth_job *jobs, char *arena, int64_t seq_base, int64_t *n_sites_out, int64_t *bytes_out)
{
    int64_t n_sites = 0, bytes = 0;
    *n_sites_out = *bytes_out = 0;
    if (ref_len < 2 || n_rec == 0) return true;                                              // an empty record bounds nothing
    std::vector<char> ref_seq((size_t)ref_len);
    for (int64_t i = 0; i < ref_len; ++i) ref_seq[(size_t)i] = possible0((char)toupper((unsigned char)ref[i]));   // meth.c:288-306
    std::vector<int> cpg;
    for (int64_t i = 0; i < ref_len - 1; ++i)
        if (ref_seq[(size_t)i] == 'C' && ref_seq[(size_t)i + 1] == 'G') cpg.push_back((int)i);
    const int min_separation = 10;
    const size_t n_cpg = cpg.size();
    size_t curr = 0;
    while (curr < n_cpg) {
        size_t end = curr + 1;
        while (end < n_cpg) { if (cpg[end] - cpg[end - 1] > min_separation) break; end += 1; }
        const size_t start_idx = curr, end_idx = end;
        curr = end;
        const int sub_start_pos = cpg[start_idx] - min_separation, sub_end_pos = cpg[end_idx - 1] + min_separation;
        const int span = cpg[end_idx - 1] - cpg[start_idx];
        if (sub_start_pos <= min_separation || span > 200) continue;
        int64_t L = sub_end_pos - sub_start_pos + 1;                                          // substr clamps at the end of the segment
        if (L > ref_len - sub_start_pos) L = ref_len - sub_start_pos;
        const int calling_start = sub_start_pos + ref_start_pos, calling_end = sub_end_pos + ref_start_pos;
        int e1 = 0, e2 = 0;
        if (!find_by_ref_bounds(rec, n_rec, calling_start, calling_end, e1, e2)) continue;
        const double ratio = fabs((double)(e2 - e1)) / (calling_start - calling_end);        // as written: negative, never above the bound
        if (abs(e2 - e1) <= 10 || ratio > 20) continue;
        if ((e1 <= e2) == rc) return false;
        if (sites) {
            char *sub = arena + seq_base + bytes, *rcs = sub + L, *msub = rcs + L, *mrc = msub + L;
            memcpy(sub, ref_seq.data() + sub_start_pos, (size_t)L);
            reverse_complement(sub, L, rcs);
            methylate(sub, L, msub);
            reverse_complement_meth(msub, L, mrc);
            gbx_abea_meth_site &S = sites[n_sites];
            S.read = read;
            S.start_position = cpg[start_idx] + ref_start_pos;
            S.end_position = cpg[end_idx - 1] + ref_start_pos;
            S.n_cpg = (int32_t)(end_idx - start_idx);
            const int64_t o0 = cpg[start_idx] - GBX_ABEA_KMER + 1, o1 = cpg[end_idx - 1] + GBX_ABEA_KMER;
            S.ctx_off = o0;
            S.ctx_len = (int32_t)(std::min<int64_t>(o1, ref_len) - o0);
            S.pad_ = 0;
            for (int m = 0; m < 2; ++m) {
                gbx_abea_meth_job &J = jobs[2 * n_sites + m];
                J.seq_off = seq_base + bytes + 2 * m * L; J.rc_off = J.seq_off + L; J.seq_len = (int32_t)L; J.read = read;
                J.event_start = e1; J.event_stop = e2; J.rc = rc ? 1 : 0; J.flags = GBX_ABEA_METH_PRE_CLIP | GBX_ABEA_METH_POST_CLIP;
            }
        }
        bytes += 4 * L;
        n_sites++;
    }
    *n_sites_out = n_sites;
    *bytes_out = bytes;
    return true;
}

}  // namespace

extern "C" {

int gbx_abea_meth_tables_host(int64_t n_reads, const double *events_per_base, float *flogsum, float *trans, int64_t flank_len, float *pre_flank,
                              float *post_flank)
{
    if (n_reads < 0 || flank_len < 2 || !flogsum || !pre_flank || !post_flank || (n_reads > 0 && (!events_per_base || !trans))) {
        set_error("gbx_abea_meth_tables_host: bad argument");
        return GBX_ERR_ARG;
    }
    for (int i = 0; i < GBX_ABEA_FLOGSUM_TBL; i++) flogsum[i] = log(1. + exp((double)-i / 1000.f));           /* logsum.h:44-46 */
    for (int64_t r = 0; r < n_reads; ++r) abea_transitions(events_per_base[r], trans + r * GBX_ABEA_METH_NTRANS);      /* hmm.c:247-295 */
    /* pre_flank[i] depends on i alone (hmm.c:172-205), post_flank on the distance to the last event (hmm.c:132-168); the sums
       are double, stored to float */
    pre_flank[0] = log(1 - 0.5);
    pre_flank[1] = log(0.5) + -3.0f + log(1 - 0.9);
    for (int64_t i = 2; i < flank_len; ++i) pre_flank[i] = log(0.9) + -3.0f + pre_flank[i - 1];
    post_flank[0] = log(1 - 0.5);
    post_flank[1] = log(0.5) + -3.0f + log(1 - 0.9);
    for (int64_t j = 2; j < flank_len; ++j) post_flank[j] = log(0.9) + -3.0f + post_flank[j - 1];
    return GBX_OK;
}

int gbx_abea_meth_plan_host(int64_t n_jobs, const gbx_abea_meth_job *jobs, int64_t seq_bytes, int64_t n_reads, const int64_t *event_off,
                            const double *events_per_base, float *flogsum, float *trans, int64_t flank_len, float *pre_flank,
                            float *post_flank, int32_t *order, int64_t *class_off)
{
    if (n_jobs < 0 || n_reads < 0 || seq_bytes < 0 || flank_len < 2 || !flogsum || !pre_flank || !post_flank || !class_off ||
        (n_jobs > 0 && (!jobs || !order)) || (n_reads > 0 && (!event_off || !events_per_base || !trans))) {
        set_error("gbx_abea_meth_plan_host: bad argument");
        return GBX_ERR_ARG;
    }
    if (n_jobs > 0x7fffffffLL - 1024) { set_error("gbx_abea_meth_plan_host: more than 2^31 jobs in one call"); return GBX_ERR_UNSUPPORTED; }
    for (int64_t r = 0; r < n_reads; ++r)
        if (event_off[r + 1] < event_off[r]) { set_error("gbx_abea_meth_plan_host: event_off not monotone at read %lld", (long long)r); return GBX_ERR_ARG; }
    if (int e = gbx_abea_meth_tables_host(n_reads, events_per_base, flogsum, trans, flank_len, pre_flank, post_flank)) return e;
    std::vector<std::pair<int64_t, int32_t>> key((size_t)n_jobs);
    int64_t count[GBX_ABEA_METH_NCLASS] = {0, 0, 0, 0};
    for (int64_t j = 0; j < n_jobs; ++j) {
        const gbx_abea_meth_job &J = jobs[j];
        const int64_t nk = (int64_t)J.seq_len - GBX_ABEA_KMER + 1, rows = job_rows(J);
        if (int e = abea_meth_job_refuse(j, J, seq_bytes, n_reads, event_off, flank_len)) return e;
        const int c = job_class(nk);
        count[c]++;
        key[(size_t)j] = std::make_pair(((int64_t)c << 40) - rows, (int32_t)j);              /* class, then longest first; ties in input order */
    }
    std::sort(key.begin(), key.end());
    for (int64_t j = 0; j < n_jobs; ++j) order[j] = key[(size_t)j].second;
    class_off[0] = 0;
    for (int c = 0; c < GBX_ABEA_METH_NCLASS; ++c) class_off[c + 1] = class_off[c] + count[c];
    return GBX_OK;
}

int gbx_abea_meth_cells(int64_t n_jobs, const gbx_abea_meth_job *jobs, int64_t *cells)
{
    if (n_jobs < 0 || !cells || (n_jobs > 0 && !jobs)) { set_error("gbx_abea_meth_cells: bad argument"); return GBX_ERR_ARG; }
    int64_t v = 0;
    for (int64_t j = 0; j < n_jobs; ++j) v += job_rows(jobs[j]) * std::max<int64_t>((int64_t)jobs[j].seq_len - GBX_ABEA_KMER + 1, 0) * 3;
    *cells = v;
    return GBX_OK;
}

int gbx_abea_meth_score_device(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, const char *d_seq_arena, const int64_t *d_event_off,
                               const float *d_event_mean, const float *d_scale, const float *d_shift, const float *d_var,
                               const float *d_log_var, const gbx_abea_model *d_cpg_model, const float *d_flogsum, const float *d_trans,
                               const float *d_pre_flank, const float *d_post_flank, const int32_t *d_order, const int64_t *class_off,
                               float *d_scores, void *stream)
{
    if (n_jobs < 0) { set_error("gbx_abea_meth_score_device: bad argument"); return GBX_ERR_ARG; }
    if (n_jobs == 0) return GBX_OK;
    if (!d_jobs || !d_seq_arena || !d_event_off || !d_event_mean || !d_scale || !d_shift || !d_var || !d_log_var || !d_cpg_model ||
        !d_flogsum || !d_trans || !d_pre_flank || !d_post_flank || !d_order || !class_off || !d_scores) {
        set_error("gbx_abea_meth_score_device: null pointer");
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_meth_launch(n_jobs, d_jobs, d_seq_arena, d_event_off, d_event_mean, d_scale, d_shift, d_var, d_log_var, d_cpg_model, d_flogsum,
                            d_trans, d_pre_flank, d_post_flank, d_order, class_off, d_scores, (hipStream_t)stream);
}

int gbx_abea_meth_score_host(int64_t n_jobs, const gbx_abea_meth_job *jobs, const char *seq_arena, int64_t seq_bytes, int64_t n_reads,
                             const int64_t *event_off, const gbx_abea_event *events, const float *scale, const float *shift,
                             const float *var, const float *log_var, const double *events_per_base, const gbx_abea_model *cpg_model,
                             float *scores)
{
    RoctxRange range_("gbx_abea_meth_score_host");
    if (n_jobs < 0 || n_reads < 0 || seq_bytes < 0) { set_error("gbx_abea_meth_score_host: bad argument"); return GBX_ERR_ARG; }
    if (n_jobs == 0) return GBX_OK;
    if (!jobs || !seq_arena || !event_off || !events || !scale || !shift || !var || !log_var || !events_per_base || !cpg_model || !scores || n_reads == 0) {
        set_error("gbx_abea_meth_score_host: null pointer");
        return GBX_ERR_ARG;
    }
    if (event_off[0] < 0) { set_error("gbx_abea_meth_score_host: event_off below 0"); return GBX_ERR_ARG; }
    AbeaMethPlan plan;
    int rc = plan.build(n_jobs, jobs, seq_bytes, n_reads, event_off, events_per_base);
    if (rc) return rc;
    if ((rc = require_device())) return rc;
    // only the means of the events are read (hmm.c:76): gathered from the 24-byte records on the way up, as in gbx_abea_align_host
    const int64_t e0 = event_off[0], n_ev = event_off[n_reads] - e0;
    const std::vector<int64_t> eoff = rebased0(event_off, n_reads);
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    DevBuf djb(L), dsq(L), deo(L), dem(L), dsc(L), dsh(L), dvr(L), dlv(L), dmo(L), dfl(L), dtr(L), dpr(L), dpo(L), dor(L), dout(L);
    const size_t job_bytes = (size_t)n_jobs * sizeof(gbx_abea_meth_job), model_bytes = GBX_ABEA_NMODEL_CPG * sizeof(gbx_abea_model);
    if ((rc = djb.alloc(job_bytes)) || (rc = dsq.alloc((size_t)seq_bytes + 16)) || (rc = deo.alloc((n_reads + 1) * 8)) || (rc = dem.alloc((size_t)n_ev * 4 + 16)) ||
        (rc = dsc.alloc(n_reads * 4)) || (rc = dsh.alloc(n_reads * 4)) || (rc = dvr.alloc(n_reads * 4)) || (rc = dlv.alloc(n_reads * 4)) ||
        (rc = dmo.alloc(model_bytes)) || (rc = dfl.alloc(GBX_ABEA_FLOGSUM_TBL * 4)) || (rc = dtr.alloc(plan.trans.size() * 4)) ||
        (rc = dpr.alloc((size_t)plan.flank_len * 4)) || (rc = dpo.alloc((size_t)plan.flank_len * 4)) || (rc = dor.alloc((size_t)n_jobs * 4)) ||
        (rc = dout.alloc((size_t)n_jobs * 4)))
        return rc;
    HostPipe pipe(L, job_bytes + (size_t)seq_bytes + (size_t)n_ev * 4 + model_bytes + (size_t)n_jobs * 4 + (size_t)n_reads * 64, false);
    if ((rc = pipe.prepare(1))) return rc;
    pipe.stage(0, djb.p, jobs, job_bytes);
    if (seq_bytes) pipe.stage(0, dsq.p, seq_arena, (size_t)seq_bytes);
    pipe.stage(0, deo.p, eoff.data(), (n_reads + 1) * 8);
    if (n_ev) pipe.stage_field4(0, dem.p, &events[e0].mean, (size_t)n_ev, (int)sizeof(gbx_abea_event));
    pipe.stage(0, dsc.p, scale, n_reads * 4); pipe.stage(0, dsh.p, shift, n_reads * 4);
    pipe.stage(0, dvr.p, var, n_reads * 4); pipe.stage(0, dlv.p, log_var, n_reads * 4);
    pipe.stage(0, dmo.p, cpg_model, model_bytes);
    pipe.stage(0, dfl.p, plan.flogsum.data(), GBX_ABEA_FLOGSUM_TBL * 4); pipe.stage(0, dtr.p, plan.trans.data(), plan.trans.size() * 4);
    pipe.stage(0, dpr.p, plan.pre.data(), (size_t)plan.flank_len * 4); pipe.stage(0, dpo.p, plan.post.data(), (size_t)plan.flank_len * 4);
    pipe.stage(0, dor.p, plan.order.data(), (size_t)n_jobs * 4);
    pipe.start();
    if ((rc = pipe.wait_stage(0))) return pipe.finish(rc);
    rc = abea_meth_launch(n_jobs, djb.as<gbx_abea_meth_job>(), dsq.as<char>(), deo.as<int64_t>(), dem.as<float>(), dsc.as<float>(), dsh.as<float>(),
                          dvr.as<float>(), dlv.as<float>(), dmo.as<gbx_abea_model>(), dfl.as<float>(), dtr.as<float>(), dpr.as<float>(),
                          dpo.as<float>(), dor.as<int32_t>(), plan.class_off, dout.as<float>(), L->compute);
    if (rc) return pipe.finish(rc);
    pipe.fetch(0, scores, dout.p, (size_t)n_jobs * 4);
    if ((rc = pipe.chunk_launched(0))) return pipe.finish(rc);
    return pipe.finish();
}

int gbx_abea_meth_sites_host(int64_t n_reads, const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena,
                             const int32_t *ref_start_pos, const uint8_t *rc, const int64_t *rec_off, const gbx_abea_pair *rec,
                             int64_t site_cap, gbx_abea_meth_site *sites, gbx_abea_meth_job *jobs, int64_t *n_sites, int64_t seq_cap,
                             char *seq_arena, int64_t *seq_bytes)
{
    if (n_reads < 0 || site_cap < 0 || seq_cap < 0 || !n_sites || !seq_bytes) { set_error("gbx_abea_meth_sites_host: bad argument"); return GBX_ERR_ARG; }
    *n_sites = *seq_bytes = 0;
    if (n_reads == 0) return GBX_OK;
    if (!ref_off || !ref_len || !ref_arena || !ref_start_pos || !rc || !rec_off || (site_cap > 0 && (!sites || !jobs)) || (seq_cap > 0 && !seq_arena)) {
        set_error("gbx_abea_meth_sites_host: null pointer");
        return GBX_ERR_ARG;
    }
    if (n_reads > 0x7fffffffLL) { set_error("gbx_abea_meth_sites_host: more than 2^31 reads"); return GBX_ERR_UNSUPPORTED; }
    for (int64_t r = 0; r < n_reads; ++r) {
        if (ref_off[r] < 0 || ref_len[r] < 0 || rec_off[r + 1] < rec_off[r] || rec_off[r] < 0 || (rec_off[r + 1] > rec_off[r] && !rec)) {
            set_error("gbx_abea_meth_sites_host: bad offsets at read %lld", (long long)r);
            return GBX_ERR_ARG;
        }
        if (rec_off[r + 1] - rec_off[r] > 0x7fffffffLL) { set_error("gbx_abea_meth_sites_host: the record of read %lld is too long", (long long)r); return GBX_ERR_UNSUPPORTED; }
    }
    std::vector<int64_t> site_off((size_t)n_reads + 1, 0), byte_off((size_t)n_reads + 1, 0);
    std::vector<uint8_t> bad((size_t)n_reads, 0);
    auto pass = [&](bool fill) {
        parallel_ranges(n_reads, host_workers(), [&](int, int64_t lo, int64_t hi) {
            for (int64_t r = lo; r < hi; ++r) {
                int64_t ns = 0, nb = 0;
                const bool ok = sites_of_read((int32_t)r, ref_arena + ref_off[r], ref_len[r], ref_start_pos[r], rc[r] != 0, rec ? rec + rec_off[r] : nullptr,
                                              rec_off[r + 1] - rec_off[r], fill ? sites + site_off[(size_t)r] : nullptr,
                                              fill ? jobs + 2 * site_off[(size_t)r] : nullptr, seq_arena, byte_off[(size_t)r], &ns, &nb);
                if (!ok) bad[(size_t)r] = 1;
                if (!fill) { site_off[(size_t)r + 1] = ns; byte_off[(size_t)r + 1] = nb; }
            }
        });
    };
    pass(false);
    for (int64_t r = 0; r < n_reads; ++r) {
        if (bad[(size_t)r]) { set_error("gbx_abea_meth_sites_host: the record of read %lld runs against its strand", (long long)r); return GBX_ERR_ARG; }
        site_off[(size_t)r + 1] += site_off[(size_t)r];
        byte_off[(size_t)r + 1] += byte_off[(size_t)r];
    }
    *n_sites = site_off[(size_t)n_reads];
    *seq_bytes = byte_off[(size_t)n_reads];
    if (*n_sites > site_cap || *seq_bytes > seq_cap) {
        set_error("gbx_abea_meth_sites_host: %lld sites and %lld string bytes, room for %lld and %lld", (long long)*n_sites, (long long)*seq_bytes,
                  (long long)site_cap, (long long)seq_cap);
        return GBX_ERR_ARG;
    }
    pass(true);
    return GBX_OK;
}

int64_t gbx_abea_meth_sites_work(int64_t n_reads, int64_t ref_bytes)
{
    if (n_reads < 0 || ref_bytes < 0) return 0;
    return (int64_t)abea_meth_sites_work_bytes(n_reads);
}

int gbx_abea_meth_sites_device(int pass, int64_t n_reads, const int64_t *d_ref_off, const int32_t *d_ref_len, const char *d_ref_arena,
                               const int32_t *d_ref_start_pos, const uint8_t *d_rc, const int64_t *d_rec_off, const gbx_abea_pair *d_rec, void *d_work,
                               int64_t *d_site_off, int64_t *d_byte_off, uint8_t *d_bad, int64_t site_cap, gbx_abea_meth_site *d_sites,
                               gbx_abea_meth_job *d_jobs, int64_t seq_cap, char *d_seq_arena, void *stream)
{
    const char *who = "gbx_abea_meth_sites_device";
    if (n_reads < 0 || site_cap < 0 || seq_cap < 0 || pass < 1 || pass > (GBX_ABEA_METH_SITES_COUNT | GBX_ABEA_METH_SITES_FILL)) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (n_reads == 0) return GBX_OK;
    if (!d_ref_off || !d_ref_len || !d_ref_arena || !d_ref_start_pos || !d_rc || !d_rec_off || !d_rec || !d_work || !d_site_off || !d_byte_off || !d_bad ||
        ((pass & GBX_ABEA_METH_SITES_FILL) && ((site_cap > 0 && (!d_sites || !d_jobs)) || (seq_cap > 0 && !d_seq_arena)))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_meth_sites_launch(pass, n_reads, d_ref_off, d_ref_len, d_ref_arena, d_ref_start_pos, d_rc, d_rec_off, d_rec, d_work, d_site_off, d_byte_off,
                                  d_bad, site_cap, d_sites, d_jobs, seq_cap, d_seq_arena, (hipStream_t)stream);
}

int64_t gbx_abea_meth_order_work(int64_t n_jobs) { return n_jobs < 0 ? 0 : (int64_t)abea_meth_order_work_bytes(n_jobs); }

int gbx_abea_meth_order_device(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, int64_t seq_bytes, int64_t n_reads, const int64_t *d_event_off,
                               int64_t flank_len, int max_rows_bits, void *d_work, int32_t *d_order, int64_t *d_class_off, int64_t *d_first_bad,
                               void *stream)
{
    const char *who = "gbx_abea_meth_order_device";
    if (n_jobs < 0 || n_reads < 0 || seq_bytes < 0 || flank_len < 2 || max_rows_bits < 1 || max_rows_bits > 30 || flank_len > (1ll << max_rows_bits)) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!d_class_off || !d_first_bad || (n_jobs > 0 && (!d_jobs || !d_work || !d_order)) || (n_jobs > 0 && n_reads > 0 && !d_event_off)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_meth_order_launch(n_jobs, d_jobs, seq_bytes, n_reads, d_event_off, flank_len, max_rows_bits, d_work, d_order, d_class_off, d_first_bad,
                                  (hipStream_t)stream);
}

int gbx_abea_meth_tsv_host(int64_t n_sites, const gbx_abea_meth_site *sites, const float *scores, int64_t n_reads, const char *const *read_names,
                           const char *const *contig_names, const uint8_t *rc, const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena,
                           int version, int32_t clip_start, int32_t clip_end, int with_header, int64_t cap, char *out, int64_t *n_bytes)
{
    const char *who = "gbx_abea_meth_tsv_host";
    if (!n_bytes || n_sites < 0 || n_reads < 0 || cap < 0 || (version != 1 && version != 2)) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    *n_bytes = 0;
    if (n_sites > 0 && (!sites || !scores || !read_names || !contig_names || !rc || !ref_off || !ref_len || !ref_arena)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    std::string text;
    char line[256];
    if (with_header)                                                                         /* meth_main.c:449-457 */
        text += version == 1 ? "chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_cpgs\tsequence\n"
                             : "chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_motifs\tsequence\n";
    for (int64_t s = 0; s < n_sites; ++s) {                                                  /* f5c.c:1629-1653 */
        const gbx_abea_meth_site &S = sites[s];
        if (S.read < 0 || S.read >= n_reads || !read_names[S.read] || !contig_names[S.read]) { set_error("%s: site %lld names read %d", who, (long long)s, S.read); return GBX_ERR_ARG; }
        const int64_t len = ref_len[S.read];
        if (ref_off[S.read] < 0 || S.ctx_len < 0 || S.ctx_off < 0 || S.ctx_off + S.ctx_len > len) {
            set_error("%s: the context of site %lld lies outside its reference segment", who, (long long)s);
            return GBX_ERR_ARG;
        }
        if ((clip_start != -1 && S.start_position < clip_start) || (clip_end != -1 && S.end_position >= clip_end)) continue;
        const double sum_ll_m = scores[2 * s + 1], sum_ll_u = scores[2 * s], diff = sum_ll_m - sum_ll_u;
        text += contig_names[S.read];
        if (version == 1) snprintf(line, sizeof line, "\t%d\t%d\t", S.start_position, S.end_position);
        else snprintf(line, sizeof line, "\t%c\t%d\t%d\t", rc[S.read] ? '-' : '+', S.start_position, S.end_position);
        text += line;
        text += read_names[S.read];
        snprintf(line, sizeof line, "\t%.2lf\t%.2lf\t%.2lf\t%d\t%d\t", diff, sum_ll_m, sum_ll_u, 1, S.n_cpg);
        text += line;
        const char *seg = ref_arena + ref_off[S.read] + S.ctx_off;
        for (int32_t i = 0; i < S.ctx_len; ++i) text += possible0((char)toupper((unsigned char)seg[i]));      /* ss.sequence: of ref_seq, meth.c:288-306 */
        text += "\n";
    }
    *n_bytes = (int64_t)text.size();
    if ((int64_t)text.size() > cap) { set_error("%s: %lld bytes of text, room for %lld", who, (long long)text.size(), (long long)cap); return GBX_ERR_ARG; }
    if (!text.empty()) { if (!out) { set_error("%s: null pointer", who); return GBX_ERR_ARG; } memcpy(out, text.data(), text.size()); }
    return GBX_OK;
}

}  // extern "C"
