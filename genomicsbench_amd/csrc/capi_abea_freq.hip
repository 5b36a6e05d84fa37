// capi_abea_freq.hip — abea methylation frequency (f5c meth-freq, freq.c): the entries of the C-ABI (include/gbx.h) over
// abea_freq_kernels.hip, and the host-only reader of the call-methylation TSV.
#include "capi_common.h"
#include "abea_freq_rules.h"
#include <map>

using namespace gbx;

namespace {

namespace R = abea_freq_rules;

int bits_for(int64_t v) { int b = 1; while (b < 31 && (v >> b)) ++b; return b; }

int up(void *dst, const void *src, size_t n, hipStream_t s)
{
    if (n) GBX_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s));
    return GBX_OK;
}
int down(void *dst, const void *src, size_t n, hipStream_t s)                   // synchronises
{
    if (n) GBX_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

int refuse_flags(const char *who, const int64_t *counts)
{
    const int64_t f = counts[4];
    if (f & GBX_ABEA_FREQ_SUM_OVERFLOW) { set_error("%s: a site's called_sites is above INT32_MAX (the reference's int overflows)", who); return GBX_ERR_UNSUPPORTED; }
    if (f & GBX_ABEA_FREQ_POS_OVERFLOW) { set_error("%s: a split position is above INT32_MAX", who); return GBX_ERR_UNSUPPORTED; }
    if (f) { set_error("%s: the device flagged its input (flags %lld)", who, (long long)f); return GBX_ERR_ARG; }
    return GBX_OK;
}

// the table's sizes against the caller's room, then the fill's downloads
int deliver(const char *who, const int64_t *counts, int64_t site_cap, gbx_abea_freq_site *sites, int64_t *n_sites, int64_t seq_cap, char *seq_arena,
            int64_t *seq_bytes)
{
    *n_sites = counts[2]; *seq_bytes = counts[3];
    if (*n_sites > site_cap || *seq_bytes > seq_cap) {
        set_error("%s: %lld sites and %lld sequence bytes, room for %lld and %lld", who, (long long)*n_sites, (long long)*seq_bytes, (long long)site_cap,
                  (long long)seq_cap);
        return GBX_ERR_ARG;
    }
    if ((*n_sites > 0 && !sites) || (*seq_bytes > 0 && !seq_arena)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    return GBX_OK;
}

bool bad_pass(int pass, int allowed) { return pass < 1 || (pass & ~allowed); }

// strtok over one line: the next run of bytes outside `delim` at or after *at (nullptr: none), terminated in place
char *next_token(char *line, size_t len, size_t *at, const char *delim)
{
    size_t i = *at;
    while (i < len && strchr(delim, line[i])) ++i;
    if (i >= len) { *at = len; return nullptr; }
    const size_t b = i;
    while (i < len && !strchr(delim, line[i])) ++i;
    if (i < len) { line[i] = 0; *at = i + 1; } else *at = len;
    return line + b;
}

const char *const IN_HEADERS[4] = {
    "chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_cpgs\tsequence\n",
    "chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_motifs\tsequence\n",
    "chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_cpgs\tsequence\n",
    "chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_motifs\tsequence\n"};

}  // namespace

extern "C" {

int64_t gbx_abea_freq_work(int64_t n_records, int64_t n_items)
{
    if (n_records < 0 || n_items < 0) return 0;
    return (int64_t)abea_freq_work_bytes(n_records, n_items);
}

int gbx_abea_freq_device(int pass, int64_t n_records, const gbx_abea_freq_record *d_records, const char *d_rec_arena, double threshold, int split_groups,
                         int pos_bits, int contig_bits, int64_t n_items, void *d_work, int64_t *d_item_off, int64_t *d_counts, int64_t site_cap,
                         gbx_abea_freq_site *d_sites, int64_t seq_cap, char *d_seq_arena, void *stream)
{
    const char *who = "gbx_abea_freq_device";
    const int all = GBX_ABEA_FREQ_COUNT | GBX_ABEA_FREQ_REDUCE | GBX_ABEA_FREQ_FILL;
    if (bad_pass(pass, all) || n_records < 0 || n_items < 0 || site_cap < 0 || seq_cap < 0 || pos_bits < 1 || pos_bits > 31 || contig_bits < 1 || contig_bits > 31) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if ((pass & GBX_ABEA_FREQ_COUNT) && (pass & ~GBX_ABEA_FREQ_COUNT)) { set_error("%s: the count pass runs alone (n_items is its result)", who); return GBX_ERR_ARG; }
    if (!d_work || !d_item_off || !d_counts || (n_records > 0 && (!d_records || !d_rec_arena)) ||
        ((pass & GBX_ABEA_FREQ_FILL) && ((site_cap > 0 && !d_sites) || (seq_cap > 0 && !d_seq_arena)))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_freq_launch(pass, n_records, d_records, d_rec_arena, threshold, split_groups, pos_bits, contig_bits, n_items, d_work, d_item_off, d_counts,
                            site_cap, d_sites, seq_cap, d_seq_arena, (hipStream_t)stream);
}

int gbx_abea_freq_host(int64_t n_records, const gbx_abea_freq_record *records, const char *rec_arena, int64_t rec_arena_bytes, double threshold,
                       int split_groups, int64_t site_cap, gbx_abea_freq_site *sites, int64_t *n_sites, int64_t seq_cap, char *seq_arena, int64_t *seq_bytes)
{
    const char *who = "gbx_abea_freq_host";
    RoctxRange range_(who);
    if (n_records < 0 || rec_arena_bytes < 0 || site_cap < 0 || seq_cap < 0 || !n_sites || !seq_bytes) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    *n_sites = *seq_bytes = 0;
    if (n_records == 0) return GBX_OK;
    if (!records || (rec_arena_bytes > 0 && !rec_arena)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (n_records > 0x7fffffffLL - 1024) { set_error("%s: more than 2^31 records in one call", who); return GBX_ERR_UNSUPPORTED; }
    int64_t max_pos = 0, max_contig = 0;
    for (int64_t r = 0; r < n_records; ++r) {
        const gbx_abea_freq_record &c = records[r];
        if (c.contig < 0 || c.start < 0 || c.end < 0 || c.n_cpg < 0) { set_error("%s: record %lld has a negative contig, coordinate or count", who, (long long)r); return GBX_ERR_ARG; }
        if (c.seq_len < 0 || c.seq_off < 0 || c.seq_off + c.seq_len > rec_arena_bytes) {
            set_error("%s: the sequence of record %lld lies outside the arena", who, (long long)r);
            return GBX_ERR_ARG;
        }
        const int64_t reach = R::splits(split_groups, c.n_cpg) ? std::min<int64_t>((int64_t)c.start + c.seq_len, 0x7fffffffLL) : 0;
        max_pos = std::max<int64_t>(max_pos, std::max<int64_t>(std::max<int64_t>(c.start, c.end), reach));
        max_contig = std::max<int64_t>(max_contig, c.contig);
    }
    const int pos_bits = bits_for(max_pos), contig_bits = bits_for(max_contig);
    int rc = require_device();
    if (rc) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    DevBuf drec(L), dar(L), doff(L), dcnt(L), dwork0(L), dwork(L), dsites(L), dseq(L);
    if ((rc = drec.alloc((size_t)n_records * sizeof(gbx_abea_freq_record))) || (rc = dar.alloc((size_t)rec_arena_bytes)) ||
        (rc = doff.alloc((size_t)(n_records + 1) * 8)) || (rc = dcnt.alloc(GBX_ABEA_FREQ_NCOUNTS * 8)) || (rc = dwork0.alloc(abea_freq_work_bytes(n_records, 0))))
        return rc;
    if ((rc = up(drec.p, records, (size_t)n_records * sizeof(gbx_abea_freq_record), s)) || (rc = up(dar.p, rec_arena, (size_t)rec_arena_bytes, s))) return rc;
    int64_t counts[GBX_ABEA_FREQ_NCOUNTS] = {0};
    auto run = [&](int pass, int64_t n_items, void *work, int64_t scap, int64_t bcap) {
        return abea_freq_launch(pass, n_records, drec.as<gbx_abea_freq_record>(), dar.as<char>(), threshold, split_groups, pos_bits, contig_bits, n_items, work,
                                doff.as<int64_t>(), dcnt.as<int64_t>(), scap, dsites.as<gbx_abea_freq_site>(), bcap, dseq.as<char>(), s);
    };
    if ((rc = run(GBX_ABEA_FREQ_COUNT, 0, dwork0.p, 0, 0)) || (rc = down(counts, dcnt.p, 8, s))) return rc;
    const int64_t n_items = counts[0];
    if (n_items > 0x7fffffffLL - 1024) { set_error("%s: more than 2^31 items in one call", who); return GBX_ERR_UNSUPPORTED; }
    if ((rc = dwork.alloc(abea_freq_work_bytes(n_records, n_items))) || (rc = run(GBX_ABEA_FREQ_REDUCE, n_items, dwork.p, 0, 0)) ||
        (rc = down(counts, dcnt.p, sizeof counts, s)) || (rc = refuse_flags(who, counts)) ||
        (rc = deliver(who, counts, site_cap, sites, n_sites, seq_cap, seq_arena, seq_bytes)))
        return rc;
    if (*n_sites == 0) return GBX_OK;
    if ((rc = dsites.alloc((size_t)*n_sites * sizeof(gbx_abea_freq_site))) || (rc = dseq.alloc((size_t)*seq_bytes)) ||
        (rc = run(GBX_ABEA_FREQ_FILL, n_items, dwork.p, *n_sites, *seq_bytes)))
        return rc;
    if (*seq_bytes) GBX_HIP(hipMemcpyAsync(seq_arena, dseq.p, (size_t)*seq_bytes, hipMemcpyDeviceToHost, s));
    return down(sites, dsites.p, (size_t)*n_sites * sizeof(gbx_abea_freq_site), s);
}

int64_t gbx_abea_freq_records_work(int64_t n_sites) { return n_sites < 0 ? 0 : (int64_t)abea_freq_records_work_bytes(n_sites); }

int gbx_abea_freq_records_device(int pass, int64_t n_sites, const gbx_abea_meth_site *d_sites, const float *d_scores, int64_t n_reads,
                                 const int32_t *d_contig_of_read, const int64_t *d_ref_off, const int32_t *d_ref_len, const char *d_ref_arena,
                                 int32_t clip_start, int32_t clip_end, void *d_work, int64_t *d_off, int64_t rec_cap, gbx_abea_freq_record *d_records,
                                 int64_t seq_cap, char *d_seq_arena, void *stream)
{
    const char *who = "gbx_abea_freq_records_device";
    if (bad_pass(pass, GBX_ABEA_FREQ_COUNT | GBX_ABEA_FREQ_FILL) || n_sites < 0 || n_reads < 0 || rec_cap < 0 || seq_cap < 0) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!d_work || !d_off || (n_sites > 0 && (!d_sites || !d_scores || !d_contig_of_read || !d_ref_off || !d_ref_len || !d_ref_arena)) ||
        ((pass & GBX_ABEA_FREQ_FILL) && ((rec_cap > 0 && !d_records) || (seq_cap > 0 && !d_seq_arena)))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_freq_records_launch(pass, n_sites, d_sites, d_scores, n_reads, d_contig_of_read, d_ref_off, d_ref_len, d_ref_arena, clip_start, clip_end, d_work,
                                    d_off, rec_cap, d_records, seq_cap, d_seq_arena, (hipStream_t)stream);
}

int gbx_abea_freq_records_host(int64_t n_sites, const gbx_abea_meth_site *sites, const float *scores, int64_t n_reads, const int32_t *contig_of_read,
                               const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena, int32_t clip_start, int32_t clip_end, int64_t rec_cap,
                               gbx_abea_freq_record *records, int64_t *n_records, int64_t seq_cap, char *seq_arena, int64_t *seq_bytes)
{
    const char *who = "gbx_abea_freq_records_host";
    RoctxRange range_(who);
    if (n_sites < 0 || n_reads < 0 || rec_cap < 0 || seq_cap < 0 || !n_records || !seq_bytes) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    *n_records = *seq_bytes = 0;
    if (n_sites == 0) return GBX_OK;
    if (!sites || !scores || !contig_of_read || !ref_off || !ref_len || !ref_arena || n_reads == 0) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (n_sites > 0x7fffffffLL - 1024) { set_error("%s: more than 2^31 sites in one call", who); return GBX_ERR_UNSUPPORTED; }
    int64_t ref_bytes = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (ref_off[r] < 0 || ref_len[r] < 0 || contig_of_read[r] < 0) { set_error("%s: read %lld has a negative offset, length or contig", who, (long long)r); return GBX_ERR_ARG; }
        ref_bytes = std::max<int64_t>(ref_bytes, ref_off[r] + ref_len[r]);
    }
    for (int64_t k = 0; k < n_sites; ++k) {
        const gbx_abea_meth_site &S = sites[k];
        if (S.read < 0 || S.read >= n_reads) { set_error("%s: site %lld names read %d", who, (long long)k, S.read); return GBX_ERR_ARG; }
        if (S.ctx_len < 0 || S.ctx_off < 0 || S.ctx_off + S.ctx_len > ref_len[S.read]) {
            set_error("%s: the context of site %lld lies outside its reference segment", who, (long long)k);
            return GBX_ERR_ARG;
        }
    }
    int rc = require_device();
    if (rc) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    DevBuf dsi(L), dsc(L), dco(L), dro(L), drl(L), dra(L), dwork(L), doff(L), drec(L), dseq(L);
    if ((rc = dsi.alloc((size_t)n_sites * sizeof(gbx_abea_meth_site))) || (rc = dsc.alloc((size_t)n_sites * 8)) || (rc = dco.alloc((size_t)n_reads * 4)) ||
        (rc = dro.alloc((size_t)n_reads * 8)) || (rc = drl.alloc((size_t)n_reads * 4)) || (rc = dra.alloc((size_t)ref_bytes)) ||
        (rc = dwork.alloc(abea_freq_records_work_bytes(n_sites))) || (rc = doff.alloc((size_t)(n_sites + 1) * 16)))
        return rc;
    if ((rc = up(dsi.p, sites, (size_t)n_sites * sizeof(gbx_abea_meth_site), s)) || (rc = up(dsc.p, scores, (size_t)n_sites * 8, s)) ||
        (rc = up(dco.p, contig_of_read, (size_t)n_reads * 4, s)) || (rc = up(dro.p, ref_off, (size_t)n_reads * 8, s)) ||
        (rc = up(drl.p, ref_len, (size_t)n_reads * 4, s)) || (rc = up(dra.p, ref_arena, (size_t)ref_bytes, s)))
        return rc;
    auto run = [&](int pass, int64_t rcap, int64_t bcap) {
        return abea_freq_records_launch(pass, n_sites, dsi.as<gbx_abea_meth_site>(), dsc.as<float>(), n_reads, dco.as<int32_t>(), dro.as<int64_t>(),
                                        drl.as<int32_t>(), dra.as<char>(), clip_start, clip_end, dwork.p, doff.as<int64_t>(), rcap,
                                        drec.as<gbx_abea_freq_record>(), bcap, dseq.as<char>(), s);
    };
    int64_t tot[2] = {0, 0};
    if ((rc = run(GBX_ABEA_FREQ_COUNT, 0, 0))) return rc;
    GBX_HIP(hipMemcpyAsync(&tot[0], doff.as<int64_t>() + n_sites, 8, hipMemcpyDeviceToHost, s));
    if ((rc = down(&tot[1], doff.as<int64_t>() + 2 * n_sites + 1, 8, s))) return rc;
    *n_records = tot[0]; *seq_bytes = tot[1];
    if (tot[0] > rec_cap || tot[1] > seq_cap) {
        set_error("%s: %lld records and %lld sequence bytes, room for %lld and %lld", who, (long long)tot[0], (long long)tot[1], (long long)rec_cap, (long long)seq_cap);
        return GBX_ERR_ARG;
    }
    if ((tot[0] > 0 && !records) || (tot[1] > 0 && !seq_arena)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (tot[0] == 0) return GBX_OK;
    if ((rc = drec.alloc((size_t)tot[0] * sizeof(gbx_abea_freq_record))) || (rc = dseq.alloc((size_t)tot[1])) || (rc = run(GBX_ABEA_FREQ_FILL, tot[0], tot[1]))) return rc;
    if (tot[1]) GBX_HIP(hipMemcpyAsync(seq_arena, dseq.p, (size_t)tot[1], hipMemcpyDeviceToHost, s));
    return down(records, drec.p, (size_t)tot[0] * sizeof(gbx_abea_freq_record), s);
}

int gbx_abea_freq_merge_device(int pass, int64_t n_a, const gbx_abea_freq_site *d_sites_a, const char *d_arena_a, int64_t n_b,
                               const gbx_abea_freq_site *d_sites_b, const char *d_arena_b, int pos_bits, int contig_bits, void *d_work, int64_t *d_counts,
                               int64_t site_cap, gbx_abea_freq_site *d_sites, int64_t seq_cap, char *d_seq_arena, void *stream)
{
    const char *who = "gbx_abea_freq_merge_device";
    if (bad_pass(pass, GBX_ABEA_FREQ_REDUCE | GBX_ABEA_FREQ_FILL) || n_a < 0 || n_b < 0 || site_cap < 0 || seq_cap < 0 || pos_bits < 1 || pos_bits > 31 ||
        contig_bits < 1 || contig_bits > 31) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!d_work || !d_counts || (n_a > 0 && (!d_sites_a || !d_arena_a)) || (n_b > 0 && (!d_sites_b || !d_arena_b)) ||
        ((pass & GBX_ABEA_FREQ_FILL) && ((site_cap > 0 && !d_sites) || (seq_cap > 0 && !d_seq_arena)))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_freq_merge_launch(pass, n_a, d_sites_a, d_arena_a, n_b, d_sites_b, d_arena_b, pos_bits, contig_bits, d_work, d_counts, site_cap, d_sites, seq_cap,
                                  d_seq_arena, (hipStream_t)stream);
}

static int check_table(const char *who, const char *which, int64_t n, const gbx_abea_freq_site *t, int64_t arena_bytes, int64_t n_contigs, int64_t *max_pos,
                       int64_t *max_contig)
{
    for (int64_t k = 0; k < n; ++k) {
        const gbx_abea_freq_site &S = t[k];
        if (S.contig < 0 || (n_contigs >= 0 && S.contig >= n_contigs) || S.start < 0 || S.end < 0 || S.group_size < 0 || S.called_sites <= 0 ||
            S.called_sites_methylated < 0 || S.called_sites_methylated > S.called_sites) {
            set_error("%s: site %lld of %s is not a site of a table", who, (long long)k, which);
            return GBX_ERR_ARG;
        }
        if (S.seq_len < -1 || (S.seq_len >= 0 && (S.seq_off < 0 || S.seq_off + S.seq_len > arena_bytes))) {
            set_error("%s: the sequence of site %lld of %s lies outside its arena", who, (long long)k, which);
            return GBX_ERR_ARG;
        }
        if (max_pos) *max_pos = std::max<int64_t>(*max_pos, std::max(S.start, S.end));
        if (max_contig) *max_contig = std::max<int64_t>(*max_contig, S.contig);
    }
    return GBX_OK;
}

int gbx_abea_freq_merge_host(int64_t n_a, const gbx_abea_freq_site *sites_a, const char *arena_a, int64_t arena_a_bytes, int64_t n_b,
                             const gbx_abea_freq_site *sites_b, const char *arena_b, int64_t arena_b_bytes, int64_t site_cap, gbx_abea_freq_site *sites,
                             int64_t *n_sites, int64_t seq_cap, char *seq_arena, int64_t *seq_bytes)
{
    const char *who = "gbx_abea_freq_merge_host";
    RoctxRange range_(who);
    if (n_a < 0 || n_b < 0 || arena_a_bytes < 0 || arena_b_bytes < 0 || site_cap < 0 || seq_cap < 0 || !n_sites || !seq_bytes) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    *n_sites = *seq_bytes = 0;
    const int64_t n = n_a + n_b;
    if (n == 0) return GBX_OK;
    if ((n_a > 0 && !sites_a) || (n_b > 0 && !sites_b) || (arena_a_bytes > 0 && !arena_a) || (arena_b_bytes > 0 && !arena_b)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if (n > 0x7fffffffLL - 1024) { set_error("%s: more than 2^31 sites in one call", who); return GBX_ERR_UNSUPPORTED; }
    int64_t max_pos = 0, max_contig = 0;
    int rc;
    if ((rc = check_table(who, "the first table", n_a, sites_a, arena_a_bytes, -1, &max_pos, &max_contig)) ||
        (rc = check_table(who, "the second table", n_b, sites_b, arena_b_bytes, -1, &max_pos, &max_contig)))
        return rc;
    const int pos_bits = bits_for(max_pos), contig_bits = bits_for(max_contig);
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    DevBuf dsa(L), daa(L), dsb(L), dab(L), dcnt(L), dwork(L), dsites(L), dseq(L);
    const size_t ss = sizeof(gbx_abea_freq_site);
    if ((rc = dsa.alloc((size_t)n_a * ss)) || (rc = daa.alloc((size_t)arena_a_bytes)) || (rc = dsb.alloc((size_t)n_b * ss)) || (rc = dab.alloc((size_t)arena_b_bytes)) ||
        (rc = dcnt.alloc(GBX_ABEA_FREQ_NCOUNTS * 8)) || (rc = dwork.alloc(abea_freq_work_bytes(n, n))))
        return rc;
    if ((rc = up(dsa.p, sites_a, (size_t)n_a * ss, s)) || (rc = up(daa.p, arena_a, (size_t)arena_a_bytes, s)) || (rc = up(dsb.p, sites_b, (size_t)n_b * ss, s)) ||
        (rc = up(dab.p, arena_b, (size_t)arena_b_bytes, s)))
        return rc;
    auto run = [&](int pass, int64_t scap, int64_t bcap) {
        return abea_freq_merge_launch(pass, n_a, dsa.as<gbx_abea_freq_site>(), daa.as<char>(), n_b, dsb.as<gbx_abea_freq_site>(), dab.as<char>(), pos_bits, contig_bits,
                                      dwork.p, dcnt.as<int64_t>(), scap, dsites.as<gbx_abea_freq_site>(), bcap, dseq.as<char>(), s);
    };
    int64_t counts[GBX_ABEA_FREQ_NCOUNTS] = {0};
    if ((rc = run(GBX_ABEA_FREQ_REDUCE, 0, 0)) || (rc = down(counts, dcnt.p, sizeof counts, s)) || (rc = refuse_flags(who, counts)) ||
        (rc = deliver(who, counts, site_cap, sites, n_sites, seq_cap, seq_arena, seq_bytes)))
        return rc;
    if (*n_sites == 0) return GBX_OK;
    if ((rc = dsites.alloc((size_t)*n_sites * ss)) || (rc = dseq.alloc((size_t)*seq_bytes)) || (rc = run(GBX_ABEA_FREQ_FILL, *n_sites, *seq_bytes))) return rc;
    if (*seq_bytes) GBX_HIP(hipMemcpyAsync(seq_arena, dseq.p, (size_t)*seq_bytes, hipMemcpyDeviceToHost, s));
    return down(sites, dsites.p, (size_t)*n_sites * ss, s);
}

int64_t gbx_abea_freq_tsv_work(int64_t n_sites) { return n_sites < 0 ? 0 : (int64_t)abea_freq_tsv_work_bytes(n_sites); }

int gbx_abea_freq_tsv_device(int pass, int64_t n_sites, const gbx_abea_freq_site *d_sites, const char *d_seq_arena, int64_t n_contigs, const int64_t *d_name_off,
                             const char *d_names, int header_kind, int with_header, void *d_work, int64_t *d_line_off, int64_t cap, char *d_out, void *stream)
{
    const char *who = "gbx_abea_freq_tsv_device";
    if (bad_pass(pass, GBX_ABEA_FREQ_COUNT | GBX_ABEA_FREQ_FILL) || n_sites < 0 || n_contigs < 0 || cap < 0 ||
        (header_kind != GBX_ABEA_FREQ_CPGS && header_kind != GBX_ABEA_FREQ_MOTIFS)) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!d_work || !d_line_off || (n_sites > 0 && (!d_sites || !d_seq_arena || !d_name_off || !d_names)) || ((pass & GBX_ABEA_FREQ_FILL) && cap > 0 && !d_out)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return abea_freq_tsv_launch(pass, n_sites, d_sites, d_seq_arena, n_contigs, d_name_off, d_names, header_kind, with_header, d_work, d_line_off, cap, d_out,
                                (hipStream_t)stream);
}

int gbx_abea_freq_tsv_host(int64_t n_sites, const gbx_abea_freq_site *sites, const char *seq_arena, int64_t seq_bytes, int64_t n_contigs,
                           const char *const *contig_names, int header_kind, int with_header, int64_t cap, char *out, int64_t *n_bytes)
{
    const char *who = "gbx_abea_freq_tsv_host";
    RoctxRange range_(who);
    if (n_sites < 0 || seq_bytes < 0 || n_contigs < 0 || cap < 0 || !n_bytes || (header_kind != GBX_ABEA_FREQ_CPGS && header_kind != GBX_ABEA_FREQ_MOTIFS)) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    *n_bytes = 0;
    if ((n_sites > 0 && (!sites || !contig_names)) || (seq_bytes > 0 && !seq_arena)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (n_sites > 0x7fffffffLL - 1024) { set_error("%s: more than 2^31 sites in one call", who); return GBX_ERR_UNSUPPORTED; }
    std::vector<int64_t> name_off((size_t)n_contigs + 1, 0);
    for (int64_t c = 0; c < n_contigs; ++c) {
        if (n_sites > 0 && !contig_names[c]) { set_error("%s: contig %lld has no name", who, (long long)c); return GBX_ERR_ARG; }
        name_off[(size_t)c + 1] = name_off[(size_t)c] + (n_sites > 0 ? (int64_t)strlen(contig_names[c]) : 0);
    }
    int rc;
    if ((rc = check_table(who, "the table", n_sites, sites, seq_bytes, n_contigs, nullptr, nullptr))) return rc;
    std::string names;
    names.reserve((size_t)name_off[(size_t)n_contigs]);
    for (int64_t c = 0; c < n_contigs && n_sites > 0; ++c) names += contig_names[c];
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    DevBuf dsi(L), dar(L), dno(L), dna(L), dwork(L), dlo(L), dout(L);
    const size_t ss = sizeof(gbx_abea_freq_site);
    if ((rc = dsi.alloc((size_t)n_sites * ss)) || (rc = dar.alloc((size_t)seq_bytes)) || (rc = dno.alloc(name_off.size() * 8)) || (rc = dna.alloc(names.size())) ||
        (rc = dwork.alloc(abea_freq_tsv_work_bytes(n_sites))) || (rc = dlo.alloc((size_t)(n_sites + 2) * 8)))
        return rc;
    if ((rc = up(dsi.p, sites, (size_t)n_sites * ss, s)) || (rc = up(dar.p, seq_arena, (size_t)seq_bytes, s)) || (rc = up(dno.p, name_off.data(), name_off.size() * 8, s)) ||
        (rc = up(dna.p, names.data(), names.size(), s)))
        return rc;
    auto run = [&](int pass, int64_t room) {
        return abea_freq_tsv_launch(pass, n_sites, dsi.as<gbx_abea_freq_site>(), dar.as<char>(), n_contigs, dno.as<int64_t>(), dna.as<char>(), header_kind, with_header,
                                    dwork.p, dlo.as<int64_t>(), room, dout.as<char>(), s);
    };
    if ((rc = run(GBX_ABEA_FREQ_COUNT, 0)) || (rc = down(n_bytes, dlo.as<int64_t>() + n_sites + 1, 8, s))) return rc;
    if (*n_bytes > cap) { set_error("%s: %lld bytes of text, room for %lld", who, (long long)*n_bytes, (long long)cap); return GBX_ERR_ARG; }
    if (*n_bytes == 0) return GBX_OK;
    if (!out) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = dout.alloc((size_t)*n_bytes)) || (rc = run(GBX_ABEA_FREQ_FILL, *n_bytes))) return rc;
    return down(out, dout.p, (size_t)*n_bytes, s);
}

int gbx_abea_freq_parse_host(const char *text, int64_t n_bytes, int64_t rec_cap, gbx_abea_freq_record *records, int64_t seq_cap, char *seq_arena,
                             int64_t name_cap, char *names, int64_t *counts, int *header_kind, int64_t *bad_line)
{
    const char *who = "gbx_abea_freq_parse_host";
    if (n_bytes < 0 || rec_cap < 0 || seq_cap < 0 || name_cap < 0 || !counts || !header_kind || !bad_line || (n_bytes > 0 && !text)) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    *header_kind = 0;
    *bad_line = 0;
    const char *const end = text + n_bytes;
    auto line_end = [&](const char *p) { const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p)); return nl ? nl + 1 : end; };    // getline: through the '\n'
    if (n_bytes == 0) { set_error("Bad file format with no header?\n"); return GBX_ERR_ARG; }
    const char *p = line_end(text);
    const std::string head(text, (size_t)(p - text));
    int version = 0;
    for (int h = 0; h < 4; ++h)
        if (head == IN_HEADERS[h]) { version = h < 2 ? 1 : 2; *header_kind = (h & 1) ? GBX_ABEA_FREQ_MOTIFS : GBX_ABEA_FREQ_CPGS; }
    if (!version) { set_error("Incorrect header: %s\n", std::string(head.c_str()).c_str()); return GBX_ERR_ARG; }
    struct Row { int32_t start, end, n_cpg; double llr; int64_t seq_off; int32_t seq_len; const std::pair<const std::string, int32_t> *contig; };
    std::vector<Row> rows;
    std::map<std::string, int32_t> rank;
    std::string arena, line;
    int64_t line_num = 2;                                                                    // freq.c:335-336
    auto fail = [&](const char *fmt) { *bad_line = line_num; set_error(fmt, (long)line_num); return GBX_ERR_ARG; };
    while (p < end) {
        const char *q = line_end(p);
        line.assign(p, (size_t)(q - p));
        p = q;
        const size_t len = strlen(line.c_str());                                             // the C string: what strtok sees
        char *buf = &line[0];
        size_t at = 0;
        const char *corrupted = "Corrupted tsv file? Offending line is line number %ld (1-based index)\n";
        Row row;
        char *tok = next_token(buf, len, &at, "\t");
        if (!tok) return fail(corrupted);
        const std::string chrom(tok);
        if (version == 2 && !next_token(buf, len, &at, "\t")) return fail(corrupted);        // strand: ignored
        if (!(tok = next_token(buf, len, &at, "\t"))) return fail(corrupted);
        row.start = (int32_t)strtol(tok, nullptr, 10);
        if (!(tok = next_token(buf, len, &at, "\t"))) return fail(corrupted);
        row.end = (int32_t)strtol(tok, nullptr, 10);
        if (row.start < 0 || row.end < 0) return fail("chromosome coordinates cannot be negative. Offending line is line number %ld (1-based index)\n");
        if (!next_token(buf, len, &at, "\t")) return fail(corrupted);                        // read name
        if (!(tok = next_token(buf, len, &at, "\t"))) return fail(corrupted);
        row.llr = strtod(tok, nullptr);
        next_token(buf, len, &at, "\t");                                                     // log_lik_methylated
        next_token(buf, len, &at, "\t");                                                     // log_lik_unmethylated
        if (!next_token(buf, len, &at, "\t")) return fail(corrupted);                        // num_calling_strands
        if (!(tok = next_token(buf, len, &at, "\t"))) return fail(corrupted);
        row.n_cpg = (int32_t)strtol(tok, nullptr, 10);
        if (row.n_cpg < 0) return fail("num_cpgs cannot be negative. Offending line is line number %ld (1-based index)\n");
        if (!(tok = next_token(buf, len, &at, "\t\n"))) return fail(corrupted);
        const size_t sl = strlen(tok);
        if (sl > 0x7fffffffu) { set_error("%s: a sequence of 2^31 bytes", who); return GBX_ERR_UNSUPPORTED; }
        row.seq_off = (int64_t)arena.size(); row.seq_len = (int32_t)sl;
        arena.append(tok, sl);
        if (next_token(buf, len, &at, "\t\n")) return fail("encountered more columns than expected. Offending line is line number %ld (1-based index)\n");
        if (chrom.find_first_of(":\t\n") != std::string::npos) {
            *bad_line = line_num;
            set_error("%s: the contig name of line %lld holds ':', a tab or a newline", who, (long long)line_num);
            return GBX_ERR_UNSUPPORTED;
        }
        row.contig = &*rank.emplace(chrom, 0).first;
        rows.push_back(row);
        line_num++;
    }
    if (rows.size() > (size_t)0x7fffffff - 1024) { set_error("%s: more than 2^31 records", who); return GBX_ERR_UNSUPPORTED; }
    int64_t name_bytes = 0;
    int32_t k = 0;
    for (auto &e : rank) { e.second = k++; name_bytes += (int64_t)e.first.size() + 1; }      // std::string orders as strcmp does: unsigned bytes
    counts[0] = (int64_t)rows.size(); counts[1] = (int64_t)arena.size(); counts[2] = (int64_t)rank.size(); counts[3] = name_bytes;
    if (counts[0] > rec_cap || counts[1] > seq_cap || counts[3] > name_cap) {
        *bad_line = -1;
        set_error("%s: %lld records, %lld sequence bytes and %lld name bytes, room for %lld, %lld and %lld", who, (long long)counts[0], (long long)counts[1],
                  (long long)counts[3], (long long)rec_cap, (long long)seq_cap, (long long)name_cap);
        return GBX_ERR_ARG;
    }
    if ((counts[0] > 0 && !records) || (counts[1] > 0 && !seq_arena) || (counts[3] > 0 && !names)) { *bad_line = -1; set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    for (size_t r = 0; r < rows.size(); ++r) {
        gbx_abea_freq_record &c = records[r];
        c.contig = rows[r].contig->second; c.start = rows[r].start; c.end = rows[r].end; c.n_cpg = rows[r].n_cpg; c.llr = rows[r].llr;
        c.seq_off = rows[r].seq_off; c.seq_len = rows[r].seq_len; c.pad_ = 0;
    }
    if (!arena.empty()) memcpy(seq_arena, arena.data(), arena.size());
    char *o = names;
    for (auto &e : rank) { memcpy(o, e.first.c_str(), e.first.size() + 1); o += e.first.size() + 1; }
    return GBX_OK;
}

}  // extern "C"
