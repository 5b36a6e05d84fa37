// capi_mem_sam.hip — SAM-record entries of the C-ABI (include/gbx.h): the regions of the regs / paired stage and the CIGAR
// stage's answer for their list -> gbx_mem_sam_rec records, the MD bytes and the SAM text.
#include "capi_common.h"

using namespace gbx;

namespace {
int common_check(const gbx_mem_sam_params *p, int64_t n_reads, int32_t mode, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (p->softclip != 0 && p->softclip != 1) { set_error("%s: softclip = %d (0 or 1)", who, p->softclip); return GBX_ERR_ARG; }
    if (mode != 0 && mode != 1) { set_error("%s: mode = %d (0 or 1)", who, mode); return GBX_ERR_ARG; }
    if (n_reads < 0 || (mode == 1 && (n_reads & 1))) { set_error("%s: n_reads = %lld (at least 0, even in mode 1)", who, (long long)n_reads); return GBX_ERR_ARG; }
    return GBX_OK;
}
}  // namespace

extern "C" {

void gbx_mem_sam_default_params(gbx_mem_sam_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
}

size_t gbx_mem_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t n_alns)
{
    return mem_sam_workspace_bytes(n_reads, reg_cap, n_alns);
}

size_t gbx_mem_sam_text_cap(int64_t rec_cap, int64_t cigar_words, int64_t read_bytes, int64_t name_bytes, int32_t max_contig_name,
                            int32_t max_recs, int32_t max_del)
{
    const size_t R = (size_t)std::max<int64_t>(rec_cap, 0), W = (size_t)std::max<int64_t>(cigar_words, 0), C = (size_t)std::max(max_contig_name, 1);
    const size_t U = (size_t)std::max(max_recs, 1), D = (size_t)std::max(max_del, 0);
    // per record: the fixed fields and tag heads (192), RNAME and RNEXT, the other records' SA entries without their CIGARs, its
    // deleted bases; per read and record: the name, SEQ, QUAL and the M part of MD; per word: its text in CIGAR, MC, SA and MD
    return R * (192 + 2 * C + (U - 1) * (C + 64) + D) + U * ((size_t)std::max<int64_t>(name_bytes, 0) + 4 * (size_t)std::max<int64_t>(read_bytes, 0)) +
           (2 * U + 1) * 11 * W;
}

int gbx_mem_sam_device(const gbx_mem_sam_params *p, int64_t n_reads, int32_t mode,
                       const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                       const gbx_mem_pair *d_pairs,
                       const gbx_mem_aln *d_alns, int64_t n_alns, const uint32_t *d_cigar, const int64_t *d_n_cigar, int64_t cigar_cap,
                       const uint8_t *d_qer, int64_t qer_bytes, const int64_t *d_read_off, const int32_t *d_read_len, const uint8_t *d_qual,
                       const uint8_t *d_names, const int64_t *d_name_off, int64_t name_bytes,
                       const uint8_t *d_cnames, const int64_t *d_cname_off, int64_t cname_bytes,
                       const uint8_t *d_text, int64_t text_bytes, int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                       gbx_mem_sam_rec *d_recs, int64_t rec_cap, int64_t *d_rec_off, int64_t *d_n_recs,
                       uint8_t *d_md, int64_t md_cap, int64_t *d_n_md, uint8_t *d_lines, int64_t text_cap, int64_t *d_n_text,
                       void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mem_sam_device";
    int rc = common_check(p, n_reads, mode, who);
    if (rc) return rc;
    if (reg_cap < 0 || n_alns < 0 || cigar_cap < 0 || qer_bytes < 0 || name_bytes < 0 || cname_bytes < 0 || l_pac < 1 || n_contigs < 1 ||
        text_bytes < 2 * l_pac || rec_cap < 0 || md_cap < 0 || text_cap < 0) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!d_reg_off || !d_n_regs || !d_n_cigar || !d_read_off || !d_read_len || !d_name_off || !d_cname_off || !d_text || !d_contig_off ||
        !d_rec_off || !d_n_recs || !d_n_md || !d_n_text || !d_work || (reg_cap > 0 && !d_regs) || (mode == 1 && n_reads > 0 && !d_pairs) ||
        (n_alns > 0 && !d_alns) || (cigar_cap > 0 && !d_cigar) || (qer_bytes > 0 && !d_qer) || (name_bytes > 0 && !d_names) ||
        (cname_bytes > 0 && !d_cnames) || (rec_cap > 0 && !d_recs) || (md_cap > 0 && !d_md) || (text_cap > 0 && !d_lines)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MemSamIo io{d_regs, d_reg_off, d_n_regs, reg_cap, d_pairs, d_alns, n_alns, d_cigar, d_n_cigar, cigar_cap, d_qer, qer_bytes, d_read_off,
                      d_read_len, d_qual, d_names, d_name_off, name_bytes, d_cnames, d_cname_off, cname_bytes, d_text, text_bytes, l_pac,
                      n_contigs, d_contig_off, d_recs, rec_cap, d_rec_off, d_n_recs, d_md, md_cap, d_n_md, d_lines, text_cap, d_n_text};
    return mem_sam_launch(p, n_reads, mode, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mem_sam_host(const gbx_mem_sam_params *p, int64_t n_reads, int32_t mode,
                     const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs, const gbx_mem_pair *pairs,
                     const gbx_mem_aln *alns, int64_t n_alns, const uint32_t *cigar, int64_t n_cigar,
                     const uint8_t *qer, int64_t qer_bytes, const int64_t *read_off, const int32_t *read_len, const uint8_t *qual,
                     const uint8_t *names, const int64_t *name_off, int64_t name_bytes,
                     const uint8_t *cnames, const int64_t *cname_off, int64_t cname_bytes,
                     const uint8_t *text, int64_t text_bytes, int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                     gbx_mem_sam_rec *recs, int64_t rec_cap, int64_t *rec_off, int64_t *n_recs,
                     uint8_t *md, int64_t md_cap, int64_t *n_md, uint8_t *lines, int64_t text_cap, int64_t *n_text)
{
    RoctxRange range_("gbx_mem_sam_host");
    const char *who = "gbx_mem_sam_host";
    int rc = common_check(p, n_reads, mode, who);
    if (rc) return rc;
    if (n_regs < 0 || n_alns < 0 || n_cigar < 0 || qer_bytes < 0 || name_bytes < 0 || cname_bytes < 0 || l_pac < 1 || n_contigs < 1 ||
        rec_cap < 0 || md_cap < 0 || text_cap < 0) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (text_bytes < 2 * l_pac) { set_error("%s: text_bytes = %lld is below 2 l_pac", who, (long long)text_bytes); return GBX_ERR_ARG; }
    if (!reg_off || !read_off || !read_len || !name_off || !cname_off || !text || !contig_off || !rec_off || !n_recs || !n_md || !n_text ||
        (n_regs > 0 && !regs) || (mode == 1 && n_reads > 0 && !pairs) || (n_alns > 0 && !alns) || (n_cigar > 0 && !cigar) ||
        (qer_bytes > 0 && !qer) || (name_bytes > 0 && !names) || (cname_bytes > 0 && !cnames) || (rec_cap > 0 && !recs) || (md_cap > 0 && !md) ||
        (text_cap > 0 && !lines)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    // everything is checked before the device is touched
    if ((rc = contig_off_check(contig_off, n_contigs, l_pac, who))) return rc;
    if ((rc = offsets_check(reg_off, n_reads, n_regs, "reg_off", "regions", "read", who))) return rc;
    if ((rc = offsets_check(name_off, n_reads, name_bytes, "name_off", "name bytes", "read", who))) return rc;
    if ((rc = offsets_check(cname_off, n_contigs, cname_bytes, "cname_off", "contig name bytes", "contig", who))) return rc;
    for (int64_t r = 0; r < n_reads; ++r)
        if (read_len[r] < 1 || read_off[r] < 0 || read_off[r] > qer_bytes - read_len[r]) {
            set_error("%s: read %lld: offset %lld, length %d lies outside the %lld read bytes (at least one base)", who, (long long)r,
                      (long long)read_off[r], read_len[r], (long long)qer_bytes);
            return GBX_ERR_ARG;
        }
    for (int64_t r = 0; r < n_reads; ++r)
        for (int64_t g = reg_off[r]; g < reg_off[r + 1]; ++g) {
            if (!(regs[g].flag & 1)) continue;
            if (regs[g].sel < 0 || regs[g].sel >= n_alns) {
                set_error("%s: region %lld: sel = %d lies outside the %lld alignments", who, (long long)g, regs[g].sel, (long long)n_alns);
                return GBX_ERR_ARG;
            }
            const gbx_mem_aln &a = alns[regs[g].sel];
            if (a.rid < 0 || a.rid >= n_contigs) {
                set_error("%s: region %lld: its alignment's rid = %d lies outside the %d contigs", who, (long long)g, a.rid, n_contigs);
                return GBX_ERR_ARG;
            }
            if (a.n_cigar < 1 || a.cigar_off < 0 || a.cigar_off > n_cigar - a.n_cigar) {
                set_error("%s: region %lld: its CIGAR words lie outside the %lld words", who, (long long)g, (long long)n_cigar);
                return GBX_ERR_ARG;
            }
            int64_t ql = 0, rl = 0;
            for (int k = 0; k < a.n_cigar; ++k) {
                const uint32_t w = cigar[a.cigar_off + k];
                const int op = (int)(w & 15u);
                if (op != 0 && op != 1 && op != 2 && op != 4) {
                    set_error("%s: region %lld: CIGAR op %d (M, I, D and S only)", who, (long long)g, op);
                    return GBX_ERR_ARG;
                }
                if (op != 2) ql += w >> 4;
                if (op == 0 || op == 2) rl += w >> 4;
            }
            if (ql != read_len[r] || a.pos < 0 || a.pos + rl > contig_off[a.rid + 1] - contig_off[a.rid]) {
                set_error("%s: region %lld: its CIGAR covers %lld read bases of %d and ends at %lld on a contig of %lld", who, (long long)g,
                          (long long)ql, read_len[r], (long long)(a.pos + rl), (long long)(contig_off[a.rid + 1] - contig_off[a.rid]));
                return GBX_ERR_ARG;
            }
        }
    *n_recs = *n_md = *n_text = 0;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    const int64_t rmax = mem_sam_rec_max(n_reads, n_regs, n_alns);
    const int64_t rcap = std::min(rec_cap, rmax);
    DevBuf drg(L), dro(L), dpa(L), dal(L), dcg(L), dq(L), dqo(L), dql(L), dqu(L), dnm(L), dno(L), dcn(L), dcno(L), dtx(L), dco(L), dn(L),
           drec(L), drof(L), dmd(L), dli(L), dw(L);
    const size_t wb = mem_sam_workspace_bytes(n_reads, n_regs, n_alns);
    // of the text the stage reads the forward strand only: [0, l_pac) goes up
    const int64_t counts[5] = {n_regs, n_cigar, 0, 0, 0};
    if ((rc = upload(drg, regs, (size_t)n_regs * sizeof(gbx_mem_reg), st)) || (rc = upload(dro, reg_off, (size_t)(n_reads + 1) * 8, st)) ||
        (rc = upload(dpa, pairs, mode == 1 ? (size_t)(n_reads / 2) * sizeof(gbx_mem_pair) : 0, st)) ||
        (rc = upload(dal, alns, (size_t)n_alns * sizeof(gbx_mem_aln), st)) || (rc = upload(dcg, cigar, (size_t)n_cigar * 4, st)) ||
        (rc = upload(dq, qer, (size_t)qer_bytes, st)) || (rc = upload(dqo, read_off, (size_t)n_reads * 8, st)) ||
        (rc = upload(dql, read_len, (size_t)n_reads * 4, st)) || (rc = upload(dqu, qual, qual ? (size_t)qer_bytes : 0, st)) ||
        (rc = upload(dnm, names, (size_t)name_bytes, st)) || (rc = upload(dno, name_off, (size_t)(n_reads + 1) * 8, st)) ||
        (rc = upload(dcn, cnames, (size_t)cname_bytes, st)) || (rc = upload(dcno, cname_off, (size_t)(n_contigs + 1) * 8, st)) ||
        (rc = upload(dtx, text, (size_t)l_pac, st)) || (rc = upload(dco, contig_off, (size_t)(n_contigs + 1) * 8, st)) ||
        (rc = upload(dn, counts, sizeof(counts), st)) || (rc = drec.alloc((size_t)rcap * sizeof(gbx_mem_sam_rec))) ||
        (rc = drof.alloc((size_t)(n_reads + 1) * 8)) || (rc = dmd.alloc((size_t)md_cap)) || (rc = dli.alloc((size_t)text_cap)) || (rc = dw.alloc(wb)))
        return rc;
    int64_t *const d_n = dn.as<int64_t>();
    const MemSamIo io{drg.as<gbx_mem_reg>(), dro.as<int64_t>(), d_n, n_regs, dpa.as<gbx_mem_pair>(), dal.as<gbx_mem_aln>(), n_alns,
                      dcg.as<uint32_t>(), d_n + 1, n_cigar, dq.as<uint8_t>(), qer_bytes, dqo.as<int64_t>(), dql.as<int32_t>(),
                      qual ? dqu.as<uint8_t>() : nullptr, dnm.as<uint8_t>(), dno.as<int64_t>(), name_bytes, dcn.as<uint8_t>(), dcno.as<int64_t>(),
                      cname_bytes, dtx.as<uint8_t>(), l_pac, l_pac, n_contigs, dco.as<int64_t>(), drec.as<gbx_mem_sam_rec>(), rcap,
                      drof.as<int64_t>(), d_n + 2, dmd.as<uint8_t>(), md_cap, d_n + 3, dli.as<uint8_t>(), text_cap, d_n + 4};
    if ((rc = mem_sam_launch(p, n_reads, mode, io, dw.p, wb, st))) return rc;
    int64_t got[3] = {-1, -1, -1};
    GBX_HIP(hipMemcpyAsync(got, d_n + 2, 24, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipMemcpyAsync(rec_off, drof.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    *n_recs = got[0]; *n_md = got[1]; *n_text = got[2];
    if (got[0] < 0 || got[0] > rmax || got[1] < 0 || got[2] < 0) {
        set_error("%s: the device counted %lld records, %lld md bytes and %lld text bytes from %lld regions", who, (long long)got[0],
                  (long long)got[1], (long long)got[2], (long long)n_regs);
        return GBX_ERR_HIP;
    }
    if (got[0] > rec_cap || got[1] > md_cap || got[2] > text_cap) {
        set_error("%s: %lld records, %lld md bytes and %lld text bytes do not fit rec_cap = %lld, md_cap = %lld and text_cap = %lld", who,
                  (long long)got[0], (long long)got[1], (long long)got[2], (long long)rec_cap, (long long)md_cap, (long long)text_cap);
        return GBX_ERR_ARG;
    }
    if (got[0]) GBX_HIP(hipMemcpyAsync(recs, drec.p, (size_t)got[0] * sizeof(gbx_mem_sam_rec), hipMemcpyDeviceToHost, st));
    if (got[1]) GBX_HIP(hipMemcpyAsync(md, dmd.p, (size_t)got[1], hipMemcpyDeviceToHost, st));
    if (got[2]) GBX_HIP(hipMemcpyAsync(lines, dli.p, (size_t)got[2], hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    return GBX_OK;
}

}  // extern "C"
