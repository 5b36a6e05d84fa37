// capi_mm_sam.hip — the entries of the C-ABI (include/gbx.h) behind the alignments: SAM records and the PAF line with cs:Z: / MD:Z:
// and = / X operations (gbx_mm_sam_*).
#include "host_mm.h"

using namespace gbx;

namespace {

int params_check(const gbx_mm_sam_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (p->format < 0 || p->format > 1) { set_error("%s: format = %d (0 PAF, 1 SAM)", who, p->format); return GBX_ERR_ARG; }
    if (p->cs < 0 || p->cs > 2) { set_error("%s: cs = %d (0 none, 1 short, 2 long)", who, p->cs); return GBX_ERR_ARG; }
    if (p->md < 0 || p->md > 1) { set_error("%s: md = %d (0 or 1)", who, p->md); return GBX_ERR_ARG; }
    if (p->eqx < 0 || p->eqx > 1) { set_error("%s: eqx = %d (0 or 1)", who, p->eqx); return GBX_ERR_ARG; }
    if (p->softclip < 0 || p->softclip > 1) { set_error("%s: softclip = %d (0 or 1)", who, p->softclip); return GBX_ERR_ARG; }
    return GBX_OK;
}

}  // namespace

extern "C" {

void gbx_mm_sam_default_params(gbx_mm_sam_params *p)
{
    if (p) memset(p, 0, sizeof(*p));
}

int gbx_mm_sam_check_params(const gbx_mm_sam_params *p) { return params_check(p, "gbx_mm_sam_check_params"); }

size_t gbx_mm_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap)
{
    if (n_reads < 0 || reg_cap < 0) return 0;
    return mm_sam_workspace_bytes(n_reads, reg_cap);
}

int gbx_mm_sam_device(const gbx_mm_sam_params *p, int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs,
                      int64_t reg_cap, const gbx_mm_aln *d_alns, const uint32_t *d_cigar, int64_t cigar_cap,
                      const uint8_t *d_qnames, const int64_t *d_qname_off, const uint8_t *d_seq, const uint8_t *d_qual, const int64_t *d_seq_off,
                      const int32_t *d_rep_len, int64_t n_targets, const uint8_t *d_tnames, const int64_t *d_tname_off, const uint8_t *d_tseq,
                      const int64_t *d_tseq_off, uint8_t *d_lines, int64_t text_cap, int64_t *d_line_off, int64_t *d_n_text, int64_t *d_counts,
                      void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mm_sam_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if ((rc = mm_reads_check(n_reads, who))) return rc;
    if (reg_cap < 0 || n_targets < 0 || text_cap < 0 || cigar_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!d_reg_off || !d_n_regs || !d_qname_off || !d_seq_off || !d_line_off || !d_n_text || !d_counts || !d_work ||
        (reg_cap > 0 && (!d_regs || !d_alns)) || (cigar_cap > 0 && !d_cigar) || (n_reads > 0 && (!d_rep_len || !d_seq)) ||
        (n_targets > 0 && (!d_tname_off || !d_tseq_off || !d_tseq)) || (text_cap > 0 && !d_lines)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MmSamIo io{MmPafIo{n_reads, d_regs, d_reg_off, d_n_regs, reg_cap, d_alns, d_cigar, cigar_cap, d_qnames, d_qname_off, d_seq_off, d_rep_len, n_targets,
                             d_tnames, d_tname_off, d_tseq_off, d_lines, text_cap, d_line_off, d_n_text},
                     d_seq, d_qual, d_tseq, d_counts};
    return mm_sam_launch(p, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mm_sam_host(const gbx_mm_sam_params *p, int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns,
                    const uint32_t *cigar, int64_t n_cigar, const uint8_t *qnames, const int64_t *qname_off, const uint8_t *seq, const uint8_t *qual,
                    const int64_t *seq_off, const int32_t *rep_len, int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off,
                    const uint8_t *tseq, const int64_t *tseq_off, uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *n_text,
                    int64_t *counts)
{
    const char *who = "gbx_mm_sam_host";
    RoctxRange range_(who);
    int rc = params_check(p, who);
    if (rc) return rc;
    if ((rc = mm_reads_check(n_reads, who))) return rc;
    if (n_targets < 0 || n_targets >= (1ll << 31) || text_cap < 0 || n_cigar < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!line_off || !n_text || !counts || (n_reads > 0 && !rep_len) || (text_cap > 0 && !lines) || (n_cigar > 0 && !cigar)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = mm_offsets_check(reg_off, n_reads, "reg_off", "read", who)) || (rc = mm_offsets_check(qname_off, n_reads, "qname_off", "read", who)) ||
        (rc = mm_offsets_check(seq_off, n_reads, "seq_off", "read", who, 28)))
        return rc;
    if (n_targets > 0 && ((rc = mm_offsets_check(tname_off, n_targets, "tname_off", "target", who)) ||
                          (rc = mm_offsets_check(tseq_off, n_targets, "tseq_off", "target", who, 28))))
        return rc;
    const int64_t nr = reg_off[n_reads], qb = qname_off[n_reads], tb = n_targets > 0 ? tname_off[n_targets] : 0, sb = seq_off[n_reads],
                  cb = n_targets > 0 ? tseq_off[n_targets] : 0;
    if ((nr > 0 && (!regs || !alns)) || (qb > 0 && !qnames) || (tb > 0 && !tnames) || (sb > 0 && !seq) || (cb > 0 && !tseq)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = mm_regions_check(regs, reg_off, n_reads, who))) return rc;
    *n_text = 0;
    counts[0] = counts[1] = 0;
    line_off[0] = 0;
    if (n_reads == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    const size_t wb = mm_sam_workspace_bytes(n_reads, nr);
    const int64_t none[2] = {0, 0};
    DevBuf dr(L), dro(L), dn(L), da(L), dcg(L), dq(L), dqo(L), ds(L), dql(L), dso(L), drl(L), dt(L), dto(L), dtq(L), dts(L), dl(L), dlo(L), dnt(L), dc(L), dw(L);
    if ((rc = upload(dr, regs, (size_t)nr * sizeof(gbx_mm_reg), s)) || (rc = upload(dro, reg_off, (size_t)(n_reads + 1) * 8, s)) || (rc = upload(dn, &nr, 8, s)) ||
        (rc = upload(da, alns, (size_t)nr * sizeof(gbx_mm_aln), s)) || (rc = upload(dcg, cigar, (size_t)n_cigar * 4, s)) ||
        (rc = upload(dq, qnames, (size_t)qb, s)) || (rc = upload(dqo, qname_off, (size_t)(n_reads + 1) * 8, s)) || (rc = upload(ds, seq, (size_t)sb, s)) ||
        (qual && (rc = upload(dql, qual, (size_t)sb, s))) || (rc = upload(dso, seq_off, (size_t)(n_reads + 1) * 8, s)) ||
        (rc = upload(drl, rep_len, (size_t)n_reads * 4, s)) || (rc = upload(dt, tnames, (size_t)tb, s)) ||
        (rc = upload(dto, n_targets > 0 ? tname_off : none, (size_t)(n_targets + 1) * 8, s)) || (rc = upload(dtq, tseq, (size_t)cb, s)) ||
        (rc = upload(dts, n_targets > 0 ? tseq_off : none, (size_t)(n_targets + 1) * 8, s)) || (rc = dl.alloc((size_t)text_cap)) ||
        (rc = dlo.alloc((size_t)(n_reads + 1) * 8)) || (rc = dnt.alloc(8)) || (rc = dc.alloc(16)) || (rc = dw.alloc(wb)))
        return rc;
    const MmSamIo io{MmPafIo{n_reads, dr.as<gbx_mm_reg>(), dro.as<int64_t>(), dn.as<int64_t>(), nr, da.as<gbx_mm_aln>(), dcg.as<uint32_t>(), n_cigar,
                             dq.as<uint8_t>(), dqo.as<int64_t>(), dso.as<int64_t>(), drl.as<int32_t>(), n_targets, dt.as<uint8_t>(), dto.as<int64_t>(),
                             dts.as<int64_t>(), dl.as<uint8_t>(), text_cap, dlo.as<int64_t>(), dnt.as<int64_t>()},
                     ds.as<uint8_t>(), qual ? dql.as<uint8_t>() : nullptr, dtq.as<uint8_t>(), dc.as<int64_t>()};
    if ((rc = mm_sam_launch(p, io, dw.p, wb, s))) return rc;
    GBX_HIP(hipMemcpyAsync(n_text, dnt.p, 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(counts, dc.p, 16, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(line_off, dlo.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (*n_text < 0) { set_error("%s: the device counted %lld bytes of text", who, (long long)*n_text); return GBX_ERR_HIP; }
    if (*n_text > text_cap) { set_error("%s: %lld bytes of text do not fit text_cap = %lld", who, (long long)*n_text, (long long)text_cap); return GBX_ERR_ARG; }
    if (*n_text) GBX_HIP(hipMemcpyAsync(lines, dl.p, (size_t)*n_text, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

}  // extern "C"
