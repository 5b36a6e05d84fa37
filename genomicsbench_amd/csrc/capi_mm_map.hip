// capi_mm_map.hip — the entries of the C-ABI (include/gbx.h) behind the chain scores: chains and regions, and the PAF text without
// and with the alignments (gbx_mm_paf_*, gbx_mm_paf_cigar_*: one body a pair).
#include "host_mm.h"

using namespace gbx;

namespace {

int params_check(const gbx_mm_map_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (p->min_cnt < 1) { set_error("%s: min_cnt = %d (at least 1)", who, p->min_cnt); return GBX_ERR_ARG; }
    if (p->min_chain_score < 0) { set_error("%s: min_chain_score = %d is negative", who, p->min_chain_score); return GBX_ERR_ARG; }
    if (p->best_n < 0) { set_error("%s: best_n = %d is negative", who, p->best_n); return GBX_ERR_ARG; }
    if (!(p->mask_level == p->mask_level)) { set_error("%s: mask_level is not a number", who); return GBX_ERR_ARG; }
    if (!(p->pri_ratio == p->pri_ratio)) { set_error("%s: pri_ratio is not a number", who); return GBX_ERR_ARG; }
    return GBX_OK;
}

// The body of gbx_mm_paf_device and gbx_mm_paf_cigar_device.  with_alns: the entry takes alignments (io.alns, io.cigar, io.cigar_cap) and
// checks them; without, they are null and every region prints the plain line.
int paf_device(const char *who, bool with_alns, const MmPafIo &io, void *d_work, size_t work_bytes, void *stream)
{
    int rc = mm_reads_check(io.n_reads, who);
    if (rc) return rc;
    if (io.reg_cap < 0 || io.n_targets < 0 || io.text_cap < 0 || (with_alns && io.cigar_cap < 0)) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!io.reg_off || !io.n_regs || !io.qname_off || !io.seq_off || !io.line_off || !io.n_text || !d_work ||
        (io.reg_cap > 0 && (!io.regs || (with_alns && !io.alns))) || (with_alns && io.cigar_cap > 0 && !io.cigar) || (io.n_reads > 0 && !io.rep_len) ||
        (io.n_targets > 0 && (!io.tname_off || !io.tseq_off)) || (io.text_cap > 0 && !io.lines)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return mm_paf_launch(io, d_work, work_bytes, (hipStream_t)stream);
}

// The body of gbx_mm_paf_host and gbx_mm_paf_cigar_host, with_alns as above.  A text_cap too small is GBX_ERR_ARG with the need in *n_text.
int paf_host(const char *who, bool with_alns, int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns, const uint32_t *cigar,
             int64_t n_cigar, const uint8_t *qnames, const int64_t *qname_off, const int64_t *seq_off, const int32_t *rep_len, int64_t n_targets,
             const uint8_t *tnames, const int64_t *tname_off, const int64_t *tseq_off, uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *n_text)
{
    RoctxRange range_(who);
    int rc = mm_reads_check(n_reads, who);
    if (rc) return rc;
    if (n_targets < 0 || n_targets >= (1ll << 31) || text_cap < 0 || n_cigar < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!line_off || !n_text || (n_reads > 0 && !rep_len) || (text_cap > 0 && !lines) || (n_cigar > 0 && !cigar)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = mm_offsets_check(reg_off, n_reads, "reg_off", "read", who)) || (rc = mm_offsets_check(qname_off, n_reads, "qname_off", "read", who)) ||
        (rc = mm_offsets_check(seq_off, n_reads, "seq_off", "read", who)))
        return rc;
    if (n_targets > 0 && ((rc = mm_offsets_check(tname_off, n_targets, "tname_off", "target", who)) || (rc = mm_offsets_check(tseq_off, n_targets, "tseq_off", "target", who))))
        return rc;
    const int64_t nr = reg_off[n_reads], qb = qname_off[n_reads], tb = n_targets > 0 ? tname_off[n_targets] : 0;
    if ((nr > 0 && (!regs || (with_alns && !alns))) || (qb > 0 && !qnames) || (tb > 0 && !tnames)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = mm_regions_check(regs, reg_off, n_reads, who))) return rc;
    *n_text = 0;
    line_off[0] = 0;
    if (n_reads == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    const size_t wb = mm_paf_workspace_bytes(nr);
    const int64_t none[2] = {0, 0};
    DevBuf dr(L), dro(L), dn(L), da(L), dcg(L), dq(L), dqo(L), dso(L), drl(L), dt(L), dto(L), dts(L), dl(L), dlo(L), dnt(L), dw(L);
    if ((rc = upload(dr, regs, (size_t)nr * sizeof(gbx_mm_reg), s)) || (rc = upload(dro, reg_off, (size_t)(n_reads + 1) * 8, s)) || (rc = upload(dn, &nr, 8, s)) ||
        (with_alns && ((rc = upload(da, alns, (size_t)nr * sizeof(gbx_mm_aln), s)) || (rc = upload(dcg, cigar, (size_t)n_cigar * 4, s)))) ||
        (rc = upload(dq, qnames, (size_t)qb, s)) || (rc = upload(dqo, qname_off, (size_t)(n_reads + 1) * 8, s)) ||
        (rc = upload(dso, seq_off, (size_t)(n_reads + 1) * 8, s)) || (rc = upload(drl, rep_len, (size_t)n_reads * 4, s)) || (rc = upload(dt, tnames, (size_t)tb, s)) ||
        (rc = upload(dto, n_targets > 0 ? tname_off : none, (size_t)(n_targets + 1) * 8, s)) ||
        (rc = upload(dts, n_targets > 0 ? tseq_off : none, (size_t)(n_targets + 1) * 8, s)) || (rc = dl.alloc((size_t)text_cap)) ||
        (rc = dlo.alloc((size_t)(n_reads + 1) * 8)) || (rc = dnt.alloc(8)) || (rc = dw.alloc(wb)))
        return rc;
    const MmPafIo io{n_reads, dr.as<gbx_mm_reg>(), dro.as<int64_t>(), dn.as<int64_t>(), nr, with_alns ? da.as<gbx_mm_aln>() : nullptr, dcg.as<uint32_t>(), n_cigar,
                     dq.as<uint8_t>(), dqo.as<int64_t>(), dso.as<int64_t>(), drl.as<int32_t>(), n_targets, dt.as<uint8_t>(), dto.as<int64_t>(), dts.as<int64_t>(),
                     dl.as<uint8_t>(), text_cap, dlo.as<int64_t>(), dnt.as<int64_t>()};
    if ((rc = mm_paf_launch(io, dw.p, wb, s))) return rc;
    GBX_HIP(hipMemcpyAsync(n_text, dnt.p, 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(line_off, dlo.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (*n_text < 0) { set_error("%s: the device counted %lld bytes of text", who, (long long)*n_text); return GBX_ERR_HIP; }
    if (*n_text > text_cap) { set_error("%s: %lld bytes of text do not fit text_cap = %lld", who, (long long)*n_text, (long long)text_cap); return GBX_ERR_ARG; }
    if (*n_text) GBX_HIP(hipMemcpyAsync(lines, dl.p, (size_t)*n_text, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

}  // namespace

extern "C" {

void gbx_mm_map_default_params(gbx_mm_map_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->min_cnt = 3; p->min_chain_score = 40; p->mask_level = 0.5f; p->pri_ratio = 0.8f; p->best_n = 5; p->min_diff = 30;
}

int gbx_mm_map_check_params(const gbx_mm_map_params *p) { return params_check(p, "gbx_mm_map_check_params"); }

size_t gbx_mm_map_workspace_bytes(int64_t n_reads, int64_t anchor_cap, int64_t chain_cap)
{
    if (n_reads < 0 || anchor_cap < 0 || chain_cap < 0) return 0;
    return mm_map_workspace_bytes(n_reads, anchor_cap, chain_cap);
}

int gbx_mm_map_device(const gbx_mm_map_params *p, int64_t n_reads, const int64_t *d_off, const uint64_t *d_ax, const uint64_t *d_ay,
                      int64_t anchor_cap, const int32_t *d_score, const int32_t *d_parent, const int32_t *d_peak,
                      const int64_t *d_seq_off, const int32_t *d_rep_len, const uint32_t *d_hash,
                      int64_t *d_chain_off, uint64_t *d_u, int64_t chain_cap, uint64_t *d_cax, uint64_t *d_cay, int32_t *d_n_chained,
                      int64_t *d_reg_off, gbx_mm_reg *d_regs, int64_t reg_cap, int64_t *d_counts, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mm_map_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if ((rc = mm_reads_check(n_reads, who))) return rc;
    if (anchor_cap < 0 || chain_cap < 0 || reg_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!d_off || !d_seq_off || !d_chain_off || !d_reg_off || !d_counts || !d_work || (n_reads > 0 && (!d_rep_len || !d_hash || !d_n_chained)) ||
        (anchor_cap > 0 && (!d_ax || !d_ay || !d_score || !d_parent || !d_peak || !d_cax || !d_cay)) || (chain_cap > 0 && !d_u) || (reg_cap > 0 && !d_regs)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MmMapIo io{n_reads, d_off, d_ax, d_ay, anchor_cap, d_score, d_parent, d_peak, d_seq_off, d_rep_len, d_hash, d_chain_off, d_u, chain_cap,
                     d_cax, d_cay, d_n_chained, d_reg_off, d_regs, reg_cap, d_counts};
    return mm_map_launch(p, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mm_map_host(const gbx_mm_map_params *p, int64_t n_reads, const int64_t *off, const uint64_t *ax, const uint64_t *ay,
                    const int32_t *score, const int32_t *parent, const int32_t *peak,
                    const int64_t *seq_off, const int32_t *rep_len, const uint32_t *hash,
                    int64_t *chain_off, uint64_t *u, int64_t chain_cap, uint64_t *cax, uint64_t *cay, int32_t *n_chained,
                    int64_t *reg_off, gbx_mm_reg *regs, int64_t reg_cap, int64_t *counts)
{
    RoctxRange range_("gbx_mm_map_host");
    const char *who = "gbx_mm_map_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    if ((rc = mm_reads_check(n_reads, who))) return rc;
    if (chain_cap < 0 || reg_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!chain_off || !reg_off || !counts || (n_reads > 0 && (!rep_len || !hash || !n_chained)) || (chain_cap > 0 && !u) || (reg_cap > 0 && !regs)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = mm_offsets_check(off, n_reads, "off", "read", who)) || (rc = mm_offsets_check(seq_off, n_reads, "seq_off", "read", who))) return rc;
    const int64_t na = off[n_reads];
    if (na > 0 && (!ax || !ay || !score || !parent || !peak || !cax || !cay)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n_reads; ++r)
        for (int64_t i = off[r]; i < off[r + 1]; ++i)
            if (parent[i] < -1 || parent[i] >= i - off[r]) {
                set_error("%s: parent = %d at anchor %lld of read %lld (-1 .. %lld)", who, parent[i], (long long)(i - off[r]), (long long)r,
                          (long long)(i - off[r] - 1));
                return GBX_ERR_ARG;
            }
    counts[0] = counts[1] = 0;
    chain_off[0] = reg_off[0] = 0;
    if (n_reads == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    const int64_t acap = std::max<int64_t>(na, 1);
    const size_t wb = mm_map_workspace_bytes(n_reads, acap, chain_cap);
    DevBuf doff(L), dax(L), day(L), df(L), dp(L), dv(L), dso(L), drl(L), dh(L), dco(L), du(L), dcx(L), dcy(L), dnc(L), dro(L), dr(L), dc(L), dw(L);
    if ((rc = upload(doff, off, (size_t)(n_reads + 1) * 8, s)) || (rc = upload(dax, ax, (size_t)na * 8, s)) || (rc = upload(day, ay, (size_t)na * 8, s)) ||
        (rc = upload(df, score, (size_t)na * 4, s)) || (rc = upload(dp, parent, (size_t)na * 4, s)) || (rc = upload(dv, peak, (size_t)na * 4, s)) ||
        (rc = upload(dso, seq_off, (size_t)(n_reads + 1) * 8, s)) || (rc = upload(drl, rep_len, (size_t)n_reads * 4, s)) ||
        (rc = upload(dh, hash, (size_t)n_reads * 4, s)) || (rc = dco.alloc((size_t)(n_reads + 1) * 8)) || (rc = du.alloc((size_t)chain_cap * 8)) ||
        (rc = dcx.alloc((size_t)acap * 8)) || (rc = dcy.alloc((size_t)acap * 8)) || (rc = dnc.alloc((size_t)n_reads * 4)) ||
        (rc = dro.alloc((size_t)(n_reads + 1) * 8)) || (rc = dr.alloc((size_t)reg_cap * sizeof(gbx_mm_reg))) || (rc = dc.alloc(16)) || (rc = dw.alloc(wb)))
        return rc;
    const MmMapIo io{n_reads, doff.as<int64_t>(), dax.as<uint64_t>(), day.as<uint64_t>(), na, df.as<int32_t>(), dp.as<int32_t>(), dv.as<int32_t>(),
                     dso.as<int64_t>(), drl.as<int32_t>(), dh.as<uint32_t>(), dco.as<int64_t>(), du.as<uint64_t>(), chain_cap, dcx.as<uint64_t>(),
                     dcy.as<uint64_t>(), dnc.as<int32_t>(), dro.as<int64_t>(), dr.as<gbx_mm_reg>(), reg_cap, dc.as<int64_t>()};
    if ((rc = mm_map_launch(p, io, dw.p, wb, s))) return rc;
    GBX_HIP(hipMemcpyAsync(counts, dc.p, 16, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(chain_off, dco.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(reg_off, dro.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(n_chained, dnc.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (counts[0] < 0 || counts[0] > na || counts[1] > counts[0]) {
        set_error("%s: the device counted %lld chains and %lld regions of %lld anchors", who, (long long)counts[0], (long long)counts[1], (long long)na);
        return GBX_ERR_HIP;
    }
    if (counts[0] > chain_cap || counts[1] > reg_cap) {
        set_error("%s: %lld chains and %lld regions do not fit chain_cap = %lld, reg_cap = %lld", who, (long long)counts[0], (long long)counts[1],
                  (long long)chain_cap, (long long)reg_cap);
        return GBX_ERR_ARG;
    }
    if (counts[0]) GBX_HIP(hipMemcpyAsync(u, du.p, (size_t)counts[0] * 8, hipMemcpyDeviceToHost, s));
    if (counts[1]) GBX_HIP(hipMemcpyAsync(regs, dr.p, (size_t)counts[1] * sizeof(gbx_mm_reg), hipMemcpyDeviceToHost, s));
    if (na) {
        GBX_HIP(hipMemcpyAsync(cax, dcx.p, (size_t)na * 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(cay, dcy.p, (size_t)na * 8, hipMemcpyDeviceToHost, s));
    }
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

size_t gbx_mm_paf_workspace_bytes(int64_t n_reads, int64_t reg_cap)
{
    if (n_reads < 0 || reg_cap < 0) return 0;
    return mm_paf_workspace_bytes(reg_cap);
}

size_t gbx_mm_paf_cigar_workspace_bytes(int64_t n_reads, int64_t reg_cap) { return gbx_mm_paf_workspace_bytes(n_reads, reg_cap); }

int gbx_mm_paf_device(int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                      const uint8_t *d_qnames, const int64_t *d_qname_off, const int64_t *d_seq_off, const int32_t *d_rep_len,
                      int64_t n_targets, const uint8_t *d_tnames, const int64_t *d_tname_off, const int64_t *d_tseq_off,
                      uint8_t *d_lines, int64_t text_cap, int64_t *d_line_off, int64_t *d_n_text, void *d_work, size_t work_bytes, void *stream)
{
    return paf_device("gbx_mm_paf_device", false, MmPafIo{n_reads, d_regs, d_reg_off, d_n_regs, reg_cap, nullptr, nullptr, 0, d_qnames, d_qname_off, d_seq_off,
                                                          d_rep_len, n_targets, d_tnames, d_tname_off, d_tseq_off, d_lines, text_cap, d_line_off, d_n_text},
                      d_work, work_bytes, stream);
}

int gbx_mm_paf_cigar_device(int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                            const gbx_mm_aln *d_alns, const uint32_t *d_cigar, int64_t cigar_cap,
                            const uint8_t *d_qnames, const int64_t *d_qname_off, const int64_t *d_seq_off, const int32_t *d_rep_len,
                            int64_t n_targets, const uint8_t *d_tnames, const int64_t *d_tname_off, const int64_t *d_tseq_off,
                            uint8_t *d_lines, int64_t text_cap, int64_t *d_line_off, int64_t *d_n_text, void *d_work, size_t work_bytes, void *stream)
{
    return paf_device("gbx_mm_paf_cigar_device", true, MmPafIo{n_reads, d_regs, d_reg_off, d_n_regs, reg_cap, d_alns, d_cigar, cigar_cap, d_qnames, d_qname_off,
                                                               d_seq_off, d_rep_len, n_targets, d_tnames, d_tname_off, d_tseq_off, d_lines, text_cap, d_line_off,
                                                               d_n_text},
                      d_work, work_bytes, stream);
}

int gbx_mm_paf_host(int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off,
                    const uint8_t *qnames, const int64_t *qname_off, const int64_t *seq_off, const int32_t *rep_len,
                    int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off, const int64_t *tseq_off,
                    uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *n_text)
{
    return paf_host("gbx_mm_paf_host", false, n_reads, regs, reg_off, nullptr, nullptr, 0, qnames, qname_off, seq_off, rep_len, n_targets, tnames, tname_off,
                    tseq_off, lines, text_cap, line_off, n_text);
}

int gbx_mm_paf_cigar_host(int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns, const uint32_t *cigar,
                          int64_t n_cigar, const uint8_t *qnames, const int64_t *qname_off, const int64_t *seq_off, const int32_t *rep_len,
                          int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off, const int64_t *tseq_off,
                          uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *n_text)
{
    return paf_host("gbx_mm_paf_cigar_host", true, n_reads, regs, reg_off, alns, cigar, n_cigar, qnames, qname_off, seq_off, rep_len, n_targets, tnames,
                    tname_off, tseq_off, lines, text_cap, line_off, n_text);
}

}  // extern "C"
