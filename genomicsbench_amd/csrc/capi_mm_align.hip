// capi_mm_align.hip — the entries of the C-ABI (include/gbx.h) for the base-level alignment of the regions.  The PAF text with
// CIGAR is written by the PAF entries of capi_mm_map.hip.
#include "host_mm.h"

using namespace gbx;

namespace {

int params_check(const gbx_mm_align_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (p->a < 1) { set_error("%s: a = %d (at least 1)", who, p->a); return GBX_ERR_ARG; }
    const struct { const char *name; int32_t v; } neg[] = {{"b", p->b}, {"sc_ambi", p->sc_ambi}, {"q", p->q}, {"q2", p->q2}, {"end_bonus", p->end_bonus}};
    for (const auto &f : neg)
        if (f.v < 0) { set_error("%s: %s = %d is negative", who, f.name, f.v); return GBX_ERR_ARG; }
    if (p->e < 1) { set_error("%s: e = %d (at least 1)", who, p->e); return GBX_ERR_ARG; }
    if (p->e2 < 1) { set_error("%s: e2 = %d (at least 1)", who, p->e2); return GBX_ERR_ARG; }
    if (p->bw < 1) { set_error("%s: bw = %d (at least 1)", who, p->bw); return GBX_ERR_ARG; }
    if (p->min_ksw_len < 1) { set_error("%s: min_ksw_len = %d (at least 1)", who, p->min_ksw_len); return GBX_ERR_ARG; }
    if (p->max_ext < 0) { set_error("%s: max_ext = %d is negative", who, p->max_ext); return GBX_ERR_ARG; }
    const struct { const char *name; int32_t v; } big[] = {{"a", p->a}, {"b", p->b}, {"sc_ambi", p->sc_ambi}, {"q", p->q}, {"e", p->e}, {"q2", p->q2},
                                                            {"e2", p->e2}, {"end_bonus", p->end_bonus}};
    for (const auto &f : big)
        if (f.v > 255) { set_error("%s: %s = %d (at most 255)", who, f.name, f.v); return GBX_ERR_ARG; }
    return GBX_OK;
}

}  // namespace

extern "C" {

void gbx_mm_align_default_params(gbx_mm_align_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->a = 2; p->b = 4; p->sc_ambi = 1; p->q = 4; p->e = 2; p->q2 = 24; p->e2 = 1; p->bw = 500; p->zdrop = 400; p->end_bonus = 0;
    p->min_ksw_len = 200; p->max_ext = 5000;
}

int gbx_mm_align_check_params(const gbx_mm_align_params *p) { return params_check(p, "gbx_mm_align_check_params"); }

size_t gbx_mm_align_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t anchor_cap)
{
    if (n_reads < 0 || reg_cap < 0 || anchor_cap < 0) return 0;
    return mm_align_workspace_bytes(n_reads, reg_cap, anchor_cap);
}

int gbx_mm_align_device(const gbx_mm_align_params *p, int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs,
                        int64_t reg_cap, const int64_t *d_off, const uint64_t *d_cax, const uint64_t *d_cay, const int32_t *d_n_chained,
                        int64_t anchor_cap, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t n_targets, const uint8_t *d_tseq,
                        const int64_t *d_tseq_off, gbx_mm_aln *d_alns, uint32_t *d_cigar, int64_t cigar_cap, int64_t *d_counts,
                        void *d_z, int64_t z_bytes, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mm_align_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if ((rc = mm_reads_check(n_reads, who))) return rc;
    if (reg_cap < 0 || anchor_cap < 0 || n_targets < 0 || n_targets >= (1ll << 31) || cigar_cap < 0 || z_bytes < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!d_reg_off || !d_n_regs || !d_off || !d_seq_off || !d_counts || !d_work || (reg_cap > 0 && (!d_regs || !d_alns)) || (n_reads > 0 && !d_n_chained) ||
        (anchor_cap > 0 && (!d_cax || !d_cay)) || (n_targets > 0 && !d_tseq_off) || (cigar_cap > 0 && !d_cigar) || (z_bytes > 0 && !d_z)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((uintptr_t)d_z & 15) { set_error("%s: d_z is not 16-aligned", who); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    const MmAlignIo io{n_reads, d_regs, d_n_regs, reg_cap, d_off, d_cax, d_cay, d_n_chained, anchor_cap, d_seq, d_seq_off, n_targets, d_tseq, d_tseq_off,
                       d_alns, d_cigar, cigar_cap, d_counts, (uint8_t *)d_z, z_bytes};
    return mm_align_launch(p, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mm_align_host(const gbx_mm_align_params *p, int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off,
                      const int64_t *off, const uint64_t *cax, const uint64_t *cay, const int32_t *n_chained,
                      const uint8_t *seq, const int64_t *seq_off, int64_t n_targets, const uint8_t *tseq, const int64_t *tseq_off,
                      gbx_mm_aln *alns, uint32_t *cigar, int64_t cigar_cap, int64_t z_bytes, int64_t *counts)
{
    RoctxRange range_("gbx_mm_align_host");
    const char *who = "gbx_mm_align_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    if ((rc = mm_reads_check(n_reads, who))) return rc;
    if (n_targets < 0 || n_targets >= (1ll << 31) || cigar_cap < 0 || z_bytes < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!counts || (cigar_cap > 0 && !cigar) || (n_reads > 0 && !n_chained)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = mm_offsets_check(reg_off, n_reads, "reg_off", "read", who)) || (rc = mm_offsets_check(off, n_reads, "off", "read", who)) ||
        (rc = mm_offsets_check(seq_off, n_reads, "seq_off", "read", who, 28)))
        return rc;
    if (n_targets > 0 && (rc = mm_offsets_check(tseq_off, n_targets, "tseq_off", "target", who, 28))) return rc;
    const int64_t nr = reg_off[n_reads], na = off[n_reads], nb = seq_off[n_reads], tb = n_targets > 0 ? tseq_off[n_targets] : 0;
    if ((nr > 0 && (!regs || !alns)) || (na > 0 && (!cax || !cay)) || (nb > 0 && !seq) || (tb > 0 && !tseq)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = mm_regions_check(regs, reg_off, n_reads, who))) return rc;
    for (int64_t r = 0; r < n_reads; ++r)
        if (n_chained[r] < 0 || n_chained[r] > off[r + 1] - off[r]) {
            set_error("%s: n_chained = %d at read %lld (0 .. %lld)", who, n_chained[r], (long long)r, (long long)(off[r + 1] - off[r]));
            return GBX_ERR_ARG;
        }
    counts[0] = counts[1] = counts[2] = 0;
    if (nr == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    const size_t wb = mm_align_workspace_bytes(n_reads, nr, na);
    const int64_t none[2] = {0, 0};
    DevBuf dr(L), dn(L), doff(L), dcx(L), dcy(L), dnc(L), dq(L), dso(L), dt(L), dto(L), da(L), dc(L), dcnt(L), dz(L), dw(L);
    if ((rc = upload(dr, regs, (size_t)nr * sizeof(gbx_mm_reg), s)) || (rc = upload(dn, &nr, 8, s)) || (rc = upload(doff, off, (size_t)(n_reads + 1) * 8, s)) ||
        (rc = upload(dcx, cax, (size_t)na * 8, s)) || (rc = upload(dcy, cay, (size_t)na * 8, s)) || (rc = upload(dnc, n_chained, (size_t)n_reads * 4, s)) ||
        (rc = upload(dq, seq, (size_t)nb, s)) || (rc = upload(dso, seq_off, (size_t)(n_reads + 1) * 8, s)) || (rc = upload(dt, tseq, (size_t)tb, s)) ||
        (rc = upload(dto, n_targets > 0 ? tseq_off : none, (size_t)(n_targets + 1) * 8, s)) || (rc = da.alloc((size_t)nr * sizeof(gbx_mm_aln))) ||
        (rc = dc.alloc((size_t)cigar_cap * 4)) || (rc = dcnt.alloc(24)) || (rc = dz.alloc((size_t)z_bytes)) || (rc = dw.alloc(wb)))
        return rc;
    const MmAlignIo io{n_reads, dr.as<gbx_mm_reg>(), dn.as<int64_t>(), nr, doff.as<int64_t>(), dcx.as<uint64_t>(), dcy.as<uint64_t>(), dnc.as<int32_t>(), na,
                       dq.as<uint8_t>(), dso.as<int64_t>(), n_targets, dt.as<uint8_t>(), dto.as<int64_t>(), da.as<gbx_mm_aln>(), dc.as<uint32_t>(), cigar_cap,
                       dcnt.as<int64_t>(), dz.as<uint8_t>(), z_bytes};
    if ((rc = mm_align_launch(p, io, dw.p, wb, s))) return rc;
    GBX_HIP(hipMemcpyAsync(counts, dcnt.p, 24, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(alns, da.p, (size_t)nr * sizeof(gbx_mm_aln), hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (counts[0] < 0 || counts[1] < 0 || counts[2] < 0) {
        set_error("%s: the device counted %lld jobs, %lld words and %lld bytes", who, (long long)counts[0], (long long)counts[1], (long long)counts[2]);
        return GBX_ERR_HIP;
    }
    if (counts[1] > cigar_cap || counts[2] > z_bytes) {
        set_error("%s: %lld CIGAR words and %lld bytes of z do not fit cigar_cap = %lld, z_bytes = %lld", who, (long long)counts[1], (long long)counts[2],
                  (long long)cigar_cap, (long long)z_bytes);
        return GBX_ERR_ARG;
    }
    if (counts[1]) GBX_HIP(hipMemcpyAsync(cigar, dc.p, (size_t)counts[1] * 4, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

}  // extern "C"
