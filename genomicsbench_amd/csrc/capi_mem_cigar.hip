// capi_mem_cigar.hip — CIGAR entries of the C-ABI (include/gbx.h): seeds and their extension results -> gbx_mem_aln records and
// CIGAR words.
#include "capi_common.h"

using namespace gbx;

namespace {
int params_check(const gbx_mem_cigar_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (p->w < 0 || p->w > (1 << 27)) { set_error("%s: w = %d (0 .. 2^27)", who, p->w); return GBX_ERR_ARG; }
    return gap_extend_check(p->e_del, p->e_ins, who);
}
}  // namespace

extern "C" {

void gbx_mem_cigar_default_params(gbx_mem_cigar_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    for (int t = 0; t < 5; ++t)
        for (int q = 0; q < 5; ++q) p->mat[t * 5 + q] = t == 4 || q == 4 ? -1 : t == q ? 1 : -4;
    p->o_del = 6; p->e_del = 1; p->o_ins = 6; p->e_ins = 1; p->w = 100;
}

size_t gbx_mem_cigar_record_z_bytes(const gbx_mem_cigar_params *p, int32_t lq, int32_t lt)
{
    return p ? mem_cigar_record_z_bytes(p, lq, lt) : 0;
}

size_t gbx_mem_cigar_workspace_bytes(int64_t n, int64_t z_bytes)
{
    return mem_cigar_fixed_bytes(n) + (size_t)(z_bytes < 0 ? 0 : z_bytes);
}

int gbx_mem_cigar_device(const gbx_mem_cigar_params *p, int64_t n,
                         const gbx_bsw_seed *d_seeds, const gbx_bsw_seed_result *d_res,
                         const uint8_t *d_text, int64_t text_bytes, const uint8_t *d_qer, int64_t qer_bytes,
                         int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                         gbx_mem_aln *d_alns, uint32_t *d_cigar, int64_t cigar_cap, int64_t *d_n_cigar,
                         void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mem_cigar_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n < 0 || text_bytes < 0 || qer_bytes < 0 || cigar_cap < 0 || l_pac < 1 || n_contigs < 1) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!d_contig_off || !d_n_cigar || !d_work || (n > 0 && (!d_seeds || !d_res || !d_alns)) || (text_bytes > 0 && !d_text) ||
        (qer_bytes > 0 && !d_qer) || (cigar_cap > 0 && !d_cigar)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    const size_t fixed = mem_cigar_fixed_bytes(n);
    if (work_bytes < fixed) { set_error("%s: workspace too small", who); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    const MemCigarIo io{d_seeds, d_res, d_text, text_bytes, d_qer, qer_bytes, l_pac, n_contigs, d_contig_off, d_alns, d_cigar, cigar_cap, d_n_cigar};
    return mem_cigar_launch(p, n, io, d_work, work_bytes, (int64_t)(work_bytes - fixed), (hipStream_t)stream);
}

int gbx_mem_cigar_host(const gbx_mem_cigar_params *p, int64_t n,
                       const gbx_bsw_seed *seeds, const gbx_bsw_seed_result *res,
                       const uint8_t *text, int64_t text_bytes, const uint8_t *qer, int64_t qer_bytes,
                       int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                       gbx_mem_aln *alns, uint32_t *cigar, int64_t cigar_cap, int64_t *n_cigar)
{
    RoctxRange range_("gbx_mem_cigar_host");
    const char *who = "gbx_mem_cigar_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n < 0 || text_bytes < 0 || qer_bytes < 0 || cigar_cap < 0 || l_pac < 1 || n_contigs < 1) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!contig_off || !n_cigar || (n > 0 && (!seeds || !res || !alns)) || (text_bytes > 0 && !text) || (qer_bytes > 0 && !qer) ||
        (cigar_cap > 0 && !cigar)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    // everything is checked before the device is touched
    if ((rc = contig_off_check(contig_off, n_contigs, l_pac, who))) return rc;
    size_t z_bytes = 0;
    for (int64_t k = 0; k < n; ++k) {
        size_t need = 0;
        if (mem_cigar_record_host(p, seeds[k], res[k], text_bytes, qer_bytes, l_pac, &need) < 0) {
            set_error("%s: record %lld: its read or its region lies outside the arenas", who, (long long)k);
            return GBX_ERR_ARG;
        }
        z_bytes += need;
    }
    *n_cigar = 0;
    if (n == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    DevBuf dsd(L), drs(L), dtx(L), dqr(L), dco(L), dal(L), dcg(L), dn(L), dw(L);
    const size_t wb = mem_cigar_fixed_bytes(n) + z_bytes;
    if ((rc = upload(dsd, seeds, (size_t)n * sizeof(gbx_bsw_seed), st)) || (rc = upload(drs, res, (size_t)n * sizeof(gbx_bsw_seed_result), st)) ||
        (rc = upload(dtx, text, (size_t)text_bytes, st)) || (rc = upload(dqr, qer, (size_t)qer_bytes, st)) ||
        (rc = upload(dco, contig_off, (size_t)(n_contigs + 1) * 8, st)) || (rc = dal.alloc((size_t)n * sizeof(gbx_mem_aln))) ||
        (rc = dcg.alloc((size_t)cigar_cap * 4)) || (rc = dn.alloc(8)) || (rc = dw.alloc(wb)))
        return rc;
    const MemCigarIo io{dsd.as<gbx_bsw_seed>(), drs.as<gbx_bsw_seed_result>(), dtx.as<uint8_t>(), text_bytes, dqr.as<uint8_t>(), qer_bytes,
                        l_pac, n_contigs, dco.as<int64_t>(), dal.as<gbx_mem_aln>(), dcg.as<uint32_t>(), cigar_cap, dn.as<int64_t>()};
    if ((rc = mem_cigar_launch(p, n, io, dw.p, wb, (int64_t)z_bytes, st))) return rc;
    int64_t got = -1;
    GBX_HIP(hipMemcpyAsync(&got, dn.p, 8, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipMemcpyAsync(alns, dal.p, (size_t)n * sizeof(gbx_mem_aln), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    *n_cigar = got;
    if (got < 0) { set_error("%s: the device counted %lld CIGAR words", who, (long long)got); return GBX_ERR_HIP; }
    if (got > cigar_cap) {
        set_error("%s: %lld CIGAR words do not fit cigar_cap = %lld", who, (long long)got, (long long)cigar_cap);
        return GBX_ERR_ARG;
    }
    if (got) GBX_HIP(hipMemcpyAsync(cigar, dcg.p, (size_t)got * 4, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    return GBX_OK;
}

}  // extern "C"
