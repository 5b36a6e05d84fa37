// capi_mem_pair.hip — paired-end entries of the C-ABI (include/gbx.h): the regs stage's regions of interleaved reads -> the
// insert-size estimate, a gbx_mem_pair per pair, the changed regions and the new CIGAR list.
#include <cmath>
#include "capi_common.h"

using namespace gbx;

namespace {
int params_check(const gbx_mem_pair_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc;
    if ((rc = gap_extend_check(p->e_del, p->e_ins, who)) || (rc = match_check(p->a, p->b, who))) return rc;
    if (p->max_ins < 1 || p->max_ins > (1 << 20)) { set_error("%s: max_ins = %d (1 .. 2^20)", who, p->max_ins); return GBX_ERR_ARG; }
    if ((rc = mapq_coef_len_check(p->mapq_coef_len, who))) return rc;
    return number_check("mask_level / mapq_coef_fac", {p->mask_level, p->mapq_coef_fac}, who);
}

int ids_check(int64_t n_pairs, int64_t pair_id0, const char *who)
{
    if (n_pairs < 0 || pair_id0 < 0 || pair_id0 > (1ll << 23) || n_pairs > (1ll << 23) - pair_id0) {
        set_error("%s: pair_id0 = %lld, n_pairs = %lld (pair ids lie in [0, 2^23])", who, (long long)pair_id0, (long long)n_pairs);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int pes_check(const gbx_mem_pestat *pes_in, const char *who)
{
    if (pes_in)
        for (int d = 0; d < 4; ++d)
            if (pes_in[d].failed == 0 && !(pes_in[d].std > 0.)) {
                set_error("%s: pes_in: direction %d has not failed and its std is not above 0", who, d);
                return GBX_ERR_ARG;
            }
    return GBX_OK;
}
}  // namespace

extern "C" {

void gbx_mem_pair_default_params(gbx_mem_pair_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->a = 1; p->b = 4; p->o_del = 6; p->e_del = 1; p->o_ins = 6; p->e_ins = 1; p->min_seed_len = 19; p->T = 30; p->pen_unpaired = 17;
    p->max_ins = 10000; p->mapq_coef_len = 50; p->mapq_coef_fac = (float)log((double)p->mapq_coef_len); p->mask_level = 0.5f;
    p->no_pairing = 0;
}

size_t gbx_mem_pair_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_ins)
{
    return mem_pair_workspace_bytes(n_pairs, reg_cap, max_ins);
}

// gbx_mem_pair_device (the estimate: pes_in, a host pointer) and gbx_mem_pair_device_pes (d_pes_in, a device pointer)
static int pair_device(const char *who, const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0,
                       const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                       const gbx_bsw_seed *d_sel_seeds, const gbx_bsw_seed_result *d_sel_res, int64_t sel_cap,
                       const gbx_bsw_seed *d_seeds, int64_t seed_cap, const int32_t *d_l_rep,
                       int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                       const gbx_mem_pestat *pes_in, const gbx_mem_pestat *d_pes_in, gbx_mem_pestat *d_pes, gbx_mem_pair *d_pairs,
                       gbx_mem_reg *d_pregs, gbx_bsw_seed *d_psel_seeds, gbx_bsw_seed_result *d_psel_res, int64_t psel_cap,
                       int64_t *d_n_psel, void *d_work, size_t work_bytes, void *stream)
{
    int rc = params_check(p, who);
    if (rc || (rc = ids_check(n_pairs, pair_id0, who)) || (rc = pes_check(pes_in, who))) return rc;
    if (reg_cap < 0 || sel_cap < 0 || seed_cap < 0 || psel_cap < 0 || l_pac < 1 || n_contigs < 1) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!d_reg_off || !d_n_regs || !d_contig_off || !d_pes || !d_n_psel || !d_work || (reg_cap > 0 && (!d_regs || !d_pregs)) ||
        (sel_cap > 0 && (!d_sel_seeds || !d_sel_res)) || (seed_cap > 0 && !d_seeds) || (n_pairs > 0 && (!d_l_rep || !d_pairs)) ||
        (psel_cap > 0 && (!d_psel_seeds || !d_psel_res))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MemPairIo io{d_regs, d_reg_off, d_n_regs, reg_cap, d_sel_seeds, d_sel_res, sel_cap, d_seeds, seed_cap, d_l_rep, l_pac, n_contigs,
                       d_contig_off, d_pes, d_pairs, d_pregs, d_psel_seeds, d_psel_res, psel_cap, d_n_psel};
    return mem_pair_launch(p, n_pairs, pair_id0, io, pes_in, d_work, work_bytes, (hipStream_t)stream, d_pes_in);
}

int gbx_mem_pair_device(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0,
                        const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                        const gbx_bsw_seed *d_sel_seeds, const gbx_bsw_seed_result *d_sel_res, int64_t sel_cap,
                        const gbx_bsw_seed *d_seeds, int64_t seed_cap, const int32_t *d_l_rep,
                        int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                        const gbx_mem_pestat *pes_in, gbx_mem_pestat *d_pes, gbx_mem_pair *d_pairs, gbx_mem_reg *d_pregs,
                        gbx_bsw_seed *d_psel_seeds, gbx_bsw_seed_result *d_psel_res, int64_t psel_cap, int64_t *d_n_psel,
                        void *d_work, size_t work_bytes, void *stream)
{
    return pair_device("gbx_mem_pair_device", p, n_pairs, pair_id0, d_regs, d_reg_off, d_n_regs, reg_cap, d_sel_seeds, d_sel_res, sel_cap,
                       d_seeds, seed_cap, d_l_rep, l_pac, n_contigs, d_contig_off, pes_in, nullptr, d_pes, d_pairs, d_pregs, d_psel_seeds,
                       d_psel_res, psel_cap, d_n_psel, d_work, work_bytes, stream);
}

int gbx_mem_pair_device_pes(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0,
                            const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                            const gbx_bsw_seed *d_sel_seeds, const gbx_bsw_seed_result *d_sel_res, int64_t sel_cap,
                            const gbx_bsw_seed *d_seeds, int64_t seed_cap, const int32_t *d_l_rep,
                            int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                            const gbx_mem_pestat *d_pes_in, gbx_mem_pestat *d_pes, gbx_mem_pair *d_pairs, gbx_mem_reg *d_pregs,
                            gbx_bsw_seed *d_psel_seeds, gbx_bsw_seed_result *d_psel_res, int64_t psel_cap, int64_t *d_n_psel,
                            void *d_work, size_t work_bytes, void *stream)
{
    return pair_device("gbx_mem_pair_device_pes", p, n_pairs, pair_id0, d_regs, d_reg_off, d_n_regs, reg_cap, d_sel_seeds, d_sel_res,
                       sel_cap, d_seeds, seed_cap, d_l_rep, l_pac, n_contigs, d_contig_off, nullptr, d_pes_in, d_pes, d_pairs, d_pregs,
                       d_psel_seeds, d_psel_res, psel_cap, d_n_psel, d_work, work_bytes, stream);
}

int gbx_mem_pair_host(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0,
                      const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs,
                      const gbx_bsw_seed *sel_seeds, const gbx_bsw_seed_result *sel_res, int64_t n_sel,
                      const gbx_bsw_seed *seeds, int64_t n_seeds, const int32_t *l_rep,
                      int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                      const gbx_mem_pestat *pes_in, gbx_mem_pestat *pes, gbx_mem_pair *pairs, gbx_mem_reg *pregs,
                      gbx_bsw_seed *psel_seeds, gbx_bsw_seed_result *psel_res, int64_t psel_cap, int64_t *n_psel)
{
    RoctxRange range_("gbx_mem_pair_host");
    const char *who = "gbx_mem_pair_host";
    int rc = params_check(p, who);
    if (rc || (rc = ids_check(n_pairs, pair_id0, who)) || (rc = pes_check(pes_in, who))) return rc;
    if (n_regs < 0 || n_sel < 0 || n_seeds < 0 || psel_cap < 0 || l_pac < 1 || n_contigs < 1) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!reg_off || !contig_off || !pes || !n_psel || (n_regs > 0 && (!regs || !pregs)) || (n_sel > 0 && (!sel_seeds || !sel_res)) ||
        (n_seeds > 0 && !seeds) || (n_pairs > 0 && (!l_rep || !pairs)) || (psel_cap > 0 && (!psel_seeds || !psel_res))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    // everything is checked before the device is touched
    if ((rc = contig_off_check(contig_off, n_contigs, l_pac, who))) return rc;
    const int64_t n_reads = 2 * n_pairs;
    if ((rc = offsets_check(reg_off, n_reads, n_regs, "reg_off", "regions", "read", who))) return rc;
    for (int64_t g = 0; g < n_regs; ++g) {
        if (regs[g].rid < 0 || regs[g].rid >= n_contigs) {
            set_error("%s: region %lld: rid = %d lies outside the %d contigs", who, (long long)g, regs[g].rid, n_contigs);
            return GBX_ERR_ARG;
        }
        if (regs[g].seed < 0 || regs[g].seed >= n_seeds) {
            set_error("%s: region %lld: seed = %lld lies outside the %lld seeds", who, (long long)g, (long long)regs[g].seed, (long long)n_seeds);
            return GBX_ERR_ARG;
        }
    }
    *n_psel = 0;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    // capacities on the device: the list never holds more records than there are regions
    const int64_t pcap = std::min(psel_cap, n_regs);
    DevBuf drg(L), dro(L), dss(L), dsr(L), dsd(L), dlr(L), dco(L), dn(L), dpe(L), dpa(L), dpr(L), dps(L), dpq(L), dw(L);
    const size_t wb = mem_pair_workspace_bytes(n_pairs, n_regs, p->max_ins);
    const int64_t counts[2] = {n_regs, 0};
    if ((rc = upload(drg, regs, (size_t)n_regs * sizeof(gbx_mem_reg), st)) || (rc = upload(dro, reg_off, (size_t)(n_reads + 1) * 8, st)) ||
        (rc = upload(dss, sel_seeds, (size_t)n_sel * sizeof(gbx_bsw_seed), st)) ||
        (rc = upload(dsr, sel_res, (size_t)n_sel * sizeof(gbx_bsw_seed_result), st)) ||
        (rc = upload(dsd, seeds, (size_t)n_seeds * sizeof(gbx_bsw_seed), st)) || (rc = upload(dlr, l_rep, (size_t)n_reads * 4, st)) ||
        (rc = upload(dco, contig_off, (size_t)(n_contigs + 1) * 8, st)) || (rc = upload(dn, counts, 16, st)) ||
        (rc = dpe.alloc(4 * sizeof(gbx_mem_pestat))) || (rc = dpa.alloc((size_t)n_pairs * sizeof(gbx_mem_pair))) ||
        (rc = dpr.alloc((size_t)n_regs * sizeof(gbx_mem_reg))) || (rc = dps.alloc((size_t)pcap * sizeof(gbx_bsw_seed))) ||
        (rc = dpq.alloc((size_t)pcap * sizeof(gbx_bsw_seed_result))) || (rc = dw.alloc(wb)))
        return rc;
    int64_t *const d_n = dn.as<int64_t>();
    const MemPairIo io{drg.as<gbx_mem_reg>(), dro.as<int64_t>(), d_n, n_regs, dss.as<gbx_bsw_seed>(), dsr.as<gbx_bsw_seed_result>(), n_sel,
                       dsd.as<gbx_bsw_seed>(), n_seeds, dlr.as<int32_t>(), l_pac, n_contigs, dco.as<int64_t>(), dpe.as<gbx_mem_pestat>(),
                       dpa.as<gbx_mem_pair>(), dpr.as<gbx_mem_reg>(), dps.as<gbx_bsw_seed>(), dpq.as<gbx_bsw_seed_result>(), pcap, d_n + 1};
    if ((rc = mem_pair_launch(p, n_pairs, pair_id0, io, pes_in, dw.p, wb, st))) return rc;
    int64_t got = -1;
    GBX_HIP(hipMemcpyAsync(&got, d_n + 1, 8, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipMemcpyAsync(pes, dpe.p, 4 * sizeof(gbx_mem_pestat), hipMemcpyDeviceToHost, st));
    if (n_pairs) GBX_HIP(hipMemcpyAsync(pairs, dpa.p, (size_t)n_pairs * sizeof(gbx_mem_pair), hipMemcpyDeviceToHost, st));
    if (n_regs) GBX_HIP(hipMemcpyAsync(pregs, dpr.p, (size_t)n_regs * sizeof(gbx_mem_reg), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    *n_psel = got;
    if (got < 0 || got > n_regs) {
        set_error("%s: the device counted %lld reported regions from %lld regions", who, (long long)got, (long long)n_regs);
        return GBX_ERR_HIP;
    }
    if (got > psel_cap) {
        set_error("%s: %lld reported regions do not fit psel_cap = %lld", who, (long long)got, (long long)psel_cap);
        return GBX_ERR_ARG;
    }
    if (pcap) GBX_HIP(hipMemcpyAsync(psel_seeds, dps.p, (size_t)pcap * sizeof(gbx_bsw_seed), hipMemcpyDeviceToHost, st));
    if (pcap) GBX_HIP(hipMemcpyAsync(psel_res, dpq.p, (size_t)pcap * sizeof(gbx_bsw_seed_result), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    sel_tail_fill(psel_seeds, psel_res, pcap, psel_cap);
    return GBX_OK;
}

}  // extern "C"
