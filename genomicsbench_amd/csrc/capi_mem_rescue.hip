// capi_mem_rescue.hip — mate-rescue entries of the C-ABI (include/gbx.h): the regs stage's regions of interleaved reads and the
// insert-size estimate -> the same lists with the rescued regions, their seed records and the new CIGAR list; and the estimate
// alone (gbx_mem_pestat_*).
#include <cmath>
#include "capi_common.h"

using namespace gbx;

namespace {
constexpr int MAX_READ = 1024, MAX_WIN = 1 << 20;

int params_check(const gbx_mem_rescue_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc;
    if ((rc = gap_extend_check(p->e_del, p->e_ins, who)) || (rc = match_check(p->a, p->b, who))) return rc;
    if (p->o_del < 0 || p->o_ins < 0) { set_error("%s: o_del = %d, o_ins = %d (both at least 0)", who, p->o_del, p->o_ins); return GBX_ERR_ARG; }
    if (p->max_matesw < 1) { set_error("%s: max_matesw = %d (at least 1)", who, p->max_matesw); return GBX_ERR_ARG; }
    if (p->a > 63 || p->b > 5) {
        set_error("%s: a = %d, b = %d: a > 63 (16-bit cells) and b > 5 (byte mode's early exit) are not modelled", who, p->a, p->b);
        return GBX_ERR_UNSUPPORTED;
    }
    if ((rc = mapq_coef_len_check(p->mapq_coef_len, who))) return rc;
    return number_check("mask_level / mask_level_redun / mapq_coef_fac", {p->mask_level, p->mask_level_redun, p->mapq_coef_fac}, who);
}

int pestat_params_check(const gbx_mem_pair_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (p->a < 1) { set_error("%s: a = %d (at least 1)", who, p->a); return GBX_ERR_ARG; }
    if (p->max_ins < 1 || p->max_ins > (1 << 20)) { set_error("%s: max_ins = %d (1 .. 2^20)", who, p->max_ins); return GBX_ERR_ARG; }
    return number_check("mask_level", {p->mask_level}, who);
}

int ids_check(int64_t n_pairs, int64_t pair_id0, const char *who)
{
    if (n_pairs < 0 || pair_id0 < 0 || pair_id0 > (1ll << 23) || n_pairs > (1ll << 23) - pair_id0) {
        set_error("%s: pair_id0 = %lld, n_pairs = %lld (pair ids lie in [0, 2^23])", who, (long long)pair_id0, (long long)n_pairs);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

// what a call can add at most: four regions per anchor
int64_t most_added(int64_t n_pairs, int64_t n_regs, int32_t max_matesw)
{
    return 4 * std::min(n_regs, 2 * n_pairs * (int64_t)max_matesw);
}
}  // namespace

extern "C" {

void gbx_mem_rescue_default_params(gbx_mem_rescue_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->a = 1; p->b = 4; p->o_del = 6; p->e_del = 1; p->o_ins = 6; p->e_ins = 1; p->min_seed_len = 19; p->T = 30; p->pen_unpaired = 17;
    p->max_matesw = 50; p->max_chain_gap = 10000; p->mapq_coef_len = 50; p->mapq_coef_fac = (float)log((double)p->mapq_coef_len);
    p->mask_level = 0.5f; p->mask_level_redun = 0.95f;
}

size_t gbx_mem_pestat_workspace_bytes(int32_t max_ins) { return mem_pestat_workspace_bytes(max_ins); }

int gbx_mem_pestat_device(const gbx_mem_pair_params *p, int64_t n_pairs,
                          const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap, int64_t l_pac,
                          gbx_mem_pestat *d_pes, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mem_pestat_device";
    int rc = pestat_params_check(p, who);
    if (rc) return rc;
    if (n_pairs < 0 || reg_cap < 0 || l_pac < 1) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!d_reg_off || !d_n_regs || !d_pes || !d_work || (reg_cap > 0 && !d_regs)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    MemPairIo io{};
    io.regs = d_regs; io.reg_off = d_reg_off; io.n_regs = d_n_regs; io.reg_cap = reg_cap; io.l_pac = l_pac; io.pes = d_pes;
    return mem_pestat_launch(p, n_pairs, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mem_pestat_host(const gbx_mem_pair_params *p, int64_t n_pairs, const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs,
                        int64_t l_pac, gbx_mem_pestat *pes)
{
    RoctxRange range_("gbx_mem_pestat_host");
    const char *who = "gbx_mem_pestat_host";
    int rc = pestat_params_check(p, who);
    if (rc) return rc;
    if (n_pairs < 0 || n_regs < 0 || l_pac < 1) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!reg_off || !pes || (n_regs > 0 && !regs)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = offsets_check(reg_off, 2 * n_pairs, n_regs, "reg_off", "regions", "read", who))) return rc;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    DevBuf drg(L), dro(L), dn(L), dpe(L), dw(L);
    const size_t wb = mem_pestat_workspace_bytes(p->max_ins);
    if ((rc = upload(drg, regs, (size_t)n_regs * sizeof(gbx_mem_reg), st)) || (rc = upload(dro, reg_off, (size_t)(2 * n_pairs + 1) * 8, st)) ||
        (rc = upload(dn, &n_regs, 8, st)) || (rc = dpe.alloc(4 * sizeof(gbx_mem_pestat))) || (rc = dw.alloc(wb)))
        return rc;
    MemPairIo io{};
    io.regs = drg.as<gbx_mem_reg>(); io.reg_off = dro.as<int64_t>(); io.n_regs = dn.as<int64_t>(); io.reg_cap = n_regs; io.l_pac = l_pac;
    io.pes = dpe.as<gbx_mem_pestat>();
    if ((rc = mem_pestat_launch(p, n_pairs, io, dw.p, wb, st))) return rc;
    GBX_HIP(hipMemcpyAsync(pes, dpe.p, 4 * sizeof(gbx_mem_pestat), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    return GBX_OK;
}

size_t gbx_mem_rescue_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_matesw)
{
    return mem_rescue_workspace_bytes(n_pairs, reg_cap, max_matesw);
}

int gbx_mem_rescue_device(const gbx_mem_rescue_params *p, int64_t n_pairs, int64_t pair_id0,
                          const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                          const gbx_bsw_seed *d_seeds, int64_t seed_cap, const int32_t *d_l_rep,
                          const int64_t *d_read_off, const int32_t *d_read_len,
                          const uint8_t *d_text, int64_t text_bytes, const uint8_t *d_qer, int64_t qer_bytes,
                          int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off, const gbx_mem_pestat *d_pes,
                          gbx_mem_reg *d_xregs, int64_t xreg_cap, int64_t *d_xreg_off, int64_t *d_n_xregs,
                          gbx_bsw_seed *d_xseeds, int64_t xseed_cap, int64_t *d_n_xseeds,
                          gbx_bsw_seed *d_xsel_seeds, gbx_bsw_seed_result *d_xsel_res, int64_t xsel_cap, int64_t *d_n_xsel,
                          gbx_mem_rescue_stat *d_stats, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mem_rescue_device";
    int rc = params_check(p, who);
    if (rc || (rc = ids_check(n_pairs, pair_id0, who))) return rc;
    if (reg_cap < 0 || seed_cap < 0 || xreg_cap < 0 || xseed_cap < 0 || xsel_cap < 0 || qer_bytes < 0 || l_pac < 1 || n_contigs < 1 ||
        text_bytes < 2 * l_pac) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!d_reg_off || !d_n_regs || !d_contig_off || !d_pes || !d_text || !d_xreg_off || !d_n_xregs || !d_n_xseeds || !d_n_xsel || !d_work ||
        (reg_cap > 0 && !d_regs) || (seed_cap > 0 && !d_seeds) || (n_pairs > 0 && (!d_l_rep || !d_read_off || !d_read_len || !d_qer || !d_stats)) ||
        (xreg_cap > 0 && !d_xregs) || (xseed_cap > 0 && !d_xseeds) || (xsel_cap > 0 && (!d_xsel_seeds || !d_xsel_res))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MemRescueIo io{d_regs, d_reg_off, d_n_regs, reg_cap, d_seeds, seed_cap, d_l_rep, d_read_off, d_read_len, d_text, text_bytes, d_qer,
                         qer_bytes, l_pac, n_contigs, d_contig_off, d_pes, d_xregs, xreg_cap, d_xreg_off, d_n_xregs, d_xseeds, xseed_cap,
                         d_n_xseeds, d_xsel_seeds, d_xsel_res, xsel_cap, d_n_xsel, d_stats};
    return mem_rescue_launch(p, n_pairs, pair_id0, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mem_rescue_host(const gbx_mem_rescue_params *p, int64_t n_pairs, int64_t pair_id0,
                        const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs,
                        const gbx_bsw_seed *seeds, int64_t n_seeds, const int32_t *l_rep,
                        const int64_t *read_off, const int32_t *read_len,
                        const uint8_t *text, int64_t text_bytes, const uint8_t *qer, int64_t qer_bytes,
                        int64_t l_pac, int32_t n_contigs, const int64_t *contig_off, const gbx_mem_pestat *pes,
                        gbx_mem_reg *xregs, int64_t xreg_cap, int64_t *xreg_off, int64_t *n_xregs,
                        gbx_bsw_seed *xseeds, int64_t xseed_cap, int64_t *n_xseeds,
                        gbx_bsw_seed *xsel_seeds, gbx_bsw_seed_result *xsel_res, int64_t xsel_cap, int64_t *n_xsel,
                        gbx_mem_rescue_stat *stats)
{
    RoctxRange range_("gbx_mem_rescue_host");
    const char *who = "gbx_mem_rescue_host";
    int rc = params_check(p, who);
    if (rc || (rc = ids_check(n_pairs, pair_id0, who))) return rc;
    if (n_regs < 0 || n_seeds < 0 || xreg_cap < 0 || xseed_cap < 0 || xsel_cap < 0 || qer_bytes < 0 || l_pac < 1 || n_contigs < 1) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!reg_off || !contig_off || !pes || !text || !xreg_off || !n_xregs || !n_xseeds || !n_xsel || (n_regs > 0 && !regs) ||
        (n_seeds > 0 && !seeds) || (n_pairs > 0 && (!l_rep || !read_off || !read_len || !qer || !stats)) || (xreg_cap > 0 && !xregs) ||
        (xseed_cap > 0 && !xseeds) || (xsel_cap > 0 && (!xsel_seeds || !xsel_res))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    // everything is checked before the device is touched
    if ((rc = contig_off_check(contig_off, n_contigs, l_pac, who))) return rc;
    if (text_bytes < 2 * l_pac) { set_error("%s: text_bytes = %lld is below 2 l_pac = %lld", who, (long long)text_bytes, (long long)(2 * l_pac)); return GBX_ERR_ARG; }
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
    for (int64_t r = 0; r < n_reads; ++r) {
        if (read_len[r] > MAX_READ) {
            set_error("%s: read %lld has %d bases: mates above %d are not modelled", who, (long long)r, read_len[r], MAX_READ);
            return GBX_ERR_UNSUPPORTED;
        }
        if (read_len[r] < 1 || read_off[r] < 0 || read_off[r] > qer_bytes - read_len[r]) {
            set_error("%s: read %lld: [%lld, %lld + %d) leaves the %lld bytes of qer", who, (long long)r, (long long)read_off[r],
                      (long long)read_off[r], read_len[r], (long long)qer_bytes);
            return GBX_ERR_ARG;
        }
    }
    for (int d = 0; d < 4; ++d)
        if (!pes[d].failed && (pes[d].low < 0 || pes[d].low > pes[d].high || pes[d].high > MAX_WIN)) {
            set_error("%s: pes: direction %d has not failed and has low = %d, high = %d (0 <= low <= high <= 2^20)", who, d, pes[d].low, pes[d].high);
            return GBX_ERR_ARG;
        }
    *n_xregs = 0; *n_xseeds = 0; *n_xsel = 0;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    // capacities on the device: the caller's, cut to what a call can make at most
    const int64_t extra = most_added(n_pairs, n_regs, p->max_matesw);
    const int64_t rcap = std::min(xreg_cap, n_regs + extra), kcap = std::min(xseed_cap, n_seeds + extra), scap = std::min(xsel_cap, n_regs + extra);
    DevBuf drg(L), dro(L), dsd(L), dlr(L), dqo(L), dql(L), dtx(L), dqr(L), dco(L), dpe(L), dn(L), dxr(L), dxo(L), dxs(L), dss(L), dsr(L), dst(L), dw(L);
    const size_t wb = mem_rescue_workspace_bytes(n_pairs, n_regs, p->max_matesw);
    const int64_t counts[4] = {n_regs, 0, 0, 0};
    if ((rc = upload(drg, regs, (size_t)n_regs * sizeof(gbx_mem_reg), st)) || (rc = upload(dro, reg_off, (size_t)(n_reads + 1) * 8, st)) ||
        (rc = upload(dsd, seeds, (size_t)n_seeds * sizeof(gbx_bsw_seed), st)) || (rc = upload(dlr, l_rep, (size_t)n_reads * 4, st)) ||
        (rc = upload(dqo, read_off, (size_t)n_reads * 8, st)) || (rc = upload(dql, read_len, (size_t)n_reads * 4, st)) ||
        (rc = upload(dtx, text, (size_t)(2 * l_pac), st)) || (rc = upload(dqr, qer, (size_t)qer_bytes, st)) ||
        (rc = upload(dco, contig_off, (size_t)(n_contigs + 1) * 8, st)) || (rc = upload(dpe, pes, 4 * sizeof(gbx_mem_pestat), st)) ||
        (rc = upload(dn, counts, 32, st)) || (rc = dxr.alloc((size_t)rcap * sizeof(gbx_mem_reg))) || (rc = dxo.alloc((size_t)(n_reads + 1) * 8)) ||
        (rc = dxs.alloc((size_t)kcap * sizeof(gbx_bsw_seed))) || (rc = dss.alloc((size_t)scap * sizeof(gbx_bsw_seed))) ||
        (rc = dsr.alloc((size_t)scap * sizeof(gbx_bsw_seed_result))) || (rc = dst.alloc((size_t)n_pairs * sizeof(gbx_mem_rescue_stat))) ||
        (rc = dw.alloc(wb)))
        return rc;
    int64_t *const d_n = dn.as<int64_t>();
    const MemRescueIo io{drg.as<gbx_mem_reg>(), dro.as<int64_t>(), d_n, n_regs, dsd.as<gbx_bsw_seed>(), n_seeds, dlr.as<int32_t>(),
                         dqo.as<int64_t>(), dql.as<int32_t>(), dtx.as<uint8_t>(), 2 * l_pac, dqr.as<uint8_t>(), qer_bytes, l_pac, n_contigs,
                         dco.as<int64_t>(), dpe.as<gbx_mem_pestat>(), dxr.as<gbx_mem_reg>(), rcap, dxo.as<int64_t>(), d_n + 1,
                         dxs.as<gbx_bsw_seed>(), kcap, d_n + 2, dss.as<gbx_bsw_seed>(), dsr.as<gbx_bsw_seed_result>(), scap, d_n + 3,
                         dst.as<gbx_mem_rescue_stat>()};
    if ((rc = mem_rescue_launch(p, n_pairs, pair_id0, io, dw.p, wb, st))) return rc;
    int64_t got[3] = {-1, -1, -1};
    GBX_HIP(hipMemcpyAsync(got, d_n + 1, 24, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipMemcpyAsync(xreg_off, dxo.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n_pairs) GBX_HIP(hipMemcpyAsync(stats, dst.p, (size_t)n_pairs * sizeof(gbx_mem_rescue_stat), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    *n_xregs = got[0]; *n_xseeds = got[1]; *n_xsel = got[2];
    if (got[0] < 0 || got[0] > n_regs + extra || got[1] < n_seeds || got[1] > n_seeds + extra || got[2] < 0 || got[2] > got[0]) {
        set_error("%s: the device counted %lld regions, %lld seed records and %lld reported regions from %lld regions and %lld seeds", who,
                  (long long)got[0], (long long)got[1], (long long)got[2], (long long)n_regs, (long long)n_seeds);
        return GBX_ERR_HIP;
    }
    if (got[0] > xreg_cap || got[1] > xseed_cap || got[2] > xsel_cap) {
        set_error("%s: %lld regions, %lld seed records and %lld reported regions do not fit xreg_cap = %lld, xseed_cap = %lld, xsel_cap = %lld",
                  who, (long long)got[0], (long long)got[1], (long long)got[2], (long long)xreg_cap, (long long)xseed_cap, (long long)xsel_cap);
        return GBX_ERR_ARG;
    }
    if (got[0]) GBX_HIP(hipMemcpyAsync(xregs, dxr.p, (size_t)got[0] * sizeof(gbx_mem_reg), hipMemcpyDeviceToHost, st));
    if (kcap) GBX_HIP(hipMemcpyAsync(xseeds, dxs.p, (size_t)kcap * sizeof(gbx_bsw_seed), hipMemcpyDeviceToHost, st));
    if (scap) GBX_HIP(hipMemcpyAsync(xsel_seeds, dss.p, (size_t)scap * sizeof(gbx_bsw_seed), hipMemcpyDeviceToHost, st));
    if (scap) GBX_HIP(hipMemcpyAsync(xsel_res, dsr.p, (size_t)scap * sizeof(gbx_bsw_seed_result), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    if (xseed_cap > kcap) memset(xseeds + kcap, 0, (size_t)(xseed_cap - kcap) * sizeof(gbx_bsw_seed));
    sel_tail_fill(xsel_seeds, xsel_res, scap, xsel_cap);
    return GBX_OK;
}

}  // extern "C"
