// capi_mem_regs.hip — alignment-region entries of the C-ABI (include/gbx.h): chains, seeds and their extension results ->
// gbx_mem_reg records and the CIGAR list (the seeds and results gbx_mem_cigar_* is to align).
#include <cmath>
#include "capi_common.h"

using namespace gbx;

namespace {
int params_check(const gbx_mem_regs_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc;
    if ((rc = gap_extend_check(p->e_del, p->e_ins, who)) || (rc = match_check(p->a, p->b, who)) || (rc = band_check(p->w, who)) ||
        (rc = mapq_coef_len_check(p->mapq_coef_len, who)))
        return rc;
    return number_check("mask_level / mask_level_redun / drop_ratio / mapq_coef_fac",
                        {p->mask_level, p->mask_level_redun, p->drop_ratio, p->mapq_coef_fac}, who);
}
}  // namespace

extern "C" {

void gbx_mem_regs_default_params(gbx_mem_regs_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->a = 1; p->b = 4; p->o_del = 6; p->e_del = 1; p->o_ins = 6; p->e_ins = 1; p->w = 100; p->max_chain_gap = 10000;
    p->min_seed_len = 19; p->T = 30; p->mapq_coef_len = 50; p->mapq_coef_fac = (float)log((double)p->mapq_coef_len);
    p->mask_level = 0.5f; p->mask_level_redun = 0.95f; p->drop_ratio = 0.5f;
}

size_t gbx_mem_regs_workspace_bytes(int64_t n_reads, int64_t seed_cap)
{
    return mem_regs_workspace_bytes(n_reads, seed_cap);
}

int gbx_mem_regs_device(const gbx_mem_regs_params *p, int64_t n_reads, int64_t read_id0,
                        const gbx_mem_chain *d_chains, const int64_t *d_n_chains, int64_t chain_cap, const int64_t *d_chain_off,
                        const gbx_bsw_seed *d_seeds, const int64_t *d_n_seeds, int64_t seed_cap,
                        const gbx_bsw_seed_result *d_res, const int32_t *d_l_rep,
                        gbx_mem_reg *d_regs, int64_t reg_cap, int64_t *d_reg_off, int64_t *d_n_regs,
                        gbx_bsw_seed *d_sel_seeds, gbx_bsw_seed_result *d_sel_res, int64_t sel_cap, int64_t *d_n_sel,
                        void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mem_regs_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || chain_cap < 0 || seed_cap < 0 || reg_cap < 0 || sel_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!d_n_chains || !d_chain_off || !d_n_seeds || !d_reg_off || !d_n_regs || !d_n_sel || !d_work || (chain_cap > 0 && !d_chains) ||
        (seed_cap > 0 && (!d_seeds || !d_res)) || (n_reads > 0 && !d_l_rep) || (reg_cap > 0 && !d_regs) ||
        (sel_cap > 0 && (!d_sel_seeds || !d_sel_res))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MemRegsIo io{d_chains, d_n_chains, chain_cap, d_chain_off, d_seeds, d_n_seeds, seed_cap, d_res, d_l_rep,
                       d_regs, reg_cap, d_reg_off, d_n_regs, d_sel_seeds, d_sel_res, sel_cap, d_n_sel};
    return mem_regs_launch(p, n_reads, read_id0, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mem_regs_host(const gbx_mem_regs_params *p, int64_t n_reads, int64_t read_id0,
                      const gbx_mem_chain *chains, int64_t n_chains, const int64_t *chain_off,
                      const gbx_bsw_seed *seeds, int64_t n_seeds, const gbx_bsw_seed_result *res, const int32_t *l_rep,
                      gbx_mem_reg *regs, int64_t reg_cap, int64_t *reg_off, int64_t *n_regs,
                      gbx_bsw_seed *sel_seeds, gbx_bsw_seed_result *sel_res, int64_t sel_cap, int64_t *n_sel)
{
    RoctxRange range_("gbx_mem_regs_host");
    const char *who = "gbx_mem_regs_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || n_chains < 0 || n_seeds < 0 || reg_cap < 0 || sel_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!chain_off || !n_regs || !n_sel || (n_chains > 0 && !chains) || (n_seeds > 0 && (!seeds || !res)) || (n_reads > 0 && !l_rep) ||
        (reg_cap > 0 && !regs) || (sel_cap > 0 && (!sel_seeds || !sel_res))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    // everything is checked before the device is touched
    if ((rc = offsets_check(chain_off, n_reads, n_chains, "chain_off", "chains", "read", who))) return rc;
    for (int64_t c = 0; c < n_chains; ++c)
        if (chains[c].seed_off < 0 || chains[c].n_seeds < 0 || chains[c].seed_off > n_seeds || chains[c].n_seeds > n_seeds - chains[c].seed_off) {
            set_error("%s: chain %lld: its seeds [%lld, %lld + %d) leave the %lld seeds", who, (long long)c, (long long)chains[c].seed_off,
                      (long long)chains[c].seed_off, chains[c].n_seeds, (long long)n_seeds);
            return GBX_ERR_ARG;
        }
    *n_regs = 0; *n_sel = 0;
    if (n_reads == 0 || n_seeds == 0 || n_chains == 0) {
        if (reg_off) memset(reg_off, 0, (size_t)(n_reads + 1) * 8);
        sel_tail_fill(sel_seeds, sel_res, 0, sel_cap);
        return GBX_OK;
    }
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    // capacities on the device: no more regions than seeds can come out, so the caller's are cut to that
    const int64_t rcap = std::min(reg_cap, n_seeds), scap = std::min(sel_cap, n_seeds);
    DevBuf dch(L), dco(L), dsd(L), drs(L), dlr(L), dn(L), drg(L), dro(L), dss(L), dsr(L), dw(L);
    const size_t wb = mem_regs_workspace_bytes(n_reads, n_seeds);
    const int64_t counts[4] = {n_chains, n_seeds, 0, 0};
    if ((rc = upload(dch, chains, (size_t)n_chains * sizeof(gbx_mem_chain), st)) || (rc = upload(dco, chain_off, (size_t)(n_reads + 1) * 8, st)) ||
        (rc = upload(dsd, seeds, (size_t)n_seeds * sizeof(gbx_bsw_seed), st)) ||
        (rc = upload(drs, res, (size_t)n_seeds * sizeof(gbx_bsw_seed_result), st)) || (rc = upload(dlr, l_rep, (size_t)n_reads * 4, st)) ||
        (rc = upload(dn, counts, 32, st)) || (rc = drg.alloc((size_t)rcap * sizeof(gbx_mem_reg))) || (rc = dro.alloc((size_t)(n_reads + 1) * 8)) ||
        (rc = dss.alloc((size_t)scap * sizeof(gbx_bsw_seed))) || (rc = dsr.alloc((size_t)scap * sizeof(gbx_bsw_seed_result))) || (rc = dw.alloc(wb)))
        return rc;
    int64_t *const d_n = dn.as<int64_t>();
    const MemRegsIo io{dch.as<gbx_mem_chain>(), d_n, n_chains, dco.as<int64_t>(), dsd.as<gbx_bsw_seed>(), d_n + 1, n_seeds,
                       drs.as<gbx_bsw_seed_result>(), dlr.as<int32_t>(), drg.as<gbx_mem_reg>(), rcap, dro.as<int64_t>(), d_n + 2,
                       dss.as<gbx_bsw_seed>(), dsr.as<gbx_bsw_seed_result>(), scap, d_n + 3};
    if ((rc = mem_regs_launch(p, n_reads, read_id0, io, dw.p, wb, st))) return rc;
    int64_t got[2] = {-1, -1};
    GBX_HIP(hipMemcpyAsync(got, d_n + 2, 16, hipMemcpyDeviceToHost, st));
    if (reg_off) GBX_HIP(hipMemcpyAsync(reg_off, dro.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    *n_regs = got[0]; *n_sel = got[1];
    if (got[0] < 0 || got[1] < 0 || got[0] > n_seeds || got[1] > got[0]) {
        set_error("%s: the device counted %lld regions and %lld reported ones from %lld seeds", who, (long long)got[0], (long long)got[1],
                  (long long)n_seeds);
        return GBX_ERR_HIP;
    }
    if (got[0] > reg_cap || got[1] > sel_cap) {
        set_error("%s: %lld regions and %lld reported ones do not fit reg_cap = %lld, sel_cap = %lld", who, (long long)got[0], (long long)got[1],
                  (long long)reg_cap, (long long)sel_cap);
        return GBX_ERR_ARG;
    }
    if (got[0]) GBX_HIP(hipMemcpyAsync(regs, drg.p, (size_t)got[0] * sizeof(gbx_mem_reg), hipMemcpyDeviceToHost, st));
    if (scap) GBX_HIP(hipMemcpyAsync(sel_seeds, dss.p, (size_t)scap * sizeof(gbx_bsw_seed), hipMemcpyDeviceToHost, st));
    if (scap) GBX_HIP(hipMemcpyAsync(sel_res, dsr.p, (size_t)scap * sizeof(gbx_bsw_seed_result), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    sel_tail_fill(sel_seeds, sel_res, scap, sel_cap);
    return GBX_OK;
}

}  // extern "C"
