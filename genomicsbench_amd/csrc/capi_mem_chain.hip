// capi_mem_chain.hip — seed chaining entries of the C-ABI (include/gbx.h): SMEM hits -> chains -> gbx_bsw_seed records.
#include "capi_common.h"

using namespace gbx;

namespace {
int params_check(const gbx_mem_chain_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc;
    if ((rc = band_check(p->w, who)) || (rc = gap_extend_check(p->e_del, p->e_ins, who))) return rc;
    return number_check("mask_level / drop_ratio", {p->mask_level, p->drop_ratio}, who);
}
}  // namespace

extern "C" {

void gbx_mem_chain_default_params(gbx_mem_chain_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->w = 100; p->max_chain_gap = 10000; p->max_occ = 500; p->min_seed_len = 19; p->min_chain_weight = 0;
    p->max_chain_extend = 1 << 30; p->mask_level = 0.5f; p->drop_ratio = 0.5f;
    p->a = 1; p->o_del = 6; p->e_del = 1; p->o_ins = 6; p->e_ins = 1;
}

size_t gbx_mem_chain_workspace_bytes(int64_t n_reads, int64_t smem_cap, int64_t pos_cap)
{
    return mem_chain_workspace_bytes(n_reads, smem_cap, pos_cap);
}

int gbx_mem_chain_device(const gbx_mem_chain_params *p, int64_t n_reads,
                         const gbx_fmi_smem *d_smems, const int64_t *d_n_smem, int64_t smem_cap, const int64_t *d_smem_off,
                         const int64_t *d_pos, const int64_t *d_n_pos, int64_t pos_cap, const int64_t *d_pos_off,
                         const int64_t *d_read_off, const int32_t *d_read_len,
                         int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                         gbx_mem_chain *d_chains, int64_t chain_cap, int64_t *d_chain_off,
                         gbx_bsw_seed *d_seeds, int64_t seed_cap, int32_t *d_l_rep, int64_t *d_n_chains, int64_t *d_n_seeds,
                         void *d_work, size_t work_bytes, void *stream)
{
    int rc = params_check(p, "gbx_mem_chain_device");
    if (rc) return rc;
    if (n_reads < 0 || smem_cap < 0 || pos_cap < 0 || chain_cap < 0 || seed_cap < 0 || l_pac < 1 || n_contigs < 1) {
        set_error("gbx_mem_chain_device: bad argument");
        return GBX_ERR_ARG;
    }
    if (!d_n_smem || !d_smem_off || !d_n_pos || !d_pos_off || !d_contig_off || !d_chain_off || !d_n_chains || !d_n_seeds || !d_work ||
        (smem_cap > 0 && !d_smems) || (pos_cap > 0 && !d_pos) || (n_reads > 0 && (!d_read_off || !d_read_len || !d_l_rep)) ||
        (chain_cap > 0 && !d_chains) || (seed_cap > 0 && !d_seeds)) {
        set_error("gbx_mem_chain_device: null pointer");
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MemChainIo io{d_smems, d_n_smem, smem_cap, d_smem_off, d_pos, d_n_pos, pos_cap, d_pos_off, d_read_off, d_read_len,
                        l_pac, n_contigs, d_contig_off, d_chains, chain_cap, d_chain_off, d_seeds, seed_cap, d_l_rep, d_n_chains, d_n_seeds};
    return mem_chain_launch(p, n_reads, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mem_chain_host(const gbx_mem_chain_params *p, int64_t n_reads,
                       const gbx_fmi_smem *smems, int64_t n_smem, const int64_t *smem_off,
                       const int64_t *pos, int64_t n_pos, const int64_t *pos_off,
                       const int64_t *read_off, const int32_t *read_len,
                       int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                       gbx_mem_chain *chains, int64_t chain_cap, int64_t *chain_off,
                       gbx_bsw_seed *seeds, int64_t seed_cap, int32_t *l_rep, int64_t *n_chains, int64_t *n_seeds)
{
    RoctxRange range_("gbx_mem_chain_host");
    const char *who = "gbx_mem_chain_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || n_smem < 0 || n_pos < 0 || chain_cap < 0 || seed_cap < 0 || l_pac < 1 || n_contigs < 1) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (!smem_off || !pos_off || !contig_off || !n_chains || !n_seeds || (n_smem > 0 && !smems) || (n_pos > 0 && !pos) ||
        (n_reads > 0 && (!read_off || !read_len)) || (chain_cap > 0 && !chains) || (seed_cap > 0 && !seeds)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    // everything is checked before the device is touched
    if ((rc = contig_off_check(contig_off, n_contigs, l_pac, who))) return rc;
    // (smem_off is checked in the loop over the reads, not by offsets_check: the lowest read with either fault is named)
    if (smem_off[0] < 0 || smem_off[n_reads] > n_smem) { set_error("%s: smem_off leaves the %lld SMEMs", who, (long long)n_smem); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n_reads; ++r) {
        if (smem_off[r + 1] < smem_off[r]) { set_error("%s: smem_off is not monotone at read %lld", who, (long long)r); return GBX_ERR_ARG; }
        if (read_len[r] < 0 || read_off[r] < 0) { set_error("%s: read %lld has a negative length or offset", who, (long long)r); return GBX_ERR_ARG; }
    }
    if ((rc = offsets_check(pos_off, n_smem, n_pos, "pos_off", "hits", "SMEM", who))) return rc;
    *n_chains = 0; *n_seeds = 0;
    if (n_reads == 0) {
        if (chain_off) chain_off[0] = 0;
        return GBX_OK;
    }
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    // capacities on the device: no more chains or seeds than hits can come out, so the caller's are cut to that
    const int64_t ccap = std::min(chain_cap, n_pos), scap = std::min(seed_cap, n_pos);
    DevBuf dsm(L), dso(L), dpos(L), dpo(L), dro(L), drl(L), dco(L), dn(L), dch(L), dcho(L), dsd(L), dlr(L), dw(L);
    const size_t wb = mem_chain_workspace_bytes(n_reads, n_smem, n_pos);
    const int64_t counts[4] = {n_smem, n_pos, 0, 0};
    if ((rc = upload(dsm, smems, (size_t)n_smem * sizeof(gbx_fmi_smem), st)) || (rc = upload(dso, smem_off, (size_t)(n_reads + 1) * 8, st)) ||
        (rc = upload(dpos, pos, (size_t)n_pos * 8, st)) || (rc = upload(dpo, pos_off, (size_t)(n_smem + 1) * 8, st)) ||
        (rc = upload(dro, read_off, (size_t)n_reads * 8, st)) || (rc = upload(drl, read_len, (size_t)n_reads * 4, st)) ||
        (rc = upload(dco, contig_off, (size_t)(n_contigs + 1) * 8, st)) || (rc = upload(dn, counts, 32, st)) ||
        (rc = dch.alloc((size_t)ccap * sizeof(gbx_mem_chain))) || (rc = dcho.alloc((size_t)(n_reads + 1) * 8)) ||
        (rc = dsd.alloc((size_t)scap * sizeof(gbx_bsw_seed))) || (rc = dlr.alloc((size_t)n_reads * 4)) || (rc = dw.alloc(wb)))
        return rc;
    int64_t *const d_n = dn.as<int64_t>();
    const MemChainIo io{dsm.as<gbx_fmi_smem>(), d_n, n_smem, dso.as<int64_t>(), dpos.as<int64_t>(), d_n + 1, n_pos, dpo.as<int64_t>(),
                        dro.as<int64_t>(), drl.as<int32_t>(), l_pac, n_contigs, dco.as<int64_t>(), dch.as<gbx_mem_chain>(), ccap,
                        dcho.as<int64_t>(), dsd.as<gbx_bsw_seed>(), scap, dlr.as<int32_t>(), d_n + 2, d_n + 3};
    if ((rc = mem_chain_launch(p, n_reads, io, dw.p, wb, st))) return rc;
    int64_t got[2] = {-1, -1};
    GBX_HIP(hipMemcpyAsync(got, d_n + 2, 16, hipMemcpyDeviceToHost, st));
    if (chain_off) GBX_HIP(hipMemcpyAsync(chain_off, dcho.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    if (l_rep) GBX_HIP(hipMemcpyAsync(l_rep, dlr.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    *n_chains = got[0]; *n_seeds = got[1];
    if (got[0] < 0 || got[1] < 0 || got[0] > n_pos || got[1] > n_pos) {
        set_error("%s: the device counted %lld chains and %lld seeds from %lld hits", who, (long long)got[0], (long long)got[1], (long long)n_pos);
        return GBX_ERR_HIP;
    }
    if (got[0] > chain_cap || got[1] > seed_cap) {
        set_error("%s: %lld chains and %lld seeds do not fit chain_cap = %lld, seed_cap = %lld", who, (long long)got[0], (long long)got[1],
                  (long long)chain_cap, (long long)seed_cap);
        return GBX_ERR_ARG;
    }
    if (got[0]) GBX_HIP(hipMemcpyAsync(chains, dch.p, (size_t)got[0] * sizeof(gbx_mem_chain), hipMemcpyDeviceToHost, st));
    if (got[1]) GBX_HIP(hipMemcpyAsync(seeds, dsd.p, (size_t)got[1] * sizeof(gbx_bsw_seed), hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    return GBX_OK;
}

}  // extern "C"
