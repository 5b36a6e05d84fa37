// dbg_host.h — the argument checks and the reads' slot prefix that the dbg entries (capi_dbg.hip) and the assembly entries behind
// them (capi_dbg_asm.hip) share.
#pragma once
#include "capi_common.h"
#include "dev_prims.h"      // align256

namespace gbx {

inline int dbg_params_check(const gbx_dbg_params *p, const char *who)
{
    if (!p) { set_error("%s: null params", who); return GBX_ERR_ARG; }
    if (p->k < GBX_DBG_MIN_K || p->k > GBX_DBG_MAX_K || p->min_qual < 0 || p->min_qual > 255 || p->region_size < 1) {
        set_error("%s: k = %d (%d..%d), min_qual = %d (0..255), region_size = %d (>= 1)", who, p->k, GBX_DBG_MIN_K, GBX_DBG_MAX_K, p->min_qual,
                  p->region_size);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

// rcp[r] = occurrence slots of the reads before r
inline std::vector<int64_t> dbg_read_prefix(int k, int64_t n, const int64_t *seq_off)
{
    std::vector<int64_t> rcp((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) rcp[(size_t)r + 1] = rcp[(size_t)r] + std::max<int64_t>(0, seq_off[r + 1] - seq_off[r] - k - 1);
    return rcp;
}

inline int dbg_check(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, const char *who)
{
    int rc = dbg_params_check(p, who);
    if (rc) return rc;
    if (!R || !W) { set_error("%s: null reads or windows", who); return GBX_ERR_ARG; }
    const int64_t n = R->n_reads, nw = W->n_win;
    if (n < 0 || R->seq_bytes < 0 || nw < 0 || W->ref_bytes < 0) {
        set_error("%s: n_reads %lld, seq_bytes %lld, n_win %lld, ref_bytes %lld", who, (long long)n, (long long)R->seq_bytes, (long long)nw,
                  (long long)W->ref_bytes);
        return GBX_ERR_ARG;
    }
    if (!R->seq_off || (n > 0 && !R->flag) || (R->seq_bytes > 0 && (!R->seq || !R->qual))) { set_error("%s: null read arrays", who); return GBX_ERR_ARG; }
    if (!W->ref_off || (nw > 0 && (!W->ref_pos || !W->read_lo || !W->read_hi)) || (W->ref_bytes > 0 && !W->ref)) {
        set_error("%s: null window arrays", who);
        return GBX_ERR_ARG;
    }
    if (R->seq_off[0] < 0 || R->seq_off[n] > R->seq_bytes) { set_error("%s: seq_off outside [0, seq_bytes]", who); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n; ++r)
        if (R->seq_off[r + 1] < R->seq_off[r]) { set_error("%s: seq_off decreases at read %lld", who, (long long)r); return GBX_ERR_ARG; }
    if (W->ref_off[0] < 0 || W->ref_off[nw] > W->ref_bytes) { set_error("%s: ref_off outside [0, ref_bytes]", who); return GBX_ERR_ARG; }
    for (int64_t w = 0; w < nw; ++w) {
        const char *bad = nullptr;
        if (W->ref_off[w + 1] < W->ref_off[w]) bad = "ref_off decreases";
        else if (W->ref_pos[w] < 0 || W->ref_pos[w] + (W->ref_off[w + 1] - W->ref_off[w]) > INT32_MAX) bad = "its reference lies outside [0, 2^31)";
        else if (W->read_lo[w] < 0 || W->read_lo[w] > W->read_hi[w] || W->read_hi[w] > n) bad = "its reads are not 0 <= read_lo <= read_hi <= n_reads";
        if (bad) { set_error("%s: window %lld: %s", who, (long long)w, bad); return GBX_ERR_ARG; }
    }
    if (W->ref_bytes + R->seq_bytes >= ((int64_t)1 << 40)) { set_error("%s: more than 2^40 bytes of reference and reads", who); return GBX_ERR_UNSUPPORTED; }
    return GBX_OK;
}

}  // namespace gbx
