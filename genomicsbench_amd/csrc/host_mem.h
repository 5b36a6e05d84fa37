// host_mem.h — what the bwa-mem entries (capi_mem_chain / _cigar / _regs / _pair / _rescue / _sam .hip) share on the host: the argument checks
// with their error texts, the tail fill of a CIGAR list and the upload of one input.  Every check sets the error text and
// returns GBX_ERR_ARG (mapq_coef_len_check: GBX_ERR_UNSUPPORTED), or returns GBX_OK.
#pragma once
#include <initializer_list>

namespace gbx {

// contig_off[0 .. n_contigs] runs from 0 to l_pac, strictly increasing
inline int contig_off_check(const int64_t *contig_off, int32_t n_contigs, int64_t l_pac, const char *who)
{
    if (contig_off[0] != 0 || contig_off[n_contigs] != l_pac) {
        set_error("%s: contig_off must run from 0 to l_pac = %lld", who, (long long)l_pac);
        return GBX_ERR_ARG;
    }
    for (int32_t c = 0; c < n_contigs; ++c)
        if (contig_off[c + 1] <= contig_off[c]) { set_error("%s: contig_off is not strictly increasing at contig %d", who, c); return GBX_ERR_ARG; }
    return GBX_OK;
}

// off[0 .. n] stays within [0, total] and never decreases; `name` is the array, `things` what it indexes, `unit` what has an entry
inline int offsets_check(const int64_t *off, int64_t n, int64_t total, const char *name, const char *things, const char *unit, const char *who)
{
    if (off[0] < 0 || off[n] > total) { set_error("%s: %s leaves the %lld %s", who, name, (long long)total, things); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n; ++r)
        if (off[r + 1] < off[r]) { set_error("%s: %s is not monotone at %s %lld", who, name, unit, (long long)r); return GBX_ERR_ARG; }
    return GBX_OK;
}

// ---- the pieces of a stage's params_check
inline int gap_extend_check(int e_del, int e_ins, const char *who)
{
    if (e_del < 1 || e_ins < 1) { set_error("%s: e_del = %d, e_ins = %d (both at least 1)", who, e_del, e_ins); return GBX_ERR_ARG; }
    return GBX_OK;
}
inline int match_check(int a, int b, const char *who)
{
    if (a < 1 || (long long)a + b < 1) { set_error("%s: a = %d, b = %d (a and a + b at least 1)", who, a, b); return GBX_ERR_ARG; }
    return GBX_OK;
}
inline int band_check(int w, const char *who)
{
    if (w < 0) { set_error("%s: w = %d is negative", who, w); return GBX_ERR_ARG; }
    return GBX_OK;
}
inline int mapq_coef_len_check(int mapq_coef_len, const char *who)
{
    if (mapq_coef_len <= 0) {
        set_error("%s: mapq_coef_len = %d: bwa's mapq formula for mapq_coef_len <= 0 is not modelled", who, mapq_coef_len);
        return GBX_ERR_UNSUPPORTED;
    }
    return GBX_OK;
}
// names: the fields as the text lists them, "mask_level / drop_ratio"
inline int number_check(const char *names, std::initializer_list<float> values, const char *who)
{
    for (float v : values)
        if (!(v == v)) { set_error("%s: %s is not a number", who, names); return GBX_ERR_ARG; }
    return GBX_OK;
}

// the CIGAR list from record `from` up to cap: zeroed seeds (len = 0 is no seed) with results of all -1
inline void sel_tail_fill(gbx_bsw_seed *seeds, gbx_bsw_seed_result *res, int64_t from, int64_t cap)
{
    if (from >= cap) return;
    memset(seeds + from, 0, (size_t)(cap - from) * sizeof(gbx_bsw_seed));
    memset(res + from, 0xff, (size_t)(cap - from) * sizeof(gbx_bsw_seed_result));
}

}  // namespace gbx
