// host_mm.h — the checks the host entries of the long-read stages share (capi_mm_map.hip, capi_mm_align.hip), all made before a
// device is touched.
#pragma once
#include "capi_common.h"

namespace gbx {

// off[0 .. n]: from 0, never decreasing, steps below 2^bits
inline int mm_offsets_check(const int64_t *off, int64_t n, const char *name, const char *what, const char *who, int bits = 31)
{
    if (!off) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (off[0] != 0) { set_error("%s: %s[0] must be 0", who, name); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = off[r + 1] - off[r];
        if (len < 0) { set_error("%s: %s is not monotone at %s %lld", who, name, what, (long long)r); return GBX_ERR_ARG; }
        if (len >= (1ll << bits)) {
            set_error("%s: %s %lld spans %lld in %s (fewer than 2^%d)", who, what, (long long)r, (long long)len, name, bits);
            return GBX_ERR_UNSUPPORTED;
        }
    }
    return GBX_OK;
}

inline int mm_reads_check(int64_t n_reads, const char *who)
{
    if (n_reads < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_reads > GBX_MM_MAX_READS) { set_error("%s: %lld reads (at most %d a call)", who, (long long)n_reads, GBX_MM_MAX_READS); return GBX_ERR_UNSUPPORTED; }
    return GBX_OK;
}

// every region lies in the read that reg_off puts it in
inline int mm_regions_check(const gbx_mm_reg *regs, const int64_t *reg_off, int64_t n_reads, const char *who)
{
    for (int64_t r = 0; r < n_reads; ++r)
        for (int64_t g = reg_off[r]; g < reg_off[r + 1]; ++g)
            if (regs[g].read != r) { set_error("%s: region %lld names read %d, it lies in read %lld", who, (long long)g, regs[g].read, (long long)r); return GBX_ERR_ARG; }
    return GBX_OK;
}

}  // namespace gbx
