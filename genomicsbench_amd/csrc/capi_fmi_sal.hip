// capi_fmi_sal.hip — suffix-array lookup entries of the C-ABI (include/gbx.h): SMEM hits -> text positions.
#include "capi_common.h"

using namespace gbx;

namespace {
int sal_index_check(const gbx_fmi_index *idx, const gbx_fmi_sa *sa, const char *who)
{
    if (!idx || !sa) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc = fmi_index_check(idx, (1ll << 40) - 1, who);
    if (rc) return rc;
    if (sa->sa_compx != 0 && sa->sa_compx != 3) { set_error("%s: sa_compx must be 3 or 0", who); return GBX_ERR_ARG; }
    const int64_t want = sa->sa_compx ? (idx->ref_seq_len >> 3) + 1 : idx->ref_seq_len;
    if (sa->n_sa != want) {
        set_error("%s: n_sa = %lld, sa_compx %d wants %lld", who, (long long)sa->n_sa, sa->sa_compx, (long long)want);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

// The device copies of the samples gbx_fmi_sal_host keeps between calls, one per device, keyed like the indexes by their
// scalars and a fingerprint of their content.  The layout width is part of the key: GBX_FMI_WIDE=1 switches it at the same
// length.
int sa_acquire(const gbx_fmi_sa *sa, int64_t len, int dev, hipStream_t s, void **out)
{
    const HostCacheKey key{dev, {len, sa->n_sa, sa->sa_compx, fmi_sa_wide(len)},
                           sampled_fingerprint(sa->n_sa, [&](auto &mix, size_t i) { mix(&sa->ms_byte[i], 1); mix(&sa->ls_word[i], 4); })};
    return fmi_sa_cache.acquire(key, [&](void **d_sa) {
        const size_t bytes = fmi_sa_bytes(sa->n_sa, len), n = (size_t)sa->n_sa;
        void *d_ms = nullptr, *d_ls = nullptr;
        hipError_t e = hipMalloc(d_sa, bytes);
        if (e != hipSuccess) *d_sa = nullptr;
        if (e == hipSuccess) e = hipMalloc(&d_ms, n);
        if (e == hipSuccess) e = hipMalloc(&d_ls, n * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(d_ms, sa->ms_byte, n, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_ls, sa->ls_word, n * 4, hipMemcpyHostToDevice, s);
        int rc = e == hipSuccess ? GBX_OK : hip_fail(e, "fmi sample upload");
        if (!rc) {
            gbx_fmi_sa dsa = *sa;
            dsa.ms_byte = (const int8_t *)d_ms;
            dsa.ls_word = (const uint32_t *)d_ls;
            rc = fmi_sa_build(&dsa, len, *d_sa, bytes, s);
            const hipError_t e2 = hipStreamSynchronize(s);
            if (!rc && e2 != hipSuccess) rc = hip_fail(e2, "fmi sample build");
        }
        if (d_ms) (void)hipFree(d_ms);
        if (d_ls) (void)hipFree(d_ls);
        if (rc && *d_sa) { (void)hipFree(*d_sa); *d_sa = nullptr; }
        return rc;
    }, out);
}
}  // namespace

HostCache gbx::fmi_sa_cache;

extern "C" {

size_t gbx_fmi_sa_bytes(int64_t n_sa, int64_t ref_seq_len) { return fmi_sa_bytes(n_sa, ref_seq_len); }

int gbx_fmi_sa_build(const gbx_fmi_sa *sa, int64_t ref_seq_len, void *d_sa, size_t sa_bytes, void *stream)
{
    if (!sa || !sa->ms_byte || !sa->ls_word || !d_sa) { set_error("gbx_fmi_sa_build: null pointer"); return GBX_ERR_ARG; }
    int rc = require_device();
    if (rc) return rc;
    return fmi_sa_build(sa, ref_seq_len, d_sa, sa_bytes, (hipStream_t)stream);
}

size_t gbx_fmi_sal_workspace_bytes(int64_t smem_cap, int64_t pos_cap) { return fmi_sal_workspace_bytes(smem_cap, pos_cap); }

int gbx_fmi_sal_device(const gbx_fmi_index *idx, const void *d_index, const gbx_fmi_sa *sa, const void *d_sa,
                       const gbx_fmi_smem *d_smems, const int64_t *d_n_smem, int64_t smem_cap, int32_t max_occ,
                       int64_t *d_pos, int64_t pos_cap, int64_t *d_pos_off, int64_t *d_n_pos, void *d_work, size_t work_bytes,
                       void *stream)
{
    int rc = sal_index_check(idx, sa, "gbx_fmi_sal_device");
    if (rc) return rc;
    if (smem_cap < 0 || pos_cap < 0) { set_error("gbx_fmi_sal_device: bad argument"); return GBX_ERR_ARG; }
    if (!d_index || !d_sa || !d_n_smem || !d_pos_off || !d_n_pos || !d_work || (smem_cap > 0 && !d_smems) || (pos_cap > 0 && !d_pos)) {
        set_error("gbx_fmi_sal_device: null pointer");
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return fmi_sal_launch(idx, d_index, sa, d_sa, d_smems, d_n_smem, smem_cap, max_occ, d_pos, pos_cap, d_pos_off, d_n_pos, d_work,
                          work_bytes, (hipStream_t)stream);
}

int gbx_fmi_sal_steps(const void *d_work, int64_t *steps, int64_t *max_steps, void *stream)
{
    if (!d_work || !steps || !max_steps) { set_error("gbx_fmi_sal_steps: null pointer"); return GBX_ERR_ARG; }
    return fmi_sal_read_steps(d_work, steps, max_steps, (hipStream_t)stream);
}

int gbx_fmi_sal_host(const gbx_fmi_index *idx, const gbx_fmi_sa *sa, const gbx_fmi_smem *smems, int64_t n_smem, int32_t max_occ,
                     int64_t *pos, int64_t pos_cap, int64_t *pos_off, int64_t *n_pos)
{
    RoctxRange range_("gbx_fmi_sal_host");
    int rc = sal_index_check(idx, sa, "gbx_fmi_sal_host");
    if (rc) return rc;
    if (n_smem < 0 || pos_cap < 0) { set_error("gbx_fmi_sal_host: bad argument"); return GBX_ERR_ARG; }
    if (!idx->cp_occ || !sa->ms_byte || !sa->ls_word || !n_pos || (n_smem > 0 && !smems) || (pos_cap > 0 && !pos)) {
        set_error("gbx_fmi_sal_host: null pointer");
        return GBX_ERR_ARG;
    }
    // every SMEM is checked, and the hits counted, before the device is touched
    const int64_t len = idx->ref_seq_len;
    int64_t total = 0;
    for (int64_t j = 0; j < n_smem; ++j) {
        const int64_t k = smems[j].k, s = smems[j].s;
        if (k < 0 || s < 1 || k > len - s) {
            set_error("gbx_fmi_sal_host: SMEM %lld (k %lld, s %lld) is not an interval of the %lld SA rows", (long long)j, (long long)k,
                      (long long)s, (long long)len);
            return GBX_ERR_ARG;
        }
        total += max_occ > 0 && s > max_occ ? max_occ : s;
    }
    *n_pos = total;
    if (total > pos_cap) {
        set_error("gbx_fmi_sal_host: %lld hits do not fit pos_cap = %lld", (long long)total, (long long)pos_cap);
        return GBX_ERR_ARG;
    }
    if (n_smem == 0) {
        if (pos_off) pos_off[0] = 0;
        return GBX_OK;
    }
    if ((rc = require_device())) return rc;
    int dev = 0;
    GBX_HIP(hipGetDevice(&dev));
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    HostCache::Use index(fmi_index_cache), samples(fmi_sa_cache);
    if ((rc = fmi_index_acquire(idx, dev, st, &index.p))) return rc;
    if ((rc = sa_acquire(sa, len, dev, st, &samples.p))) return rc;
    DevBuf dsm(L), dn(L), dpos(L), doff(L), dnp(L), dw(L);
    const size_t wb = fmi_sal_workspace_bytes(n_smem, total);
    if ((rc = dsm.alloc((size_t)n_smem * sizeof(gbx_fmi_smem))) || (rc = dn.alloc(8)) || (rc = dpos.alloc((size_t)total * 8)) ||
        (rc = doff.alloc((size_t)(n_smem + 1) * 8)) || (rc = dnp.alloc(8)) || (rc = dw.alloc(wb)))
        return rc;
    GBX_HIP(hipMemcpyAsync(dsm.p, smems, (size_t)n_smem * sizeof(gbx_fmi_smem), hipMemcpyHostToDevice, st));
    GBX_HIP(hipMemcpyAsync(dn.p, &n_smem, 8, hipMemcpyHostToDevice, st));
    if ((rc = fmi_sal_launch(idx, index.p, sa, samples.p, dsm.as<gbx_fmi_smem>(), dn.as<int64_t>(), n_smem, max_occ, dpos.as<int64_t>(),
                             total, doff.as<int64_t>(), dnp.as<int64_t>(), dw.p, wb, st)))
        return rc;
    int64_t got = -1;
    GBX_HIP(hipMemcpyAsync(&got, dnp.p, 8, hipMemcpyDeviceToHost, st));
    if (total > 0) GBX_HIP(hipMemcpyAsync(pos, dpos.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    if (pos_off) GBX_HIP(hipMemcpyAsync(pos_off, doff.p, (size_t)(n_smem + 1) * 8, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    if (got != total) {
        set_error("gbx_fmi_sal_host: the device counted %lld hits, the host %lld", (long long)got, (long long)total);
        return GBX_ERR_HIP;
    }
    return GBX_OK;
}

}  // extern "C"
