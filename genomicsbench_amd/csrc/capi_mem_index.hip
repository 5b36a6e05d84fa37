// capi_mem_index.hip — index construction entries of the C-ABI (include/gbx.h): a genome -> count[], sentinel_index, the CP_OCC
// checkpoints and the suffix-array samples, built by mem_index_kernels.hip.  gbx_mem_index_build, which hands the device arrays
// on to the aligner's index, is beside gbx_mem_index_create in capi_mem_align.hip.
#include "capi_common.h"

using namespace gbx;

namespace gbx {

// the host checks every build entry makes before any device work; genome: host codes, or null when they are on the device
int fmi_build_check(const uint8_t *genome, int64_t l_pac, int32_t sa_compx, const char *who)
{
    if (l_pac < 1) { set_error("%s: l_pac = %lld (at least 1)", who, (long long)l_pac); return GBX_ERR_ARG; }
    if (!fmi_build_fits(l_pac)) {
        set_error("%s: l_pac = %lld: positions and ranks are 32-bit, 2 l_pac + 1 must not exceed 2^32 - 1 (l_pac <= 2147483647)", who, (long long)l_pac);
        return GBX_ERR_UNSUPPORTED;
    }
    if (sa_compx != 3 && sa_compx != 0) { set_error("%s: sa_compx = %d (3 or 0)", who, sa_compx); return GBX_ERR_ARG; }
    if (genome)
        for (int64_t i = 0; i < l_pac; ++i)
            if (genome[i] > 3) { set_error("%s: base %lld has code %d (0..3)", who, (long long)i, (int)genome[i]); return GBX_ERR_ARG; }
    return GBX_OK;
}

}  // namespace gbx

namespace {
struct Dev {                              // one device allocation, freed with its owner
    void *p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 1)); }
};
struct OwnStream {
    hipStream_t s = nullptr;
    ~OwnStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};
}  // namespace

extern "C" {

size_t gbx_fmi_build_workspace_bytes(int64_t l_pac) { return fmi_build_workspace_bytes(l_pac); }

int gbx_fmi_build_device(const uint8_t *d_genome, int64_t l_pac, int32_t sa_compx, void *d_cp_occ, int8_t *d_ms, uint32_t *d_ls, uint8_t *d_text,
                         int64_t *d_info, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_fmi_build_device";
    if (!d_genome || !d_cp_occ || !d_ms || !d_ls || !d_info || !d_work) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc = fmi_build_check(nullptr, l_pac, sa_compx, who);
    if (rc) return rc;
    const size_t need = fmi_build_workspace_bytes(l_pac);
    if (work_bytes < need) { set_error("%s: workspace too small (%zu bytes, %zu needed)", who, work_bytes, need); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    return fmi_build_launch(d_genome, l_pac, sa_compx, (gbx_fmi_cp_occ *)d_cp_occ, d_ms, d_ls, d_text, d_info, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_fmi_build_rounds(int64_t *slots, int32_t cap, int32_t *n_rounds)
{
    if (!n_rounds || cap < 0 || (cap > 0 && !slots)) { set_error("gbx_fmi_build_rounds: bad argument"); return GBX_ERR_ARG; }
    return fmi_build_rounds(slots, cap, n_rounds);
}

int gbx_fmi_build_host(const uint8_t *genome, int64_t l_pac, int32_t sa_compx, gbx_fmi_index *idx, gbx_fmi_cp_occ *cp_occ, int8_t *ms, uint32_t *ls,
                       int64_t *info)
{
    RoctxRange range_("gbx_fmi_build_host");
    const char *who = "gbx_fmi_build_host";
    if (!genome || !idx || !cp_occ || !ms || !ls) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc = fmi_build_check(genome, l_pac, sa_compx, who);
    if (rc) return rc;
    if ((rc = require_device())) return rc;
    const int64_t N = 2 * l_pac + 1;
    const size_t ncp = (size_t)(N >> 6) + 1, n_sa = (size_t)(sa_compx ? (N >> 3) + 1 : N), wb = fmi_build_workspace_bytes(l_pac);
    Dev dg, dcp, dms, dls, dinfo, dw;
    OwnStream st;
    GBX_HIP(hipStreamCreate(&st.s));
    GBX_HIP(dg.alloc((size_t)l_pac));
    GBX_HIP(dcp.alloc(ncp * sizeof(gbx_fmi_cp_occ)));
    GBX_HIP(dms.alloc(n_sa));
    GBX_HIP(dls.alloc(n_sa * 4));
    GBX_HIP(dinfo.alloc(64));
    GBX_HIP(dw.alloc(wb));
    GBX_HIP(hipMemcpyAsync(dg.p, genome, (size_t)l_pac, hipMemcpyHostToDevice, st.s));
    if ((rc = fmi_build_launch((const uint8_t *)dg.p, l_pac, sa_compx, (gbx_fmi_cp_occ *)dcp.p, (int8_t *)dms.p, (uint32_t *)dls.p, nullptr,
                               (int64_t *)dinfo.p, dw.p, wb, st.s)))
        return rc;
    int64_t w[8];
    GBX_HIP(hipMemcpyAsync(w, dinfo.p, 64, hipMemcpyDeviceToHost, st.s));
    GBX_HIP(hipMemcpyAsync(cp_occ, dcp.p, ncp * sizeof(gbx_fmi_cp_occ), hipMemcpyDeviceToHost, st.s));
    GBX_HIP(hipMemcpyAsync(ms, dms.p, n_sa, hipMemcpyDeviceToHost, st.s));
    GBX_HIP(hipMemcpyAsync(ls, dls.p, n_sa * 4, hipMemcpyDeviceToHost, st.s));
    GBX_HIP(hipStreamSynchronize(st.s));
    idx->ref_seq_len = N;
    for (int c = 0; c < 5; ++c) idx->count[c] = w[c];
    idx->sentinel_index = w[5];
    idx->cp_occ = cp_occ;
    if (info) memcpy(info, w, 64);
    return GBX_OK;
}

}  // extern "C"
