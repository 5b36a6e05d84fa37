// capi_kmer.hip — canonical k-mer counting entries of the C-ABI (include/gbx.h, kmer section).
#include "capi_common.h"

using namespace gbx;

namespace {
int kmer_params_check(const gbx_kmer_params *p, const char *who)
{
    if (!p) { set_error("%s: null params", who); return GBX_ERR_ARG; }
    if (p->k < 1 || p->k > GBX_KMER_MAX_K) {
        set_error("%s: k = %d outside 1..%d (the reference's flat counter, R/vertex_index.cpp:518-521)", who, p->k, GBX_KMER_MAX_K);
        return GBX_ERR_ARG;
    }
    if (p->n_hist < 0 || p->n_hist == 1 || p->n_hist > GBX_KMER_MAX_HIST) {
        set_error("%s: n_hist = %d: 0, or 2..%d", who, p->n_hist, GBX_KMER_MAX_HIST);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

// one host call at a time: the table of a call is up to 4 GB of device memory
std::mutex kmer_host_mu;
}  // namespace

extern "C" {

size_t gbx_kmer_workspace_bytes(int32_t k, int64_t n_reads, int32_t n_hist)
{
    (void)n_hist;                                                  // the histogram lives in LDS and in the caller's d_hist
    if (k < 1 || k > GBX_KMER_MAX_K || n_reads < 0) return 0;
    return kmer_workspace_bytes(k, n_reads);
}

int gbx_kmer_count_device(const gbx_kmer_params *p, int64_t n_reads, const uint8_t *d_enc, const int64_t *d_read_off,
                          const int32_t *d_read_len, gbx_kmer_stats *d_stats, int64_t *d_hist, uint64_t *d_sel_kmer,
                          uint32_t *d_sel_count, int64_t sel_cap, void *d_work, size_t work_bytes, void *stream)
{
    int rc = kmer_params_check(p, "gbx_kmer_count_device");
    if (rc) return rc;
    if (n_reads < 0 || sel_cap < 0) { set_error("gbx_kmer_count_device: bad argument"); return GBX_ERR_ARG; }
    if (!d_stats || !d_work || (n_reads > 0 && (!d_enc || !d_read_off || !d_read_len)) || (p->n_hist > 0 && !d_hist) ||
        (sel_cap > 0 && (!d_sel_kmer || !d_sel_count))) {
        set_error("gbx_kmer_count_device: null pointer");
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return kmer_launch(p, n_reads, d_enc, d_read_off, d_read_len, d_stats, d_hist, d_sel_kmer, d_sel_count, sel_cap, d_work, work_bytes,
                       (hipStream_t)stream);
}

int gbx_kmer_count_host(const gbx_kmer_params *p, int64_t n_reads, const uint8_t *enc, int64_t enc_bytes, const int64_t *read_off,
                        const int32_t *read_len, gbx_kmer_stats *st, int64_t *hist, uint64_t *sel_kmer, uint32_t *sel_count,
                        int64_t sel_cap)
{
    RoctxRange range_("gbx_kmer_count_host");
    int rc = kmer_params_check(p, "gbx_kmer_count_host");
    if (rc) return rc;
    if (n_reads < 0 || enc_bytes < 0 || sel_cap < 0) { set_error("gbx_kmer_count_host: bad argument"); return GBX_ERR_ARG; }
    if (!st || (n_reads > 0 && (!enc || !read_off || !read_len)) || (p->n_hist > 0 && !hist) || (sel_cap > 0 && (!sel_kmer || !sel_count))) {
        set_error("gbx_kmer_count_host: null pointer");
        return GBX_ERR_ARG;
    }
    // every read is checked, and the positions counted, before the device is touched
    int64_t positions = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (read_len[r] < 0 || read_off[r] < 0 || read_off[r] > enc_bytes - read_len[r]) {
            set_error("gbx_kmer_count_host: read %lld (offset %lld, length %d) is not inside the %lld bytes of enc", (long long)r,
                      (long long)read_off[r], read_len[r], (long long)enc_bytes);
            return GBX_ERR_ARG;
        }
        positions += std::max<int64_t>(0, (int64_t)read_len[r] - p->k);
    }
    if (positions >= (1ll << 32)) {
        set_error("gbx_kmer_count_host: %lld k-mer positions; the 32-bit counters take fewer than 2^32", (long long)positions);
        return GBX_ERR_UNSUPPORTED;
    }
    if ((rc = require_device())) return rc;
    std::lock_guard<std::mutex> serial(kmer_host_mu);
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    DevBuf denc(L), doff(L), dlen(L), dst(L), dhist(L), dkm(L), dcnt(L), dw(L);
    const size_t wb = kmer_workspace_bytes(p->k, n_reads);
    const size_t nh = (size_t)p->n_hist;
    if ((rc = denc.alloc((size_t)enc_bytes)) || (rc = doff.alloc((size_t)n_reads * 8)) || (rc = dlen.alloc((size_t)n_reads * 4)) ||
        (rc = dst.alloc(sizeof(gbx_kmer_stats))) || (rc = dhist.alloc(nh * 8)) || (rc = dkm.alloc((size_t)sel_cap * 8)) ||
        (rc = dcnt.alloc((size_t)sel_cap * 4)) || (rc = dw.alloc(wb)))
        return rc;
    if (enc_bytes > 0) GBX_HIP(hipMemcpyAsync(denc.p, enc, (size_t)enc_bytes, hipMemcpyHostToDevice, s));
    if (n_reads > 0) {
        GBX_HIP(hipMemcpyAsync(doff.p, read_off, (size_t)n_reads * 8, hipMemcpyHostToDevice, s));
        GBX_HIP(hipMemcpyAsync(dlen.p, read_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
    }
    if ((rc = kmer_launch(p, n_reads, denc.as<uint8_t>(), doff.as<int64_t>(), dlen.as<int32_t>(), dst.as<gbx_kmer_stats>(),
                          dhist.as<int64_t>(), dkm.as<uint64_t>(), dcnt.as<uint32_t>(), sel_cap, dw.p, wb, s)))
        return rc;
    GBX_HIP(hipMemcpyAsync(st, dst.p, sizeof(gbx_kmer_stats), hipMemcpyDeviceToHost, s));
    if (nh > 0) GBX_HIP(hipMemcpyAsync(hist, dhist.p, nh * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    const int64_t got = std::min<int64_t>(st->n_selected, sel_cap);
    if (got > 0) {
        GBX_HIP(hipMemcpyAsync(sel_kmer, dkm.p, (size_t)got * 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(sel_count, dcnt.p, (size_t)got * 4, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipStreamSynchronize(s));
    }
    if (st->n_positions != positions) {
        set_error("gbx_kmer_count_host: the device counted %lld positions, the host %lld", (long long)st->n_positions, (long long)positions);
        return GBX_ERR_HIP;
    }
    if (st->n_selected > sel_cap) {
        set_error("gbx_kmer_count_host: %lld selected k-mers do not fit sel_cap = %lld", (long long)st->n_selected, (long long)sel_cap);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

}  // extern "C"
