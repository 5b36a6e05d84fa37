// capi_kmer_index.hip — the minimizer index entries of the C-ABI (include/gbx.h, kmer index section).
#include "capi_common.h"
#include "kmer_index_rules.h"

using namespace gbx;

static_assert(GBX_KMER_INDEX_MAX_K == KI_MAX_K && GBX_KMER_INDEX_MAX_WINDOW == KI_MAX_WINDOW, "gbx.h and kmer_index_rules.h disagree");

namespace {
int ki_params_check(const gbx_kmer_index_params *p, const char *who)
{
    if (!p) { set_error("%s: null params", who); return GBX_ERR_ARG; }
    if (p->k < 1 || p->k > KI_MAX_K) {
        set_error("%s: k = %d outside 1..%d (the reference's k-mer mask, 1 << 2k, is undefined at 32: R/kmer.h:71)", who, p->k, KI_MAX_K);
        return GBX_ERR_ARG;
    }
    if (p->window < 1 || p->window > KI_MAX_WINDOW) {
        set_error("%s: window = %d outside 1..%d (the tile's halo of hashes)", who, p->window, KI_MAX_WINDOW);
        return GBX_ERR_ARG;
    }
    if (!(p->repeat_rate >= 0.f && p->repeat_rate <= KI_MAX_RATE)) {
        set_error("%s: repeat_rate = %g outside 0..%g", who, (double)p->repeat_rate, (double)KI_MAX_RATE);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int ki_total_check(int64_t total_len, const char *who)
{
    if (total_len < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (2 * (unsigned long long)total_len >= (unsigned long long)KI_MAX_GLOBAL) {
        set_error("%s: %lld bases; global positions run to 2 * bases and must stay below 2^40 (the reference's 5-byte IndexChunk)", who,
                  (long long)total_len);
        return GBX_ERR_UNSUPPORTED;
    }
    return GBX_OK;
}

// every read inside enc, before the device is touched; *total_len: the sum of the lengths
int ki_reads_check(int64_t n_reads, int64_t enc_bytes, const int64_t *read_off, const int32_t *read_len, int64_t *total_len, const char *who)
{
    int64_t total = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (read_len[r] < 0 || read_off[r] < 0 || read_off[r] > enc_bytes - read_len[r]) {
            set_error("%s: read %lld (offset %lld, length %d) is not inside the %lld bytes of enc", who, (long long)r, (long long)read_off[r],
                      read_len[r], (long long)enc_bytes);
            return GBX_ERR_ARG;
        }
        total += read_len[r];
    }
    *total_len = total;
    return ki_total_check(total, who);
}

// one host call at a time: a call's workspace is 48 bytes a base
std::mutex ki_host_mu;

struct HostReads {
    DevBuf enc, off, len;
    explicit HostReads(Lane *L) : enc(L), off(L), len(L) {}
    int put(int64_t n_reads, const uint8_t *h_enc, int64_t enc_bytes, const int64_t *h_off, const int32_t *h_len, hipStream_t s)
    {
        int rc;
        if ((rc = enc.alloc((size_t)enc_bytes)) || (rc = off.alloc((size_t)n_reads * 8)) || (rc = len.alloc((size_t)n_reads * 4))) return rc;
        if (enc_bytes > 0) GBX_HIP(hipMemcpyAsync(enc.p, h_enc, (size_t)enc_bytes, hipMemcpyHostToDevice, s));
        if (n_reads > 0) {
            GBX_HIP(hipMemcpyAsync(off.p, h_off, (size_t)n_reads * 8, hipMemcpyHostToDevice, s));
            GBX_HIP(hipMemcpyAsync(len.p, h_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
        }
        return GBX_OK;
    }
};
}  // namespace

extern "C" {

size_t gbx_kmer_index_workspace_bytes(int32_t k, int64_t n_reads, int64_t total_len, int32_t index)
{
    if (k < 1 || k > KI_MAX_K || n_reads < 0 || total_len < 0 || 2 * (unsigned long long)total_len >= (unsigned long long)KI_MAX_GLOBAL) return 0;
    return kmer_index_workspace_bytes(n_reads, total_len, index != 0);
}

int gbx_kmer_minimizers_device(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *d_enc, const int64_t *d_read_off,
                               const int32_t *d_read_len, int64_t total_len, int64_t *d_mini_off, int32_t *d_mini_pos, uint8_t *d_mini_rev,
                               int64_t mini_cap, int64_t *d_n_mini, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_kmer_minimizers_device";
    int rc = ki_params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || mini_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if ((rc = ki_total_check(total_len, who))) return rc;
    if (!d_mini_off || !d_n_mini || !d_work || (n_reads > 0 && (!d_enc || !d_read_off || !d_read_len)) || (mini_cap > 0 && (!d_mini_pos || !d_mini_rev))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return kmer_minimizers_launch(p, KmerIndexReads{d_enc, d_read_off, d_read_len, n_reads, total_len}, d_mini_off, d_mini_pos, d_mini_rev, mini_cap,
                                  d_n_mini, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_kmer_index_device(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *d_enc, const int64_t *d_read_off,
                          const int32_t *d_read_len, int64_t total_len, gbx_kmer_index_stats *d_stats, uint64_t *d_kmer, int64_t *d_off,
                          int64_t kmer_cap, uint64_t *d_pos, int64_t pos_cap, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_kmer_index_device";
    int rc = ki_params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || kmer_cap < 0 || pos_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if ((rc = ki_total_check(total_len, who))) return rc;
    if (!d_stats || !d_off || !d_work || (n_reads > 0 && (!d_enc || !d_read_off || !d_read_len)) || (kmer_cap > 0 && !d_kmer) || (pos_cap > 0 && !d_pos)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return kmer_index_launch(p, KmerIndexReads{d_enc, d_read_off, d_read_len, n_reads, total_len}, d_stats, d_kmer, d_off, kmer_cap, d_pos, pos_cap,
                             d_work, work_bytes, (hipStream_t)stream);
}

int gbx_kmer_minimizers_host(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *enc, int64_t enc_bytes, const int64_t *read_off,
                             const int32_t *read_len, int64_t *mini_off, int32_t *mini_pos, uint8_t *mini_rev, int64_t mini_cap, int64_t *n_mini)
{
    const char *who = "gbx_kmer_minimizers_host";
    RoctxRange range_(who);
    int rc = ki_params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || enc_bytes < 0 || mini_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!mini_off || !n_mini || (n_reads > 0 && (!enc || !read_off || !read_len)) || (mini_cap > 0 && (!mini_pos || !mini_rev))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int64_t total_len = 0;
    if ((rc = ki_reads_check(n_reads, enc_bytes, read_off, read_len, &total_len, who))) return rc;
    if ((rc = require_device())) return rc;
    std::lock_guard<std::mutex> serial(ki_host_mu);
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    HostReads rd(L);
    DevBuf doff(L), dpos(L), drev(L), dn(L), dw(L);
    const size_t wb = kmer_index_workspace_bytes(n_reads, total_len, false);
    if ((rc = rd.put(n_reads, enc, enc_bytes, read_off, read_len, s)) || (rc = doff.alloc((size_t)(n_reads + 1) * 8)) ||
        (rc = dpos.alloc((size_t)mini_cap * 4)) || (rc = drev.alloc((size_t)mini_cap)) || (rc = dn.alloc(8)) || (rc = dw.alloc(wb)))
        return rc;
    if ((rc = kmer_minimizers_launch(p, KmerIndexReads{rd.enc.as<uint8_t>(), rd.off.as<int64_t>(), rd.len.as<int32_t>(), n_reads, total_len},
                                     doff.as<int64_t>(), dpos.as<int32_t>(), drev.as<uint8_t>(), mini_cap, dn.as<int64_t>(), dw.p, wb, s)))
        return rc;
    GBX_HIP(hipMemcpyAsync(n_mini, dn.p, 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(mini_off, doff.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (*n_mini < 0) { set_error("%s: the device found another sum of the read lengths than the host's %lld", who, (long long)total_len); return GBX_ERR_HIP; }
    const int64_t got = std::min<int64_t>(*n_mini, mini_cap);
    if (got > 0) {
        GBX_HIP(hipMemcpyAsync(mini_pos, dpos.p, (size_t)got * 4, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(mini_rev, drev.p, (size_t)got, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipStreamSynchronize(s));
    }
    if (*n_mini > mini_cap) {
        set_error("%s: %lld minimizers do not fit mini_cap = %lld", who, (long long)*n_mini, (long long)mini_cap);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int gbx_kmer_index_host(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *enc, int64_t enc_bytes, const int64_t *read_off,
                        const int32_t *read_len, gbx_kmer_index_stats *st, uint64_t *kmer, int64_t *off, int64_t kmer_cap, uint64_t *pos,
                        int64_t pos_cap)
{
    const char *who = "gbx_kmer_index_host";
    RoctxRange range_(who);
    int rc = ki_params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || enc_bytes < 0 || kmer_cap < 0 || pos_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!st || !off || (n_reads > 0 && (!enc || !read_off || !read_len)) || (kmer_cap > 0 && !kmer) || (pos_cap > 0 && !pos)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int64_t total_len = 0;
    if ((rc = ki_reads_check(n_reads, enc_bytes, read_off, read_len, &total_len, who))) return rc;
    if ((rc = require_device())) return rc;
    std::lock_guard<std::mutex> serial(ki_host_mu);
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    HostReads rd(L);
    DevBuf dst(L), dkm(L), doff(L), dpos(L), dw(L);
    const size_t wb = kmer_index_workspace_bytes(n_reads, total_len, true);
    if ((rc = rd.put(n_reads, enc, enc_bytes, read_off, read_len, s)) || (rc = dst.alloc(sizeof(gbx_kmer_index_stats))) ||
        (rc = dkm.alloc((size_t)kmer_cap * 8)) || (rc = doff.alloc((size_t)(kmer_cap + 1) * 8)) || (rc = dpos.alloc((size_t)pos_cap * 8)) ||
        (rc = dw.alloc(wb)))
        return rc;
    if ((rc = kmer_index_launch(p, KmerIndexReads{rd.enc.as<uint8_t>(), rd.off.as<int64_t>(), rd.len.as<int32_t>(), n_reads, total_len},
                                dst.as<gbx_kmer_index_stats>(), dkm.as<uint64_t>(), doff.as<int64_t>(), kmer_cap, dpos.as<uint64_t>(), pos_cap, dw.p,
                                wb, s)))
        return rc;
    GBX_HIP(hipMemcpyAsync(st, dst.p, sizeof(gbx_kmer_index_stats), hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (st->total_len != total_len) {
        set_error("%s: the device summed the read lengths to %lld, the host to %lld", who, (long long)st->total_len, (long long)total_len);
        return GBX_ERR_HIP;
    }
    const int64_t nk = std::min<int64_t>(st->n_selected, kmer_cap), np = std::min<int64_t>(st->n_entries, pos_cap);
    if (nk > 0) GBX_HIP(hipMemcpyAsync(kmer, dkm.p, (size_t)nk * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(off, doff.p, (size_t)(nk + 1) * 8, hipMemcpyDeviceToHost, s));
    if (np > 0) GBX_HIP(hipMemcpyAsync(pos, dpos.p, (size_t)np * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (st->n_selected > kmer_cap || st->n_entries > pos_cap) {
        set_error("%s: %lld k-mers with %lld positions do not fit kmer_cap = %lld, pos_cap = %lld", who, (long long)st->n_selected,
                  (long long)st->n_entries, (long long)kmer_cap, (long long)pos_cap);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

}  // extern "C"
