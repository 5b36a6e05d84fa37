// capi_mm.hip — minimizer seeding entries of the C-ABI (include/gbx.h): sketch, index, seeds -> a chain batch.
#include "capi_common.h"

using namespace gbx;

namespace {

int params_check(const gbx_mm_params *p, const char *who)
{
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (p->k < 1 || p->k > 28) { set_error("%s: k = %d (1..28)", who, p->k); return GBX_ERR_ARG; }
    if (p->w < 1 || p->w > 255) { set_error("%s: w = %d (1..255)", who, p->w); return GBX_ERR_ARG; }
    if (p->mid_occ < 0) { set_error("%s: mid_occ = %d is negative", who, p->mid_occ); return GBX_ERR_ARG; }
    if (p->max_gap < 0 || p->bw < 0) { set_error("%s: max_gap = %d, bw = %d (neither may be negative)", who, p->max_gap, p->bw); return GBX_ERR_ARG; }
    if (!(p->mid_occ_frac == p->mid_occ_frac) || p->mid_occ_frac >= 1.f) {
        set_error("%s: mid_occ_frac = %g (a number below 1)", who, (double)p->mid_occ_frac);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

// the host checks of a batch of sequences; *max_len: the longest
int seqs_check(int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off, const char *what, int64_t *max_len, const char *who)
{
    if (n_seqs < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_seqs >= (1ll << 31)) { set_error("%s: %lld %ss (fewer than 2^31)", who, (long long)n_seqs, what); return GBX_ERR_UNSUPPORTED; }
    if (!seq_off) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (seq_off[0] != 0) { set_error("%s: seq_off[0] must be 0", who); return GBX_ERR_ARG; }
    *max_len = 0;
    for (int64_t s = 0; s < n_seqs; ++s) {
        const int64_t len = seq_off[s + 1] - seq_off[s];
        if (len < 0) { set_error("%s: seq_off is not monotone at %s %lld", who, what, (long long)s); return GBX_ERR_ARG; }
        if (len >= (1ll << 31)) { set_error("%s: %s %lld has %lld bases (fewer than 2^31)", who, what, (long long)s, (long long)len); return GBX_ERR_UNSUPPORTED; }
        if (len > *max_len) *max_len = len;
    }
    if (seq_off[n_seqs] > 0 && !seq) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    return GBX_OK;
}

}  // namespace

extern "C" {

void gbx_mm_default_params(gbx_mm_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->k = 15; p->w = 10; p->is_hpc = 0; p->mid_occ = 0; p->mid_occ_frac = 2e-4f; p->max_gap = 5000; p->bw = 500;
}

int gbx_mm_check_params(const gbx_mm_params *p) { return params_check(p, "gbx_mm_check_params"); }

size_t gbx_mm_sketch_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len)
{
    if (params_check(p, "gbx_mm_sketch_workspace_bytes") || n_seqs < 0 || total_len < 0) return 0;
    return mm_sketch_workspace_bytes(p, n_seqs, total_len);
}

int gbx_mm_sketch_device(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len,
                         int32_t rid_ordinal, uint64_t *d_mini_x, uint64_t *d_mini_y, int64_t mini_cap, int64_t *d_mini_off,
                         int64_t *d_n_mini, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mm_sketch_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n_seqs < 0 || total_len < 0 || mini_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_seqs >= (1ll << 31)) { set_error("%s: %lld sequences (fewer than 2^31)", who, (long long)n_seqs); return GBX_ERR_UNSUPPORTED; }
    if (!d_seq_off || !d_mini_off || !d_n_mini || !d_work || (total_len > 0 && !d_seq) || (mini_cap > 0 && (!d_mini_x || !d_mini_y))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return mm_sketch_launch(p, n_seqs, d_seq, d_seq_off, total_len, rid_ordinal != 0, d_mini_x, d_mini_y, mini_cap, d_mini_off, d_n_mini, d_work,
                            work_bytes, (hipStream_t)stream);
}

int gbx_mm_sketch_host(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off, int32_t rid_ordinal,
                       uint64_t *mini_x, uint64_t *mini_y, int64_t mini_cap, int64_t *mini_off, int64_t *n_mini)
{
    RoctxRange range_("gbx_mm_sketch_host");
    const char *who = "gbx_mm_sketch_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    int64_t max_len;
    if (!n_mini || !mini_off || mini_cap < 0 || (mini_cap > 0 && (!mini_x || !mini_y))) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = seqs_check(n_seqs, seq, seq_off, "sequence", &max_len, who))) return rc;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t st = L->compute;
    const int64_t total = seq_off[n_seqs], cap = std::min(mini_cap, total);
    const size_t wb = mm_sketch_workspace_bytes(p, n_seqs, total);
    DevBuf dseq(L), doff(L), dx(L), dy(L), dmo(L), dn(L), dw(L);
    if ((rc = upload(dseq, seq, (size_t)total, st)) || (rc = upload(doff, seq_off, (size_t)(n_seqs + 1) * 8, st)) || (rc = dx.alloc((size_t)cap * 8)) ||
        (rc = dy.alloc((size_t)cap * 8)) || (rc = dmo.alloc((size_t)(n_seqs + 1) * 8)) || (rc = dn.alloc(8)) || (rc = dw.alloc(wb)))
        return rc;
    if ((rc = mm_sketch_launch(p, n_seqs, dseq.as<uint8_t>(), doff.as<int64_t>(), total, rid_ordinal != 0, dx.as<uint64_t>(), dy.as<uint64_t>(), cap,
                               dmo.as<int64_t>(), dn.as<int64_t>(), dw.p, wb, st)))
        return rc;
    int64_t got = -1;
    GBX_HIP(hipMemcpyAsync(&got, dn.p, 8, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipMemcpyAsync(mini_off, dmo.p, (size_t)(n_seqs + 1) * 8, hipMemcpyDeviceToHost, st));
    GBX_HIP(hipStreamSynchronize(st));
    *n_mini = got;
    if (got < 0 || got > total) { set_error("%s: the device counted %lld minimizers in %lld bases", who, (long long)got, (long long)total); return GBX_ERR_HIP; }
    if (got > mini_cap) { set_error("%s: %lld minimizers do not fit mini_cap = %lld", who, (long long)got, (long long)mini_cap); return GBX_ERR_ARG; }
    if (got) {
        GBX_HIP(hipMemcpyAsync(mini_x, dx.p, (size_t)got * 8, hipMemcpyDeviceToHost, st));
        GBX_HIP(hipMemcpyAsync(mini_y, dy.p, (size_t)got * 8, hipMemcpyDeviceToHost, st));
        GBX_HIP(hipStreamSynchronize(st));
    }
    return GBX_OK;
}

size_t gbx_mm_index_bytes(int64_t mini_cap) { return mini_cap < 0 ? 0 : mm_index_bytes(mini_cap); }

size_t gbx_mm_index_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len, int64_t mini_cap)
{
    if (params_check(p, "gbx_mm_index_workspace_bytes") || n_seqs < 0 || total_len < 0 || mini_cap < 0) return 0;
    return mm_index_workspace_bytes(p, n_seqs, total_len, mini_cap);
}

int gbx_mm_index_build_device(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len,
                              void *d_index, int64_t mini_cap, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mm_index_build_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n_seqs < 0 || total_len < 0 || mini_cap < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (n_seqs >= (1ll << 31)) { set_error("%s: %lld sequences (fewer than 2^31)", who, (long long)n_seqs); return GBX_ERR_UNSUPPORTED; }
    if (!d_seq_off || !d_index || !d_work || (total_len > 0 && !d_seq)) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    return mm_index_launch(p, n_seqs, d_seq, d_seq_off, total_len, d_index, mini_cap, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mm_index_stats(const void *d_index, int64_t mini_cap, gbx_mm_index_info *st, void *stream)
{
    const char *who = "gbx_mm_index_stats";
    if (!d_index || !st || mini_cap < 0) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc = require_device();
    if (rc) return rc;
    int64_t h[6] = {-1, -1, -1, -1, -1, -1};
    GBX_HIP(hipMemcpyAsync(h, d_index, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GBX_HIP(hipStreamSynchronize((hipStream_t)stream));
    st->n_vals = h[0]; st->n_keys = h[1]; st->mid_occ = (int32_t)h[2]; st->k = (int32_t)h[3]; st->w = (int32_t)h[4]; st->is_hpc = (int32_t)h[5];
    if (h[0] > mini_cap) { set_error("%s: %lld minimizers do not fit mini_cap = %lld", who, (long long)h[0], (long long)mini_cap); return GBX_ERR_ARG; }
    if (h[0] < 0 || h[1] < 0 || h[1] > h[0]) {
        set_error("%s: the device counted %lld keys of %lld minimizers", who, (long long)h[1], (long long)h[0]);
        return GBX_ERR_HIP;
    }
    return GBX_OK;
}

int gbx_mm_index_build_host(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off,
                            uint64_t *keys, int64_t *key_off, int64_t key_cap, uint64_t *vals, int64_t val_cap, gbx_mm_index_info *st)
{
    RoctxRange range_("gbx_mm_index_build_host");
    const char *who = "gbx_mm_index_build_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    int64_t max_len;
    if (!st || key_cap < 0 || val_cap < 0 || (key_cap > 0 && (!keys || !key_off)) || (val_cap > 0 && !vals)) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = seqs_check(n_seqs, seq, seq_off, "sequence", &max_len, who))) return rc;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    const int64_t total = seq_off[n_seqs], cap = total;            // a base ends one minimizer at most
    const size_t wb = mm_index_workspace_bytes(p, n_seqs, total, cap);
    DevBuf dseq(L), doff(L), di(L), dw(L);
    if ((rc = upload(dseq, seq, (size_t)total, s)) || (rc = upload(doff, seq_off, (size_t)(n_seqs + 1) * 8, s)) ||
        (rc = di.alloc(mm_index_bytes(cap))) || (rc = dw.alloc(wb)))
        return rc;
    if ((rc = mm_index_launch(p, n_seqs, dseq.as<uint8_t>(), doff.as<int64_t>(), total, di.p, cap, dw.p, wb, s))) return rc;
    if ((rc = gbx_mm_index_stats(di.p, cap, st, s))) return rc;
    if (st->n_keys > key_cap || st->n_vals > val_cap) {
        set_error("%s: %lld keys and %lld minimizers do not fit key_cap = %lld, val_cap = %lld", who, (long long)st->n_keys, (long long)st->n_vals,
                  (long long)key_cap, (long long)val_cap);
        return GBX_ERR_ARG;
    }
    const MmIndexView v = mm_index_view(di.p, cap);
    if (st->n_keys) GBX_HIP(hipMemcpyAsync(keys, v.keys, (size_t)st->n_keys * 8, hipMemcpyDeviceToHost, s));
    if (key_off) GBX_HIP(hipMemcpyAsync(key_off, v.koff, (size_t)(st->n_keys + 1) * 8, hipMemcpyDeviceToHost, s));
    if (st->n_vals) GBX_HIP(hipMemcpyAsync(vals, v.vals, (size_t)st->n_vals * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

size_t gbx_mm_seed_workspace_bytes(const gbx_mm_params *p, int64_t n_reads, int64_t total_len, int64_t mini_cap, int64_t anchor_cap)
{
    if (params_check(p, "gbx_mm_seed_workspace_bytes") || n_reads < 0 || total_len < 0 || mini_cap < 0 || anchor_cap < 0) return 0;
    return mm_seed_workspace_bytes(p, n_reads, total_len, mini_cap, anchor_cap);
}

int gbx_mm_seed_device(const gbx_mm_params *p, const void *d_index, int64_t index_mini_cap, int64_t ref_n_seqs, int64_t ref_max_len,
                       int64_t n_reads, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len,
                       uint64_t *d_mini_x, uint64_t *d_mini_y, int64_t mini_cap, int64_t *d_mini_off,
                       uint64_t *d_ax, uint64_t *d_ay, int64_t anchor_cap, int64_t *d_off, gbx_chain_call *d_hdr,
                       int32_t *d_rep_len, int32_t *d_n_mini, int64_t *d_counts, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_mm_seed_device";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n_reads < 0 || total_len < 0 || mini_cap < 0 || anchor_cap < 0 || index_mini_cap < 0 || ref_n_seqs < 0 || ref_max_len < 0) {
        set_error("%s: bad argument", who);
        return GBX_ERR_ARG;
    }
    if (n_reads > GBX_MM_MAX_READS) { set_error("%s: %lld reads (at most %d a call)", who, (long long)n_reads, GBX_MM_MAX_READS); return GBX_ERR_UNSUPPORTED; }
    if (ref_n_seqs >= (1ll << 31) || ref_max_len >= (1ll << 31)) { set_error("%s: the reference's sizes leave 31 bits", who); return GBX_ERR_UNSUPPORTED; }
    if (!d_index || !d_seq_off || !d_mini_off || !d_off || !d_counts || !d_work || (total_len > 0 && !d_seq) ||
        (mini_cap > 0 && (!d_mini_x || !d_mini_y)) || (anchor_cap > 0 && (!d_ax || !d_ay)) || (n_reads > 0 && (!d_hdr || !d_rep_len || !d_n_mini))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    const MmSeedIo io{d_index, index_mini_cap, ref_n_seqs, ref_max_len, n_reads, d_seq, d_seq_off, total_len, d_mini_x, d_mini_y, mini_cap, d_mini_off,
                      d_ax, d_ay, anchor_cap, d_off, d_hdr, d_rep_len, d_n_mini, d_counts};
    return mm_seed_launch(p, io, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_mm_seed_host(const gbx_mm_params *p, const uint64_t *keys, const int64_t *key_off, int64_t n_keys, const uint64_t *vals,
                     int32_t mid_occ, int64_t ref_n_seqs, int64_t ref_max_len,
                     int64_t n_reads, const uint8_t *seq, const int64_t *seq_off,
                     uint64_t *mini_x, uint64_t *mini_y, int64_t mini_cap, int64_t *mini_off,
                     uint64_t *ax, uint64_t *ay, int64_t anchor_cap, int64_t *off, gbx_chain_call *hdr,
                     int32_t *rep_len, int32_t *n_mini, int64_t *counts)
{
    RoctxRange range_("gbx_mm_seed_host");
    const char *who = "gbx_mm_seed_host";
    int rc = params_check(p, who);
    if (rc) return rc;
    if (n_keys < 0 || mini_cap < 0 || anchor_cap < 0 || ref_n_seqs < 0 || ref_max_len < 0 || mid_occ < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (!key_off || !off || !counts || (n_keys > 0 && !keys) || (mini_cap > 0 && (!mini_x || !mini_y || !mini_off)) || (anchor_cap > 0 && (!ax || !ay)) ||
        (n_reads > 0 && (!hdr || !rep_len || !n_mini))) {
        set_error("%s: null pointer", who);
        return GBX_ERR_ARG;
    }
    int64_t max_len;
    if ((rc = seqs_check(n_reads, seq, seq_off, "read", &max_len, who))) return rc;
    if (n_reads > GBX_MM_MAX_READS) { set_error("%s: %lld reads (at most %d a call)", who, (long long)n_reads, GBX_MM_MAX_READS); return GBX_ERR_UNSUPPORTED; }
    if (ref_n_seqs >= (1ll << 31) || ref_max_len >= (1ll << 31)) { set_error("%s: the reference's sizes leave 31 bits", who); return GBX_ERR_UNSUPPORTED; }
    if (key_off[0] != 0) { set_error("%s: key_off[0] must be 0", who); return GBX_ERR_ARG; }
    for (int64_t j = 0; j < n_keys; ++j)
        if (key_off[j + 1] < key_off[j]) { set_error("%s: key_off is not monotone at key %lld", who, (long long)j); return GBX_ERR_ARG; }
    const int64_t n_vals = key_off[n_keys];
    if (n_vals > 0 && !vals) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    counts[0] = counts[1] = 0;
    off[0] = 0;
    if (n_reads == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    const int64_t total = seq_off[n_reads], mcap = total, icap = std::max<int64_t>(n_vals, 1);
    const size_t wb = mm_seed_workspace_bytes(p, n_reads, total, mcap, anchor_cap);
    DevBuf di(L), dseq(L), dso(L), dmx(L), dmy(L), dmo(L), dax(L), day(L), doff(L), dh(L), drl(L), dnm(L), dc(L), dw(L);
    if ((rc = di.alloc(mm_index_bytes(icap)))) return rc;
    const MmIndexView v = mm_index_view(di.p, icap);
    const int64_t h[6] = {n_vals, n_keys, mid_occ, p->k, p->w, p->is_hpc};
    GBX_HIP(hipMemcpyAsync(v.hdr, h, sizeof(h), hipMemcpyHostToDevice, s));
    if (n_keys) GBX_HIP(hipMemcpyAsync(v.keys, keys, (size_t)n_keys * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(v.koff, key_off, (size_t)(n_keys + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_vals) GBX_HIP(hipMemcpyAsync(v.vals, vals, (size_t)n_vals * 8, hipMemcpyHostToDevice, s));
    if ((rc = upload(dseq, seq, (size_t)total, s)) || (rc = upload(dso, seq_off, (size_t)(n_reads + 1) * 8, s)) || (rc = dmx.alloc((size_t)mcap * 8)) ||
        (rc = dmy.alloc((size_t)mcap * 8)) || (rc = dmo.alloc((size_t)(n_reads + 1) * 8)) || (rc = dax.alloc((size_t)anchor_cap * 8)) ||
        (rc = day.alloc((size_t)anchor_cap * 8)) || (rc = doff.alloc((size_t)(n_reads + 1) * 8)) || (rc = dh.alloc((size_t)n_reads * sizeof(gbx_chain_call))) ||
        (rc = drl.alloc((size_t)n_reads * 4)) || (rc = dnm.alloc((size_t)n_reads * 4)) || (rc = dc.alloc(16)) || (rc = dw.alloc(wb)))
        return rc;
    const MmSeedIo io{di.p, icap, ref_n_seqs, ref_max_len, n_reads, dseq.as<uint8_t>(), dso.as<int64_t>(), total, dmx.as<uint64_t>(), dmy.as<uint64_t>(),
                      mcap, dmo.as<int64_t>(), dax.as<uint64_t>(), day.as<uint64_t>(), anchor_cap, doff.as<int64_t>(), dh.as<gbx_chain_call>(),
                      drl.as<int32_t>(), dnm.as<int32_t>(), dc.as<int64_t>()};
    if ((rc = mm_seed_launch(p, io, dw.p, wb, s))) return rc;
    GBX_HIP(hipMemcpyAsync(counts, dc.p, 16, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(off, doff.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(hdr, dh.p, (size_t)n_reads * sizeof(gbx_chain_call), hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(rep_len, drl.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(n_mini, dnm.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
    if (mini_off) GBX_HIP(hipMemcpyAsync(mini_off, dmo.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (counts[0] < 0 || counts[0] > total || counts[1] < 0) {
        set_error("%s: the device counted %lld minimizers and %lld anchors in %lld bases", who, (long long)counts[0], (long long)counts[1], (long long)total);
        return GBX_ERR_HIP;
    }
    if ((mini_x && counts[0] > mini_cap) || counts[1] > anchor_cap) {
        set_error("%s: %lld minimizers and %lld anchors do not fit mini_cap = %lld, anchor_cap = %lld", who, (long long)counts[0], (long long)counts[1],
                  (long long)mini_cap, (long long)anchor_cap);
        return GBX_ERR_ARG;
    }
    if (mini_x && counts[0]) {
        GBX_HIP(hipMemcpyAsync(mini_x, dmx.p, (size_t)counts[0] * 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(mini_y, dmy.p, (size_t)counts[0] * 8, hipMemcpyDeviceToHost, s));
    }
    if (counts[1]) {
        GBX_HIP(hipMemcpyAsync(ax, dax.p, (size_t)counts[1] * 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(ay, day.p, (size_t)counts[1] * 8, hipMemcpyDeviceToHost, s));
    }
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

}  // extern "C"
