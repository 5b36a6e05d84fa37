// dbg_host.h — what the dbg entries (capi_dbg.hip) and the assembly entries behind them (capi_dbg_asm.hip) share on the host:
// the argument checks, the device entries' read-back of the offsets and ranges, the host entries' upload of reads and
// windows, the kernels' inputs and the error word.  The planning rules and the workspace layouts are in dbg_plan.h.
#pragma once
#include "capi_common.h"

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

// ---- the checks: the structs (nothing else is dereferenced), ...
inline int dbg_structs_check(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, const char *who)
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
    return GBX_OK;
}

// ... the offsets and ranges, as host arrays (the caller's own, or what a device entry read back), ...
inline int dbg_arrays_check(const gbx_dbg_reads *R, const gbx_dbg_wins *W, const int64_t *seq_off, const int64_t *ref_off, const int64_t *ref_pos,
                            const int64_t *read_lo, const int64_t *read_hi, const char *who)
{
    const int64_t n = R->n_reads, nw = W->n_win;
    if (seq_off[0] < 0 || seq_off[n] > R->seq_bytes) { set_error("%s: seq_off outside [0, seq_bytes]", who); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n; ++r)
        if (seq_off[r + 1] < seq_off[r]) { set_error("%s: seq_off decreases at read %lld", who, (long long)r); return GBX_ERR_ARG; }
    if (ref_off[0] < 0 || ref_off[nw] > W->ref_bytes) { set_error("%s: ref_off outside [0, ref_bytes]", who); return GBX_ERR_ARG; }
    for (int64_t w = 0; w < nw; ++w) {
        const char *bad = nullptr;
        if (ref_off[w + 1] < ref_off[w]) bad = "ref_off decreases";
        else if (ref_pos[w] < 0 || ref_pos[w] + (ref_off[w + 1] - ref_off[w]) > INT32_MAX) bad = "its reference lies outside [0, 2^31)";
        else if (read_lo[w] < 0 || read_lo[w] > read_hi[w] || read_hi[w] > n) bad = "its reads are not 0 <= read_lo <= read_hi <= n_reads";
        if (bad) { set_error("%s: window %lld: %s", who, (long long)w, bad); return GBX_ERR_ARG; }
    }
    return GBX_OK;
}
// ... and the kernels' one address space of reference and read bytes.
inline int dbg_total_check(const gbx_dbg_reads *R, const gbx_dbg_wins *W, const char *who)
{
    if (W->ref_bytes + R->seq_bytes >= ((int64_t)1 << 40)) { set_error("%s: more than 2^40 bytes of reference and reads", who); return GBX_ERR_UNSUPPORTED; }
    return GBX_OK;
}
// a host entry's reads and windows: all three
inline int dbg_check(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, const char *who)
{
    int rc = dbg_structs_check(p, R, W, who);
    if (rc || (rc = dbg_arrays_check(R, W, R->seq_off, W->ref_off, W->ref_pos, W->read_lo, W->read_hi, who))) return rc;
    return dbg_total_check(R, W, who);
}

// ---- A device entry's offsets and ranges read back into H on s (synchronised) and checked as the host entries check the caller's.
inline int dbg_read_back(const gbx_dbg_reads *R, const gbx_dbg_wins *W, hipStream_t s, const char *who, DbgHostArrays &H)
{
    auto down = [s](std::vector<int64_t> &v, const int64_t *d, int64_t n) {
        v.resize((size_t)n);
        return n ? hipMemcpyAsync(v.data(), d, (size_t)n * 8, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    GBX_HIP(down(H.seq_off, R->seq_off, R->n_reads + 1));
    GBX_HIP(down(H.ref_off, W->ref_off, W->n_win + 1));
    GBX_HIP(down(H.ref_pos, W->ref_pos, W->n_win));
    GBX_HIP(down(H.read_lo, W->read_lo, W->n_win));
    GBX_HIP(down(H.read_hi, W->read_hi, W->n_win));
    GBX_HIP(hipStreamSynchronize(s));
    return dbg_arrays_check(R, W, H.seq_off.data(), H.ref_off.data(), H.ref_pos.data(), H.read_lo.data(), H.read_hi.data(), who);
}

// ---- A host entry's reads [ra, rb) and windows [lo, hi) on the lane's device, rebased to the first read, window and byte
// of the range (an empty window's reads become [0, 0)).  R / W carry device pointers for what the kernels read - the bytes,
// seq_off and flag; the windows' offsets and ranges the runs take from h, so those stay null in W.  The queued copies read
// h: declare a StreamDrain behind this.
struct DbgUpload {
    DevBuf ref, seq, qual, soff, flag;
    DbgHostArrays h;
    gbx_dbg_reads R;
    gbx_dbg_wins W;                                // n_win, ref_bytes and ref only
    explicit DbgUpload(Lane *L) : ref(L), seq(L), qual(L), soff(L), flag(L), R(), W() {}
    int up(const gbx_dbg_reads *R0, const gbx_dbg_wins *W0, int64_t ra, int64_t rb, int64_t lo, int64_t hi, hipStream_t s)
    {
        const int64_t nr = rb - ra, m = hi - lo, b0 = R0->seq_off[ra], b1 = R0->seq_off[rb], f0 = W0->ref_off[lo], f1 = W0->ref_off[hi];
        h.seq_off.resize((size_t)nr + 1); h.ref_off.resize((size_t)m + 1); h.read_lo.resize((size_t)m); h.read_hi.resize((size_t)m);
        h.ref_pos.assign(W0->ref_pos + lo, W0->ref_pos + hi);
        for (int64_t j = 0; j <= nr; ++j) h.seq_off[(size_t)j] = R0->seq_off[ra + j] - b0;
        for (int64_t j = 0; j <= m; ++j) h.ref_off[(size_t)j] = W0->ref_off[lo + j] - f0;
        for (int64_t j = 0; j < m; ++j) {
            const bool any = W0->read_lo[lo + j] < W0->read_hi[lo + j];
            h.read_lo[(size_t)j] = any ? W0->read_lo[lo + j] - ra : 0; h.read_hi[(size_t)j] = any ? W0->read_hi[lo + j] - ra : 0;
        }
        int rc;                                      // + 128 / + 8: the kernels read past the last base and the last flag
        if ((rc = ref.alloc((size_t)(f1 - f0) + 128)) || (rc = seq.alloc((size_t)(b1 - b0) + 128)) || (rc = qual.alloc((size_t)(b1 - b0) + 128)) ||
            (rc = flag.alloc((size_t)nr * 2 + 8)) || (rc = upload(soff, h.seq_off.data(), (size_t)(nr + 1) * 8, s)))
            return rc;
        auto up1 = [s](DevBuf &b, const void *src, int64_t bytes) { return bytes ? hipMemcpyAsync(b.p, src, (size_t)bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
        GBX_HIP(up1(ref, W0->ref + f0, f1 - f0));
        GBX_HIP(up1(seq, R0->seq + b0, b1 - b0));
        GBX_HIP(up1(qual, R0->qual + b0, b1 - b0));
        GBX_HIP(up1(flag, R0->flag + ra, nr * 2));
        R.n_reads = nr; R.seq_bytes = b1 - b0; R.seq_off = soff.as<int64_t>(); R.seq = seq.as<uint8_t>(); R.qual = qual.as<uint8_t>(); R.flag = flag.as<uint16_t>();
        W.n_win = m; W.ref_bytes = f1 - f0; W.ref = ref.as<uint8_t>();
        return GBX_OK;
    }
};

// the kernels' inputs at k: R / W with device pointers, d_rcp the reads' slot prefix at k on the device
inline DbgDev dbg_dev(int k, const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, const int64_t *d_rcp)
{
    return DbgDev{k, p->min_qual, W->ref_bytes, W->ref, R->seq, R->qual, R->seq_off, d_rcp, R->flag};
}

// the error word of dbg_launch behind the launches and copies queued so far (synchronises s)
inline int dbg_err_check(const int *d_err, hipStream_t s, const char *who)
{
    int err = 0;
    GBX_HIP(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (err) { set_error("%s: a window's table filled (%d): cannot happen by its sizing", who, err); return GBX_ERR_HIP; }
    return GBX_OK;
}

}  // namespace gbx
