// capi_pileup.hip — medaka pileup feature-count entries of the C-ABI (include/gbx.h, pileup section).
#include "capi_common.h"

using namespace gbx;

namespace {

// Device memory of a host entry's slice: per position about 40 bytes (pos_col, the layout's marks, the scan), per column
// 8 + 4 F bytes (major, minor, the counters), and the slice's reads.  So a slice is bounded by positions and, for the count,
// by columns: at most PLP_SLICE_POSITIONS positions (about 170 MB) and, by default, PLP_SLICE_CELLS counters (256 MB) of
// columns - except one position whose 1 + max_ins columns alone exceed that, which is a slice of its own.
constexpr int64_t PLP_SLICE_CELLS = 64ll << 20;
constexpr int64_t PLP_SLICE_POSITIONS = 1ll << 22;

int plp_params_check(const gbx_pileup_params *p, const char *who)
{
    if (!p) { set_error("%s: null params", who); return GBX_ERR_ARG; }
    if (p->weibull) { set_error("%s: Weibull summation is not built (the benchmark's driver never asks for it)", who); return GBX_ERR_UNSUPPORTED; }
    if (p->num_dtypes < 1 || p->num_dtypes > GBX_PILEUP_MAX_DTYPES || p->num_homop < 1 || p->num_homop > GBX_PILEUP_MAX_HOMOP ||
        GBX_PILEUP_FEATLEN * p->num_dtypes * p->num_homop > GBX_PILEUP_MAX_F) {
        set_error("%s: num_dtypes = %d, num_homop = %d: 1..%d each and 10 * num_dtypes * num_homop <= %d", who, p->num_dtypes, p->num_homop,
                  GBX_PILEUP_MAX_DTYPES, GBX_PILEUP_MAX_F);
        return GBX_ERR_ARG;
    }
    if (p->start < 0 || p->end < p->start || p->end > INT32_MAX || p->slice_positions < 0) {
        set_error("%s: region [%lld, %lld) (0 <= start <= end < 2^31), slice_positions %lld", who, (long long)p->start, (long long)p->end,
                  (long long)p->slice_positions);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int plp_feat(const gbx_pileup_params *p) { return GBX_PILEUP_FEATLEN * p->num_dtypes * p->num_homop; }

int64_t plp_slice_positions(const gbx_pileup_params *p)
{
    return p->slice_positions > 0 ? p->slice_positions : PLP_SLICE_POSITIONS;
}

// The layout's slices: [cuts[k], cuts[k+1]) of at most sp positions each
std::vector<int64_t> plp_position_cuts(int64_t S, int64_t E, int64_t sp)
{
    std::vector<int64_t> cuts{S};
    for (int64_t q = S; q < E;) { q = std::min(E, q + sp); cuts.push_back(q); }
    return cuts;
}

// The count's slices of [p0, p1): at most sp positions and at most max_cols columns each (a position with more columns
// than that is a slice of its own).  pos_col is the layout's, index q - S, non-decreasing.
std::vector<int64_t> plp_column_cuts(const int64_t *pos_col, int64_t S, int64_t p0, int64_t p1, int64_t sp, int64_t max_cols)
{
    std::vector<int64_t> cuts{p0};
    for (int64_t q0 = p0; q0 < p1;) {
        const int64_t hi = std::min(p1, q0 + sp);
        // the last q in (q0, hi] with pos_col[q] - pos_col[q0] <= max_cols
        const int64_t *b = pos_col + (q0 + 1 - S), *e = pos_col + (hi - S) + 1;
        int64_t q1 = q0 + (std::upper_bound(b, e, pos_col[q0 - S] + max_cols) - b);
        if (q1 <= q0) q1 = q0 + 1;
        cuts.push_back(q1);
        q0 = q1;
    }
    return cuts;
}

bool op_ref(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
bool op_query(int op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

// What the host entries know about the reads after checking them: each read's end, the prefix maximum of the ends (the
// reads of a slice are a contiguous range: from the first whose prefix maximum passes the slice to the first that starts
// after it) and the aligned bases of every slice of the region (the devices' shares are cut by those).
struct PlpHostReads {
    std::vector<int32_t> rend, pmax;
    std::vector<int64_t> cuts;                   // slice k = positions [cuts[k], cuts[k+1])
    std::vector<double> slice_cost;
};

int plp_check_reads(const gbx_pileup_params *p, const gbx_pileup_reads *R, std::vector<int64_t> cuts, PlpHostReads &H, const char *who)
{
    if (!R) { set_error("%s: null reads", who); return GBX_ERR_ARG; }
    const int64_t n = R->n_reads;
    if (n < 0 || R->seq_bytes < 0) { set_error("%s: n_reads %lld, seq_bytes %lld", who, (long long)n, (long long)R->seq_bytes); return GBX_ERR_ARG; }
    if (n > 0 && (!R->pos || !R->cigar_off || !R->seq_off || !R->seq_boff || !R->rev || (p->num_dtypes > 1 && !R->dtype))) {
        set_error("%s: null pointer among the reads' arrays", who);
        return GBX_ERR_ARG;
    }
    if (n > 0 && (R->cigar_off[0] < 0 || R->seq_off[0] < 0)) { set_error("%s: negative first offset", who); return GBX_ERR_ARG; }
    if (n > 0 && ((R->cigar_off[n] > R->cigar_off[0] && !R->cigar) || (R->seq_off[n] > R->seq_off[0] && (!R->seq || !R->qual)))) {
        set_error("%s: null pointer among the reads' arrays", who);
        return GBX_ERR_ARG;
    }
    H.rend.assign((size_t)n, 0);
    H.pmax.assign((size_t)n, 0);
    const int64_t S = p->start, E = p->end, n_slices = (int64_t)cuts.size() - 1;
    H.cuts = std::move(cuts);
    const int64_t *ct = H.cuts.data();
    const int T = std::max(1, std::min<int>(host_workers(), (int)std::max<int64_t>(1, n / 1024)));
    std::vector<std::vector<double>> cost((size_t)T);
    std::vector<int64_t> first_bad((size_t)T, -1);
    std::vector<std::string> why((size_t)T);
    parallel_ranges(n, T, [&](int t, int64_t lo, int64_t hi) {
        std::vector<double> &c = cost[(size_t)t];
        c.assign((size_t)n_slices, 0.0);
        char buf[256];
        for (int64_t r = lo; r < hi; ++r) {
            const int64_t k0 = R->cigar_off[r], k1 = R->cigar_off[r + 1], b0 = R->seq_off[r], b1 = R->seq_off[r + 1];
            const int64_t l_seq = b1 - b0;
            const char *bad = nullptr;
            if (k1 < k0 || b1 < b0) bad = "offsets decrease";
            else if (R->pos[r] < 0) bad = "negative pos";
            else if (r > 0 && R->pos[r] < R->pos[r - 1]) bad = "reads are not sorted by pos";
            else if (R->seq_boff[r] < 0 || R->seq_boff[r] > R->seq_bytes - (l_seq + 1) / 2) bad = "its bases lie outside seq_bytes";
            int64_t rp = R->pos[r], qlen = 0;
            for (int64_t k = k0; !bad && k < k1; ++k) {
                const int op = (int)(R->cigar[k] & 15u);
                const int64_t len = (int64_t)(R->cigar[k] >> 4);
                if (op > 8) { bad = "a CIGAR op outside MIDNSHP=X"; break; }
                if (op_ref(op)) {
                    if ((op == 0 || op == 7 || op == 8) && n_slices > 0) {
                        int64_t a = std::max(rp, S);
                        const int64_t b = std::min(rp + len, E);
                        while (a < b) {
                            const int64_t sl = (std::upper_bound(ct, ct + n_slices + 1, a) - ct) - 1, se = std::min(b, ct[sl + 1]);
                            c[(size_t)sl] += (double)(se - a);
                            a = se;
                        }
                    }
                    rp += len;
                }
                if (op_query(op)) qlen += len;
            }
            if (!bad && qlen != l_seq) {
                snprintf(buf, sizeof buf, "the CIGAR's query length %lld is not l_seq = %lld", (long long)qlen, (long long)l_seq);
                bad = buf;
            }
            if (!bad && rp > INT32_MAX) bad = "it ends at or beyond 2^31";
            if (bad) { first_bad[(size_t)t] = r; why[(size_t)t] = bad; return; }
            H.rend[(size_t)r] = (int32_t)rp;
        }
    });
    for (int t = 0; t < T; ++t)
        if (first_bad[(size_t)t] >= 0) {
            set_error("%s: read %lld: %s", who, (long long)first_bad[(size_t)t], why[(size_t)t].c_str());
            return GBX_ERR_ARG;
        }
    int32_t m = INT32_MIN;
    for (int64_t r = 0; r < n; ++r) { m = std::max(m, H.rend[(size_t)r]); H.pmax[(size_t)r] = m; }
    H.slice_cost.assign((size_t)n_slices, 0.0);
    for (int t = 0; t < T; ++t)
        for (int64_t k = 0; k < n_slices && !cost[(size_t)t].empty(); ++k) H.slice_cost[(size_t)k] += cost[(size_t)t][(size_t)k];
    return GBX_OK;
}

// The reads of positions [q0, q1), uploaded as a gbx_pileup_reads of their own (offsets rebased) into buffers of the lane.
struct SliceReads {
    int64_t ra = 0, rb = 0;
    gbx_pileup_reads d{};
    int64_t n_cigar = 0;
};

int plp_upload_reads(const gbx_pileup_reads *R, const PlpHostReads &H, int64_t q0, int64_t q1, bool need_dtype, hipStream_t s,
                     DevBuf &dpos, DevBuf &dcoff, DevBuf &dcig, DevBuf &dsoff, DevBuf &dsboff, DevBuf &dseq, DevBuf &dqual, DevBuf &drev,
                     DevBuf &ddt, SliceReads &out)
{
    const int64_t n = R->n_reads;
    const int32_t *pm = H.pmax.data();
    out.ra = std::upper_bound(pm, pm + n, (int32_t)q0) - pm;
    out.rb = n > 0 ? std::lower_bound(R->pos, R->pos + n, (int32_t)std::min<int64_t>(q1, INT32_MAX)) - R->pos : 0;
    if (out.rb < out.ra) out.rb = out.ra;
    const int64_t ra = out.ra, m = out.rb - out.ra;
    out.d = gbx_pileup_reads{};
    out.d.n_reads = m;
    if (m == 0) return GBX_OK;
    const int64_t c0 = R->cigar_off[ra], c1 = R->cigar_off[ra + m], b0 = R->seq_off[ra], b1 = R->seq_off[ra + m];
    out.n_cigar = c1 - c0;
    int64_t s0 = INT64_MAX, s1 = 0;
    for (int64_t j = ra; j < ra + m; ++j) {
        s0 = std::min(s0, R->seq_boff[j]);
        s1 = std::max(s1, R->seq_boff[j] + (R->seq_off[j + 1] - R->seq_off[j] + 1) / 2);
    }
    std::vector<int64_t> coff((size_t)m + 1), soff((size_t)m + 1), sboff((size_t)m);
    for (int64_t j = 0; j <= m; ++j) { coff[(size_t)j] = R->cigar_off[ra + j] - c0; soff[(size_t)j] = R->seq_off[ra + j] - b0; }
    for (int64_t j = 0; j < m; ++j) sboff[(size_t)j] = R->seq_boff[ra + j] - s0;
    int rc;
    if ((rc = dpos.alloc((size_t)m * 4)) || (rc = dcoff.alloc((size_t)(m + 1) * 8)) || (rc = dcig.alloc((size_t)(c1 - c0) * 4)) ||
        (rc = dsoff.alloc((size_t)(m + 1) * 8)) || (rc = dsboff.alloc((size_t)m * 8)) || (rc = dseq.alloc((size_t)(s1 - s0))) ||
        (rc = dqual.alloc((size_t)(b1 - b0))) || (rc = drev.alloc((size_t)m)) || (rc = ddt.alloc((size_t)m)))
        return rc;
    GBX_HIP(hipMemcpyAsync(dpos.p, R->pos + ra, (size_t)m * 4, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(dcoff.p, coff.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
    if (c1 > c0) GBX_HIP(hipMemcpyAsync(dcig.p, R->cigar + c0, (size_t)(c1 - c0) * 4, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(dsoff.p, soff.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(dsboff.p, sboff.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
    if (s1 > s0) GBX_HIP(hipMemcpyAsync(dseq.p, R->seq + s0, (size_t)(s1 - s0), hipMemcpyHostToDevice, s));
    if (b1 > b0) GBX_HIP(hipMemcpyAsync(dqual.p, R->qual + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(drev.p, R->rev + ra, (size_t)m, hipMemcpyHostToDevice, s));
    if (need_dtype) GBX_HIP(hipMemcpyAsync(ddt.p, R->dtype + ra, (size_t)m, hipMemcpyHostToDevice, s));
    // the copies above read pageable host vectors of this frame: they are complete before the caller's next sync, which
    // every slice makes before its vectors go out of scope
    GBX_HIP(hipStreamSynchronize(s));
    out.d.seq_bytes = s1 - s0;
    out.d.pos = dpos.as<int32_t>();
    out.d.cigar_off = dcoff.as<int64_t>();
    out.d.cigar = dcig.as<uint32_t>();
    out.d.seq_off = dsoff.as<int64_t>();
    out.d.seq_boff = dsboff.as<int64_t>();
    out.d.seq = dseq.as<uint8_t>();
    out.d.qual = dqual.as<uint8_t>();
    out.d.rev = drev.as<uint8_t>();
    out.d.dtype = need_dtype ? ddt.as<int8_t>() : nullptr;
    return GBX_OK;
}

// Slices [lo, hi) of the region on the current device, one after the other; fn(k, q0, q1) does slice k.
template <class Fn> int plp_run_slices(const PlpHostReads &H, const char *who, Fn fn)
{
    const int64_t n_slices = (int64_t)H.slice_cost.size();
    auto range = [&](int64_t lo, int64_t hi) -> int {
        for (int64_t k = lo; k < hi; ++k) {
            const int rc = fn(k, H.cuts[(size_t)k], H.cuts[(size_t)k + 1]);
            if (rc) return rc;
        }
        return GBX_OK;
    };
    return spread_over_devices(who, n_slices, n_slices, 1, [&](int64_t k) { return H.slice_cost[(size_t)k] + 1.0; },
                               [&]() { return range(0, n_slices); }, [&](int, int64_t lo, int64_t hi) { return range(lo, hi); });
}

}  // namespace

extern "C" {

size_t gbx_pileup_workspace_bytes(const gbx_pileup_params *p, int64_t n_reads, int64_t n_cigar)
{
    if (!p || p->start < 0 || p->end < p->start || n_reads < 0 || n_cigar < 0) return 0;
    return pileup_workspace_bytes(n_reads, n_cigar, p->end - p->start);
}

int gbx_pileup_layout_device(const gbx_pileup_params *p, const gbx_pileup_reads *reads, int64_t *d_pos_col, gbx_pileup_layout_stats *d_stats,
                             void *d_work, size_t work_bytes, void *stream)
{
    int rc = plp_params_check(p, "gbx_pileup_layout_device");
    if (rc) return rc;
    if (!reads || reads->n_reads < 0 || !d_pos_col || !d_stats || !d_work ||
        (reads->n_reads > 0 && (!reads->pos || !reads->cigar_off || !reads->cigar || !reads->seq_off || !reads->seq_boff || !reads->rev))) {
        set_error("gbx_pileup_layout_device: null pointer or negative n_reads");
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return pileup_layout_launch(p, reads, d_pos_col, d_stats, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_pileup_count_device(const gbx_pileup_params *p, const gbx_pileup_reads *reads, const int64_t *d_pos_col, int64_t p0, int64_t p1,
                            int32_t *d_major, int32_t *d_minor, uint32_t *d_counts, void *d_work, size_t work_bytes, void *stream)
{
    int rc = plp_params_check(p, "gbx_pileup_count_device");
    if (rc) return rc;
    if (p0 < p->start || p1 < p0 || p1 > p->end) {
        set_error("gbx_pileup_count_device: positions [%lld, %lld) outside the region [%lld, %lld)", (long long)p0, (long long)p1,
                  (long long)p->start, (long long)p->end);
        return GBX_ERR_ARG;
    }
    if (!reads || reads->n_reads < 0 || !d_pos_col || !d_work || (p1 > p0 && (!d_major || !d_minor || !d_counts)) ||
        (reads->n_reads > 0 && (!reads->pos || !reads->cigar_off || !reads->cigar || !reads->seq_off || !reads->seq_boff || !reads->seq ||
                                !reads->qual || !reads->rev))) {
        set_error("gbx_pileup_count_device: null pointer or negative n_reads");
        return GBX_ERR_ARG;
    }
    if ((rc = require_device())) return rc;
    return pileup_count_launch(p, reads, d_pos_col, p0, p1, d_major, d_minor, d_counts, d_work, work_bytes, (hipStream_t)stream);
}

// The host entries: the region in slices of slice_positions positions, each with the reads that overlap it, spread over the
// devices by aligned bases (host_multi.h).  A slice's layout gives its own pos_col from 0; the slices' column totals then
// move every slice's values to the region's numbering.
int gbx_pileup_layout_host(const gbx_pileup_params *p, const gbx_pileup_reads *reads, int64_t *pos_col, gbx_pileup_layout_stats *st)
{
    RoctxRange range_("gbx_pileup_layout_host");
    const char *who = "gbx_pileup_layout_host";
    int rc = plp_params_check(p, who);
    if (rc) return rc;
    if (!pos_col || !st) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    PlpHostReads H;
    if ((rc = plp_check_reads(p, reads, plp_position_cuts(p->start, p->end, plp_slice_positions(p)), H, who))) return rc;
    if ((rc = require_device())) return rc;
    const int64_t n_slices = (int64_t)H.slice_cost.size();
    std::vector<gbx_pileup_layout_stats> sst((size_t)n_slices);
    std::vector<int64_t> sra((size_t)n_slices, 0);
    const bool need_dt = p->num_dtypes > 1;
    rc = plp_run_slices(H, who, [&](int64_t k, int64_t q0, int64_t q1) -> int {
        HostLane lane;
        int rc1;
        if ((rc1 = lane.acquire())) return rc1;
        Lane *L = lane.l;
        hipStream_t s = L->compute;
        DevBuf dpos(L), dcoff(L), dcig(L), dsoff(L), dsboff(L), dseq(L), dqual(L), drev(L), ddt(L), dpc(L), dst(L), dw(L);
        SliceReads sr;
        if ((rc1 = plp_upload_reads(reads, H, q0, q1, need_dt, s, dpos, dcoff, dcig, dsoff, dsboff, dseq, dqual, drev, ddt, sr))) return rc1;
        sra[(size_t)k] = sr.ra;
        gbx_pileup_params sp_ = *p;
        sp_.start = q0; sp_.end = q1;
        const size_t wb = pileup_workspace_bytes(sr.d.n_reads, sr.n_cigar, q1 - q0);
        if ((rc1 = dpc.alloc((size_t)(q1 - q0 + 1) * 8)) || (rc1 = dst.alloc(sizeof(gbx_pileup_layout_stats))) || (rc1 = dw.alloc(wb))) return rc1;
        if ((rc1 = pileup_layout_launch(&sp_, &sr.d, dpc.as<int64_t>(), dst.as<gbx_pileup_layout_stats>(), dw.p, wb, s))) return rc1;
        GBX_HIP(hipMemcpyAsync(pos_col + (q0 - p->start), dpc.p, (size_t)(q1 - q0) * 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(&sst[(size_t)k], dst.p, sizeof(gbx_pileup_layout_stats), hipMemcpyDeviceToHost, s));
        GBX_HIP(hipStreamSynchronize(s));
        return GBX_OK;
    });
    if (rc) return rc;
    gbx_pileup_layout_stats t{};
    t.bad_read = -1;
    std::vector<int64_t> base((size_t)n_slices, 0);
    for (int64_t k = 0; k < n_slices; ++k) {
        const gbx_pileup_layout_stats &a = sst[(size_t)k];
        base[(size_t)k] = t.n_cols;
        t.n_cols += a.n_cols;
        t.n_positions += a.n_positions;
        t.max_ins = std::max(t.max_ins, a.max_ins);
        t.max_depth = std::max(t.max_depth, a.max_depth);
        t.aligned_bases += a.aligned_bases;
        if (a.bad_read >= 0 && (t.bad_read < 0 || sra[(size_t)k] + a.bad_read < t.bad_read)) t.bad_read = sra[(size_t)k] + a.bad_read;
    }
    parallel_ranges(n_slices, std::min(host_workers(), (int)std::max<int64_t>(1, n_slices)), [&](int, int64_t lo, int64_t hi) {
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t q0 = H.cuts[(size_t)k], q1 = H.cuts[(size_t)k + 1], b = base[(size_t)k];
            if (b) for (int64_t q = q0; q < q1; ++q) pos_col[q - p->start] += b;
        }
    });
    pos_col[p->end - p->start] = t.n_cols;
    *st = t;
    if (t.bad_read >= 0) {
        set_error("%s: read %lld has no valid dtype (num_dtypes = %d)", who, (long long)t.bad_read, p->num_dtypes);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int gbx_pileup_count_host(const gbx_pileup_params *p, const gbx_pileup_reads *reads, const int64_t *pos_col, int64_t p0, int64_t p1,
                          int32_t *major, int32_t *minor, uint32_t *counts)
{
    RoctxRange range_("gbx_pileup_count_host");
    const char *who = "gbx_pileup_count_host";
    int rc = plp_params_check(p, who);
    if (rc) return rc;
    if (p0 < p->start || p1 < p0 || p1 > p->end) {
        set_error("%s: positions [%lld, %lld) outside the region [%lld, %lld)", who, (long long)p0, (long long)p1, (long long)p->start,
                  (long long)p->end);
        return GBX_ERR_ARG;
    }
    if (!pos_col) { set_error("%s: null pos_col", who); return GBX_ERR_ARG; }
    for (int64_t q = p0; q < p1; ++q)
        if (pos_col[q + 1 - p->start] < pos_col[q - p->start] || pos_col[q - p->start] < 0) {
            set_error("%s: pos_col decreases at position %lld", who, (long long)q);
            return GBX_ERR_ARG;
        }
    const int64_t c_base = pos_col[p0 - p->start], n_cols = pos_col[p1 - p->start] - c_base;
    if (n_cols > 0 && (!major || !minor || !counts)) { set_error("%s: null output", who); return GBX_ERR_ARG; }
    // the count slices cover [p0, p1) only: the region stays the layout's, the slices start at p0
    gbx_pileup_params q = *p;
    q.start = p0; q.end = p1;
    const int F = plp_feat(p);
    PlpHostReads H;
    if ((rc = plp_check_reads(&q, reads, plp_column_cuts(pos_col, p->start, p0, p1, plp_slice_positions(p), std::max<int64_t>(1, PLP_SLICE_CELLS / F)),
                              H, who)))
        return rc;
    if (n_cols == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    const bool need_dt = p->num_dtypes > 1;
    std::vector<int64_t> bad((size_t)H.slice_cost.size(), -1);
    rc = plp_run_slices(H, who, [&](int64_t k, int64_t q0, int64_t q1) -> int {
        const int64_t cs = pos_col[q0 - p->start], ce = pos_col[q1 - p->start], nc = ce - cs;
        if (nc == 0) return GBX_OK;
        HostLane lane;
        int rc1;
        if ((rc1 = lane.acquire())) return rc1;
        Lane *L = lane.l;
        hipStream_t s = L->compute;
        DevBuf dpos(L), dcoff(L), dcig(L), dsoff(L), dsboff(L), dseq(L), dqual(L), drev(L), ddt(L), dpc(L), dmaj(L), dmin(L), dcnt(L), dw(L);
        SliceReads sr;
        if ((rc1 = plp_upload_reads(reads, H, q0, q1, need_dt, s, dpos, dcoff, dcig, dsoff, dsboff, dseq, dqual, drev, ddt, sr))) return rc1;
        gbx_pileup_params sp_ = *p;
        sp_.start = q0; sp_.end = q1;
        const size_t wb = pileup_workspace_bytes(sr.d.n_reads, sr.n_cigar, q1 - q0);
        if ((rc1 = dpc.alloc((size_t)(q1 - q0 + 1) * 8)) || (rc1 = dmaj.alloc((size_t)nc * 4)) || (rc1 = dmin.alloc((size_t)nc * 4)) ||
            (rc1 = dcnt.alloc((size_t)nc * F * 4)) || (rc1 = dw.alloc(wb)))
            return rc1;
        GBX_HIP(hipMemcpyAsync(dpc.p, pos_col + (q0 - p->start), (size_t)(q1 - q0 + 1) * 8, hipMemcpyHostToDevice, s));
        if ((rc1 = pileup_count_launch(&sp_, &sr.d, dpc.as<int64_t>(), q0, q1, dmaj.as<int32_t>(), dmin.as<int32_t>(), dcnt.as<uint32_t>(), dw.p,
                                       wb, s)))
            return rc1;
        const int64_t at = cs - c_base;
        GBX_HIP(hipMemcpyAsync(major + at, dmaj.p, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(minor + at, dmin.p, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(counts + at * F, dcnt.p, (size_t)nc * F * 4, hipMemcpyDeviceToHost, s));
        int64_t b = -1;
        if ((rc1 = pileup_read_bad(&sp_, &sr.d, dw.p, &b, s))) return rc1;
        if (b >= 0) bad[(size_t)k] = sr.ra + b;
        return GBX_OK;
    });
    if (rc) return rc;
    for (int64_t b : bad)
        if (b >= 0) {
            set_error("%s: read %lld has no valid dtype (num_dtypes = %d)", who, (long long)b, p->num_dtypes);
            return GBX_ERR_ARG;
        }
    return GBX_OK;
}

}  // extern "C"
