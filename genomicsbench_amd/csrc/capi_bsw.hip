// capi_bsw.hip — bsw entries of the C-ABI (include/gbx.h): device entry, host-buffer entry, the SeqPair drop-in.
#include "capi_common.h"

static constexpr int BSW_HOST_WORKERS = 4;        // upload / validation helpers of a bsw host call (host_workers: GBX_HOST_THREADS overrides)

using namespace gbx;

extern "C" {

/* --------------------------------------------------------------------- bsw */
void gbx_bsw_fill_scmat(int a, int b, int ambig, int8_t mat[25])
{
    int k = 0;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j) mat[k++] = (int8_t)(i == j ? a : -b);
        mat[k++] = (int8_t)ambig;
    }
    for (int j = 0; j < 5; ++j) mat[k++] = (int8_t)ambig;
}

void gbx_bsw_default_params(gbx_bsw_params *p)
{
    memset(p, 0, sizeof(*p));
    p->o_del = p->o_ins = 6; p->e_del = p->e_ins = 1;
    p->zdrop = 100; p->end_bonus = 5; p->w = 100;
    gbx_bsw_fill_scmat(1, 4, -1, p->mat);
}

size_t gbx_bsw_workspace_bytes(int64_t n) { return bsw_workspace_bytes(n); }

// Debug read-back of the lane sort (the tests): the sorted pair indices (n ints, the lists' total of them valid) and the
// first position of every key row (LANE_ROWS + 1 ints, the last = the total) of the last call on a workspace of n pairs.
int gbx_debug_bsw_lane_lists(const void *d_work, int64_t n, int32_t *h_order, int32_t *h_row_first)
{
    if (!d_work || !h_order || !h_row_first) { set_error("gbx_debug_bsw_lane_lists: null pointer"); return GBX_ERR_ARG; }
    return bsw_debug_lane_lists(d_work, n, h_order, h_row_first);
}
int gbx_debug_bsw_lane_sort_tile(void) { return bsw_lane_sort_tile(); }

int gbx_bsw_extend_device(const gbx_bsw_params *p, int64_t n,
                          const uint8_t *d_ref, const uint8_t *d_qer,
                          const int64_t *d_idr, const int64_t *d_idq,
                          const int32_t *d_len1, const int32_t *d_len2,
                          const int32_t *d_h0, gbx_bsw_result *d_out,
                          void *d_work, size_t work_bytes, void *stream)
{
    if (!p || n < 0) { set_error("gbx_bsw_extend_device: bad argument"); return GBX_ERR_ARG; }
    if (n == 0) return GBX_OK;
    if (!d_ref || !d_qer || !d_idr || !d_idq || !d_len1 || !d_len2 || !d_h0 || !d_out || !d_work) {
        set_error("gbx_bsw_extend_device: null pointer");
        return GBX_ERR_ARG;
    }
    int rc = require_device();
    if (rc) return rc;
    return bsw_launch(p, n, d_ref, d_qer, d_idr, d_idq, d_len1, d_len2, d_h0, d_out, d_work, work_bytes,
                      (hipStream_t)stream);
}

// Is a pair inside the arenas, and within what the kernels hold?  Outside the arenas is the error a call reports first.
enum BswPairFault { BSW_PAIR_OK = 0, BSW_PAIR_OUTSIDE, BSW_PAIR_TOO_LONG };
static inline BswPairFault bsw_pair_fault(int64_t idr, int64_t idq, int64_t len1, int64_t len2, int64_t ref_bytes, int64_t qer_bytes)
{
    if (len1 < 0 || len2 < 0 || idr < 0 || idq < 0 || idr + len1 > ref_bytes || idq + len2 > qer_bytes) return BSW_PAIR_OUTSIDE;
    return len2 > GBX_BSW_MAX_QLEN || len1 > GBX_BSW_MAX_TLEN ? BSW_PAIR_TOO_LONG : BSW_PAIR_OK;
}

// The arguments of a host call.  `base` = index of pairs[0] in the caller's job (error texts only).
struct BswHostJob {
    const gbx_bsw_params *p; int64_t n;
    const uint8_t *ref; int64_t ref_bytes; const uint8_t *qer; int64_t qer_bytes;
    const int64_t *idr, *idq; const int32_t *len1, *len2, *h0; gbx_bsw_result *out; int64_t base;
};

// The device buffers of a host call (ref_p / qer_p: the packed images of the arenas, when the bases go up two per byte)
struct BswHostBufs {
    DevBuf ref, qer, idr, idq, l1, l2, h0, out, work, ref_p, qer_p;
    explicit BswHostBufs(Lane *L) : ref(L), qer(L), idr(L), idq(L), l1(L), l2(L), h0(L), out(L), work(L), ref_p(L), qer_p(L) {}
};

// The plan of a host call.  One pass over the pairs, in slices of 32 Ki pairs and with a few threads when there are many:
// validation, and what the pipeline needs to know of them.  Then the pipeline's chunks (chunk c = pairs [cut[c], cut[c + 1])):
// what each needs of the arenas, and its uploads.
struct BswHostPlan {
    static constexpr int64_t SL = 32768;
    const BswHostJob &j;
    const std::vector<int64_t> cut = bsw_host_cuts(j.n);
    const int64_t n_chunks = (int64_t)cut.size() - 1, n_slices = (j.n + SL - 1) / SL;
    int64_t chunk = 0;                                                  // the largest chunk
    BswLaneRule rule = {0, 0, 0, 0};                                    // of a launch of `chunk` pairs
    // per slice: the furthest arena bytes its pairs need; its first failing pair, or -1; the pairs the lane kernels will not take
    // (BswChunkPrep::rows_pairs); the longest query if every pair has 1 <= qlen <= 256, tlen >= 1 and a small h0 (bsw_launch_direct), else 0
    std::vector<int64_t> far_r, far_q, bad, slice_rows, plain;
    // per chunk: the furthest arena bytes it needs, its rows_pairs, and the ranges of the packed arenas that went up with it
    std::vector<int64_t> need_r, need_q, rows_pairs, lo_r, hi_r, lo_q, hi_q;
    int64_t up_r = 0, up_q = 0;                                         // the arenas are uploaded up to here
    explicit BswHostPlan(const BswHostJob &job)
        : j(job), far_r((size_t)n_slices), far_q(far_r), bad((size_t)n_slices, -1), slice_rows(far_r), plain(far_r), need_r((size_t)n_chunks),
          need_q(need_r), rows_pairs((size_t)n_chunks, -1), lo_r(need_r), hi_r(need_r), lo_q(need_r), hi_q(need_r)
    {
        for (int64_t c = 0; c < n_chunks; ++c) chunk = pairs(c) > chunk ? pairs(c) : chunk;
        if (bsw_lane_rule(j.p, chunk, &rule) != GBX_OK) rule.on = 0;    // (bad parameters: the launch reports them)
    }
    int64_t pairs(int64_t c) const { return cut[(size_t)c + 1] - cut[(size_t)c]; }
    void check_slice(int64_t sl)
    {
        const int64_t a = sl * SL, b = a + SL < j.n ? a + SL : j.n;
        const int64_t *idr = j.idr, *idq = j.idq;
        const int32_t *len1 = j.len1, *len2 = j.len2, *h0 = j.h0;
        int64_t mr = 0, mq = 0, nrows = 0;
        bool all_plain = true;
        int maxq = 1;
        for (int64_t k = a; k < b; ++k) {
            nrows += !bsw_lane_takes(rule, len2[k], len1[k], h0[k]) && len1[k] != 0 && len2[k] != 0;
            all_plain = all_plain && len2[k] >= 1 && len2[k] <= 256 && len1[k] >= 1 && h0[k] < 1000000;
            maxq = len2[k] > maxq ? len2[k] : maxq;
            if (bsw_pair_fault(idr[k], idq[k], len1[k], len2[k], j.ref_bytes, j.qer_bytes)) { bad[(size_t)sl] = k; return; }
            const int64_t er = idr[k] + len1[k], eq = idq[k] + len2[k];
            mr = er > mr ? er : mr; mq = eq > mq ? eq : mq;
        }
        far_r[(size_t)sl] = mr; far_q[(size_t)sl] = mq; plain[(size_t)sl] = all_plain ? maxq : 0; slice_rows[(size_t)sl] = nrows;
    }
    // slices [s0, s1): checked by a few threads; the lowest failing pair is reported
    int validate(int64_t s0, int64_t s1)
    {
        const int64_t cnt = s1 - s0;
        const int vt = cnt >= 24 ? 12 : cnt >= 8 ? (int)(cnt / 2) : 1;      // 2.5 ns a pair and thread: 0.9 ms with 4 threads at 2 M pairs
        std::vector<Helper> th;
        for (int t = 1; t < vt; ++t) th.emplace_back([this, s0, s1, vt, t] { for (int64_t sl = s0 + t; sl < s1; sl += vt) check_slice(sl); }, true);
        for (int64_t sl = s0; sl < s1; sl += vt) check_slice(sl);
        for (auto &x : th) x.join();
        for (int64_t sl = s0; sl < s1; ++sl) {
            const int64_t k = bad[(size_t)sl];
            if (k < 0) continue;
            const bool too_long = bsw_pair_fault(j.idr[k], j.idq[k], j.len1[k], j.len2[k], j.ref_bytes, j.qer_bytes) == BSW_PAIR_TOO_LONG;
            set_error(too_long ? "gbx_bsw_extend_host: pair %lld exceeds GBX_BSW_MAX_QLEN/TLEN" : "gbx_bsw_extend_host: pair %lld lies outside the arenas",
                      (long long)(j.base + k));
            return too_long ? GBX_ERR_UNSUPPORTED : GBX_ERR_ARG;
        }
        return GBX_OK;
    }
    void needs(int64_t c)
    {
        int64_t mr = 0, mq = 0, rows = 0;
        // chunks are multiples of 64 pairs, slices of 32768: a slice may straddle two chunks, which only makes
        // the earlier chunk wait for a few more bytes
        for (int64_t sl = cut[(size_t)c] / SL; sl < n_slices && sl * SL < cut[(size_t)c + 1]; ++sl) {
            mr = far_r[(size_t)sl] > mr ? far_r[(size_t)sl] : mr;
            mq = far_q[(size_t)sl] > mq ? far_q[(size_t)sl] : mq;
            rows += slice_rows[(size_t)sl];
        }
        need_r[(size_t)c] = mr; need_q[(size_t)c] = mq;
        // (an upper bound: a slice that straddles two chunks counts for both; a short last chunk may run without the lane path)
        BswLaneRule last = rule;
        if (pairs(c) != chunk && bsw_lane_rule(j.p, pairs(c), &last) != GBX_OK) last.on = 0;
        rows_pairs[(size_t)c] = rule.on && last.on ? rows : -1;
    }
    // Two upload stages per chunk: its index arrays (stage 2c: all the preparing passes read) and then its bases (2c + 1)
    void stage(int64_t c, HostPipe &pipe, BswHostBufs &d, bool pack_bases)
    {
        const int64_t a = cut[(size_t)c], m = pairs(c);
        pipe.stage(2 * c, d.idr.as<int64_t>() + a, j.idr + a, m * 8);
        pipe.stage(2 * c, d.idq.as<int64_t>() + a, j.idq + a, m * 8);
        pipe.stage(2 * c, d.l1.as<int32_t>() + a, j.len1 + a, m * 4);
        pipe.stage(2 * c, d.l2.as<int32_t>() + a, j.len2 + a, m * 4);
        pipe.stage(2 * c, d.h0.as<int32_t>() + a, j.h0 + a, m * 4);
        int64_t nr = need_r[(size_t)c] > up_r ? need_r[(size_t)c] : up_r;
        int64_t nq = need_q[(size_t)c] > up_q ? need_q[(size_t)c] : up_q;
        if (pack_bases) {
            // packed ranges start at even offsets: round the ends up to even while the arena allows it
            if ((nr & 1) && nr < j.ref_bytes) ++nr;
            if ((nq & 1) && nq < j.qer_bytes) ++nq;
            pipe.stage_pack4(2 * c + 1, d.ref_p.as<uint8_t>() + up_r / 2, j.ref + up_r, (size_t)(nr - up_r));
            pipe.stage_pack4(2 * c + 1, d.qer_p.as<uint8_t>() + up_q / 2, j.qer + up_q, (size_t)(nq - up_q));
            lo_r[(size_t)c] = up_r; hi_r[(size_t)c] = nr; lo_q[(size_t)c] = up_q; hi_q[(size_t)c] = nq;
        } else {
            pipe.stage(2 * c + 1, d.ref.as<uint8_t>() + up_r, j.ref + up_r, (size_t)(nr - up_r));
            pipe.stage(2 * c + 1, d.qer.as<uint8_t>() + up_q, j.qer + up_q, (size_t)(nq - up_q));
        }
        up_r = nr; up_q = nq;
    }
};

// One device (the calling thread's current one).
static int bsw_host_one(const gbx_bsw_params *p, int64_t n,
                        const uint8_t *ref, int64_t ref_bytes,
                        const uint8_t *qer, int64_t qer_bytes,
                        const int64_t *idr, const int64_t *idq,
                        const int32_t *len1, const int32_t *len2,
                        const int32_t *h0, gbx_bsw_result *out, int64_t base = 0)
{
    RoctxRange range_("gbx_bsw_extend_host");
    if (!p || n < 0 || ref_bytes < 0 || qer_bytes < 0) { set_error("gbx_bsw_extend_host: bad argument"); return GBX_ERR_ARG; }
    if (n == 0) return GBX_OK;
    if (!ref || !qer || !idr || !idq || !len1 || !len2 || !h0 || !out) {
        set_error("gbx_bsw_extend_host: null pointer");
        return GBX_ERR_ARG;
    }
    const BswHostJob j = {p, n, ref, ref_bytes, qer, qer_bytes, idr, idq, len1, len2, h0, out, base};
    const bool trace = getenv("GBX_HOST_TRACE") != nullptr;     /* timeline of this call on stderr */
    const double t_begin = wall_s();
    auto mark = [&](const char *what, int64_t k) { if (trace) fprintf(stderr, "[gbx host] %8.3f ms %s %lld\n", (wall_s() - t_begin) * 1e3, what, (long long)k); };
    BswHostPlan plan(j);
    const int64_t n_chunks = plan.n_chunks, n_slices = plan.n_slices, SL = plan.SL, chunk = plan.chunk;
    // A pipelined call checks the first chunk's pairs, starts its upload, and checks the rest while it is on its way (the
    // whole pass is 0.75 ms at 2 M pairs, and nothing else of the call can start before the first chunk is on the device).
    const int64_t s_first = n_chunks > 1 && (plan.cut[1] + SL - 1) / SL < n_slices ? (plan.cut[1] + SL - 1) / SL : n_slices;
    int rc = plan.validate(0, s_first);
    if (rc) return rc;
    plan.needs(0);
    if ((rc = require_device())) return rc;
    mark("validated", s_first * SL < n ? s_first * SL : n);
    // Upload, compute and download are pipelined over chunks of pairs (host_pipeline.h).  Chunk k's bases and
    // index slices go up while earlier chunks run; the arenas are uploaded front to back up to the furthest
    // byte any pair seen so far needs (a running maximum), which is right for every offset layout and streams
    // perfectly for the usual monotone one.  The chunks are queued back to back without a barrier between them
    // (own workspace each; the launch records the events a chunk's download waits for), and their results come
    // back while later chunks run.  Chunks are multiples of 64 pairs.
    const size_t wb1 = (bsw_workspace_bytes(chunk) + 255) & ~(size_t)255;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    BswHostBufs d(L);
    if ((rc = d.ref.alloc((size_t)ref_bytes)) || (rc = d.qer.alloc((size_t)qer_bytes)) ||
        (rc = d.idr.alloc(n * 8)) || (rc = d.idq.alloc(n * 8)) || (rc = d.l1.alloc(n * 4)) ||
        (rc = d.l2.alloc(n * 4)) || (rc = d.h0.alloc(n * 4)) || (rc = d.out.alloc(n * sizeof(gbx_bsw_result))) ||
        (rc = d.work.alloc(wb1 * (size_t)n_chunks)))
        return rc;
    mark("allocated", 0);
    HostPipe pipe(L, (size_t)ref_bytes + (size_t)qer_bytes + (size_t)n * 28, n_chunks > 1, BSW_HOST_WORKERS);
    if ((rc = pipe.prepare(n_chunks))) return rc;
    // Staged (large) calls send the bases two per byte: the upload workers pack them on their way into the pinned slabs
    // (host_pipeline.h: pack4), the device expands them into the byte arenas the kernels read (bsw_unpack4) - the
    // arenas are most of the upload (2 M pairs: 590 of 640 MB), and PCIe is the longest leg of the call.
    const bool pack_bases = pipe.staged && !(getenv("GBX_BSW_PACK") && atoi(getenv("GBX_BSW_PACK")) == 0);
    if (pack_bases && ((rc = d.ref_p.alloc((size_t)ref_bytes / 2 + 16)) || (rc = d.qer_p.alloc((size_t)qer_bytes / 2 + 16)))) return rc;
    int64_t unp_r = 0, unp_q = 0;       // the byte arenas are expanded up to here (BswChunkPrep::unp_r)
    pipe.upload_stages(2 * n_chunks);
    plan.stage(0, pipe, d, pack_bases);
    if (n_chunks > 1) pipe.keep_open();
    pipe.start();
    mark("pipeline started, chunks", n_chunks);
    if (n_chunks > 1) {
        if ((rc = plan.validate(s_first, n_slices))) return pipe.finish(rc);
        for (int64_t c = 1; c < n_chunks; ++c) { plan.needs(c); plan.stage(c, pipe, d, pack_bases); }
        pipe.seal();
        mark("all chunks staged", n);
    }
    // small jobs of plain pairs: one kernel launch instead of the binning passes and the class kernels
    bool direct = n <= 16384 && n_chunks == 1 && !(getenv("GBX_BSW_DIRECT") && atoi(getenv("GBX_BSW_DIRECT")) == 0);
    int64_t direct_q = 1;
    for (int64_t sl = 0; sl < n_slices && direct; ++sl) {
        direct = plan.plain[(size_t)sl] != 0;
        direct_q = plan.plain[(size_t)sl] > direct_q ? plan.plain[(size_t)sl] : direct_q;
    }
    if (direct) {
        if ((rc = pipe.wait_stage(0)) || (rc = pipe.wait_stage(1))) return pipe.finish(rc);
        if (pack_bases &&
            ((rc = bsw_unpack4(d.ref_p.as<uint8_t>(), d.ref.as<uint8_t>(), plan.lo_r[0], plan.hi_r[0], L->compute)) ||
             (rc = bsw_unpack4(d.qer_p.as<uint8_t>(), d.qer.as<uint8_t>(), plan.lo_q[0], plan.hi_q[0], L->compute))))
            return pipe.finish(rc);
        rc = bsw_launch_direct(p, n, (int)direct_q, d.ref.as<uint8_t>(), d.qer.as<uint8_t>(), d.idr.as<int64_t>(), d.idq.as<int64_t>(),
                               d.l1.as<int32_t>(), d.l2.as<int32_t>(), d.h0.as<int32_t>(), d.out.as<gbx_bsw_result>(), L->compute);
        if (!rc) { pipe.fetch(0, out, d.out.p, n * sizeof(gbx_bsw_result)); rc = pipe.chunk_launched(0, 0); }
        return pipe.finish(rc);
    }
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t a = plan.cut[(size_t)c], m = plan.pairs(c);
        // pipelined calls: no barrier between the chunks, the launch records one event per kernel stream, and what
        // prepares a chunk (classify, the lane sort; unpacking, if it has row-kernel pairs) waits for its uploads only
        // (BswChunkPrep) - in two calls where the launch allows it: the preparing passes behind the index arrays, while
        // the bases are still on their way, the kernels behind the bases
        hipEvent_t *je = n_chunks > 1 ? pipe.join_events(c) : nullptr;
        BswChunkPrep prep = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, plan.rows_pairs[(size_t)c], 0, L->ev_pre, L->ev_aux};
        if (pack_bases) {
            prep.ref_packed = d.ref_p.as<uint8_t>(); prep.ref_bytes = d.ref.as<uint8_t>();
            prep.qer_packed = d.qer_p.as<uint8_t>(); prep.qer_bytes = d.qer.as<uint8_t>();
            prep.lo_r = plan.lo_r[(size_t)c]; prep.hi_r = plan.hi_r[(size_t)c]; prep.lo_q = plan.lo_q[(size_t)c]; prep.hi_q = plan.hi_q[(size_t)c];
            prep.unp_r = &unp_r; prep.unp_q = &unp_q;
        }
        auto launch = [&]() {
            return bsw_launch(p, m, d.ref.as<uint8_t>(), d.qer.as<uint8_t>(), d.idr.as<int64_t>() + a, d.idq.as<int64_t>() + a,
                              d.l1.as<int32_t>() + a, d.l2.as<int32_t>() + a, d.h0.as<int32_t>() + a,
                              d.out.as<gbx_bsw_result>() + a, (char *)d.work.p + wb1 * (size_t)c, wb1, L->compute, je, &prep);
        };
        static const bool split_off = getenv("GBX_BSW_SPLIT_PREP") && atoi(getenv("GBX_BSW_SPLIT_PREP")) == 0;
        bool split = je && pipe.stage_event() && !split_off;
        if (split) {
            if ((rc = pipe.wait_stage(2 * c, L->ev_part))) return pipe.finish(rc);
            mark("index arrays queued, chunk", c);
            prep.phase = 1; prep.uploaded = L->ev_part;
            rc = launch();
            if (rc == 1) { split = false; rc = GBX_OK; }
            if (rc) return pipe.finish(rc);
        } else if ((rc = pipe.wait_stage(2 * c))) return pipe.finish(rc);
        if ((rc = pipe.wait_stage(2 * c + 1))) return pipe.finish(rc);
        mark("uploads queued, chunk", c);
        prep.phase = split ? 2 : 0;
        prep.uploaded = je ? pipe.stage_event() : nullptr;
        rc = launch();
        if (!rc) {
            pipe.fetch(c, out + a, d.out.as<gbx_bsw_result>() + a, m * sizeof(gbx_bsw_result));
            rc = pipe.chunk_launched(c, je ? Lane::JOIN_EVENTS : 0);
        }
        if (rc) return pipe.finish(rc);
    }
    mark("kernels queued", n_chunks);
    rc = pipe.finish();
    mark("results downloaded", 0);
    return rc;
}

// Would bsw_host_one accept this call?  (It checks the same itself, interleaved with its pipeline; this is the question the
// multi-device path and the call combiner ask first, so that a bad call takes the one-device path, whose error names the pair.)
static bool bsw_call_ok(const gbx_bsw_params *p, int64_t n, const uint8_t *ref, int64_t ref_bytes, const uint8_t *qer, int64_t qer_bytes,
                        const int64_t *idr, const int64_t *idq, const int32_t *len1, const int32_t *len2, const int32_t *h0,
                        const gbx_bsw_result *out)
{
    if (!p || n <= 0 || !ref || !qer || !idr || !idq || !len1 || !len2 || !h0 || !out || ref_bytes < 0 || qer_bytes < 0) return false;
    return !any_bad_unit(n, host_workers(BSW_HOST_WORKERS), [&](int64_t j) {
        return bsw_pair_fault(idr[j], idq[j], len1[j], len2[j], ref_bytes, qer_bytes) != BSW_PAIR_OK;
    });
}

// The host entry: one device, or the pairs cut into contiguous ranges of equal nominal cells (len1 x len2, the reference's
// own cell count, main_banded.cpp:183,323) over the devices of gbx_host_set_devices / GBX_GPUS - the reference's per-thread
// slices (main_banded.cpp:279-291) as per-device slices.  Each shard's bases are the byte range of the arenas its pairs
// span, sent by that device's own lane; results are written in place.
static int bsw_host_entry(const gbx_bsw_params *p, int64_t n,
                          const uint8_t *ref, int64_t ref_bytes,
                          const uint8_t *qer, int64_t qer_bytes,
                          const int64_t *idr, const int64_t *idq,
                          const int32_t *len1, const int32_t *len2,
                          const int32_t *h0, gbx_bsw_result *out)
{
    auto one = [&] { return bsw_host_one(p, n, ref, ref_bytes, qer, qer_bytes, idr, idq, len1, len2, h0, out); };
    if (!host_multi_wanted() || !bsw_call_ok(p, n, ref, ref_bytes, qer, qer_bytes, idr, idq, len1, len2, h0, out)) return one();
    return spread_over_devices("gbx_bsw_extend_host", n, n, 131072,
        [&](int64_t k) { return len1[k] > 0 && len2[k] > 0 ? (double)len1[k] * (double)len2[k] : 0.0; }, one,
        [&](int, int64_t lo, int64_t hi) {
            const Span r = span_of(idr, len1, lo, hi), q = span_of(idq, len2, lo, hi);
            const std::vector<int64_t> r2 = rebased(idr, lo, hi, r.a0), q2 = rebased(idq, lo, hi, q.a0);
            return bsw_host_one(p, hi - lo, ref + r.a0, r.a1 - r.a0, qer + q.a0, q.a1 - q.a0, r2.data(), q2.data(), len1 + lo, len2 + lo,
                                h0 + lo, out + lo, lo);
        });
}

}  // extern "C"

// ---- small concurrent calls combined (host_combine.h).  The reference's driver calls getScores16 once per 512 pairs from
// every OpenMP thread (main_banded.cpp:279-291): the calls that are pending together become one job - the pairs of all
// requests end to end, their bases gathered into two compact arenas (4-byte aligned per pair, as the SeqPair entry does for
// the driver's strided slots) - and every caller gets its own slice of the results.
namespace {
constexpr int64_t BSW_COMBINE_MAX_CALL = 65536, BSW_COMBINE_MAX_JOB = (int64_t)1 << 20;
struct BswReq : CombineReq {
    const gbx_bsw_params *p; int64_t n;
    const uint8_t *ref; int64_t ref_bytes; const uint8_t *qer; int64_t qer_bytes;
    const int64_t *idr, *idq; const int32_t *len1, *len2, *h0; gbx_bsw_result *out;
    int64_t cr, cq;                       // bytes of its pairs in the compact arenas
    struct Scratch { gbx::Scratch<uint8_t> ref, qer; gbx::Scratch<int64_t> idr, idq; gbx::Scratch<int32_t> l1, l2, h0; gbx::Scratch<gbx_bsw_result> out; };

    int run() const { return bsw_host_entry(p, n, ref, ref_bytes, qer, qer_bytes, idr, idq, len1, len2, h0, out); }
    static bool same(const BswReq &a, const BswReq &b) { return memcmp(a.p, b.p, offsetof(gbx_bsw_params, pad_)) == 0; }
    static int combined(const std::vector<BswReq *> &batch, Scratch &S)
    {
        const size_t nb = batch.size();
        std::vector<int64_t> p0(nb + 1, 0), r0(nb + 1, 0), q0(nb + 1, 0);
        for (size_t k = 0; k < nb; ++k) { p0[k + 1] = p0[k] + batch[k]->n; r0[k + 1] = r0[k] + batch[k]->cr; q0[k + 1] = q0[k] + batch[k]->cq; }
        const int64_t N = p0[nb], R = r0[nb], Q = q0[nb];
        uint8_t *mref = S.ref.get((size_t)R + 16), *mqer = S.qer.get((size_t)Q + 16);
        int64_t *midr = S.idr.get((size_t)N), *midq = S.idq.get((size_t)N);
        int32_t *ml1 = S.l1.get((size_t)N), *ml2 = S.l2.get((size_t)N), *mh0 = S.h0.get((size_t)N);
        gbx_bsw_result *mout = S.out.get((size_t)N);
        combine_parallel((int64_t)nb, host_workers(), [&](int64_t k) {
            const BswReq *r = batch[(size_t)k];
            int64_t pr = r0[(size_t)k], pq = q0[(size_t)k];
            const int64_t a = p0[(size_t)k];
            for (int64_t j = 0; j < r->n; ++j) {
                memcpy(mref + pr, r->ref + r->idr[j], (size_t)r->len1[j]);
                memcpy(mqer + pq, r->qer + r->idq[j], (size_t)r->len2[j]);
                midr[a + j] = pr; midq[a + j] = pq;
                pr += (r->len1[j] + 3) & ~3; pq += (r->len2[j] + 3) & ~3;
            }
            memcpy(ml1 + a, r->len1, (size_t)r->n * 4); memcpy(ml2 + a, r->len2, (size_t)r->n * 4); memcpy(mh0 + a, r->h0, (size_t)r->n * 4);
        });
        const int rc = bsw_host_entry(batch[0]->p, N, mref, R + 8, mqer, Q + 8, midr, midq, ml1, ml2, mh0, mout);
        if (rc) return rc;
        combine_parallel((int64_t)nb, nb >= 8 ? 4 : 1, [&](int64_t k) {
            BswReq *r = batch[(size_t)k];
            memcpy(r->out, mout + p0[(size_t)k], (size_t)r->n * sizeof(gbx_bsw_result));
            r->rc = GBX_OK;
        });
        return GBX_OK;
    }
};
}
namespace gbx { Combiner &combiner_bsw() { static Combiner *c = new Combiner(); return *c; } }

extern "C" {

int gbx_bsw_extend_host(const gbx_bsw_params *p, int64_t n,
                        const uint8_t *ref, int64_t ref_bytes,
                        const uint8_t *qer, int64_t qer_bytes,
                        const int64_t *idr, const int64_t *idq,
                        const int32_t *len1, const int32_t *len2,
                        const int32_t *h0, gbx_bsw_result *out)
{
    BswReq r;
    r.p = p; r.n = n; r.ref = ref; r.ref_bytes = ref_bytes; r.qer = qer; r.qer_bytes = qer_bytes;
    r.idr = idr; r.idq = idq; r.len1 = len1; r.len2 = len2; r.h0 = h0; r.out = out; r.units = n; r.cr = r.cq = 0;
    // a call with a bad pair goes its own way: its error names the pair
    if (n > BSW_COMBINE_MAX_CALL || !bsw_call_ok(p, n, ref, ref_bytes, qer, qer_bytes, idr, idq, len1, len2, h0, out)) return r.run();
    for (int64_t k = 0; k < n; ++k) { r.cr += (len1[k] + 3) & ~3; r.cq += (len2[k] + 3) & ~3; }
    return combine_call(combiner_bsw(), r, BSW_COMBINE_MAX_JOB, 1);
}

int gbx_bsw_extend_seqpairs(const gbx_bsw_params *p, gbx_seqpair *pairs, int64_t n,
                            const uint8_t *ref, int64_t ref_bytes,
                            const uint8_t *qer, int64_t qer_bytes)
{
    RoctxRange range_("gbx_bsw_extend_seqpairs");
    if (!p || n < 0) { set_error("gbx_bsw_extend_seqpairs: bad argument"); return GBX_ERR_ARG; }
    if (n == 0) return GBX_OK;
    if (!pairs) { set_error("gbx_bsw_extend_seqpairs: null pointer"); return GBX_ERR_ARG; }
    if (!ref || !qer || ref_bytes < 0 || qer_bytes < 0) { set_error("gbx_bsw_extend_seqpairs: bad arena"); return GBX_ERR_ARG; }
    // The reference's driver gives every pair a fixed-stride slot in the two buffers (MAX_SEQ_LEN_REF / _QER bytes,
    // main_banded.cpp:56-58,160-172), so the arenas are mostly holes: 2 M pairs span 4.6 GB for 0.6 GB of bases.
    // The flat arrays are extracted with a few threads, and when the layout is that sparse the bases are gathered
    // into packed arenas first instead of sending the holes over PCIe.
    const int T = host_workers(BSW_HOST_WORKERS);
    std::vector<int64_t> idr(n), idq(n);
    std::vector<int32_t> l1(n), l2(n), h0(n);
    std::vector<gbx_bsw_result> out(n);
    std::vector<int64_t> part_r((size_t)T + 1, 0), part_q((size_t)T + 1, 0), part_bad((size_t)T, -1);
    parallel_ranges(n, T, [&](int t, int64_t lo, int64_t hi) {
        int64_t sr = 0, sq = 0;
        for (int64_t k = lo; k < hi; ++k) {
            const gbx_seqpair &sp = pairs[k];
            // (a pair over GBX_BSW_MAX_QLEN/TLEN goes on: the host entry below names it)
            if (bsw_pair_fault(sp.idr, sp.idq, sp.len1, sp.len2, ref_bytes, qer_bytes) == BSW_PAIR_OUTSIDE) { part_bad[(size_t)t] = k; return; }
            idr[k] = sp.idr; idq[k] = sp.idq; l1[k] = sp.len1; l2[k] = sp.len2; h0[k] = sp.h0;
            sr += (sp.len1 + 3) & ~3; sq += (sp.len2 + 3) & ~3;
        }
        part_r[(size_t)t + 1] = sr; part_q[(size_t)t + 1] = sq;
    });
    for (int t = 0; t < T; ++t)
        if (part_bad[(size_t)t] >= 0) {
            set_error("gbx_bsw_extend_seqpairs: pair %lld lies outside the arenas", (long long)part_bad[(size_t)t]);
            return GBX_ERR_ARG;
        }
    for (int t = 0; t < T; ++t) { part_r[(size_t)t + 1] += part_r[(size_t)t]; part_q[(size_t)t + 1] += part_q[(size_t)t]; }
    const int64_t packed_r = part_r[(size_t)T], packed_q = part_q[(size_t)T];
    std::vector<uint8_t> cref, cqer;
    // (small calls too: the driver's 512-pair batch spans 1.1 MB of slots for 180 KB of bases, and a call that size is mostly the
    // copy into the pinned slab and the DMA)
    const bool sparse = (ref_bytes + qer_bytes) > 2 * (packed_r + packed_q) + ((int64_t)64 << 10);
    if (sparse) {
        cref.resize((size_t)packed_r + 8); cqer.resize((size_t)packed_q + 8);
        // same thread ranges as above, so every thread knows where its pairs start in the packed arenas
        parallel_ranges(n, T, [&](int t, int64_t lo, int64_t hi) {
            int64_t pr = part_r[(size_t)t], pq = part_q[(size_t)t];
            for (int64_t k = lo; k < hi; ++k) {
                memcpy(&cref[(size_t)pr], ref + idr[k], (size_t)l1[k]);
                memcpy(&cqer[(size_t)pq], qer + idq[k], (size_t)l2[k]);
                idr[k] = pr; idq[k] = pq;
                pr += (l1[k] + 3) & ~3; pq += (l2[k] + 3) & ~3;
            }
        });
        ref = cref.data(); ref_bytes = packed_r + 8; qer = cqer.data(); qer_bytes = packed_q + 8;
    }
    int rc = gbx_bsw_extend_host(p, n, ref, ref_bytes, qer, qer_bytes, idr.data(), idq.data(), l1.data(),
                                 l2.data(), h0.data(), out.data());
    if (rc) return rc;
    parallel_ranges(n, T, [&](int, int64_t lo, int64_t hi) {
        for (int64_t k = lo; k < hi; ++k) {
            pairs[k].score = out[k].score; pairs[k].tle = out[k].tle; pairs[k].gtle = out[k].gtle;
            pairs[k].qle = out[k].qle; pairs[k].gscore = out[k].gscore; pairs[k].max_off = out[k].max_off;
        }
    });
    return GBX_OK;
}


}  // extern "C"
