// capi_dbg.hip — Platypus de Bruijn graph entries of the C-ABI (include/gbx.h, dbg section).
#include "capi_common.h"
#include "dbg_host.h"

using namespace gbx;

namespace {

// A batch's tables: at most this much device memory, or one window's if that alone is more (dbg_window_bytes).
constexpr size_t DBG_TABLE_BYTES = (size_t)2 << 30;

// Windows [lo, hi) on the current device from host arrays: their reads and references uploaded (rebased), planned, run.
// stats: the windows' stats (index w - lo); nodes / edges, when given, with node_off / edge_off[hi - lo + 1] of the caller
// rebased to this range (first_edge is moved back by edge_base afterwards).
int dbg_run_host_range(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, const std::vector<int64_t> &rcp, int64_t lo,
                       int64_t hi, gbx_dbg_stats *stats, const int64_t *node_off, const int64_t *edge_off, gbx_dbg_node *nodes,
                       gbx_dbg_edge *edges, const char *who)
{
    const int64_t m = hi - lo;
    if (m <= 0) return GBX_OK;
    int64_t ra = R->n_reads, rb = 0;
    for (int64_t w = lo; w < hi; ++w)
        if (W->read_lo[w] < W->read_hi[w]) { ra = std::min(ra, W->read_lo[w]); rb = std::max(rb, W->read_hi[w]); }
    if (rb < ra) ra = rb = 0;
    const int64_t nr = rb - ra, b0 = R->seq_off[ra], b1 = R->seq_off[rb], f0 = W->ref_off[lo], f1 = W->ref_off[hi];
    std::vector<int64_t> soff((size_t)nr + 1), rp((size_t)nr + 1), roff((size_t)m + 1), rlo((size_t)m), rhi((size_t)m);
    for (int64_t j = 0; j <= nr; ++j) { soff[(size_t)j] = R->seq_off[ra + j] - b0; rp[(size_t)j] = rcp[(size_t)(ra + j)] - rcp[(size_t)ra]; }
    for (int64_t j = 0; j <= m; ++j) roff[(size_t)j] = W->ref_off[lo + j] - f0;
    for (int64_t j = 0; j < m; ++j) {
        const bool any = W->read_lo[lo + j] < W->read_hi[lo + j];
        rlo[(size_t)j] = any ? W->read_lo[lo + j] - ra : 0;
        rhi[(size_t)j] = any ? W->read_hi[lo + j] - ra : 0;
    }
    std::vector<DbgWinPlan> plan;
    std::vector<int64_t> batches;
    size_t need = 0, biggest = 0;
    for (int64_t j = 0; j < m; ++j) {
        const int64_t C = std::max<int64_t>(0, roff[(size_t)j + 1] - roff[(size_t)j] - p->k - 1) + rp[(size_t)rhi[(size_t)j]] - rp[(size_t)rlo[(size_t)j]];
        const size_t b = dbg_window_bytes(C);
        need += b;
        biggest = std::max(biggest, b);
    }
    const size_t table = std::max(biggest, std::min(need, DBG_TABLE_BYTES));
    int rc = dbg_plan(p->k, 0, m, roff.data(), W->ref_pos + lo, rlo.data(), rhi.data(), rp.data(), table, plan, batches);
    if (rc) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    DevBuf dref(L), dseq(L), dqual(L), dsoff(L), drcp(L), dflag(L), dplan(L), derr(L), dreg(L), dst(L), dnoff(L), deoff(L), dnodes(L), dedges(L);
    if ((rc = dref.alloc((size_t)(f1 - f0) + 128)) || (rc = dseq.alloc((size_t)(b1 - b0) + 128)) || (rc = dqual.alloc((size_t)(b1 - b0) + 128)) ||
        (rc = dsoff.alloc((size_t)(nr + 1) * 8)) || (rc = drcp.alloc((size_t)(nr + 1) * 8)) || (rc = dflag.alloc((size_t)nr * 2 + 8)) ||
        (rc = dplan.alloc(plan.size() * sizeof(DbgWinPlan))) || (rc = derr.alloc(8)) || (rc = dreg.alloc(table)) ||
        (rc = dst.alloc((size_t)m * sizeof(gbx_dbg_stats))))
        return rc;
    if (f1 > f0) GBX_HIP(hipMemcpyAsync(dref.p, W->ref + f0, (size_t)(f1 - f0), hipMemcpyHostToDevice, s));
    if (b1 > b0) {
        GBX_HIP(hipMemcpyAsync(dseq.p, R->seq + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, s));
        GBX_HIP(hipMemcpyAsync(dqual.p, R->qual + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, s));
    }
    GBX_HIP(hipMemcpyAsync(dsoff.p, soff.data(), (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(drcp.p, rp.data(), (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, s));
    if (nr > 0) GBX_HIP(hipMemcpyAsync(dflag.p, R->flag + ra, (size_t)nr * 2, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemsetAsync(derr.p, 0, 8, s));
    DbgDev a;
    a.k = p->k; a.min_qual = p->min_qual; a.ref_bytes = f1 - f0;
    a.ref = dref.as<uint8_t>(); a.seq = dseq.as<uint8_t>(); a.qual = dqual.as<uint8_t>();
    a.seq_off = dsoff.as<int64_t>(); a.rcp = drcp.as<int64_t>(); a.flag = dflag.as<uint16_t>();
    DbgGraphOut g;
    std::vector<int64_t> noff, eoff;
    if (nodes) {
        noff.resize((size_t)m + 1); eoff.resize((size_t)m + 1);
        for (int64_t j = 0; j <= m; ++j) { noff[(size_t)j] = node_off[j] - node_off[0]; eoff[(size_t)j] = edge_off[j] - edge_off[0]; }
        if ((rc = dnoff.alloc((size_t)(m + 1) * 8)) || (rc = deoff.alloc((size_t)(m + 1) * 8)) ||
            (rc = dnodes.alloc((size_t)noff[(size_t)m] * sizeof(gbx_dbg_node))) || (rc = dedges.alloc((size_t)eoff[(size_t)m] * sizeof(gbx_dbg_edge))))
            return rc;
        GBX_HIP(hipMemcpyAsync(dnoff.p, noff.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
        GBX_HIP(hipMemcpyAsync(deoff.p, eoff.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
        g.nodes = dnodes.as<gbx_dbg_node>(); g.edges = dedges.as<gbx_dbg_edge>();
        g.node_off = dnoff.as<int64_t>(); g.edge_off = deoff.as<int64_t>();
        g.ref_shift = f0; g.seq_shift = b0;
    }
    if ((rc = dbg_launch(a, plan, batches, dplan.as<DbgWinPlan>(), derr.as<int>(), dreg.as<char>(), dst.as<gbx_dbg_stats>(), g, s))) return rc;
    int err = 0;
    std::vector<gbx_dbg_stats> st((size_t)m);
    GBX_HIP(hipMemcpyAsync(&err, derr.p, 4, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(st.data(), dst.p, (size_t)m * sizeof(gbx_dbg_stats), hipMemcpyDeviceToHost, s));
    if (nodes) {
        if (noff[(size_t)m]) GBX_HIP(hipMemcpyAsync(nodes, dnodes.p, (size_t)noff[(size_t)m] * sizeof(gbx_dbg_node), hipMemcpyDeviceToHost, s));
        if (eoff[(size_t)m]) GBX_HIP(hipMemcpyAsync(edges, dedges.p, (size_t)eoff[(size_t)m] * sizeof(gbx_dbg_edge), hipMemcpyDeviceToHost, s));
    }
    GBX_HIP(hipStreamSynchronize(s));
    if (err) { set_error("%s: a window's table filled (%d): cannot happen by its sizing", who, err); return GBX_ERR_HIP; }
    if (stats) memcpy(stats, st.data(), (size_t)m * sizeof(gbx_dbg_stats));
    if (nodes) {
        for (int64_t j = 0; j < m; ++j)
            if (noff[(size_t)j + 1] - noff[(size_t)j] != st[(size_t)j].n_nodes || eoff[(size_t)j + 1] - eoff[(size_t)j] != st[(size_t)j].n_edges) {
                set_error("%s: window %lld has %lld nodes and %lld edges, node_off / edge_off give room for %lld and %lld", who, (long long)(lo + j),
                          (long long)st[(size_t)j].n_nodes, (long long)st[(size_t)j].n_edges, (long long)(noff[(size_t)j + 1] - noff[(size_t)j]),
                          (long long)(eoff[(size_t)j + 1] - eoff[(size_t)j]));
                return GBX_ERR_ARG;
            }
        for (int64_t x = 0; x < noff[(size_t)m]; ++x) nodes[x].first_edge += edge_off[0];
    }
    return GBX_OK;
}

int dbg_host(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, int64_t w0, int64_t w1, gbx_dbg_stats *stats,
             const int64_t *node_off, const int64_t *edge_off, gbx_dbg_node *nodes, gbx_dbg_edge *edges, const char *who)
{
    const std::vector<int64_t> rcp = dbg_read_prefix(p->k, R->n_reads, R->seq_off);
    auto cost = [&](int64_t j) {
        const int64_t w = w0 + j;
        return (double)(std::max<int64_t>(0, W->ref_off[w + 1] - W->ref_off[w] - p->k - 1) + rcp[(size_t)W->read_hi[w]] - rcp[(size_t)W->read_lo[w]] + 1);
    };
    auto range = [&](int64_t lo, int64_t hi) -> int {
        return dbg_run_host_range(p, R, W, rcp, w0 + lo, w0 + hi, stats ? stats + lo : nullptr, nodes ? node_off + lo : nullptr,
                                  nodes ? edge_off + lo : nullptr, nodes ? nodes + node_off[lo] : nullptr,
                                  nodes ? edges + edge_off[lo] : nullptr, who);
    };
    const int64_t n = w1 - w0;
    return spread_over_devices(who, n, n, 64, cost, [&]() { return range(0, n); }, [&](int, int64_t lo, int64_t hi) { return range(lo, hi); });
}

// The device entries' plan: the offsets and ranges read back (stream synchronised), the read prefix uploaded into the workspace.
struct DevWork {
    int64_t *rcp;
    DbgWinPlan *plan;
    int *err;
    char *region;
    size_t table;
};
size_t dev_head_bytes(int64_t n_win, int64_t n_reads)
{
    return align256((size_t)(n_reads + 1) * 8) + align256((size_t)std::max<int64_t>(n_win, 1) * sizeof(DbgWinPlan)) + 256;
}

int dbg_device(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, int64_t w0, int64_t w1, gbx_dbg_stats *d_stats,
               const DbgGraphOut &g, void *d_work, size_t work_bytes, hipStream_t s, const char *who)
{
    int rc = dbg_params_check(p, who);
    if (rc) return rc;
    if (!R || !W || R->n_reads < 0 || W->n_win < 0 || R->seq_bytes < 0 || W->ref_bytes < 0 || !R->seq_off || !W->ref_off || !d_work ||
        (W->n_win > 0 && (!W->ref_pos || !W->read_lo || !W->read_hi)) || (R->n_reads > 0 && !R->flag) ||
        (R->seq_bytes > 0 && (!R->seq || !R->qual)) || (W->ref_bytes > 0 && !W->ref)) {
        set_error("%s: null pointer or negative size", who);
        return GBX_ERR_ARG;
    }
    if (W->ref_bytes + R->seq_bytes >= ((int64_t)1 << 40)) { set_error("%s: more than 2^40 bytes of reference and reads", who); return GBX_ERR_UNSUPPORTED; }
    if (w0 < 0 || w1 < w0 || w1 > W->n_win) { set_error("%s: windows [%lld, %lld) of %lld", who, (long long)w0, (long long)w1, (long long)W->n_win); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    const int64_t n = R->n_reads, nw = W->n_win;
    const size_t head = dev_head_bytes(nw, n);
    if (work_bytes < head) { set_error("%s: workspace of %zu bytes, at least %zu needed", who, work_bytes, head); return GBX_ERR_ARG; }
    std::vector<int64_t> soff((size_t)n + 1), roff((size_t)nw + 1), rpos((size_t)nw), rlo((size_t)nw), rhi((size_t)nw);
    GBX_HIP(hipMemcpyAsync(soff.data(), R->seq_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(roff.data(), W->ref_off, (size_t)(nw + 1) * 8, hipMemcpyDeviceToHost, s));
    if (nw > 0) {
        GBX_HIP(hipMemcpyAsync(rpos.data(), W->ref_pos, (size_t)nw * 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(rlo.data(), W->read_lo, (size_t)nw * 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(rhi.data(), W->read_hi, (size_t)nw * 8, hipMemcpyDeviceToHost, s));
    }
    GBX_HIP(hipStreamSynchronize(s));
    for (int64_t w = 0; w < nw; ++w)
        if (rlo[(size_t)w] < 0 || rlo[(size_t)w] > rhi[(size_t)w] || rhi[(size_t)w] > n || roff[(size_t)w + 1] < roff[(size_t)w] ||
            roff[(size_t)w] < 0 || roff[(size_t)w + 1] > W->ref_bytes || rpos[(size_t)w] < 0 ||
            rpos[(size_t)w] + (roff[(size_t)w + 1] - roff[(size_t)w]) > INT32_MAX) {
            set_error("%s: window %lld: bad read range, reference offsets or a reference outside [0, 2^31)", who, (long long)w);
            return GBX_ERR_ARG;
        }
    for (int64_t r = 0; r < n; ++r)
        if (soff[(size_t)r + 1] < soff[(size_t)r] || soff[(size_t)r] < 0 || soff[(size_t)r + 1] > R->seq_bytes) {
            set_error("%s: read %lld: bad seq_off", who, (long long)r);
            return GBX_ERR_ARG;
        }
    const std::vector<int64_t> rcp = dbg_read_prefix(p->k, n, soff.data());
    char *w = (char *)d_work;
    DevWork D;
    D.rcp = (int64_t *)w; w += align256((size_t)(n + 1) * 8);
    D.plan = (DbgWinPlan *)w; w += align256((size_t)std::max<int64_t>(nw, 1) * sizeof(DbgWinPlan));
    D.err = (int *)w; w += 256;
    D.region = w;
    D.table = work_bytes - head;
    std::vector<DbgWinPlan> plan;
    std::vector<int64_t> batches;
    if ((rc = dbg_plan(p->k, w0, w1, roff.data(), rpos.data(), rlo.data(), rhi.data(), rcp.data(), D.table, plan, batches))) return rc;
    GBX_HIP(hipMemcpyAsync(D.rcp, rcp.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemsetAsync(D.err, 0, 4, s));
    DbgDev a;
    a.k = p->k; a.min_qual = p->min_qual; a.ref_bytes = W->ref_bytes;
    a.ref = W->ref; a.seq = R->seq; a.qual = R->qual; a.seq_off = R->seq_off; a.rcp = D.rcp; a.flag = R->flag;
    rc = dbg_launch(a, plan, batches, D.plan, D.err, D.region, d_stats, g, s);
    // the host vectors above were read by asynchronous copies: they must live until the copies are done
    GBX_HIP(hipStreamSynchronize(s));
    return rc;
}

}  // namespace

extern "C" {

void gbx_dbg_default_params(gbx_dbg_params *p)
{
    if (!p) return;
    p->k = 15; p->min_qual = 20; p->region_size = 1500; p->pad_ = 0;
}

int gbx_dbg_windows(const gbx_dbg_params *p, const gbx_dbg_reads *R, int64_t beg, int64_t end, int64_t cap, int64_t *n_win, int64_t *assem_start,
                    int64_t *assem_end, int64_t *ref_start, int64_t *ref_end, int64_t *read_lo, int64_t *read_hi)
{
    const char *who = "gbx_dbg_windows";
    int rc = dbg_params_check(p, who);
    if (rc) return rc;
    if (!R || !n_win || R->n_reads < 0 || (R->n_reads > 0 && (!R->pos || !R->end)) || beg < 0 || end > INT32_MAX || cap < 0) {
        set_error("%s: null pointer, negative size or region [%lld, %lld) outside [0, 2^31)", who, (long long)beg, (long long)end);
        return GBX_ERR_ARG;
    }
    const int64_t n = R->n_reads;
    const int32_t size = p->region_size, shift = std::max(100, std::min(1000, size / 2));
    int32_t longest = 0;
    for (int64_t r = 0; r < n; ++r) longest = std::max(longest, (int32_t)(uint32_t)(R->end[r] - R->pos[r]));
    auto bisect = [&](uint32_t x) {          // bisect_left over the reads' pos, unsigned
        int64_t a = 0, b = n;
        while (a < b) {
            const int64_t mid = (a + b) / 2;
            if (R->pos[mid] < x) a = mid + 1; else b = mid;
        }
        return a;
    };
    int64_t w = 0;
    for (int64_t k = beg; k < end; k += shift, ++w) {
        const int64_t a0 = k, a1 = std::min<int64_t>(k + size, end), f0 = std::max<int64_t>(0, k - size), f1 = a1 + size;
        int64_t lo = 0, hi = 0;
        if (n > 0) {
            const int32_t first = (int32_t)std::max<int64_t>(1, (int64_t)(int32_t)((uint32_t)a0 - (uint32_t)longest));
            lo = bisect((uint32_t)first);
            hi = bisect((uint32_t)a1);
            while (lo < n && R->end[lo] <= (uint32_t)a0) ++lo;
        }
        if (w < cap) {
            if (assem_start) assem_start[w] = a0;
            if (assem_end) assem_end[w] = a1;
            if (ref_start) ref_start[w] = f0;
            if (ref_end) ref_end[w] = f1;
            if (read_lo) read_lo[w] = lo;
            if (read_hi) read_hi[w] = lo > hi ? hi : std::min(hi, n);
        }
        if (lo > hi) {
            *n_win = w + 1;
            set_error("%s: window %lld at %lld: read start %lld > read end %lld (the reference's fatal error)", who, (long long)w, (long long)a0, (long long)lo,
                      (long long)hi);
            return GBX_ERR_ARG;
        }
    }
    *n_win = w;
    return GBX_OK;
}

size_t gbx_dbg_workspace_bytes(const gbx_dbg_params *p, int64_t n_win, int64_t n_reads, int64_t max_window_occ)
{
    if (!p || n_win < 0 || n_reads < 0 || max_window_occ < 0) return 0;
    const size_t one = dbg_window_bytes(max_window_occ);
    const size_t all = n_win > 0 && one > ((size_t)-1) / (size_t)n_win ? (size_t)-1 : one * (size_t)std::max<int64_t>(n_win, 1);
    return dev_head_bytes(n_win, n_reads) + std::max(one, std::min(all, DBG_TABLE_BYTES));
}

int gbx_dbg_build_device(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, gbx_dbg_stats *d_stats, void *d_work,
                         size_t work_bytes, void *stream)
{
    if (!d_stats) { set_error("gbx_dbg_build_device: null stats"); return GBX_ERR_ARG; }
    return dbg_device(p, reads, wins, 0, wins ? wins->n_win : 0, d_stats, DbgGraphOut(), d_work, work_bytes, (hipStream_t)stream,
                      "gbx_dbg_build_device");
}

int gbx_dbg_graph_device(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, int64_t w0, int64_t w1,
                         const int64_t *d_node_off, const int64_t *d_edge_off, gbx_dbg_node *d_nodes, gbx_dbg_edge *d_edges, void *d_work,
                         size_t work_bytes, void *stream)
{
    if (!d_node_off || !d_edge_off || !d_nodes || !d_edges) { set_error("gbx_dbg_graph_device: null output"); return GBX_ERR_ARG; }
    DbgGraphOut g;
    g.nodes = d_nodes; g.edges = d_edges; g.node_off = d_node_off; g.edge_off = d_edge_off;
    return dbg_device(p, reads, wins, w0, w1, nullptr, g, d_work, work_bytes, (hipStream_t)stream, "gbx_dbg_graph_device");
}

int gbx_dbg_build_host(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, gbx_dbg_stats *stats)
{
    RoctxRange range_("gbx_dbg_build_host");
    const char *who = "gbx_dbg_build_host";
    int rc = dbg_check(p, reads, wins, who);
    if (rc) return rc;
    if (!stats) { set_error("%s: null stats", who); return GBX_ERR_ARG; }
    if (wins->n_win == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    return dbg_host(p, reads, wins, 0, wins->n_win, stats, nullptr, nullptr, nullptr, nullptr, who);
}

int gbx_dbg_graph_host(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, int64_t w0, int64_t w1,
                       const int64_t *node_off, const int64_t *edge_off, gbx_dbg_node *nodes, gbx_dbg_edge *edges)
{
    RoctxRange range_("gbx_dbg_graph_host");
    const char *who = "gbx_dbg_graph_host";
    int rc = dbg_check(p, reads, wins, who);
    if (rc) return rc;
    if (w0 < 0 || w1 < w0 || w1 > wins->n_win) { set_error("%s: windows [%lld, %lld) of %lld", who, (long long)w0, (long long)w1, (long long)wins->n_win); return GBX_ERR_ARG; }
    if (!node_off || !edge_off) { set_error("%s: null node_off / edge_off", who); return GBX_ERR_ARG; }
    for (int64_t j = 0; j < w1 - w0; ++j)
        if (node_off[j + 1] < node_off[j] || edge_off[j + 1] < edge_off[j] || node_off[j] < 0 || edge_off[j] < 0) {
            set_error("%s: node_off / edge_off decrease at window %lld", who, (long long)(w0 + j));
            return GBX_ERR_ARG;
        }
    if ((node_off[w1 - w0] > node_off[0] && !nodes) || (edge_off[w1 - w0] > edge_off[0] && !edges)) { set_error("%s: null output", who); return GBX_ERR_ARG; }
    if (w1 == w0) return GBX_OK;
    if ((rc = require_device())) return rc;
    gbx_dbg_node dummy_n;
    gbx_dbg_edge dummy_e;
    return dbg_host(p, reads, wins, w0, w1, nullptr, node_off, edge_off, nodes ? nodes : &dummy_n, edges ? edges : &dummy_e, who);
}

}  // extern "C"
