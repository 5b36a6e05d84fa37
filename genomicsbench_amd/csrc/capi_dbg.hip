// capi_dbg.hip — Platypus de Bruijn graph entries of the C-ABI (include/gbx.h, dbg section).
#include "capi_common.h"
#include "dbg_host.h"

using namespace gbx;

namespace {

// Windows [w0, w1) of H cut into batches for a table region of `table` bytes; a window that does not fit alone is refused.
int cut_batches(int k, int64_t w0, int64_t w1, const DbgHostArrays &H, const int64_t *rcp, size_t table, std::vector<DbgWinPlan> &plan,
                std::vector<int64_t> &batches)
{
    const int64_t bad = dbg_cut_batches(k, w0, w1, H, rcp, table, plan, batches);
    if (bad < 0) return GBX_OK;
    set_error("dbg: window %lld needs %zu bytes of tables, the workspace has %zu (gbx_dbg_workspace_bytes: max_window_occ)", (long long)bad,
              dbg_window_bytes(dbg_win_plan(k, bad, H, rcp).C), table);
    return GBX_ERR_ARG;
}

// Windows [lo, hi) on the current device from host arrays: their reads and references uploaded (rebased), planned, run.
// stats: the windows' stats (index w - lo); nodes / edges, when given, with node_off / edge_off[hi - lo + 1] of the caller
// rebased to this range (first_edge is moved back by edge_base afterwards).
int dbg_run_host_range(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, int64_t lo, int64_t hi, gbx_dbg_stats *stats,
                       const int64_t *node_off, const int64_t *edge_off, gbx_dbg_node *nodes, gbx_dbg_edge *edges, const char *who)
{
    const int64_t m = hi - lo;
    if (m <= 0) return GBX_OK;
    int64_t ra = R->n_reads, rb = 0;
    for (int64_t w = lo; w < hi; ++w)
        if (W->read_lo[w] < W->read_hi[w]) { ra = std::min(ra, W->read_lo[w]); rb = std::max(rb, W->read_hi[w]); }
    if (rb < ra) ra = rb = 0;
    HostLane lane;
    int rc = lane.acquire();
    if (rc) return rc;
    Lane *L = lane.l; hipStream_t s = L->compute;
    DbgUpload U(L);
    DevBuf drcp(L), dplan(L), derr(L), dreg(L), dst(L), dnoff(L), deoff(L), dnodes(L), dedges(L);
    std::vector<int64_t> rcp, batches, noff, eoff;
    std::vector<DbgWinPlan> plan;
    std::vector<gbx_dbg_stats> st((size_t)m);
    StreamDrain drain{s};                            // the host arrays above outlive the queued copies
    if ((rc = U.up(R, W, ra, rb, lo, hi, s))) return rc;
    const DbgHostArrays &H = U.h;
    rcp = dbg_read_prefix(p->k, U.R.n_reads, H.seq_off.data());
    size_t need = 0, biggest = 0;
    for (int64_t j = 0; j < m; ++j) {
        const size_t b = dbg_window_bytes(dbg_win_plan(p->k, j, H, rcp.data()).C);
        need += b;
        biggest = std::max(biggest, b);
    }
    const size_t table = dbg_area_bytes(biggest, need);
    if ((rc = cut_batches(p->k, 0, m, H, rcp.data(), table, plan, batches))) return rc;
    if ((rc = upload(drcp, rcp.data(), rcp.size() * 8, s)) || (rc = dplan.alloc(plan.size() * sizeof(DbgWinPlan))) || (rc = derr.alloc(8)) ||
        (rc = dreg.alloc(table)) || (rc = dst.alloc((size_t)m * sizeof(gbx_dbg_stats))))
        return rc;
    GBX_HIP(hipMemsetAsync(derr.p, 0, 8, s));
    DbgGraphOut g;
    if (nodes) {
        noff.resize((size_t)m + 1); eoff.resize((size_t)m + 1);
        for (int64_t j = 0; j <= m; ++j) { noff[(size_t)j] = node_off[j] - node_off[0]; eoff[(size_t)j] = edge_off[j] - edge_off[0]; }
        if ((rc = upload(dnoff, noff.data(), (size_t)(m + 1) * 8, s)) || (rc = upload(deoff, eoff.data(), (size_t)(m + 1) * 8, s)) ||
            (rc = dnodes.alloc((size_t)noff[(size_t)m] * sizeof(gbx_dbg_node))) || (rc = dedges.alloc((size_t)eoff[(size_t)m] * sizeof(gbx_dbg_edge))))
            return rc;
        g.nodes = dnodes.as<gbx_dbg_node>(); g.edges = dedges.as<gbx_dbg_edge>();
        g.node_off = dnoff.as<int64_t>(); g.edge_off = deoff.as<int64_t>();
        g.ref_shift = W->ref_off[lo]; g.seq_shift = R->seq_off[ra];
    }
    if ((rc = dbg_launch(dbg_dev(p->k, p, &U.R, &U.W, drcp.as<int64_t>()), plan, batches, dplan.as<DbgWinPlan>(), derr.as<int>(), dreg.as<char>(),
                         dst.as<gbx_dbg_stats>(), g, s)))
        return rc;
    GBX_HIP(hipMemcpyAsync(st.data(), dst.p, (size_t)m * sizeof(gbx_dbg_stats), hipMemcpyDeviceToHost, s));
    if (nodes) {
        if (noff[(size_t)m]) GBX_HIP(hipMemcpyAsync(nodes, dnodes.p, (size_t)noff[(size_t)m] * sizeof(gbx_dbg_node), hipMemcpyDeviceToHost, s));
        if (eoff[(size_t)m]) GBX_HIP(hipMemcpyAsync(edges, dedges.p, (size_t)eoff[(size_t)m] * sizeof(gbx_dbg_edge), hipMemcpyDeviceToHost, s));
    }
    if ((rc = dbg_err_check(derr.as<int>(), s, who))) return rc;
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
    auto cost = [&](int64_t j) { return (double)(dbg_window_occ(p->k, W->ref_off[w0 + j + 1] - W->ref_off[w0 + j], rcp.data(), W->read_lo[w0 + j], W->read_hi[w0 + j]) + 1); };
    auto range = [&](int64_t lo, int64_t hi) -> int {
        return dbg_run_host_range(p, R, W, w0 + lo, w0 + hi, stats ? stats + lo : nullptr, nodes ? node_off + lo : nullptr,
                                  nodes ? edge_off + lo : nullptr, nodes ? nodes + node_off[lo] : nullptr,
                                  nodes ? edges + edge_off[lo] : nullptr, who);
    };
    const int64_t n = w1 - w0;
    return spread_over_devices(who, n, n, 64, cost, [&]() { return range(0, n); }, [&](int, int64_t lo, int64_t hi) { return range(lo, hi); });
}

// A device entry: the offsets and ranges read back and checked, windows [w0, w1) planned into the workspace's table region, run.
int dbg_device(const gbx_dbg_params *p, const gbx_dbg_reads *R, const gbx_dbg_wins *W, int64_t w0, int64_t w1, gbx_dbg_stats *d_stats,
               const DbgGraphOut &g, void *d_work, size_t work_bytes, hipStream_t s, const char *who)
{
    int rc = dbg_structs_check(p, R, W, who);
    if (rc) return rc;
    if (!d_work) { set_error("%s: null workspace", who); return GBX_ERR_ARG; }
    if ((rc = dbg_total_check(R, W, who))) return rc;
    if (w0 < 0 || w1 < w0 || w1 > W->n_win) { set_error("%s: windows [%lld, %lld) of %lld", who, (long long)w0, (long long)w1, (long long)W->n_win); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    const DbgBuildLayout L = dbg_build_layout(W->n_win, R->n_reads, 0);
    if (work_bytes < L.region) { set_error("%s: workspace of %zu bytes, at least %zu needed", who, work_bytes, L.region); return GBX_ERR_ARG; }
    DbgHostArrays H;
    std::vector<int64_t> rcp, batches;
    std::vector<DbgWinPlan> plan;
    StreamDrain drain{s};                            // the host arrays above outlive the queued copies
    if ((rc = dbg_read_back(R, W, s, who, H))) return rc;
    rcp = dbg_read_prefix(p->k, R->n_reads, H.seq_off.data());
    if ((rc = cut_batches(p->k, w0, w1, H, rcp.data(), work_bytes - L.region, plan, batches))) return rc;
    char *work = (char *)d_work;
    int64_t *d_rcp = (int64_t *)(work + L.rcp);
    int *d_err = (int *)(work + L.err);
    GBX_HIP(hipMemcpyAsync(d_rcp, rcp.data(), rcp.size() * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemsetAsync(d_err, 0, 4, s));
    if ((rc = dbg_launch(dbg_dev(p->k, p, R, W, d_rcp), plan, batches, (DbgWinPlan *)(work + L.plan), d_err, work + L.region, d_stats, g, s))) return rc;
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
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
    return dbg_build_layout(n_win, n_reads, max_window_occ).bytes;
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
