// capi_dbg_asm.hip — the assembly entries behind the dbg build (include/gbx.h, dbg_asm section): the retry loop over k on the
// host, each round's builds (dbg_kernels.hip) and the cycle check, start list and path search (dbg_asm_kernels.hip) queued range
// by range on one stream.
#include <list>
#include "capi_common.h"
#include "dbg_host.h"

using namespace gbx;

namespace {

// the largest k the retry can reach from k
int asm_k_max(int k, const gbx_dbg_asm_params *ap)
{
    if (k > ap->k_last) return k;
    const int64_t rounds = ((int64_t)ap->k_last - k) / ap->k_step + 1;
    return (int)std::min<int64_t>(INT32_MAX, k + rounds * ap->k_step);
}

int asm_params_check(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const char *who)
{
    int rc = dbg_params_check(p, who);
    if (rc) return rc;
    if (!ap) { set_error("%s: null assembly params", who); return GBX_ERR_ARG; }
    if (ap->min_weight < 0 || ap->k_step < 1 || ap->max_pending < 0 || ap->max_pending > GBX_DBG_ASM_MAX_PENDING || ap->max_finished < 0 ||
        ap->max_steps < 0) {
        set_error("%s: min_weight = %d (>= 0), k_step = %d (>= 1), max_pending = %d (0..%d), max_finished = %d (>= 0), max_steps = %lld (>= 0)", who,
                  ap->min_weight, ap->k_step, ap->max_pending, GBX_DBG_ASM_MAX_PENDING, ap->max_finished, (long long)ap->max_steps);
        return GBX_ERR_ARG;
    }
    if (asm_k_max(p->k, ap) > GBX_DBG_MAX_K) {
        set_error("%s: k = %d, k_step = %d, k_last = %d: the retry would reach k = %d (%d..%d)", who, p->k, ap->k_step, ap->k_last, asm_k_max(p->k, ap),
                  GBX_DBG_MIN_K, GBX_DBG_MAX_K);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int asm_out_check(const gbx_dbg_asm_out *o, int64_t n_win, const char *who)
{
    if (!o || !o->totals || (n_win > 0 && (!o->stats || !o->wins)) || o->cap_starts < 0 || o->cap_paths < 0 || o->cap_path_nodes < 0 ||
        (o->cap_starts > 0 && !o->starts) || (o->cap_paths > 0 && !o->paths) || (o->cap_path_nodes > 0 && (!o->path_nodes || !o->path_seq))) {
        set_error("%s: null output or negative capacity", who);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

// The call on one device with everything in device memory; H: the host's copies of the offsets and ranges (checked by the
// caller).  Synchronises s after every round and however it returns.
int asm_run(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const gbx_dbg_reads *R, const gbx_dbg_wins *W, const gbx_dbg_asm_out *out,
            const DbgHostArrays &H, void *d_work, size_t work_bytes, hipStream_t s, int64_t *totals, const char *who)
{
    const int64_t n = R->n_reads, nw = W->n_win;
    totals[0] = totals[1] = totals[2] = 0;
    if (nw == 0) {
        GBX_HIP(hipMemsetAsync(out->totals, 0, 24, s));
        GBX_HIP(hipStreamSynchronize(s));
        return GBX_OK;
    }
    std::vector<int64_t> rcp = dbg_read_prefix(p->k, n, H.seq_off.data());
    const int64_t max_occ = dbg_max_occ(p->k, H, rcp.data());
    const DbgAsmLayout L = dbg_asm_layout(nw, n, max_occ);
    if (work_bytes < L.least) {
        set_error("%s: workspace of %zu bytes, at least %zu needed (gbx_dbg_assemble_workspace_bytes: max_window_occ %lld)", who, work_bytes, L.least,
                  (long long)max_occ);
        return GBX_ERR_ARG;
    }
    char *work = (char *)d_work, *area = work + L.area;
    int64_t *d_rcp = (int64_t *)(work + L.rcp), *d_noff = (int64_t *)(work + L.node_off), *d_eoff = (int64_t *)(work + L.edge_off);
    DbgWinPlan *d_plan = (DbgWinPlan *)(work + L.plan); int *d_err = (int *)(work + L.err);
    DbgAsmDev A;
    A.cyc = (int32_t *)(work + L.cyc); A.win_slot = (int32_t *)(work + L.win_slot); A.fin = (int32_t *)(work + L.fin);
    A.wstart = (int64_t *)(work + L.wstart); A.counters = (int64_t *)(work + L.counters); A.pathbuf = (int32_t *)(work + L.pathbuf);
    A.path_slice = L.path_slice; A.path_blocks = (int32_t)L.path_blocks;
    A.ref = W->ref; A.seq = R->seq; A.ap = *ap; A.out = *out;
    const size_t limit = dbg_area_bytes(L.least - L.area, work_bytes - L.area);      // a range: the area, the largest window's share at least

    std::vector<int64_t> S((size_t)nw);
    for (int64_t w = 0; w < nw; ++w) S[(size_t)w] = w;
    std::vector<int32_t> cyc((size_t)nw, 0);
    std::list<DbgAsmRange> ranges;                   // a round's plans and offsets: the queued copies read them
    StreamDrain drain{s};                            // the host arrays above outlive the queued copies
    GBX_HIP(hipMemsetAsync(d_err, 0, 4, s));
    GBX_HIP(hipMemsetAsync(A.counters, 0, 64, s));
    int k = p->k;
    for (int round = 1; !S.empty(); ++round) {
        if (round > 1) rcp = dbg_read_prefix(k, n, H.seq_off.data());
        ranges.clear();
        GBX_HIP(hipMemcpyAsync(d_rcp, rcp.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        const DbgDev a = dbg_dev(k, p, R, W, d_rcp);
        A.k = k; A.n_builds = round; A.last_round = k > ap->k_last;
        for (size_t done = 0; done < S.size();) {
            ranges.emplace_back();
            DbgAsmRange &r = ranges.back();
            done = dbg_asm_cut_range(k, S, done, H, rcp.data(), limit, r);
            const size_t m = r.plan.size();
            const DbgAsmRangeLayout G = dbg_asm_range_layout(r.tables, r.node_off.back(), r.edge_off.back());
            DbgGraphOut g;
            g.nodes = (gbx_dbg_node *)(area + G.at[DBG_ASM_NODES]); g.edges = (gbx_dbg_edge *)(area + G.at[DBG_ASM_EDGES]);
            A.deg = (int32_t *)(area + G.at[DBG_ASM_DEG]); A.list = (int32_t *)(area + G.at[DBG_ASM_LIST]); A.nxt = (int32_t *)(area + G.at[DBG_ASM_NXT]);
            g.node_off = d_noff; g.edge_off = d_eoff;
            GBX_HIP(hipMemcpyAsync(d_noff, r.node_off.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
            GBX_HIP(hipMemcpyAsync(d_eoff, r.edge_off.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
            int rc = dbg_launch(a, r.plan, {0, (int64_t)m}, d_plan, d_err, area + G.at[DBG_ASM_TABLES], out->stats, g, s);
            if (rc) return rc;
            A.nw = (int32_t)m; A.plan = d_plan;
            A.node_off = g.node_off; A.edge_off = g.edge_off; A.nodes = g.nodes; A.edges = g.edges;
            if ((rc = dbg_asm_launch(A, s))) return rc;
            // (the next range's plan and offsets take the same place: its copies run behind these kernels in stream order)
        }
        GBX_HIP(hipMemcpyAsync(cyc.data(), A.cyc, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
        const int rc = dbg_err_check(d_err, s, who);
        if (rc) return rc;
        if (k > ap->k_last) break;
        std::vector<int64_t> next;
        for (int64_t w : S)
            if (cyc[(size_t)w]) next.push_back(w);
        S.swap(next);
        k += ap->k_step;
    }
    GBX_HIP(hipMemcpyAsync(out->totals, A.counters, 24, hipMemcpyDeviceToDevice, s));
    GBX_HIP(hipMemcpyAsync(totals, A.counters, 24, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (totals[0] > out->cap_starts || totals[1] > out->cap_paths || totals[2] > out->cap_path_nodes) {
        set_error("%s: %lld starts, %lld paths and %lld path nodes%s; the capacities are %lld, %lld and %lld", who, (long long)totals[0],
                  (long long)totals[1], (long long)totals[2], totals[0] > out->cap_starts ? " among the starts that fitted" : "",
                  (long long)out->cap_starts, (long long)out->cap_paths, (long long)out->cap_path_nodes);
        return GBX_ERR_UNSUPPORTED;
    }
    return GBX_OK;
}

}  // namespace

extern "C" {

void gbx_dbg_asm_default_params(gbx_dbg_asm_params *p)
{
    if (!p) return;
    p->min_weight = 40; p->k_step = 5; p->k_last = 50; p->max_pending = 20; p->max_finished = 20; p->pad_ = 0;
    p->max_steps = (int64_t)1 << 20;
}

size_t gbx_dbg_assemble_workspace_bytes(const gbx_dbg_params *p, int64_t n_win, int64_t n_reads, int64_t max_window_occ)
{
    if (!p || n_win < 0 || n_reads < 0 || max_window_occ < 0) return 0;
    return dbg_asm_layout(n_win, n_reads, max_window_occ).bytes;
}

int gbx_dbg_assemble_device(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const gbx_dbg_reads *R, const gbx_dbg_wins *W,
                            const gbx_dbg_asm_out *out, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_dbg_assemble_device";
    hipStream_t s = (hipStream_t)stream;
    int rc = asm_params_check(p, ap, who);
    if (rc || (rc = dbg_structs_check(p, R, W, who))) return rc;
    if (!d_work) { set_error("%s: null workspace", who); return GBX_ERR_ARG; }
    if ((rc = asm_out_check(out, W->n_win, who)) || (rc = dbg_total_check(R, W, who)) || (rc = require_device())) return rc;
    DbgHostArrays H;
    int64_t totals[3];
    StreamDrain drain{s};                            // the host arrays above outlive the queued copies
    if ((rc = dbg_read_back(R, W, s, who, H))) return rc;
    return asm_run(p, ap, R, W, out, H, d_work, work_bytes, s, totals, who);
}

int gbx_dbg_assemble_host(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const gbx_dbg_reads *R, const gbx_dbg_wins *W,
                          const gbx_dbg_asm_out *out)
{
    RoctxRange range_("gbx_dbg_assemble_host");
    const char *who = "gbx_dbg_assemble_host";
    int rc = asm_params_check(p, ap, who);
    if (rc) return rc;
    if ((rc = dbg_check(p, R, W, who))) return rc;
    if ((rc = asm_out_check(out, W->n_win, who))) return rc;
    out->totals[0] = out->totals[1] = out->totals[2] = 0;
    const int64_t n = R->n_reads, nw = W->n_win;
    if (nw == 0) return GBX_OK;
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l; hipStream_t s = L->compute;
    DbgUpload U(L);
    DevBuf dst(L), dwin(L), dstart(L), dpath(L), dpn(L), dps(L), dtot(L), dwork(L);
    int64_t totals[3];
    StreamDrain drain{s};                            // the host arrays above outlive the queued copies
    if ((rc = U.up(R, W, 0, n, 0, nw, s))) return rc;
    const std::vector<int64_t> rcp = dbg_read_prefix(p->k, n, U.h.seq_off.data());
    const size_t work_bytes = dbg_asm_layout(nw, n, dbg_max_occ(p->k, U.h, rcp.data())).bytes;
    if ((rc = dst.alloc((size_t)nw * sizeof(gbx_dbg_stats))) || (rc = dwin.alloc((size_t)nw * sizeof(gbx_dbg_asm_win))) ||
        (rc = dstart.alloc((size_t)out->cap_starts * sizeof(gbx_dbg_asm_start))) || (rc = dpath.alloc((size_t)out->cap_paths * sizeof(gbx_dbg_asm_path))) ||
        (rc = dpn.alloc((size_t)out->cap_path_nodes * 4)) || (rc = dps.alloc((size_t)out->cap_path_nodes)) || (rc = dtot.alloc(64)) ||
        (rc = dwork.alloc(work_bytes)))
        return rc;
    gbx_dbg_asm_out dO = *out;
    dO.stats = dst.as<gbx_dbg_stats>(); dO.wins = dwin.as<gbx_dbg_asm_win>(); dO.starts = dstart.as<gbx_dbg_asm_start>();
    dO.paths = dpath.as<gbx_dbg_asm_path>(); dO.path_nodes = dpn.as<int32_t>(); dO.path_seq = dps.as<uint8_t>(); dO.totals = dtot.as<int64_t>();
    rc = asm_run(p, ap, &U.R, &U.W, &dO, U.h, dwork.p, work_bytes, s, totals, who);
    if (rc && rc != GBX_ERR_UNSUPPORTED) return rc;
    const int64_t ns = std::min(totals[0], out->cap_starts), np = std::min(totals[1], out->cap_paths), nn = std::min(totals[2], out->cap_path_nodes);
    GBX_HIP(hipMemcpyAsync(out->stats, dst.p, (size_t)nw * sizeof(gbx_dbg_stats), hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(out->wins, dwin.p, (size_t)nw * sizeof(gbx_dbg_asm_win), hipMemcpyDeviceToHost, s));
    if (ns) GBX_HIP(hipMemcpyAsync(out->starts, dstart.p, (size_t)ns * sizeof(gbx_dbg_asm_start), hipMemcpyDeviceToHost, s));
    if (np) GBX_HIP(hipMemcpyAsync(out->paths, dpath.p, (size_t)np * sizeof(gbx_dbg_asm_path), hipMemcpyDeviceToHost, s));
    if (nn) {
        GBX_HIP(hipMemcpyAsync(out->path_nodes, dpn.p, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(out->path_seq, dps.p, (size_t)nn, hipMemcpyDeviceToHost, s));
    }
    GBX_HIP(hipStreamSynchronize(s));
    out->totals[0] = totals[0]; out->totals[1] = totals[1]; out->totals[2] = totals[2];
    return rc;
}

}  // extern "C"
