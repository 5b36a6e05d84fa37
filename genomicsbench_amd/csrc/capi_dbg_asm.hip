// capi_dbg_asm.hip — the assembly entries behind the dbg build (include/gbx.h, dbg_asm section): the retry loop over k on the
// host, each round's builds (dbg_kernels.hip) and the cycle check, start list and path search (dbg_asm_kernels.hip) queued range
// by range on one stream.
#include <list>
#include "capi_common.h"
#include "dbg_host.h"
#include "dbg_hash.h"

using namespace gbx;

namespace {

// A range's graphs (tables, nodes, edges, in-degrees, list and pointers): at most this much, or one window's if that alone is more.
constexpr size_t ASM_RANGE_BYTES = (size_t)2 << 30;
// The searches' current paths: at most this much, 1024 wavefronts, at least one.
constexpr size_t ASM_PATH_BYTES = (size_t)256 << 20;
constexpr int ASM_PATH_BLOCKS = 1024;

// what one window of C occurrence slots takes of a range: its tables, 2C nodes, C edges, 2C in-degrees, list entries and pointers
size_t asm_window_bytes(int64_t C)
{
    return align256(dbg_window_bytes(C)) + (size_t)C * (2 * sizeof(gbx_dbg_node) + sizeof(gbx_dbg_edge) + 24);
}
constexpr size_t ASM_RANGE_SLACK = 6 * 256;          // the six arrays behind the tables start at multiples of 256

int64_t asm_path_slice(int64_t max_occ) { return (2 * max_occ + 2 + 63) & ~(int64_t)63; }
int asm_path_blocks(int64_t slice)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(ASM_PATH_BLOCKS, (int64_t)(ASM_PATH_BYTES / ((size_t)slice * 4))));
}

size_t asm_head_bytes(int64_t n_win, int64_t n_reads)
{
    const size_t nw = (size_t)std::max<int64_t>(n_win, 1);
    return align256((size_t)(n_reads + 1) * 8) + align256(nw * sizeof(DbgWinPlan)) + 256 + 3 * align256(nw * 4) + align256(nw * 8) + 256 +
           2 * align256((nw + 1) * 8);
}

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

// The call on one device with everything in device memory; soff / roff / rpos / rlo / rhi: the host's copies of the offsets and
// ranges (checked by the caller).  Synchronises s after every round and at the end.
int asm_run(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const gbx_dbg_reads *R, const gbx_dbg_wins *W, const gbx_dbg_asm_out *out,
            const int64_t *soff, const int64_t *roff, const int64_t *rpos, const int64_t *rlo, const int64_t *rhi, void *d_work, size_t work_bytes,
            hipStream_t s, int64_t *totals, const char *who)
{
    const int64_t n = R->n_reads, nw = W->n_win;
    totals[0] = totals[1] = totals[2] = 0;
    if (nw == 0) {
        GBX_HIP(hipMemsetAsync(out->totals, 0, 24, s));
        GBX_HIP(hipStreamSynchronize(s));
        return GBX_OK;
    }
    // the workspace: head, the searches' paths, the range area
    std::vector<int64_t> rcp = dbg_read_prefix(p->k, n, soff);
    int64_t max_occ = 0;
    for (int64_t w = 0; w < nw; ++w)
        max_occ = std::max(max_occ, std::max<int64_t>(0, roff[w + 1] - roff[w] - p->k - 1) + rcp[(size_t)rhi[w]] - rcp[(size_t)rlo[w]]);
    const int64_t slice = asm_path_slice(max_occ);
    const int blocks = asm_path_blocks(slice);
    const size_t head = asm_head_bytes(nw, n), paths = align256((size_t)blocks * (size_t)slice * 4);
    if (work_bytes < head + paths + asm_window_bytes(max_occ) + ASM_RANGE_SLACK) {
        set_error("%s: workspace of %zu bytes, at least %zu needed (gbx_dbg_assemble_workspace_bytes: max_window_occ %lld)", who, work_bytes,
                  head + paths + asm_window_bytes(max_occ) + ASM_RANGE_SLACK, (long long)max_occ);
        return GBX_ERR_ARG;
    }
    char *wp = (char *)d_work;
    auto take = [&](size_t bytes) { char *q = wp; wp += align256(bytes); return q; };
    int64_t *d_rcp = (int64_t *)take((size_t)(n + 1) * 8);
    DbgWinPlan *d_plan = (DbgWinPlan *)take((size_t)nw * sizeof(DbgWinPlan));
    int *d_err = (int *)take(256);
    DbgAsmDev A;
    A.ap = *ap;
    A.cyc = (int32_t *)take((size_t)nw * 4);
    A.win_slot = (int32_t *)take((size_t)nw * 4);
    A.fin = (int32_t *)take((size_t)nw * 4);
    A.wstart = (int64_t *)take((size_t)nw * 8);
    A.counters = (int64_t *)take(256);
    int64_t *d_noff = (int64_t *)take((size_t)(nw + 1) * 8), *d_eoff = (int64_t *)take((size_t)(nw + 1) * 8);
    A.pathbuf = (int32_t *)take((size_t)blocks * (size_t)slice * 4);
    A.path_slice = slice;
    A.path_blocks = blocks;
    A.ref = W->ref; A.seq = R->seq;
    A.out = *out;
    char *area = wp;
    const size_t area_bytes = work_bytes - (size_t)(wp - (char *)d_work);
    GBX_HIP(hipMemsetAsync(d_err, 0, 4, s));
    GBX_HIP(hipMemsetAsync(A.counters, 0, 64, s));

    std::vector<int64_t> S((size_t)nw);
    for (int64_t w = 0; w < nw; ++w) S[(size_t)w] = w;
    std::vector<int32_t> cyc((size_t)nw, 0);
    int k = p->k;
    for (int round = 1; !S.empty(); ++round) {
        if (round > 1) rcp = dbg_read_prefix(k, n, soff);
        GBX_HIP(hipMemcpyAsync(d_rcp, rcp.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        DbgDev a;
        a.k = k; a.min_qual = p->min_qual; a.ref_bytes = W->ref_bytes;
        a.ref = W->ref; a.seq = R->seq; a.qual = R->qual; a.seq_off = R->seq_off; a.rcp = d_rcp; a.flag = R->flag;
        A.k = k; A.n_builds = round; A.last_round = k > ap->k_last;
        // the host arrays the queued copies read: kept until the round's synchronisation
        std::list<std::vector<DbgWinPlan>> plans;
        std::list<std::vector<int64_t>> offs;
        size_t done = 0;
        while (done < S.size()) {
            plans.emplace_back();
            std::vector<DbgWinPlan> &plan = plans.back();
            offs.emplace_back(1, 0);
            std::vector<int64_t> &noff = offs.back();
            offs.emplace_back(1, 0);
            std::vector<int64_t> &eoff = offs.back();
            size_t tables = 0, used = ASM_RANGE_SLACK;
            int64_t cand = 0;
            const size_t limit = std::min(area_bytes, std::max(ASM_RANGE_BYTES, asm_window_bytes(max_occ) + ASM_RANGE_SLACK));
            for (; done < S.size() && plan.size() < ((size_t)1 << 20); ++done) {
                const int64_t w = S[done];
                DbgWinPlan P;
                P.nref_c = std::max<int64_t>(0, roff[w + 1] - roff[w] - k - 1);
                P.read_lo = rlo[w];
                P.read_hi = std::max(rlo[w], rhi[w]);
                P.C = P.nref_c + (rcp[(size_t)P.read_hi] - rcp[(size_t)P.read_lo]);
                const size_t b = asm_window_bytes(P.C);
                if (used + b > limit && !plan.empty()) break;
                P.ref_off = roff[w]; P.ref_pos = rpos[w]; P.win = w;
                P.nc = dbg_node_slots(P.C); P.ec = dbg_edge_slots(P.C);
                P.base = (int64_t)tables; P.cand0 = cand;
                tables += align256(dbg_window_bytes(P.C));
                used += b;
                cand += P.C;
                noff.push_back(noff.back() + 2 * P.C);
                eoff.push_back(eoff.back() + P.C);
                plan.push_back(P);
            }
            const size_t m = plan.size();
            const int64_t ncap = noff.back(), ecap = eoff.back();
            char *q = area + align256(tables);
            DbgGraphOut g;
            g.nodes = (gbx_dbg_node *)q; q += align256((size_t)ncap * sizeof(gbx_dbg_node));
            g.edges = (gbx_dbg_edge *)q; q += align256((size_t)ecap * sizeof(gbx_dbg_edge));
            A.deg = (int32_t *)q; q += align256((size_t)ncap * 4);
            A.list = (int32_t *)q; q += align256((size_t)ncap * 4);
            A.nxt = (int32_t *)q;
            g.node_off = d_noff; g.edge_off = d_eoff;
            GBX_HIP(hipMemcpyAsync(d_noff, noff.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
            GBX_HIP(hipMemcpyAsync(d_eoff, eoff.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
            const std::vector<int64_t> one = {0, (int64_t)m};
            int rc = dbg_launch(a, plan, one, d_plan, d_err, area, out->stats, g, s);
            if (rc) return rc;
            A.nw = (int32_t)m; A.plan = d_plan;
            A.node_off = g.node_off; A.edge_off = g.edge_off; A.nodes = g.nodes; A.edges = g.edges;
            if ((rc = dbg_asm_launch(A, s))) return rc;
            // (the next range's plan and offsets take the same place: its copies run behind these kernels in stream order)
        }
        int err = 0;
        GBX_HIP(hipMemcpyAsync(cyc.data(), A.cyc, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipStreamSynchronize(s));
        if (err) { set_error("%s: a window's table filled (%d): cannot happen by its sizing", who, err); return GBX_ERR_HIP; }
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

size_t asm_workspace(int64_t n_win, int64_t n_reads, int64_t max_occ)
{
    const size_t one = asm_window_bytes(max_occ) + ASM_RANGE_SLACK;
    const size_t all = n_win > 0 && one > ((size_t)-1) / (size_t)n_win ? (size_t)-1 : one * (size_t)std::max<int64_t>(n_win, 1);
    const int64_t slice = asm_path_slice(max_occ);
    return asm_head_bytes(n_win, n_reads) + align256((size_t)asm_path_blocks(slice) * (size_t)slice * 4) + std::max(one, std::min(all, ASM_RANGE_BYTES)) +
           256;
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
    return asm_workspace(n_win, n_reads, max_window_occ);
}

int gbx_dbg_assemble_device(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const gbx_dbg_reads *R, const gbx_dbg_wins *W,
                            const gbx_dbg_asm_out *out, void *d_work, size_t work_bytes, void *stream)
{
    const char *who = "gbx_dbg_assemble_device";
    hipStream_t s = (hipStream_t)stream;
    int rc = asm_params_check(p, ap, who);
    if (rc) return rc;
    if (!R || !W || R->n_reads < 0 || W->n_win < 0 || R->seq_bytes < 0 || W->ref_bytes < 0 || !R->seq_off || !W->ref_off || !d_work ||
        (W->n_win > 0 && (!W->ref_pos || !W->read_lo || !W->read_hi)) || (R->n_reads > 0 && !R->flag) ||
        (R->seq_bytes > 0 && (!R->seq || !R->qual)) || (W->ref_bytes > 0 && !W->ref)) {
        set_error("%s: null pointer or negative size", who);
        return GBX_ERR_ARG;
    }
    if ((rc = asm_out_check(out, W->n_win, who))) return rc;
    if (W->ref_bytes + R->seq_bytes >= ((int64_t)1 << 40)) { set_error("%s: more than 2^40 bytes of reference and reads", who); return GBX_ERR_UNSUPPORTED; }
    if ((rc = require_device())) return rc;
    const int64_t n = R->n_reads, nw = W->n_win;
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
    int64_t totals[3];
    return asm_run(p, ap, R, W, out, soff.data(), roff.data(), rpos.data(), rlo.data(), rhi.data(), d_work, work_bytes, s, totals, who);
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
    const std::vector<int64_t> rcp = dbg_read_prefix(p->k, n, R->seq_off);
    int64_t max_occ = 0;
    for (int64_t w = 0; w < nw; ++w)
        max_occ = std::max(max_occ, std::max<int64_t>(0, W->ref_off[w + 1] - W->ref_off[w] - p->k - 1) + rcp[(size_t)W->read_hi[w]] - rcp[(size_t)W->read_lo[w]]);
    const size_t work_bytes = asm_workspace(nw, n, max_occ);
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    hipStream_t s = L->compute;
    DevBuf dref(L), dseq(L), dqual(L), dsoff(L), dflag(L), droff(L), drpos(L), drlo(L), drhi(L), dst(L), dwin(L), dstart(L), dpath(L), dpn(L), dps(L),
        dtot(L), dwork(L);
    if ((rc = dref.alloc((size_t)W->ref_bytes + 128)) || (rc = dseq.alloc((size_t)R->seq_bytes + 128)) || (rc = dqual.alloc((size_t)R->seq_bytes + 128)) ||
        (rc = dsoff.alloc((size_t)(n + 1) * 8)) || (rc = dflag.alloc((size_t)n * 2 + 8)) || (rc = droff.alloc((size_t)(nw + 1) * 8)) ||
        (rc = drpos.alloc((size_t)nw * 8)) || (rc = drlo.alloc((size_t)nw * 8)) || (rc = drhi.alloc((size_t)nw * 8)) ||
        (rc = dst.alloc((size_t)nw * sizeof(gbx_dbg_stats))) || (rc = dwin.alloc((size_t)nw * sizeof(gbx_dbg_asm_win))) ||
        (rc = dstart.alloc((size_t)out->cap_starts * sizeof(gbx_dbg_asm_start))) || (rc = dpath.alloc((size_t)out->cap_paths * sizeof(gbx_dbg_asm_path))) ||
        (rc = dpn.alloc((size_t)out->cap_path_nodes * 4)) || (rc = dps.alloc((size_t)out->cap_path_nodes)) || (rc = dtot.alloc(64)) ||
        (rc = dwork.alloc(work_bytes)))
        return rc;
    if (W->ref_bytes > 0) GBX_HIP(hipMemcpyAsync(dref.p, W->ref, (size_t)W->ref_bytes, hipMemcpyHostToDevice, s));
    if (R->seq_bytes > 0) {
        GBX_HIP(hipMemcpyAsync(dseq.p, R->seq, (size_t)R->seq_bytes, hipMemcpyHostToDevice, s));
        GBX_HIP(hipMemcpyAsync(dqual.p, R->qual, (size_t)R->seq_bytes, hipMemcpyHostToDevice, s));
    }
    GBX_HIP(hipMemcpyAsync(dsoff.p, R->seq_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
    if (n > 0) GBX_HIP(hipMemcpyAsync(dflag.p, R->flag, (size_t)n * 2, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(droff.p, W->ref_off, (size_t)(nw + 1) * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(drpos.p, W->ref_pos, (size_t)nw * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(drlo.p, W->read_lo, (size_t)nw * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(drhi.p, W->read_hi, (size_t)nw * 8, hipMemcpyHostToDevice, s));
    gbx_dbg_reads dR = *R;
    dR.seq_off = dsoff.as<int64_t>(); dR.seq = dseq.as<uint8_t>(); dR.qual = dqual.as<uint8_t>(); dR.flag = dflag.as<uint16_t>(); dR.pos = dR.end = nullptr;
    gbx_dbg_wins dW = *W;
    dW.ref_off = droff.as<int64_t>(); dW.ref = dref.as<uint8_t>(); dW.ref_pos = drpos.as<int64_t>(); dW.read_lo = drlo.as<int64_t>(); dW.read_hi = drhi.as<int64_t>();
    gbx_dbg_asm_out dO = *out;
    dO.stats = dst.as<gbx_dbg_stats>(); dO.wins = dwin.as<gbx_dbg_asm_win>(); dO.starts = dstart.as<gbx_dbg_asm_start>();
    dO.paths = dpath.as<gbx_dbg_asm_path>(); dO.path_nodes = dpn.as<int32_t>(); dO.path_seq = dps.as<uint8_t>(); dO.totals = dtot.as<int64_t>();
    int64_t totals[3];
    rc = asm_run(p, ap, &dR, &dW, &dO, R->seq_off, W->ref_off, W->ref_pos, W->read_lo, W->read_hi, dwork.p, work_bytes, s, totals, who);
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
