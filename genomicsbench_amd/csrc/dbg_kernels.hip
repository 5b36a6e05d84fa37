// dbg_kernels.hip — Platypus's de Bruijn graph per assembly window (R/benchmarks/dbg/debruijn.cpp:1262-1385, 740-920) for
// gfx950 (MI355X).
//
// Semantics: include/gbx.h, dbg section.  The windows are done in batches; a batch's windows each get tables of their own in
// global memory, sized from the window's occurrence slots C (ref_len - k - 1 and l_seq - k - 1 per read, QC-fail reads and
// skipped occurrences included): a node table of the first power of two above 2C (a window has at most 2C distinct nodes,
// so the table never fills and capacity is exact at any depth), an edge table of the first power of two above C, and a
// first-touch index of 2C entries.  Three passes per batch:
//   init     one workgroup per window: keys 0, first-touch keys and list heads all ones, sums 0.
//   insert   one lane per occurrence slot.  The slot is decoded (window by a binary search over the batch's slot offsets,
//            read by one over the reads' slot prefix), checked (flag 0x200, 'N', min_qual) and both k-mers hashed in one pass
//            over the k + 1 bytes.  A node is found by linear probing; a slot's key is a 23-bit hash tag and the byte address
//            of some occurrence of the k-mer, claimed by a 64-bit compare-and-swap, and a tag match is confirmed by comparing
//            the k bytes with that address.  The occurrence's order 2o + side (o its slot number: ref first, then reads by
//            index and offset) goes to the node by atomicMin, its weight by atomicAdd, its colour by atomicOr.  The edge's
//            key is (start node slot, next byte): exact, no byte compare.  The lane that creates an edge pushes it onto the
//            start node's list (atomicExch), and every occurrence adds its order (atomicMin), weight and count.
//   finish   one workgroup per window: the nodes are scattered to their first-touch key and compacted with a block scan
//            (the rank = the reference's allNodes order); then, 256 ranks at a time, each lane walks its node's edge list,
//            keeps the 4 successors of least first appearance, forms the node's digest record in LDS at its scanned offset,
//            and (for gbx_dbg_graph_*) writes the node and its edges; one lane folds the records into the FNV-1a digest.
// Everything is integer sums, minima and ORs, so the graph does not depend on the schedule.  Every loop is bounded: probes
// by the table size, the list walk by the edge table size, the binary searches by log2 of their range; in the
// GBX_LOOP_GUARD build the probe and list loops count down from those bounds as well (kernel 9).
// The hash (FNV-1a fold, mix64, tag / home split, edge key) and the table sizing are in dbg_hash.h, which the plain host compiler
// takes as well: tests/hostcheck/dbg_hash_check.cpp holds the tests' colliding k-mers (tests/dbg_cases.py) against it.
#include <algorithm>
#include "gbx_internal.h"
#include "dbg_hash.h"

namespace gbx {
namespace {

constexpr int FIN_THREADS = 256;
constexpr int INS_THREADS = 256;
constexpr int REC_MAX = GBX_DBG_MAX_K + 1 + 4 + 8 + 1 + 4 * 12;   // one node's digest record at most
constexpr uint64_t FNV_BASIS = DBG_FNV_BASIS, FNV_PRIME = DBG_FNV_PRIME;   // (the digest is FNV-1a too)
constexpr uint64_t ADDR_MASK = (1ull << DBG_TAG_SHIFT) - 1;

struct Tables {                      // one window's tables inside the batch region (dbg_window_bytes)
    uint64_t *key, *first, *weight;  // node slots
    uint32_t *col;
    int32_t *head, *rank;
    uint64_t *ekey, *efirst, *ew;    // edge slots
    uint32_t *ecnt;
    int32_t *eend, *enext;
    int32_t *byfirst;                // 2C
};

__device__ inline Tables tables_of(char *region, const DbgWinPlan &W)
{
    Tables t;
    char *p = region + W.base;
    const int64_t nc = W.nc, ec = W.ec;
    t.key = (uint64_t *)p; p += nc * 8;
    t.first = (uint64_t *)p; p += nc * 8;
    t.weight = (uint64_t *)p; p += nc * 8;
    t.col = (uint32_t *)p; p += nc * 4;
    t.head = (int32_t *)p; p += nc * 4;
    t.rank = (int32_t *)p; p += nc * 4;
    t.ekey = (uint64_t *)p; p += ec * 8;
    t.efirst = (uint64_t *)p; p += ec * 8;
    t.ew = (uint64_t *)p; p += ec * 8;
    t.ecnt = (uint32_t *)p; p += ec * 4;
    t.eend = (int32_t *)p; p += ec * 4;
    t.enext = (int32_t *)p; p += ec * 4;
    t.byfirst = (int32_t *)p;
    return t;
}

__global__ void __launch_bounds__(FIN_THREADS) dbg_init_kernel(const DbgWinPlan *plan, char *region)
{
    const DbgWinPlan W = plan[blockIdx.x];
    Tables t = tables_of(region, W);
    for (int64_t i = threadIdx.x; i < W.nc; i += FIN_THREADS) {
        t.key[i] = 0; t.first[i] = ~0ull; t.weight[i] = 0; t.col[i] = 0; t.head[i] = -1;
    }
    for (int64_t i = threadIdx.x; i < W.ec; i += FIN_THREADS) { t.ekey[i] = 0; t.efirst[i] = ~0ull; t.ew[i] = 0; t.ecnt[i] = 0; }
    for (int64_t i = threadIdx.x; i < 2 * W.C; i += FIN_THREADS) t.byfirst[i] = -1;
}

__device__ inline const uint8_t *text_at(const DbgDev &a, uint64_t addr)
{
    return addr < (uint64_t)a.ref_bytes ? a.ref + addr : a.seq + (addr - (uint64_t)a.ref_bytes);
}

// the node slot of the k-mer at byte address addr (hash h), inserting it; -1 only if the table were full (it cannot be)
__device__ inline int64_t node_slot(const DbgDev &a, const Tables &t, int64_t nc, uint64_t h, uint64_t addr, const uint8_t *mine,
                                    int k, int64_t unit)
{
    const uint64_t tag = dbg_node_tag(h), want = tag << DBG_TAG_SHIFT | (addr + 1), mask = (uint64_t)nc - 1;
    uint64_t i = dbg_node_home(h, nc);
    GBX_GUARD(gd, nc);
    for (int64_t probe = 0; probe < nc; ++probe, i = (i + 1) & mask) {
        if (GBX_GUARD_TRIP(gd, GBX_GK_DBG, 1, unit)) break;
        uint64_t cur = __hip_atomic_load(&t.key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS((unsigned long long *)&t.key[i], 0ull, (unsigned long long)want);
            if (cur == 0) return (int64_t)i;
        }
        if (dbg_node_tag(cur) == tag) {
            const uint8_t *o = text_at(a, (cur & ADDR_MASK) - 1);
            bool eq = true;
            for (int j = 0; j < k; ++j)
                if (o[j] != mine[j]) { eq = false; break; }
            if (eq) return (int64_t)i;
        }
    }
    return -1;
}

__global__ void __launch_bounds__(INS_THREADS) dbg_insert_kernel(DbgDev a, const DbgWinPlan *plan, int nw, int64_t total, char *region,
                                                                 int *err)
{
    const int64_t t = (int64_t)blockIdx.x * INS_THREADS + threadIdx.x;
    if (t >= total) return;
    int lo = 0, hi = nw;                          // the last window whose first slot is <= t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (plan[mid].cand0 <= t) lo = mid; else hi = mid;
    }
    const DbgWinPlan &W = plan[lo];
    const int64_t c = t - W.cand0;
    const int k = a.k;
    const uint8_t *s;
    uint64_t addr;
    uint32_t wgt, colour;
    uint64_t h1 = FNV_BASIS, h2 = FNV_BASIS;
    if (c < W.nref_c) {
        addr = (uint64_t)(W.ref_off + c);
        s = a.ref + addr;
        wgt = 1; colour = GBX_DBG_REF;
        for (int j = 0; j <= k; ++j) {
            const uint64_t b = s[j];
            if (j < k) h1 = dbg_fnv_step(h1, b);
            if (j > 0) h2 = dbg_fnv_step(h2, b);
        }
    } else {
        const int64_t g = a.rcp[W.read_lo] + (c - W.nref_c);
        int64_t rl = W.read_lo, rh = W.read_hi;   // the last read r with rcp[r] <= g
        while (rh - rl > 1) {
            const int64_t mid = (rl + rh) >> 1;
            if (a.rcp[mid] <= g) rl = mid; else rh = mid;
        }
        if (a.flag[rl] & 0x200) return;
        const int64_t off = a.seq_off[rl] + (g - a.rcp[rl]);
        s = a.seq + off;
        const uint8_t *q = a.qual + off;
        uint32_t mq = 255;
        bool has_n = false;
        for (int j = 0; j <= k; ++j) {
            const uint64_t b = s[j];
            mq = min(mq, (uint32_t)q[j]);
            has_n |= b == 'N';
            if (j < k) h1 = dbg_fnv_step(h1, b);
            if (j > 0) h2 = dbg_fnv_step(h2, b);
        }
        if (has_n || (int)mq < a.min_qual) return;
        addr = (uint64_t)a.ref_bytes + (uint64_t)off;
        wgt = mq; colour = GBX_DBG_READ;
    }
    h1 = dbg_mix64(h1); h2 = dbg_mix64(h2);
    const Tables tb = tables_of(region, W);
    const int64_t sa = node_slot(a, tb, W.nc, h1, addr, s, k, t);
    const int64_t sb = sa < 0 ? -1 : node_slot(a, tb, W.nc, h2, addr + 1, s + 1, k, t);
    if (sb < 0) { atomicOr(err, 1); return; }
    atomicMin((unsigned long long *)&tb.first[sa], (unsigned long long)(2 * c));
    atomicAdd((unsigned long long *)&tb.weight[sa], (unsigned long long)wgt);
    atomicOr(&tb.col[sa], colour);
    atomicMin((unsigned long long *)&tb.first[sb], (unsigned long long)(2 * c + 1));
    atomicAdd((unsigned long long *)&tb.weight[sb], (unsigned long long)wgt);
    atomicOr(&tb.col[sb], colour);
    // the edge (start slot, next byte)
    const uint64_t ek = dbg_edge_key(sa, s[k]), emask = (uint64_t)W.ec - 1;
    uint64_t i = dbg_edge_home(ek, W.ec);
    int64_t j = -1;
    GBX_GUARD(gd, W.ec);
    for (int64_t probe = 0; probe < W.ec; ++probe, i = (i + 1) & emask) {
        if (GBX_GUARD_TRIP(gd, GBX_GK_DBG, 2, t)) break;
        uint64_t cur = __hip_atomic_load(&tb.ekey[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS((unsigned long long *)&tb.ekey[i], 0ull, (unsigned long long)ek);
            if (cur == 0) {
                tb.eend[i] = (int32_t)sb;
                tb.enext[i] = atomicExch(&tb.head[sa], (int32_t)i);
                j = (int64_t)i;
                break;
            }
        }
        if (cur == ek) { j = (int64_t)i; break; }
    }
    if (j < 0) { atomicOr(err, 2); return; }
    atomicMin((unsigned long long *)&tb.efirst[j], (unsigned long long)c);
    atomicAdd((unsigned long long *)&tb.ew[j], (unsigned long long)wgt);
    atomicAdd(&tb.ecnt[j], 1u);
}

__device__ inline int wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// exclusive prefix of v over the workgroup; *total = the sum (sh: 4 ints of LDS)
__device__ inline int block_excl_scan(int v, int *total, int *sh)
{
    const int inc = wave_incl_scan(v), w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) sh[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
    for (int x = 0; x < FIN_THREADS / 64; ++x) { const int y = sh[x]; if (x < w) off += y; tot += y; }
    __syncthreads();
    *total = tot;
    return off + inc - v;
}

__device__ inline void put32(uint8_t *b, uint32_t v) { b[0] = (uint8_t)v; b[1] = (uint8_t)(v >> 8); b[2] = (uint8_t)(v >> 16); b[3] = (uint8_t)(v >> 24); }
__device__ inline void put64(uint8_t *b, uint64_t v) { put32(b, (uint32_t)v); put32(b + 4, (uint32_t)(v >> 32)); }

__global__ void __launch_bounds__(FIN_THREADS) dbg_finish_kernel(DbgDev a, const DbgWinPlan *plan, char *region, gbx_dbg_stats *stats,
                                                                 DbgGraphOut g)
{
    __shared__ int sh[FIN_THREADS / 64];
    __shared__ unsigned long long acc[7];
    __shared__ uint8_t rec[FIN_THREADS * REC_MAX];
    __shared__ uint64_t s_digest;
    const DbgWinPlan W = plan[blockIdx.x];
    const Tables t = tables_of(region, W);
    const int tid = threadIdx.x, k = a.k;
    if (tid < 7) acc[tid] = 0;
    if (tid == 0) s_digest = FNV_BASIS;
    // every node at its first-touch key, then compacted: byfirst[rank] = slot, rank[slot] = rank
    for (int64_t i = tid; i < W.nc; i += FIN_THREADS)
        if (t.key[i] && t.first[i] < (uint64_t)(2 * W.C)) t.byfirst[t.first[i]] = (int32_t)i;
    __syncthreads();
    int64_t n = 0;
    for (int64_t c0 = 0; c0 < 2 * W.C; c0 += FIN_THREADS) {
        const int64_t j = c0 + tid;
        const int32_t v = j < 2 * W.C ? t.byfirst[j] : -1;
        int tot;
        const int pre = block_excl_scan(v >= 0 ? 1 : 0, &tot, sh);
        if (v >= 0) { t.byfirst[n + pre] = v; t.rank[v] = (int32_t)(n + pre); }   // n + pre <= j: that entry has been read
        n += tot;
        __syncthreads();
    }
    // 256 ranks at a time: edges, stats, the digest records, the graph
    int64_t ebase = 0;
    for (int64_t r0 = 0; r0 < n; r0 += FIN_THREADS) {
        const int64_t r = r0 + tid;
        int len = 0, ne = 0;
        int32_t kept[4];
        uint64_t kf[4];
        int64_t src = 0, wsum = 0, occ = 0, d = 0;
        int32_t slot = -1, pos = -1;
        uint32_t col = 0;
        uint64_t nw = 0;
        if (r < n) {
            slot = t.byfirst[r];
            const uint64_t f = t.first[slot], c = f >> 1;
            const int side = (int)(f & 1);
            if ((int64_t)c < W.nref_c) {
                src = W.ref_off + (int64_t)c + side;
                pos = (int32_t)(W.ref_pos + (int64_t)c + side);
            } else {
                const int64_t gg = a.rcp[W.read_lo] + ((int64_t)c - W.nref_c);
                int64_t rl = W.read_lo, rh = W.read_hi;
                while (rh - rl > 1) {
                    const int64_t mid = (rl + rh) >> 1;
                    if (a.rcp[mid] <= gg) rl = mid; else rh = mid;
                }
                src = -1 - (a.seq_off[rl] + (gg - a.rcp[rl]) + side);
            }
            col = t.col[slot];
            nw = t.weight[slot];
            int32_t e = t.head[slot];
            GBX_GUARD(gd, W.ec);
            for (int64_t steps = 0; e >= 0 && steps < W.ec; ++steps) {
                if (GBX_GUARD_TRIP(gd, GBX_GK_DBG, 3, r)) break;
                const uint64_t ef = t.efirst[e];
                ++d;
                occ += t.ecnt[e];
                wsum += (int64_t)t.ew[e];
                int x = ne < 4 ? ne++ : 4;               // insertion into the 4 of least first appearance
                if (x == 4 && ef < kf[3]) x = 3;
                if (x < 4) {
                    while (x > 0 && kf[x - 1] > ef) { kf[x] = kf[x - 1]; kept[x] = kept[x - 1]; --x; }
                    kf[x] = ef; kept[x] = e;
                }
                e = t.enext[e];
            }
            len = k + 14 + 12 * ne;
        }
        int tot_len, tot_e;
        const int at = block_excl_scan(len, &tot_len, sh);
        const int eat = block_excl_scan(ne, &tot_e, sh);
        if (r < n) {
            uint8_t *b = rec + at;
            const uint8_t *kb = src >= 0 ? a.ref + src : a.seq + (-1 - src);
            for (int j = 0; j < k; ++j) b[j] = kb[j];
            b += k;
            b[0] = (uint8_t)col;
            put32(b + 1, (uint32_t)pos);
            put64(b + 5, nw);
            b[13] = (uint8_t)ne;
            b += 14;
            int32_t ends[4];
            for (int x = 0; x < ne; ++x) {
                ends[x] = t.rank[t.eend[kept[x]]];
                put32(b + 12 * x, (uint32_t)ends[x]);
                put64(b + 12 * x + 4, t.ew[kept[x]]);
            }
            const int64_t nslot = g.nodes ? g.node_off[blockIdx.x] + r : 0;
            if (g.nodes && nslot < g.node_off[blockIdx.x + 1]) {          // (the host entries check the counts; this bounds the writes)
                gbx_dbg_node nd;
                nd.weight = (int64_t)nw;
                nd.src = src >= 0 ? src + g.ref_shift : src - g.seq_shift;
                nd.first_edge = g.edge_off[blockIdx.x] + ebase + eat;
                nd.position = pos;
                nd.colours = (uint8_t)col;
                nd.n_edges = (uint8_t)ne;
                nd.pad_[0] = nd.pad_[1] = 0;
                g.nodes[nslot] = nd;
                for (int x = 0; x < ne && nd.first_edge + x < g.edge_off[blockIdx.x + 1]; ++x) {
                    gbx_dbg_edge ed;
                    ed.weight = (int64_t)t.ew[kept[x]];
                    ed.end = ends[x];
                    ed.pad_ = 0;
                    g.edges[nd.first_edge + x] = ed;
                }
            }
            atomicAdd(&acc[0], (unsigned long long)ne);
            atomicAdd(&acc[1], (unsigned long long)(d - ne));
            atomicAdd(&acc[2], (unsigned long long)occ);
            atomicAdd(&acc[3], (unsigned long long)wsum);
            atomicAdd(&acc[col == GBX_DBG_REF ? 4 : col == GBX_DBG_READ ? 5 : 6], 1ull);
        }
        ebase += tot_e;
        __syncthreads();
        if (tid == 0) {                                // the records of these ranks, in rank order, into the digest
            uint64_t h = s_digest;
            for (int x = 0; x < tot_len; ++x) h = (h ^ rec[x]) * FNV_PRIME;
            s_digest = h;
        }
        __syncthreads();
    }
    if (tid == 0 && stats) {
        gbx_dbg_stats st;
        st.n_nodes = n;
        st.n_edges = (int64_t)acc[0];
        st.n_dropped = (int64_t)acc[1];
        st.n_occ = (int64_t)acc[2];
        st.weight_sum = (int64_t)acc[3];
        st.n_ref = (int64_t)acc[4];
        st.n_read = (int64_t)acc[5];
        st.n_both = (int64_t)acc[6];
        st.digest = s_digest;
        stats[W.win] = st;
    }
}

}  // namespace

// Batches of plan (cut by dbg_cut_batches, dbg_plan.h) on stream s.  d_plan: room for the plan in the workspace; d_err: an int there.
int dbg_launch(const DbgDev &a, const std::vector<DbgWinPlan> &plan, const std::vector<int64_t> &batches, DbgWinPlan *d_plan, int *d_err,
               char *d_region, gbx_dbg_stats *d_stats, const DbgGraphOut &g, hipStream_t s)
{
    if (plan.empty()) return GBX_OK;
    GBX_HIP(hipMemcpyAsync(d_plan, plan.data(), plan.size() * sizeof(DbgWinPlan), hipMemcpyHostToDevice, s));
    for (size_t b = 0; b + 1 < batches.size(); ++b) {
        const int64_t p0 = batches[b], p1 = batches[b + 1], nw = p1 - p0;
        if (nw <= 0) continue;
        const int64_t total = plan[(size_t)p1 - 1].cand0 + plan[(size_t)p1 - 1].C;
        {
            Stage st_("dbg_init", s);
            dbg_init_kernel<<<(unsigned)nw, FIN_THREADS, 0, s>>>(d_plan + p0, d_region);
        }
        if (total > 0) {
            Stage st_("dbg_insert", s);
            dbg_insert_kernel<<<(unsigned)((total + INS_THREADS - 1) / INS_THREADS), INS_THREADS, 0, s>>>(a, d_plan + p0, (int)nw, total, d_region, d_err);
        }
        {
            Stage st_("dbg_finish", s);
            DbgGraphOut gg = g;
            if (g.nodes) { gg.node_off = g.node_off + p0; gg.edge_off = g.edge_off + p0; }
            dbg_finish_kernel<<<(unsigned)nw, FIN_THREADS, 0, s>>>(a, d_plan + p0, d_region, d_stats, gg);
        }
        GBX_HIP(hipGetLastError());
    }
    GBX_GUARD_CHECK("dbg_launch");
    return GBX_OK;
}

}  // namespace gbx
