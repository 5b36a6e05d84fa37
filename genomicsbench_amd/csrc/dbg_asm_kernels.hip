// dbg_asm_kernels.hip — Platypus's cycle check, start list and variant path search on the de Bruijn graphs of dbg_kernels.hip
// (R/benchmarks/dbg/debruijn.cpp:923-998, 1094-1239) for gfx950 (MI355X).
//
// Semantics: include/gbx.h, dbg_asm section.  The kernels read one range of windows whose graphs gbx_dbg's finish kernel has
// just written (gbx_dbg_node / gbx_dbg_edge at capacity offsets), in six launches per range, all but the first of one wavefront per workgroup:
//   cycle    one workgroup of four wavefronts per window.  In-degrees over the counted edges (atomicAdd).  These graphs are close
//            to a line, where peeling takes one node per trip, so the unary chains are contracted first: a node with one
//            counted edge in and one out (no self-loop) points at its successor, every other node at itself, and pointer
//            jumping in place (log2(n) + 2 rounds at most, early exit) makes every chain node point at the node behind its
//            chain.  A unary node that still points at a unary node lies on a ring of unary nodes: cyclic (a ring whose nodes
//            end up pointing at themselves is left to the peeling, which cannot take them: see the kernel).  Else Kahn's
//            peeling runs on the other nodes alone, over edges taken through the chains, by the first wavefront: the
//            nodes of in-degree 0 go to a list, up to 64 are taken per trip, each lane lowers its node's successors and appends
//            those that reach 0 at a ballot-ranked place; cyclic iff the list ends short of their number.  In-degrees, list and
//            pointers live in LDS up to DBG_ASM_LDS_NODES nodes, else in the workspace.  It also sets the window's k /
//            n_builds / cyclic, decides whether the graph is final (acyclic, or no retry left) and counts a final window's starts.
//   scan     one wavefront: the range's start counts to offsets behind the call's running total.
//   starts   one wavefront per final window: its starts, 64 nodes at a time in first-touch order, at ballot-ranked places.
//   search   one wavefront per start (grid-stride), run twice: the first run counts (status, paths, path nodes), a one-wavefront
//            pass turns the counts into offsets, the second run repeats the search (it is deterministic) and writes the
//            paths.  The LIFO stack of paths is a depth-first walk, so a path is its parent's prefix plus one node: the stack
//            holds (node, depth, weight) in LDS and the one current path lies in the wavefront's workspace slice; the 64 lanes
//            share the membership test of the new last node and the copy of a finished path.
// Loops: the peeling makes at most n trips, the search at most max_steps pops with a stack of at most max_pending + 4, the
// scans walk their counts 64 at a time; in the GBX_LOOP_GUARD build the peeling and the search count down as well (kernel 9,
// loops 4 and 5).
#include "gbx_internal.h"

namespace gbx {
namespace {

constexpr int WAVE = 64;
constexpr int STACK = GBX_DBG_ASM_MAX_PENDING + 5;
constexpr int CYC_THREADS = 256;

__device__ inline int32_t ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ inline void wave_sync() { __threadfence_block(); __syncthreads(); }      // in the kernels of one wavefront per workgroup
__device__ inline void block_sync() { __threadfence_block(); __syncthreads(); }
__device__ inline void wave_fence() { __threadfence_block(); __builtin_amdgcn_wave_barrier(); }       // one wavefront among several
__device__ inline int lanes_below(uint64_t mask) { return __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1)); }

__device__ inline bool counted(const gbx_dbg_node *nodes, const gbx_dbg_edge &e, int min_weight)
{
    return !(nodes[e.end].colours == GBX_DBG_READ && e.weight < (int64_t)min_weight);
}
// the start edges of node i: bit x set when edge x starts a path
__device__ inline int start_mask(const gbx_dbg_node *nodes, const gbx_dbg_edge *edges, int64_t i, int min_weight)
{
    const gbx_dbg_node &nd = nodes[i];
    int m = 0;
    if (nd.colours != (GBX_DBG_REF | GBX_DBG_READ)) return 0;
    for (int x = 0; x < nd.n_edges; ++x) {
        const gbx_dbg_edge &e = edges[nd.first_edge + x];
        if (nodes[e.end].colours == GBX_DBG_READ && e.weight >= (int64_t)min_weight) m |= 1 << x;
    }
    return m;
}

// the counted successors of node v: their number, the last one in *succ
__device__ inline int counted_out(const gbx_dbg_node *nodes, const gbx_dbg_edge *edges, int64_t v, int mw, int32_t *succ)
{
    const gbx_dbg_node nd = nodes[v];
    int out = 0;
    for (int x = 0; x < nd.n_edges; ++x) {
        const gbx_dbg_edge e = edges[nd.first_edge + x];
        if (counted(nodes, e, mw)) { ++out; *succ = e.end; }
    }
    return out;
}

__global__ void __launch_bounds__(CYC_THREADS) dbg_asm_cycle_kernel(DbgAsmDev a)
{
    __shared__ int32_t s_deg[DBG_ASM_LDS_NODES], s_list[DBG_ASM_LDS_NODES], s_nxt[DBG_ASM_LDS_NODES];
    __shared__ int s_ring, s_cyclic;
    __shared__ unsigned long long s_starts;
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int64_t win = a.plan[j].win, n = a.out.stats[win].n_nodes, nb = a.node_off[j];
    const gbx_dbg_node *nodes = a.nodes + nb;
    const gbx_dbg_edge *edges = a.edges;
    const bool lds = n <= DBG_ASM_LDS_NODES;
    int32_t *deg = lds ? s_deg : a.deg + nb, *list = lds ? s_list : a.list + nb, *nxt = lds ? s_nxt : a.nxt + nb;
    const int mw = a.ap.min_weight;
    if (tid == 0) { s_ring = 0; s_starts = 0; }
    // in-degrees over the counted edges
    for (int64_t i = tid; i < n; i += CYC_THREADS) st(&deg[i], 0);
    block_sync();
    for (int64_t i = tid; i < n; i += CYC_THREADS) {
        const gbx_dbg_node nd = nodes[i];
        for (int x = 0; x < nd.n_edges; ++x) {
            const gbx_dbg_edge e = edges[nd.first_edge + x];
            if (counted(nodes, e, mw)) atomicAdd(&deg[e.end], 1);
        }
    }
    block_sync();
    // unary nodes (one counted edge in, one out, no self-loop) point at their successor, every other node at itself
    for (int64_t i = tid; i < n; i += CYC_THREADS) {
        int32_t succ = (int32_t)i;
        const int out = counted_out(nodes, edges, i, mw, &succ);
        st(&nxt[i], ld(&deg[i]) == 1 && out == 1 ? succ : (int32_t)i);
    }
    block_sync();
    // pointer jumping, in place: a chain of m unary nodes points at the node behind it after log2(m) + 1 rounds
    int rounds = 2;
    for (int64_t m = 1; m < n; m <<= 1) ++rounds;
    for (int r = 0; r < rounds; ++r) {                      // bounded by log2(n) + 2; ends early once nothing moves
        bool moved = false;
        for (int64_t i = tid; i < n; i += CYC_THREADS) {
            const int32_t t = ld(&nxt[i]), u = ld(&nxt[t]);
            if (u != t) { st(&nxt[i], u); moved = true; }
        }
        __threadfence_block();
        if (!__syncthreads_or(moved)) break;                // the barrier between rounds, and one answer for every wavefront
    }
    // Rings of unary nodes.  Jumping never ends on one, so behind the rounds a ring shows in one of two ways.  A unary node
    // that still points at a node that points elsewhere lies on a ring: s_ring.  Or the in-place jumps have made ring nodes
    // point at themselves (a ring of two: 0 -> 1 -> 0 becomes 0 -> 0; any ring whose jumps land on their own node, a power
    // of two for one), and the rest of the ring at those.  Such a node then passes for one that is not unary, and its one
    // edge leads, through its successor's pointer, to a self-pointing node of the same ring: among them every node has an
    // edge into the set, so the set holds a cycle of the contracted graph, none of them ever reaches in-degree 0 and the
    // peeling ends short.  A ring has no edge in or out, so nothing else is touched.  Either way: cyclic.
    // Then the other nodes' in-degrees over the contracted edges (through a chain to the node behind it).
    for (int64_t i = tid; i < n; i += CYC_THREADS) {
        const int32_t t = ld(&nxt[i]);
        if (ld(&nxt[t]) != t) s_ring = 1;
        st(&deg[i], 0);
    }
    block_sync();
    for (int64_t i = tid; i < n; i += CYC_THREADS) {
        if (ld(&nxt[i]) != (int32_t)i) continue;
        const gbx_dbg_node nd = nodes[i];
        for (int x = 0; x < nd.n_edges; ++x) {
            const gbx_dbg_edge e = edges[nd.first_edge + x];
            if (counted(nodes, e, mw)) atomicAdd(&deg[ld(&nxt[e.end])], 1);
        }
    }
    block_sync();
    // Kahn's peeling over the nodes that are not unary, by the first wavefront
    if (tid < WAVE && !s_ring) {
        int64_t head = 0, tail = 0, total = 0;
        for (int64_t i0 = 0; i0 < n; i0 += WAVE) {
            const int64_t i = i0 + lane;
            const bool mine = i < n && ld(&nxt[i]) == (int32_t)i, z = mine && ld(&deg[i]) == 0;
            const uint64_t mask = __ballot(z);
            if (z) st(&list[tail + lanes_below(mask)], (int32_t)i);
            tail += __popcll(mask);
            total += __popcll(__ballot(mine));
        }
        wave_fence();
        GBX_GUARD(gd, n);
        while (head < tail) {                               // every trip takes at least one node: at most n trips
            if (GBX_GUARD_TRIP(gd, GBX_GK_DBG, 4, win)) break;
            const int64_t m = imin64(WAVE, tail - head);
            const int32_t v = lane < m ? ld(&list[head + lane]) : -1;
            head += m;
            int ne = 0;
            int64_t fe = 0;
            if (v >= 0) { ne = nodes[v].n_edges; fe = nodes[v].first_edge; }
            for (int x = 0; x < 4; ++x) {
                bool push = false;
                int32_t end = -1;
                if (x < ne) {
                    const gbx_dbg_edge e = edges[fe + x];
                    if (counted(nodes, e, mw)) { end = ld(&nxt[e.end]); push = atomicSub(&deg[end], 1) == 1; }
                }
                const uint64_t mask = __ballot(push);
                if (push && tail + lanes_below(mask) < n) st(&list[tail + lanes_below(mask)], end);   // (a node enters once: the bound never binds)
                tail += __popcll(mask);
            }
            wave_fence();
        }
        if (lane == 0) s_cyclic = tail != total;
    }
    block_sync();
    const int cyclic = s_ring || s_cyclic;
    const bool fin = !cyclic || a.last_round;
    // a final window's starts
    if (fin) {
        unsigned long long cnt = 0;
        for (int64_t i = tid; i < n; i += CYC_THREADS) cnt += __popc(start_mask(nodes, edges, i, mw));
        if (cnt) atomicAdd(&s_starts, cnt);
    }
    block_sync();
    if (tid == 0) {
        const int64_t cnt = (int64_t)s_starts;
        a.cyc[win] = cyclic;
        a.win_slot[win] = j;
        a.fin[j] = fin;
        a.wstart[j] = cnt;
        gbx_dbg_asm_win w;
        w.k = a.k; w.n_builds = a.n_builds; w.cyclic = cyclic; w.pad_ = 0;
        w.first_start = 0; w.n_starts = cnt;
        w.n_paths = w.n_path_nodes = w.n_gave_up = w.n_steps = 0;
        a.out.wins[win] = w;
    }
}

// exclusive scan of v over the wavefront; *total = the sum
__device__ inline int64_t wave_excl_scan(int64_t v, int64_t *total)
{
    const int lane = threadIdx.x & 63;
    int64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    *total = __shfl(inc, 63, 64);
    return inc - v;
}

// wstart[j]: counts -> the first start of window j in the call's start array; counters[3] = the range's first start
__global__ void __launch_bounds__(WAVE) dbg_asm_scan_kernel(DbgAsmDev a)
{
    const int lane = threadIdx.x;
    const int64_t base = a.counters[0];
    int64_t run = base;
    for (int j0 = 0; j0 < a.nw; j0 += WAVE) {
        const int j = j0 + lane;
        const int64_t c = j < a.nw ? a.wstart[j] : 0;
        int64_t tot;
        const int64_t at = run + wave_excl_scan(c, &tot);
        if (j < a.nw) {
            a.wstart[j] = at;
            if (a.fin[j]) a.out.wins[a.plan[j].win].first_start = at;
        }
        run += tot;
    }
    __syncthreads();
    if (lane == 0) { a.counters[3] = base; a.counters[0] = run; }
}

__global__ void __launch_bounds__(WAVE) dbg_asm_starts_kernel(DbgAsmDev a)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    if (!a.fin[j]) return;
    const int64_t win = a.plan[j].win, n = a.out.stats[win].n_nodes;
    const gbx_dbg_node *nodes = a.nodes + a.node_off[j];
    int64_t run = a.wstart[j];
    for (int64_t i0 = 0; i0 < n; i0 += WAVE) {
        const int64_t i = i0 + lane;
        const int m = i < n ? start_mask(nodes, a.edges, i, a.ap.min_weight) : 0;
        int64_t tot;
        int64_t at = run + wave_excl_scan(__popc(m), &tot);
        for (int x = 0; x < 4; ++x)
            if (m >> x & 1) {
                if (at < a.out.cap_starts) {
                    gbx_dbg_asm_start sr;
                    sr.first_path = sr.n_paths = sr.first_node = sr.n_nodes = 0;
                    sr.win = (int32_t)win; sr.node = (int32_t)i; sr.edge = x; sr.status = GBX_DBG_ASM_OK;
                    a.out.starts[at] = sr;
                }
                ++at;
            }
        run += tot;
    }
}

// One search per wavefront.  FILL = false: status and counts into the start; true: the paths of a start of status OK.
template <bool FILL>
__global__ void __launch_bounds__(WAVE) dbg_asm_search_kernel(DbgAsmDev a)
{
    __shared__ int32_t st_node[STACK], st_depth[STACK];
    __shared__ int64_t st_w[STACK];
    const int lane = threadIdx.x;
    const int64_t s0 = a.counters[3], s1 = imin64(a.counters[0], a.out.cap_starts);
    int32_t *cur = a.pathbuf + (int64_t)blockIdx.x * a.path_slice;
    const int mw = a.ap.min_weight;
    for (int64_t s = s0 + blockIdx.x; s < s1; s += gridDim.x) {
        gbx_dbg_asm_start sr = a.out.starts[s];
        if (FILL && sr.status != GBX_DBG_ASM_OK) continue;
        const int j = a.win_slot[sr.win];
        const gbx_dbg_node *nodes = a.nodes + a.node_off[j];
        const gbx_dbg_edge *edges = a.edges;
        __syncthreads();
        if (lane == 0) {
            const gbx_dbg_edge e = edges[nodes[sr.node].first_edge + sr.edge];
            st_node[0] = e.end; st_depth[0] = 1; st_w[0] = e.weight;
            st(&cur[0], sr.node);
        }
        wave_sync();
        int sp = 1, status = GBX_DBG_ASM_OK;
        int64_t steps = 0, nfin = 0, nn = 0;
        GBX_GUARD(gd, a.ap.max_steps + 1);
        while (sp > 0) {
            if (GBX_GUARD_TRIP(gd, GBX_GK_DBG, 5, s)) break;
            --sp;
            const int32_t node = st_node[sp], d = st_depth[sp];
            const int64_t w = st_w[sp];
            if (++steps > a.ap.max_steps) { status = GBX_DBG_ASM_STEPS; break; }
            if (sp > a.ap.max_pending || nfin > a.ap.max_finished) { status = GBX_DBG_ASM_GAVE_UP; break; }
            bool hit = false;
            for (int i = lane; i < d; i += WAVE) hit |= ld(&cur[i]) == node;
            if (__ballot(hit)) continue;                      // the path holds its last node twice: dropped
            const gbx_dbg_node nd = nodes[node];
            if (nd.colours == (GBX_DBG_REF | GBX_DBG_READ)) {       // back on the reference: finished
                if (FILL) {
                    const int64_t pi = sr.first_path + nfin, n0 = sr.first_node + nn;
                    for (int i = lane; i <= d; i += WAVE) {
                        const int32_t v = i < d ? ld(&cur[i]) : node;
                        if (n0 + i < a.out.cap_path_nodes) {
                            const int64_t src = nodes[v].src;
                            a.out.path_nodes[n0 + i] = v;
                            a.out.path_seq[n0 + i] = src >= 0 ? a.ref[src] : a.seq[-1 - src];
                        }
                    }
                    if (lane == 0 && pi < a.out.cap_paths) {
                        gbx_dbg_asm_path p;
                        p.weight = w; p.first_node = n0; p.n_nodes = d + 1;
                        p.pos_first = nodes[sr.node].position; p.pos_last = nd.position; p.pad_ = 0;
                        a.out.paths[pi] = p;
                    }
                }
                ++nfin;
                nn += d + 1;
                continue;
            }
            if (nd.colours == GBX_DBG_REF) continue;          // reference only: dropped
            __syncthreads();                                  // (every lane has read this pop's stack entry)
            if (lane == 0) {
                st(&cur[d], node);
                int q = sp;
                for (int x = 0; x < nd.n_edges; ++x) {
                    const gbx_dbg_edge e = edges[nd.first_edge + x];
                    if (e.weight >= (int64_t)mw || (nodes[e.end].colours & GBX_DBG_REF)) {
                        st_node[q] = e.end; st_depth[q] = d + 1; st_w[q] = w + e.weight;
                        ++q;
                    }
                }
                st_depth[STACK - 1] = q;                      // (never a live entry: sp <= max_pending + 4 < STACK - 1)
            }
            wave_sync();
            sp = st_depth[STACK - 1];
        }
        if (!FILL && lane == 0) {
            const bool ok = status == GBX_DBG_ASM_OK;
            sr.status = status;
            sr.n_paths = ok ? nfin : 0;
            sr.n_nodes = ok ? nn : 0;
            a.out.starts[s] = sr;
        }
    }
}

// the range's starts: counts -> first_path / first_node behind the call's running totals; the windows' sums
__global__ void __launch_bounds__(WAVE) dbg_asm_offsets_kernel(DbgAsmDev a)
{
    const int lane = threadIdx.x;
    const int64_t s0 = a.counters[3], s1 = imin64(a.counters[0], a.out.cap_starts);
    int64_t pr = a.counters[1], nr = a.counters[2];
    for (int64_t c0 = s0; c0 < s1; c0 += WAVE) {
        const int64_t s = c0 + lane;
        gbx_dbg_asm_start sr;
        sr.n_paths = sr.n_nodes = 0;
        if (s < s1) sr = a.out.starts[s];
        int64_t tp, tn;
        const int64_t ap = pr + wave_excl_scan(sr.n_paths, &tp), an = nr + wave_excl_scan(sr.n_nodes, &tn);
        if (s < s1) {
            a.out.starts[s].first_path = ap;
            a.out.starts[s].first_node = an;
            gbx_dbg_asm_win *w = a.out.wins + sr.win;
            if (sr.n_paths) atomicAdd((unsigned long long *)&w->n_paths, (unsigned long long)sr.n_paths);
            if (sr.n_nodes) atomicAdd((unsigned long long *)&w->n_path_nodes, (unsigned long long)sr.n_nodes);
            if (sr.status == GBX_DBG_ASM_GAVE_UP) atomicAdd((unsigned long long *)&w->n_gave_up, 1ull);
            if (sr.status == GBX_DBG_ASM_STEPS) atomicAdd((unsigned long long *)&w->n_steps, 1ull);
        }
        pr += tp; nr += tn;
    }
    __syncthreads();
    if (lane == 0) { a.counters[1] = pr; a.counters[2] = nr; }
}

}  // namespace

int dbg_asm_launch(const DbgAsmDev &a, hipStream_t s)
{
    if (a.nw <= 0) return GBX_OK;
    {
        Stage st_("dbg_asm_cycle", s);
        dbg_asm_cycle_kernel<<<(unsigned)a.nw, CYC_THREADS, 0, s>>>(a);
    }
    {
        Stage st_("dbg_asm_starts", s);
        dbg_asm_scan_kernel<<<1, WAVE, 0, s>>>(a);
        dbg_asm_starts_kernel<<<(unsigned)a.nw, WAVE, 0, s>>>(a);
    }
    {
        Stage st_("dbg_asm_search", s);
        dbg_asm_search_kernel<false><<<(unsigned)a.path_blocks, WAVE, 0, s>>>(a);
        dbg_asm_offsets_kernel<<<1, WAVE, 0, s>>>(a);
        dbg_asm_search_kernel<true><<<(unsigned)a.path_blocks, WAVE, 0, s>>>(a);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("dbg_asm_launch");
    return GBX_OK;
}

}  // namespace gbx
