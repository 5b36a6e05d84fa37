// mem_chain_kernels.hip — seed chaining between the suffix-array lookup and the seed extension (bwa-mem's mem_chain,
// mem_chain_flt and the window of mem_chain2aln) for gfx950 (MI355X).
//
// Semantics: include/gbx.h and DESIGN 3.10 (restated in tests/mem_chain_ref.py, which pins them).
//
// Shape: one read per wavefront.  A read's seeds arrive in a fixed order and every insertion depends on the one before, so a
// read is serial in its seeds; what is parallel is the chain set (the look-up of `lower`, the insertion, the weight sort, the
// overlap scan of the filter) and, in the pack pass, the hits.  The control flow of a wavefront is uniform: every lane
// carries the seed and the chain it is tested against, lane 0 stores, and a barrier (free for a one-wave block) orders the
// store before the next seed's loads.
//   * All per-read state lives in slabs of the workspace indexed by the read's first hit: a read has at most as many
//     chains as hits, so slab h0 .. h0 + hits of every per-chain array is its own, whatever the count - no capacity
//     a read could exceed, no second path.
//   * chain heads: (pos, id) sorted by (pos, creation).  `lower` is the last head with pos <= rbeg: a bisection down to 64
//     heads, then one compare per lane and a ballot.  A new chain shifts the heads above it up by one, 64 at a time from the top.
//   * a seed keeps only its chain's id and its index in the chain; weight, query / reference cover and the window's min /
//     max are kept per chain as the seeds join (they join in order), so no pass walks a chain's seeds again.
//   * weight sort: 64-bit keys (2^30 - 1 - weight, head index), unique, so any correct sort gives the same order - in
//     registers with shuffles up to 64 chains, a bitonic network over the slab above that.
//   * the filter's K scan is serial in i and parallel in j; the lowest stopping j comes from a ballot and `first` is set
//     only for the js up to it.
//   * output: the read kernel leaves per-read counts, a scan over the reads turns them into offsets (chain_off), a pack
//     pass writes chain and seed records at their final places: the output does not depend on the scheduling.
#include <algorithm>
#include "mem_common.h"

namespace gbx {
namespace {

constexpr int MC_WMAX = (1 << 30) - 1;

struct McHit { int cid, idx, qbeg, len; };          // per hit: its chain (creation id, -1: none) and place in it
struct McChainSt {                                  // per chain, 96 bytes
    long long pos, l_rbeg, endr, rmin, rmax;        // first.rbeg; last.rbeg; reference cover end; window candidates
    int f_qbeg, l_qbeg, l_len, contig, nseeds, endq, wq, wr, weight, first, kept, out_idx, out_soff, pad_;
};
static_assert(sizeof(McChainSt) == 96, "McChainSt");
static_assert(sizeof(gbx_mem_chain) == 56 && sizeof(gbx_bsw_seed) == 40, "records");

struct McArgs {
    gbx_mem_chain_params p;
    MemChainIo io;
    long long n_reads;
    long long *cnt;                  // [2][n_reads + 1]: kept chains / seeds per read, then their exclusive scan
    int *nch;                        // [n_reads]: chains a read made (kept or not)
    McHit *hit;                      // [pos_cap]
    McChainSt *ch;                   // [pos_cap]   slab of a read: its first hit
    long long *spos;                 // [pos_cap]   sorted heads
    int *sid, *ord, *K;              // [pos_cap]   sorted heads' ids; chain at rank i of the weight order; the filter's K
    unsigned long long *key;         // [2 pos_cap] slab at twice the first hit: the sort pads to a power of two
};

struct McSpan { long long j0, j1, hb, he; };
__device__ inline McSpan mc_span(const McArgs &A, long long r)
{
    const long long n_smem = clampll(*A.io.n_smem, 0, A.io.smem_cap), n_pos = clampll(*A.io.n_pos, 0, A.io.pos_cap);
    McSpan s;
    s.j0 = clampll(A.io.smem_off[r], 0, n_smem);
    s.j1 = clampll(A.io.smem_off[r + 1], s.j0, n_smem);
    s.hb = clampll(A.io.pos_off[s.j0], 0, n_pos);
    s.he = clampll(A.io.pos_off[s.j1], s.hb, n_pos);
    return s;
}

// bns_intv2rid of [rb, re): the contig, or -1 when the interval crosses L or a contig boundary
__device__ inline int mc_contig(const McArgs &A, long long rb, long long re)
{
    const long long L = A.io.l_pac;
    if (rb < L && L < re) return -1;
    long long b = rb, e = re;
    if (re > L) { b = 2 * L - re; e = 2 * L - rb; }
    int lo = 0, hi = A.io.n_contigs + 1;            // the first entry above b
    for (int it = 0; it < 32; ++it) {
        if (lo >= hi) break;
        const int mid = (lo + hi) >> 1;
        if (A.io.contig_off[mid] <= b) lo = mid + 1; else hi = mid;
    }
    const int c = lo - 1;
    if (c < 0 || c >= A.io.n_contigs) return -1;
    return e <= A.io.contig_off[c + 1] ? c : -1;
}

// the seed joins the chain's running sums: query and reference cover, window candidates, last seed
__device__ inline void mc_join(McChainSt &C, int qbeg, int len, long long rbeg, int lq, const gbx_mem_chain_params &p)
{
    const int qe = qbeg + len;
    if (qbeg >= C.endq) C.wq += len; else if (qe > C.endq) C.wq += qe - C.endq;
    C.endq = qe > C.endq ? qe : C.endq;
    const long long re = rbeg + len;
    long long add = 0;
    if (rbeg >= C.endr) add = len; else if (re > C.endr) add = re - C.endr;
    const long long wr = (long long)C.wr + add;
    C.wr = wr > 0x7fffffffll ? 0x7fffffff : (int)wr;          // (saturates above every possible wq: the minimum is exact)
    C.endr = re > C.endr ? re : C.endr;
    const long long lo = rbeg - (qbeg + max_gap(qbeg, p));
    const long long rest = (long long)lq - qe;
    const long long hi = re + rest + max_gap(rest, p);
    C.rmin = lo < C.rmin ? lo : C.rmin;
    C.rmax = hi > C.rmax ? hi : C.rmax;
    C.l_qbeg = qbeg; C.l_len = len; C.l_rbeg = rbeg;
    ++C.nseeds;
}

// ---- chaining, weights, filter and windows of one read; leaves the read's counts and its state in the slabs
__global__ void __launch_bounds__(64) mem_chain_read_kernel(McArgs A)
{
    const long long r = blockIdx.x;
    const int lane = threadIdx.x;
    const gbx_mem_chain_params p = A.p;
    const McSpan S = mc_span(A, r);
    const long long L = A.io.l_pac;
    const int lq = A.io.read_len[r];
    McChainSt *const ch = A.ch + S.hb;
    long long *const spos = A.spos + S.hb;
    int *const sid = A.sid + S.hb, *const ord = A.ord + S.hb, *const K = A.K + S.hb;
    unsigned long long *const key = A.key + 2 * S.hb;

    // ---- 1, 2: l_rep and chaining, serial in the seeds
    int nch = 0;
    int rep_b = 0, rep_e = 0, l_rep = 0;
    for (long long j = S.j0; j < S.j1; ++j) {
        const gbx_fmi_smem sm = A.io.smems[j];
        const int qbeg = (int)sm.m, len = (int)sm.n + 1 - (int)sm.m;
        if (sm.s > p.max_occ) {
            const int sb = qbeg, se = (int)sm.n + 1;
            if (sb > rep_e) { l_rep += rep_e - rep_b; rep_b = sb; rep_e = se; }
            else rep_e = rep_e > se ? rep_e : se;
        }
        const long long a = clampll(A.io.pos_off[j], S.hb, S.he), e = clampll(A.io.pos_off[j + 1], a, S.he);
        for (long long h = a; h < e; ++h) {
            const long long rbeg = A.io.pos[h];
            McHit rec = {-1, 0, qbeg, len};
            const int c = rbeg >= 0 && len >= 1 && qbeg >= 0 ? mc_contig(A, rbeg, rbeg + len) : -1;
            if (c >= 0) {
                // heads with pos <= rbeg: bisect to 64, then a compare per lane
                int lo = 0, hi = nch;
                for (int it = 0; it < 32; ++it) {
                    if (hi - lo <= 64) break;
                    const int mid = (lo + hi) >> 1;
                    if (spos[mid] <= rbeg) lo = mid + 1; else hi = mid;
                }
                const bool le = lo + lane < hi && spos[lo + lane] <= rbeg;
                const int at = lo + __builtin_popcountll(__ballot(le));
                bool merged = false;
                if (at > 0) {
                    const int lc = sid[at - 1];
                    McChainSt C = ch[lc];
                    __builtin_amdgcn_wave_barrier();                             // (every lane has the chain before lane 0 stores it)
                    if (c == C.contig) {
                        const bool inside = qbeg >= C.f_qbeg && qbeg + len <= C.l_qbeg + C.l_len && rbeg >= C.pos &&
                                            rbeg + len <= C.l_rbeg + C.l_len;
                        if (inside) merged = true;                               // contained: dropped
                        else if (!((C.l_rbeg < L || C.pos < L) && rbeg >= L)) {
                            const long long x = qbeg - C.l_qbeg, y = rbeg - C.l_rbeg;
                            if (y >= 0 && x - y <= p.w && y - x <= p.w && x - C.l_len < p.max_chain_gap && y - C.l_len < p.max_chain_gap) {
                                rec.cid = lc; rec.idx = C.nseeds;
                                mc_join(C, qbeg, len, rbeg, lq, p);
                                if (lane == 0) ch[lc] = C;
                                merged = true;
                            }
                        }
                    }
                }
                if (!merged) {
                    // heads [at, nch) move up by one, 64 at a time from the top (a block's loads are all back before its stores)
                    for (int top = nch; top > at; top -= 64) {
                        const int i = top - 1 - lane;
                        const bool act = i >= at;
                        const long long v = act ? spos[i] : 0;
                        const int w = act ? sid[i] : 0;
                        __builtin_amdgcn_wave_barrier();                         // (no instruction: keeps the stores below the loads)
                        if (act) { spos[i + 1] = v; sid[i + 1] = w; }
                    }
                    McChainSt C;
                    C.pos = rbeg; C.l_rbeg = rbeg; C.endr = 0; C.rmin = 0x7fffffffffffffffll; C.rmax = -0x7fffffffffffffffll;
                    C.f_qbeg = qbeg; C.l_qbeg = qbeg; C.l_len = len; C.contig = c; C.nseeds = 0; C.endq = 0; C.wq = 0; C.wr = 0;
                    C.weight = 0; C.first = -1; C.kept = 0; C.out_idx = -1; C.out_soff = 0; C.pad_ = 0;
                    mc_join(C, qbeg, len, rbeg, lq, p);
                    if (lane == 0) { spos[at] = rbeg; sid[at] = nch; ch[nch] = C; }
                    rec.cid = nch; rec.idx = 0;
                    ++nch;
                }
            }
            if (lane == 0) A.hit[h] = rec;
            __syncthreads();
        }
    }
    l_rep += rep_e - rep_b;

    // ---- 3: weights and sort keys, by head index (the order the filter breaks ties by)
    const bool small = nch <= 64;
    int P = 1;
    for (int it = 0; it < 31; ++it) { if (P >= nch) break; P <<= 1; }
    int m = 0;
    unsigned long long v = ~0ull;
    for (int b0 = 0; b0 < (small ? 64 : P); b0 += 64) {
        const int si = b0 + lane;
        unsigned long long k = ~0ull;
        if (si < nch) {
            const int c = sid[si];
            const int wq = ch[c].wq, wr = ch[c].wr;
            int w = wq < wr ? wq : wr;
            w = w < MC_WMAX ? w : MC_WMAX;
            ch[c].weight = w;
            if (w >= p.min_chain_weight) k = (unsigned long long)(MC_WMAX - w) << 32 | (unsigned)si;
        }
        m += __builtin_popcountll(__ballot(k != ~0ull));
        if (small) v = k; else key[si] = k;
    }
    __syncthreads();
    // ---- ascending sort of the unique keys: weight descending, ties by head index
    if (small) {
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const unsigned long long o = __shfl_xor(v, j);
                const bool up = (lane & k) == 0, lower = (lane & j) == 0;
                v = (lower == up) ? (v < o ? v : o) : (v > o ? v : o);
            }
        if (lane < m) ord[lane] = sid[(unsigned)v];
    } else {
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;
                    const unsigned long long x = key[i], y = key[o];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { key[i] = y; key[o] = x; }
                }
                __syncthreads();
            }
        for (int i = lane; i < m; i += 64) ord[i] = sid[(unsigned)key[i]];
    }
    __syncthreads();

    // ---- 4: mem_chain_flt.  K holds chain ids; `first` the chain id of the first chain a kept one shadows
    int nK = 0;
    if (m > 0) {
        if (lane == 0) { K[0] = ord[0]; ch[ord[0]].kept = 3; }
        nK = 1;
        __syncthreads();
    }
    for (int i = 1; i < m; ++i) {
        const int ci = ord[i];
        const int bi = ch[ci].f_qbeg, ei = ch[ci].l_qbeg + ch[ci].l_len, wi = ch[ci].weight;
        bool large = false, stopped = false;
        for (int jb = 0; jb < nK; jb += 64) {
            const int j = jb + lane;
            bool ov = false, stop = false;
            int cj = 0;
            if (j < nK) {
                cj = K[j];
                const int bj = ch[cj].f_qbeg, ej = ch[cj].l_qbeg + ch[cj].l_len, wj = ch[cj].weight;
                const int b_max = bj > bi ? bj : bi, e_min = ej < ei ? ej : ei;
                if (e_min > b_max) {
                    const int li = ei - bi, lj = ej - bj, min_l = li < lj ? li : lj;
                    if ((float)(e_min - b_max) >= (float)min_l * p.mask_level && min_l < p.max_chain_gap) {
                        ov = true;
                        stop = (float)wi < (float)wj * p.drop_ratio && wj - wi >= 2 * p.min_seed_len;
                    }
                }
            }
            const unsigned long long bs = __ballot(stop);
            const int ls = bs ? __builtin_ctzll(bs) : 64;
            const bool eff = ov && lane <= ls;
            if (eff && ch[cj].first < 0) ch[cj].first = ci;
            if (__ballot(eff)) large = true;
            if (bs) { stopped = true; break; }
        }
        if (!stopped) {
            if (lane == 0) { K[nK] = ci; ch[ci].kept = large ? 2 : 3; }
            ++nK;
        }
        __syncthreads();
    }
    for (int j = lane; j < nK; j += 64) {
        const int f = ch[K[j]].first;
        if (f >= 0) ch[f].kept = 1;
    }
    __syncthreads();
    // the max_chain_extend cap: after the chain that brings the count of kept 1 / 2 chains to the cap, only kept 3 stays
    {
        long long k = 0;
        int stop_rank = -1;
        for (int b0 = 0; b0 < m; b0 += 64) {
            const int i = b0 + lane;
            const int c = i < m ? ord[i] : 0;
            const int kept = i < m ? ch[c].kept : 0;
            const bool flag = kept == 1 || kept == 2;
            const unsigned long long bf = __ballot(flag);
            if (stop_rank < 0) {
                const int pre = __builtin_popcountll(bf & (~0ull >> (63 - lane)));
                const unsigned long long bh = __ballot(flag && k + pre >= p.max_chain_extend);
                if (bh) stop_rank = b0 + __builtin_ctzll(bh);
            }
            k += __builtin_popcountll(bf);
            if (stop_rank >= 0 && i < m && i > stop_rank && kept < 3) ch[c].kept = 0;
        }
    }
    __syncthreads();

    // ---- 5, 6: windows of the kept chains, their places in the read's output, the read's counts
    int n_out = 0, n_seeds = 0;
    for (int b0 = 0; b0 < m; b0 += 64) {
        const int i = b0 + lane;
        const int c = i < m ? ord[i] : 0;
        const bool out = i < m && ch[c].kept > 0;
        const int ns = out ? ch[c].nseeds : 0;
        const unsigned long long bo = __ballot(out);
        const int incl = wave_scan_incl(ns, lane);
        if (out) {
            long long r0 = ch[c].rmin, r1 = ch[c].rmax;
            r0 = clampll(r0, 0, 2 * L); r1 = clampll(r1, 0, 2 * L);
            const bool fwd = ch[c].pos < L;
            if (r0 < L && L < r1) { if (fwd) r1 = L; else r0 = L; }
            const int cg = ch[c].contig;
            const long long c0 = A.io.contig_off[cg], c1 = A.io.contig_off[cg + 1];
            const long long lo = fwd ? c0 : 2 * L - c1, hi = fwd ? c1 : 2 * L - c0;
            r0 = r0 > lo ? r0 : lo; r1 = r1 < hi ? r1 : hi;
            ch[c].rmin = r0; ch[c].rmax = r1;
            ch[c].out_idx = n_out + __builtin_popcountll(bo & ((1ull << lane) - 1));
            ch[c].out_soff = n_seeds + incl - ns;
        }
        n_out += __builtin_popcountll(bo);
        n_seeds += __shfl(incl, 63);
    }
    if (lane == 0) {
        A.cnt[r] = n_out;
        A.cnt[A.n_reads + 1 + r] = n_seeds;
        A.nch[r] = nch;
        A.io.l_rep[r] = l_rep;
    }
}

// ---- the records at their final places: lanes over the read's chains, then over its hits
__global__ void __launch_bounds__(64) mem_chain_pack_kernel(McArgs A)
{
    const long long r = blockIdx.x;
    const int lane = threadIdx.x;
    const McSpan S = mc_span(A, r);
    const McChainSt *const ch = A.ch + S.hb;
    const long long cbase = A.cnt[r], sbase = A.cnt[A.n_reads + 1 + r];
    const int nch = A.nch[r];
    for (int c = lane; c < nch; c += 64) {
        const McChainSt C = ch[c];
        if (C.out_idx < 0) continue;
        const long long g = cbase + C.out_idx;
        if (g < 0 || g >= A.io.chain_cap) continue;
        gbx_mem_chain o;
        o.pos = C.pos; o.seed_off = sbase + C.out_soff; o.rmax0 = C.rmin; o.rmax1 = C.rmax;
        o.read = (int32_t)r; o.contig = C.contig; o.n_seeds = C.nseeds; o.weight = C.weight; o.kept = C.kept; o.pad_ = 0;
        A.io.chains[g] = o;
    }
    const long long qoff = A.io.read_off[r];
    const int lq = A.io.read_len[r];
    for (long long h = S.hb + lane; h < S.he; h += 64) {
        const McHit rec = A.hit[h];
        if (rec.cid < 0 || rec.cid >= nch) continue;
        const McChainSt &C = ch[rec.cid];
        if (C.out_idx < 0) continue;
        const long long g = sbase + C.out_soff + rec.idx;
        if (g < 0 || g >= A.io.seed_cap) continue;
        gbx_bsw_seed s;
        s.qoff = qoff; s.roff = C.rmin; s.lq = lq; s.rlen = (int32_t)(C.rmax - C.rmin);
        s.qbeg = rec.qbeg; s.rbeg = (int32_t)(A.io.pos[h] - C.rmin); s.len = rec.len; s.pad_ = 0;
        A.io.seeds[g] = s;
    }
}

// the seed records past the count, up to the capacity: zero (len = 0 is no seed: the extension answers -1)
__global__ void __launch_bounds__(256) mem_chain_tail_kernel(McArgs A)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;              // 8-byte words, five a record
    const long long n = *A.io.n_seeds;
    if (t >= A.io.seed_cap * 5 || t < (n < 0 ? 0 : n) * 5) return;
    ((long long *)A.io.seeds)[t] = 0;
}

struct McLayout { size_t o_cnt, o_bsum, o_nch, o_hit, o_ch, o_spos, o_sid, o_ord, o_K, o_key, total; int blocks; };
McLayout mc_layout(int64_t n_reads, int64_t pos_cap)
{
    McLayout L;
    const size_t nr = (size_t)n_reads, np = (size_t)pos_cap;
    L.blocks = mem_scan_blocks(n_reads);
    L.o_cnt = 0;
    L.o_bsum = L.o_cnt + align256(2 * (nr + 1) * 8);
    L.o_nch = L.o_bsum + align256(2 * (size_t)L.blocks * 8);
    L.o_hit = L.o_nch + align256(nr * 4);
    L.o_ch = L.o_hit + align256(np * sizeof(McHit));
    L.o_spos = L.o_ch + align256(np * sizeof(McChainSt));
    L.o_sid = L.o_spos + align256(np * 8);
    L.o_ord = L.o_sid + align256(np * 4);
    L.o_K = L.o_ord + align256(np * 4);
    L.o_key = L.o_K + align256(np * 4);
    L.total = L.o_key + align256(2 * np * 8);
    return L;
}

}  // namespace

size_t mem_chain_workspace_bytes(int64_t n_reads, int64_t, int64_t pos_cap)
{
    return mc_layout(n_reads < 0 ? 0 : n_reads, pos_cap < 0 ? 0 : pos_cap).total;
}

int mem_chain_launch(const gbx_mem_chain_params *p, int64_t n_reads, const MemChainIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    if (n_reads >= (1ll << 31) - 1) { set_error("mem chain: more than 2^31 - 2 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    const McLayout L = mc_layout(n_reads, io.pos_cap);
    if (work_bytes < L.total) { set_error("mem chain: workspace too small"); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    McArgs A;
    A.p = *p; A.io = io; A.n_reads = n_reads;
    A.cnt = (long long *)(wb + L.o_cnt); A.nch = (int *)(wb + L.o_nch);
    A.hit = (McHit *)(wb + L.o_hit); A.ch = (McChainSt *)(wb + L.o_ch); A.spos = (long long *)(wb + L.o_spos);
    A.sid = (int *)(wb + L.o_sid); A.ord = (int *)(wb + L.o_ord); A.K = (int *)(wb + L.o_K);
    A.key = (unsigned long long *)(wb + L.o_key);
    if (n_reads > 0) {
        Stage st("mem_chain_read", s);
        hipLaunchKernelGGL(mem_chain_read_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, A);
    }
    {
        Stage st("mem_chain_scan", s);
        mem_scan_launch({A.cnt, n_reads, 2, (long long *)(wb + L.o_bsum), L.blocks, {io.n_chains, io.n_seeds}, io.chain_off, {}}, s);
    }
    if (n_reads > 0) {
        Stage st("mem_chain_pack", s);
        hipLaunchKernelGGL(mem_chain_pack_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, A);
    }
    if (io.seed_cap > 0) {
        Stage st("mem_chain_tail", s);
        const long long blocks = (io.seed_cap * 5 + 255) / 256;
        if (blocks >= (1ll << 31)) { set_error("mem chain: seed_cap too large"); return GBX_ERR_UNSUPPORTED; }
        hipLaunchKernelGGL(mem_chain_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("mem chain");
    return GBX_OK;
}

}  // namespace gbx
