// mem_regs_kernels.hip — alignment regions between the seed extension and the CIGAR stage (bwa-mem's redundancy skip of
// mem_chain2aln, mem_sort_dedup_patch without the patch, mem_mark_primary_se, mem_approx_mapq_se and the region choice of
// mem_reg2sam) for gfx950 (MI355X).
//
// Semantics: include/gbx.h and DESIGN 3.12 (restated in tests/mem_regs_ref.py, which pins them).
//
// Shape: one read per wavefront, as in mem_chain_kernels.hip.  A read is serial in its seeds (a seed is tested against the
// regions made before it), in the i of the dedup walk and in the i of the primary scan; what is parallel is the list each of
// them scans (the read's regions, the walk's j, z), the chain's seeds (the overlap test, seedcov), the sorts and the mapq.  The
// control flow of a wavefront is uniform; lane 0 (or the one lane a ballot picks) stores, and a barrier (free for a one-wave
// block) orders the store before the next step's loads.
//   * All per-read state lives in slabs of the workspace indexed by the read's first seed: a read has at most as many regions
//     as seeds, so slab s0 .. s0 + seeds of every per-region array is its own, whatever the count - no capacity a read could
//     exceed, no second path.  Regions stay where they were created; the orders are index lists (ord / ordb).
//   * a scan that stops at an element takes the first such element from a ballot; what the elements before it are owed (the
//     walk's exclusions) is applied to the lanes below it only.
//   * sorts: 192-bit keys (three words, compared in order), unique, so any correct sort gives the same order - wave_sort of
//     mem_common.h: in registers with shuffles up to 64 keys, a bitonic network over the slab above that.
//   * output: the read kernel leaves per-read counts, a scan over the reads turns them into offsets (reg_off and the CIGAR
//     list's), a pack pass writes region, seed and result records at their final places: no dependence on the scheduling.
#include "mem_common.h"

namespace gbx {
namespace {

using MrKey = RegKey;
static_assert(sizeof(MrKey) == 24, "MrKey");
static_assert(sizeof(gbx_mem_reg) == 88 && sizeof(gbx_mem_regs_params) == 64 && sizeof(gbx_bsw_seed_result) == 32, "records");

struct MrArgs {
    gbx_mem_regs_params p;
    MemRegsIo io;
    long long n_reads, read_id0;
    long long *cnt;                  // [2][n_reads + 1]: regions / reported regions per read, then their exclusive scan
    gbx_mem_reg *rg;                 // [seed_cap]   slab of a read: its first seed; regions in creation order
    int *took;                       // [seed_cap]   per seed: it made a region
    int *ord, *ordb, *z, *excl;      // [seed_cap]   two index lists; the primaries; the dedup's exclusions (by creation index)
    MrKey *key;                      // [2 seed_cap] slab at twice the first seed: the sort pads to a power of two
};

struct MrSpan { long long c0, c1, s0, room, n_seeds; bool ok; };
__device__ inline bool mr_upstream_ok(const MrArgs &A) { return *A.io.n_chains <= A.io.chain_cap && *A.io.n_seeds <= A.io.seed_cap; }
__device__ inline MrSpan mr_span(const MrArgs &A, long long r)
{
    MrSpan s;
    s.ok = mr_upstream_ok(A);
    const long long n_chains = clampll(*A.io.n_chains, 0, A.io.chain_cap);
    s.n_seeds = clampll(*A.io.n_seeds, 0, A.io.seed_cap);
    s.c0 = clampll(A.io.chain_off[r], 0, n_chains);
    s.c1 = clampll(A.io.chain_off[r + 1], s.c0, n_chains);
    s.s0 = s.c1 > s.c0 ? clampll(A.io.chains[s.c0].seed_off, 0, s.n_seeds) : 0;
    s.room = s.n_seeds - s.s0;                      // the slab's length: what the read's chains can hold when they lie in order
    return s;
}

// the seed [sq, sq + sl) x [sr, sr + sl) lies inside the region and around its diagonal, ahead or behind (mem_chain2aln)
__device__ inline bool mr_around(const gbx_mem_reg &P, int sq, long long sr, int sl, int lq, const gbx_mem_regs_params &p)
{
    if (sr < P.rb || sr + sl > P.re || sq < P.qb || sq + sl > P.qe) return false;
    if ((double)(sl - P.seedlen0) > .1 * (double)lq) return false;
    long long qd = sq - P.qb, rd = sr - P.rb;
    long long wg = max_gap(qd < rd ? qd : rd, p);
    wg = wg < P.w ? wg : P.w;
    if (qd - rd < wg && rd - qd < wg) return true;
    qd = P.qe - (sq + sl); rd = P.re - (sr + sl);
    wg = max_gap(qd < rd ? qd : rd, p);
    wg = wg < P.w ? wg : P.w;
    return qd - rd < wg && rd - qd < wg;
}

// ---- the regions of one read, in their output order; leaves the read's counts and its state in the slabs
__global__ void __launch_bounds__(64) mem_regs_read_kernel(MrArgs A)
{
    const long long r = blockIdx.x;
    const int lane = threadIdx.x;
    const gbx_mem_regs_params p = A.p;
    const MrSpan S = mr_span(A, r);
    if (!S.ok || S.c1 == S.c0) {
        if (lane == 0) { A.cnt[r] = 0; A.cnt[A.n_reads + 1 + r] = 0; }
        return;
    }
    gbx_mem_reg *const rg = A.rg + S.s0;
    int *const ord = A.ord + S.s0, *const ordb = A.ordb + S.s0, *const z = A.z + S.s0, *const excl = A.excl + S.s0;
    MrKey *const key = A.key + 2 * S.s0;
    const MrKey pad = {{~0ull, ~0ull, ~0ull}};

    // ---- 1: the choice of seeds, serial in the seeds of every chain
    int nav = 0;
    for (long long c = S.c0; c < S.c1; ++c) {
        const gbx_mem_chain ch = A.io.chains[c];
        const long long so = clampll(ch.seed_off, 0, S.n_seeds);
        const int ns = (int)clampll(ch.n_seeds, 0, S.n_seeds - so);
        const gbx_bsw_seed *const seeds = A.io.seeds + so;
        const gbx_bsw_seed_result *const res = A.io.res + so;
        int *const took = A.took + so;
        if (ns > S.room) continue;                                               // (chains out of order: no room in the slab's keys)
        int m = 0;
        for (int b0 = 0; b0 < ns; b0 += 64) {
            const int k = b0 + lane;
            const bool present = k < ns && res[k].qb >= 0;
            if (k < ns) {
                took[k] = 0;
                MrKey v = pad;
                if (present) { v.w[0] = (unsigned)seeds[k].len ^ 0x80000000u; v.w[1] = 0; v.w[2] = (unsigned)k; }
                key[k] = v;
            }
            m += __builtin_popcountll(__ballot(present));
        }
        __syncthreads();
        wave_sort(key, ns, lane);
        for (int t = m - 1; t >= 0; --t) {                                       // by (len, index) from the largest down
            const int k = (int)(unsigned)key[t].w[2];
            const gbx_bsw_seed s = seeds[k];
            const gbx_bsw_seed_result e = res[k];
            const long long sr = s.roff + s.rbeg;
            bool stopped = false;
            for (int jb = 0; jb < nav; jb += 64) {
                const int j = jb + lane;
                const bool stop = j < nav && mr_around(rg[j], s.qbeg, sr, s.len, s.lq, p);
                if (__ballot(stop)) { stopped = true; break; }
            }
            bool take = !stopped;
            if (stopped)                                                          // a taken seed of the chain that overlaps it off its diagonal
                for (int b0 = 0; b0 < ns; b0 += 64) {
                    const int i = b0 + lane;
                    bool ok = false;
                    if (i < ns && took[i]) {
                        const gbx_bsw_seed u = seeds[i];
                        if (!((double)u.len < (double)s.len * .95)) {
                            const int q4 = s.len >> 2;
                            ok = (s.qbeg <= u.qbeg && s.qbeg + s.len - u.qbeg >= q4 && u.qbeg - s.qbeg != u.rbeg - s.rbeg) ||
                                 (u.qbeg <= s.qbeg && u.qbeg + u.len - s.qbeg >= q4 && s.qbeg - u.qbeg != s.rbeg - u.rbeg);
                        }
                    }
                    if (__ballot(ok)) { take = true; break; }
                }
            if (take && nav < S.room) {
                gbx_mem_reg R;
                R.rb = s.roff + e.rb; R.re = s.roff + e.re; R.seed = so + k;
                R.qb = e.qb; R.qe = e.qe; R.read = (int32_t)r; R.rid = ch.contig;
                R.score = e.score; R.truesc = e.truesc; R.sub = 0; R.sub_n = 0; R.w = e.w; R.seedcov = 0; R.seedlen0 = s.len;
                R.secondary = -1; R.mapq = 0; R.flag = 0; R.sel = -1; R.csub = 0;
                int cov = 0;
                for (int b0 = 0; b0 < ns; b0 += 64) {
                    const int i = b0 + lane;
                    if (i < ns && res[i].qb >= 0) {
                        const gbx_bsw_seed u = seeds[i];
                        const long long ur = u.roff + u.rbeg;
                        if (u.qbeg >= R.qb && u.qbeg + u.len <= R.qe && ur >= R.rb && ur + u.len <= R.re) cov += u.len;
                    }
                }
                for (int d = 32; d > 0; d >>= 1) cov += __shfl_xor(cov, d);
                R.seedcov = cov;
                if (lane == 0) { rg[nav] = R; took[k] = 1; }
                ++nav;
            }
            __syncthreads();
        }
    }

    // ---- 2: mem_sort_dedup_patch without the patch; the survivors end up in ordb
    const int n = wave_reg_dedup(rg, nullptr, nav, ord, ordb, excl, key, p, lane);

    // ---- 3: mem_mark_primary_se.  ord becomes the output order; z holds places in it
    wave_reg_mark_primary(rg, ordb, n, ord, z, key, A.read_id0 + r, p, lane);

    // ---- 4, 5: mapq, the reported regions and their places in the read's part of the CIGAR list
    const int l_rep = A.io.l_rep[r];
    const int n_rep = wave_reg_report(rg, ord, n, [&](const gbx_mem_reg &R) { return reg_frac_rep(R, l_rep, A.io.seeds[R.seed].lq); }, p, lane);
    if (lane == 0) { A.cnt[r] = n; A.cnt[A.n_reads + 1 + r] = n_rep; }
}

// ---- the records at their final places: lanes over the read's regions in output order
__global__ void __launch_bounds__(64) mem_regs_pack_kernel(MrArgs A)
{
    const long long r = blockIdx.x;
    const int lane = threadIdx.x;
    const MrSpan S = mr_span(A, r);
    const long long base = A.cnt[r], sbase = A.cnt[A.n_reads + 1 + r];
    const long long n = A.cnt[r + 1] - base;
    if (!S.ok || n <= 0 || n > S.room) return;
    const gbx_mem_reg *const rg = A.rg + S.s0;
    const int *const ord = A.ord + S.s0;
    for (long long i = lane; i < n; i += 64) {
        gbx_mem_reg R = rg[ord[i]];
        const bool rep = R.sel >= 0;
        const long long gs = sbase + R.sel;
        if (rep) R.sel = (int32_t)gs;
        const long long g = base + i;
        if (g < A.io.reg_cap) A.io.regs[g] = R;
        if (rep && gs < A.io.sel_cap) {
            const gbx_bsw_seed s = A.io.seeds[R.seed];
            A.io.sel_seeds[gs] = s;
            A.io.sel_res[gs] = reg_result(R, s);
        }
    }
}

struct MrLayout { size_t o_cnt, o_bsum, o_rg, o_took, o_ord, o_ordb, o_z, o_excl, o_key, total; int blocks; };
MrLayout mr_layout(int64_t n_reads, int64_t seed_cap)
{
    MrLayout L;
    const size_t nr = (size_t)n_reads, np = (size_t)seed_cap;
    L.blocks = mem_scan_blocks(n_reads);
    L.o_cnt = 0;
    L.o_bsum = L.o_cnt + align256(2 * (nr + 1) * 8);
    L.o_rg = L.o_bsum + align256(2 * (size_t)L.blocks * 8);
    L.o_took = L.o_rg + align256(np * sizeof(gbx_mem_reg));
    L.o_ord = L.o_took + align256(np * 4);
    L.o_ordb = L.o_ord + align256(np * 4);
    L.o_z = L.o_ordb + align256(np * 4);
    L.o_excl = L.o_z + align256(np * 4);
    L.o_key = L.o_excl + align256(np * 4);
    L.total = L.o_key + align256(2 * np * sizeof(MrKey));
    return L;
}

}  // namespace

size_t mem_regs_workspace_bytes(int64_t n_reads, int64_t seed_cap)
{
    return mr_layout(n_reads < 0 ? 0 : n_reads, seed_cap < 0 ? 0 : seed_cap).total;
}

int mem_regs_launch(const gbx_mem_regs_params *p, int64_t n_reads, int64_t read_id0, const MemRegsIo &io, void *d_work, size_t work_bytes,
                    hipStream_t s)
{
    if (n_reads >= (1ll << 31) - 1) { set_error("mem regs: more than 2^31 - 2 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    if (io.seed_cap >= (1ll << 31) || io.sel_cap >= (1ll << 31) * 256) { set_error("mem regs: seed_cap or sel_cap too large"); return GBX_ERR_UNSUPPORTED; }
    const MrLayout L = mr_layout(n_reads, io.seed_cap);
    if (work_bytes < L.total) { set_error("mem regs: workspace too small"); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    MrArgs A;
    A.p = *p; A.io = io; A.n_reads = n_reads; A.read_id0 = read_id0;
    A.cnt = (long long *)(wb + L.o_cnt); A.rg = (gbx_mem_reg *)(wb + L.o_rg);
    A.took = (int *)(wb + L.o_took); A.ord = (int *)(wb + L.o_ord); A.ordb = (int *)(wb + L.o_ordb); A.z = (int *)(wb + L.o_z);
    A.excl = (int *)(wb + L.o_excl); A.key = (MrKey *)(wb + L.o_key);
    if (n_reads > 0) {
        Stage st("mem_regs_read", s);
        hipLaunchKernelGGL(mem_regs_read_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, A);
    }
    {
        Stage st("mem_regs_scan", s);
        // the totals are -1 when the chaining overflowed: the condition of mr_upstream_ok
        mem_scan_launch({A.cnt, n_reads, 2, (long long *)(wb + L.o_bsum), L.blocks, {io.n_regs, io.n_sel}, io.reg_off,
                         {{io.n_chains, INT64_MIN, io.chain_cap}, {io.n_seeds, INT64_MIN, io.seed_cap}}}, s);
    }
    if (n_reads > 0) {
        Stage st("mem_regs_pack", s);
        hipLaunchKernelGGL(mem_regs_pack_kernel, dim3((unsigned)n_reads), dim3(64), 0, s, A);
    }
    if (io.sel_cap > 0) {
        Stage st("mem_regs_tail", s);
        mem_sel_tail_launch(io.sel_seeds, io.sel_res, io.sel_cap, io.n_sel, s);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("mem regs");
    return GBX_OK;
}

}  // namespace gbx
