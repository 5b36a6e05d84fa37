// mm_map_kernels.hip — minimap2 behind the chain scores: chains, regions, parents, selection, mapq, and the PAF text
// with or without the alignments of DESIGN 3.20.  The rules are in mm_map_rules.h and mm_paf_rules.h, one text for these kernels
// and for the host build the CPU tests run; this file gives them a team (one wavefront a read: a block of 64, __syncthreads()
// as the barrier) and the memory.
//
//   chains    a wavefront per read: ends and their peaks, the keys sorted in the read's workspace, every key's walk at once
//             (atomicMin on the owner), chain order, the chained anchors -> per-read counts
//   scan      chain_off in place, the total into counts[0]
//   regions   a wavefront per read: u to its place, mm_gen_regs per lane, then lane 0 takes parents, selection and mapq into a
//             staging record per chain -> per-read counts; scan; a copy to reg_off
//   PAF       a lane per region measures its line (plain, or with cg:Z: where alignments are given and the region has one), scan,
//             a lane per region writes it
// The scans are one launch of one block (mm_map_scan_kernel), not the three launches of the shared scan (mem_scan_launch): with
// the shared scan 400 reads took 1.035 against 1.017 ms to map and 0.055 against 0.051 ms to print (profiles/mm_refactor_ab.json).
// Counts live on the device, nothing is written past a capacity, no kernel waits for another block and no entry synchronises
// with the host.
#include "dev_prims.h"
#include "mm_paf_rules.h"

namespace gbx {
namespace {

constexpr int SCAN_T = 1024;

struct MmWave {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int size() const { return (int)blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ int atomic_min(int32_t *p, int32_t v) const { return atomicMin(p, v); }
    __device__ int atomic_add(int32_t *p, int32_t v) const { return atomicAdd(p, v); }
};

struct MapLayout { size_t o_own, o_top, o_perm, o_key, o_urank, o_uws, o_nkeys, o_nch, o_nreg, o_z, o_w, o_stage, total; };
MapLayout map_layout(int64_t n_reads, int64_t anchor_cap, int64_t chain_cap)
{
    const size_t A = (size_t)(anchor_cap > 0 ? anchor_cap : 1), R = (size_t)(n_reads > 0 ? n_reads : 1), Cc = (size_t)(chain_cap > 0 ? chain_cap : 1);
    MapLayout L;
    Carver take;
    L.o_own = take(A * 4); L.o_top = take(A * 4); L.o_perm = take(A * 4);
    L.o_key = take(A * 8); L.o_urank = take(A * 8); L.o_uws = take(A * 8);
    L.o_nkeys = take(R * 4); L.o_nch = take(R * 4); L.o_nreg = take(R * 4);
    L.o_z = take(Cc * sizeof(MmZ)); L.o_w = take(Cc * 4); L.o_stage = take(Cc * sizeof(gbx_mm_reg));
    L.total = take.at;
    return L;
}

struct MapJob {
    MmMapIo io;
    gbx_mm_map_params P;
    int32_t *own, *top, *perm, *nkeys, *nch, *nreg, *w;
    uint64_t *key, *urank, *uws;
    MmZ *z;
    gbx_mm_reg *stage;
};

// the read's anchors [o, o + n), or none where off is not what it must be
__device__ inline void read_span(const MapJob &J, long long r, long long *o, int32_t *n)
{
    const long long lo = J.io.off[r], hi = J.io.off[r + 1];
    const bool ok = lo >= 0 && hi >= lo && hi <= J.io.anchor_cap && hi - lo < 0x7fffffffll;
    *o = ok ? lo : 0;
    *n = ok ? (int32_t)(hi - lo) : 0;
}

__device__ inline MmMapRead read_of(const MapJob &J, long long r, long long o, int32_t n)
{
    const long long ql = J.io.seq_off[r + 1] - J.io.seq_off[r];
    return MmMapRead{n, J.io.ax + o, J.io.ay + o, J.io.f + o, J.io.p + o, J.io.v + o, (int32_t)ql, J.io.rep_len[r], J.io.hash[r]};
}

__global__ void __launch_bounds__(64) mm_map_chain_kernel(MapJob J)
{
    const long long r = blockIdx.x;
    long long o;
    int32_t n;
    read_span(J, r, &o, &n);
    // Parents and owners stay in the workspace: staging them in LDS (32 KiB a wavefront, 4 096 anchors) left five wavefronts a CU
    // where sixteen stood and measured slower on the large preset (backtrack 1.50 -> 2.18 ms, profiles/mm_map_lds_ab.json).
    const MmChainWork w{J.own + o, J.top + o, J.perm + o, J.key + o, J.urank + o, J.nkeys + r};
    const MmMapRead rd = read_of(J, r, o, n);
    mm_map_chains(MmWave(), rd, J.P, w, J.uws + o, J.io.cax + o, J.io.cay + o, J.nch + r, J.io.n_chained + r);
    if (threadIdx.x == 0) J.io.chain_off[r] = J.nch[r];
}

// exclusive scan of a[0 .. n) in place, a[n] = the total, also to *total (-1 where *guard > guard_cap); one block
__global__ void __launch_bounds__(SCAN_T) mm_map_scan_kernel(int64_t *a, long long n, int64_t *total, const int64_t *guard, long long guard_cap)
{
    __shared__ long long part[SCAN_T];
    const long long chunk = (n + SCAN_T - 1) / SCAN_T, lo = (long long)threadIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    long long sum = 0;
    for (long long i = lo; i < hi; ++i) sum += a[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_T; d <<= 1) {
        const long long add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    long long run = part[threadIdx.x] - sum;
    for (long long i = lo; i < hi; ++i) { const long long c = a[i]; a[i] = run; run += c; }
    if (threadIdx.x == 0) {
        const long long tot = part[SCAN_T - 1];
        a[n] = tot;
        if (total) *total = guard && *guard > guard_cap ? -1 : tot;
    }
}

inline void map_scan(int64_t *a, long long n, int64_t *total, const int64_t *guard, long long guard_cap, hipStream_t s)
{
    hipLaunchKernelGGL(mm_map_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, a, n, total, guard, guard_cap);
}

__global__ void __launch_bounds__(64) mm_map_reg_kernel(MapJob J)
{
    const long long r = blockIdx.x;
    long long o;
    int32_t n;
    read_span(J, r, &o, &n);
    const long long co = J.io.chain_off[r];
    const int32_t nch = J.nch[r];
    for (int32_t i = threadIdx.x; i < nch; i += 64)
        if (co + i < J.io.chain_cap) J.io.u[co + i] = J.uws[o + i];
    if (J.io.counts[0] > J.io.chain_cap) {                            // not all chains have a place: no regions
        if (threadIdx.x == 0) J.io.reg_off[r] = 0;
        return;
    }
    mm_map_regs(MmWave(), read_of(J, r, o, n), (int32_t)r, J.P, nch, J.uws + o, J.io.cax + o, J.io.cay + o, J.z + co, J.w + co, J.stage + co, J.nreg + r);
    if (threadIdx.x == 0) J.io.reg_off[r] = J.nreg[r];
}

__global__ void __launch_bounds__(64) mm_map_place_kernel(MapJob J)
{
    const long long r = blockIdx.x;
    if (J.io.counts[0] > J.io.chain_cap) return;
    const long long ro = J.io.reg_off[r], co = J.io.chain_off[r];
    const int32_t n = J.nreg[r];
    for (int32_t i = threadIdx.x; i < n; i += 64)
        if (ro + i < J.io.reg_cap) J.io.regs[ro + i] = J.stage[co + i];
}

// ------------------------------------------------------------------------------------------------ PAF
struct PafJob {
    MmPafView v;
    const int64_t *reg_off, *n_regs; int64_t reg_cap;
    uint8_t *lines; int64_t text_cap; int64_t *line_off;
    int64_t *at;                                    // [reg_cap + 1]: the lines' lengths, then their offsets
};

__global__ void __launch_bounds__(MM_EL) mm_paf_measure_kernel(PafJob J)
{
    const long long g = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (g >= J.reg_cap) return;                                       // at[reg_cap] is the scan's to write
    J.at[g] = g < clip_count(J.n_regs, J.reg_cap) ? mm_paf_region_line(J.v, g, nullptr, 0, 0) : 0;
}

__global__ void __launch_bounds__(MM_EL) mm_paf_write_kernel(PafJob J)
{
    const long long g = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (g < clip_count(J.n_regs, J.reg_cap)) mm_paf_region_line(J.v, g, J.lines, J.at[g], J.text_cap);
    if (g <= J.v.n_reads) {
        const long long ro = J.reg_off[g];
        J.line_off[g] = J.at[ro < 0 ? 0 : ro > J.reg_cap ? J.reg_cap : ro];
    }
}

}  // namespace

size_t mm_map_workspace_bytes(int64_t n_reads, int64_t anchor_cap, int64_t chain_cap) { return map_layout(n_reads, anchor_cap, chain_cap).total; }

int mm_map_launch(const gbx_mm_map_params *p, const MmMapIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    const MapLayout L = map_layout(io.n_reads, io.anchor_cap, io.chain_cap);
    if (work_bytes < L.total) { set_error("mm map: workspace too small (%zu bytes, %zu needed)", work_bytes, L.total); return GBX_ERR_ARG; }
    if (io.n_reads == 0) {
        GBX_HIP(hipMemsetAsync(io.chain_off, 0, 8, s));
        GBX_HIP(hipMemsetAsync(io.reg_off, 0, 8, s));
        GBX_HIP(hipMemsetAsync(io.counts, 0, 16, s));
        return GBX_OK;
    }
    char *wb = (char *)d_work;
    MapJob J;
    J.io = io; J.P = *p;
    J.own = (int32_t *)(wb + L.o_own); J.top = (int32_t *)(wb + L.o_top); J.perm = (int32_t *)(wb + L.o_perm);
    J.key = (uint64_t *)(wb + L.o_key); J.urank = (uint64_t *)(wb + L.o_urank); J.uws = (uint64_t *)(wb + L.o_uws);
    J.nkeys = (int32_t *)(wb + L.o_nkeys); J.nch = (int32_t *)(wb + L.o_nch); J.nreg = (int32_t *)(wb + L.o_nreg);
    J.z = (MmZ *)(wb + L.o_z); J.w = (int32_t *)(wb + L.o_w); J.stage = (gbx_mm_reg *)(wb + L.o_stage);
    const dim3 grid((unsigned)io.n_reads);
    {
        Stage st("mm_map_chains", s);
        hipLaunchKernelGGL(mm_map_chain_kernel, grid, dim3(64), 0, s, J);
        map_scan(io.chain_off, io.n_reads, io.counts, nullptr, 0, s);
    }
    {
        Stage st("mm_map_regs", s);
        hipLaunchKernelGGL(mm_map_reg_kernel, grid, dim3(64), 0, s, J);
        map_scan(io.reg_off, io.n_reads, io.counts + 1, io.counts, io.chain_cap, s);      // -1: the chains did not fit
        hipLaunchKernelGGL(mm_map_place_kernel, grid, dim3(64), 0, s, J);
    }
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

size_t mm_paf_workspace_bytes(int64_t reg_cap) { return align256((size_t)((reg_cap > 0 ? reg_cap : 0) + 1) * 8); }

// measure, scan, write; with io.alns the aligned regions print their cg:Z: lines
int mm_paf_launch(const MmPafIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    const char *who = io.alns ? "mm paf cigar" : "mm paf";
    const size_t need = mm_paf_workspace_bytes(io.reg_cap);
    if (work_bytes < need) { set_error("%s: workspace too small (%zu bytes, %zu needed)", who, work_bytes, need); return GBX_ERR_ARG; }
    const long long R = io.reg_cap > 0 ? io.reg_cap : 0;
    const PafJob J{MmPafView{io.n_reads, io.regs, io.alns, io.cigar, io.cigar_cap, io.qnames, io.qname_off, io.seq_off, io.rep_len, io.n_targets, io.tnames,
                             io.tname_off, io.tseq_off}, io.reg_off, io.n_regs, io.reg_cap, io.lines, io.text_cap, io.line_off, (int64_t *)d_work};
    Stage st(io.alns ? "mm_paf_cigar" : "mm_paf", s);
    if (R > 0) hipLaunchKernelGGL(mm_paf_measure_kernel, dim3(mm_el_blocks(R)), dim3(MM_EL), 0, s, J);
    map_scan(J.at, R, io.n_text, nullptr, 0, s);
    const long long span = R > io.n_reads + 1 ? R : io.n_reads + 1;
    hipLaunchKernelGGL(mm_paf_write_kernel, dim3(mm_el_blocks(span)), dim3(MM_EL), 0, s, J);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
