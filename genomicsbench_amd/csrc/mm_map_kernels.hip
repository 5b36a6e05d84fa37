// mm_map_kernels.hip — minimap2 behind the chain scores: chains, regions, parents, selection, mapq and the PAF text.
// The rules are in mm_map_rules.h, one text for these kernels and for the host build the CPU tests run; this file gives them a
// team (one wavefront a read: a block of 64, __syncthreads() as the barrier) and the memory.
//
//   chains    a wavefront per read: ends and their peaks, the keys sorted in the read's workspace, every key's walk at once
//             (atomicMin on the owner), chain order, the chained anchors -> per-read counts
//   scan      chain_off in place, the total into counts[0]
//   regions   a wavefront per read: u to its place, mm_gen_regs per lane, then lane 0 takes parents, selection and mapq into a
//             staging record per chain -> per-read counts; scan; a copy to reg_off
//   PAF       a lane per region measures its line, scan, a lane per region writes it
// Counts live on the device, nothing is written past a capacity, no kernel waits for another block and no entry synchronises
// with the host.
#include "dev_prims.h"
#include "mm_map_rules.h"

namespace gbx {
namespace {

constexpr int EL = 256, SCAN_T = 1024;
inline unsigned el_blocks(long long n) { const long long b = (n + EL - 1) / EL; return (unsigned)(b > 0 ? b : 1); }

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
__global__ void __launch_bounds__(SCAN_T) mm_map_scan_kernel(int64_t *a, const int64_t *n_dev, long long n_cap, int64_t *total, const int64_t *guard,
                                                             long long guard_cap)
{
    __shared__ long long part[SCAN_T];
    const long long n = n_dev ? clip_count(n_dev, n_cap) : n_cap;
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
        for (long long i = n; i <= n_cap; ++i) a[i] = tot;            // n_cap - n entries at most: the tail of a clipped count
        if (total) *total = guard && *guard > guard_cap ? -1 : tot;
    }
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
struct PafJob { MmPafIo io; int64_t *at; };

__device__ inline long long paf_line(const PafJob &J, long long g, uint8_t *out, long long at)
{
    const gbx_mm_reg reg = J.io.regs[g];
    const long long r = reg.read;
    if (r < 0 || r >= J.io.n_reads) return 0;
    const long long q0 = J.io.qname_off[r], q1 = J.io.qname_off[r + 1];
    const bool tok = reg.rid >= 0 && reg.rid < J.io.n_targets;
    const long long t0 = tok ? J.io.tname_off[reg.rid] : 0, t1 = tok ? J.io.tname_off[reg.rid + 1] : 0;
    const int32_t tlen = tok ? (int32_t)(J.io.tseq_off[reg.rid + 1] - J.io.tseq_off[reg.rid]) : 0;
    return mm_paf_line(out, at, J.io.text_cap, reg, J.io.qnames + q0, q1 > q0 ? q1 - q0 : 0, (int32_t)(J.io.seq_off[r + 1] - J.io.seq_off[r]),
                       tok ? J.io.tnames + t0 : nullptr, t1 > t0 ? t1 - t0 : 0, tlen, J.io.rep_len[r]);
}

__global__ void __launch_bounds__(EL) mm_paf_measure_kernel(PafJob J)
{
    const long long g = (long long)blockIdx.x * EL + threadIdx.x;
    if (g >= J.io.reg_cap) return;
    J.at[g] = g < clip_count(J.io.n_regs, J.io.reg_cap) ? paf_line(J, g, nullptr, 0) : 0;
}

__global__ void __launch_bounds__(EL) mm_paf_write_kernel(PafJob J)
{
    const long long g = (long long)blockIdx.x * EL + threadIdx.x;
    if (g < clip_count(J.io.n_regs, J.io.reg_cap)) paf_line(J, g, J.io.lines, J.at[g]);
    if (g <= J.io.n_reads) {
        const long long ro = J.io.reg_off[g];
        J.io.line_off[g] = J.at[ro < 0 ? 0 : ro > J.io.reg_cap ? J.io.reg_cap : ro];
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
        hipLaunchKernelGGL(mm_map_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, io.chain_off, (const int64_t *)nullptr, (long long)io.n_reads, io.counts,
                           (const int64_t *)nullptr, 0ll);
    }
    {
        Stage st("mm_map_regs", s);
        hipLaunchKernelGGL(mm_map_reg_kernel, grid, dim3(64), 0, s, J);
        hipLaunchKernelGGL(mm_map_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, io.reg_off, (const int64_t *)nullptr, (long long)io.n_reads, io.counts + 1,
                           (const int64_t *)io.counts, (long long)io.chain_cap);
        hipLaunchKernelGGL(mm_map_place_kernel, grid, dim3(64), 0, s, J);
    }
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

size_t mm_paf_workspace_bytes(int64_t n_reads, int64_t reg_cap) { (void)n_reads; return align256((size_t)((reg_cap > 0 ? reg_cap : 0) + 1) * 8); }

int mm_paf_launch(const MmPafIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    const size_t need = mm_paf_workspace_bytes(io.n_reads, io.reg_cap);
    if (work_bytes < need) { set_error("mm paf: workspace too small (%zu bytes, %zu needed)", work_bytes, need); return GBX_ERR_ARG; }
    PafJob J{io, (int64_t *)d_work};
    Stage st("mm_paf", s);
    if (io.reg_cap > 0) hipLaunchKernelGGL(mm_paf_measure_kernel, dim3(el_blocks(io.reg_cap)), dim3(EL), 0, s, J);
    hipLaunchKernelGGL(mm_map_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, J.at, (const int64_t *)nullptr, (long long)io.reg_cap, io.n_text,
                       (const int64_t *)nullptr, 0ll);
    const long long span = io.reg_cap > io.n_reads + 1 ? io.reg_cap : io.n_reads + 1;
    hipLaunchKernelGGL(mm_paf_write_kernel, dim3(el_blocks(span)), dim3(EL), 0, s, J);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
