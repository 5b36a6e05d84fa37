// mm_sam_kernels.hip — SAM records, cs / MD tags and = / X operations of the aligned regions.  The rules are in
// mm_sam_rules.h, one text for these kernels and for the host build the CPU tests run; this file gives them a team (a wavefront:
// ballots, a shuffle scan) and the memory.
//
//   units     one a region and one a read: region g of read r has slot g + r, read r's own line (the SAM line of a read none of
//             whose regions prints) the slot behind its regions', so the slots are in text order
//   measure   a wavefront a unit: the line's length from the counting sink -> at[slot]; counts[2] by integer atomics
//   scan      mem_scan_launch over the slots -> where every line starts, *n_text the true need
//   write     a wavefront a unit: the same function with the storing sink, below text_cap only; line_off from the slots
// Integer VALU and vector stores only.  Every loop is counted on entry (words, columns / 64, a read's regions, digits, a binary
// search of at most 40 halvings), so the GBX_LOOP_GUARD build has nothing to add; nothing is written at or past a capacity, no
// kernel waits for another block and the entry does not synchronise with the host.
#include "dev_prims.h"
#include "mm_sam_rules.h"

namespace gbx {
namespace {

constexpr long long GRID_MOST = 1 << 20;

struct MmSamWave {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int size() const { return 64; }
    __device__ void sync() const {}
    __device__ uint64_t ballot(bool b) const { return __ballot(b); }
    __device__ int64_t scan(int64_t v, int64_t *total) const
    {
        const long long in = wave_scan_incl((long long)v, lane());
        *total = __shfl(in, 63);
        return in - v;
    }
    __device__ int64_t shfl(int64_t v, int l) const { return __shfl((long long)v, l); }
};

struct SamJob {
    MmSamView v;
    const int64_t *n_regs; int64_t reg_cap;
    uint8_t *lines; int64_t text_cap; int64_t *line_off; int64_t *counts;
    long long *at;                                  // reg_cap + n_reads + 1 slots
};

__device__ inline long long clamp_to(long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the read reg_off puts region g in, or -1
__device__ inline long long read_of(const SamJob &J, long long g)
{
    long long a = 0, b = J.v.paf.n_reads - 1;                          // the last read whose regions start at or before g
    if (b < 0) return -1;
    for (int it = 0; it < 40 && a < b; ++it) { const long long m = (a + b + 1) >> 1; if (J.v.reg_off[m] <= g) a = m; else b = m - 1; }
    return J.v.reg_off[a] <= g && g < J.v.reg_off[a + 1] ? a : -1;
}

// unit u -> its slot (or -1: it has no line) and its line through the sink W
template <bool W>
__device__ inline long long unit_line(const SamJob &J, long long u, long long n_regs, long long *slot)
{
    const MmSamWave tm;
    const long long R = J.reg_cap, n_reads = J.v.paf.n_reads;
    *slot = -1;
    if (u < R) {
        if (u >= n_regs) return 0;
        const long long r = read_of(J, u);
        if (r < 0) return 0;
        *slot = u + r;
        return mm_sam_region_line<W>(tm, J.v, n_regs, u, r, J.lines, W ? J.at[*slot] : 0, J.text_cap);
    }
    const long long r = u - R;
    if (r >= n_reads) return 0;
    *slot = clamp_to(J.v.reg_off[r + 1], n_regs) + r;
    return mm_sam_unmapped_line<W>(tm, J.v, n_regs, r, J.lines, W ? J.at[*slot] : 0, J.text_cap);
}

__global__ void __launch_bounds__(64) mm_sam_measure_kernel(SamJob J)
{
    const long long n_regs = clip_count(J.n_regs, J.reg_cap), N = J.reg_cap + J.v.paf.n_reads;
    for (long long u = blockIdx.x; u < N; u += gridDim.x) {
        long long slot;
        const long long len = unit_line<false>(J, u, n_regs, &slot);
        if (threadIdx.x == 0) {
            if (slot >= 0) J.at[slot] = len;
            if (len > 0) atomicAdd((unsigned long long *)J.counts, 1ull);
            else if (u < n_regs) atomicAdd((unsigned long long *)J.counts + 1, 1ull);
        }
    }
}

__global__ void __launch_bounds__(64) mm_sam_write_kernel(SamJob J)
{
    const long long n_regs = clip_count(J.n_regs, J.reg_cap), n_reads = J.v.paf.n_reads, N = J.reg_cap + n_reads;
    for (long long u = blockIdx.x; u <= N; u += gridDim.x) {
        long long slot;
        if (u < N) unit_line<true>(J, u, n_regs, &slot);
        if (u <= n_reads && threadIdx.x == 0) J.line_off[u] = J.at[clamp_to(J.v.reg_off[u], n_regs) + u];
    }
}

struct SamLayout { size_t o_at, o_bsum, total; long long n; };
SamLayout sam_layout(int64_t n_reads, int64_t reg_cap)
{
    SamLayout L;
    Carver take;
    L.n = (reg_cap > 0 ? reg_cap : 0) + (n_reads > 0 ? n_reads : 0);
    L.o_at = take((size_t)(L.n + 1) * 8);
    L.o_bsum = take((size_t)mem_scan_blocks(L.n) * 8);
    L.total = take.at;
    return L;
}

}  // namespace

size_t mm_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap) { return sam_layout(n_reads, reg_cap).total; }

int mm_sam_launch(const gbx_mm_sam_params *p, const MmSamIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    const MmPafIo &f = io.paf;
    const SamLayout L = sam_layout(f.n_reads, f.reg_cap);
    if (work_bytes < L.total) { set_error("mm sam: workspace too small (%zu bytes, %zu needed)", work_bytes, L.total); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    SamJob J;
    J.v = MmSamView{MmPafView{f.n_reads, f.regs, f.alns, f.cigar, f.cigar_cap, f.qnames, f.qname_off, f.seq_off, f.rep_len, f.n_targets, f.tnames, f.tname_off,
                              f.tseq_off},
                    f.reg_off, io.seq, io.qual, io.tseq, *p};
    J.n_regs = f.n_regs; J.reg_cap = f.reg_cap > 0 ? f.reg_cap : 0;
    J.lines = f.lines; J.text_cap = f.text_cap; J.line_off = f.line_off; J.counts = io.counts;
    J.at = (long long *)(wb + L.o_at);
    Stage st("mm_sam", s);
    GBX_HIP(hipMemsetAsync(J.at, 0, (size_t)(L.n + 1) * 8, s));
    GBX_HIP(hipMemsetAsync(io.counts, 0, 16, s));
    const unsigned grid = (unsigned)(L.n + 1 > GRID_MOST ? GRID_MOST : L.n + 1);
    if (L.n > 0) hipLaunchKernelGGL(mm_sam_measure_kernel, dim3(grid), dim3(64), 0, s, J);
    scan_launch1(J.at, L.n, (long long *)(wb + L.o_bsum), f.n_text, MemScanGuard{}, s);
    hipLaunchKernelGGL(mm_sam_write_kernel, dim3(grid), dim3(64), 0, s, J);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
