// mem_scan.hip — the exclusive scan that turns per-unit counts into offsets (the bwa-mem stages, the index builder, mm seeding
// and mm alignment, and the radix sort of dev_sort.hip) and the tail fill of a CIGAR list (regs, pair).  mm_map_kernels.hip keeps a
// one-launch scan for its map and PAF stages, where three launches measured slower.  The pieces of the scan are in dev_prims.h.
#include "dev_prims.h"

namespace gbx {
namespace {

// ---- exclusive scan of the counts (n + 1 entries per quantity; blockIdx.y: the quantity)
__global__ void __launch_bounds__(MEM_SCAN) mem_scan_kernel(MemScanJob J)
{
    __shared__ long long sh[MEM_SCAN / 64];
    long long *const cnt = J.cnt + (long long)blockIdx.y * (J.n + 1);
    const long long i = (long long)blockIdx.x * MEM_SCAN + threadIdx.x;
    const long long c = i < J.n ? cnt[i] : 0;
    long long total;
    const long long before = block_scan_excl(c, sh, &total);
    if (i <= J.n) cnt[i] = before;
    if (threadIdx.x == MEM_SCAN - 1) J.bsum[(long long)blockIdx.y * J.blocks + blockIdx.x] = total;
}

// one block per quantity: exclusive scan of the block sums, the total (-1: the stage before it overflowed) to its place
__global__ void __launch_bounds__(1024) mem_scan_top_kernel(MemScanJob J)
{
    const long long carry = scan_block_sums(J.bsum + (long long)blockIdx.x * J.blocks, J.blocks);
    int64_t *const total = blockIdx.x == 0 ? J.total[0] : J.total[1];
    if (threadIdx.x != 0 || !total) return;
    bool ok = true;
    for (int g = 0; g < 2; ++g)
        if (J.guard[g].n) { const int64_t n = *J.guard[g].n; ok = ok && n >= J.guard[g].lo && n <= J.guard[g].hi; }
    *total = ok ? carry : -1;
}

__global__ void __launch_bounds__(MEM_SCAN) mem_scan_offset_kernel(MemScanJob J)
{
    long long *const cnt = J.cnt + (long long)blockIdx.y * (J.n + 1);
    const long long i = (long long)blockIdx.x * MEM_SCAN + threadIdx.x;
    if (i > J.n) return;
    const long long v = cnt[i] + J.bsum[(long long)blockIdx.y * J.blocks + blockIdx.x];
    cnt[i] = v;
    if (blockIdx.y == 0 && J.off0) J.off0[i] = v;
}

__global__ void __launch_bounds__(256) sel_tail_kernel(gbx_bsw_seed *seeds, gbx_bsw_seed_result *res, long long cap, const int64_t *n_sel)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = *n_sel;
    if (t >= cap || t < (n < 0 ? 0 : n)) return;
    long long *const s = (long long *)(seeds + t), *const e = (long long *)(res + t);
    for (int k = 0; k < 5; ++k) s[k] = 0;
    for (int k = 0; k < 4; ++k) e[k] = -1;
}

}  // namespace

void mem_scan_launch(const MemScanJob &J, hipStream_t s)
{
    hipLaunchKernelGGL(mem_scan_kernel, dim3(J.blocks, J.nq), dim3(MEM_SCAN), 0, s, J);
    hipLaunchKernelGGL(mem_scan_top_kernel, dim3(J.nq), dim3(1024), 0, s, J);
    hipLaunchKernelGGL(mem_scan_offset_kernel, dim3(J.blocks, J.nq), dim3(MEM_SCAN), 0, s, J);
}

void mem_sel_tail_launch(gbx_bsw_seed *seeds, gbx_bsw_seed_result *res, int64_t cap, const int64_t *n, hipStream_t s)
{
    hipLaunchKernelGGL(sel_tail_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, seeds, res, (long long)cap, n);
}

}  // namespace gbx
