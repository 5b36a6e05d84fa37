// dev_prims.h — the device helpers that belong to no one pipeline: workspace carving, a device count clipped to its capacity
// and the pieces of the exclusive scan over per-unit counts.  The scan's own kernels are in mem_scan.hip (mem_scan_launch:
// gbx_internal.h); fmi_kernels.hip and fmi_sal_kernels.hip use the pieces inside their fused kernels.  The radix sort built on
// them is dev_sort.hip.  What only the bwa-mem stages share is in mem_common.h.
#pragma once
#include "gbx_internal.h"
#include "carver.h"           // align256, Carver

namespace gbx {

constexpr int MEM_SCAN = 1024;                      // entries a block of the scan takes
inline int mem_scan_blocks(int64_t n) { return (int)((n + 1 + MEM_SCAN - 1) / MEM_SCAN); }     // n counts make n + 1 offsets

// the block of the mm stages' element-wise kernels (mm_kernels.hip, mm_map_kernels.hip, mm_align_kernels.hip) and the grid over n
constexpr int MM_EL = 256;
inline unsigned mm_el_blocks(long long n) { const long long b = (n + MM_EL - 1) / MM_EL; return (unsigned)(b > 0 ? b : 1); }

// a count that lives on the device, as far as its capacity holds it
__device__ inline long long clip_count(const int64_t *n, long long cap)
{
    const long long v = *n;
    return v < 0 ? 0 : v > cap ? cap : v;
}

// mem_scan_launch over one quantity: cnt[0 .. n) becomes its offsets, cnt[n] and *total (nullptr: nowhere) the total
inline void scan_launch1(long long *cnt, long long n, long long *bsum, int64_t *total, const MemScanGuard &guard, hipStream_t s)
{
    MemScanJob J{};
    J.cnt = cnt; J.n = n; J.nq = 1; J.bsum = bsum; J.blocks = mem_scan_blocks(n);
    J.total[0] = total; J.guard[0] = guard;
    mem_scan_launch(J, s);
}

// ---- exclusive scan, the pieces.  A block scans its entries (block_scan_excl) and leaves its sum; one block scans the sums
// (scan_block_sums); an offset pass adds a block's scanned sum to its entries.
template <class T>
__device__ inline T wave_scan_incl(T v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) { const T u = __shfl_up(v, d); if (lane >= d) v += u; }
    return v;
}

// every thread of the block calls it with its count c; -> the sum of the counts of the threads before it.  sh: a long long per
// wavefront of the block.  *block_total: the sum up to and including this thread - in the block's last thread, the block's sum.
__device__ inline long long block_scan_excl(long long c, long long *sh, long long *block_total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long v = wave_scan_incl(c, lane);
    if (lane == 63) sh[wv] = v;
    __syncthreads();
    long long before = 0;
    for (int w = 0; w < wv; ++w) before += sh[w];
    *block_total = before + v;
    return before + v - c;
}

// one block of 1024 threads: bsum[0 .. blocks) becomes its exclusive scan; -> the total (in every thread)
__device__ inline long long scan_block_sums(long long *bsum, int blocks)
{
    __shared__ long long sh[1024];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < blocks; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const long long v = i < blocks ? bsum[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const long long u = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += u;
            __syncthreads();
        }
        if (i < blocks) bsum[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    return carry;
}

}  // namespace gbx
