// dev_sort.hip — the one LSD radix sort of the device pipelines (radix_sort: gbx_internal.h).  The FM-index builder
// (mem_index_kernels.hip) sorts (key, position) pairs of a count the host knows; the minimap2 seeding stage (mm_kernels.hip) sorts
// 128-bit items of a count that lives on the device, under a grid that covers the capacity.  A pass is three plain launches:
// per-block digit histograms, the shared exclusive scan (mem_scan_launch) and a stable scatter (ranks inside a wavefront from
// ballots over the digit's bits, across the waves of a block from LDS counters).  No block waits for another inside a kernel.
#include "dev_prims.h"

namespace gbx {
namespace {

constexpr int SORT_WAVES = SORT_THREADS / 64;
using u32 = uint32_t;
using u64 = uint64_t;

__device__ inline long long sort_count(const SortCount &c) { return c.dev ? clip_count(c.dev, c.n) : c.n; }

// hist[d * blocks + b]: elements of block b with digit d.  word: the array that holds the digit.  A block past the count still
// writes its (zero) column
__global__ void __launch_bounds__(SORT_THREADS) sort_hist_kernel(const u64 *word, SortCount count, int shift, u32 mask, long long *hist, long long blocks)
{
    __shared__ u32 h[256];
    const long long m = sort_count(count);
    mask &= 255u;                                                            // a digit indexes 256 counters, whatever the caller passed
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * SORT_TILE;
    if (base < m) {
#pragma unroll 4
        for (int r = 0; r < SORT_ITEMS; ++r) {
            const long long i = base + (long long)r * SORT_THREADS + threadIdx.x;
            if (i < m) atomicAdd(&h[(u32)(word[i] >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    hist[(long long)threadIdx.x * blocks + blockIdx.x] = h[threadIdx.x];
}

// hist has become its exclusive scan: where block b's elements of digit d start.  A wave takes SORT_ITEMS * 64 consecutive
// elements, 64 a trip, so the order inside a block is wave, trip, lane.
template <class V>
__global__ void __launch_bounds__(SORT_THREADS) sort_scatter_kernel(const u64 *a, const V *b, SortCount count, SortPass pass, const long long *hist,
                                                                   long long blocks, u64 *a_out, V *b_out)
{
    __shared__ long long wcount[SORT_WAVES][256];
    const long long m = sort_count(count);
    if ((long long)blockIdx.x * SORT_TILE >= m) return;                      // (the whole block leaves)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 below = (1ull << lane) - 1;
    const bool in_b = sizeof(V) == 8 && pass.word;                           // (u32 payloads carry no digits)
    const u32 mask = pass.mask & 255u;                                       // a digit indexes 256 counters, whatever the caller passed
    for (int w = 0; w < SORT_WAVES; ++w) wcount[w][threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * SORT_TILE + (long long)wv * SORT_ITEMS * 64;
    u64 ka[SORT_ITEMS];
    V kb[SORT_ITEMS];
    u32 at[SORT_ITEMS];
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long long i = base + r * 64 + lane;
        const bool act = i < m;
        ka[r] = act ? a[i] : 0;
        kb[r] = act ? b[i] : 0;
        const u32 d = (u32)((in_b ? (u64)kb[r] : ka[r]) >> pass.shift) & mask;
        u64 same = __ballot(act);
#pragma unroll
        for (int bit_no = 0; bit_no < 8; ++bit_no) {
            const bool bit = (d >> bit_no) & 1u;
            const u64 bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const u32 before = (u32)wcount[wv][d];                               // every lane of a digit reads before its first lane adds
        at[r] = before + (u32)__builtin_popcountll(same & below);
        __builtin_amdgcn_wave_barrier();
        if (act && (same & below) == 0) wcount[wv][d] = before + (u32)__builtin_popcountll(same);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        long long o = hist[(long long)threadIdx.x * blocks + blockIdx.x];
        for (int w = 0; w < SORT_WAVES; ++w) { const long long c = wcount[w][threadIdx.x]; wcount[w][threadIdx.x] = o; o += c; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long long i = base + r * 64 + lane;
        if (i < m) {
            const long long dst = wcount[wv][(u32)((in_b ? (u64)kb[r] : ka[r]) >> pass.shift) & mask] + at[r];
            a_out[dst] = ka[r];
            b_out[dst] = kb[r];
        }
    }
}

}  // namespace

template <class V>
int radix_sort(const SortBufs<V> &B, const SortCount &count, const SortPass *pass, int n_pass, hipStream_t s)
{
    const long long blocks = sort_blocks(count.n);
    int cur = 0;
    for (int p = 0; p < n_pass; ++p) {
        const u64 *const word = sizeof(V) == 8 && pass[p].word ? (const u64 *)B.b[cur] : B.a[cur];
        hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)blocks), dim3(SORT_THREADS), 0, s, word, count, pass[p].shift, pass[p].mask, B.hist, blocks);
        scan_launch1(B.hist, 256 * blocks, B.hsum, nullptr, MemScanGuard{}, s);
        hipLaunchKernelGGL(sort_scatter_kernel<V>, dim3((unsigned)blocks), dim3(SORT_THREADS), 0, s, (const u64 *)B.a[cur], (const V *)B.b[cur], count,
                           pass[p], (const long long *)B.hist, blocks, B.a[cur ^ 1], B.b[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
}
template int radix_sort<u32>(const SortBufs<u32> &, const SortCount &, const SortPass *, int, hipStream_t);
template int radix_sort<u64>(const SortBufs<u64> &, const SortCount &, const SortPass *, int, hipStream_t);

SortLayout sort_layout(int64_t cap, Carver &carve)
{
    SortLayout L;
    const size_t c = (size_t)(cap > 0 ? cap : 1);
    for (int i = 0; i < 2; ++i) { L.o_a[i] = carve(c * 8); L.o_b[i] = carve(c * 8); }
    const long long he = 256 * sort_blocks(cap);
    L.o_hist = carve((size_t)(he + 1) * 8);
    L.o_hsum = carve((size_t)mem_scan_blocks(he) * 8);
    return L;
}

SortBufs<u64> sort_bufs(char *wb, const SortLayout &L)
{
    SortBufs<u64> B;
    for (int i = 0; i < 2; ++i) { B.a[i] = (u64 *)(wb + L.o_a[i]); B.b[i] = (u64 *)(wb + L.o_b[i]); }
    B.hist = (long long *)(wb + L.o_hist); B.hsum = (long long *)(wb + L.o_hsum);
    return B;
}

}  // namespace gbx
