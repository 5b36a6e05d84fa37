// atomic_peak — what the MI355X sustains for kmer_count_kernel's access pattern: no-return 32-bit integer atomic adds of 1
// (global_atomic_add_u32) to random words of a large table, every lane of a wavefront on a different line.  The ceiling
// the count pass's adds per second are read against.
//
//   hipcc -O2 --offload-arch=gfx950 scripts/atomic_peak.hip -o scripts/atomic_peak && ./scripts/atomic_peak > profiles/atomic_peak.json
//
// Forms: "random" = every lane adds to a hashed word of a table of `table_mib` (64 MiB .. 4 GiB); "hot" = the same over only
// 4096 words (contention, as a homopolymer or repeat gives); "coalesced" = each wavefront adds to 64 consecutive words
// (256 contiguous bytes, the float-atomic form MI355X_MICROARCH measures at full rate).  Reported: G adds/s over wall time
// of the kernel (HIP events), best of five launches after a warm-up.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

__device__ inline unsigned mix(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// MODE 0 random, 1 coalesced; words_mask + 1 = table words (a power of two)
template <int MODE>
__global__ void __launch_bounds__(256) adds(unsigned *table, unsigned words_mask, int per_lane)
{
    const unsigned gid = blockIdx.x * 256 + threadIdx.x;
    unsigned state = mix(gid * 2654435761u + 977u);
    for (int i = 0; i < per_lane; ++i) {
        unsigned w;
        if (MODE == 0) { state = mix(state + i); w = state & words_mask; }
        else w = ((mix((gid >> 6) * 131u + i) << 6) + (gid & 63)) & words_mask;
        atomicAdd(&table[w], 1u);
    }
}

template <int MODE>
double run(unsigned *t, size_t words, int blocks, int per_lane)
{
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    hipLaunchKernelGGL(adds<MODE>, dim3(blocks), dim3(256), 0, 0, t, (unsigned)(words - 1), per_lane);
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int r = 0; r < 5; ++r) {
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL(adds<MODE>, dim3(blocks), dim3(256), 0, 0, t, (unsigned)(words - 1), per_lane);
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        best = ms < best ? ms : best;
    }
    CHECK(hipGetLastError());
    CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
    return (double)blocks * 256 * per_lane / (best * 1e-3) / 1e9;
}

int main()
{
    const size_t max_words = (size_t)1 << 30;                  // 4 GiB of counters
    unsigned *t = nullptr;
    CHECK(hipMalloc(&t, max_words * 4));
    CHECK(hipMemset(t, 0, max_words * 4));
    const int blocks = 256 * 8, per_lane = 256;                 // the count pass's grid; 134 M adds per launch
    printf("{\n \"what\": \"no-return global_atomic_add_u32 of 1, %d workgroups x 256 lanes x %d adds (scripts/atomic_peak.hip)\",\n", blocks, per_lane);
    printf(" \"unit\": \"G adds/s\",\n \"rows\": [\n");
    const size_t mib[] = {64, 1024, 4096};
    for (int i = 0; i < 3; ++i) {
        const size_t words = mib[i] << 18;
        printf("  {\"table_mib\": %zu, \"random\": %.2f, \"coalesced\": %.2f},\n", mib[i], run<0>(t, words, blocks, per_lane),
               run<1>(t, words, blocks, per_lane));
    }
    printf("  {\"table_words\": 4096, \"hot_random\": %.2f}\n ]\n}\n", run<0>(t, 4096, blocks, per_lane));
    CHECK(hipFree(t));
    return 0;
}
