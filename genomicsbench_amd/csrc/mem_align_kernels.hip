// mem_align_kernels.hip — the one kernel of the aligner (capi_mem_align.hip) that is not a stage's: behind the chain it gathers
// every stage's count and overflow word into a gbx_mem_align_counts record, so that the host reads the state of the whole chain
// with one copy and one synchronisation.  The words are read where the stages leave them; the two counts over the CIGAR stage's
// records (rid == -2: no room for the direction bytes; rid >= 0: aligned) are summed per block and added with vector atomics.
#include <hip/hip_runtime.h>
#include "gbx_internal.h"

namespace gbx {
namespace {

static_assert(sizeof(gbx_mem_align_counts) == 144 && sizeof(gbx_mem_aln) == 48, "records");

__device__ inline long long ga_word(const int64_t *p) { return p ? (long long)*p : 0ll; }

// out was zeroed on the stream before the launch
__global__ void __launch_bounds__(256) mem_align_gather_kernel(MemAlignGather G)
{
    __shared__ unsigned long long part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long miss = 0, ok = 0;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < G.n_alns; k += (long long)gridDim.x * 256) {
        const int rid = G.alns[k].rid;
        miss += rid == -2;
        ok += rid >= 0;
    }
    for (int s = 32; s > 0; s >>= 1) { miss += __shfl_xor(miss, s); ok += __shfl_xor(ok, s); }
    if (lane == 0) { part[0][wave] = miss; part[1][wave] = ok; }
    __syncthreads();
    if (threadIdx.x == 0) {
        miss = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        ok = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (miss) atomicAdd((unsigned long long *)&G.out->n_z_miss, miss);
        if (ok) atomicAdd((unsigned long long *)&G.out->n_alns, ok);
    }
    if (blockIdx.x != 0 || threadIdx.x >= 14) return;
    long long v = 0;
    int64_t *dst = nullptr;
    switch (threadIdx.x) {
    case 0: v = G.fmi_counters ? (long long)G.fmi_counters[2] : 0; dst = &G.out->slot_worst; break;
    case 1: v = ga_word(G.n_smem); dst = &G.out->n_smem; break;
    case 2: v = ga_word(G.n_pos); dst = &G.out->n_pos; break;
    case 3: v = ga_word(G.n_chains); dst = &G.out->n_chains; break;
    case 4: v = ga_word(G.n_seeds); dst = &G.out->n_seeds; break;
    case 5: v = ga_word(G.n_regs); dst = &G.out->n_regs; break;
    case 6: v = ga_word(G.n_sel); dst = &G.out->n_sel; break;
    case 7: v = ga_word(G.n_xregs); dst = &G.out->n_xregs; break;
    case 8: v = ga_word(G.n_xseeds); dst = &G.out->n_xseeds; break;
    case 9: v = ga_word(G.n_xsel); dst = &G.out->n_xsel; break;
    case 10: v = ga_word(G.n_psel); dst = &G.out->n_psel; break;
    case 11: v = ga_word(G.n_cigar); dst = &G.out->n_cigar; break;
    case 12: v = ga_word(G.n_recs); dst = &G.out->n_recs; break;
    default: v = ga_word(G.n_md); dst = &G.out->n_md; break;
    }
    *dst = v;
    if (threadIdx.x == 0) G.out->n_text = ga_word(G.n_text);
}

}  // namespace

int mem_align_gather_launch(const MemAlignGather &g, hipStream_t s)
{
    if (!g.out || g.n_alns < 0 || (g.n_alns > 0 && !g.alns)) { set_error("mem align gather: bad argument"); return GBX_ERR_ARG; }
    Stage st("mem_align_gather", s);
    GBX_HIP(hipMemsetAsync(g.out, 0, sizeof(gbx_mem_align_counts), s));
    const long long want = (g.n_alns + 255) / 256;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : want > 1024 ? 1024 : want);
    hipLaunchKernelGGL(mem_align_gather_kernel, dim3(blocks), dim3(256), 0, s, g);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
