// mm_align_kernels.hip — base-level alignment of minimap2's regions.  The rules are in mm_align_rules.h, one text for
// these kernels and for the host build the CPU tests run; this file gives them a team (a wavefront: a block of 64, __syncthreads()
// as the barrier, a butterfly of shuffles as the reduction) and the memory.
//
//   plan      a lane per region: valid or not, its jobs (left extension, fills, right extension) and the bytes of z they take
//   scans     job offsets and z offsets in region order (mem_scan_launch) -> counts[0], counts[2]
//   jobs      a lane per region writes its job records; a region whose jobs end past z_bytes is marked (flag 32)
//   DP        a wavefront per job, whichever region it belongs to: lanes across the antidiagonal, the rows of three diagonals in
//             LDS when the band's ring is at most 512 wide (22 KiB a wavefront: the default band of 500), else in the job's room
//             (L2-resident), a direction byte a cell in the order the diagonals make them; lane 0 walks back once for the job's
//             run count and consumed spans
//   place     a lane per region: where each job's words go within the region, neighbours merged -> words per region; scan
//   pack      a wavefront per region: a lane per job walks again and writes its words at their final places, lane 0 adds the
//             merged boundary runs, walks the statistics and writes the record
// Integer VALU only.  Counts live on the device, every loop is counted (diagonals, a walk of at most tl + ql steps), nothing is
// written at or past a capacity, no kernel waits for another block and the entry does not synchronise with the host.
#include <cstdlib>
#include "dev_prims.h"
#include "mm_align_rules.h"

namespace gbx {
namespace {

constexpr int LDS_M = 512;
constexpr long long GRID_MOST = 1 << 20;
inline unsigned wave_blocks(long long n) { return (unsigned)(n < 1 ? 1 : n > GRID_MOST ? GRID_MOST : n); }

struct MmAlnWave {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int size() const { return (int)blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ int64_t max_key(int64_t k) const
    {
        for (int d = 32; d > 0; d >>= 1) { const long long o = __shfl_xor((long long)k, d); if (o > k) k = o; }
        return k;
    }
};

struct AlnLayout { size_t o_njobs, o_zneed, o_words, o_bsum, o_jobs, total; int64_t job_cap; };
AlnLayout aln_layout(int64_t reg_cap, int64_t anchor_cap)
{
    const int64_t R = reg_cap > 0 ? reg_cap : 0, A = anchor_cap > 0 ? anchor_cap : 0;
    AlnLayout L;
    Carver take;
    L.job_cap = A + 2 * R;                                             // a region of cnt anchors has cnt + 1 jobs
    L.o_njobs = take((size_t)(R + 1) * 8); L.o_zneed = take((size_t)(R + 1) * 8); L.o_words = take((size_t)(R + 1) * 8);
    L.o_bsum = take((size_t)mem_scan_blocks(R) * 8);
    L.o_jobs = take((size_t)(L.job_cap > 0 ? L.job_cap : 1) * sizeof(MmAlnJob));
    L.total = take.at;
    return L;
}

struct AlnArgs {
    MmAlignIo io;
    gbx_mm_align_params P;
    long long *njobs, *zneed, *words;
    MmAlnJob *jobs;
    long long job_cap;
    int32_t lds_m;                                  // the widest row LDS takes (0: every job's rows in its room)
};

__device__ inline bool region_view(const AlnArgs &A, const gbx_mm_reg &g, MmAlnSeq *S, const uint64_t **x, const uint64_t **y, int32_t *n_chained)
{
    const MmAlignIo &io = A.io;
    const MmAlnIn in{io.n_reads, io.off, io.cax, io.cay, io.n_chained, io.anchor_cap, io.seq, io.seq_off, io.n_targets, io.tseq, io.tseq_off};
    return mm_aln_region_view(in, g, S, x, y, n_chained);
}

__device__ inline bool region_valid(const AlnArgs &A, const gbx_mm_reg &g, MmAlnSeq *S, const uint64_t **x, const uint64_t **y)
{
    int32_t nc;
    return region_view(A, g, S, x, y, &nc) && mm_aln_valid(g, A.io.n_targets, nc, *x, *y, S->tlen, S->qlen);
}

__global__ void __launch_bounds__(MM_EL) mm_align_plan_kernel(AlnArgs A)
{
    const long long g = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (g > A.io.reg_cap) return;
    long long nj = 0, zb = 0;
    if (g < clip_count(A.io.n_regs, A.io.reg_cap)) {
        const gbx_mm_reg reg = A.io.regs[g];
        MmAlnSeq S;
        const uint64_t *x, *y;
        if (region_valid(A, reg, &S, &x, &y)) {
            MmAlnPlanCount c;
            mm_aln_plan(A.P, reg.cnt, x, y, S.tlen, S.qlen, c);
            nj = c.n; zb = c.bytes;
        } else mm_aln_copy(reg, GBX_MM_ALN_INVALID, &A.io.alns[g]);
    }
    A.njobs[g] = nj; A.zneed[g] = zb; A.words[g] = 0;
}

__global__ void __launch_bounds__(MM_EL) mm_align_jobs_kernel(AlnArgs A)
{
    const long long g = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (g >= clip_count(A.io.n_regs, A.io.reg_cap)) return;
    const long long j0 = A.njobs[g], j1 = A.njobs[g + 1];
    if (j1 <= j0) return;
    const gbx_mm_reg reg = A.io.regs[g];
    MmAlnSeq S;
    const uint64_t *x, *y;
    if (!region_valid(A, reg, &S, &x, &y)) return;
    const int32_t skip = A.zneed[g + 1] > A.io.z_bytes || j1 > A.job_cap;
    MmAlnPlanWrite wr{A.jobs, j0, A.job_cap, A.zneed[g], (int32_t)g, skip};
    mm_aln_plan(A.P, reg.cnt, x, y, S.tlen, S.qlen, wr);
    if (skip) mm_aln_copy(reg, GBX_MM_ALN_NO_ROOM, &A.io.alns[g]);
}

__global__ void __launch_bounds__(64) mm_align_dp_kernel(AlnArgs A)
{
    __shared__ int32_t rows[MMA_ROWS * LDS_M];
    const long long n = clip_count(A.io.counts, A.job_cap);
    for (long long k = blockIdx.x; k < n; k += gridDim.x) {
        MmAlnJob *J = A.jobs + k;
        const int32_t g = J->reg;
        if (J->skip || g < 0 || g >= A.io.reg_cap) continue;
        const gbx_mm_reg reg = A.io.regs[g];
        MmAlnSeq S;
        const uint64_t *x, *y;
        int32_t nc;
        if (!region_view(A, reg, &S, &x, &y, &nc)) continue;
        mm_aln_job_run(MmAlnWave(), A.P, S, A.io.z + J->z_at, A.lds_m ? rows : nullptr, A.lds_m, J);
    }
}

__global__ void __launch_bounds__(MM_EL) mm_align_place_kernel(AlnArgs A)
{
    const long long g = (long long)blockIdx.x * MM_EL + threadIdx.x;
    if (g >= clip_count(A.io.n_regs, A.io.reg_cap)) return;
    const long long j0 = A.njobs[g], j1 = A.njobs[g + 1];
    if (j1 <= j0 || j1 > A.job_cap || A.jobs[j0].skip) return;
    A.words[g] = mm_aln_place(A.jobs + j0, (int32_t)(j1 - j0));
}

__global__ void __launch_bounds__(64) mm_align_pack_kernel(AlnArgs A)
{
    const long long n = clip_count(A.io.n_regs, A.io.reg_cap);
    for (long long g = blockIdx.x; g < n; g += gridDim.x) {
        const long long j0 = A.njobs[g], j1 = A.njobs[g + 1];
        if (j1 <= j0 || j1 > A.job_cap || A.jobs[j0].skip) continue;
        const gbx_mm_reg reg = A.io.regs[g];
        MmAlnSeq S;
        const uint64_t *x, *y;
        int32_t nc;
        if (!region_view(A, reg, &S, &x, &y, &nc)) continue;
        mm_aln_pack(MmAlnWave(), A.P, reg, S, A.jobs + j0, (int32_t)(j1 - j0), (int32_t)(A.words[g + 1] - A.words[g]), A.io.z, A.io.cigar, A.words[g],
                    A.io.cigar_cap, &A.io.alns[g]);
    }
}

}  // namespace

size_t mm_align_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t anchor_cap) { (void)n_reads; return aln_layout(reg_cap, anchor_cap).total; }

int mm_align_launch(const gbx_mm_align_params *p, const MmAlignIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    const AlnLayout L = aln_layout(io.reg_cap, io.anchor_cap);
    if (work_bytes < L.total) { set_error("mm align: workspace too small (%zu bytes, %zu needed)", work_bytes, L.total); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    AlnArgs A;
    A.io = io; A.P = *p;
    A.njobs = (long long *)(wb + L.o_njobs); A.zneed = (long long *)(wb + L.o_zneed); A.words = (long long *)(wb + L.o_words);
    A.jobs = (MmAlnJob *)(wb + L.o_jobs); A.job_cap = L.job_cap;
    const char *e = getenv("GBX_MM_ALIGN_LDS");                        /* measuring aid, read per call: 0 keeps every job's rows in its room */
    A.lds_m = e && atoi(e) == 0 ? 0 : LDS_M;
    long long *bsum = (long long *)(wb + L.o_bsum);
    const long long R = io.reg_cap;
    {
        Stage st("mm_align_plan", s);
        hipLaunchKernelGGL(mm_align_plan_kernel, dim3(mm_el_blocks(R + 1)), dim3(MM_EL), 0, s, A);
        scan_launch1(A.njobs, R, bsum, io.counts, MemScanGuard{}, s);
        scan_launch1(A.zneed, R, bsum, io.counts + 2, MemScanGuard{}, s);
        hipLaunchKernelGGL(mm_align_jobs_kernel, dim3(mm_el_blocks(R)), dim3(MM_EL), 0, s, A);
    }
    {
        Stage st("mm_align_dp", s);
        hipLaunchKernelGGL(mm_align_dp_kernel, dim3(wave_blocks(L.job_cap)), dim3(64), 0, s, A);
    }
    {
        Stage st("mm_align_pack", s);
        hipLaunchKernelGGL(mm_align_place_kernel, dim3(mm_el_blocks(R)), dim3(MM_EL), 0, s, A);
        scan_launch1(A.words, R, bsum, io.counts + 1, MemScanGuard{}, s);
        hipLaunchKernelGGL(mm_align_pack_kernel, dim3(wave_blocks(R)), dim3(64), 0, s, A);
    }
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
