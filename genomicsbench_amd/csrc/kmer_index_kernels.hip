// kmer_index_kernels.hip — Flye's minimizer index of long reads (VertexIndex::buildIndexMinimizers) for gfx950 (MI355X).
//
// Semantics: include/gbx.h, kmer index section; the rules (hash, roll, next(F), the reset test, global positions, the fp32
// filter, the tiling constants) are in kmer_index_rules.h, which the plain host compiler takes as well.  DESIGN 3.7.1.
//
// Selection.  A read's len - k positions are cut into tiles of KI_TILE; a workgroup takes a tile, a wavefront KI_WAVE
// consecutive positions of it, a lane KI_LANE.
//   tile   each lane rolls the codes of KI_LANE consecutive positions (k - 1 bases of lead-in) and leaves their hashes in LDS:
//          the tile's and a halo of w - 1 positions before and w behind it.  From them every position p gets one byte
//          step[p] = next(p) - p (0: the chain ends) and the bit "p is a reset point", both functions of the hashes alone;
//          in this second phase a lane takes every KI_THREADS-th position, so a wavefront reads consecutive LDS words.
//   walk   the minimizers are the positions reachable from 0 over step[].  A reset point is on that chain whatever came before
//          it, so every reset point walks the chain from itself up to the next reset point and marks what it passes.  Each
//          stretch between two reset points is walked once, by one lane: a run that has no reset point (a homopolymer, a short
//          tandem repeat: equal hashes never reset) costs one lane a load per minimizer of the run, linear in its length, and
//          no warm-up length is assumed anywhere.
//   count  chosen positions per tile; their exclusive scan (mem_scan_launch) gives every tile's first output slot and, at a
//          read's first tile, mini_off
//   emit   block scan inside the tile; a chosen position rolls its k bases again and writes (position, strand) or, for the
//          index, (canonical code, global position) into the sort's buffers
// Index.  One radix_sort<uint64_t> of the pairs over the bits in use (the bits of 2 * total_len, then 2k key bits); run heads
// and their scan give the k-mers' capacities and the distinct count; one thread computes the filter scalar; a scan over the
// runs of (kept, kept capacity) places the k-mers and their positions in the CSR.
//
// Loops: the tile loops are counted by the tile total, the roll by KI_LANE + k - 1 bases, the rules' loops by w; the walk is
// the data-dependent one and carries a GBX_GUARD of the position total.  Nothing synchronises with the host.
// Bounds: the units kernel checks the reads' length sum against the total_len the workspace was sized with; with another sum
// the tile and position totals are 0 and nothing below runs past a buffer.
#include <algorithm>
#include "dev_prims.h"
#include "kmer_index_rules.h"

namespace gbx {
namespace {

constexpr int KI_GRID = 256 * 8;                   // the tile kernels' grid: eight workgroups per CU, tiles in a grid-stride loop
constexpr int KI_SLOTS = KI_TILE + 2 * KI_HALO;    // hashes in LDS: LDS slot i holds position p0 - KI_HALO + i
enum { CTL_NPOS = 0, CTL_OK = 1, CTL_NTILES = 2, CTL_NCHOSEN = 3, CTL_N = 4 };
constexpr uint8_t F_RESET = 1, F_CHOSEN = 2;

struct KiLayout {
    long long cap, nt;
    size_t o_tile, o_pos, o_len, o_ctl, o_tread, o_step, o_flag, o_tcnt, o_tsum, o_cnt2, o_bsum2, total;
    SortLayout S;
};

KiLayout ki_layout(long long n_reads, long long total_len, bool index)
{
    KiLayout L;
    Carver carve;
    L.cap = total_len;                                               // positions, chosen positions and pairs: at most a base each
    L.nt = total_len / KI_TILE + n_reads;                            // tiles: at most len / KI_TILE + 1 a read
    L.o_tile = carve((size_t)(n_reads + 1) * 8);                     // prefix sums over the reads: tiles,
    L.o_pos = carve((size_t)(n_reads + 1) * 8);                      // positions
    L.o_len = carve((size_t)(n_reads + 1) * 8);                      // and lengths
    L.o_ctl = carve(CTL_N * 8);
    L.o_tread = carve((size_t)(L.nt + 1) * 8);                       // a tile's read
    L.o_step = carve((size_t)L.cap + 1);
    L.o_flag = carve((size_t)L.cap + 1);
    L.o_tcnt = carve((size_t)(L.nt + 1) * 8);
    L.o_tsum = carve((size_t)mem_scan_blocks(L.nt) * 8);
    L.o_cnt2 = L.o_bsum2 = 0;
    if (index) {
        L.S = sort_layout(L.cap + 1, carve);                          // + 1: the spare pair of buffers holds n + 1 offsets later
        L.o_cnt2 = carve((size_t)(L.cap + 1) * 2 * 8);
        L.o_bsum2 = carve((size_t)mem_scan_blocks(L.cap) * 2 * 8);
    }
    L.total = carve.at + 64;
    return L;
}

struct KiArgs {
    const uint8_t *enc;
    const int64_t *read_off;
    const int32_t *read_len;
    long long n_reads, total_len;
    long long *tile_off, *pos_off, *len_off, *ctl, *tile_read, *tile_cnt;
    uint8_t *step, *flag;
    int k, w;
};

// One workgroup: the three prefix sums over the reads, and whether the lengths sum to the total the buffers were sized with.
__global__ void __launch_bounds__(1024) ki_units_kernel(KiArgs A)
{
    __shared__ long long sh[3][1024];
    const int t = threadIdx.x;
    const long long per = (A.n_reads + 1023) / 1024, r0 = std::min(A.n_reads, t * per), r1 = std::min(A.n_reads, r0 + per);
    long long v[3] = {0, 0, 0};
    for (long long r = r0; r < r1; ++r) {
        const long long len = std::max(0, A.read_len[r]);
        v[0] += ki_read_tiles(len, A.k);
        v[1] += std::max(0ll, len - A.k);
        v[2] += len;
    }
    for (int q = 0; q < 3; ++q) sh[q][t] = v[q];
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        long long u[3];
        for (int q = 0; q < 3; ++q) u[q] = t >= d ? sh[q][t - d] : 0;
        __syncthreads();
        for (int q = 0; q < 3; ++q) sh[q][t] += u[q];
        __syncthreads();
    }
    long long run[3];
    for (int q = 0; q < 3; ++q) run[q] = sh[q][t] - v[q];
    for (long long r = r0; r < r1; ++r) {
        const long long len = std::max(0, A.read_len[r]);
        A.tile_off[r] = run[0]; A.pos_off[r] = run[1]; A.len_off[r] = run[2];
        run[0] += ki_read_tiles(len, A.k); run[1] += std::max(0ll, len - A.k); run[2] += len;
    }
    if (t == 1023) {
        const bool ok = sh[2][1023] == A.total_len;
        A.tile_off[A.n_reads] = sh[0][1023]; A.pos_off[A.n_reads] = sh[1][1023]; A.len_off[A.n_reads] = sh[2][1023];
        A.ctl[CTL_OK] = ok;
        A.ctl[CTL_NTILES] = ok ? sh[0][1023] : 0;
        A.ctl[CTL_NPOS] = ok ? sh[1][1023] : 0;
    }
}

// the canonical code of the k-mer at s[0 .. k) and its strand
__device__ inline uint64_t ki_code_at(const uint8_t *s, int k, bool *reversed)
{
    uint64_t fwd = 0, rev = 0;
    for (int b = 0; b < k; ++b) ki_roll(&fwd, &rev, s[b], k);
    return ki_canonical(fwd, rev, reversed);
}

__global__ void __launch_bounds__(KI_THREADS) ki_tile_kernel(KiArgs A)
{
    __shared__ uint64_t sh_h[KI_SLOTS];
    __shared__ long long sh_read;
    const int t = threadIdx.x, k = A.k, w = A.w;
    const long long n_tiles = A.ctl[CTL_NTILES];
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (t == 0) {
            // the read of the tile: the largest r with tile_off[r] <= tile (reads without tiles share their offset with the next)
            long long a = 0, b = A.n_reads;
            while (b - a > 1) {
                const long long m = (a + b) >> 1;
                if (A.tile_off[m] <= tile) a = m; else b = m;
            }
            sh_read = a;
            A.tile_read[tile] = a;
        }
        __syncthreads();
        const long long a = sh_read;
        const long long n = (long long)A.read_len[a] - k;                  // the read's positions; > p0, or the tile would not exist
        const long long p0 = (tile - A.tile_off[a]) * KI_TILE;
        const long long lo = std::max(0ll, p0 - (w - 1)), hi = std::min(n, p0 + KI_TILE + w);      // the hashes the tile needs
        const uint8_t *seq = A.enc + A.read_off[a];
        for (int c = t; c < KI_SLOTS / KI_LANE; c += KI_THREADS) {
            const long long q0 = p0 - KI_HALO + (long long)c * KI_LANE;
            const long long a0 = std::max(q0, lo), a1 = std::min(q0 + KI_LANE, hi);
            if (a0 >= a1) continue;
            uint64_t fwd = 0, rev = 0;
            for (long long b = a0; b < a1 + k - 1; ++b) {                  // bases a0 .. a1 + k - 2 <= len - 2
                ki_roll(&fwd, &rev, seq[b], k);
                const long long p = b - (k - 1);
                if (p >= a0) {
                    bool reversed;
                    sh_h[p - p0 + KI_HALO] = ki_hash(ki_canonical(fwd, rev, &reversed));
                }
            }
        }
        __syncthreads();
        // the step and the reset bit: here neighbouring lanes take neighbouring positions (i = j * KI_THREADS + t), so that a
        // wavefront's LDS reads fall on consecutive 8-byte words and its byte stores are coalesced
        const long long gp0 = A.pos_off[a] + p0;
#pragma unroll
        for (int j = 0; j < KI_LANE; ++j) {
            const long long i = (long long)j * KI_THREADS + t, p = p0 + i;
            if (p >= n) break;
            const uint64_t *h = sh_h + KI_HALO + i;
            A.step[gp0 + i] = (uint8_t)ki_next_step(h, n - p, w);
            A.flag[gp0 + i] = ki_is_reset(h, p, w) ? F_RESET : 0;
        }
        __syncthreads();
    }
}

// A lane per position; the reset points walk.  step[] never leaves a read, so the walk never leaves the positions.
// The one location two lanes touch without an order between them is a reset point's flag byte: its own walker stores
// F_RESET | F_CHOSEN there while the walker that arrives from the left loads it to test F_RESET.  The tile kernel set that bit
// in an earlier launch and the store keeps it, so the load sees it set whichever value it meets; byte stores are whole.
__global__ void __launch_bounds__(256) ki_walk_kernel(KiArgs A)
{
    const long long n_pos = A.ctl[CTL_NPOS];
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_pos; g += stride) {
        if (!(A.flag[g] & F_RESET)) continue;
        long long q = g;
        uint8_t f = F_RESET | F_CHOSEN;
        GBX_GUARD(guard, n_pos);
        while (true) {
            A.flag[q] = f;                                   // nobody else writes q: the stretches between reset points are disjoint
            const int d = A.step[q];
            if (d == 0) break;
            q += d;
            if (A.flag[q] & F_RESET) break;                  // the next reset point marks itself and goes on
            f = F_CHOSEN;
            if (GBX_GUARD_TRIP(guard, GBX_GK_KMER_INDEX, 1, g)) break;
        }
    }
}

__device__ inline int ki_lane_count(const KiArgs &A, long long gp0, long long left, unsigned *bits)
{
    // the chosen ones among the lane's KI_LANE positions gp0 + t * KI_LANE ..; left: the tile's positions
    const long long i0 = (long long)threadIdx.x * KI_LANE;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < KI_LANE; ++j)
        if (i0 + j < left && (A.flag[gp0 + i0 + j] & F_CHOSEN)) m |= 1u << j;
    *bits = m;
    return __builtin_popcount(m);
}

__global__ void __launch_bounds__(KI_THREADS) ki_count_kernel(KiArgs A)
{
    __shared__ long long sh[KI_THREADS / 64];
    const long long n_tiles = A.ctl[CTL_NTILES];
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long a = A.tile_read[tile];
        const long long p0 = (tile - A.tile_off[a]) * KI_TILE, n = (long long)A.read_len[a] - A.k;
        unsigned bits;
        const long long c = ki_lane_count(A, A.pos_off[a] + p0, std::min<long long>(KI_TILE, n - p0), &bits);
        long long total;
        block_scan_excl(c, sh, &total);
        if (threadIdx.x == KI_THREADS - 1) A.tile_cnt[tile] = total;
        __syncthreads();
    }
}

struct EmitArgs {
    int32_t *mini_pos; uint8_t *mini_rev; long long mini_cap;      // the selection's output, or
    uint64_t *key, *gpos;                                          // the index's pairs (cap of them: never short)
};

__global__ void __launch_bounds__(KI_THREADS) ki_emit_kernel(KiArgs A, EmitArgs E)
{
    __shared__ long long sh[KI_THREADS / 64];
    const long long n_tiles = A.ctl[CTL_NTILES];
    const int k = A.k;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long a = A.tile_read[tile];
        const long long len = A.read_len[a];
        const long long p0 = (tile - A.tile_off[a]) * KI_TILE, n = len - k;
        unsigned bits;
        const long long c = ki_lane_count(A, A.pos_off[a] + p0, std::min<long long>(KI_TILE, n - p0), &bits);
        long long total;
        long long o = A.tile_cnt[tile] + block_scan_excl(c, sh, &total);
        const uint8_t *seq = A.enc + A.read_off[a];
#pragma unroll
        for (int j = 0; j < KI_LANE; ++j) {
            if (!(bits >> j & 1u)) continue;
            const long long p = p0 + (long long)threadIdx.x * KI_LANE + j;
            bool reversed;
            const uint64_t code = ki_code_at(seq + p, k, &reversed);
            if (E.key) {
                E.key[o] = code;
                E.gpos[o] = ki_global_pos(2ull * (uint64_t)A.len_off[a], len, p, k, reversed);
            } else if (o < E.mini_cap) {
                E.mini_pos[o] = (int32_t)p;
                E.mini_rev[o] = reversed;
            }
            ++o;
        }
        __syncthreads();
    }
}

// mini_off[r] = the first slot of read r's first tile (a read without tiles shares it with the next); *n_mini the total
__global__ void __launch_bounds__(256) ki_mini_off_kernel(KiArgs A, int64_t *mini_off, int64_t *n_mini)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > A.n_reads) return;
    const bool ok = A.ctl[CTL_OK] == 1;
    mini_off[r] = ok ? A.tile_cnt[A.tile_off[r]] : 0;
    if (r == A.n_reads) *n_mini = ok ? A.ctl[CTL_NCHOSEN] : -1;
}

// ---- the index behind the sort.  key[0 .. m) ascending, equal keys by ascending position; m = the chosen count.
struct BuildArgs {
    const uint64_t *key, *gpos;
    long long *head, *run_start, *cnt2;
    long long cap;
    const long long *ctl;
    gbx_kmer_index_stats *st;
    float rate;
    uint64_t *kmer; int64_t *off; long long kmer_cap; uint64_t *pos; long long pos_cap;
};

__device__ inline bool ki_is_head(const BuildArgs &B, long long i) { return i == 0 || B.key[i] != B.key[i - 1]; }

__global__ void __launch_bounds__(256) ki_head_kernel(BuildArgs B)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.cap) return;
    B.head[i] = i < B.ctl[CTL_NCHOSEN] && ki_is_head(B, i);
}

// head[] has become its exclusive scan (the run of a head), st->n_distinct the runs
__global__ void __launch_bounds__(256) ki_runs_kernel(BuildArgs B)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long m = B.ctl[CTL_NCHOSEN];
    if (i == 0) {
        const long long u = B.st->n_distinct;
        B.run_start[u] = m;
        const float mean = ki_mean_frequency((uint64_t)m, (uint64_t)u);
        B.st->n_chosen = m;
        B.st->mean_frequency = mean;
        B.st->repetitive_frequency = (int64_t)ki_repetitive_frequency(mean, B.rate);
        B.st->reserved_ = 0;
    }
    if (i < m && ki_is_head(B, i)) B.run_start[B.head[i]] = i;
}

// per run: kept or not, and the kept capacity
__global__ void __launch_bounds__(256) ki_keep_kernel(BuildArgs B)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B.cap) return;
    long long keep = 0, c = 0;
    if (j < B.st->n_distinct) {
        c = B.run_start[j + 1] - B.run_start[j];
        keep = !ki_is_repetitive((uint64_t)c, (uint64_t)B.st->repetitive_frequency);
    }
    B.cnt2[j] = keep;
    B.cnt2[B.cap + 1 + j] = keep ? c : 0;
}

// cnt2 has become its two exclusive scans, st->n_selected and st->n_entries the totals
__global__ void __launch_bounds__(256) ki_compact_kernel(BuildArgs B)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long m = B.ctl[CTL_NCHOSEN];
    if (i == 0) {
        gbx_kmer_index_stats *st = B.st;
        if (B.ctl[CTL_OK] == 1) {
            st->n_repetitive_kmers = st->n_distinct - st->n_selected;
            st->n_repetitive_entries = m - st->n_entries;
            st->total_len = B.cap;
            if (st->n_selected <= B.kmer_cap) B.off[st->n_selected] = st->n_entries;
        } else {
            st->n_chosen = st->n_distinct = st->repetitive_frequency = st->n_repetitive_kmers = st->n_repetitive_entries = -1;
            st->n_selected = st->n_entries = st->total_len = -1;
            st->mean_frequency = 0.f;
            if (B.kmer_cap >= 0) B.off[0] = 0;
        }
    }
    if (i >= m) return;
    const bool head = ki_is_head(B, i);
    const long long j = B.head[i] - (head ? 0 : 1), first = B.run_start[j];
    if (ki_is_repetitive((uint64_t)(B.run_start[j + 1] - first), (uint64_t)B.st->repetitive_frequency)) return;
    const long long o = B.cnt2[j], e0 = B.cnt2[B.cap + 1 + j], e = e0 + (i - first);
    if (head) {
        if (o < B.kmer_cap) B.kmer[o] = B.key[i];
        if (o <= B.kmer_cap) B.off[o] = e0;
    }
    if (e < B.pos_cap) B.pos[e] = B.gpos[i];
}

int bit_length(unsigned long long v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

KiArgs ki_args(const gbx_kmer_index_params *p, const KmerIndexReads &rd, char *wb, const KiLayout &L)
{
    KiArgs A{};
    A.enc = rd.enc; A.read_off = rd.read_off; A.read_len = rd.read_len;
    A.n_reads = rd.n_reads; A.total_len = rd.total_len;
    A.tile_off = (long long *)(wb + L.o_tile); A.pos_off = (long long *)(wb + L.o_pos); A.len_off = (long long *)(wb + L.o_len);
    A.ctl = (long long *)(wb + L.o_ctl); A.tile_read = (long long *)(wb + L.o_tread); A.tile_cnt = (long long *)(wb + L.o_tcnt);
    A.step = (uint8_t *)(wb + L.o_step); A.flag = (uint8_t *)(wb + L.o_flag);
    A.k = p->k; A.w = p->window;
    return A;
}

// units, tile, walk, count and the tiles' scan: after it tile_cnt holds every tile's first slot and ctl[CTL_NCHOSEN] the total
int ki_select(const KiArgs &A, const KiLayout &L, char *wb, hipStream_t s)
{
    GBX_HIP(hipMemsetAsync(A.ctl, 0, CTL_N * 8, s));
    GBX_HIP(hipMemsetAsync(A.tile_cnt, 0, (size_t)(L.nt + 1) * 8, s));
    Stage st("kmer_index_select", s);
    hipLaunchKernelGGL(ki_units_kernel, dim3(1), dim3(1024), 0, s, A);
    const unsigned grid = (unsigned)std::max(1ll, std::min<long long>(KI_GRID, L.nt));
    hipLaunchKernelGGL(ki_tile_kernel, dim3(grid), dim3(KI_THREADS), 0, s, A);
    hipLaunchKernelGGL(ki_walk_kernel, dim3((unsigned)std::max(1ll, std::min<long long>(KI_GRID * 4, (L.cap + 255) / 256))), dim3(256), 0, s, A);
    hipLaunchKernelGGL(ki_count_kernel, dim3(grid), dim3(KI_THREADS), 0, s, A);
    scan_launch1(A.tile_cnt, L.nt, (long long *)(wb + L.o_tsum), (int64_t *)&A.ctl[CTL_NCHOSEN], MemScanGuard{}, s);
    return GBX_OK;
}

}  // namespace

size_t kmer_index_workspace_bytes(int64_t n_reads, int64_t total_len, bool index) { return ki_layout(n_reads, total_len, index).total; }

int kmer_minimizers_launch(const gbx_kmer_index_params *p, const KmerIndexReads &rd, int64_t *d_mini_off, int32_t *d_mini_pos,
                           uint8_t *d_mini_rev, int64_t mini_cap, int64_t *d_n_mini, void *d_work, size_t work_bytes, hipStream_t s)
{
    const KiLayout L = ki_layout(rd.n_reads, rd.total_len, false);
    if (work_bytes < L.total) {
        set_error("kmer minimizers: workspace of %zu bytes, %lld reads of %lld bases need %zu", work_bytes, (long long)rd.n_reads,
                  (long long)rd.total_len, L.total);
        return GBX_ERR_ARG;
    }
    char *wb = (char *)d_work;
    const KiArgs A = ki_args(p, rd, wb, L);
    int rc = ki_select(A, L, wb, s);
    if (rc) return rc;
    {
        Stage st("kmer_index_emit", s);
        const unsigned grid = (unsigned)std::max(1ll, std::min<long long>(KI_GRID, L.nt));
        hipLaunchKernelGGL(ki_emit_kernel, dim3(grid), dim3(KI_THREADS), 0, s, A, EmitArgs{d_mini_pos, d_mini_rev, (long long)mini_cap, nullptr, nullptr});
        hipLaunchKernelGGL(ki_mini_off_kernel, dim3(mm_el_blocks(rd.n_reads + 1)), dim3(256), 0, s, A, d_mini_off, d_n_mini);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("kmer minimizers");
    return GBX_OK;
}

int kmer_index_launch(const gbx_kmer_index_params *p, const KmerIndexReads &rd, gbx_kmer_index_stats *d_stats, uint64_t *d_kmer,
                      int64_t *d_off, int64_t kmer_cap, uint64_t *d_pos, int64_t pos_cap, void *d_work, size_t work_bytes, hipStream_t s)
{
    const KiLayout L = ki_layout(rd.n_reads, rd.total_len, true);
    if (work_bytes < L.total) {
        set_error("kmer index: workspace of %zu bytes, %lld reads of %lld bases need %zu", work_bytes, (long long)rd.n_reads,
                  (long long)rd.total_len, L.total);
        return GBX_ERR_ARG;
    }
    char *wb = (char *)d_work;
    const KiArgs A = ki_args(p, rd, wb, L);
    GBX_HIP(hipMemsetAsync(d_stats, 0, sizeof(gbx_kmer_index_stats), s));
    int rc = ki_select(A, L, wb, s);
    if (rc) return rc;
    const SortBufs<uint64_t> S = sort_bufs(wb, L.S);
    {
        Stage st("kmer_index_emit", s);
        const unsigned grid = (unsigned)std::max(1ll, std::min<long long>(KI_GRID, L.nt));
        hipLaunchKernelGGL(ki_emit_kernel, dim3(grid), dim3(KI_THREADS), 0, s, A, EmitArgs{nullptr, nullptr, 0, S.a[0], S.b[0]});
    }
    int cur;
    {
        // least significant digits first: the position's bits in use, then the key's 2k
        Stage st("kmer_index_sort", s);
        SortPass pass[16];
        int n_pass = 0;
        const int bits[2] = {2 * p->k, std::max(1, bit_length(2ull * (unsigned long long)rd.total_len))};
        for (int word = 1; word >= 0; --word)
            for (int sh = 0; sh < bits[word]; sh += 8)
                pass[n_pass++] = SortPass{word, sh, (uint32_t)((1u << std::min(8, bits[word] - sh)) - 1)};
        cur = radix_sort<uint64_t>(S, SortCount{(const int64_t *)&A.ctl[CTL_NCHOSEN], L.cap}, pass, n_pass, s);
    }
    {
        Stage st("kmer_index_build", s);
        BuildArgs B{};
        B.key = S.a[cur]; B.gpos = S.b[cur];
        B.head = (long long *)S.a[cur ^ 1]; B.run_start = (long long *)S.b[cur ^ 1]; B.cnt2 = (long long *)(wb + L.o_cnt2);
        B.cap = L.cap; B.ctl = A.ctl; B.st = d_stats; B.rate = p->repeat_rate;
        B.kmer = d_kmer; B.off = d_off; B.kmer_cap = kmer_cap; B.pos = d_pos; B.pos_cap = pos_cap;
        const unsigned grid = mm_el_blocks(L.cap);
        hipLaunchKernelGGL(ki_head_kernel, dim3(grid), dim3(256), 0, s, B);
        scan_launch1(B.head, L.cap, (long long *)(wb + L.o_bsum2), &d_stats->n_distinct, MemScanGuard{}, s);
        hipLaunchKernelGGL(ki_runs_kernel, dim3(grid), dim3(256), 0, s, B);
        hipLaunchKernelGGL(ki_keep_kernel, dim3(grid), dim3(256), 0, s, B);
        MemScanJob J{};
        J.cnt = B.cnt2; J.n = L.cap; J.nq = 2; J.bsum = (long long *)(wb + L.o_bsum2); J.blocks = mem_scan_blocks(L.cap);
        J.total[0] = &d_stats->n_selected; J.total[1] = &d_stats->n_entries;
        mem_scan_launch(J, s);
        hipLaunchKernelGGL(ki_compact_kernel, dim3(grid), dim3(256), 0, s, B);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("kmer index");
    return GBX_OK;
}

}  // namespace gbx
