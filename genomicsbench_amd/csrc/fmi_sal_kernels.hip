// fmi_sal_kernels.hip — suffix-array lookup of SMEM hits (bwa-mem2's FMI_search::get_sa_entry) for gfx950 (MI355X).
//
// Semantics (include/gbx.h): the hits of an SMEM [k, k + s) are rows k + i step as bwa-mem's mem_chain samples them; the
// SA of a row is found by walking the LF mapping until a sampled row (or the sentinel row) is reached, counting the steps.
// Any correct walk gives the true SA, so the result is pinned by an independently computed suffix array.
//
// What bounds it: one LF step is one random 64-byte line of the checkpoint table - the look-up fmi_smem_kernel is built
// around - and a hit is a chain of dependent steps (about 8 at 1-in-8 sampling, geometric, a tail of walks
// into the hundreds).  Millions of independent chains: the kernel keeps as many lines in flight as it can.
//   * four lanes per hit, lane b = base b: lane b loads the 16-byte {count, one-hot} pair of base b from the device
//     checkpoint layout (the quad's four loads are one line); the lane whose one-hot bit is set at the row is the row's
//     BWT symbol and computes LF, two DPP quad_perm steps OR it into all four lanes.
//   * a trip of the main loop issues every load a quad needs next together - the checkpoint line of a walking hit, the
//     sample of a finished one, the record of the quad's next SMEM - so a hit that ends costs the wavefront no extra wait.
//   * quads draw SAL_CHUNK consecutive hits from a cursor (walk lengths vary too much for a fixed share per quad); the SMEM
//     of a chunk's first hit is one load from a table the scan fills (chunk -> SMEM), after that the SMEM advances with the
//     hits.  (A binary search of pos_off per chunk instead - ~23 dependent loads for 8.6 M SMEMs - measured the same:
//     14.82 against 14.83 ms for the 36 M hits of 1 M reads on the 'large' shape, profiles/fmi_sal_time.json.)
//   * rows and samples in 32 bits when the text has fewer than 2^32 rows, in 64 otherwise (two instances, as fmi).
//   * per-SMEM hit counts and their exclusive scan (pos_off) are computed on the device from the device SMEM count, so
//     the lookup chains behind gbx_fmi_smem_device on one stream.
#include <algorithm>
#include "dev_prims.h"

namespace gbx {
namespace {

constexpr int SAL_SCAN = 1024;                    // pos_off entries per block of the count scan
constexpr int SAL_CHUNK = 32;                     // consecutive hits a quad draws from the cursor at a time
constexpr long long SAL_MAX_BLOCKS = 256ll * 4 * 8;   // resident wavefronts on 256 CUs at eight per SIMD

struct SalArgs {
    const uint4 *index;                // device checkpoint layout of fmi_index_build: checkpoint i, base b at 4 i + b
    long long count[5];
    long long sentinel, ref_seq_len;
    const void *sa;                    // samples, 4 or 8 bytes each (fmi_sa_build)
    int sa_compx;
    const gbx_fmi_smem *smems;
    const int64_t *n_smem;             // on the device; at most smem_cap are used
    long long smem_cap, max_occ;
    int64_t *pos;
    long long pos_cap;
    int64_t *pos_off;                  // smem_cap + 1 entries
    int64_t *n_pos;
    unsigned long long *counters;      // [0] hit cursor, [1] LF steps, [2] longest walk of a hit
    long long *bsum;                   // per-block sums of the count scan
    long long *chunk_smem;             // [pos_cap / SAL_CHUNK + 1]: the SMEM of hit c SAL_CHUNK
    long long n_chunk;
};

template <int CTRL> __device__ inline unsigned dpp(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true); }
template <int CTRL> __device__ inline unsigned long long dpp(unsigned long long v)
{
    return ((unsigned long long)dpp<CTRL>((unsigned)(v >> 32)) << 32) | dpp<CTRL>((unsigned)v);
}
constexpr int QP_BCAST0 = 0x00, QP_XOR1 = 0xb1, QP_XOR2 = 0x4e;     // quad_perm [0,0,0,0], [1,0,3,2], [2,3,0,1]

__device__ inline long long sal_n_smem(const SalArgs &A)
{
    const long long n = *A.n_smem;
    return n < 0 ? 0 : n > A.smem_cap ? A.smem_cap : n;
}
__device__ inline bool sal_bad(long long k, long long s, long long len) { return k < 0 || s < 1 || k > len - s; }
// min(s, max_occ) (every row for max_occ <= 0); a bad SMEM counts as min(s, ref_seq_len)
__device__ inline long long sal_hits(long long s, long long max_occ, long long len)
{
    if (s < 1) return 0;
    if (s > len) s = len;
    return max_occ > 0 && s > max_occ ? max_occ : s;
}

// ---- per-SMEM hit counts -> pos_off (exclusive scan over smem_cap + 1 entries; those past the SMEM count repeat the total)
__global__ void __launch_bounds__(SAL_SCAN) fmi_sal_count_kernel(SalArgs A)
{
    __shared__ long long sh[SAL_SCAN / 64];
    const long long n = sal_n_smem(A);
    const long long i = (long long)blockIdx.x * SAL_SCAN + threadIdx.x;
    const long long c = i < n ? sal_hits(A.smems[i].s, A.max_occ, A.ref_seq_len) : 0;
    long long total;
    const long long before = block_scan_excl(c, sh, &total);
    if (i <= A.smem_cap) A.pos_off[i] = before;
    if (threadIdx.x == SAL_SCAN - 1) A.bsum[blockIdx.x] = total;
}

// one block: exclusive scan of the block sums, the total to *n_pos, the counters reset
__global__ void __launch_bounds__(1024) fmi_sal_scan_kernel(long long *bsum, int n_blocks, unsigned long long *counters, int64_t *n_pos)
{
    const long long carry = scan_block_sums(bsum, n_blocks);
    if (threadIdx.x == 0) {
        *n_pos = carry;
        counters[0] = 0; counters[1] = 0; counters[2] = 0;
    }
}

__global__ void __launch_bounds__(SAL_SCAN) fmi_sal_offset_kernel(int64_t *pos_off, long long smem_cap, const long long *bsum)
{
    const long long i = (long long)blockIdx.x * SAL_SCAN + threadIdx.x;
    if (i <= smem_cap) pos_off[i] += bsum[blockIdx.x];
}

// the SMEM of every chunk's first hit: SMEM j writes the chunks that start among its hits
__global__ void __launch_bounds__(SAL_SCAN) fmi_sal_chunk_kernel(SalArgs A)
{
    const long long n = sal_n_smem(A);
    const long long i = (long long)blockIdx.x * SAL_SCAN + threadIdx.x;
    if (i >= n) return;
    const long long a = A.pos_off[i], e = A.pos_off[i + 1];
    for (long long c = (a + SAL_CHUNK - 1) / SAL_CHUNK; c * SAL_CHUNK < e && c < A.n_chunk; ++c) A.chunk_smem[c] = i;
}

// ---- the walks.  IV: rows and samples, unsigned when the text has fewer than 2^32 rows, else unsigned long long.
template <class IV>
__global__ void __launch_bounds__(64, 8) fmi_sal_kernel(SalArgs A)
{
    __shared__ IV cnt_lds[8];
    const int lane = threadIdx.x, b = lane & 3;
    if (lane < 5) cnt_lds[lane] = (IV)A.count[lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    typedef __attribute__((address_space(3))) const IV lds_iv;        // typed LDS pointer: ds_read, not a FLAT load
    const IV cnt_b = ((lds_iv *)cnt_lds)[b];                           // lane b only ever needs count[b]
    const long long n_pos = *A.n_pos, n_hits = n_pos < A.pos_cap ? n_pos : A.pos_cap;     // nothing past pos_cap is written
    const long long n_smem = sal_n_smem(A), len = A.ref_seq_len;
    const IV sentinel = (IV)A.sentinel, smask = (IV)((1u << A.sa_compx) - 1u);
    const int cx = A.sa_compx;
    const IV *const sa = (const IV *)A.sa;

    // quad-uniform state
    long long h = 0, h_end = 0;                  // current hit, end of the quad's chunk
    long long j = 0, jend = 0;                   // current SMEM, end of its hits
    long long nk = 0, ns = 0, njend = 0;         // SMEM j + 1: record and end of its hits, requested one trip ahead
    bool want_next = false, bad = false;
    IV row = 0, step = 1;                        // start row of hit h, row step of SMEM j
    IV r = 0;                                    // the walk of hit h
    unsigned t = 0, max_t = 0;
    unsigned long long n_steps = 0;
    GBX_GUARD(gd_walk, 0);                       // LF steps the current hit may still take (ref_seq_len)
    GBX_GUARD(gd_skip, 0);                       // SMEMs without hits skipped in one go (smem_cap)

    auto load_smem = [&](long long jj, long long &k_, long long &s_, long long &e_) {
        if (jj < n_smem) { k_ = A.smems[jj].k; s_ = A.smems[jj].s; e_ = A.pos_off[jj + 1]; }
        else { k_ = 0; s_ = 0; e_ = n_hits; }
    };
    auto enter_smem = [&](long long k_, long long s_) {
        bad = sal_bad(k_, s_, len);
        step = (!bad && A.max_occ > 0 && s_ > A.max_occ) ? (IV)(s_ / A.max_occ) : (IV)1;
        row = bad ? (IV)0 : (IV)k_;
        want_next = true;
    };
    auto begin_hit = [&]() {
        r = row; t = 0;
#ifdef GBX_LOOP_GUARD
        gd_walk = len;
#endif
    };
    // SAL_CHUNK hits from the cursor; the SMEM of the first from the chunk table
    auto draw = [&]() -> bool {
        unsigned long long c = 0;
        if (b == 0) c = atomicAdd(&A.counters[0], (unsigned long long)SAL_CHUNK);
        c = dpp<QP_BCAST0>(c);
        if ((long long)c >= n_hits) return false;
        h = (long long)c;
        h_end = h + SAL_CHUNK < n_hits ? h + SAL_CHUNK : n_hits;
        j = A.chunk_smem[h / SAL_CHUNK];
        long long k_, s_;
        load_smem(j, k_, s_, jend);
        enter_smem(k_, s_);
        if (!bad) row += (IV)(h - A.pos_off[j]) * step;
        return true;
    };
    // hit h is the first past SMEM j: on to the next SMEM with hits
    auto advance = [&]() {
        ++j;
        long long k_ = nk, s_ = ns;
        jend = njend;
#ifdef GBX_LOOP_GUARD
        gd_skip = A.smem_cap;
#endif
        while (jend <= h) {
            if (GBX_GUARD_TRIP(gd_skip, GBX_GK_FMI, 4, h)) { jend = h_end; break; }
            ++j;
            load_smem(j, k_, s_, jend);
        }
        enter_smem(k_, s_);
    };

    bool live = draw();
    if (live) begin_hit();
    for (;;) {
        if (__ballot(live) == 0) break;
        // every load the quad needs next, issued together: the checkpoint line of the row, or the sample that ends the walk;
        // and the record of SMEM j + 1 when the quad has just entered SMEM j
        const bool in = r < (IV)len;                                   // (a consistent index never leaves the table)
        const bool sampled = (r & smask) == 0;
        const bool walk = live && !bad && in && !sampled && r != sentinel;
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        IV smp = 0;
        if (walk) c = A.index[(size_t)(r >> 6) * 4 + b];
        // one 16-byte request per lane also in the 32-bit instance, which has no use for the count's upper word
        asm volatile("" : "+v"(c.x), "+v"(c.y), "+v"(c.z), "+v"(c.w));
        if (live && !bad && in && sampled) smp = sa[(size_t)(r >> cx)];
        if (live && want_next) { load_smem(j + 1, nk, ns, njend); want_next = false; }
        if (walk) {
            const int y = (int)(r & 63);
            const unsigned long long oh = ((unsigned long long)c.w << 32) | c.z;
            const bool mine = (oh >> (63 - y)) & 1ull;                 // this lane's base is the BWT symbol at r
            const unsigned long long m = y ? ~0ull << (64 - y) : 0ull;
            const unsigned pc = (unsigned)__builtin_popcountll(oh & m);
            const IV occ = sizeof(IV) == 4 ? (IV)(c.x + pc) : (IV)((((unsigned long long)c.y << 32) | c.x) + pc);
            IV v = mine ? cnt_b + occ : (IV)0;
            v |= dpp<QP_XOR1>(v);
            v |= dpp<QP_XOR2>(v);
            r = v;
            ++t;
            if (GBX_GUARD_TRIP(gd_walk, GBX_GK_FMI, 3, h)) r = (IV)len;  // (given up: the call fails)
        } else if (live) {
            const long long v = bad || !in ? -1ll : sampled ? (long long)smp + (long long)t : (long long)t;
            if (b == 0) A.pos[h] = v;
            n_steps += t;
            max_t = t > max_t ? t : max_t;
            ++h;
            if (h >= h_end) live = draw();
            else if (h >= jend) advance();
            else row += step;
            if (live) begin_hit();
        }
    }
    // LF steps of the wavefront (one count per quad) and its longest walk
    unsigned long long tot = b == 0 ? n_steps : 0;
    unsigned mx = max_t;
    for (int d = 32; d; d >>= 1) {
        tot += __shfl_xor(tot, d);
        const unsigned o = (unsigned)__shfl_xor((int)mx, d);
        mx = o > mx ? o : mx;
    }
    if (lane == 0 && tot) atomicAdd(&A.counters[1], tot);
    if (lane == 0 && mx) atomicMax(&A.counters[2], (unsigned long long)mx);
}

// the file's samples (int8 upper bytes, uint32 lower words) -> one word per sample
template <class W>
__global__ void __launch_bounds__(256) fmi_sa_kernel(const int8_t *ms, const uint32_t *ls, long long n, W *dst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dst[i] = (W)(((unsigned long long)(uint8_t)ms[i] << 32) | ls[i]);
}

struct SalLayout { size_t o_bsum, o_chunk, total; int blocks; long long n_chunk; };
SalLayout sal_layout(int64_t smem_cap, int64_t pos_cap)
{
    SalLayout L;
    L.blocks = (int)((smem_cap + 1 + SAL_SCAN - 1) / SAL_SCAN);
    L.n_chunk = pos_cap / SAL_CHUNK + 1;
    L.o_bsum = 64;                                                     // counters: 8 x u64
    L.o_chunk = L.o_bsum + (((size_t)L.blocks * 8 + 255) & ~(size_t)255);
    L.total = L.o_chunk + (((size_t)L.n_chunk * 8 + 255) & ~(size_t)255);
    return L;
}

}  // namespace

bool fmi_sa_wide(int64_t ref_seq_len)
{
    const char *w = getenv("GBX_FMI_WIDE");
    return ref_seq_len >= (1ll << 32) || (w && atoi(w));
}

size_t fmi_sa_bytes(int64_t n_sa, int64_t ref_seq_len)
{
    return n_sa > 0 ? (size_t)n_sa * (fmi_sa_wide(ref_seq_len) ? 8 : 4) : 0;
}

static int sa_check(const gbx_fmi_sa *sa, int64_t ref_seq_len, const char *who)
{
    if (sa->sa_compx != 0 && sa->sa_compx != 3) { set_error("%s: sa_compx must be 3 or 0", who); return GBX_ERR_ARG; }
    if (ref_seq_len < 2 || ref_seq_len >= (1ll << 40)) { set_error("%s: bad reference length", who); return GBX_ERR_ARG; }
    const int64_t want = sa->sa_compx ? (ref_seq_len >> 3) + 1 : ref_seq_len;
    if (sa->n_sa != want) {
        set_error("%s: n_sa = %lld, sa_compx %d wants %lld", who, (long long)sa->n_sa, sa->sa_compx, (long long)want);
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int fmi_sa_build(const gbx_fmi_sa *sa, int64_t ref_seq_len, void *d_sa, size_t sa_bytes, hipStream_t s)
{
    int rc = sa_check(sa, ref_seq_len, "gbx_fmi_sa_build");
    if (rc) return rc;
    if (sa_bytes < fmi_sa_bytes(sa->n_sa, ref_seq_len)) { set_error("gbx_fmi_sa_build: device sample buffer too small"); return GBX_ERR_ARG; }
    const long long n = sa->n_sa;
    const dim3 g((unsigned)((n + 255) / 256)), tb(256);
    Stage st("fmi_sa", s);
    if (fmi_sa_wide(ref_seq_len)) hipLaunchKernelGGL(fmi_sa_kernel<unsigned long long>, g, tb, 0, s, sa->ms_byte, sa->ls_word, n, (unsigned long long *)d_sa);
    else hipLaunchKernelGGL(fmi_sa_kernel<unsigned>, g, tb, 0, s, sa->ms_byte, sa->ls_word, n, (unsigned *)d_sa);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

size_t fmi_sal_workspace_bytes(int64_t smem_cap, int64_t pos_cap) { return sal_layout(smem_cap < 0 ? 0 : smem_cap, pos_cap < 0 ? 0 : pos_cap).total; }

int fmi_sal_launch(const gbx_fmi_index *idx, const void *d_index, const gbx_fmi_sa *sa, const void *d_sa, const gbx_fmi_smem *d_smems,
                   const int64_t *d_n_smem, int64_t smem_cap, int32_t max_occ, int64_t *d_pos, int64_t pos_cap, int64_t *d_pos_off,
                   int64_t *d_n_pos, void *d_work, size_t work_bytes, hipStream_t s)
{
    int rc = sa_check(sa, idx->ref_seq_len, "fmi sal");
    if (rc) return rc;
    const SalLayout L = sal_layout(smem_cap, pos_cap);
    if (work_bytes < L.total) { set_error("fmi sal: workspace too small"); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    SalArgs A;
    A.index = (const uint4 *)d_index;
    for (int c = 0; c < 5; ++c) A.count[c] = idx->count[c];
    A.sentinel = idx->sentinel_index; A.ref_seq_len = idx->ref_seq_len;
    A.sa = d_sa; A.sa_compx = sa->sa_compx;
    A.smems = d_smems; A.n_smem = d_n_smem; A.smem_cap = smem_cap; A.max_occ = max_occ;
    A.pos = d_pos; A.pos_cap = pos_cap; A.pos_off = d_pos_off; A.n_pos = d_n_pos;
    A.counters = (unsigned long long *)wb;
    A.bsum = (long long *)(wb + L.o_bsum);
    A.chunk_smem = (long long *)(wb + L.o_chunk);
    A.n_chunk = L.n_chunk;
    {
        Stage st("fmi_sal_count", s);
        hipLaunchKernelGGL(fmi_sal_count_kernel, dim3(L.blocks), dim3(SAL_SCAN), 0, s, A);
        hipLaunchKernelGGL(fmi_sal_scan_kernel, dim3(1), dim3(1024), 0, s, A.bsum, L.blocks, A.counters, d_n_pos);
        hipLaunchKernelGGL(fmi_sal_offset_kernel, dim3(L.blocks), dim3(SAL_SCAN), 0, s, d_pos_off, (long long)smem_cap, (const long long *)A.bsum);
        hipLaunchKernelGGL(fmi_sal_chunk_kernel, dim3(L.blocks), dim3(SAL_SCAN), 0, s, A);
    }
    // the hit count is only known on the device: the grid is sized for pos_cap hits (a wavefront without work leaves at once)
    const long long want = (pos_cap + 16 * SAL_CHUNK - 1) / (16 * SAL_CHUNK);
    const long long blocks = std::max<long long>(1, std::min<long long>(want, SAL_MAX_BLOCKS));
    if (pos_cap > 0) {
        Stage st("fmi_sal", s);
        if (fmi_sa_wide(idx->ref_seq_len)) hipLaunchKernelGGL(fmi_sal_kernel<unsigned long long>, dim3((unsigned)blocks), dim3(64), 0, s, A);
        else hipLaunchKernelGGL(fmi_sal_kernel<unsigned>, dim3((unsigned)blocks), dim3(64), 0, s, A);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("fmi sal");
    return GBX_OK;
}

int fmi_sal_read_steps(const void *d_work, int64_t *steps, int64_t *max_steps, hipStream_t s)
{
    unsigned long long v[3] = {0, 0, 0};
    GBX_HIP(hipMemcpyAsync(v, d_work, sizeof(v), hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    if (steps) *steps = (int64_t)v[1];
    if (max_steps) *max_steps = (int64_t)v[2];
    return GBX_OK;
}

}  // namespace gbx
