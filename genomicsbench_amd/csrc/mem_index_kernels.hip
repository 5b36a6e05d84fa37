// mem_index_kernels.hip — the FM index of a genome, built on the device (the job of `bwa-mem2 index`).
// Input: l_pac base codes 0..3 of one strand.  The text is the strand and its reverse complement, n = 2 l_pac symbols; its
// N = n + 1 suffixes include the empty one, which sorts first (the convention of fmi.suffix_array).  Output: count[5],
// sentinel_index, the CP_OCC checkpoints and the suffix-array samples, byte for byte what fmi.build_index makes.
//
// Suffix array by prefix doubling on radix sorts (Larsson-Sadakane numbering: a suffix's rank is the slot of its group's head):
//   keys      the first 16 symbols of a suffix in 32 bits, zero-padded past the end, then min(16, n - i) in 5 bits
//   sort      LSD radix sort of (key, position), 8 bits a pass: radix_sort of dev_sort.hip, with the count the host knows
//   groups    a head flag per slot whose key differs from the slot before it; rank[sa[j]] = the slot of j's group head
//   rounds    h = 16, 32, ..: the slots of groups with more than one member are compacted (flags, scan; the host reads the
//             count), keyed by (group head << 32 | rank[pos + h] + 1, 0 past the end), sorted, written back in order to the
//             same slots, re-flagged, and only their ranks rewritten.  Keys are built before any rank changes.
//   bwt       one wavefront per 64 rows: four bit-reversed ballots are the one-hot words, their popcounts the block's counts;
//             mem_scan_launch turns the counts into cp_count and the totals into count[].
// Positions and ranks are 32-bit: N <= 2^32 - 1.  Every device loop here has a trip count the host fixed (a constant or a
// function of the launch's sizes); the one data-dependent loop is the host's round loop, bounded by ceil(log2 N) + 1.
#include "dev_prims.h"

namespace gbx {
namespace {

constexpr int EL = 1024;                                         // the element-wise kernels' block

using u32 = uint32_t;
using u64 = uint64_t;

inline long long el_blocks(long long m) { return (m + EL - 1) / EL; }

struct Layout {
    long long N;                          // suffixes
    size_t o_text, o_sa, o_rank, o_flags, o_cslot, o_key[2], o_val[2], o_hist, o_hsum, o_cnt, o_csum, o_bmax, o_misc, total;
    long long hist_entries, cnt_blocks;
};

Layout layout_of(int64_t l_pac)
{
    Layout L;
    const size_t N = (size_t)(2 * l_pac + 1);
    L.N = (long long)N;
    Carver take;
    L.o_text = take(N + 16);                                     // n symbols and zeros behind them (the key kernel reads 16 past any start)
    L.o_sa = take(N * 4);
    L.o_rank = take(N * 4);
    L.o_flags = take(N + 1);                                     // flags[N] = 1: the end closes the last group
    L.o_cslot = take(N * 4);
    L.o_key[0] = take(N * 8); L.o_key[1] = take(N * 8);          // the BWT pass's four count arrays live here afterwards
    L.o_val[0] = take(N * 4); L.o_val[1] = take(N * 4);
    L.hist_entries = 256 * sort_blocks((long long)N);
    L.o_hist = take(((size_t)L.hist_entries + 1) * 8);
    L.o_hsum = take((size_t)mem_scan_blocks(L.hist_entries) * 8);
    L.cnt_blocks = el_blocks((long long)N);
    L.o_cnt = take(((size_t)L.cnt_blocks + 1) * 8);
    L.o_csum = take((size_t)mem_scan_blocks(L.cnt_blocks) * 8);
    L.o_bmax = take((size_t)L.cnt_blocks * 4);
    L.o_misc = take(256);
    L.total = take.at;
    return L;
}

// ---- the text: the strand, then its reverse complement, then 16 zeros
__global__ void __launch_bounds__(EL) text_kernel(const uint8_t *g, long long l_pac, uint8_t *text, uint8_t *text_out)
{
    const long long i = (long long)blockIdx.x * EL + threadIdx.x;
    if (i < l_pac) {
        const uint8_t c = g[i];
        const long long j = 2 * l_pac - 1 - i;
        text[i] = c; text[j] = (uint8_t)(3 - c);
        if (text_out) { text_out[i] = c; text_out[j] = (uint8_t)(3 - c); }
    }
    if (i < 16) text[2 * l_pac + i] = 0;
}

// ---- the first keys: 16 symbols in 32 bits, the length (up to 16) in 5
__global__ void __launch_bounds__(EL) first_key_kernel(const uint8_t *text, long long N, u64 *key, u32 *val)
{
    const long long i = (long long)blockIdx.x * EL + threadIdx.x;
    if (i >= N) return;
    u32 k = 0;
#pragma unroll
    for (int d = 0; d < 16; ++d) k = k << 2 | (u32)(text[i + d] & 3);       // past the end: the zeros behind the text
    const long long left = N - 1 - i;
    key[i] = (u64)k << 5 | (u64)(left < 16 ? left : 16);
    val[i] = (u32)i;
}

// ---- after a sort of m elements: element k belongs in slot cslot[k] (null: k).  Writes the position there, the slot's head
// flag, and a block's last head slot + 1 (0: none) for the rank pass
__global__ void __launch_bounds__(EL) place_kernel(const u64 *key, const u32 *val, long long m, const u32 *cslot, u32 *sa, uint8_t *flags, u32 *bmax)
{
    __shared__ u32 sh[EL / 64];
    const long long k = (long long)blockIdx.x * EL + threadIdx.x;
    u32 hv = 0;
    if (k < m) {
        const u32 slot = cslot ? cslot[k] : (u32)k;
        const bool head = k == 0 || key[k] != key[k - 1];
        sa[slot] = val[k];
        flags[slot] = head ? 1 : 0;
        hv = head ? slot + 1 : 0;
    }
    for (int d = 32; d > 0; d >>= 1) { const u32 o = __shfl_xor(hv, d); hv = o > hv ? o : hv; }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = hv;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 x = 0;
        for (int w = 0; w < EL / 64; ++w) x = sh[w] > x ? sh[w] : x;
        bmax[blockIdx.x] = x;
    }
}

// one block: bmax[0 .. blocks) becomes its exclusive running maximum
__global__ void __launch_bounds__(1024) bmax_scan_kernel(u32 *bmax, long long blocks)
{
    __shared__ u32 sh[1024];
    __shared__ u32 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < blocks; b0 += 1024) {
        const long long i = b0 + threadIdx.x;
        sh[threadIdx.x] = i < blocks ? bmax[i] : 0;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const u32 u = threadIdx.x >= (u32)d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            if (u > sh[threadIdx.x]) sh[threadIdx.x] = u;
            __syncthreads();
        }
        const u32 before = threadIdx.x ? sh[threadIdx.x - 1] : 0;
        if (i < blocks) bmax[i] = before > carry ? before : carry;
        __syncthreads();
        if (threadIdx.x == 1023 && sh[1023] > carry) carry = sh[1023];
        __syncthreads();
    }
}

// rank[sa[slot]] = the head slot of the slot's group, for the m elements just placed (heads carry increasing slots, so the group
// head of element k is the running maximum of the head slots up to k)
__global__ void __launch_bounds__(EL) rank_kernel(const u32 *val, long long m, const u32 *cslot, const uint8_t *flags, const u32 *bmax, u32 *rank)
{
    __shared__ u32 sh[EL / 64];
    const long long k = (long long)blockIdx.x * EL + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 hv = 0;
    if (k < m) {
        const u32 slot = cslot ? cslot[k] : (u32)k;
        hv = flags[slot] ? slot + 1 : 0;
    }
    for (int d = 1; d < 64; d <<= 1) { const u32 o = __shfl_up(hv, d); if (lane >= d && o > hv) hv = o; }
    if (lane == 63) sh[wv] = hv;
    __syncthreads();
    u32 x = bmax[blockIdx.x];
    for (int w = 0; w < wv; ++w) x = sh[w] > x ? sh[w] : x;
    hv = hv > x ? hv : x;
    if (k < m) rank[val[k]] = hv - 1;                                       // element 0 is a head: hv >= 1
}

// ---- a round's work list: the slots whose group has more than one member
__device__ inline bool unresolved(const uint8_t *flags, long long j) { return !(flags[j] && flags[j + 1]); }

__global__ void __launch_bounds__(EL) open_count_kernel(const uint8_t *flags, long long N, long long *cnt)
{
    __shared__ u32 sh[EL / 64];
    const long long j = (long long)blockIdx.x * EL + threadIdx.x;
    const u64 bal = __ballot(j < N && unresolved(flags, j));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (u32)__builtin_popcountll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long c = 0;
        for (int w = 0; w < EL / 64; ++w) c += sh[w];
        cnt[blockIdx.x] = c;
    }
}

// cnt has become the blocks' offsets
__global__ void __launch_bounds__(EL) open_list_kernel(const uint8_t *flags, long long N, const long long *cnt, u32 *cslot)
{
    __shared__ long long sh[EL / 64];
    const long long j = (long long)blockIdx.x * EL + threadIdx.x;
    const bool open = j < N && unresolved(flags, j);
    long long total;
    const long long before = block_scan_excl(open ? 1 : 0, sh, &total);
    if (open) cslot[cnt[blockIdx.x] + before] = (u32)j;
}

// the keys of a round, from the ranks of the round before it
__global__ void __launch_bounds__(EL) round_key_kernel(const u32 *cslot, long long m, const u32 *sa, const u32 *rank, long long N, long long h, u64 *key, u32 *val)
{
    const long long k = (long long)blockIdx.x * EL + threadIdx.x;
    if (k >= m) return;
    const u32 p = sa[cslot[k]];
    const long long q = (long long)p + h;
    const u64 next = q < N ? (u64)rank[q] + 1 : 0;
    key[k] = (u64)rank[p] << 32 | next;
    val[k] = p;
}

// ---- BWT and checkpoints: one wavefront per 64 rows
__global__ void __launch_bounds__(256) bwt_kernel(const u32 *sa, const uint8_t *text, long long N, long long ncp, gbx_fmi_cp_occ *cp, long long *cnt, int64_t *info)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= ncp) return;
    const long long r = b * 64 + lane;
    int sym = 4;
    if (r < N) {
        const u32 p = sa[r];
        if (p == 0) info[5] = r; else sym = text[p - 1];
    }
    u64 word[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) word[c] = __brevll(__ballot(sym == c));
    if (lane < 4) {
        const u64 w = lane == 0 ? word[0] : lane == 1 ? word[1] : lane == 2 ? word[2] : word[3];
        cp[b].one_hot_bwt_str[lane] = w;
        cnt[(long long)lane * (ncp + 1) + b] = __builtin_popcountll(w);
    }
}

// cnt has become the checkpoints' counts, tot[c] the totals
__global__ void __launch_bounds__(256) cp_count_kernel(const long long *cnt, const int64_t *tot, long long ncp, gbx_fmi_cp_occ *cp, int64_t *info, long long rounds, long long first_open)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < ncp * 4) cp[t >> 2].cp_count[t & 3] = cnt[(t & 3) * (ncp + 1) + (t >> 2)];
    if (t == 0) {
        long long c = 1;
        info[0] = c;
        for (int k = 0; k < 4; ++k) { c += tot[k]; info[1 + k] = c; }
        info[6] = rounds; info[7] = first_open;
    }
}

__global__ void __launch_bounds__(EL) sample_kernel(const u32 *sa, long long N, long long n_sa, int compx, int8_t *ms, u32 *ls)
{
    const long long i = (long long)blockIdx.x * EL + threadIdx.x;
    if (i >= n_sa) return;
    const long long r = i << compx;
    ms[i] = 0;                                                              // positions are 32-bit here
    ls[i] = r < N ? sa[r] : 0;
}

thread_local std::vector<long long> last_rounds;      // the slots each round of this thread's last build sorted

// two quantities of n counts in one scan, their totals to t[0] and t[1]
void scan2(long long *cnt, long long n, long long *bsum, int64_t *t, hipStream_t s)
{
    MemScanJob J{};
    J.cnt = cnt; J.n = n; J.nq = 2; J.bsum = bsum; J.blocks = mem_scan_blocks(n);
    J.total[0] = t; J.total[1] = t + 1;
    mem_scan_launch(J, s);
}

}  // namespace

bool fmi_build_fits(int64_t l_pac) { return l_pac >= 1 && l_pac <= ((1ll << 32) - 2) / 2; }      // 2 l_pac + 1 <= 2^32 - 1

size_t fmi_build_workspace_bytes(int64_t l_pac)
{
    if (!fmi_build_fits(l_pac)) return 0;
    return layout_of(l_pac).total;
}

int fmi_build_rounds(int64_t *slots, int32_t cap, int32_t *n_rounds)
{
    *n_rounds = (int32_t)last_rounds.size();
    for (int32_t k = 0; k < cap && k < *n_rounds; ++k) slots[k] = last_rounds[(size_t)k];
    return GBX_OK;
}

int fmi_build_launch(const uint8_t *d_genome, int64_t l_pac, int32_t sa_compx, gbx_fmi_cp_occ *d_cp, int8_t *d_ms, uint32_t *d_ls, uint8_t *d_text,
                     int64_t *d_info, void *d_work, size_t work_bytes, hipStream_t s)
{
    const Layout L = layout_of(l_pac);
    if (work_bytes < L.total) { set_error("fmi build: workspace too small (%zu bytes, %zu needed)", work_bytes, L.total); return GBX_ERR_ARG; }
    char *const wb = (char *)d_work;
    const long long N = L.N;
    uint8_t *const text = (uint8_t *)(wb + L.o_text), *const flags = (uint8_t *)(wb + L.o_flags);
    u32 *const sa = (u32 *)(wb + L.o_sa), *const rank = (u32 *)(wb + L.o_rank), *const cslot = (u32 *)(wb + L.o_cslot), *const bmax = (u32 *)(wb + L.o_bmax);
    const SortBufs<u32> B{{(u64 *)(wb + L.o_key[0]), (u64 *)(wb + L.o_key[1])}, {(u32 *)(wb + L.o_val[0]), (u32 *)(wb + L.o_val[1])},
                          (long long *)(wb + L.o_hist), (long long *)(wb + L.o_hsum)};
    u64 *const *const key = B.a;
    u32 *const *const val = B.b;
    long long *const cnt = (long long *)(wb + L.o_cnt), *const csum = (long long *)(wb + L.o_csum);
    int64_t *const misc = (int64_t *)(wb + L.o_misc);                       // [0]: a round's open slots; [1 .. 4]: the BWT's totals
    const dim3 gN((unsigned)el_blocks(N)), tb(EL);

    {
        Stage st("mem_index_keys", s);
        hipLaunchKernelGGL(text_kernel, dim3((unsigned)el_blocks(std::max<long long>(l_pac, 16))), tb, 0, s, d_genome, (long long)l_pac, text, d_text);
        hipLaunchKernelGGL(first_key_kernel, gN, tb, 0, s, (const uint8_t *)text, N, key[0], val[0]);
        GBX_HIP(hipMemsetAsync(flags + N, 1, 1, s));
    }
    auto place = [&](int cur, long long m, const u32 *list) {
        const long long blocks = el_blocks(m);
        hipLaunchKernelGGL(place_kernel, dim3((unsigned)blocks), tb, 0, s, (const u64 *)key[cur], (const u32 *)val[cur], m, list, sa, flags, bmax);
        hipLaunchKernelGGL(bmax_scan_kernel, dim3(1), dim3(1024), 0, s, bmax, blocks);
        hipLaunchKernelGGL(rank_kernel, dim3((unsigned)blocks), tb, 0, s, (const u32 *)val[cur], m, list, (const uint8_t *)flags, (const u32 *)bmax, rank);
    };
    {
        Stage st("mem_index_sort0", s);
        const SortPass first[5] = {{0, 0, 255u}, {0, 8, 255u}, {0, 16, 255u}, {0, 24, 255u}, {0, 32, 255u}};      // 37 key bits
        const int cur = radix_sort(B, SortCount{nullptr, N}, first, 5, s);
        place(cur, N, nullptr);
    }
    GBX_HIP(hipGetLastError());
    int bits = 1;
    while (bits < 33 && (1ll << bits) <= N) ++bits;                          // N < 2^bits: ranks and ranks + 1 (at most N) fit
    SortPass pass[8];
    int n_pass = 0;
    for (int b = 0; b < bits; b += 8) pass[n_pass++] = SortPass{0, b, 255u};
    for (int b = 0; b < bits; b += 8) pass[n_pass++] = SortPass{0, 32 + b, 255u};
    const int max_rounds = bits + 1;                                        // ceil(log2 N) rounds can be needed; one more is an error
    long long rounds = 0, first_open = 0;
    last_rounds.clear();
    for (long long h = 16;; h <<= 1) {
        {
            Stage st("mem_index_open", s);
            hipLaunchKernelGGL(open_count_kernel, gN, tb, 0, s, (const uint8_t *)flags, N, cnt);
            scan_launch1(cnt, L.cnt_blocks, csum, misc, MemScanGuard{}, s);
        }
        long long m = -1;
        GBX_HIP(hipMemcpyAsync(&m, misc, 8, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipStreamSynchronize(s));
        if (m == 0) break;
        if (m < 2 || m > N) { set_error("fmi build: %lld open slots of %lld in round %lld (internal error)", m, N, rounds); return GBX_ERR_HIP; }
        if (rounds >= max_rounds) {
            set_error("fmi build: %lld slots still tied after %lld doubling rounds, more than %lld suffixes allow (internal error)", m, rounds, N);
            return GBX_ERR_HIP;
        }
        if (rounds == 0) first_open = m;
        last_rounds.push_back(m);
        ++rounds;
        Stage st("mem_index_round", s);
        hipLaunchKernelGGL(open_list_kernel, gN, tb, 0, s, (const uint8_t *)flags, N, (const long long *)cnt, cslot);
        hipLaunchKernelGGL(round_key_kernel, dim3((unsigned)el_blocks(m)), tb, 0, s, (const u32 *)cslot, m, (const u32 *)sa, (const u32 *)rank, N, h, key[0], val[0]);
        const int cur = radix_sort(B, SortCount{nullptr, m}, pass, n_pass, s);
        place(cur, m, cslot);
        GBX_HIP(hipGetLastError());
    }
    {
        Stage st("mem_index_bwt", s);
        const long long ncp = (N >> 6) + 1;
        long long *const bc = (long long *)key[0];                          // 4 (ncp + 1) counts: far below the key buffer's 8 N bytes
        long long *const bs = (long long *)key[1];
        GBX_HIP(hipMemsetAsync(d_info, 0, 64, s));
        hipLaunchKernelGGL(bwt_kernel, dim3((unsigned)((ncp + 3) / 4)), dim3(256), 0, s, (const u32 *)sa, (const uint8_t *)text, N, ncp, d_cp, bc, d_info);
        scan2(bc, ncp, bs, misc + 1, s);
        scan2(bc + 2 * (ncp + 1), ncp, bs, misc + 3, s);
        hipLaunchKernelGGL(cp_count_kernel, dim3((unsigned)((ncp * 4 + 255) / 256)), dim3(256), 0, s, (const long long *)bc, (const int64_t *)(misc + 1), ncp, d_cp,
                           d_info, rounds, first_open);
        const long long n_sa = sa_compx ? (N >> 3) + 1 : N;
        hipLaunchKernelGGL(sample_kernel, dim3((unsigned)el_blocks(n_sa)), tb, 0, s, (const u32 *)sa, N, n_sa, (int)sa_compx, d_ms, d_ls);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("fmi build");
    return GBX_OK;
}

}  // namespace gbx
