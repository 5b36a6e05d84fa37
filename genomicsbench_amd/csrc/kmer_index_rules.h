// kmer_index_rules.h — the rules of Flye's minimizer index (VertexIndex::buildIndexMinimizers, R/vertex_index.cpp:389-497) that
// kmer_index_kernels.hip applies, for the device and for the plain host compiler (no HIP header in that mode):
// tests/hostcheck/kmer_index_check.cpp builds it with g++ and the CPU tests hold it against their literal restatement of the
// reference's deque (tests/kmer_index_ref.py).  DESIGN 3.7.1.
//   k-mers     positions 0 .. len - k - 1; code = 2 bits a base, first base most significant; canonical = min(fwd, revcomp),
//              "reversed" only when revcomp < fwd (R/kmer.h:54-63: a palindrome stays forward)
//   hash       splitmix64 of the canonical code (R/kmer.h:91-98), a bijection
//   selection  yieldMinimizers (R/kmer.h:206-262) as a recurrence on the deque's front position F with no other state:
//                  next(F) = the first s in (F, F + w) with h[s] < h[F], if there is one
//                          = the RIGHTMOST argmin of h over [F + 1, F + w] otherwise (the chain ends if F + w >= len - k)
//              and the minimizers are 0, next(0), next(next(0)), ...  A position whose hash is strictly below every hash of the
//              w - 1 positions before it is on the chain whatever came earlier (a reset point): the front before it either
//              loses to it at once or expires exactly when it is the rightmost minimum.  Position 0 is one, and with w = 1
//              every position is.
//   positions  SequenceContainer::globalPosition: read r occupies [G_r, G_r + L), its reverse complement [G_r + L, G_r + 2 L)
//   filter     filterFrequentKmers(1, rate) in fp32, round to nearest, the product truncated to an integer
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GBX_KI_HD __host__ __device__ inline
#else
#define GBX_KI_HD inline
#endif

namespace gbx {

constexpr int KI_MAX_K = 31;                       // 1 << 64 is undefined in the reference's own mask at 32
constexpr int KI_MAX_WINDOW = 64;                  // the step to the next minimizer fits the halo the tile kernel keeps
constexpr int KI_THREADS = 256;                    // a workgroup of the tile kernels: four wavefronts
constexpr int KI_LANE = 8;                         // consecutive positions a lane takes
constexpr int KI_WAVE = 64 * KI_LANE;              // ... a wavefront
constexpr int KI_TILE = KI_THREADS * KI_LANE;      // ... a workgroup: the tile; a read's tiles start at multiples of it
constexpr int KI_HALO = KI_MAX_WINDOW;             // hashes kept on either side of a tile
constexpr long long KI_MAX_GLOBAL = 1ll << 40;     // 2 * total_len stays below it (the reference's 5-byte IndexChunk)
constexpr float KI_MAX_RATE = 1048576.0f;          // repeat_rate in [0, 2^20]: rate * mean stays far inside 64 bits

// The tiles of one read: KI_TILE positions each, the last one shorter; none for len <= k.
GBX_KI_HD long long ki_read_tiles(long long len, int k)
{
    const long long np = len - k > 0 ? len - k : 0;
    return (np + KI_TILE - 1) / KI_TILE;
}

GBX_KI_HD uint64_t ki_hash(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one base (its low two bits) enters on the right of the forward code and on the left of the reverse complement's
GBX_KI_HD void ki_roll(uint64_t *fwd, uint64_t *rev, unsigned base, int k)
{
    const uint64_t mask = (1ull << (2 * k)) - 1;          // k <= 31
    const unsigned c = base & 3u;
    *fwd = ((*fwd << 2) | c) & mask;
    *rev = (*rev >> 2) | ((uint64_t)(3u - c) << (2 * (k - 1)));
}

// the canonical code; *reversed: the reference's standardForm()
GBX_KI_HD uint64_t ki_canonical(uint64_t fwd, uint64_t rev, bool *reversed)
{
    *reversed = rev < fwd;
    return rev < fwd ? rev : fwd;
}

// The step from the chain position F to next(F), 0 where the chain ends.  h points at F's hash, h[j] is position F + j's;
// room = (len - k) - F positions exist from F on, so only h[0 .. room) is read.  1 <= w <= KI_MAX_WINDOW; the result is <= w.
GBX_KI_HD int ki_next_step(const uint64_t *h, long long room, int w)
{
    const uint64_t hf = h[0];
    for (int j = 1; j < w; ++j) {
        if (j >= room) return 0;
        if (h[j] < hf) return j;
    }
    if (w >= room) return 0;
    int best = 1;
    uint64_t hb = h[1];
    for (int j = 2; j <= w; ++j)
        if (h[j] <= hb) { hb = h[j]; best = j; }
    return best;
}

// Whether position s is a reset point.  h points at s's hash, h[-j] is position s - j's; only h[-min(s, w - 1)] .. h[0] is read.
GBX_KI_HD bool ki_is_reset(const uint64_t *h, long long s, int w)
{
    const int back = s < w - 1 ? (int)s : w - 1;
    for (int j = 1; j <= back; ++j)
        if (h[-j] <= h[0]) return false;
    return true;
}

// The global position of the canonical strand's copy of the k-mer at p of a read of L bases whose forward copy starts at g
// (g = 2 * the lengths of the reads before it): a reversed k-mer lies in the reverse complement held right behind the read.
GBX_KI_HD uint64_t ki_global_pos(uint64_t g, int64_t L, int64_t p, int k, bool reversed)
{
    return reversed ? g + (uint64_t)L + (uint64_t)(L - p - k) : g + (uint64_t)p;
}

// the float conversions and the divide of the filter, round to nearest in both builds (never a fast-math form: the
// truncation below makes one ulp visible)
GBX_KI_HD float ki_to_float(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ull2float_rn(v);
#else
    return (float)v;
#endif
}

GBX_KI_HD float ki_div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

GBX_KI_HD float ki_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}

// filterFrequentKmers(1, rate): the mean of `total` chosen positions over `unique` k-mers, (float)total / (unique + 1) with the
// divisor converted to float as C does it ...
GBX_KI_HD float ki_mean_frequency(uint64_t total, uint64_t unique) { return ki_div(ki_to_float(total), ki_to_float(unique + 1)); }

// ... and _repetitiveFrequency = rate * mean, a float truncated on assignment to a size_t; a k-mer with more chosen positions
// than that leaves the index.  0 <= rate <= KI_MAX_RATE.
GBX_KI_HD uint64_t ki_repetitive_frequency(float mean, float rate) { return (uint64_t)ki_mul(rate, mean); }

GBX_KI_HD bool ki_is_repetitive(uint64_t capacity, uint64_t repetitive_frequency) { return capacity > repetitive_frequency; }

}  // namespace gbx
