// kmer_split.h — how kmer_kernels.hip cuts its work, for the device and for the plain host compiler (no HIP header in that
// mode): tests/hostcheck/kmer_split_check.cpp builds it with g++, so that the boundary cases of tests/kmer_cases.py are
// held against the kernels' own idea of where a unit, a sweep workgroup and a slice end.
//   units   a read of len bases has max(0, len - k) counted positions, in units of KC_CHUNK consecutive ones
//   sweeps  a slice of n counters is swept by nb <= KC_MAX_BLOCKS workgroups of `per` counters each, per a multiple of KC_SWEEP
//   slices  the 4^k counters are processed KC_SLICE at a time: one slice for k <= 15, 4 for k = 16, 16 for k = 17
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GBX_KMER_HD __host__ __device__ inline
#else
#define GBX_KMER_HD inline
#endif

namespace gbx {

constexpr int KC_CHUNK = 256;                      // positions per unit of the count pass
constexpr int KC_THREADS = 256;
constexpr int KC_SWEEP = KC_THREADS * 4;           // counters a workgroup of the sweeps covers per round (one uint4 a lane)
constexpr int KC_MAX_BLOCKS = 2048;                // workgroups of the sweeps
constexpr long long KC_SLICE = 1ll << 30;          // counters per slice

// The units of one read: KC_CHUNK positions each, the last one shorter; none for len <= k.
GBX_KMER_HD long long kmer_read_units(long long len, int k)
{
    const long long np = len - k > 0 ? len - k : 0;
    return (np + KC_CHUNK - 1) / KC_CHUNK;
}

// The sweeps' split of a slice: nb workgroups of `per` counters each (a multiple of KC_SWEEP), the last one shorter.
GBX_KMER_HD void sweep_split(long long n, int *nb, long long *per)
{
    const long long rounds = (n + KC_SWEEP - 1) / KC_SWEEP;
    const long long rpb = (rounds + KC_MAX_BLOCKS - 1) / KC_MAX_BLOCKS;
    *per = rpb * KC_SWEEP;
    *nb = (int)((n + *per - 1) / *per);
}

// Counters per slice and slices of the 4^k code space.
GBX_KMER_HD long long kmer_slice_n(int k)
{
    const long long space = 1ll << (2 * k);
    return space < KC_SLICE ? space : KC_SLICE;
}

GBX_KMER_HD long long kmer_n_slices(int k) { return (1ll << (2 * k)) / kmer_slice_n(k); }

}  // namespace gbx
