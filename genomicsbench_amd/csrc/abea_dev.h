// abea_dev.h — device functions that more than one abea kernel file uses: the rank of a base (abea_events_kernels.hip,
// abea_calib_kernels.hip), the wavefront scan over CIGAR operations and get_closest_event_to over the base-to-event map and its
// nearest-k-mer table (abea_calib_kernels.hip writes that table in the record's count pass; abea_eventalign_kernels.hip reads it).
#pragma once
#include "gbx_internal.h"

namespace gbx {
namespace abea_dev {

__device__ inline unsigned base_rank(char b) { return b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 0u; }   // align.c:10-23

constexpr int REC_WINDOW = 1000;           // get_closest_event_to, meth.c:107-108

__device__ inline long long rec_scan_incl(long long v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// get_closest_event_to, meth.c:105-117: backwards over k_idx .. max(0, k_idx - 1000) + 1, forwards over k_idx ..
// min(k_idx + 1000, n_kmers - 1) - 1; -1 is a legal result
__device__ inline int rec_closest(const int2 *mp, const int2 *nr, int k_idx, int n_kmers)
{
    const int stop_before = max(0, k_idx - REC_WINDOW), stop_after = min(k_idx + REC_WINDOW, n_kmers - 1);
    const int2 nn = nr[k_idx];
    const int before = nn.x > stop_before ? mp[nn.x].x : -1;
    const int after = nn.y < stop_after ? mp[nn.y].x : -1;
    return before == -1 ? after : before;
}

}  // namespace abea_dev
}  // namespace gbx
