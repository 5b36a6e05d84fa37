// abea_meth_rules.h — the rules of the call-methylation site planner (calculate_methylation_for_read, meth.c:500-658) and of the
// per-job checks of the score plan, per group, per position and per job, as functions the device kernels
// (abea_meth_plan_kernels.hip) and a host program (tests/sanitize_abea_meth) compile from the same text.  Nothing here allocates,
// loops over more than a binary search's 32 steps, or reads outside the segment, the record or the job it is handed.
// sites_of_read in capi_abea_meth.hip states the same rules serially and stays the independent yardstick.
#pragma once
#include <stdint.h>
#include "../../include/gbx.h"

#if defined(__HIPCC__)
#define GBX_AMR_HD __host__ __device__
#else
#define GBX_AMR_HD
#endif

namespace gbx {
namespace abea_meth_rules {

constexpr int MIN_SEPARATION = 10;         // meth.c:533
constexpr int MAX_SPAN = 200;              // meth.c:571
constexpr int SEARCH_STEPS = 32;           // a lower bound over at most 2^31 pairs

// ---- per position
GBX_AMR_HD inline char upper(char c) { return c >= 'a' && c <= 'z' ? (char)(c - 'a' + 'A') : c; }          // toupper, C locale

GBX_AMR_HD inline char possible0(char c)                     // getPossibleSymbols(c)[0], meth.c:221-256
{
    switch (c) {
        case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 'A';
        case 'C': case 'S': case 'Y': case 'B': return 'C';
        case 'G': case 'K': return 'G';
        case 'T': return 'T';
        default: return 'A';                                 // not a IUPAC symbol (the reference asserts): ranks as A
    }
}

GBX_AMR_HD inline char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'T'; }     // meth.c:261-273

// base i of the disambiguated segment (meth.c:288-306): only A, C, G, T come out
GBX_AMR_HD inline char ref_base(const char *ref, int64_t i) { return possible0(upper(ref[i])); }

// a CpG starts at i: C followed by G inside the segment
GBX_AMR_HD inline bool cpg_at(const char *ref, int64_t ref_len, int64_t i)
{
    return i >= 0 && i + 1 < ref_len && ref_base(ref, i) == 'C' && ref_base(ref, i + 1) == 'G';
}

// Byte i of string `which` of a site whose substring is sub[0 .. L) = segment[sub_start .. sub_start + L): 0 the substring, 1 its
// reverse complement, 2 the methylated substring, 3 the methylated reverse complement.  methylate (meth.c:359-382): a C whose
// successor inside the substring is G becomes M.  reverse_complement_meth (meth.c:387-420) at position j writes out[L - 1 - j]:
// G for an M, M for a G preceded by M, otherwise the complement.  The n <= 2 branch of match_to_site (meth.c:326-354) is
// unreachable: a substring holds its first CpG with ten bases before it, so L >= 12.
GBX_AMR_HD inline char site_byte(const char *ref, int64_t sub_start, int64_t L, int which, int64_t i)
{
    const int64_t j = (which & 1) ? L - 1 - i : i;                                       // the substring position this byte comes from
    const char c = ref_base(ref, sub_start + j);
    if (which == 0) return c;
    if (which == 1) return complement(c);
    const bool m_here = c == 'C' && j + 1 < L && ref_base(ref, sub_start + j + 1) == 'G';
    if (which == 2) return m_here ? 'M' : c;
    if (m_here) return 'G';
    if (c == 'G' && j > 0 && ref_base(ref, sub_start + j - 1) == 'C') return 'M';        // the G of an M G pair
    return complement(c);
}

// ---- per group
struct Group { int32_t first, last, n_cpg; };                // the positions of its first and last CpG in the segment
struct Kept {                                                // what a kept group hands to the fill
    int32_t sub_start, L, e1, e2;
};
enum { GROUP_SKIP = 0, GROUP_KEEP = 1, GROUP_AGAINST_STRAND = 2 };

// a new group starts at a CpG that has no CpG before it, or whose predecessor is more than MIN_SEPARATION back (meth.c:540-548)
GBX_AMR_HD inline bool group_starts(bool has_prev, int32_t prev, int32_t pos) { return !has_prev || pos - prev > MIN_SEPARATION; }

GBX_AMR_HD inline int pair_lower_bound(const gbx_abea_pair *a, int n, int v)              // meth.c:422-431
{
    int lo = 0, hi = n;
    for (int step = 0; step < SEARCH_STEPS && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid].ref_pos < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// meth.c:433-467, as written: start_i == size || stop_i == size rejects; right_bounded has its stop_i + 1 < size guard and
// compares against ref_start (meth.c:448-450)
GBX_AMR_HD inline bool find_by_ref_bounds(const gbx_abea_pair *pairs, int size, int ref_start, int ref_stop, int *read_start, int *read_stop)
{
    const int start_i = pair_lower_bound(pairs, size, ref_start), stop_i = pair_lower_bound(pairs, size, ref_stop);
    if (start_i == size || stop_i == size) return false;
    const bool left_bounded = pairs[start_i].ref_pos <= ref_start || (start_i != 0 && pairs[start_i - 1].ref_pos <= ref_start);
    const bool right_bounded = pairs[stop_i].ref_pos >= ref_stop || (stop_i + 1 < size && pairs[stop_i + 1].ref_pos >= ref_start);
    if (!(left_bounded && right_bounded)) return false;
    *read_start = pairs[start_i].read_pos;
    *read_stop = pairs[stop_i].read_pos;
    return true;
}

// The skips of meth.c:565-615 for one group of a read with ref_len >= 2 and n_rec >= 1.  The ratio filter (meth.c:607-612)
// divides by calling_start - calling_end, a negative number: it never rejects, and is not evaluated.
GBX_AMR_HD inline int group_decide(const Group &g, int64_t ref_len, int32_t ref_start_pos, bool rc, const gbx_abea_pair *rec, int n_rec, Kept *k)
{
    const int sub_start_pos = g.first - MIN_SEPARATION, sub_end_pos = g.last + MIN_SEPARATION;
    const int span = g.last - g.first;
    if (sub_start_pos <= MIN_SEPARATION || span > MAX_SPAN) return GROUP_SKIP;
    int64_t L = (int64_t)sub_end_pos - sub_start_pos + 1;                                 // substr clamps at the end of the segment
    if (L > ref_len - sub_start_pos) L = ref_len - sub_start_pos;
    const int calling_start = sub_start_pos + ref_start_pos, calling_end = sub_end_pos + ref_start_pos;
    int e1 = 0, e2 = 0;
    if (!find_by_ref_bounds(rec, n_rec, calling_start, calling_end, &e1, &e2)) return GROUP_SKIP;
    const int64_t d = (int64_t)e2 - e1;
    if ((d < 0 ? -d : d) <= 10) return GROUP_SKIP;
    if ((e1 <= e2) == rc) return GROUP_AGAINST_STRAND;
    k->sub_start = sub_start_pos; k->L = (int32_t)L; k->e1 = e1; k->e2 = e2;
    return GROUP_KEEP;
}

GBX_AMR_HD inline gbx_abea_meth_site site_of(int32_t read, const Group &g, int64_t ref_len, int32_t ref_start_pos)
{
    gbx_abea_meth_site S;
    S.read = read;
    S.start_position = g.first + ref_start_pos;
    S.end_position = g.last + ref_start_pos;
    S.n_cpg = g.n_cpg;
    const int64_t o0 = (int64_t)g.first - GBX_ABEA_KMER + 1, o1 = (int64_t)g.last + GBX_ABEA_KMER;
    S.ctx_off = o0;
    S.ctx_len = (int32_t)((o1 < ref_len ? o1 : ref_len) - o0);
    S.pad_ = 0;
    return S;
}

// job m (0 unmethylated, 1 methylated) of a site whose four strings start at byte `base` of the arena
GBX_AMR_HD inline gbx_abea_meth_job job_of(int32_t read, const Kept &k, bool rc, int64_t base, int m)
{
    gbx_abea_meth_job J;
    J.seq_off = base + 2 * (int64_t)m * k.L; J.rc_off = J.seq_off + k.L; J.seq_len = k.L; J.read = read;
    J.event_start = k.e1; J.event_stop = k.e2; J.rc = rc ? 1 : 0; J.flags = GBX_ABEA_METH_PRE_CLIP | GBX_ABEA_METH_POST_CLIP;
    return J;
}

// ---- per job: the checks of the score plan, in the order gbx_abea_meth_plan_host makes them
enum { JOB_OK = 0, JOB_STRINGS, JOB_TOO_LONG, JOB_READ, JOB_EVENTS, JOB_ROWS };

GBX_AMR_HD inline int job_class(int64_t n_kmers) { return n_kmers <= 16 ? 0 : n_kmers <= 64 ? 1 : n_kmers <= 128 ? 2 : 3; }

GBX_AMR_HD inline int64_t job_rows(const gbx_abea_meth_job &J)
{
    return J.event_stop > J.event_start ? (int64_t)J.event_stop - J.event_start + 1 : (int64_t)J.event_start - J.event_stop + 1;
}

// event_off: n_reads + 1 entries, read only once J.read is known to lie inside them
GBX_AMR_HD inline int job_check(const gbx_abea_meth_job &J, int64_t seq_bytes, int64_t n_reads, const int64_t *event_off, int64_t flank_len)
{
    const int64_t nk = (int64_t)J.seq_len - GBX_ABEA_KMER + 1;
    if (nk < 1 || J.seq_off < 0 || J.rc_off < 0 || J.seq_off + J.seq_len > seq_bytes || J.rc_off + J.seq_len > seq_bytes) return JOB_STRINGS;
    if (nk > GBX_ABEA_METH_MAX_KMERS) return JOB_TOO_LONG;
    if (J.read < 0 || J.read >= n_reads) return JOB_READ;
    const int64_t ne = event_off[J.read + 1] - event_off[J.read];
    if (J.event_start < 0 || J.event_stop < 0 || J.event_start >= ne || J.event_stop >= ne ||
        (J.rc ? J.event_stop > J.event_start : J.event_stop < J.event_start))
        return JOB_EVENTS;
    if (job_rows(J) + 1 > flank_len) return JOB_ROWS;
    return JOB_OK;
}

}  // namespace abea_meth_rules
}  // namespace gbx
