// abea_freq_rules.h — the rules of f5c meth-freq (freq.c) as functions the device kernels (abea_freq_kernels.hip), the host
// entries (capi_abea_freq.hip) and a host program (tests/sanitize_freq) compile from the same text: the call decision, the
// two-decimal log-likelihood ratio that call-methylation's "%.2lf" and meth-freq's strtod make of a double, the CG step of the
// split, the key order, and the digits and lengths of the output line ("%d", "%.3lf").  Integer work only behind the one
// division each rule names; nothing here allocates or reads outside the bytes it is handed.
#pragma once
#include <stdint.h>
#include <string.h>
#include "abea_meth_rules.h"

#if defined(__HIPCC__)
#define GBX_AFR_HD __host__ __device__
#else
#define GBX_AFR_HD
#endif

namespace gbx {
namespace abea_freq_rules {

constexpr int SPLIT_LEN = 11;                                // strlen("split-group")
constexpr int FREQ_LEN = 5;                                  // "%.3lf" of a value in [0, 1]: d.ddd
constexpr double LLR_EXACT_BELOW = 70368744177664.0;         // 2^46: from here a double's neighbours are further than 0.01 apart

GBX_AFR_HD inline uint64_t bits_of(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
GBX_AFR_HD inline double abs_of(double x) { uint64_t u = bits_of(x) & 0x7fffffffffffffffull; double r; memcpy(&r, &u, 8); return r; }

// ---- the call (freq.c:343-351): dropped iff fabs(llr) < threshold, so a NaN is kept; methylated iff llr > 0
GBX_AFR_HD inline bool called(double llr, double threshold) { return !(abs_of(llr) < threshold); }
GBX_AFR_HD inline bool methylated(double llr) { return llr > 0; }

// round(|x| * scale) for a finite |x| = mant * 2^e with e < 0 and mant * scale < 2^63: the exact binary value, ties to even -
// what glibc's printf prints in round-to-nearest
GBX_AFR_HD inline uint64_t scaled_round(double x, uint64_t scale)
{
    const uint64_t u = bits_of(x) & 0x7fffffffffffffffull;
    const int ex = (int)(u >> 52);
    const uint64_t mant = ex ? (u & 0xfffffffffffffull) | (1ull << 52) : (u & 0xfffffffffffffull);
    const int sh = 1075 - (ex ? ex : 1);                     // |x| = mant / 2^sh
    const uint64_t P = mant * scale;
    if (sh <= 0) return P << -sh;                            // (an integer; the callers stay below 2^63)
    if (sh >= 64) return 0;                                  // P < 2^63 <= half of 2^sh
    const uint64_t q = P >> sh, rem = P & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    return q + ((rem > half || (rem == half && (q & 1))) ? 1 : 0);
}

// strtod of "%.2lf" of x (f5c.c:1643 -> freq.c:222).  Below 2^46 the hundredths q are exact in a double and q / 100.0, one
// correctly rounded division of two exact integers, is the number the text names.  From 2^46 the spacing of doubles is
// 2^-6 or more, so the text, which lies within 0.005 of x, reads back as x; inf and NaN print and read back as themselves.
GBX_AFR_HD inline double llr_as_printed(double x)
{
    if (!(abs_of(x) < LLR_EXACT_BELOW)) return x;
    const double r = (double)scaled_round(x, 100) / 100.0;
    return (bits_of(x) >> 63) ? -r : r;                      // "-0.00" reads back as -0.0
}

// ---- the split (freq.c:353-370): strstr over "CG", case-sensitive; an occurrence starts at i
GBX_AFR_HD inline bool cg_at(const char *seq, int64_t len, int64_t i) { return i >= 0 && i + 1 < len && seq[i] == 'C' && seq[i + 1] == 'G'; }
// one item per record, or one per occurrence
GBX_AFR_HD inline bool splits(int split_groups, int32_t n_cpg) { return split_groups && n_cpg > 1; }
// a byte of a call-methylation site's context as its TSV line carries it (f5c.c:1649 of meth.c:288-306)
GBX_AFR_HD inline char site_byte(char c) { return abea_meth_rules::possible0(abea_meth_rules::upper(c)); }

// ---- the key order (cmp_key, freq.c:96-132) over contig ranks that follow strcmp of the names
GBX_AFR_HD inline int key_cmp(int32_t ca, int32_t sa, int32_t ea, int32_t cb, int32_t sb, int32_t eb)
{
    if (ca != cb) return ca < cb ? -1 : 1;
    if (sa != sb) return sa < sb ? -1 : 1;
    return ea < eb ? -1 : ea > eb ? 1 : 0;
}

// ---- the output line (freq.c:407-408)
GBX_AFR_HD inline int dec_len(int64_t v)                       // strlen of "%d"
{
    int n = v < 0 ? 2 : 1;
    uint64_t m = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    while (m >= 10) { m /= 10; ++n; }
    return n;
}
GBX_AFR_HD inline int dec_put(char *out, int64_t v)            // -> the bytes written, dec_len(v)
{
    const int n = dec_len(v);
    uint64_t m = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    for (int i = n - 1; i >= (v < 0 ? 1 : 0); --i) { out[i] = (char)('0' + m % 10); m /= 10; }
    if (v < 0) out[0] = '-';
    return n;
}
// the thousandths "%.3lf" prints of f = (double)methylated / called, 0 <= methylated <= called, called > 0: 0 .. 1000.  The
// division is the reference's own; the rounding is of the double's exact binary value, not of the rational.
GBX_AFR_HD inline int freq_milli(int64_t methylated, int64_t called_sites)
{
    const double f = (double)methylated / (double)called_sites;
    return (int)scaled_round(f, 1000);
}
GBX_AFR_HD inline void freq_put(char *out, int milli)          // FREQ_LEN bytes
{
    out[0] = (char)('0' + milli / 1000); out[1] = '.';
    out[2] = (char)('0' + milli / 100 % 10); out[3] = (char)('0' + milli / 10 % 10); out[4] = (char)('0' + milli % 10);
}
// the bytes of a site's line without the contig name: six tabs behind it, five numbers, the frequency, the sequence, '\n'
GBX_AFR_HD inline int64_t line_tail_len(int32_t start, int32_t end, int32_t group_size, int32_t called_sites, int32_t meth, int32_t seq_len)
{
    return 7 + dec_len(start) + dec_len(end) + dec_len(group_size) + dec_len(called_sites) + dec_len(meth) + FREQ_LEN +
           (seq_len < 0 ? SPLIT_LEN : seq_len) + 1;
}

}  // namespace abea_freq_rules
}  // namespace gbx
