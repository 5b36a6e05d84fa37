// mm_paf_rules.h — from "region g of this PAF input" to its line: the names and lengths the region's read and
// target give, and whether it prints its alignment (mm_paf_cigar_line) or the plain line (mm_paf_line).  One text for the PAF
// kernels (mm_paf.hip) and for the host build (shims/mm_map_cpu_twin.cpp, shims/mm_align_cpu_twin.cpp).
#pragma once
#include "mm_align_rules.h"

namespace gbx {

struct MmPafView {
    int64_t n_reads; const gbx_mm_reg *regs;
    const gbx_mm_aln *alns; const uint32_t *cigar; int64_t cigar_cap;       // alns null: every region prints the plain line
    const uint8_t *qnames; const int64_t *qname_off, *seq_off; const int32_t *rep_len;
    int64_t n_targets; const uint8_t *tnames; const int64_t *tname_off, *tseq_off;
};

// the line of region g at out[at ..), written below cap only (out may be null: the length alone) -> its length; a region that
// names no read of the input has no line
GBX_MM_HD inline int64_t mm_paf_region_line(const MmPafView &V, int64_t g, uint8_t *out, int64_t at, int64_t cap)
{
    const gbx_mm_reg reg = V.regs[g];
    const int64_t r = reg.read;
    if (r < 0 || r >= V.n_reads) return 0;
    const int64_t q0 = V.qname_off[r], q1 = V.qname_off[r + 1];
    const bool tok = reg.rid >= 0 && reg.rid < V.n_targets;
    const int64_t t0 = tok ? V.tname_off[reg.rid] : 0, t1 = tok ? V.tname_off[reg.rid + 1] : 0;
    const uint8_t *qn = V.qnames + q0, *tn = tok ? V.tnames + t0 : nullptr;
    const int64_t qnl = q1 > q0 ? q1 - q0 : 0, tnl = t1 > t0 ? t1 - t0 : 0;
    const int32_t tlen = tok ? (int32_t)(V.tseq_off[reg.rid + 1] - V.tseq_off[reg.rid]) : 0, qlen = (int32_t)(V.seq_off[r + 1] - V.seq_off[r]);
    if (V.alns) {
        const gbx_mm_aln a = V.alns[g];
        if ((a.flags & GBX_MM_ALN_ALIGNED) && !(a.flags & (GBX_MM_ALN_NO_ROOM | GBX_MM_ALN_INVALID)) && a.n_cigar >= 0 && a.cigar_off >= 0 &&
            a.cigar_off + a.n_cigar <= V.cigar_cap)
            return mm_paf_cigar_line(out, at, cap, reg, a, V.cigar, qn, qnl, qlen, tn, tnl, tlen, V.rep_len[r]);
    }
    return mm_paf_line(out, at, cap, reg, qn, qnl, qlen, tn, tnl, tlen, V.rep_len[r]);
}

// the host build: the text of every read's regions in order -> its length; bytes below text_cap are written, line_off[n_reads + 1] always
inline int64_t mm_paf_text(const MmPafView &V, const int64_t *reg_off, uint8_t *lines, int64_t text_cap, int64_t *line_off)
{
    int64_t at = 0;
    for (int64_t r = 0; r < V.n_reads; ++r) {
        line_off[r] = at;
        for (int64_t g = reg_off[r]; g < reg_off[r + 1]; ++g) at += mm_paf_region_line(V, g, lines, at, text_cap);
    }
    line_off[V.n_reads] = at;
    return at;
}

}  // namespace gbx
