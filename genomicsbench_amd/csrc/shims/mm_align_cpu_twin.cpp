// mm_align_cpu_twin.cpp — the device's alignment rules (mm_align_rules.h) compiled for the host into libgbx_mm_cpu.so: a team of
// one lane.  The CPU tests hold it against the plain-Python restatement tests/mm_align_ref.py, so the text the kernels run is
// tested where there is no GPU.
#include <vector>
#include "../mm_paf_rules.h"

extern "C" {

// The regions of a batch as gbx_mm_align_device aligns them: alns[n_regs], cigar below cigar_cap, counts[3] = jobs, words, bytes of
// z needed; a region whose jobs end past z_bytes (in region order) gets flag 32.
int gbx_mm_align_cpu(const gbx_mm_align_params *P, int64_t n_reads, int64_t n_regs, const gbx_mm_reg *regs, const int64_t *off, const uint64_t *cax,
                     const uint64_t *cay, const int32_t *n_chained, const uint8_t *seq, const int64_t *seq_off, int64_t n_targets, const uint8_t *tseq,
                     const int64_t *tseq_off, gbx_mm_aln *alns, uint32_t *cigar, int64_t cigar_cap, int64_t z_bytes, int64_t *counts)
{
    const gbx::MmAlnSolo t;
    const gbx::MmAlnIn in{n_reads, off, cax, cay, n_chained, -1, seq, seq_off, n_targets, tseq, tseq_off};
    int64_t n_jobs = 0, n_words = 0, z_need = 0;
    for (int64_t g = 0; g < n_regs; ++g) {
        const gbx_mm_reg &reg = regs[g];
        gbx::MmAlnSeq S;
        const uint64_t *x, *y;
        int32_t nc;
        if (!gbx::mm_aln_region_view(in, reg, &S, &x, &y, &nc) ||
            !gbx::mm_aln_valid(reg, n_targets, nc, x, y, S.tlen, S.qlen)) {
            gbx::mm_aln_copy(reg, GBX_MM_ALN_INVALID, &alns[g]);
            continue;
        }
        gbx::MmAlnPlanCount c;
        gbx::mm_aln_plan(*P, reg.cnt, x, y, S.tlen, S.qlen, c);
        n_jobs += c.n;
        z_need += c.bytes;
        if (z_need > z_bytes) { gbx::mm_aln_copy(reg, GBX_MM_ALN_NO_ROOM, &alns[g]); continue; }
        std::vector<gbx::MmAlnJob> jobs((size_t)c.n);
        std::vector<uint8_t> z((size_t)c.bytes + 16);
        gbx::MmAlnPlanWrite wr{jobs.data(), 0, c.n, 0, (int32_t)g, 0};
        gbx::mm_aln_plan(*P, reg.cnt, x, y, S.tlen, S.qlen, wr);
        for (auto &j : jobs) gbx::mm_aln_job_run(t, *P, S, z.data() + j.z_at, nullptr, 0, &j);
        const int32_t nw = gbx::mm_aln_place(jobs.data(), (int32_t)c.n);
        gbx::mm_aln_pack(t, *P, reg, S, jobs.data(), (int32_t)c.n, nw, z.data(), cigar, n_words, cigar_cap, &alns[g]);
        n_words += nw;
    }
    counts[0] = n_jobs; counts[1] = n_words; counts[2] = z_need;
    return 0;
}

// One DP job on plain sequences: mode 0 LEFT / 1 RIGHT, ext 0 global / 1 extension.  -> out[6] = score, end_t, end_q, flags
// (1 z-dropped, 2 reached the query end), consumed target, consumed query; the runs in the job's own direction into
// cigar[cigar_cap] -> their count.
int64_t gbx_mm_align_cpu_job(const gbx_mm_align_params *P, const uint8_t *T, int32_t tl, const uint8_t *Q, int32_t ql, int32_t w, int mode, int ext,
                             int32_t *out, uint32_t *cigar, int64_t cigar_cap)
{
    const gbx::MmAlnSolo t;
    gbx::MmAlnJob J{};
    J.kind = ext ? gbx::MMA_KIND_RIGHT : gbx::MMA_KIND_FILL;
    J.tl = tl; J.ql = ql; J.w = gbx::mma_band(w, tl, ql);
    std::vector<uint8_t> z((size_t)gbx::mma_job_bytes(J.w, tl, ql) + 16);
    const gbx::MmAlnSeq S{T, Q, tl, ql, 0};
    const gbx::MmAlnView V{S, 0, 0, tl, ql, 0};
    gbx::mm_aln_dp(t, *P, V, mode, ext != 0, z.data(), (int32_t *)z.data(), &J);
    gbx::mm_aln_job_runs(&J, z.data(), ext != 0);
    out[0] = J.score; out[1] = J.end_t; out[2] = J.end_q; out[3] = J.flags; out[4] = J.ct; out[5] = J.cq;
    J.w_at = 0; J.merge = 0;
    gbx::MmAlnPutRuns put{cigar, 0, cigar_cap, J.n_ops, 0, 0, 0};
    if (J.end_t >= 0) gbx::mm_aln_walk(J, z.data(), put);
    return J.n_ops;
}

// The PAF-with-CIGAR text of the regions -> its length; bytes below text_cap are written, line_off[n_reads + 1] always.
int64_t gbx_mm_paf_cigar_cpu(int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns, const uint32_t *cigar, int64_t n_cigar,
                             const uint8_t *qnames, const int64_t *qname_off, const int64_t *seq_off, const int32_t *rep_len, int64_t n_targets,
                             const uint8_t *tnames, const int64_t *tname_off, const int64_t *tseq_off, uint8_t *lines, int64_t text_cap, int64_t *line_off)
{
    const gbx::MmPafView V{n_reads, regs, alns, cigar, n_cigar, qnames, qname_off, seq_off, rep_len, n_targets, tnames, tname_off, tseq_off};
    return gbx::mm_paf_text(V, reg_off, lines, text_cap, line_off);
}

}  // extern "C"
