// mm_map_cpu_twin.cpp — the device's rules behind the chain scores (mm_map_rules.h) and of a PAF line (mm_paf_rules.h) compiled
// for the host into libgbx_mm_cpu.so: a team of one lane.  The CPU tests hold it against the plain-Python restatement
// tests/mm_map_ref.py, so the text the kernels run is tested where there is no GPU.
#include <vector>
#include "../mm_paf_rules.h"

extern "C" {

// Chains and regions of a batch; u, regs: room for one per anchor (always enough), cax / cay / chain and region lists laid out as
// gbx_mm_map_device lays them out.  counts[2] = chains, regions.
int gbx_mm_map_cpu(const gbx_mm_map_params *P, int64_t n_reads, const int64_t *off, const uint64_t *ax, const uint64_t *ay, const int32_t *f,
                   const int32_t *p, const int32_t *v, const int64_t *seq_off, const int32_t *rep_len, const uint32_t *hash, int64_t *chain_off,
                   uint64_t *u, uint64_t *cax, uint64_t *cay, int32_t *n_chained, int64_t *reg_off, gbx_mm_reg *regs, int64_t *counts)
{
    const gbx::MmSolo t;
    chain_off[0] = reg_off[0] = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t o = off[r];
        const int32_t n = (int32_t)(off[r + 1] - o);
        const size_t m = (size_t)n + 1;
        std::vector<int32_t> own(m), top(m), perm(m), w(m);
        std::vector<uint64_t> key(m), urank(m), uo(m);
        std::vector<gbx::MmZ> z(m);
        std::vector<gbx_mm_reg> stage(m);
        int32_t nk = 0, nch = 0, nreg = 0;
        const gbx::MmMapRead rd{n, ax + o, ay + o, f + o, p + o, v + o, (int32_t)(seq_off[r + 1] - seq_off[r]), rep_len[r], hash[r]};
        const gbx::MmChainWork cw{own.data(), top.data(), perm.data(), key.data(), urank.data(), &nk};
        gbx::mm_map_chains(t, rd, *P, cw, uo.data(), cax + o, cay + o, &nch, n_chained + r);
        gbx::mm_map_regs(t, rd, (int32_t)r, *P, nch, uo.data(), cax + o, cay + o, z.data(), w.data(), stage.data(), &nreg);
        for (int32_t i = 0; i < nch; ++i) u[chain_off[r] + i] = uo[(size_t)i];
        for (int32_t i = 0; i < nreg; ++i) regs[reg_off[r] + i] = stage[(size_t)i];
        chain_off[r + 1] = chain_off[r] + nch;
        reg_off[r + 1] = reg_off[r] + nreg;
    }
    counts[0] = chain_off[n_reads];
    counts[1] = reg_off[n_reads];
    return 0;
}

// The PAF text of the regions -> its length; bytes below text_cap are written, line_off[n_reads + 1] always.
int64_t gbx_mm_paf_cpu(int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const uint8_t *qnames, const int64_t *qname_off,
                       const int64_t *seq_off, const int32_t *rep_len, int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off,
                       const int64_t *tseq_off, uint8_t *lines, int64_t text_cap, int64_t *line_off)
{
    const gbx::MmPafView V{n_reads, regs, nullptr, nullptr, 0, qnames, qname_off, seq_off, rep_len, n_targets, tnames, tname_off, tseq_off};
    return gbx::mm_paf_text(V, reg_off, lines, text_cap, line_off);
}

uint32_t gbx_mm_map_cpu_read_hash(const uint8_t *name, int64_t len, int32_t qlen) { return gbx::mm_map_read_hash(name, len, qlen); }

}  // extern "C"
