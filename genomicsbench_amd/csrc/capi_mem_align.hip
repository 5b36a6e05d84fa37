// capi_mem_align.hip — the aligner of the C-ABI (include/gbx.h): gbx_mem_index, gbx_mem_align_plan and gbx_mem_aligner, which
// queues the stage entries smem .. sam on one stream, reads every count with one copy (mem_align_kernels.hip) and runs the chain
// again from the first stage whose capacity was too small.  The stages are called through their device entries, so every
// argument passes the checks those make.
#include "capi_common.h"

using namespace gbx;

struct gbx_mem_index {
    gbx_fmi_index idx;                   // scalars; cp_occ is not kept (the device layout is d_index)
    gbx_fmi_sa sa;                       // scalars; the arrays are not kept (d_sa)
    int dev;
    void *d_index, *d_sa;
    uint8_t *d_text;                     // 2 l_pac bytes and 64 of slack
    int64_t text_bytes, l_pac;
    int32_t n_contigs, max_cname;
    int64_t *d_contig_off;
    uint8_t *d_cnames;
    int64_t *d_cname_off;
    int64_t cname_bytes;
    std::vector<int64_t> contig_off, cname_off;
    std::vector<uint8_t> cnames;
};

namespace {

constexpr int N_CAPS = 16;
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static_assert(sizeof(gbx_mem_align_params) == 600 && sizeof(gbx_mem_align_caps) == 8 * N_CAPS && sizeof(gbx_mem_align_counts) == 144,
              "records");

// first guesses of the capacities that have no bound, per base (1 M reads of 151 bases give 0.057 SMEMs and 0.24 hits
// per base, profiles/fmi_sal_time.json): SMEMs 0.1, hits 0.4, chains 0.05, CIGAR words 0.1
constexpr double GUESS_SMEM = 0.10, GUESS_POS = 0.40, GUESS_CHAIN = 0.05, GUESS_CIGAR = 0.10;
// the text bound's assumptions: contig names of 32 bytes, 4 records a read, deletions of 256 bases; beyond them the stage
// reports its need and the aligner runs it again
constexpr int32_t TEXT_CNAME = 32, TEXT_RECS = 4, TEXT_DEL = 256;
constexpr double GUESS_Z_RECS = 1.5;     // CIGAR records per read whose direction room is kept
constexpr double MARGIN = 1.25;          // over the last batch's counts scaled by the bases

int64_t scaled(int64_t count, int64_t bases, int64_t last_bases)
{
    if (count <= 0) return 0;
    const long double r = last_bases > 0 ? (long double)bases / (long double)last_bases : 1.0L;
    return (int64_t)std::ceil((long double)count * r * (long double)MARGIN) + 64;
}

int64_t extra_of(const gbx_mem_align_params *p, int64_t n_reads, int64_t reg_cap)
{
    return 4 * std::min<int64_t>(reg_cap, n_reads * (int64_t)std::max(p->rescue.max_matesw, 1));
}

bool rescue_runs(const gbx_mem_align_params *p) { return p->mode == 1 && !p->no_rescue; }

// what follows from the capacities before it and costs nothing: called after any of out_cap .. z_bytes changed; never lowers one
void derive(const gbx_mem_align_params *p, int64_t n_reads, int64_t bases, int64_t name_bytes, gbx_mem_align_caps *c, bool all)
{
    if (all) {
        c->seed_cap = std::max(c->seed_cap, c->pos_cap);
        c->reg_cap = std::max(c->reg_cap, c->seed_cap);
        c->sel_cap = std::max(c->sel_cap, c->seed_cap);
    }
    if (rescue_runs(p)) {
        const int64_t extra = extra_of(p, n_reads, c->reg_cap);
        if (all) {
            c->xreg_cap = std::max(c->xreg_cap, c->reg_cap + extra);
            c->xsel_cap = std::max(c->xsel_cap, c->reg_cap + extra);
            c->xseed_cap = std::max(c->xseed_cap, c->seed_cap + extra);
        }
        c->xseed_cap = std::max(c->xseed_cap, c->seed_cap);      // the copy of the seeds is always there
        if (all) c->psel_cap = std::max(c->psel_cap, c->xreg_cap);
    } else {
        c->xreg_cap = c->xseed_cap = c->xsel_cap = 0;
        if (p->mode == 1) { if (all) c->psel_cap = std::max(c->psel_cap, c->reg_cap); }
        else c->psel_cap = 0;
    }
    if (all) {
        const int64_t list = p->mode == 1 ? c->psel_cap : c->sel_cap, rc = rescue_runs(p) ? c->xreg_cap : c->reg_cap;
        c->rec_cap = std::max(c->rec_cap, n_reads + std::min(rc, list));
        const int64_t t = (int64_t)gbx_mem_sam_text_cap(c->rec_cap, c->cigar_cap, bases, name_bytes, TEXT_CNAME, TEXT_RECS, TEXT_DEL);
        c->text_cap = std::max(c->text_cap, t);
        c->md_cap = std::max(c->md_cap, t);
    }
}

// after an overflow grew a capacity: the ones behind it that stood in an always-suffices relation to it before keep that relation
void follow(const gbx_mem_align_params *p, int64_t n_reads, int64_t bases, int64_t name_bytes, const gbx_mem_align_caps &was,
            gbx_mem_align_caps *c)
{
    const bool rescue = rescue_runs(p), paired = p->mode == 1;
    if (was.seed_cap >= was.pos_cap) c->seed_cap = std::max(c->seed_cap, c->pos_cap);
    if (was.reg_cap >= was.seed_cap) c->reg_cap = std::max(c->reg_cap, c->seed_cap);
    if (was.sel_cap >= was.seed_cap) c->sel_cap = std::max(c->sel_cap, c->seed_cap);
    if (rescue) {
        const int64_t e0 = extra_of(p, n_reads, was.reg_cap), e1 = extra_of(p, n_reads, c->reg_cap);
        if (was.xreg_cap >= was.reg_cap + e0) c->xreg_cap = std::max(c->xreg_cap, c->reg_cap + e1);
        if (was.xsel_cap >= was.reg_cap + e0) c->xsel_cap = std::max(c->xsel_cap, c->reg_cap + e1);
        if (was.xseed_cap >= was.seed_cap + e0) c->xseed_cap = std::max(c->xseed_cap, c->seed_cap + e1);
        c->xseed_cap = std::max(c->xseed_cap, c->seed_cap);
    }
    const int64_t r0 = rescue ? was.xreg_cap : was.reg_cap, r1 = rescue ? c->xreg_cap : c->reg_cap;
    if (paired && was.psel_cap >= r0) c->psel_cap = std::max(c->psel_cap, r1);
    const int64_t l0 = paired ? was.psel_cap : was.sel_cap, l1 = paired ? c->psel_cap : c->sel_cap;
    if (was.rec_cap >= n_reads + std::min(r0, l0)) c->rec_cap = std::max(c->rec_cap, n_reads + std::min(r1, l1));
    if (was.text_cap >= (int64_t)gbx_mem_sam_text_cap(was.rec_cap, was.cigar_cap, bases, name_bytes, TEXT_CNAME, TEXT_RECS, TEXT_DEL)) {
        const int64_t t = (int64_t)gbx_mem_sam_text_cap(c->rec_cap, c->cigar_cap, bases, name_bytes, TEXT_CNAME, TEXT_RECS, TEXT_DEL);
        c->text_cap = std::max(c->text_cap, t);
        if (was.md_cap >= was.text_cap) c->md_cap = std::max(c->md_cap, t);
    }
}

int pes_given_check(const gbx_mem_pestat *pes, const char *who)
{
    for (int d = 0; d < 4; ++d)
        if (pes[d].failed == 0 && !(pes[d].std > 0.)) {
            set_error("%s: pes: direction %d has not failed and its std is not above 0", who, d);
            return GBX_ERR_ARG;
        }
    return GBX_OK;
}

// a device allocation that grows and never shrinks; growing loses the content
struct Grow {
    void *p = nullptr;
    size_t cap = 0;
    int need(size_t bytes, hipStream_t s)
    {
        if (bytes <= cap && p) return GBX_OK;
        if (p) { GBX_HIP(hipStreamSynchronize(s)); (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = std::max<size_t>(bytes + bytes / 8, 256);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; set_error("gbx_mem_aligner: no device memory for %zu bytes", want); (void)hipGetLastError(); return GBX_ERR_NOMEM; }
        cap = want;
        GBX_HIP(hipMemsetAsync(p, 0, want, s));
        return GBX_OK;
    }
    void drop() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

struct Pinned {
    void *p = nullptr;
    size_t cap = 0;
    int need(size_t bytes)
    {
        if (bytes <= cap && p) return GBX_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = std::max<size_t>(bytes + bytes / 8, 4096);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; set_error("gbx_mem_aligner: no pinned host memory for %zu bytes", want); (void)hipGetLastError(); return GBX_ERR_NOMEM; }
        cap = want;
        return GBX_OK;
    }
    void drop() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

int default_slot(const gbx_mem_align_params *p, int32_t max_len)
{
    const int msl = p->fmi.min_seed_len > 1 ? p->fmi.min_seed_len : 1;
    const int c = (4 * max_len + msl - 1) / msl + 16;
    return c > 48 ? c : 48;
}

}  // namespace

struct gbx_mem_aligner {
    const gbx_mem_index *ix;
    gbx_mem_align_params p;
    gbx_mem_align_caps caps;             // in force
    bool have_first, have_last;
    gbx_mem_align_caps first;
    gbx_mem_align_counts last;
    int64_t last_bases;
    gbx_mem_align_stats stats;
    hipStream_t s;
    // device: the batch (one arena), per-stage outputs and workspaces, the counts
    Grow in, smems, smem_off, pos, pos_off, chains, chain_off, seeds, l_rep, res, regs, reg_off, sel_seeds, sel_res, xregs, xreg_off,
         xseeds, xsel_seeds, xsel_res, xstats, pairs, pregs, psel_seeds, psel_res, alns, cigar, recs, rec_off, md, lines, words;
    Grow w_fmi, w_sal, w_chain, w_ext, w_regs, w_pes, w_resc, w_pair, w_cigar, w_sam;
    Pinned h_in, h_out, h_counts;
    // offsets of the batch in `in`
    size_t o_off, o_len, o_qual, o_names, o_noff, in_bytes;
};

namespace {

// the words on the device: 32 int64 (counts of every stage), then the pestat records, then the gathered record
enum { W_SMEM = 0, W_POS = 1, W_CHAINS = 2, W_SEEDS = 3, W_REGS = 4, W_SEL = 5, W_XREGS = 6, W_XSEL = 7, W_XSEEDS = 8, W_PSEL = 9,
       W_CIGAR = 10, W_RECS = 11, W_MD = 12, W_TEXT = 13, W_N = 32 };
constexpr size_t WORDS_PES_GIVEN = W_N * 8, WORDS_PES_EST = WORDS_PES_GIVEN + 128, WORDS_PES_OUT = WORDS_PES_EST + 128,
                 WORDS_COUNTS = WORDS_PES_OUT + 128, WORDS_BYTES = WORDS_COUNTS + 256;

int64_t *word(gbx_mem_aligner *al, int k) { return al->words.as<int64_t>() + k; }
gbx_mem_pestat *pes_at(gbx_mem_aligner *al, size_t off) { return (gbx_mem_pestat *)((char *)al->words.p + off); }

// queues the chain from stage `from` on with the capacities in force
int queue_chain(gbx_mem_aligner *al, int from, int64_t n_reads, int64_t id0, int64_t enc_bytes, int32_t max_len, int64_t name_bytes,
                bool have_qual)
{
    const gbx_mem_index *ix = al->ix;
    const gbx_mem_align_params &P = al->p;
    const gbx_mem_align_caps &c = al->caps;
    hipStream_t s = al->s;
    int rc;
    const uint8_t *d_enc = al->in.as<uint8_t>();
    const int64_t *d_read_off = (const int64_t *)((char *)al->in.p + al->o_off);
    const int32_t *d_read_len = (const int32_t *)((char *)al->in.p + al->o_len);
    const uint8_t *d_qual = have_qual ? (const uint8_t *)al->in.p + al->o_qual : nullptr;
    const uint8_t *d_names = (const uint8_t *)al->in.p + al->o_names;
    const int64_t *d_name_off = (const int64_t *)((char *)al->in.p + al->o_noff);
    const bool paired = P.mode == 1, rescue = rescue_runs(&P);
    const int64_t n_pairs = n_reads / 2, read_id0 = paired ? 2 * id0 : id0;

    if (from <= GBX_MEM_ST_SMEM) {
        const size_t wb = fmi_workspace_bytes(n_reads, max_len, P.fmi.min_seed_len, (int)c.slot);
        if ((rc = al->smems.need((size_t)c.out_cap * sizeof(gbx_fmi_smem), s)) || (rc = al->smem_off.need((size_t)(n_reads + 1) * 8, s)) ||
            (rc = al->w_fmi.need(wb, s)))
            return rc;
        if ((rc = fmi_launch(&ix->idx, ix->d_index, &P.fmi, n_reads, max_len, d_enc, d_read_off, d_read_len, al->smems.as<gbx_fmi_smem>(),
                             c.out_cap, al->smem_off.as<int64_t>(), word(al, W_SMEM), al->w_fmi.p, wb, s, (int)c.slot)))
            return rc;
    }
    if (from <= GBX_MEM_ST_SAL) {
        const size_t wb = gbx_fmi_sal_workspace_bytes(c.out_cap, c.pos_cap);
        if ((rc = al->pos.need((size_t)c.pos_cap * 8, s)) || (rc = al->pos_off.need((size_t)(c.out_cap + 1) * 8, s)) || (rc = al->w_sal.need(wb, s)))
            return rc;
        if ((rc = gbx_fmi_sal_device(&ix->idx, ix->d_index, &ix->sa, ix->d_sa, al->smems.as<gbx_fmi_smem>(), word(al, W_SMEM), c.out_cap,
                                     P.max_occ, al->pos.as<int64_t>(), c.pos_cap, al->pos_off.as<int64_t>(), word(al, W_POS), al->w_sal.p, wb, s)))
            return rc;
    }
    if (from <= GBX_MEM_ST_CHAIN) {
        const size_t wb = gbx_mem_chain_workspace_bytes(n_reads, c.out_cap, c.pos_cap);
        if ((rc = al->chains.need((size_t)c.chain_cap * sizeof(gbx_mem_chain), s)) || (rc = al->chain_off.need((size_t)(n_reads + 1) * 8, s)) ||
            (rc = al->seeds.need((size_t)c.seed_cap * sizeof(gbx_bsw_seed), s)) || (rc = al->l_rep.need((size_t)n_reads * 4, s)) ||
            (rc = al->w_chain.need(wb, s)))
            return rc;
        if ((rc = gbx_mem_chain_device(&P.chain, n_reads, al->smems.as<gbx_fmi_smem>(), word(al, W_SMEM), c.out_cap, al->smem_off.as<int64_t>(),
                                       al->pos.as<int64_t>(), word(al, W_POS), c.pos_cap, al->pos_off.as<int64_t>(), d_read_off, d_read_len,
                                       ix->l_pac, ix->n_contigs, ix->d_contig_off, al->chains.as<gbx_mem_chain>(), c.chain_cap,
                                       al->chain_off.as<int64_t>(), al->seeds.as<gbx_bsw_seed>(), c.seed_cap, al->l_rep.as<int32_t>(),
                                       word(al, W_CHAINS), word(al, W_SEEDS), al->w_chain.p, wb, s)))
            return rc;
    }
    if (from <= GBX_MEM_ST_EXTEND) {
        const size_t wb = gbx_bsw_seeds_workspace_bytes(c.seed_cap, ix->text_bytes, enc_bytes);
        if ((rc = al->res.need((size_t)c.seed_cap * sizeof(gbx_bsw_seed_result), s)) || (rc = al->w_ext.need(wb, s))) return rc;
        if ((rc = gbx_bsw_extend_seeds_device(&P.bsw, c.seed_cap, ix->d_text, ix->text_bytes, d_enc, enc_bytes, al->seeds.as<gbx_bsw_seed>(),
                                              al->res.as<gbx_bsw_seed_result>(), al->w_ext.p, wb, s)))
            return rc;
    }
    if (from <= GBX_MEM_ST_REGS) {
        const size_t wb = gbx_mem_regs_workspace_bytes(n_reads, c.seed_cap);
        if ((rc = al->regs.need((size_t)c.reg_cap * sizeof(gbx_mem_reg), s)) || (rc = al->reg_off.need((size_t)(n_reads + 1) * 8, s)) ||
            (rc = al->sel_seeds.need((size_t)c.sel_cap * sizeof(gbx_bsw_seed), s)) ||
            (rc = al->sel_res.need((size_t)c.sel_cap * sizeof(gbx_bsw_seed_result), s)) || (rc = al->w_regs.need(wb, s)))
            return rc;
        if ((rc = gbx_mem_regs_device(&P.regs, n_reads, read_id0, al->chains.as<gbx_mem_chain>(), word(al, W_CHAINS), c.chain_cap,
                                      al->chain_off.as<int64_t>(), al->seeds.as<gbx_bsw_seed>(), word(al, W_SEEDS), c.seed_cap,
                                      al->res.as<gbx_bsw_seed_result>(), al->l_rep.as<int32_t>(), al->regs.as<gbx_mem_reg>(), c.reg_cap,
                                      al->reg_off.as<int64_t>(), word(al, W_REGS), al->sel_seeds.as<gbx_bsw_seed>(),
                                      al->sel_res.as<gbx_bsw_seed_result>(), c.sel_cap, word(al, W_SEL), al->w_regs.p, wb, s)))
            return rc;
    }
    // what the paired stage, the CIGAR stage and the SAM stage read: the regs stage's output, or the rescue's in its place
    const gbx_mem_reg *r_regs = al->regs.as<gbx_mem_reg>();
    const int64_t *r_off = al->reg_off.as<int64_t>(), *r_n = word(al, W_REGS);
    int64_t r_cap = c.reg_cap, k_cap = c.seed_cap, l_cap = c.sel_cap;
    const gbx_bsw_seed *k_seeds = al->seeds.as<gbx_bsw_seed>(), *l_seeds = al->sel_seeds.as<gbx_bsw_seed>();
    const gbx_bsw_seed_result *l_res = al->sel_res.as<gbx_bsw_seed_result>();
    const gbx_mem_pestat *d_pes_src = P.have_pes ? pes_at(al, WORDS_PES_GIVEN) : nullptr;
    if (rescue) {
        if (!P.have_pes) {
            d_pes_src = pes_at(al, WORDS_PES_EST);
            if (from <= GBX_MEM_ST_PESTAT) {
                const size_t wb = gbx_mem_pestat_workspace_bytes(P.pair.max_ins);
                if ((rc = al->w_pes.need(wb, s))) return rc;
                if ((rc = gbx_mem_pestat_device(&P.pair, n_pairs, r_regs, r_off, r_n, r_cap, ix->l_pac, pes_at(al, WORDS_PES_EST), al->w_pes.p, wb, s)))
                    return rc;
            }
        }
        if (from <= GBX_MEM_ST_RESCUE) {
            const size_t wb = gbx_mem_rescue_workspace_bytes(n_pairs, c.reg_cap, P.rescue.max_matesw);
            if ((rc = al->xregs.need((size_t)c.xreg_cap * sizeof(gbx_mem_reg), s)) || (rc = al->xreg_off.need((size_t)(n_reads + 1) * 8, s)) ||
                (rc = al->xseeds.need((size_t)c.xseed_cap * sizeof(gbx_bsw_seed), s)) ||
                (rc = al->xsel_seeds.need((size_t)c.xsel_cap * sizeof(gbx_bsw_seed), s)) ||
                (rc = al->xsel_res.need((size_t)c.xsel_cap * sizeof(gbx_bsw_seed_result), s)) ||
                (rc = al->xstats.need((size_t)std::max<int64_t>(n_pairs, 1) * sizeof(gbx_mem_rescue_stat), s)) || (rc = al->w_resc.need(wb, s)))
                return rc;
            if ((rc = gbx_mem_rescue_device(&P.rescue, n_pairs, id0, r_regs, r_off, r_n, r_cap, k_seeds, k_cap, al->l_rep.as<int32_t>(),
                                            d_read_off, d_read_len, ix->d_text, ix->text_bytes, d_enc, enc_bytes, ix->l_pac, ix->n_contigs,
                                            ix->d_contig_off, d_pes_src, al->xregs.as<gbx_mem_reg>(), c.xreg_cap, al->xreg_off.as<int64_t>(),
                                            word(al, W_XREGS), al->xseeds.as<gbx_bsw_seed>(), c.xseed_cap, word(al, W_XSEEDS),
                                            al->xsel_seeds.as<gbx_bsw_seed>(), al->xsel_res.as<gbx_bsw_seed_result>(), c.xsel_cap,
                                            word(al, W_XSEL), al->xstats.as<gbx_mem_rescue_stat>(), al->w_resc.p, wb, s)))
                return rc;
        }
        r_regs = al->xregs.as<gbx_mem_reg>(); r_off = al->xreg_off.as<int64_t>(); r_n = word(al, W_XREGS); r_cap = c.xreg_cap;
        k_seeds = al->xseeds.as<gbx_bsw_seed>(); k_cap = c.xseed_cap;
        l_seeds = al->xsel_seeds.as<gbx_bsw_seed>(); l_res = al->xsel_res.as<gbx_bsw_seed_result>(); l_cap = c.xsel_cap;
    }
    const gbx_mem_reg *s_regs = r_regs;              // the SAM stage's regions
    if (paired) {
        if (from <= GBX_MEM_ST_PAIR) {
            const size_t wb = gbx_mem_pair_workspace_bytes(n_pairs, r_cap, P.pair.max_ins);
            if ((rc = al->pairs.need((size_t)std::max<int64_t>(n_pairs, 1) * sizeof(gbx_mem_pair), s)) ||
                (rc = al->pregs.need((size_t)r_cap * sizeof(gbx_mem_reg), s)) ||
                (rc = al->psel_seeds.need((size_t)c.psel_cap * sizeof(gbx_bsw_seed), s)) ||
                (rc = al->psel_res.need((size_t)c.psel_cap * sizeof(gbx_bsw_seed_result), s)) || (rc = al->w_pair.need(wb, s)))
                return rc;
            if ((rc = gbx_mem_pair_device_pes(&P.pair, n_pairs, id0, r_regs, r_off, r_n, r_cap, l_seeds, l_res, l_cap, k_seeds, k_cap,
                                              al->l_rep.as<int32_t>(), ix->l_pac, ix->n_contigs, ix->d_contig_off, d_pes_src,
                                              pes_at(al, WORDS_PES_OUT), al->pairs.as<gbx_mem_pair>(), al->pregs.as<gbx_mem_reg>(),
                                              al->psel_seeds.as<gbx_bsw_seed>(), al->psel_res.as<gbx_bsw_seed_result>(), c.psel_cap,
                                              word(al, W_PSEL), al->w_pair.p, wb, s)))
                return rc;
        }
        s_regs = al->pregs.as<gbx_mem_reg>();
        l_seeds = al->psel_seeds.as<gbx_bsw_seed>(); l_res = al->psel_res.as<gbx_bsw_seed_result>(); l_cap = c.psel_cap;
    }
    if (from <= GBX_MEM_ST_CIGAR) {
        const size_t wb = gbx_mem_cigar_workspace_bytes(l_cap, c.z_bytes);
        if ((rc = al->alns.need((size_t)std::max<int64_t>(l_cap, 1) * sizeof(gbx_mem_aln), s)) || (rc = al->cigar.need((size_t)c.cigar_cap * 4, s)) ||
            (rc = al->w_cigar.need(wb, s)))
            return rc;
        if ((rc = gbx_mem_cigar_device(&P.cigar, l_cap, l_seeds, l_res, ix->d_text, ix->text_bytes, d_enc, enc_bytes, ix->l_pac, ix->n_contigs,
                                       ix->d_contig_off, al->alns.as<gbx_mem_aln>(), al->cigar.as<uint32_t>(), c.cigar_cap, word(al, W_CIGAR),
                                       al->w_cigar.p, wb, s)))
            return rc;
    }
    {
        const size_t wb = gbx_mem_sam_workspace_bytes(n_reads, r_cap, l_cap);
        if ((rc = al->recs.need((size_t)c.rec_cap * sizeof(gbx_mem_sam_rec), s)) || (rc = al->rec_off.need((size_t)(n_reads + 1) * 8, s)) ||
            (rc = al->md.need((size_t)c.md_cap, s)) || (rc = al->lines.need((size_t)c.text_cap, s)) || (rc = al->w_sam.need(wb, s)))
            return rc;
        if ((rc = gbx_mem_sam_device(&P.sam, n_reads, P.mode, s_regs, r_off, r_n, r_cap, paired ? al->pairs.as<gbx_mem_pair>() : nullptr,
                                     al->alns.as<gbx_mem_aln>(), l_cap, al->cigar.as<uint32_t>(), word(al, W_CIGAR), c.cigar_cap, d_enc, enc_bytes,
                                     d_read_off, d_read_len, d_qual, d_names, d_name_off, name_bytes, ix->d_cnames, ix->d_cname_off,
                                     ix->cname_bytes, ix->d_text, ix->text_bytes, ix->l_pac, ix->n_contigs, ix->d_contig_off,
                                     al->recs.as<gbx_mem_sam_rec>(), c.rec_cap, al->rec_off.as<int64_t>(), word(al, W_RECS), al->md.as<uint8_t>(),
                                     c.md_cap, word(al, W_MD), al->lines.as<uint8_t>(), c.text_cap, word(al, W_TEXT), al->w_sam.p, wb, s)))
            return rc;
    }
    MemAlignGather G;
    G.fmi_counters = (const unsigned long long *)al->w_fmi.p;
    G.n_smem = word(al, W_SMEM); G.n_pos = word(al, W_POS); G.n_chains = word(al, W_CHAINS); G.n_seeds = word(al, W_SEEDS);
    G.n_regs = word(al, W_REGS); G.n_sel = word(al, W_SEL);
    G.n_xregs = rescue ? word(al, W_XREGS) : nullptr; G.n_xseeds = rescue ? word(al, W_XSEEDS) : nullptr;
    G.n_xsel = rescue ? word(al, W_XSEL) : nullptr;
    G.n_psel = paired ? word(al, W_PSEL) : nullptr;
    G.n_cigar = word(al, W_CIGAR);
    G.alns = al->alns.as<gbx_mem_aln>(); G.n_alns = l_cap;
    G.n_recs = word(al, W_RECS); G.n_md = word(al, W_MD); G.n_text = word(al, W_TEXT);
    G.out = (gbx_mem_align_counts *)((char *)al->words.p + WORDS_COUNTS);
    return mem_align_gather_launch(G, s);
}

// the first stage whose capacity was too small, with that capacity grown to the need; -1: everything fitted
int first_overflow(gbx_mem_aligner *al, int64_t n_reads, int32_t max_len, const gbx_mem_align_counts &n, bool *by_slot)
{
    gbx_mem_align_caps &c = al->caps;
    const bool paired = al->p.mode == 1, rescue = rescue_runs(&al->p);
    *by_slot = false;
    auto grow = [](int64_t &cap, int64_t need) { const bool over = need > cap; if (over) cap = need; return over; };
    bool o = false;
    if (n.slot_worst > 0) {
        const int64_t now = c.slot > 0 ? c.slot : default_slot(&al->p, max_len);
        c.slot = std::max<int64_t>(n.slot_worst + 16, 2 * std::max<int64_t>(now, 48));
        *by_slot = o = true;
    }
    o |= grow(c.out_cap, n.n_smem);
    if (o) return GBX_MEM_ST_SMEM;
    if (grow(c.pos_cap, n.n_pos)) return GBX_MEM_ST_SAL;
    o = grow(c.chain_cap, n.n_chains);
    o |= grow(c.seed_cap, n.n_seeds);
    if (o) return GBX_MEM_ST_CHAIN;
    o = grow(c.reg_cap, n.n_regs);
    o |= grow(c.sel_cap, n.n_sel);
    if (o) return GBX_MEM_ST_REGS;
    if (rescue) {
        o = grow(c.xreg_cap, n.n_xregs);
        o |= grow(c.xseed_cap, n.n_xseeds);
        o |= grow(c.xsel_cap, n.n_xsel);
        if (o) return GBX_MEM_ST_RESCUE;
    }
    if (paired && grow(c.psel_cap, n.n_psel)) return GBX_MEM_ST_PAIR;
    o = grow(c.cigar_cap, n.n_cigar);
    if (n.n_z_miss > 0) {
        // the stage reports no need: the room the aligned records took, scaled to all of them, and half as much again
        const long double per = (long double)c.z_bytes / (long double)std::max<int64_t>(n.n_alns, 1);
        const int64_t est = (int64_t)std::ceil(per * (long double)(n.n_alns + n.n_z_miss) * 1.5L);
        c.z_bytes = std::max<int64_t>(2 * c.z_bytes, est);
        o = true;
    }
    if (o) return GBX_MEM_ST_CIGAR;
    o = grow(c.rec_cap, n.n_recs);
    o |= grow(c.md_cap, n.n_md);
    o |= grow(c.text_cap, n.n_text);
    if (o) return GBX_MEM_ST_SAM;
    (void)n_reads;
    return -1;
}

void set_mat(int a, int b, int32_t mat[25])
{
    for (int t = 0; t < 5; ++t)
        for (int q = 0; q < 5; ++q) mat[t * 5 + q] = t == 4 || q == 4 ? -1 : t == q ? a : -b;
}

}  // namespace

extern "C" {

void gbx_mem_align_sizes(int64_t out[5])
{
    if (!out) return;
    out[0] = sizeof(gbx_mem_align_params); out[1] = sizeof(gbx_mem_align_caps); out[2] = sizeof(gbx_mem_align_counts);
    out[3] = sizeof(gbx_mem_align_stats); out[4] = sizeof(gbx_mem_align_out);
}

void gbx_mem_align_default_params(gbx_mem_align_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    gbx_fmi_default_params(&p->fmi, 19);
    gbx_mem_chain_default_params(&p->chain);
    gbx_bsw_seed_default_params(&p->bsw);
    gbx_mem_regs_default_params(&p->regs);
    gbx_mem_pair_default_params(&p->pair);
    gbx_mem_rescue_default_params(&p->rescue);
    gbx_mem_cigar_default_params(&p->cigar);
    gbx_mem_sam_default_params(&p->sam);
    p->max_occ = p->chain.max_occ;
    p->mode = 1;
    for (int d = 0; d < 4; ++d) p->pes[d].failed = 1;
}

void gbx_mem_align_set_scoring(gbx_mem_align_params *p, int32_t a, int32_t b, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins,
                               int32_t pen_clip5, int32_t pen_clip3, int32_t pen_unpaired, int32_t w, int32_t zdrop, int32_t min_seed_len,
                               int32_t T)
{
    if (!p) return;
    p->chain.a = p->regs.a = p->pair.a = p->rescue.a = a;
    p->regs.b = p->pair.b = p->rescue.b = b;
    gbx_bsw_fill_scmat(a, b, -1, p->bsw.bsw.mat);
    set_mat(a, b, p->cigar.mat);
    p->chain.o_del = p->bsw.bsw.o_del = p->regs.o_del = p->pair.o_del = p->rescue.o_del = p->cigar.o_del = o_del;
    p->chain.e_del = p->bsw.bsw.e_del = p->regs.e_del = p->pair.e_del = p->rescue.e_del = p->cigar.e_del = e_del;
    p->chain.o_ins = p->bsw.bsw.o_ins = p->regs.o_ins = p->pair.o_ins = p->rescue.o_ins = p->cigar.o_ins = o_ins;
    p->chain.e_ins = p->bsw.bsw.e_ins = p->regs.e_ins = p->pair.e_ins = p->rescue.e_ins = p->cigar.e_ins = e_ins;
    p->chain.w = p->bsw.bsw.w = p->regs.w = p->cigar.w = w;
    p->bsw.bsw.zdrop = zdrop;
    p->bsw.pen_clip5 = pen_clip5; p->bsw.pen_clip3 = pen_clip3;
    p->pair.pen_unpaired = p->rescue.pen_unpaired = pen_unpaired;
    p->regs.T = p->pair.T = p->rescue.T = T;
    p->fmi.min_seed_len = p->chain.min_seed_len = p->regs.min_seed_len = p->pair.min_seed_len = p->rescue.min_seed_len = min_seed_len;
    p->fmi.split_len = (int32_t)(min_seed_len * 1.5 + .499);
}

int gbx_mem_align_check_params(const gbx_mem_align_params *p)
{
    const char *who = "gbx_mem_align_check_params";
    if (!p) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((p->mode != 0 && p->mode != 1) || (p->have_pes != 0 && p->have_pes != 1) || (p->no_rescue != 0 && p->no_rescue != 1)) {
        set_error("%s: mode = %d, have_pes = %d, no_rescue = %d (each 0 or 1)", who, p->mode, p->have_pes, p->no_rescue);
        return GBX_ERR_ARG;
    }
#define GBX_SAME(x, y) if (!((x) == (y))) { set_error("%s: %s and %s disagree", who, #x, #y); return GBX_ERR_ARG; }
    GBX_SAME(p->chain.a, p->regs.a) GBX_SAME(p->chain.a, p->pair.a) GBX_SAME(p->chain.a, p->rescue.a)
    GBX_SAME(p->regs.b, p->pair.b) GBX_SAME(p->regs.b, p->rescue.b)
    int8_t m8[25];
    int32_t m32[25];
    gbx_bsw_fill_scmat(p->chain.a, p->regs.b, -1, m8);
    set_mat(p->chain.a, p->regs.b, m32);
    if (memcmp(m8, p->bsw.bsw.mat, 25)) { set_error("%s: bsw.bsw.mat is not the matrix of a = %d, b = %d", who, p->chain.a, p->regs.b); return GBX_ERR_ARG; }
    if (memcmp(m32, p->cigar.mat, 100)) { set_error("%s: cigar.mat is not the matrix of a = %d, b = %d", who, p->chain.a, p->regs.b); return GBX_ERR_ARG; }
#define GBX_GAP(f) GBX_SAME(p->chain.f, p->bsw.bsw.f) GBX_SAME(p->chain.f, p->regs.f) GBX_SAME(p->chain.f, p->pair.f) \
                   GBX_SAME(p->chain.f, p->rescue.f) GBX_SAME(p->chain.f, p->cigar.f)
    GBX_GAP(o_del) GBX_GAP(e_del) GBX_GAP(o_ins) GBX_GAP(e_ins)
    GBX_SAME(p->chain.w, p->bsw.bsw.w) GBX_SAME(p->chain.w, p->regs.w) GBX_SAME(p->chain.w, p->cigar.w)
    GBX_SAME(p->pair.pen_unpaired, p->rescue.pen_unpaired)
    GBX_SAME(p->regs.T, p->pair.T) GBX_SAME(p->regs.T, p->rescue.T)
    GBX_SAME(p->fmi.min_seed_len, p->chain.min_seed_len) GBX_SAME(p->fmi.min_seed_len, p->regs.min_seed_len)
    GBX_SAME(p->fmi.min_seed_len, p->pair.min_seed_len) GBX_SAME(p->fmi.min_seed_len, p->rescue.min_seed_len)
    GBX_SAME(p->chain.max_chain_gap, p->regs.max_chain_gap) GBX_SAME(p->chain.max_chain_gap, p->rescue.max_chain_gap)
    GBX_SAME(p->chain.mask_level, p->regs.mask_level) GBX_SAME(p->chain.mask_level, p->pair.mask_level)
    GBX_SAME(p->chain.mask_level, p->rescue.mask_level)
    GBX_SAME(p->regs.mask_level_redun, p->rescue.mask_level_redun)
    GBX_SAME(p->chain.drop_ratio, p->regs.drop_ratio)
    GBX_SAME(p->regs.mapq_coef_len, p->pair.mapq_coef_len) GBX_SAME(p->regs.mapq_coef_len, p->rescue.mapq_coef_len)
    GBX_SAME(p->regs.mapq_coef_fac, p->pair.mapq_coef_fac) GBX_SAME(p->regs.mapq_coef_fac, p->rescue.mapq_coef_fac)
    GBX_SAME(p->max_occ, p->chain.max_occ)
#undef GBX_GAP
#undef GBX_SAME
    if (p->fmi.min_seed_len < 1 || p->fmi.split_len < 1) { set_error("%s: min_seed_len = %d, split_len = %d", who, p->fmi.min_seed_len, p->fmi.split_len); return GBX_ERR_ARG; }
    if (p->have_pes) return pes_given_check(p->pes, who);
    return GBX_OK;
}

int gbx_mem_align_plan(const gbx_mem_align_params *p, int64_t n_reads, int64_t bases, int32_t max_read_len, int64_t name_bytes,
                       const gbx_mem_align_counts *last, int64_t last_bases, gbx_mem_align_caps *caps)
{
    const char *who = "gbx_mem_align_plan";
    if (!p || !caps) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if (n_reads < 0 || bases < 0 || max_read_len < 0 || name_bytes < 0 || (last && last_bases < 1)) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    gbx_mem_align_caps c;
    memset(&c, 0, sizeof(c));
    c.out_cap = std::max<int64_t>(64, std::max<int64_t>(4 * n_reads, (int64_t)std::ceil(GUESS_SMEM * (double)bases)));
    c.pos_cap = std::max<int64_t>(64, (int64_t)std::ceil(GUESS_POS * (double)bases));
    c.chain_cap = std::max<int64_t>(64, std::max<int64_t>(2 * n_reads, (int64_t)std::ceil(GUESS_CHAIN * (double)bases)));
    c.cigar_cap = std::max<int64_t>(64, std::max<int64_t>(8 * n_reads, (int64_t)std::ceil(GUESS_CIGAR * (double)bases)));
    const int64_t zrec = (int64_t)gbx_mem_cigar_record_z_bytes(&p->cigar, max_read_len, max_read_len + 2 * std::max(p->cigar.w, 0));
    c.z_bytes = std::max<int64_t>(zrec, (int64_t)std::ceil(GUESS_Z_RECS * (double)n_reads) * zrec);
    if (last) {
        c.slot = last->slot_worst > 0 ? last->slot_worst + 16 : 0;
        c.out_cap = std::max<int64_t>(64, scaled(last->n_smem, bases, last_bases));
        c.pos_cap = std::max<int64_t>(64, scaled(last->n_pos, bases, last_bases));
        c.chain_cap = std::max<int64_t>(64, scaled(last->n_chains, bases, last_bases));
        c.cigar_cap = std::max<int64_t>(64, scaled(last->n_cigar, bases, last_bases));
        // every record takes the room of its own band: as many records as the last batch aligned, at the largest room one can take
        c.z_bytes = std::max<int64_t>(zrec, scaled(std::max<int64_t>(last->n_alns, 0), bases, last_bases) * zrec);
    }
    derive(p, n_reads, bases, name_bytes, &c, true);
    *caps = c;
    return GBX_OK;
}

// the contig table and names of an index entry's arguments -> the longest name
static int index_contigs_check(int64_t l_pac, int32_t n_contigs, const int64_t *contig_off, const uint8_t *cnames, const int64_t *cname_off,
                               const char *who, int32_t *max_name)
{
    int rc = contig_off_check(contig_off, n_contigs, l_pac, who);
    if (rc) return rc;
    if (cname_off[0] != 0) { set_error("%s: cname_off must start at 0", who); return GBX_ERR_ARG; }
    *max_name = 0;
    for (int32_t c = 0; c < n_contigs; ++c) {
        const int64_t l = cname_off[c + 1] - cname_off[c];
        if (l < 1 || l > 255) { set_error("%s: contig %d: a name of %lld bytes (1 .. 255)", who, c, (long long)l); return GBX_ERR_ARG; }
        *max_name = std::max<int32_t>(*max_name, (int32_t)l);
    }
    if (cname_off[n_contigs] > 0 && !cnames) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    return GBX_OK;
}

static gbx_mem_index *index_new(const gbx_fmi_index *idx, const gbx_fmi_sa *sa, int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                                const uint8_t *cnames, const int64_t *cname_off, int32_t max_name)
{
    gbx_mem_index *ix = new (std::nothrow) gbx_mem_index();
    if (!ix) return nullptr;
    const int64_t cname_bytes = cname_off[n_contigs];
    ix->idx = *idx; ix->idx.cp_occ = nullptr;
    ix->sa = *sa; ix->sa.ms_byte = nullptr; ix->sa.ls_word = nullptr;
    ix->d_index = ix->d_sa = nullptr; ix->d_text = nullptr; ix->d_contig_off = nullptr; ix->d_cnames = nullptr; ix->d_cname_off = nullptr;
    ix->l_pac = l_pac; ix->text_bytes = 2 * l_pac; ix->n_contigs = n_contigs; ix->max_cname = max_name; ix->cname_bytes = cname_bytes;
    ix->contig_off.assign(contig_off, contig_off + n_contigs + 1);
    ix->cname_off.assign(cname_off, cname_off + n_contigs + 1);
    ix->cnames.assign(cnames, cnames + cname_bytes);
    return ix;
}

// the text's 64 bytes of slack and the contig tables of ix, queued on s
static int index_tables(gbx_mem_index *ix, hipStream_t s)
{
    const size_t nc = (size_t)ix->n_contigs + 1;
    GBX_HIP(hipMemsetAsync(ix->d_text + ix->text_bytes, 0, 64, s));
    GBX_HIP(hipMalloc((void **)&ix->d_contig_off, nc * 8));
    GBX_HIP(hipMemcpyAsync(ix->d_contig_off, ix->contig_off.data(), nc * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMalloc((void **)&ix->d_cname_off, nc * 8));
    GBX_HIP(hipMemcpyAsync(ix->d_cname_off, ix->cname_off.data(), nc * 8, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMalloc((void **)&ix->d_cnames, (size_t)std::max<int64_t>(ix->cname_bytes, 1)));
    if (ix->cname_bytes) GBX_HIP(hipMemcpyAsync(ix->d_cnames, ix->cnames.data(), (size_t)ix->cname_bytes, hipMemcpyHostToDevice, s));
    return GBX_OK;
}

int gbx_mem_index_create(const gbx_fmi_index *idx, const gbx_fmi_sa *sa, const uint8_t *text, int64_t l_pac, int32_t n_contigs,
                         const int64_t *contig_off, const uint8_t *cnames, const int64_t *cname_off, gbx_mem_index **out)
{
    const char *who = "gbx_mem_index_create";
    if (!idx || !sa || !text || !contig_off || !cname_off || !out || !idx->cp_occ || !sa->ms_byte || !sa->ls_word) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    *out = nullptr;
    int rc = fmi_index_check(idx, (1ll << 40) - 1, who);
    if (rc) return rc;
    if (l_pac < 1 || n_contigs < 1 || idx->ref_seq_len != 2 * l_pac + 1) {
        set_error("%s: l_pac = %lld, n_contigs = %d, ref_seq_len = %lld (2 l_pac + 1)", who, (long long)l_pac, n_contigs, (long long)idx->ref_seq_len);
        return GBX_ERR_ARG;
    }
    const int64_t want = sa->sa_compx ? (idx->ref_seq_len >> 3) + 1 : idx->ref_seq_len;
    if ((sa->sa_compx != 0 && sa->sa_compx != 3) || sa->n_sa != want) { set_error("%s: sa_compx = %d, n_sa = %lld", who, sa->sa_compx, (long long)sa->n_sa); return GBX_ERR_ARG; }
    int32_t max_name = 0;
    if ((rc = index_contigs_check(l_pac, n_contigs, contig_off, cnames, cname_off, who, &max_name))) return rc;
    if ((rc = require_device())) return rc;
    gbx_mem_index *ix = index_new(idx, sa, l_pac, n_contigs, contig_off, cnames, cname_off, max_name);
    if (!ix) { set_error("%s: out of host memory", who); return GBX_ERR_NOMEM; }
    void *t_cp = nullptr, *t_ms = nullptr, *t_ls = nullptr;
    hipStream_t s = nullptr;
    auto work = [&]() -> int {
        GBX_HIP(hipGetDevice(&ix->dev));
        GBX_HIP(hipStreamCreate(&s));
        const size_t ib = fmi_index_bytes(idx->ref_seq_len), sb = fmi_sa_bytes(sa->n_sa, idx->ref_seq_len), n_sa = (size_t)sa->n_sa;
        GBX_HIP(hipMalloc(&ix->d_index, ib));
        GBX_HIP(hipMalloc(&t_cp, ib));
        GBX_HIP(hipMemcpyAsync(t_cp, idx->cp_occ, ((size_t)(idx->ref_seq_len >> 6) + 1) * sizeof(gbx_fmi_cp_occ), hipMemcpyHostToDevice, s));
        gbx_fmi_index di = *idx;
        di.cp_occ = (const gbx_fmi_cp_occ *)t_cp;
        int rc2 = fmi_index_build(&di, ix->d_index, ib, s);
        if (rc2) return rc2;
        GBX_HIP(hipMalloc(&ix->d_sa, std::max<size_t>(sb, 1)));
        GBX_HIP(hipMalloc(&t_ms, n_sa));
        GBX_HIP(hipMalloc(&t_ls, n_sa * 4));
        GBX_HIP(hipMemcpyAsync(t_ms, sa->ms_byte, n_sa, hipMemcpyHostToDevice, s));
        GBX_HIP(hipMemcpyAsync(t_ls, sa->ls_word, n_sa * 4, hipMemcpyHostToDevice, s));
        gbx_fmi_sa ds = *sa;
        ds.ms_byte = (const int8_t *)t_ms; ds.ls_word = (const uint32_t *)t_ls;
        if ((rc2 = fmi_sa_build(&ds, idx->ref_seq_len, ix->d_sa, sb, s))) return rc2;
        GBX_HIP(hipMalloc((void **)&ix->d_text, (size_t)ix->text_bytes + 64));
        GBX_HIP(hipMemcpyAsync(ix->d_text, text, (size_t)ix->text_bytes, hipMemcpyHostToDevice, s));
        if ((rc2 = index_tables(ix, s))) return rc2;
        GBX_HIP(hipStreamSynchronize(s));
        return GBX_OK;
    };
    rc = work();
    if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    if (t_cp) (void)hipFree(t_cp);
    if (t_ms) (void)hipFree(t_ms);
    if (t_ls) (void)hipFree(t_ls);
    if (rc) { gbx_mem_index_destroy(ix); return rc; }
    *out = ix;
    return GBX_OK;
}

int gbx_mem_index_build(const uint8_t *genome, int64_t l_pac, int32_t n_contigs, const int64_t *contig_off, const uint8_t *cnames,
                        const int64_t *cname_off, gbx_mem_index **out)
{
    const char *who = "gbx_mem_index_build";
    if (!genome || !contig_off || !cname_off || !out) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    *out = nullptr;
    int rc = fmi_build_check(genome, l_pac, 3, who);
    if (rc) return rc;
    if (n_contigs < 1) { set_error("%s: n_contigs = %d", who, n_contigs); return GBX_ERR_ARG; }
    int32_t max_name = 0;
    if ((rc = index_contigs_check(l_pac, n_contigs, contig_off, cnames, cname_off, who, &max_name))) return rc;
    if ((rc = require_device())) return rc;
    gbx_fmi_index idx{};
    idx.ref_seq_len = 2 * l_pac + 1;
    gbx_fmi_sa sa{};
    sa.sa_compx = 3; sa.n_sa = (idx.ref_seq_len >> 3) + 1;
    gbx_mem_index *ix = index_new(&idx, &sa, l_pac, n_contigs, contig_off, cnames, cname_off, max_name);
    if (!ix) { set_error("%s: out of host memory", who); return GBX_ERR_NOMEM; }
    void *t_g = nullptr, *t_cp = nullptr, *t_ms = nullptr, *t_ls = nullptr, *t_info = nullptr, *t_work = nullptr;
    hipStream_t s = nullptr;
    auto work = [&]() -> int {
        GBX_HIP(hipGetDevice(&ix->dev));
        GBX_HIP(hipStreamCreate(&s));
        const size_t ib = fmi_index_bytes(idx.ref_seq_len), sb = fmi_sa_bytes(sa.n_sa, idx.ref_seq_len), n_sa = (size_t)sa.n_sa;
        const size_t wb = fmi_build_workspace_bytes(l_pac);
        GBX_HIP(hipMalloc(&t_g, (size_t)l_pac));
        GBX_HIP(hipMalloc(&t_cp, ib));                                       // as gbx_mem_index_create sizes it
        GBX_HIP(hipMalloc(&t_ms, n_sa));
        GBX_HIP(hipMalloc(&t_ls, n_sa * 4));
        GBX_HIP(hipMalloc(&t_info, 64));
        GBX_HIP(hipMalloc(&t_work, wb));
        GBX_HIP(hipMalloc((void **)&ix->d_text, (size_t)ix->text_bytes + 64));
        GBX_HIP(hipMemcpyAsync(t_g, genome, (size_t)l_pac, hipMemcpyHostToDevice, s));
        int rc2 = fmi_build_launch((const uint8_t *)t_g, l_pac, 3, (gbx_fmi_cp_occ *)t_cp, (int8_t *)t_ms, (uint32_t *)t_ls, ix->d_text, (int64_t *)t_info,
                                   t_work, wb, s);
        if (rc2) return rc2;
        int64_t w[8];
        GBX_HIP(hipMemcpyAsync(w, t_info, 64, hipMemcpyDeviceToHost, s));
        GBX_HIP(hipStreamSynchronize(s));
        (void)hipFree(t_work); t_work = nullptr;                             // the workspace goes before the layouts come
        for (int c = 0; c < 5; ++c) ix->idx.count[c] = w[c];
        ix->idx.sentinel_index = w[5];
        if ((rc2 = fmi_index_check(&ix->idx, (1ll << 40) - 1, who))) return rc2;
        gbx_fmi_index di = ix->idx;
        di.cp_occ = (const gbx_fmi_cp_occ *)t_cp;
        GBX_HIP(hipMalloc(&ix->d_index, ib));
        if ((rc2 = fmi_index_build(&di, ix->d_index, ib, s))) return rc2;
        GBX_HIP(hipMalloc(&ix->d_sa, std::max<size_t>(sb, 1)));
        gbx_fmi_sa ds = sa;
        ds.ms_byte = (const int8_t *)t_ms; ds.ls_word = (const uint32_t *)t_ls;
        if ((rc2 = fmi_sa_build(&ds, idx.ref_seq_len, ix->d_sa, sb, s))) return rc2;
        if ((rc2 = index_tables(ix, s))) return rc2;
        GBX_HIP(hipStreamSynchronize(s));
        return GBX_OK;
    };
    rc = work();
    if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (void *q : {t_g, t_cp, t_ms, t_ls, t_info, t_work}) if (q) (void)hipFree(q);
    if (rc) { gbx_mem_index_destroy(ix); return rc; }
    *out = ix;
    return GBX_OK;
}

void gbx_mem_index_destroy(gbx_mem_index *ix)
{
    if (!ix) return;
    void *ps[] = {ix->d_index, ix->d_sa, ix->d_text, ix->d_contig_off, ix->d_cnames, ix->d_cname_off};
    for (void *q : ps) if (q) (void)hipFree(q);
    delete ix;
}

int gbx_mem_sam_header(const gbx_mem_index *ix, uint8_t *buf, int64_t cap, int64_t *need)
{
    if (!ix || !need || (cap > 0 && !buf) || cap < 0) { set_error("gbx_mem_sam_header: bad argument"); return GBX_ERR_ARG; }
    std::string h;
    for (int32_t c = 0; c < ix->n_contigs; ++c) {
        h += "@SQ\tSN:";
        h.append((const char *)ix->cnames.data() + ix->cname_off[(size_t)c], (size_t)(ix->cname_off[(size_t)c + 1] - ix->cname_off[(size_t)c]));
        h += "\tLN:" + std::to_string((long long)(ix->contig_off[(size_t)c + 1] - ix->contig_off[(size_t)c])) + "\n";
    }
    *need = (int64_t)h.size();
    if (cap < *need) { set_error("gbx_mem_sam_header: %lld bytes do not fit cap = %lld", (long long)*need, (long long)cap); return GBX_ERR_ARG; }
    memcpy(buf, h.data(), h.size());
    return GBX_OK;
}

int gbx_mem_aligner_create(const gbx_mem_index *ix, const gbx_mem_align_params *p, const gbx_mem_align_caps *first, gbx_mem_aligner **out)
{
    const char *who = "gbx_mem_aligner_create";
    if (!ix || !p || !out) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    *out = nullptr;
    int rc = gbx_mem_align_check_params(p);
    if (rc) return rc;
    if (first) {
        const int64_t *v = (const int64_t *)first;
        for (int k = 0; k < N_CAPS; ++k)
            if (v[k] < 0 || v[k] >= (1ll << 40)) { set_error("%s: first capacity %d = %lld", who, k, (long long)v[k]); return GBX_ERR_ARG; }
        if (first->slot > (1 << 20)) { set_error("%s: first slot = %lld", who, (long long)first->slot); return GBX_ERR_ARG; }
    }
    if ((rc = require_device())) return rc;
    gbx_mem_aligner *al = new (std::nothrow) gbx_mem_aligner();
    if (!al) { set_error("%s: out of host memory", who); return GBX_ERR_NOMEM; }
    al->ix = ix; al->p = *p;
    memset(&al->caps, 0, sizeof(al->caps)); memset(&al->stats, 0, sizeof(al->stats)); memset(&al->last, 0, sizeof(al->last));
    al->have_first = first != nullptr; al->have_last = false; al->last_bases = 0;
    if (first) al->first = *first;
    al->s = nullptr;
    auto work = [&]() -> int {
        GBX_HIP(hipSetDevice(ix->dev));
        GBX_HIP(hipStreamCreate(&al->s));
        int rc2;
        if ((rc2 = al->words.need(WORDS_BYTES, al->s)) || (rc2 = al->h_counts.need(sizeof(gbx_mem_align_counts) + 128))) return rc2;
        gbx_mem_pestat given[4];
        for (int d = 0; d < 4; ++d) given[d] = p->have_pes ? p->pes[d] : gbx_mem_pestat{0, 0, 1, 0, 0., 0.};
        GBX_HIP(hipMemcpyAsync(pes_at(al, WORDS_PES_GIVEN), given, sizeof(given), hipMemcpyHostToDevice, al->s));
        GBX_HIP(hipStreamSynchronize(al->s));
        return GBX_OK;
    };
    if ((rc = work())) { gbx_mem_aligner_destroy(al); return rc; }
    *out = al;
    return GBX_OK;
}

void gbx_mem_aligner_destroy(gbx_mem_aligner *al)
{
    if (!al) return;
    if (al->s) (void)hipStreamSynchronize(al->s);
    Grow *g[] = {&al->in, &al->smems, &al->smem_off, &al->pos, &al->pos_off, &al->chains, &al->chain_off, &al->seeds, &al->l_rep, &al->res,
                 &al->regs, &al->reg_off, &al->sel_seeds, &al->sel_res, &al->xregs, &al->xreg_off, &al->xseeds, &al->xsel_seeds, &al->xsel_res,
                 &al->xstats, &al->pairs, &al->pregs, &al->psel_seeds, &al->psel_res, &al->alns, &al->cigar, &al->recs, &al->rec_off, &al->md,
                 &al->lines, &al->words, &al->w_fmi, &al->w_sal, &al->w_chain, &al->w_ext, &al->w_regs, &al->w_pes, &al->w_resc, &al->w_pair,
                 &al->w_cigar, &al->w_sam};
    for (Grow *b : g) b->drop();
    al->h_in.drop(); al->h_out.drop(); al->h_counts.drop();
    if (al->s) (void)hipStreamDestroy(al->s);
    delete al;
}

int gbx_mem_aligner_stats(const gbx_mem_aligner *al, gbx_mem_align_stats *stats)
{
    if (!al || !stats) { set_error("gbx_mem_aligner_stats: null pointer"); return GBX_ERR_ARG; }
    *stats = al->stats;
    return GBX_OK;
}

int gbx_mem_aligner_run(gbx_mem_aligner *al, int64_t n_reads, int64_t id0, const uint8_t *enc, int64_t enc_bytes,
                        const int64_t *read_off, const int32_t *read_len, const uint8_t *qual,
                        const uint8_t *names, const int64_t *name_off, gbx_mem_align_out *out)
{
    RoctxRange range_("gbx_mem_aligner_run");
    const char *who = "gbx_mem_aligner_run";
    if (!al || !out || !name_off || (n_reads > 0 && (!enc || !read_off || !read_len))) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    const gbx_mem_align_params &P = al->p;
    const bool paired = P.mode == 1, rescue = rescue_runs(&P);
    if (n_reads < 0 || enc_bytes < 0 || n_reads >= (1ll << 28)) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    if (paired && (n_reads & 1)) { set_error("%s: n_reads = %lld is odd in mode 1 (interleaved pairs)", who, (long long)n_reads); return GBX_ERR_ARG; }
    const int64_t id_end = paired ? id0 + n_reads / 2 : id0 + n_reads, id_max = paired ? 1ll << 23 : 1ll << 24;
    if (id0 < 0 || id0 > id_max || id_end > id_max) {
        set_error("%s: id0 = %lld with %lld %s: ids lie in [0, 2^%d]", who, (long long)id0, (long long)(paired ? n_reads / 2 : n_reads),
                  paired ? "pairs" : "reads", paired ? 23 : 24);
        return GBX_ERR_ARG;
    }
    const int32_t len_limit = rescue ? 1024 : GBX_BSW_MAX_QLEN;
    int32_t max_len = 0;
    int64_t bases = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (read_off[r] < 0 || (r > 0 && read_off[r] < read_off[r - 1])) { set_error("%s: read_off is not monotone at read %lld", who, (long long)r); return GBX_ERR_ARG; }
        if (read_len[r] < 1) { set_error("%s: read %lld has no base", who, (long long)r); return GBX_ERR_ARG; }
        if (read_off[r] > enc_bytes - read_len[r]) { set_error("%s: read %lld lies outside the %lld bases", who, (long long)r, (long long)enc_bytes); return GBX_ERR_ARG; }
        if (read_len[r] > len_limit) {
            set_error("%s: read %lld has %d bases, more than the %d of %s", who, (long long)r, read_len[r], len_limit,
                      rescue ? "the mate rescue" : "the seed extension");
            return GBX_ERR_UNSUPPORTED;
        }
        max_len = std::max(max_len, read_len[r]);
        bases += read_len[r];
    }
    if (name_off[0] < 0) { set_error("%s: name_off leaves the names", who); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n_reads; ++r)
        if (name_off[r + 1] < name_off[r]) { set_error("%s: name_off is not monotone at read %lld", who, (long long)r); return GBX_ERR_ARG; }
    const int64_t name_bytes = name_off[n_reads];
    if (name_bytes > 0 && !names) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    int rc;
    GBX_HIP(hipSetDevice(al->ix->dev));
    hipStream_t s = al->s;

    // ---- capacities of this run
    gbx_mem_align_caps want;
    if (al->have_first && al->stats.runs == 0) want = al->first;
    else if ((rc = gbx_mem_align_plan(&P, n_reads, bases, max_len, name_bytes, al->have_last ? &al->last : nullptr, al->last_bases, &want))) return rc;
    want.slot = std::max(want.slot, al->caps.slot);
    {
        int64_t *v = (int64_t *)&want;
        for (int k = 1; k < N_CAPS; ++k) v[k] = std::max<int64_t>(v[k], 1);
        derive(&P, n_reads, bases, name_bytes, &want, false);
    }
    al->caps = want;
    al->stats.runs += 1;
    al->stats.reruns = al->stats.slot_reruns = 0;
    al->stats.bytes_up = al->stats.bytes_down = 0;
    memset(al->stats.rerun_stage, 0xff, sizeof(al->stats.rerun_stage));

    // ---- one upload: the batch in one pinned image, laid out as the device arena
    const size_t o_off = up256((size_t)enc_bytes + 64), o_len = o_off + up256((size_t)(n_reads + 1) * 8),
                 o_qual = o_len + up256((size_t)(n_reads + 1) * 4), o_names = o_qual + up256(qual ? (size_t)enc_bytes + 64 : 0),
                 o_noff = o_names + up256((size_t)name_bytes + 64), total = o_noff + up256((size_t)(n_reads + 1) * 8);
    al->o_off = o_off; al->o_len = o_len; al->o_qual = o_qual; al->o_names = o_names; al->o_noff = o_noff; al->in_bytes = total;
    if ((rc = al->h_in.need(total)) || (rc = al->in.need(total, s))) return rc;
    {
        char *h = (char *)al->h_in.p;
        memset(h, 0, total);
        if (enc_bytes) memcpy(h, enc, (size_t)enc_bytes);
        if (n_reads) memcpy(h + o_off, read_off, (size_t)n_reads * 8);
        if (n_reads) memcpy(h + o_len, read_len, (size_t)n_reads * 4);
        if (qual && enc_bytes) memcpy(h + o_qual, qual, (size_t)enc_bytes);
        if (name_bytes) memcpy(h + o_names, names, (size_t)name_bytes);
        memcpy(h + o_noff, name_off, (size_t)(n_reads + 1) * 8);
    }
    GBX_HIP(hipMemcpyAsync(al->in.p, al->h_in.p, total, hipMemcpyHostToDevice, s));
    al->stats.bytes_up += (int64_t)total;

    // ---- the chain, the counts, and again from the first stage that overflowed
    gbx_mem_align_counts *hc = (gbx_mem_align_counts *)al->h_counts.p;
    int from = GBX_MEM_ST_SMEM;
    for (;;) {
        if ((rc = queue_chain(al, from, n_reads, id0, enc_bytes, max_len, name_bytes, qual != nullptr))) { (void)hipStreamSynchronize(s); return rc; }
        GBX_HIP(hipMemcpyAsync(hc, (char *)al->words.p + WORDS_COUNTS, sizeof(*hc), hipMemcpyDeviceToHost, s));
        GBX_HIP(hipStreamSynchronize(s));
        al->stats.bytes_down += (int64_t)sizeof(*hc);
        al->stats.counts = *hc;
        bool by_slot = false;
        const gbx_mem_align_caps was = al->caps;
        from = first_overflow(al, n_reads, max_len, *hc, &by_slot);
        if (from < 0) break;
        follow(&P, n_reads, bases, name_bytes, was, &al->caps);
        if (al->caps.slot > (1 << 20) || al->stats.reruns >= 4 * GBX_MEM_ALIGN_MAX_RERUNS) {
            set_error("%s: the capacities did not settle after %d reruns (stage %d)", who, al->stats.reruns, from);
            return GBX_ERR_UNSUPPORTED;
        }
        if (al->stats.reruns < GBX_MEM_ALIGN_MAX_RERUNS) al->stats.rerun_stage[al->stats.reruns] = from;
        al->stats.reruns += 1;
        al->stats.slot_reruns += by_slot ? 1 : 0;
    }
    al->stats.caps = al->caps;
    al->last = *hc; al->last_bases = std::max<int64_t>(bases, 1); al->have_last = true;

    // ---- the download: exactly n_recs records, n_text bytes, the offsets and the estimate
    const size_t b_recs = (size_t)hc->n_recs * sizeof(gbx_mem_sam_rec), b_off = (size_t)(n_reads + 1) * 8, b_text = (size_t)hc->n_text;
    const size_t h_off = up256(b_recs), h_text = h_off + up256(b_off), h_pes = h_text + up256(b_text + 1), h_total = h_pes + 256;
    if ((rc = al->h_out.need(h_total))) return rc;
    char *ho = (char *)al->h_out.p;
    if (b_recs) GBX_HIP(hipMemcpyAsync(ho, al->recs.p, b_recs, hipMemcpyDeviceToHost, s));
    GBX_HIP(hipMemcpyAsync(ho + h_off, al->rec_off.p, b_off, hipMemcpyDeviceToHost, s));
    if (b_text) GBX_HIP(hipMemcpyAsync(ho + h_text, al->lines.p, b_text, hipMemcpyDeviceToHost, s));
    if (paired) GBX_HIP(hipMemcpyAsync(ho + h_pes, pes_at(al, WORDS_PES_OUT), 4 * sizeof(gbx_mem_pestat), hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    al->stats.bytes_down += (int64_t)(b_recs + b_off + b_text + (paired ? 128 : 0));
    out->sam = (const uint8_t *)(ho + h_text); out->n_text = hc->n_text;
    out->recs = (const gbx_mem_sam_rec *)ho; out->n_recs = hc->n_recs;
    out->rec_off = (const int64_t *)(ho + h_off);
    for (int d = 0; d < 4; ++d) out->pes[d] = paired ? ((const gbx_mem_pestat *)(ho + h_pes))[d] : gbx_mem_pestat{0, 0, 1, 0, 0., 0.};
    out->stats = al->stats;
    return GBX_OK;
}

}  // extern "C"
