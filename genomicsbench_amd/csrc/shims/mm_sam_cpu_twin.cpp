// mm_sam_cpu_twin.cpp — the device's SAM / cs / MD / eqx rules (mm_sam_rules.h) compiled for the host into libgbx_mm_cpu.so.  The
// CPU tests hold it against the plain-Python restatement tests/mm_sam_ref.py, so the text the kernels run is tested where there
// is no GPU: with a team of one lane, and with a team of up to 64 host threads that meet at every ballot, scan and shuffle as a
// wavefront's lanes do - the paths a single lane never takes (a step of many columns, a batch of many words).
#include <pthread.h>
#include <thread>
#include <vector>
#include "../mm_sam_rules.h"

namespace {

struct Meet { pthread_barrier_t bar; int64_t slot[64]; };

struct ThreadTeam {                                // lane l of n threads; every collective is two barriers around the shared slots
    int l, n; Meet *m;
    int lane() const { return l; }
    int size() const { return n; }
    void sync() const { pthread_barrier_wait(&m->bar); }
    template <class R, class F> R meet(int64_t v, F f) const
    {
        m->slot[l] = v;
        pthread_barrier_wait(&m->bar);
        const R r = f();
        pthread_barrier_wait(&m->bar);
        return r;
    }
    uint64_t ballot(bool b) const
    {
        return meet<uint64_t>(b, [&] { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)(m->slot[i] != 0) << i; return x; });
    }
    int64_t scan(int64_t v, int64_t *total) const
    {
        int64_t all = 0;
        const int64_t below = meet<int64_t>(v, [&] { int64_t s = 0; for (int i = 0; i < n; ++i) { if (i == l) s = all; all += m->slot[i]; } return s; });
        *total = all;
        return below;
    }
    int64_t shfl(int64_t v, int src) const { return meet<int64_t>(v, [&] { return m->slot[src]; }); }
};

}  // namespace

extern "C" {

// The text of gbx_mm_sam_* -> its length; bytes below text_cap are written, line_off[n_reads + 1] and counts[2] always.  qual may be
// null.  P: a gbx_mm_sam_params.  lanes: 1, or 2 .. 64 for the team of threads.
int64_t gbx_mm_sam_cpu_lanes(const gbx_mm_sam_params *P, int lanes, int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns,
                             const uint32_t *cigar, int64_t n_cigar, const uint8_t *qnames, const int64_t *qname_off, const uint8_t *seq, const uint8_t *qual,
                             const int64_t *seq_off, const int32_t *rep_len, int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off,
                             const uint8_t *tseq, const int64_t *tseq_off, uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *counts)
{
    const gbx::MmSamView V{gbx::MmPafView{n_reads, regs, alns, cigar, n_cigar, qnames, qname_off, seq_off, rep_len, n_targets, tnames, tname_off, tseq_off},
                           reg_off, seq, qual, tseq, *P};
    const int64_t n_regs = n_reads > 0 ? reg_off[n_reads] : 0;
    if (lanes <= 1) return gbx::mm_sam_text(gbx::MmSamSolo{}, V, n_regs, lines, text_cap, line_off, counts);
    if (lanes > 64) lanes = 64;
    Meet m;
    pthread_barrier_init(&m.bar, nullptr, (unsigned)lanes);
    std::vector<int64_t> len((size_t)lanes);
    std::vector<std::thread> th;
    for (int l = 0; l < lanes; ++l)
        th.emplace_back([&, l] { len[(size_t)l] = gbx::mm_sam_text(ThreadTeam{l, lanes, &m}, V, n_regs, lines, text_cap, line_off, counts); });
    for (auto &t : th) t.join();
    pthread_barrier_destroy(&m.bar);
    for (int l = 1; l < lanes; ++l)
        if (len[(size_t)l] != len[0]) return -1;                        // the lanes disagree: never
    return len[0];
}

int64_t gbx_mm_sam_cpu(const gbx_mm_sam_params *P, int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns,
                       const uint32_t *cigar, int64_t n_cigar, const uint8_t *qnames, const int64_t *qname_off, const uint8_t *seq, const uint8_t *qual,
                       const int64_t *seq_off, const int32_t *rep_len, int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off,
                       const uint8_t *tseq, const int64_t *tseq_off, uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *counts)
{
    return gbx_mm_sam_cpu_lanes(P, 1, n_reads, regs, reg_off, alns, cigar, n_cigar, qnames, qname_off, seq, qual, seq_off, rep_len, n_targets, tnames, tname_off,
                                tseq, tseq_off, lines, text_cap, line_off, counts);
}

}  // extern "C"
