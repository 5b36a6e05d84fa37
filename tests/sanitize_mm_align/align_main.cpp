// align_main.cpp — the host twin of the base-level alignment stage under ASan + UBSan, in a program of its own.
//   align_main <batch.bin> <out.bin>
// batch.bin: int64 head[10] = n_reads, n_regs, n_anchors, n_targets, read bytes, target bytes, read-name bytes, target-name bytes,
// CIGAR words, bytes of z; gbx_mm_align_params; then regs, reg_off, off, cax, cay, n_chained, seq, seq_off, tseq, tseq_off, qnames,
// qname_off, tnames, tname_off, rep_len.  Every buffer is a heap block of exactly the size the entry names, so a write or read
// past one is reported; the CIGAR room is exactly the words the batch makes and z_bytes exactly its need.
// out.bin: counts[3], alns, the words, n_text, the PAF-with-CIGAR text.
#include <cstdio>
#include <cstdlib>
#include "../../genomicsbench_amd/csrc/shims/mm_align_cpu_twin.cpp"

namespace {
template <class T> std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "align_main: short input\n"); exit(2); }
    return v;
}
template <class T> void put(FILE *f, const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: align_main <batch.bin> <out.bin>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "align_main: cannot read %s\n", argv[1]); return 1; }
    const std::vector<int64_t> h = take<int64_t>(f, 10);
    const size_t n = (size_t)h[0], nr = (size_t)h[1], na = (size_t)h[2], nt = (size_t)h[3];
    const gbx_mm_align_params P = take<gbx_mm_align_params>(f, 1)[0];
    const auto regs = take<gbx_mm_reg>(f, nr);
    const auto reg_off = take<int64_t>(f, n + 1), off = take<int64_t>(f, n + 1);
    const auto cax = take<uint64_t>(f, na), cay = take<uint64_t>(f, na);
    const auto n_chained = take<int32_t>(f, n);
    const auto seq = take<uint8_t>(f, (size_t)h[4]);
    const auto seq_off = take<int64_t>(f, n + 1);
    const auto tseq = take<uint8_t>(f, (size_t)h[5]);
    const auto tseq_off = take<int64_t>(f, nt + 1);
    const auto qn = take<uint8_t>(f, (size_t)h[6]);
    const auto qo = take<int64_t>(f, n + 1);
    const auto tn = take<uint8_t>(f, (size_t)h[7]);
    const auto to = take<int64_t>(f, nt + 1);
    const auto rep = take<int32_t>(f, n);
    fclose(f);
    std::vector<gbx_mm_aln> alns(nr);
    std::vector<uint32_t> cig((size_t)h[8]);
    int64_t counts[3];
    gbx_mm_align_cpu(&P, (int64_t)n, (int64_t)nr, regs.data(), off.data(), cax.data(), cay.data(), n_chained.data(), seq.data(), seq_off.data(), (int64_t)nt,
                     tseq.data(), tseq_off.data(), alns.data(), cig.data(), h[8], h[9], counts);
    if (counts[1] != h[8] || counts[2] != h[9]) { fprintf(stderr, "align_main: %lld words, %lld bytes of z\n", (long long)counts[1], (long long)counts[2]); return 3; }
    std::vector<int64_t> line_off(n + 1);
    // measured with no room at all, then written into exactly that much
    const int64_t need = gbx_mm_paf_cigar_cpu((int64_t)n, regs.data(), reg_off.data(), alns.data(), cig.data(), counts[1], qn.data(), qo.data(), seq_off.data(),
                                              rep.data(), (int64_t)nt, tn.data(), to.data(), tseq_off.data(), nullptr, 0, line_off.data());
    std::vector<uint8_t> text((size_t)need);
    const int64_t got = gbx_mm_paf_cigar_cpu((int64_t)n, regs.data(), reg_off.data(), alns.data(), cig.data(), counts[1], qn.data(), qo.data(), seq_off.data(),
                                             rep.data(), (int64_t)nt, tn.data(), to.data(), tseq_off.data(), text.data(), need, line_off.data());
    if (got != need) { fprintf(stderr, "align_main: the text's length changed (%lld, %lld)\n", (long long)need, (long long)got); return 3; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "align_main: cannot write %s\n", argv[2]); return 1; }
    put(o, counts, 3); put(o, alns.data(), nr); put(o, cig.data(), (size_t)counts[1]); put(o, &need, 1); put(o, text.data(), (size_t)need);
    fclose(o);
    printf("align_main: %zu reads, %zu regions, %lld jobs, %lld words, %lld bytes of text\n", n, nr, (long long)counts[0], (long long)counts[1], (long long)need);
    return 0;
}
