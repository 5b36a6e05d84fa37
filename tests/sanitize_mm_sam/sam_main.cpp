// sam_main.cpp — the host twin of the mm sam stage under ASan + UBSan, in a program of its own.
//   sam_main <batch.bin> <out.bin>
// batch.bin: int64 head[10] = n_reads, n_regs, n_targets, read bytes, target bytes, read-name bytes, target-name bytes, CIGAR words,
// 1 with qualities, n_sets; then regs, reg_off, alns, cigar, qnames, qname_off, seq, qual (with qualities), seq_off, rep_len, tnames,
// tname_off, tseq, tseq_off; then n_sets times { gbx_mm_sam_params, int32 lanes }.  Every buffer is a heap block of exactly the size
// the entry names, so a write or read past one is reported; a set's text is measured with no room at all, then written into
// exactly that much.
// out.bin: a set after another: n_text, counts[2], line_off[n_reads + 1], the text.
#include <cstdio>
#include <cstdlib>
#include "../../genomicsbench_amd/csrc/shims/mm_sam_cpu_twin.cpp"

namespace {
template <class T> std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "sam_main: short input\n"); exit(2); }
    return v;
}
template <class T> void put(FILE *f, const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: sam_main <batch.bin> <out.bin>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "sam_main: cannot read %s\n", argv[1]); return 1; }
    const std::vector<int64_t> h = take<int64_t>(f, 10);
    const size_t n = (size_t)h[0], nr = (size_t)h[1], nt = (size_t)h[2];
    const auto regs = take<gbx_mm_reg>(f, nr);
    const auto reg_off = take<int64_t>(f, n + 1);
    const auto alns = take<gbx_mm_aln>(f, nr);
    const auto cig = take<uint32_t>(f, (size_t)h[7]);
    const auto qn = take<uint8_t>(f, (size_t)h[5]);
    const auto qo = take<int64_t>(f, n + 1);
    const auto seq = take<uint8_t>(f, (size_t)h[3]);
    const auto qual = take<uint8_t>(f, h[8] ? (size_t)h[3] : 0);
    const auto seq_off = take<int64_t>(f, n + 1);
    const auto rep = take<int32_t>(f, n);
    const auto tn = take<uint8_t>(f, (size_t)h[6]);
    const auto to = take<int64_t>(f, nt + 1);
    const auto tseq = take<uint8_t>(f, (size_t)h[4]);
    const auto tseq_off = take<int64_t>(f, nt + 1);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "sam_main: cannot write %s\n", argv[2]); return 1; }
    for (int64_t k = 0; k < h[9]; ++k) {
        const gbx_mm_sam_params P = take<gbx_mm_sam_params>(f, 1)[0];
        const int lanes = take<int32_t>(f, 1)[0];
        std::vector<int64_t> line_off(n + 1);
        int64_t counts[2];
        auto run = [&](uint8_t *lines, int64_t cap) {
            return gbx_mm_sam_cpu_lanes(&P, lanes, (int64_t)n, regs.data(), reg_off.data(), alns.data(), cig.data(), h[7], qn.data(), qo.data(), seq.data(),
                                        h[8] ? qual.data() : nullptr, seq_off.data(), rep.data(), (int64_t)nt, tn.data(), to.data(), tseq.data(), tseq_off.data(),
                                        lines, cap, line_off.data(), counts);
        };
        const int64_t need = run(nullptr, 0);
        std::vector<uint8_t> text((size_t)need);
        const int64_t got = run(text.data(), need);
        if (got != need) { fprintf(stderr, "sam_main: the text's length changed (%lld, %lld)\n", (long long)need, (long long)got); return 3; }
        put(o, &need, 1); put(o, counts, 2); put(o, line_off.data(), n + 1); put(o, text.data(), (size_t)need);
    }
    fclose(f);
    if (fclose(o)) { fprintf(stderr, "sam_main: cannot write %s\n", argv[2]); return 1; }
    return 0;
}
