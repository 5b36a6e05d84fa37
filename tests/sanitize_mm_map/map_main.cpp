// map_main.cpp — the host twin of the stage behind the chain scores under ASan + UBSan, in a program of its own.
//   map_main <batch.bin> <out.bin> [min_chain_score min_cnt]
// batch.bin: int64 n_reads, n_anchors, then off[n_reads + 1], seq_off[n_reads + 1] (int64), ax, ay (uint64), f, p, v (int32),
// rep_len (int32), hash (uint32).  Every buffer is a heap block of exactly the size the entry names, so a write or read past
// one is reported.  out.bin: counts[2], chain_off, reg_off, u, regs, n_text, the PAF text (names read<i> / ref<i>, targets of
// 100 000 bases each).
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../genomicsbench_amd/csrc/shims/mm_map_cpu_twin.cpp"

namespace {
template <class T> std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "map_main: short input\n"); exit(2); }
    return v;
}
template <class T> void put(FILE *f, const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: map_main <batch.bin> <out.bin> [min_chain_score min_cnt]\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "map_main: cannot read %s\n", argv[1]); return 1; }
    const std::vector<int64_t> head = take<int64_t>(f, 2);
    const size_t n = (size_t)head[0], na = (size_t)head[1];
    const auto off = take<int64_t>(f, n + 1), seq_off = take<int64_t>(f, n + 1);
    const auto ax = take<uint64_t>(f, na), ay = take<uint64_t>(f, na);
    const auto sc = take<int32_t>(f, na), par = take<int32_t>(f, na), pk = take<int32_t>(f, na), rep = take<int32_t>(f, n);
    const auto hash = take<uint32_t>(f, n);
    fclose(f);
    gbx_mm_map_params P{3, 40, 0.5f, 0.8f, 5, 30};
    if (argc >= 5) { P.min_chain_score = atoi(argv[3]); P.min_cnt = atoi(argv[4]); }
    std::vector<int64_t> chain_off(n + 1), reg_off(n + 1), line_off(n + 1);
    std::vector<uint64_t> u(na), cax(na), cay(na);
    std::vector<int32_t> n_chained(n);
    std::vector<gbx_mm_reg> regs(na);
    int64_t counts[2];
    gbx_mm_map_cpu(&P, (int64_t)n, off.data(), ax.data(), ay.data(), sc.data(), par.data(), pk.data(), seq_off.data(), rep.data(), hash.data(),
                   chain_off.data(), u.data(), cax.data(), cay.data(), n_chained.data(), reg_off.data(), regs.data(), counts);
    std::string qn, tn;
    std::vector<int64_t> qo(1, 0), to(1, 0), tso(1, 0);
    for (size_t r = 0; r < n; ++r) { qn += "read" + std::to_string(r); qo.push_back((int64_t)qn.size()); }
    for (int t = 0; t < 2; ++t) { tn += "ref" + std::to_string(t); to.push_back((int64_t)tn.size()); tso.push_back(100000 * (t + 1)); }
    const uint8_t *qnp = (const uint8_t *)qn.data(), *tnp = (const uint8_t *)tn.data();
    // measured with no room at all, then written into exactly that much
    const int64_t need = gbx_mm_paf_cpu((int64_t)n, regs.data(), reg_off.data(), qnp, qo.data(), seq_off.data(), rep.data(), 2, tnp, to.data(), tso.data(),
                                        nullptr, 0, line_off.data());
    std::vector<uint8_t> text((size_t)need);
    const int64_t got = gbx_mm_paf_cpu((int64_t)n, regs.data(), reg_off.data(), qnp, qo.data(), seq_off.data(), rep.data(), 2, tnp, to.data(), tso.data(),
                                       text.data(), need, line_off.data());
    if (got != need) { fprintf(stderr, "map_main: the text's length changed (%lld, %lld)\n", (long long)need, (long long)got); return 3; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "map_main: cannot write %s\n", argv[2]); return 1; }
    put(o, counts, 2); put(o, chain_off.data(), n + 1); put(o, reg_off.data(), n + 1); put(o, u.data(), (size_t)counts[0]);
    put(o, regs.data(), (size_t)counts[1]); put(o, &need, 1); put(o, text.data(), (size_t)need);
    fclose(o);
    printf("map_main: %zu reads, %zu anchors, %lld chains, %lld regions, %lld bytes of text\n", n, na, (long long)counts[0], (long long)counts[1],
           (long long)need);
    return 0;
}
