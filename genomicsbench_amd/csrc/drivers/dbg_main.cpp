// dbg_main.cpp — the dbg benchmark driver (R/benchmarks/dbg/debruijn.cpp:1437-1610) over gbx_dbg_windows and
// gbx_dbg_build_host.
//
// CLI as the reference: dbg <file.bam> <chr:start-stop> <ref.fa> <n_threads>; n_threads are the ingest threads (BGZF).
// Every record of the region in file order is a read (bam_reader.h region_records: no filter); a read the reference's getRead
// refuses (name over 99 characters, l_seq 0, first quality 0xFF, l_seq over 150, more than 16 CIGAR ops) ends the run with
// its message and status 1, as does the window rule's lo > hi.  Printed as the reference (stderr): "Found N batches. Running
// with threads: T" and "Kernel runtime: X s", which brackets graph building only, after BAM and FASTA ingest.
// Not reference flags: --print (one line per window: assem start and end, ref start, read range, the stats, the digest in
// hex), --parse-only (reads, longest and a CRC-32 of the reads; no GPU), --gpus N, and --assemble: gbx_dbg_assemble_host instead
// of the build (cycle check, retry at a larger k, variant paths; default gbx_dbg_asm_params), which prints one line per window:
// the final k, the builds, the cyclic flag, starts, paths and give-ups, and with --print behind it one line per path: P, the
// positions of its first and last node, its weight and its sequence.
// Deviations: the FASTA is read whole with no .fai (the reference's fai_load would write one); a bare contig name runs to
// the contig's length, not to INT_MAX.
#include <zlib.h>
#include "bam_reader.h"
#include "driver_common.h"

namespace {

const char NT16[] = "=ACMGRSVTWYHKDBN";

// the sequence of `name` in a plain FASTA, bytes as stored (line ends dropped); false when absent
bool fasta_contig(const char *path, const std::string &name, std::string &out)
{
    std::vector<char> buf;
    if (!slurp(path, buf)) return false;
    const size_t size = buf.size() - 1;          // (slurp ends the buffer with a NUL)
    bool in = false, found = false;
    for (size_t i = 0; i < size;) {
        size_t e = i;
        while (e < size && buf[e] != '\n') ++e;
        size_t le = e;
        if (le > i && buf[le - 1] == '\r') --le;
        if (le > i && buf[i] == '>') {
            if (in) break;
            size_t ne = i + 1;
            while (ne < le && buf[ne] != ' ' && buf[ne] != '\t') ++ne;
            in = std::string(buf.data() + i + 1, ne - i - 1) == name;
            found |= in;
        } else if (in) {
            out.append(buf.data() + i, le - i);
        }
        i = e + 1;
    }
    return found;
}

}  // namespace

int main(int argc, char **argv)
{
    const int gpus = take_gpus_flag(argc, argv);
    bool print = false, parse_only = false, assemble = false;
    std::vector<char *> pos_args;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--print")) print = true;
        else if (!strcmp(argv[i], "--parse-only")) parse_only = true;
        else if (!strcmp(argv[i], "--assemble")) assemble = true;
        else pos_args.push_back(argv[i]);
    }
    if (pos_args.size() != 4) {
        fprintf(stderr, "Usage %s file.bam chr:start-stop ref.fa n_threads [--print] [--parse-only] [--assemble] [--gpus n]\n", argv[0]);
        return EXIT_FAILURE;
    }
    const char *bam_file = pos_args[0], *fa_file = pos_args[2];
    const std::string reg = pos_args[1];
    const int threads = std::max(1, atoi(pos_args[3]));
    bam::File f;
    std::string err;
    if (!bam::open_bam(bam_file, threads, f, &err)) { fprintf(stderr, "Failed to read .bam file '%s': %s\n", bam_file, err.c_str()); return EXIT_FAILURE; }
    bam::Region R;
    if (!bam::parse_region(reg, f.contigs, &R, &err)) { fprintf(stderr, "%s\n", err.c_str()); return EXIT_FAILURE; }
    std::vector<bam::Record> recs;
    if (!bam::region_records(f, R, recs, &err)) { fprintf(stderr, "Failed to read .bam file '%s': %s\n", bam_file, err.c_str()); return EXIT_FAILURE; }
    // getRead (common.cpp:24-138): the refusals in its order, then the ASCII bases, the clip-adjusted uint32 pos, bam_endpos
    const int64_t n = (int64_t)recs.size();
    std::vector<int64_t> seq_off(1, 0);
    std::vector<uint8_t> seq, qual;
    std::vector<uint16_t> flag;
    std::vector<uint32_t> pos, endp;
    for (const bam::Record &r : recs) {
        const int name_len = (int)strnlen(r.name, (size_t)r.l_name);      // strlen(qname): htslib pads names with NULs
        if (name_len + 1 > 100) { fprintf(stderr, "The maximum read name length is set to %d, but the actual read length is %d\n", 100, name_len + 1); return EXIT_FAILURE; }
        if (r.l_seq == 0) { fprintf(stderr, "The sequence length is 0. How come?\n"); return EXIT_FAILURE; }
        if (r.qual[0] == 0xff) { fprintf(stderr, "The quality score is 255 for the first base. How come?\n"); return EXIT_FAILURE; }
        if (r.l_seq + 1 > 151) { fprintf(stderr, "The maximum read length is set to %d, but the actual read length is %d\n", 151, (int)r.l_seq + 1); return EXIT_FAILURE; }
        if (r.n_cigar > 16) { fprintf(stderr, "The maximum number of cigar is set to %d, but the actual number of cigar is %d\n", 16, r.n_cigar); return EXIT_FAILURE; }
        for (int64_t i = 0; i < r.l_seq; ++i) seq.push_back((uint8_t)NT16[(r.seq[i >> 1] >> ((~i & 1) << 2)) & 15]);
        qual.insert(qual.end(), r.qual, r.qual + r.l_seq);
        seq_off.push_back((int64_t)seq.size());
        flag.push_back(r.flag);
        uint32_t p = (uint32_t)r.pos;
        if (r.n_cigar > 0 && (bam::rdu32(r.cigar) & 15u) == 4) p -= bam::rdu32(r.cigar) >> 4;
        pos.push_back(p);
        endp.push_back((uint32_t)r.endpos);
    }
    f.data = std::vector<uint8_t>();
    gbx_dbg_reads rd;
    rd.n_reads = n; rd.seq_bytes = (int64_t)seq.size();
    rd.seq_off = seq_off.data(); rd.seq = seq.data(); rd.qual = qual.data(); rd.flag = flag.data(); rd.pos = pos.data(); rd.end = endp.data();
    if (parse_only) {
        int32_t longest = 0;
        uLong crc = crc32(0L, Z_NULL, 0);
        for (int64_t r = 0; r < n; ++r) {
            longest = std::max(longest, (int32_t)(endp[(size_t)r] - pos[(size_t)r]));
            const int32_t l = (int32_t)(seq_off[(size_t)r + 1] - seq_off[(size_t)r]);
            crc = crc32(crc, (const Bytef *)&pos[(size_t)r], 4);
            crc = crc32(crc, (const Bytef *)&endp[(size_t)r], 4);
            crc = crc32(crc, (const Bytef *)&flag[(size_t)r], 2);
            crc = crc32(crc, (const Bytef *)&l, 4);
            crc = crc32(crc, seq.data() + seq_off[(size_t)r], (uInt)l);
            crc = crc32(crc, qual.data() + seq_off[(size_t)r], (uInt)l);
        }
        printf("{\"reads\": %lld, \"bases\": %lld, \"longest\": %d, \"crc32\": \"%08lx\"}\n", (long long)n, (long long)seq.size(), longest,
               (unsigned long)crc);
        return 0;
    }
    std::string contig;
    if (!fasta_contig(fa_file, R.contig, contig)) { fprintf(stderr, "Failed to fetch '%s' from '%s'\n", R.contig.c_str(), fa_file); return EXIT_FAILURE; }
    gbx_dbg_params p;
    gbx_dbg_default_params(&p);
    int64_t nw = 0;
    const int rc0 = gbx_dbg_windows(&p, &rd, R.beg, R.end, 0, &nw, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc0 && rc0 != GBX_ERR_ARG) die_on(rc0, "gbx_dbg_windows");
    std::vector<int64_t> a0((size_t)nw + 1), a1((size_t)nw + 1), f0((size_t)nw + 1), f1((size_t)nw + 1), lo((size_t)nw + 1), hi((size_t)nw + 1);
    const int rc = gbx_dbg_windows(&p, &rd, R.beg, R.end, nw, &nw, a0.data(), a1.data(), f0.data(), f1.data(), lo.data(), hi.data());
    if (rc == GBX_ERR_ARG && nw > 0) {          // setWindowPointers' fatal error (common.cpp:210-214)
        const size_t w = (size_t)nw - 1;
        fprintf(stderr, "Start pos = %d. End pos = %d. Read start pos = %d. end pos = %d\n", (int)a0[w], (int)a1[w], (int)lo[w], (int)hi[w]);
        fprintf(stderr, "There are %d reads here. This should never happen. Read start pointer > read end pointer!!\n", (int)n);
        return EXIT_FAILURE;
    }
    die_on(rc, "gbx_dbg_windows");
    // faidx_fetch_seq(refStart, refEnd - 1): the end clamped to the contig (UPSTREAM)
    std::vector<int64_t> ref_off(1, 0);
    std::string ref;
    for (int64_t w = 0; w < nw; ++w) {
        const int64_t s = f0[(size_t)w], e = std::min<int64_t>(f1[(size_t)w], (int64_t)contig.size());
        if (e > s) ref.append(contig, (size_t)s, (size_t)(e - s));
        ref_off.push_back((int64_t)ref.size());
    }
    gbx_dbg_wins wn;
    wn.n_win = nw; wn.ref_bytes = (int64_t)ref.size();
    wn.ref_off = ref_off.data(); wn.ref = (const uint8_t *)ref.data(); wn.ref_pos = f0.data(); wn.read_lo = lo.data(); wn.read_hi = hi.data();
    fprintf(stderr, "Found %lld batches. Running with threads: %d\n", (long long)nw, threads);
    print_device_banner(gpus);
    std::vector<gbx_dbg_stats> st((size_t)std::max<int64_t>(nw, 1));
    if (assemble) {
        gbx_dbg_asm_params ap;
        gbx_dbg_asm_default_params(&ap);
        std::vector<gbx_dbg_asm_win> aw((size_t)std::max<int64_t>(nw, 1));
        std::vector<gbx_dbg_asm_start> starts(1024);
        std::vector<gbx_dbg_asm_path> paths(1024);
        std::vector<int32_t> pnodes(1 << 16);
        std::vector<uint8_t> pseq(1 << 16);
        int64_t totals[3] = {0, 0, 0};
        const double t0 = now_s();
        for (int attempt = 0;; ++attempt) {          // a short capacity: the totals say what to allocate (the starts first)
            gbx_dbg_asm_out o;
            o.stats = st.data(); o.wins = aw.data(); o.starts = starts.data(); o.paths = paths.data(); o.path_nodes = pnodes.data(); o.path_seq = pseq.data();
            o.cap_starts = (int64_t)starts.size(); o.cap_paths = (int64_t)paths.size(); o.cap_path_nodes = (int64_t)pnodes.size(); o.totals = totals;
            const int arc = gbx_dbg_assemble_host(&p, &ap, &rd, &wn, &o);
            const bool is_short = totals[0] > o.cap_starts || totals[1] > o.cap_paths || totals[2] > o.cap_path_nodes;
            if (arc == GBX_ERR_UNSUPPORTED && is_short && attempt < 3) {
                starts.resize((size_t)std::max(totals[0], o.cap_starts));
                paths.resize((size_t)std::max(totals[1], o.cap_paths));
                pnodes.resize((size_t)std::max(totals[2], o.cap_path_nodes));
                pseq.resize(pnodes.size());
                continue;
            }
            die_on(arc, "gbx_dbg_assemble_host");
            break;
        }
        const double runtime = now_s() - t0;
        std::string out;
        char line[160];
        for (int64_t w = 0; w < nw; ++w) {
            const gbx_dbg_asm_win &a = aw[(size_t)w];
            out.append(line, (size_t)snprintf(line, sizeof line, "%d\t%d\t%d\t%lld\t%lld\t%lld\n", a.k, a.n_builds, a.cyclic, (long long)a.n_starts,
                                              (long long)a.n_paths, (long long)a.n_gave_up));
            for (int64_t s = a.first_start; print && s < a.first_start + a.n_starts; ++s)
                for (int64_t x = starts[(size_t)s].first_path; x < starts[(size_t)s].first_path + starts[(size_t)s].n_paths; ++x) {
                    const gbx_dbg_asm_path &pa = paths[(size_t)x];
                    out.append(line, (size_t)snprintf(line, sizeof line, "P\t%d\t%d\t%lld\t", pa.pos_first, pa.pos_last, (long long)pa.weight));
                    out.append((const char *)pseq.data() + pa.first_node, (size_t)pa.n_nodes);
                    out.push_back('\n');
                }
        }
        fwrite(out.data(), 1, out.size(), stdout);
        fflush(stdout);
        fprintf(stderr, "Kernel runtime: %.2f s\n", runtime);
        return 0;
    }
    const double t0 = now_s();
    die_on(gbx_dbg_build_host(&p, &rd, &wn, st.data()), "gbx_dbg_build_host");
    const double runtime = now_s() - t0;
    if (print) {
        std::string out;
        char line[320];
        for (int64_t w = 0; w < nw; ++w) {
            const gbx_dbg_stats &s = st[(size_t)w];
            const int k = snprintf(line, sizeof line, "%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%016llx\n",
                                   (long long)a0[(size_t)w], (long long)a1[(size_t)w], (long long)f0[(size_t)w], (long long)lo[(size_t)w],
                                   (long long)hi[(size_t)w], (long long)s.n_nodes, (long long)s.n_edges, (long long)s.n_dropped, (long long)s.n_occ,
                                   (long long)s.weight_sum, (long long)s.n_ref, (long long)s.n_read, (long long)s.n_both, (unsigned long long)s.digest);
            out.append(line, (size_t)k);
        }
        fwrite(out.data(), 1, out.size(), stdout);
        fflush(stdout);
    }
    fprintf(stderr, "Kernel runtime: %.2f s\n", runtime);
    return 0;
}
