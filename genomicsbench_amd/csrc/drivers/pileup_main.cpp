// pileup_main.cpp — the pileup benchmark driver (R/benchmarks/pileup/medaka_counts.c:482-583) over gbx_pileup_layout_host
// and gbx_pileup_count_host.
//
// CLI as the reference: pileup <bam> <region> <num_threads> [dtype ...].  The region is cut into batches of 100 000
// positions whose region strings 'chr:i-min(i+100000,end)' (i 0-based) htslib parses again, so batch k covers
// [max(i - 1, 0), min(i + 100000, end)) and consecutive batches share one position.  Every column of a position depends
// only on the reads there, so the driver computes one layout over the union of the batches and counts each position once,
// in groups of batches; a batch is a slice of that.  num_homop is 5, as the reference's main sets it.
// Printed as the reference: "Running N batches with threads: T" and "Kernel runtime: X s" (stderr).  The runtime brackets
// what the reference's does: reading the BAM and counting every batch (not printing).
// Not reference flags: --print (every batch's print_pileup_data table and its "pileup is length N, with buffer of B
// columns" line, as a PRINT_OUTPUT build prints them; B replays the reference's buffer growth from the batch's columns),
// --parse-only (reads, bases and a CRC-32 of the reads; no GPU), --gpus N.  Exactly one dtype is refused as the
// reference's calculate_pileup refuses it (num_dtypes == 1 with dtypes set, medaka_counts.c:302-305).
// The BAM is read by bam_reader.h (zlib, no htslib, no .bai: the file is scanned).
#include <zlib.h>
#include "bam_reader.h"
#include "driver_common.h"

namespace {

constexpr int64_t BATCH = 100000;
constexpr int NUM_HOMOP = 5;
constexpr int64_t GROUP_POSITIONS = 1 << 21;     // positions counted per host call (bounds the host buffer)

// positions per group of batches: GROUP_POSITIONS, or GBX_PILEUP_GROUP_POSITIONS (a test aid: a small value makes every
// batch a group of its own, so the shared position is carried from group to group)
int64_t group_positions()
{
    const char *e = getenv("GBX_PILEUP_GROUP_POSITIONS");
    const long long v = e ? atoll(e) : 0;
    return v >= 1 ? v : GROUP_POSITIONS;
}
const char PLP_BASES[] = "acgtACGTdD";

struct Out {                                     // a growing stdout buffer with fast integer formatting
    std::vector<char> b;
    void put(const char *s, size_t n) { b.insert(b.end(), s, s + n); if (b.size() > (1 << 22)) flush(); }
    void puts(const char *s) { put(s, strlen(s)); }
    void num(uint64_t v, char tail)
    {
        char t[24];
        int n = 0;
        do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        char s[24];
        for (int k = 0; k < n; ++k) s[k] = t[n - 1 - k];
        s[n++] = tail;
        put(s, (size_t)n);
    }
    void flush() { if (!b.empty()) fwrite(b.data(), 1, b.size(), stdout); b.clear(); }
};

// buffer_cols of a batch [lo, hi) after calculate_pileup (medaka_counts.c:350,365-375), from its per-position columns
size_t replay_buffer_cols(const int64_t *pos_col, int64_t lo, int64_t hi)
{
    size_t buf = 2 * (size_t)(hi - lo);
    size_t n_cols = 0;
    for (int64_t q = lo; q < hi; ++q) {
        const int64_t c = pos_col[q + 1] - pos_col[q];
        if (c == 0) continue;
        const size_t max_ins = (size_t)(c - 1);
        ++n_cols;
        if (n_cols + max_ins > buf && q > lo) {      // (at the batch's first position the reference divides by zero)
            const float cols_per_pos = (float)(n_cols + max_ins) / (float)(q - lo);
            const int64_t grow = (int64_t)(int)cols_per_pos * (hi - lo);
            buf = max_ins + std::max<size_t>(2 * buf, (size_t)grow);
        }
        n_cols += max_ins;
    }
    return buf;
}

}  // namespace

int main(int argc, char **argv)
{
    const int gpus = take_gpus_flag(argc, argv);
    bool print = false, parse_only = false;
    std::vector<char *> pos_args;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--print")) print = true;
        else if (!strcmp(argv[i], "--parse-only")) parse_only = true;
        else pos_args.push_back(argv[i]);
    }
    if (pos_args.size() < 3) {
        fprintf(stderr, "Usage %s <bam> <region> <num_threads> [dtype ...] [--print] [--parse-only] [--gpus n]\n", argv[0]);
        return EXIT_FAILURE;
    }
    const char *bam_file = pos_args[0];
    const std::string reg = pos_args[1];
    const int threads = std::max(1, atoi(pos_args[2]));
    std::vector<std::string> dtypes;
    for (size_t k = 3; k < pos_args.size(); ++k) dtypes.push_back(pos_args[k]);
    const int num_dtypes = dtypes.empty() ? 1 : (int)dtypes.size();

    const double t0 = now_s();
    bam::File f;
    std::string err;
    if (!bam::open_bam(bam_file, threads, f, &err)) { fprintf(stderr, "Failed to read .bam file '%s': %s\n", bam_file, err.c_str()); return EXIT_FAILURE; }
    bam::Region R;
    if (!bam::parse_region(reg, f.contigs, &R, &err)) { fprintf(stderr, "%s\n", err.c_str()); return EXIT_FAILURE; }
    // the batches and the union of their ranges
    struct Batch { int64_t lo, hi; };
    std::vector<Batch> batches;
    for (int64_t i = R.beg; i < R.end; i += BATCH) batches.push_back(Batch{std::max<int64_t>(i - 1, 0), std::min(i + BATCH, R.end)});
    const int64_t L = batches.empty() ? R.beg : batches.front().lo, E = batches.empty() ? R.beg : R.end;
    bam::Region U = R;
    U.beg = L; U.end = E;
    bam::Reads rd;
    if (!bam::region_reads(f, U, dtypes, rd, &err)) { fprintf(stderr, "Failed to read .bam file '%s': %s\n", bam_file, err.c_str()); return EXIT_FAILURE; }
    f.data = std::vector<uint8_t>();
    const double t_read = now_s() - t0;
    const int64_t n_reads = (int64_t)rd.pos.size();
    if (parse_only) {
        uLong crc = crc32(0L, Z_NULL, 0);
        for (int64_t r = 0; r < n_reads; ++r) {
            uint8_t h[10];
            const int32_t p = rd.pos[(size_t)r];
            const uint32_t nc = (uint32_t)(rd.cigar_off[(size_t)r + 1] - rd.cigar_off[(size_t)r]);
            const int32_t l = (int32_t)(rd.seq_off[(size_t)r + 1] - rd.seq_off[(size_t)r]);
            memcpy(h, &p, 4); h[4] = rd.rev[(size_t)r]; h[5] = (uint8_t)rd.dtype[(size_t)r]; memcpy(h + 6, &nc, 4);
            crc = crc32(crc, h, 10);
            crc = crc32(crc, (const Bytef *)(rd.cigar.data() + rd.cigar_off[(size_t)r]), nc * 4);
            crc = crc32(crc, (const Bytef *)&l, 4);
            crc = crc32(crc, rd.seq.data() + rd.seq_boff[(size_t)r], (uInt)((l + 1) / 2));
            crc = crc32(crc, rd.qual.data() + rd.seq_off[(size_t)r], (uInt)l);
        }
        fprintf(stderr, "ingest: %lld reads, %lld bases, %.3f s with %d threads\n", (long long)n_reads, (long long)rd.seq_off.back(), t_read,
                threads);
        printf("{\"reads\": %lld, \"bases\": %lld, \"crc32\": \"%08lx\"}\n", (long long)n_reads, (long long)rd.seq_off.back(), (unsigned long)crc);
        return 0;
    }
    fprintf(stderr, "Running %zu batches with threads: %d\n", batches.size(), threads);
    // one dtype named on the command line: the reference's calculate_pileup gets num_dtypes == 1 with dtypes != NULL and
    // refuses it in its first batch (medaka_counts.c:302-305)
    if (dtypes.size() == 1 && !batches.empty()) {
        fprintf(stderr, "Recieved invalid num_dtypes and dtypes args.\n");
        return EXIT_FAILURE;
    }
    print_device_banner(gpus);
    double runtime = t_read;
    double t1 = now_s();
    gbx_pileup_reads gr;
    gr.n_reads = n_reads;
    gr.seq_bytes = (int64_t)rd.seq.size();
    gr.pos = rd.pos.data(); gr.cigar_off = rd.cigar_off.data(); gr.cigar = rd.cigar.data(); gr.seq_off = rd.seq_off.data();
    gr.seq_boff = rd.seq_boff.data(); gr.seq = rd.seq.data(); gr.qual = rd.qual.data(); gr.rev = rd.rev.data(); gr.dtype = rd.dtype.data();
    gbx_pileup_params p;
    memset(&p, 0, sizeof p);
    p.num_dtypes = num_dtypes; p.num_homop = NUM_HOMOP; p.start = L; p.end = E;
    const int F = GBX_PILEUP_FEATLEN * num_dtypes * NUM_HOMOP;
    std::vector<int64_t> pos_col((size_t)(E - L + 1), 0);
    gbx_pileup_layout_stats st;
    memset(&st, 0, sizeof st);
    st.bad_read = -1;
    const int lrc = gbx_pileup_layout_host(&p, &gr, pos_col.data(), &st);
    if (lrc == GBX_ERR_ARG && st.bad_read >= 0 && st.bad_read < n_reads) {
        fprintf(stderr, "Datatype not found for %s.\n", rd.names[(size_t)st.bad_read].c_str());
        return EXIT_FAILURE;
    }
    die_on(lrc, "gbx_pileup_layout_host");
    // the counted columns of positions [buf_lo, buf_hi), numbered from pos_col[buf_lo - L]
    std::vector<int32_t> major, minor;
    std::vector<uint32_t> counts;
    int64_t buf_lo = L, buf_hi = L;
    Out out;
    const std::string header = [&] {
        std::string h = "pos\tins\t";
        char t[64];
        if (num_dtypes > 1) {
            for (const std::string &d : dtypes)
                for (int j = 0; j < GBX_PILEUP_FEATLEN; ++j) { snprintf(t, sizeof t, "%s.%c\t", d.c_str(), PLP_BASES[j]); h += t; }
        } else {
            for (int k = 0; k < NUM_HOMOP; ++k)
                for (int j = 0; j < GBX_PILEUP_FEATLEN; ++j) { snprintf(t, sizeof t, "%c.%d\t", PLP_BASES[j], k + 1); h += t; }
        }
        return h + "depth\n";
    }();
    const int64_t group = group_positions();
    size_t b0 = 0;
    while (b0 < batches.size()) {
        size_t b1 = b0 + 1;
        while (b1 < batches.size() && batches[b1].hi - batches[b0].lo <= group) ++b1;
        // keep what the buffer holds of the group's first batch (the shared position), count the rest
        const int64_t g_lo = batches[b0].lo, g_hi = batches[b1 - 1].hi;
        const int64_t keep_lo = std::max(g_lo, buf_lo), keep_hi = std::max(keep_lo, std::min(buf_hi, g_hi));
        const int64_t kc0 = pos_col[(size_t)(keep_lo - L)] - pos_col[(size_t)(buf_lo - L)];
        const int64_t kc = pos_col[(size_t)(keep_hi - L)] - pos_col[(size_t)(keep_lo - L)];
        if (kc > 0) {
            memmove(major.data(), major.data() + kc0, (size_t)kc * 4);
            memmove(minor.data(), minor.data() + kc0, (size_t)kc * 4);
            memmove(counts.data(), counts.data() + kc0 * F, (size_t)kc * F * 4);
        }
        const int64_t c_lo = std::max(keep_hi, g_lo);
        const int64_t nc = pos_col[(size_t)(g_hi - L)] - pos_col[(size_t)(c_lo - L)];
        major.resize((size_t)(kc + nc)); minor.resize((size_t)(kc + nc)); counts.resize((size_t)(kc + nc) * F);
        die_on(gbx_pileup_count_host(&p, &gr, pos_col.data(), c_lo, g_hi, major.data() + kc, minor.data() + kc, counts.data() + kc * F),
               "gbx_pileup_count_host");
        buf_lo = keep_hi > keep_lo ? keep_lo : c_lo;
        buf_hi = g_hi;
        if (print) {
            runtime += now_s() - t1;
            for (size_t b = b0; b < b1; ++b) {
                out.puts(header.c_str());
                const int64_t base = pos_col[(size_t)(buf_lo - L)];
                const int64_t c0 = pos_col[(size_t)(batches[b].lo - L)] - base, c1 = pos_col[(size_t)(batches[b].hi - L)] - base;
                for (int64_t c = c0; c < c1; ++c) {
                    out.num((uint64_t)major[(size_t)c], '\t');
                    out.num((uint64_t)minor[(size_t)c], '\t');
                    int s = 0;
                    const uint32_t *row = counts.data() + c * F;
                    for (int j = 0; j < F; ++j) { out.num(row[j], '\t'); s += (int)row[j]; }
                    char t[32];
                    const int n = snprintf(t, sizeof t, "%d\n", s);
                    out.put(t, (size_t)n);
                }
                char t[128];
                const int n = snprintf(t, sizeof t, "pileup is length %lld, with buffer of %zu columns\n", (long long)(c1 - c0),
                                       replay_buffer_cols(pos_col.data(), batches[b].lo - L, batches[b].hi - L));
                out.put(t, (size_t)n);
            }
            out.flush();
            t1 = now_s();
        }
        b0 = b1;
    }
    runtime += now_s() - t1;
    out.flush();
    fflush(stdout);
    fprintf(stderr, "layout: %lld columns over %lld positions, max insertion %lld, max depth %lld, %lld aligned bases; BAM read %.3f s\n",
            (long long)st.n_cols, (long long)st.n_positions, (long long)st.max_ins, (long long)st.max_depth, (long long)st.aligned_bases, t_read);
    fprintf(stderr, "Kernel runtime: %.2f s\n", runtime);
    return 0;
}
