// mmseed — minimap2's seeding stage on real sequence: a reference FASTA and long reads (FASTA / FASTQ) in, the chain benchmark's
// input file out (host_data_io.cpp:13-51: `n avg_qspan max_dist_x max_dist_y bw n_segs`, n lines `x y`, `EOR`), one call per
// read in read order, so that `chain -i` and the reference's chain driver run on anchors of real reads.
//   mmseed [options] <ref.fa> <reads.fa|fq>
//     -k INT  k-mer size (15)            -w INT  window (10)               -H  homopolymer-compressed k-mers
//     -f FLOAT  mid_occ_frac (2e-4)      --mid-occ INT  the threshold itself (0: from -f)
//     -g INT  max_gap (5000)             -r INT  bandwidth (500)           -o FILE  output (stdout)
// Minimizers, index and anchors are made on the device (gbx_mm_index_build_host, gbx_mm_seed_host); this file parses and prints.
#include "driver_common.h"
#include <algorithm>
#include "seq_reader.h"

namespace {

int usage(FILE *f, int rc)
{
    fprintf(f, "usage: mmseed [-k INT] [-w INT] [-H] [-f FLOAT] [--mid-occ INT] [-g INT] [-r INT] [-o calls.txt] <ref.fa> <reads.fa|fq>\n");
    return rc;
}

bool read_seqs(const char *path, std::vector<uint8_t> &text, std::vector<int64_t> &off)
{
    Reader rd;
    if (!rd.open(path, 1)) return false;
    off.assign(1, 0);
    Reader::Rec r;
    int rc;
    while ((rc = rd.next(r)) == 1) {
        for (size_t k = r.seq0; k < r.seq1; ++k) text.insert(text.end(), rd.line[k], rd.line[k] + rd.llen[k]);
        off.push_back((int64_t)text.size());
    }
    if (rc < 0) { fprintf(stderr, "%s: malformed record %zu\n", path, off.size()); return false; }
    return true;
}

bool int_arg(const char *s, int32_t *v)
{
    char *e = nullptr;
    const long x = strtol(s, &e, 10);
    if (e == s || *e || x < -2147483647L || x > 2147483647L) return false;
    *v = (int32_t)x;
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    gbx_mm_params p;
    gbx_mm_default_params(&p);
    const char *out_path = nullptr;
    std::vector<const char *> files;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        auto value = [&]() -> const char * { return i + 1 < argc ? argv[++i] : nullptr; };
        int32_t *ip = nullptr;
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) return usage(stdout, 0);
        else if (!strcmp(a, "-H")) p.is_hpc = 1;
        else if (!strcmp(a, "-k")) ip = &p.k;
        else if (!strcmp(a, "-w")) ip = &p.w;
        else if (!strcmp(a, "--mid-occ")) ip = &p.mid_occ;
        else if (!strcmp(a, "-g")) ip = &p.max_gap;
        else if (!strcmp(a, "-r")) ip = &p.bw;
        else if (!strcmp(a, "-f")) {
            const char *v = value();
            char *e = nullptr;
            if (!v || (p.mid_occ_frac = strtof(v, &e), e == v || *e)) { fprintf(stderr, "mmseed: -f takes a number\n"); return usage(stderr, 1); }
        }
        else if (!strcmp(a, "-o")) { if (!(out_path = value())) { fprintf(stderr, "mmseed: -o takes a file\n"); return usage(stderr, 1); } }
        else if (a[0] == '-' && a[1]) { fprintf(stderr, "mmseed: unknown option %s\n", a); return usage(stderr, 1); }
        else files.push_back(a);
        if (ip) {
            const char *v = value();
            if (!v || !int_arg(v, ip)) { fprintf(stderr, "mmseed: %s takes an integer\n", a); return usage(stderr, 1); }
        }
    }
    if (files.size() != 2) { fprintf(stderr, "mmseed: a reference and a read file\n"); return usage(stderr, 1); }
    if (gbx_mm_check_params(&p)) { fprintf(stderr, "mmseed: %s\n", gbx_last_error()); return 1; }

    std::vector<uint8_t> ref, reads;
    std::vector<int64_t> ref_off, read_off;
    if (!read_seqs(files[0], ref, ref_off) || !read_seqs(files[1], reads, read_off)) return 1;
    const int64_t n_ref = (int64_t)ref_off.size() - 1, n_reads = (int64_t)read_off.size() - 1;
    int64_t ref_max = 0;
    for (int64_t s = 0; s < n_ref; ++s) ref_max = std::max(ref_max, ref_off[s + 1] - ref_off[s]);

    const double t0 = now_s();
    const int64_t icap = std::max<int64_t>((int64_t)ref.size(), 1);
    std::vector<uint64_t> keys((size_t)icap), vals((size_t)icap);
    std::vector<int64_t> koff((size_t)icap + 1);
    gbx_mm_index_info info;
    if (gbx_mm_index_build_host(&p, n_ref, ref.data(), ref_off.data(), keys.data(), koff.data(), icap, vals.data(), icap, &info)) {
        fprintf(stderr, "mmseed: %s\n", gbx_last_error());
        return 1;
    }
    const double t1 = now_s();
    fprintf(stderr, "Index: %lld sequences, %lld bases, %lld minimizers of %lld keys, mid_occ %d (%.2f sec)\n", (long long)n_ref, (long long)ref.size(),
            (long long)info.n_vals, (long long)info.n_keys, info.mid_occ, t1 - t0);

    std::vector<int64_t> off((size_t)n_reads + 1);
    std::vector<gbx_chain_call> hdr((size_t)std::max<int64_t>(n_reads, 1));
    std::vector<int32_t> rep((size_t)std::max<int64_t>(n_reads, 1)), nm((size_t)std::max<int64_t>(n_reads, 1));
    std::vector<uint64_t> ax, ay;
    int64_t counts[2] = {0, 0};
    // sized by a first call without room for anchors, which reports the need
    int rc = gbx_mm_seed_host(&p, keys.data(), koff.data(), info.n_keys, vals.data(), info.mid_occ, n_ref, ref_max, n_reads, reads.data(), read_off.data(),
                              nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, off.data(), hdr.data(), rep.data(), nm.data(), counts);
    if (rc == GBX_ERR_ARG && counts[1] > 0) {
        ax.resize((size_t)counts[1]); ay.resize((size_t)counts[1]);
        rc = gbx_mm_seed_host(&p, keys.data(), koff.data(), info.n_keys, vals.data(), info.mid_occ, n_ref, ref_max, n_reads, reads.data(), read_off.data(),
                              nullptr, nullptr, 0, nullptr, ax.data(), ay.data(), counts[1], off.data(), hdr.data(), rep.data(), nm.data(), counts);
    }
    if (rc) { fprintf(stderr, "mmseed: %s\n", gbx_last_error()); return 1; }
    const double t2 = now_s();
    int64_t rep_total = 0;
    for (int64_t r = 0; r < n_reads; ++r) rep_total += rep[(size_t)r];
    fprintf(stderr, "Seeding: %lld reads, %lld bases, %lld minimizers, %lld anchors, rep_len %lld (%.2f sec)\n", (long long)n_reads, (long long)reads.size(),
            (long long)counts[0], (long long)counts[1], (long long)rep_total, t2 - t1);

    FILE *fo = out_path ? fopen(out_path, "w") : stdout;
    if (!fo) { fprintf(stderr, "mmseed: cannot write %s\n", out_path); return 1; }
    for (int64_t r = 0; r < n_reads; ++r) {
        const gbx_chain_call &h = hdr[(size_t)r];
        fprintf(fo, "%lld %.9g %d %d %d %d\n", (long long)(off[(size_t)r + 1] - off[(size_t)r]), (double)h.avg_qspan, h.max_dist_x, h.max_dist_y, h.bw, h.n_segs);
        for (int64_t i = off[(size_t)r]; i < off[(size_t)r + 1]; ++i) fprintf(fo, "%llu %llu\n", (unsigned long long)ax[(size_t)i], (unsigned long long)ay[(size_t)i]);
        fprintf(fo, "EOR\n");
    }
    if (fo != stdout && fclose(fo)) { fprintf(stderr, "mmseed: cannot write %s\n", out_path); return 1; }
    return 0;
}
