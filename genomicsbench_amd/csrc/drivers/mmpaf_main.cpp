// mmpaf — long reads to PAF or SAM, as `minimap2 -x map-ont` prints it: without -c approximate mappings, with -c the base-level
// alignment of every mapping (CIGAR in cg:Z:, NM, ms, AS, nn), with -a SAM records.  A reference FASTA and reads (FASTA / FASTQ)
// in, one PAF line per mapping or one SAM record per alignment out.
//   mmpaf [options] <ref.fa> <reads.fa|fq> > out.paf
//     -k INT  k-mer size (15)            -w INT  window (10)               -H  homopolymer-compressed k-mers
//     -f FLOAT  mid_occ_frac (2e-4)      --mid-occ INT  the threshold itself (0: from -f)
//     -g INT  max_gap (5000)             -r INT  bandwidth (500)
//     -n INT  min_cnt (3)                -m INT  min_chain_score (40)      -M FLOAT  mask_level (0.5)
//     -p FLOAT  pri_ratio (0.8)          -N INT  best_n (5)                -o FILE  output (stdout)
//     -c  base-level alignment; with it: -A INT match (2)  -B INT mismatch (4)  -O INT,INT gap open (4,24)  -E INT,INT gap
//         extension (2,1)  -z INT z-drop (400)  --end-bonus INT (0)  --min-ksw-len INT (200)  --max-ext INT (5000); -r is its band too
//         all reads are aligned in one call, which takes about 2 (r + 1) bytes of device memory a read base: split a read file
//         that does not fit
//     -a  SAM output (implies -c): a header (@HD, one @SQ a contig, @PG) and one record per aligned mapping, unmapped reads with
//         flag 4, the FASTQ qualities handed through;  -Y  soft clips on supplementary and secondary records
//     --cs[=short|long]  the cs:Z: tag    --MD  the MD:Z: tag    --eqx  = / X in place of M  (each needs -c or -a)
// Index, seeds, chain scores, chains, regions, mapq, alignments and the text are all made on the device (gbx_mm_index_build_host,
// gbx_mm_seed_host, gbx_chain_host, gbx_mm_map_host, gbx_mm_align_host, gbx_mm_paf_host / gbx_mm_paf_cigar_host / gbx_mm_sam_host);
// this file parses, hashes the read names and prints.
#include "driver_common.h"
#include <algorithm>
#include "seq_reader.h"

namespace {

int usage(FILE *f, int rc)
{
    fprintf(f, "usage: mmpaf [-k INT] [-w INT] [-H] [-f FLOAT] [--mid-occ INT] [-g INT] [-r INT] [-n INT] [-m INT] [-M FLOAT] [-p FLOAT] [-N INT]\n"
               "             [-c [-A INT] [-B INT] [-O INT,INT] [-E INT,INT] [-z INT] [--end-bonus INT] [--min-ksw-len INT] [--max-ext INT]]\n"
               "             [-a [-Y]] [--cs[=short|long]] [--MD] [--eqx]\n"
               "             [-o out.paf] <ref.fa> <reads.fa|fq>\n");
    return rc;
}

struct Seqs {
    std::vector<uint8_t> text, names, qual;            // qual: on the offsets of text, when every record brought qualities
    std::vector<int64_t> off, name_off;
    int64_t n() const { return (int64_t)off.size() - 1; }
};

// sequences and their names (the header up to the first blank)
bool read_seqs(const char *path, Seqs &s)
{
    Reader rd;
    if (!rd.open(path, 1)) return false;
    s.off.assign(1, 0);
    s.name_off.assign(1, 0);
    Reader::Rec r;
    int rc;
    while ((rc = rd.next(r)) == 1) {
        for (size_t k = r.seq0; k < r.seq1; ++k) s.text.insert(s.text.end(), rd.line[k], rd.line[k] + rd.llen[k]);
        if (r.qual) s.qual.insert(s.qual.end(), r.qual, r.qual + r.len);
        s.off.push_back((int64_t)s.text.size());
        int len = 0;
        while (len < r.head_len && r.head[len] != ' ' && r.head[len] != '\t') ++len;
        s.names.insert(s.names.end(), r.head, r.head + len);
        s.name_off.push_back((int64_t)s.names.size());
    }
    if (rc < 0) { fprintf(stderr, "%s: malformed record %zu\n", path, s.off.size()); return false; }
    if (s.qual.size() != s.text.size()) s.qual.clear();
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

// "INT,INT"
bool pair_arg(const char *s, int32_t *a, int32_t *b)
{
    const char *c = strchr(s, ',');
    if (!c) return false;
    const std::string first(s, c);
    return int_arg(first.c_str(), a) && int_arg(c + 1, b);
}

uint32_t wang(uint32_t key)
{
    key += ~(key << 15); key ^= key >> 10; key += key << 3; key ^= key >> 6; key += ~(key << 11); key ^= key >> 16;
    return key;
}

// X31(name) ^ (W(qlen) + W(11)): what minimap2 seeds a read's region hashes with
uint32_t read_hash(const uint8_t *name, int64_t len, int64_t qlen)
{
    uint32_t h = len > 0 ? name[0] : 0;
    for (int64_t i = 1; i < len; ++i) h = (h << 5) - h + name[i];
    return h ^ (wang((uint32_t)qlen) + wang(11u));
}

int fail() { fprintf(stderr, "mmpaf: %s\n", gbx_last_error()); return 1; }

}  // namespace

int main(int argc, char **argv)
{
    gbx_mm_params p;
    gbx_mm_map_params mp;
    gbx_mm_default_params(&p);
    gbx_mm_map_default_params(&mp);
    gbx_mm_align_params ap;
    gbx_mm_align_default_params(&ap);
    gbx_mm_sam_params sp;
    gbx_mm_sam_default_params(&sp);
    bool cigar = false;
    const char *align_opt = nullptr;                                   // the first option that only means something with -c
    const char *tag_opt = nullptr;                                     // the first option that needs -c or -a
    const char *out_path = nullptr;
    std::vector<const char *> files;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        auto value = [&]() -> const char * { return i + 1 < argc ? argv[++i] : nullptr; };
        int32_t *ip = nullptr;
        float *fp = nullptr;
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) return usage(stdout, 0);
        else if (!strcmp(a, "-H")) p.is_hpc = 1;
        else if (!strcmp(a, "-k")) ip = &p.k;
        else if (!strcmp(a, "-w")) ip = &p.w;
        else if (!strcmp(a, "--mid-occ")) ip = &p.mid_occ;
        else if (!strcmp(a, "-g")) ip = &p.max_gap;
        else if (!strcmp(a, "-r")) ip = &p.bw;
        else if (!strcmp(a, "-n")) ip = &mp.min_cnt;
        else if (!strcmp(a, "-m")) ip = &mp.min_chain_score;
        else if (!strcmp(a, "-N")) ip = &mp.best_n;
        else if (!strcmp(a, "-f")) fp = &p.mid_occ_frac;
        else if (!strcmp(a, "-M")) fp = &mp.mask_level;
        else if (!strcmp(a, "-p")) fp = &mp.pri_ratio;
        else if (!strcmp(a, "-c")) cigar = true;
        else if (!strcmp(a, "-a")) { sp.format = 1; cigar = true; }
        else if (!strcmp(a, "-Y")) sp.softclip = 1;
        else if (!strcmp(a, "--cs") || !strcmp(a, "--cs=short")) { sp.cs = 1; if (!tag_opt) tag_opt = a; }
        else if (!strcmp(a, "--cs=long")) { sp.cs = 2; if (!tag_opt) tag_opt = a; }
        else if (!strncmp(a, "--cs=", 5)) { fprintf(stderr, "mmpaf: --cs takes short or long\n"); return usage(stderr, 1); }
        else if (!strcmp(a, "--MD")) { sp.md = 1; if (!tag_opt) tag_opt = a; }
        else if (!strcmp(a, "--eqx")) { sp.eqx = 1; if (!tag_opt) tag_opt = a; }
        else if (!strcmp(a, "-A")) ip = &ap.a;
        else if (!strcmp(a, "-B")) ip = &ap.b;
        else if (!strcmp(a, "-z")) ip = &ap.zdrop;
        else if (!strcmp(a, "--end-bonus")) ip = &ap.end_bonus;
        else if (!strcmp(a, "--min-ksw-len")) ip = &ap.min_ksw_len;
        else if (!strcmp(a, "--max-ext")) ip = &ap.max_ext;
        else if (!strcmp(a, "-O") || !strcmp(a, "-E")) {
            const char *v = value();
            const bool open = a[1] == 'O';
            if (!v || !pair_arg(v, open ? &ap.q : &ap.e, open ? &ap.q2 : &ap.e2)) { fprintf(stderr, "mmpaf: %s takes two integers (INT,INT)\n", a); return usage(stderr, 1); }
            if (!align_opt) align_opt = a;
        }
        else if (!strcmp(a, "-o")) { if (!(out_path = value())) { fprintf(stderr, "mmpaf: -o takes a file\n"); return usage(stderr, 1); } }
        else if (a[0] == '-' && a[1]) { fprintf(stderr, "mmpaf: unknown option %s\n", a); return usage(stderr, 1); }
        else files.push_back(a);
        if (ip && !align_opt && (const char *)ip >= (const char *)&ap && (const char *)ip < (const char *)(&ap + 1)) align_opt = a;
        if (ip) {
            const char *v = value();
            if (!v || !int_arg(v, ip)) { fprintf(stderr, "mmpaf: %s takes an integer\n", a); return usage(stderr, 1); }
        }
        if (fp) {
            const char *v = value();
            char *e = nullptr;
            if (!v || (*fp = strtof(v, &e), e == v || *e)) { fprintf(stderr, "mmpaf: %s takes a number\n", a); return usage(stderr, 1); }
        }
    }
    if (files.size() != 2) { fprintf(stderr, "mmpaf: a reference and a read file\n"); return usage(stderr, 1); }
    if (align_opt && !cigar) { fprintf(stderr, "mmpaf: %s needs -c\n", align_opt); return usage(stderr, 1); }
    if (tag_opt && !cigar) { fprintf(stderr, "mmpaf: %s needs -c or -a\n", tag_opt); return usage(stderr, 1); }
    if (sp.softclip && !sp.format) { fprintf(stderr, "mmpaf: -Y needs -a\n"); return usage(stderr, 1); }
    const bool sam_stage = sp.format || sp.cs || sp.md || sp.eqx;      // without a new option the text comes from the entries it came from before
    ap.bw = p.bw;
    if (gbx_mm_check_params(&p) || gbx_mm_map_check_params(&mp) || (cigar && gbx_mm_align_check_params(&ap))) return fail();
    mp.min_diff = 2 * p.k;

    Seqs ref, rd;
    if (!read_seqs(files[0], ref) || !read_seqs(files[1], rd)) return 1;
    const int64_t n_ref = ref.n(), n_reads = rd.n();
    int64_t ref_max = 0;
    for (int64_t s = 0; s < n_ref; ++s) ref_max = std::max(ref_max, ref.off[s + 1] - ref.off[s]);

    const double t0 = now_s();
    const int64_t icap = std::max<int64_t>((int64_t)ref.text.size(), 1);
    std::vector<uint64_t> keys((size_t)icap), vals((size_t)icap);
    std::vector<int64_t> koff((size_t)icap + 1);
    gbx_mm_index_info info;
    if (gbx_mm_index_build_host(&p, n_ref, ref.text.data(), ref.off.data(), keys.data(), koff.data(), icap, vals.data(), icap, &info)) return fail();
    const double t1 = now_s();
    fprintf(stderr, "Index: %lld sequences, %lld bases, %lld minimizers, mid_occ %d (%.2f sec)\n", (long long)n_ref, (long long)ref.text.size(),
            (long long)info.n_vals, info.mid_occ, t1 - t0);

    const size_t nr = (size_t)std::max<int64_t>(n_reads, 1);
    std::vector<int64_t> off((size_t)n_reads + 1), chain_off((size_t)n_reads + 1), reg_off((size_t)n_reads + 1), line_off((size_t)n_reads + 1);
    std::vector<gbx_chain_call> hdr(nr);
    std::vector<int32_t> rep(nr), nm(nr), n_chained(nr);
    std::vector<uint64_t> ax, ay;
    int64_t counts[2] = {0, 0};
    // sized by a first call without room for anchors, which reports the need
    int rc = gbx_mm_seed_host(&p, keys.data(), koff.data(), info.n_keys, vals.data(), info.mid_occ, n_ref, ref_max, n_reads, rd.text.data(), rd.off.data(),
                              nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, off.data(), hdr.data(), rep.data(), nm.data(), counts);
    if (rc == GBX_ERR_ARG && counts[1] > 0) {
        ax.resize((size_t)counts[1]); ay.resize((size_t)counts[1]);
        rc = gbx_mm_seed_host(&p, keys.data(), koff.data(), info.n_keys, vals.data(), info.mid_occ, n_ref, ref_max, n_reads, rd.text.data(), rd.off.data(),
                              nullptr, nullptr, 0, nullptr, ax.data(), ay.data(), counts[1], off.data(), hdr.data(), rep.data(), nm.data(), counts);
    }
    if (rc) return fail();
    const int64_t na = counts[1];
    const double t2 = now_s();
    std::vector<int32_t> score((size_t)na), parent((size_t)na), peak((size_t)na);
    if (na && gbx_chain_host(n_reads, off.data(), ax.data(), ay.data(), hdr.data(), score.data(), parent.data(), nullptr, peak.data())) return fail();
    const double t3 = now_s();

    std::vector<uint32_t> hash(nr);
    for (int64_t r = 0; r < n_reads; ++r)
        hash[(size_t)r] = read_hash(rd.names.data() + rd.name_off[(size_t)r], rd.name_off[(size_t)r + 1] - rd.name_off[(size_t)r], rd.off[(size_t)r + 1] - rd.off[(size_t)r]);
    // a kept chain has min_cnt anchors of its own
    const int64_t ccap = std::max<int64_t>(na / mp.min_cnt, 1);
    std::vector<uint64_t> u((size_t)ccap), cax((size_t)std::max<int64_t>(na, 1)), cay((size_t)std::max<int64_t>(na, 1));
    std::vector<gbx_mm_reg> regs((size_t)ccap);
    int64_t mc[2] = {0, 0};
    if (gbx_mm_map_host(&mp, n_reads, off.data(), ax.data(), ay.data(), score.data(), parent.data(), peak.data(), rd.off.data(), rep.data(), hash.data(),
                        chain_off.data(), u.data(), ccap, cax.data(), cay.data(), n_chained.data(), reg_off.data(), regs.data(), ccap, mc))
        return fail();
    const double t4 = now_s();
    std::vector<uint8_t> text;
    int64_t n_text = 0;
    std::vector<gbx_mm_aln> alns((size_t)std::max<int64_t>(mc[1], 1));
    std::vector<uint32_t> cig;
    int64_t ac[3] = {0, 0, 0};
    if (cigar) {
        // z is sized by a call without room, which plans and reports the need but runs no job; the words by their bound: a
        // region's CIGAR has at most 2 qlen + 1 (every M or I run takes a query base, D runs lie between them).  One call aligns
        // every read: the z room (about 2 (bw + 1) bytes a read base) has to fit the device.
        auto align = [&](int64_t cigar_cap, int64_t z_bytes) {
            return gbx_mm_align_host(&ap, n_reads, regs.data(), reg_off.data(), off.data(), cax.data(), cay.data(), n_chained.data(), rd.text.data(),
                                     rd.off.data(), n_ref, ref.text.data(), ref.off.data(), alns.data(), cig.data(), cigar_cap, z_bytes, ac);
        };
        int64_t wcap = 0;
        for (int64_t r = 0; r < n_reads; ++r) wcap += (reg_off[(size_t)r + 1] - reg_off[(size_t)r]) * (2 * (rd.off[(size_t)r + 1] - rd.off[(size_t)r]) + 1);
        rc = align(0, 0);
        if (rc == GBX_ERR_ARG && ac[2] > 0) { cig.resize((size_t)wcap); rc = align(wcap, ac[2]); }
        if (rc) return fail();
    }
    const double t4a = now_s();
    int64_t sc[2] = {0, 0};
    auto paf = [&](uint8_t *lines, int64_t cap) {
        if (sam_stage)
            return gbx_mm_sam_host(&sp, n_reads, regs.data(), reg_off.data(), alns.data(), cig.data(), ac[1], rd.names.data(), rd.name_off.data(), rd.text.data(),
                                   rd.qual.empty() ? nullptr : rd.qual.data(), rd.off.data(), rep.data(), n_ref, ref.names.data(), ref.name_off.data(),
                                   ref.text.data(), ref.off.data(), lines, cap, line_off.data(), &n_text, sc);
        return cigar ? gbx_mm_paf_cigar_host(n_reads, regs.data(), reg_off.data(), alns.data(), cig.data(), ac[1], rd.names.data(), rd.name_off.data(),
                                             rd.off.data(), rep.data(), n_ref, ref.names.data(), ref.name_off.data(), ref.off.data(), lines, cap,
                                             line_off.data(), &n_text)
                     : gbx_mm_paf_host(n_reads, regs.data(), reg_off.data(), rd.names.data(), rd.name_off.data(), rd.off.data(), rep.data(), n_ref,
                                       ref.names.data(), ref.name_off.data(), ref.off.data(), lines, cap, line_off.data(), &n_text);
    };
    rc = paf(nullptr, 0);
    if (rc == GBX_ERR_ARG && n_text > 0) {
        text.resize((size_t)n_text);
        rc = paf(text.data(), n_text);
    }
    if (rc) return fail();
    const double t5 = now_s();
    if (cigar)
        fprintf(stderr, "Alignment: %lld jobs, %lld CIGAR words, %lld bytes of DP room (%.2f sec)\n", (long long)ac[0], (long long)ac[1], (long long)ac[2], t4a - t4);
    fprintf(stderr, "Mapping: %lld reads, %lld anchors, %lld chains, %lld mappings, %lld bytes (seeding %.2f, chain %.2f, map %.2f, text %.2f sec)\n",
            (long long)n_reads, (long long)na, (long long)mc[0], (long long)mc[1], (long long)n_text, t2 - t1, t3 - t2, t4 - t3, t5 - t4a);

    FILE *fo = out_path ? fopen(out_path, "w") : stdout;
    if (!fo) { fprintf(stderr, "mmpaf: cannot write %s\n", out_path); return 1; }
    if (sp.format) {
        fprintf(fo, "@HD\tVN:1.6\tSO:unsorted\tGO:query\n");
        for (int64_t s = 0; s < n_ref; ++s)
            fprintf(fo, "@SQ\tSN:%.*s\tLN:%lld\n", (int)(ref.name_off[(size_t)s + 1] - ref.name_off[(size_t)s]), (const char *)ref.names.data() + ref.name_off[(size_t)s],
                    (long long)(ref.off[(size_t)s + 1] - ref.off[(size_t)s]));
        fprintf(fo, "@PG\tID:mmpaf\tPN:mmpaf\tCL:mmpaf");
        for (int i = 1; i < argc; ++i) fprintf(fo, " %s", argv[i]);
        fprintf(fo, "\n");
    }
    if (n_text && fwrite(text.data(), 1, (size_t)n_text, fo) != (size_t)n_text) { fprintf(stderr, "mmpaf: cannot write the output\n"); return 1; }
    if (fo != stdout && fclose(fo)) { fprintf(stderr, "mmpaf: cannot write %s\n", out_path); return 1; }
    return 0;
}
