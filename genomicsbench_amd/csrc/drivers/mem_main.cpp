// mem — GPU driver with the command line of `bwa mem`:  mem [options] <idxprefix> <in1.fq> [in2.fq]
//                                                       mem index [-p prefix] [--parse-only] <in.fa>
// over gbx_mem_index / gbx_mem_aligner (include/gbx.h): reads in, SAM (the @SQ lines, then the records) on stdout or -o FILE.
//
// Index files, all UNPINNED (bwa-mem2 cannot be built or run here; the layouts are the published ones):
//   <prefix>.bwt.2bit.64  the FM index with REAL suffix-array samples (fmi_index_io.h has the layout)
//   <prefix>.ann          first line "l_pac n_seqs seed"; then per contig a line "gi name [comment]" and a line "offset len n_ambs"
//   <prefix>.0123         when present: 2 l_pac bytes of codes 0..3, the forward strand then its reverse complement; another
//                         size is refused
//   <prefix>.pac          otherwise: 2 bits per base, the first base in the top bits of a byte: base l = pac[l >> 2] >>
//                         ((~l & 3) << 1) & 3; the reverse-complement half is derived from it
//   <prefix>.amb          is NOT read: the holes of the reference align as the bases bwa put there
// `mem index` writes all five files from a FASTA (ref_files.h has the rules; the prefix defaults to the FASTA's path): .ann, .amb,
// .pac and .0123 on the host, .bwt.2bit.64 with sa_compx 3 through gbx_fmi_build_host (the suffix array, the BWT, the checkpoints
// and the samples are built on the GPU).  Parity UNPINNED, as for every index file.  --parse-only writes the four host files,
// prints "l_pac=.. contigs=.. holes=.. text_checksum=.." with a line per contig, and needs no GPU.  The other options of
// `bwa index` (-a, -b, -6) are refused by name.  Errors (an empty file, a sequence line before any header, a contig with no
// bases, a reference above 2147483647 bases) exit 1 with one line.
// Reads: FASTQ (four lines a record) or FASTA (sequence lines may wrap), plain text.  One file is single-end, one file with -p is
// interleaved pairs, two files are read in step (their record counts must agree).  QNAME is the header up to the first white
// space, a trailing /1 or /2 removed when the name is longer than two characters.  Bases go through bwa's table: ACGT and acgt
// are 0..3, anything else 4.  FASTA has no qualities: QUAL prints *.
// Batches: -K INT bases per batch (default 10000000; NOT multiplied by the thread count as bwa does).  Records are appended one
// at a time (one from each file with two files); after an append the batch closes when it holds at least K bases and an even
// number of reads.  A batch's first id is the number of pairs (reads, single-end) before it, bwa's n_processed.  As in bwa the
// insert-size estimate is made per batch, so the output depends on -K.
// Options (those whose value a parameter struct of the library holds; any other option of bwa's is refused by name):
//   -k INT min seed length [19]          -w INT band width [100]              -d INT z-drop [100]
//   -r FLOAT re-seed when a seed is longer than k * FLOAT [1.5]               -c INT skip seeds with more occurrences [500]
//   -A INT match score [1]: as in bwa, -B -O -E -L -U -T -d that are not given are scaled by it
//   -B INT mismatch penalty [4]          -O INT[,INT] gap open, deletion[,insertion] [6,6]     -E INT[,INT] gap extension [1,1]
//   -L INT[,INT] clipping penalty 5'[,3'] [5,5]      -U INT unpaired penalty [17]               -T INT minimum score [30]
//   -P no pairing (rescue still runs)    -S no mate rescue (and no estimate before it: regs, pair, cigar, sam)
//   -I FLOAT[,FLOAT[,INT[,INT]]] the FR insert size: mean[,std[,max[,min]]]; std = 0.1 mean, max = (int)(mean + 4 std + .499),
//      min = (int)(mean - 4 std + .499) but at least 1, unless given ((int)(value + .499)); the other three orientations fail
//   -Y soft clipping for supplementary records        -p the one input file is interleaved pairs
//   -K INT bases per batch               -t INT ingest threads (at most 16 are useful)          -o FILE output instead of stdout
// A reader thread prepares batch n + 1 while the aligner runs batch n and a writer thread writes batch n - 1.  Every return code
// is checked: the first failure stops the run, no later batch is started.
// --parse-only: no GPU.  Prints "batches=B reads=R bases=N checksum=H", a line "batch k id0=.. reads=.. bases=.." per batch, the
// four "pes" lines in force with -I, and - when <prefix>.ann exists - "l_pac=.. contigs=.. text_checksum=.." with a line per contig.
// The checksum is FNV-1a over, batch by batch, the int32 read lengths, the base codes, the quality bytes (FASTQ) and the names
// each followed by a newline.
#include <cctype>
#include <condition_variable>
#include <mutex>
#include <thread>
#include "driver_common.h"
#include "fmi_index_io.h"
#include "ref_files.h"
#include "seq_reader.h"

namespace {

struct Batch {
    int64_t id0 = 0, index = 0;
    std::vector<uint8_t> enc, qual, names;
    std::vector<int64_t> read_off, name_off;
    std::vector<int32_t> read_len;
    bool has_qual = false;
    int64_t n_reads() const { return (int64_t)read_len.size(); }
};

// one slot between two threads; close() ends the stream, fail() makes both sides stop
template <class T> struct Slot {
    std::mutex mu;
    std::condition_variable cv;
    T *item = nullptr;
    bool closed = false;
    bool put(T *x)
    {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return !item || closed; });
        if (closed) { delete x; return false; }
        item = x;
        cv.notify_all();
        return true;
    }
    T *take()
    {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return item || closed; });
        T *x = item;
        item = nullptr;
        cv.notify_all();
        return x;
    }
    void close()
    {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return !item || closed; });
        closed = true;
        cv.notify_all();
    }
    void fail()
    {
        std::lock_guard<std::mutex> l(mu);
        closed = true;
        delete item;
        item = nullptr;
        cv.notify_all();
    }
};

inline uint8_t code_of(char c)
{
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}

void append(Batch &b, const Reader &rd, const Reader::Rec &r)
{
    int n = 0;
    while (n < r.head_len && !isspace((unsigned char)r.head[n])) ++n;
    if (n > 2 && r.head[n - 2] == '/' && (r.head[n - 1] == '1' || r.head[n - 1] == '2')) n -= 2;
    b.names.insert(b.names.end(), r.head, r.head + n);
    b.name_off.push_back((int64_t)b.names.size());
    b.read_off.push_back((int64_t)b.enc.size());
    b.read_len.push_back(r.len);
    const size_t o = b.enc.size();
    b.enc.resize(o + (size_t)r.len);
    size_t w = o;
    for (size_t k = r.seq0; k < r.seq1; ++k)
        for (int c = 0; c < rd.llen[k]; ++c) b.enc[w++] = code_of(rd.line[k][c]);
    if (r.qual) { b.has_qual = true; b.qual.insert(b.qual.end(), r.qual, r.qual + r.len); }
    else b.qual.resize(o + (size_t)r.len, (uint8_t)'*');
}

// INT[,INT]: the second value defaults to the first
bool two_ints(const char *s, int32_t *a, int32_t *b)
{
    char *e = nullptr;
    const long x = strtol(s, &e, 10);
    if (e == s) return false;
    *a = *b = (int32_t)x;
    if (*e == ',') { const char *t = e + 1; const long y = strtol(t, &e, 10); if (e == t) return false; *b = (int32_t)y; }
    return *e == 0;
}

// bwa's -I: mean[,std[,max[,min]]] into the FR record; the other orientations fail
bool insert_size(const char *s, gbx_mem_pestat pes[4])
{
    for (int d = 0; d < 4; ++d) { memset(&pes[d], 0, sizeof(pes[d])); pes[d].failed = 1; }
    char *p = nullptr;
    gbx_mem_pestat &r = pes[1];
    r.failed = 0;
    r.avg = strtod(s, &p);
    if (p == s) return false;
    r.std = r.avg * .1;
    auto more = [&]() { return *p != 0 && ispunct((unsigned char)*p) && isdigit((unsigned char)p[1]); };
    if (more()) r.std = strtod(p + 1, &p);
    r.high = (int)(r.avg + 4. * r.std + .499);
    r.low = (int)(r.avg - 4. * r.std + .499);
    if (r.low < 1) r.low = 1;
    if (more()) r.high = (int)(strtod(p + 1, &p) + .499);
    if (more()) r.low = (int)(strtod(p + 1, &p) + .499);
    return *p == 0;
}

struct Reference {
    int64_t l_pac = 0;
    std::vector<int64_t> contig_off, cname_off;
    std::vector<uint8_t> cnames, text;
};

bool read_ann(const std::string &prefix, Reference &R)
{
    const std::string path = prefix + ".ann";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); return false; }
    long long l_pac = 0, seed = 0;
    int n = 0;
    bool ok = fscanf(f, "%lld %d %lld", &l_pac, &n, &seed) == 3 && l_pac > 0 && n > 0;
    R.l_pac = l_pac;
    R.cname_off.assign(1, 0);
    char name[4096];
    for (int c = 0; ok && c < n; ++c) {
        long long gi = 0, off = 0, len = 0;
        int amb = 0, ch;
        ok = fscanf(f, "%lld %4095s", &gi, name) == 2;
        while (ok && (ch = fgetc(f)) != '\n' && ch != EOF) { }                   // the comment
        ok = ok && fscanf(f, "%lld %lld %d", &off, &len, &amb) == 3 && len > 0 && off == (c ? R.contig_off.back() : 0);
        if (!ok) break;
        if (c == 0) R.contig_off.push_back(0);
        R.contig_off.push_back(off + len);
        R.cnames.insert(R.cnames.end(), name, name + strlen(name));
        R.cname_off.push_back((int64_t)R.cnames.size());
    }
    fclose(f);
    if (!ok || R.contig_off.back() != R.l_pac) { fprintf(stderr, "%s: not a .ann file whose contigs tile [0, l_pac)\n", path.c_str()); return false; }
    return true;
}

bool read_text(const std::string &prefix, Reference &R)
{
    const size_t L = (size_t)R.l_pac;
    std::vector<char> raw;
    const std::string p0123 = prefix + ".0123", ppac = prefix + ".pac";
    if (slurp(p0123.c_str(), raw)) {
        if (raw.size() - 1 != 2 * L) {
            fprintf(stderr, "%s: %zu bytes, 2 l_pac = %zu expected\n", p0123.c_str(), raw.size() - 1, 2 * L);
            return false;
        }
        R.text.assign(raw.begin(), raw.end() - 1);
        for (size_t k = 0; k < 2 * L; ++k)
            if (R.text[k] > 3) { fprintf(stderr, "%s: byte %zu is no code 0..3\n", p0123.c_str(), k); return false; }
        return true;
    }
    if (!slurp(ppac.c_str(), raw)) { fprintf(stderr, "cannot open %s or %s\n", p0123.c_str(), ppac.c_str()); return false; }
    if (raw.size() - 1 < (L + 3) / 4) { fprintf(stderr, "%s: too short for l_pac = %zu\n", ppac.c_str(), L); return false; }
    R.text.resize(2 * L);
    for (size_t l = 0; l < L; ++l) {
        const uint8_t c = (uint8_t)(((unsigned char)raw[l >> 2] >> ((~l & 3) << 1)) & 3);
        R.text[l] = c;
        R.text[2 * L - 1 - l] = (uint8_t)(3 - c);
    }
    return true;
}

int usage()
{
    fprintf(stderr,
            "Usage: mem [options] <idxprefix> <in1.fq> [in2.fq]\n"
            "       mem index [-p prefix] [--parse-only] <in.fa>   writes <prefix>.bwt.2bit.64 .ann .amb .pac .0123 (prefix: in.fa)\n"
            "  -k INT -w INT -d INT -r FLOAT -c INT -A INT -B INT -O INT[,INT] -E INT[,INT] -L INT[,INT] -U INT -T INT\n"
            "  -P  no pairing    -S  no mate rescue    -Y  soft clipping for supplementary records    -p  interleaved pairs\n"
            "  -I FLOAT[,FLOAT[,INT[,INT]]]  FR insert size: mean[,std[,max[,min]]] (std 0.1 mean, max/min mean +/- 4 std)\n"
            "  -K INT  bases per batch [10000000]; not multiplied by the thread count\n"
            "  -t INT  ingest threads (at most 16 are useful)    -o FILE  output    --parse-only  ingest only, no GPU\n"
            "  index: <idxprefix>.bwt.2bit.64 .ann and .0123 or .pac; .amb is not read\n");
    return 1;
}

// mem index [-p prefix] [--parse-only] <in.fa>
int index_main(int argc, char **argv)
{
    const char *prefix_arg = nullptr, *fasta = nullptr;
    bool parse_only = false;
    for (int i = 1; i < argc; ++i) {
        const char *s = argv[i];
        if (!strcmp(s, "--parse-only")) { parse_only = true; continue; }
        if (s[0] != '-' || s[1] == 0) {
            if (fasta) { fprintf(stderr, "mem index: one FASTA file\n"); return usage(); }
            fasta = s;
            continue;
        }
        if (s[1] != 'p') { fprintf(stderr, "mem index: option %s is not supported\n", s); return usage(); }
        prefix_arg = s[2] ? s + 2 : (i + 1 < argc ? argv[++i] : nullptr);
        if (!prefix_arg) { fprintf(stderr, "mem index: option -p needs a value\n"); return usage(); }
    }
    if (!fasta) return usage();
    const std::string prefix = prefix_arg ? prefix_arg : fasta;
    std::vector<char> raw;
    if (!ref_files::read_file(fasta, raw)) { fprintf(stderr, "mem index: cannot read %s\n", fasta); return 1; }
    ref_files::Reference R;
    std::string err;
    if (!ref_files::parse_fasta(raw.data(), raw.size(), R, err)) { fprintf(stderr, "mem index: %s: %s\n", fasta, err.c_str()); return 1; }
    std::vector<char>().swap(raw);
    if (!ref_files::write_reference(prefix, R, err)) { fprintf(stderr, "mem index: %s\n", err.c_str()); return 1; }
    if (parse_only) {
        const std::vector<uint8_t> text = ref_files::text_of(R);
        printf("l_pac=%lld contigs=%d holes=%lld text_checksum=%016llx\n", (long long)R.l_pac, (int)R.contigs.size(), (long long)R.holes.size(),
               (unsigned long long)ref_files::fnv1a(text.data(), text.size()));
        for (size_t c = 0; c < R.contigs.size(); ++c)
            printf("contig %d %s %lld %lld %d\n", (int)c, R.contigs[c].name.c_str(), (long long)R.contigs[c].off, (long long)R.contigs[c].len, R.contigs[c].n_ambs);
        return 0;
    }
    const double t0 = now_s();
    const int64_t n1 = 2 * R.l_pac + 1, n_sa = (n1 >> 3) + 1;
    std::vector<gbx_fmi_cp_occ> cp((size_t)(n1 >> 6) + 1);
    std::vector<int8_t> ms((size_t)n_sa);
    std::vector<uint32_t> ls((size_t)n_sa);
    gbx_fmi_index idx;
    int64_t info[8];
    char dev_name[256];
    if (gbx_device_name(dev_name, sizeof dev_name) == GBX_OK) fprintf(stderr, "gbx device: %s\n", dev_name);
    const int rc = gbx_fmi_build_host(R.codes.data(), R.l_pac, 3, &idx, cp.data(), ms.data(), ls.data(), info);
    if (rc != GBX_OK) { fprintf(stderr, "mem index: gbx_fmi_build_host failed (%d): %s\n", rc, gbx_last_error()); return 1; }
    if (!ref_files::write_bwt(prefix, idx.ref_seq_len, idx.count, idx.sentinel_index, cp.data(), ms.data(), ls.data(), n_sa)) {
        fprintf(stderr, "mem index: cannot write %s.bwt.2bit.64\n", prefix.c_str());
        return 1;
    }
    fprintf(stderr, "mem index: l_pac %lld, %d contigs, %lld holes, %lld doubling rounds, %.3f s\n", (long long)R.l_pac, (int)R.contigs.size(),
            (long long)R.holes.size(), (long long)info[6], now_s() - t0);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "index")) return index_main(argc - 1, argv + 1);
    gbx_mem_align_params P;
    gbx_mem_align_default_params(&P);
    int32_t a = 1, b = 4, o_del = 6, o_ins = 6, e_del = 1, e_ins = 1, clip5 = 5, clip3 = 5, unpaired = 17, w = 100, zdrop = 100, k = 19, T = 30;
    bool g_b = false, g_O = false, g_E = false, g_L = false, g_U = false, g_T = false, g_d = false, g_A = false;
    double split = 1.5;
    int64_t K = 10000000;
    int threads = 1;
    bool interleaved = false, parse_only = false, have_I = false;
    const char *out_path = nullptr;
    std::vector<const char *> pos;
    for (int i = 1; i < argc; ++i) {
        const char *s = argv[i];
        if (!strcmp(s, "--parse-only")) { parse_only = true; continue; }
        if (s[0] != '-' || s[1] == 0) { pos.push_back(s); continue; }
        if (s[1] == '-' || !strchr("kwdrcABOELUTPSIYpKto", s[1])) { fprintf(stderr, "mem: option %s is not supported\n", s); return usage(); }
        const char o = s[1];
        if (strchr("PSYp", o)) {
            if (s[2]) { fprintf(stderr, "mem: option %s is not supported\n", s); return usage(); }
            if (o == 'P') P.pair.no_pairing = 1;
            else if (o == 'S') P.no_rescue = 1;
            else if (o == 'Y') P.sam.softclip = 1;
            else interleaved = true;
            continue;
        }
        const char *v = s[2] ? s + 2 : (i + 1 < argc ? argv[++i] : nullptr);
        if (!v) { fprintf(stderr, "mem: option -%c needs a value\n", o); return usage(); }
        bool ok = true;
        switch (o) {
        case 'k': k = atoi(v); break;
        case 'w': w = atoi(v); break;
        case 'd': zdrop = atoi(v); g_d = true; break;
        case 'r': split = atof(v); break;
        case 'c': P.max_occ = P.chain.max_occ = atoi(v); break;
        case 'A': a = atoi(v); g_A = true; break;
        case 'B': b = atoi(v); g_b = true; break;
        case 'O': ok = two_ints(v, &o_del, &o_ins); g_O = true; break;
        case 'E': ok = two_ints(v, &e_del, &e_ins); g_E = true; break;
        case 'L': ok = two_ints(v, &clip5, &clip3); g_L = true; break;
        case 'U': unpaired = atoi(v); g_U = true; break;
        case 'T': T = atoi(v); g_T = true; break;
        case 'I': ok = insert_size(v, P.pes); have_I = true; break;
        case 'K': K = atoll(v); break;
        case 't': threads = atoi(v); break;
        case 'o': out_path = v; break;
        }
        if (!ok) { fprintf(stderr, "mem: bad value `%s' for -%c\n", v, o); return usage(); }
    }
    if (pos.size() < 2 || pos.size() > 3) return usage();
    if (pos.size() == 3 && interleaved) { fprintf(stderr, "mem: -p takes one input file\n"); return 1; }
    if (g_A) {                            // bwa: the penalties that were not given scale with the match score
        if (!g_b) b *= a;
        if (!g_T) T *= a;
        if (!g_O) { o_del *= a; o_ins *= a; }
        if (!g_E) { e_del *= a; e_ins *= a; }
        if (!g_d) zdrop *= a;
        if (!g_L) { clip5 *= a; clip3 *= a; }
        if (!g_U) unpaired *= a;
    }
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    if (K < 1 || k < 1 || split <= 0) { fprintf(stderr, "mem: -K, -k and -r must be positive\n"); return 1; }
    gbx_mem_align_set_scoring(&P, a, b, o_del, e_del, o_ins, e_ins, clip5, clip3, unpaired, w, zdrop, k, T);
    P.fmi.split_len = (int32_t)(k * split + .499);
    P.have_pes = have_I ? 1 : 0;
    const bool paired = pos.size() == 3 || interleaved;
    P.mode = paired ? 1 : 0;
    if (gbx_mem_align_check_params(&P) != GBX_OK) { fprintf(stderr, "mem: %s\n", gbx_last_error()); return 1; }
    const std::string prefix = pos[0];

    Reader in[2];
    const int n_in = (int)pos.size() - 1;
    for (int f = 0; f < n_in; ++f) if (!in[f].open(pos[(size_t)f + 1], threads)) return EXIT_FAILURE;

    // ---- the reader thread: batch after batch into a slot
    Slot<Batch> ready;
    std::string read_error;
    std::thread reader([&] {
        int64_t done = 0, index = 0;
        for (;;) {
            Batch *bt = new Batch();
            bt->id0 = paired ? done / 2 : done;
            bt->index = index++;
            bt->name_off.push_back(0);
            int64_t bases = 0;
            bool end = false;
            while (!end) {
                Reader::Rec r[2];
                int got[2] = {0, 0};
                for (int f = 0; f < n_in; ++f) got[f] = in[f].next(r[f]);
                for (int f = 0; f < n_in; ++f) if (got[f] < 0) read_error = std::string(pos[(size_t)f + 1]) + ": malformed record";
                if (n_in == 2 && got[0] != got[1] && read_error.empty())
                    read_error = std::string("the two input files hold different numbers of records (") + pos[got[0] ? 2 : 1] + " ends first)";
                if (!read_error.empty()) { delete bt; ready.fail(); return; }
                if (!got[0]) { end = true; break; }
                for (int f = 0; f < n_in; ++f) { append(*bt, in[f], r[f]); bases += r[f].len; }
                if (bases >= K && (bt->n_reads() & 1) == 0) break;
            }
            if (paired && (bt->n_reads() & 1)) { read_error = "an odd number of reads in interleaved input"; delete bt; ready.fail(); return; }
            if (bt->n_reads() == 0) { delete bt; break; }
            done += bt->n_reads();
            if (!ready.put(bt)) return;
            if (end) break;
        }
        ready.close();
    });

    if (parse_only) {
        int64_t n_batches = 0, reads = 0, bases = 0;
        uint64_t h = 1469598103934665603ull;
        std::string lines;
        while (Batch *bt = ready.take()) {
            h = fnv1a(bt->read_len.data(), bt->read_len.size() * 4, h);
            h = fnv1a(bt->enc.data(), bt->enc.size(), h);
            if (bt->has_qual) h = fnv1a(bt->qual.data(), bt->qual.size(), h);
            for (int64_t r = 0; r < bt->n_reads(); ++r) {
                h = fnv1a(bt->names.data() + bt->name_off[(size_t)r], (size_t)(bt->name_off[(size_t)r + 1] - bt->name_off[(size_t)r]), h);
                h = fnv1a("\n", 1, h);
            }
            char buf[160];
            snprintf(buf, sizeof buf, "batch %lld id0=%lld reads=%lld bases=%lld\n", (long long)n_batches, (long long)bt->id0, (long long)bt->n_reads(),
                     (long long)bt->enc.size());
            lines += buf;
            ++n_batches; reads += bt->n_reads(); bases += (int64_t)bt->enc.size();
            delete bt;
        }
        reader.join();
        if (!read_error.empty()) { fprintf(stderr, "mem: %s\n", read_error.c_str()); return EXIT_FAILURE; }
        printf("batches=%lld reads=%lld bases=%lld checksum=%016llx\n%s", (long long)n_batches, (long long)reads, (long long)bases, (unsigned long long)h,
               lines.c_str());
        if (have_I)
            for (int d = 0; d < 4; ++d)
                printf("pes %d low=%d high=%d failed=%d avg=%.6f std=%.6f\n", d, P.pes[d].low, P.pes[d].high, P.pes[d].failed, P.pes[d].avg, P.pes[d].std);
        FILE *ann = fopen((prefix + ".ann").c_str(), "r");
        if (ann) {
            fclose(ann);
            Reference R;
            if (!read_ann(prefix, R) || !read_text(prefix, R)) return EXIT_FAILURE;
            const int n = (int)R.contig_off.size() - 1;
            printf("l_pac=%lld contigs=%d text_checksum=%016llx\n", (long long)R.l_pac, n, (unsigned long long)fnv1a(R.text.data(), R.text.size()));
            for (int c = 0; c < n; ++c)
                printf("contig %d %.*s %lld %lld\n", c, (int)(R.cname_off[(size_t)c + 1] - R.cname_off[(size_t)c]),
                       (const char *)R.cnames.data() + R.cname_off[(size_t)c], (long long)R.contig_off[(size_t)c],
                       (long long)(R.contig_off[(size_t)c + 1] - R.contig_off[(size_t)c]));
        }
        return 0;
    }

    // ---- the index, the aligner
    auto stop = [&](const char *what) {
        fprintf(stderr, "mem: %s\n", what);
        ready.fail();
        reader.join();
        return EXIT_FAILURE;
    };
    Reference R;
    if (!read_ann(prefix, R) || !read_text(prefix, R)) return stop("no reference");
    gbx_fmi_index idx;
    std::vector<gbx_fmi_cp_occ> cp;
    gbx_fmi_sa sa{};
    std::vector<int8_t> sa_ms;
    std::vector<uint32_t> sa_ls;
    if (!read_index(prefix.c_str(), idx, cp) || !read_sa(prefix.c_str(), idx, sa, sa_ms, sa_ls)) return stop("no index");
    idx.cp_occ = cp.data();
    if (idx.ref_seq_len != 2 * R.l_pac + 1) return stop("the .bwt.2bit.64 file and the .ann file are of different references");
    char dev_name[256];
    if (gbx_device_name(dev_name, sizeof dev_name) == GBX_OK) fprintf(stderr, "gbx device: %s\n", dev_name);
    gbx_mem_index *ix = nullptr;
    gbx_mem_aligner *al = nullptr;
    int rc = gbx_mem_index_create(&idx, &sa, R.text.data(), R.l_pac, (int32_t)R.contig_off.size() - 1, R.contig_off.data(), R.cnames.data(),
                                  R.cname_off.data(), &ix);
    if (rc == GBX_OK) rc = gbx_mem_aligner_create(ix, &P, nullptr, &al);
    if (rc != GBX_OK) { gbx_mem_index_destroy(ix); return stop(gbx_last_error()); }
    FILE *out = out_path ? fopen(out_path, "wb") : stdout;
    if (!out) { gbx_mem_aligner_destroy(al); gbx_mem_index_destroy(ix); return stop("cannot open the output file"); }

    // ---- the writer thread
    Slot<std::string> done;
    bool write_failed = false;
    std::thread writer([&] {
        while (std::string *t = done.take()) {
            if (!write_failed && !t->empty() && fwrite(t->data(), 1, t->size(), out) != t->size()) { write_failed = true; done.fail(); }
            delete t;
        }
    });
    {
        int64_t need = 0;
        (void)gbx_mem_sam_header(ix, nullptr, 0, &need);
        std::string *h = new std::string((size_t)need, '\0');
        rc = gbx_mem_sam_header(ix, (uint8_t *)&(*h)[0], need, &need);
        if (rc == GBX_OK) done.put(h); else delete h;
    }
    const double t0 = now_s();
    int64_t n_reads = 0, reruns = 0;
    std::string error;
    while (rc == GBX_OK && !write_failed) {
        Batch *bt = ready.take();
        if (!bt) break;
        gbx_mem_align_out o;
        rc = gbx_mem_aligner_run(al, bt->n_reads(), bt->id0, bt->enc.data(), (int64_t)bt->enc.size(), bt->read_off.data(), bt->read_len.data(),
                                 bt->has_qual ? bt->qual.data() : nullptr, bt->names.data(), bt->name_off.data(), &o);
        if (rc != GBX_OK) error = gbx_last_error();
        else {
            n_reads += bt->n_reads(); reruns += o.stats.reruns;
            if (!done.put(new std::string((const char *)o.sam, (size_t)o.n_text))) rc = GBX_ERR_ARG;
        }
        delete bt;
    }
    if (rc != GBX_OK) ready.fail();       // no later batch is started
    reader.join();
    done.close();
    writer.join();
    gbx_mem_aligner_destroy(al);
    gbx_mem_index_destroy(ix);
    bool bad = rc != GBX_OK || write_failed || !read_error.empty();
    if (out_path) bad = (fclose(out) != 0) || bad; else bad = (fflush(stdout) != 0) || bad;
    if (!read_error.empty()) fprintf(stderr, "mem: %s\n", read_error.c_str());
    if (!error.empty()) fprintf(stderr, "mem: gbx_mem_aligner_run failed (%d): %s\n", rc, error.c_str());
    if (write_failed) fprintf(stderr, "mem: writing the output failed\n");
    fprintf(stderr, "mem: %lld reads, %lld reruns, %.3f s\n", (long long)n_reads, (long long)reruns, now_s() - t0);
    return bad ? EXIT_FAILURE : 0;
}
