// meth_freq_main.cpp — f5c meth-freq (R/benchmarks/abea/src/freq.c) over the C-ABI of libgbx.so: the call-methylation TSV in,
// one line per genomic site out.  The options are freq.c's getopt ("c:i:o:s"), input from stdin and output to stdout unless
// -i / -o name files; where the reference exits on its input, so does this, with its message and status 1.
// --parse-only (not a reference flag): read and parse, print the record and contig counts and a checksum, touch no GPU.
#include <getopt.h>
#include <cerrno>
#include "driver_common.h"

static const char usage[] = "Usage: %s [options...]\n"
                            "\n"
                            "  -c [float]        Call threshold. Default is 2.5.\n"
                            "  -i [file]         Input file. Read from stdin if not specified.\n"
                            "  -o [file]         Output file. Write to stdout if not specified.\n"
                            "  -s                Split groups\n";

int main(int argc, char **argv)
{
    FILE *input = stdin;
    double call_threshold = 2.5;
    bool split_groups = false, parse_only = false;
    static const struct option longopts[] = {{"parse-only", no_argument, nullptr, 1000}, {nullptr, 0, nullptr, 0}};
    int c;
    while ((c = getopt_long(argc, argv, "c:i:o:s", longopts, nullptr)) != -1) {
        switch (c) {
            case 'c': call_threshold = strtod(optarg, nullptr); break;
            case 'i': {
                FILE *in = fopen(optarg, "r");
                if (!in) {                                           // F_CHK (error.h:48-58); its second line names the reference's own source line
                    fprintf(stderr, "[freq_main::ERROR]\033[1;31m Failed to open %s : %s.\033[0m\n", optarg, strerror(errno));
                    exit(EXIT_FAILURE);
                }
                input = in;
                break;
            }
            case 's': split_groups = true; break;
            case 1000: parse_only = true; break;
            case ':':
                fprintf(stderr, "Option -%c requires an operand\n", optopt);
                fprintf(stderr, usage, argv[0]);
                exit(EXIT_FAILURE);
            case '?':
                fprintf(stderr, "Unrecognized option: -%c\n", optopt);
                fprintf(stderr, usage, argv[0]);
                exit(EXIT_FAILURE);
            case 'o':
                if (strcmp(optarg, "-") != 0 && freopen(optarg, "wb", stdout) == nullptr) {
                    fprintf(stderr, "[freq_main::ERROR]\033[1;31m failed to write the output to file %s : %s\033[0m\n", optarg, strerror(errno));   // ERROR, error.h:16-18
                    exit(EXIT_FAILURE);
                }
                break;
            default: break;
        }
    }
    if (input == stdin) fprintf(stderr, "Scanning the input from stdin ...\n");
    std::vector<char> text;
    {
        char chunk[1 << 16];
        size_t got;
        while ((got = fread(chunk, 1, sizeof chunk, input)) > 0) text.insert(text.end(), chunk, chunk + got);
        if (input != stdin) fclose(input);
    }
    // sizes first, then the arrays
    int64_t counts[4] = {0, 0, 0, 0}, bad_line = 0;
    int header_kind = 0;
    int rc = gbx_abea_freq_parse_host(text.data(), (int64_t)text.size(), 0, nullptr, 0, nullptr, 0, nullptr, counts, &header_kind, &bad_line);
    if (rc != GBX_OK && bad_line >= 0) {                              // the reference's own message
        if (rc == GBX_ERR_UNSUPPORTED) fprintf(stderr, "%s\n", gbx_last_error()); else fputs(gbx_last_error(), stderr);
        return EXIT_FAILURE;
    }
    std::vector<gbx_abea_freq_record> records((size_t)counts[0] + 1);
    std::vector<char> arena((size_t)counts[1] + 1), names((size_t)counts[3] + 1);
    die_on(gbx_abea_freq_parse_host(text.data(), (int64_t)text.size(), counts[0], records.data(), counts[1], arena.data(), counts[3], names.data(), counts,
                                    &header_kind, &bad_line),
           "gbx_abea_freq_parse_host");
    std::vector<char>().swap(text);
    std::vector<const char *> contig((size_t)counts[2] + 1, nullptr);
    {
        const char *p = names.data();
        for (int64_t k = 0; k < counts[2]; ++k) { contig[(size_t)k] = p; p += strlen(p) + 1; }
    }
    if (parse_only) {
        uint64_t h = fnv1a(records.data(), (size_t)counts[0] * sizeof(gbx_abea_freq_record));
        h = fnv1a(arena.data(), (size_t)counts[1], h);
        h = fnv1a(names.data(), (size_t)counts[3], h);
        printf("records %lld contigs %lld sequence_bytes %lld header_kind %d checksum %016llx\n", (long long)counts[0], (long long)counts[2],
               (long long)counts[1], header_kind, (unsigned long long)h);
        return 0;
    }
    int64_t n_sites = 0, seq_bytes = 0;
    rc = gbx_abea_freq_host(counts[0], records.data(), arena.data(), counts[1], call_threshold, split_groups ? 1 : 0, 0, nullptr, &n_sites, 0, nullptr, &seq_bytes);
    if (rc != GBX_OK && !(rc == GBX_ERR_ARG && (n_sites > 0 || seq_bytes > 0))) die_on(rc, "gbx_abea_freq_host");
    std::vector<gbx_abea_freq_site> sites((size_t)n_sites + 1);
    std::vector<char> seqs((size_t)seq_bytes + 1);
    if (n_sites > 0)
        die_on(gbx_abea_freq_host(counts[0], records.data(), arena.data(), counts[1], call_threshold, split_groups ? 1 : 0, n_sites, sites.data(), &n_sites, seq_bytes,
                                  seqs.data(), &seq_bytes),
               "gbx_abea_freq_host");
    int64_t n_text = 0;
    rc = gbx_abea_freq_tsv_host(n_sites, sites.data(), seqs.data(), seq_bytes, counts[2], contig.data(), header_kind, 1, 0, nullptr, &n_text);
    if (rc != GBX_OK && !(rc == GBX_ERR_ARG && n_text > 0)) die_on(rc, "gbx_abea_freq_tsv_host");
    std::vector<char> out((size_t)n_text + 1);
    die_on(gbx_abea_freq_tsv_host(n_sites, sites.data(), seqs.data(), seq_bytes, counts[2], contig.data(), header_kind, 1, n_text, out.data(), &n_text),
           "gbx_abea_freq_tsv_host");
    if (fwrite(out.data(), 1, (size_t)n_text, stdout) != (size_t)n_text) { fprintf(stderr, "short write\n"); return EXIT_FAILURE; }
    return 0;
}
