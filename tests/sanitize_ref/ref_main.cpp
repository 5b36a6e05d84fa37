// ref_main — csrc/drivers/ref_files.h on its own, for the ASan + UBSan build (tests/sanitize_ref/Makefile):
//   ref_main <outdir> <in.fa>...
// parses every file, writes the four reference files of the ones that parse under <outdir>/<k>, reads .pac back against the
// codes, and prints one line per file: "ok l_pac=.. contigs=.. holes=.. text_checksum=.." or "error: ..".  A file that does not
// parse is not a failure of this program; what the sanitizers find is.
#include "../../genomicsbench_amd/csrc/drivers/ref_files.h"

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: ref_main <outdir> <in.fa>...\n"); return 2; }
    for (int k = 2; k < argc; ++k) {
        std::vector<char> raw;
        if (!ref_files::read_file(argv[k], raw)) { printf("error: cannot read %s\n", argv[k]); continue; }
        ref_files::Reference R;
        std::string err;
        if (!ref_files::parse_fasta(raw.data(), raw.size(), R, err)) { printf("error: %s\n", err.c_str()); continue; }
        const std::string prefix = std::string(argv[1]) + "/" + std::to_string(k - 2);
        if (!ref_files::write_reference(prefix, R, err)) { printf("error: %s\n", err.c_str()); return 1; }
        std::vector<char> pac;
        if (!ref_files::read_file((prefix + ".pac").c_str(), pac)) return 1;
        for (int64_t l = 0; l < R.l_pac; ++l)
            if ((((unsigned char)pac[(size_t)l >> 2] >> ((~l & 3) << 1)) & 3) != R.codes[(size_t)l]) { printf("error: .pac base %lld\n", (long long)l); return 1; }
        // the index file's writer on made-up tables of the right sizes
        const int64_t n1 = 2 * R.l_pac + 1, n_sa = (n1 >> 3) + 1, count[5] = {1, 1, 1, 1, n1};
        std::vector<uint64_t> cp(((size_t)(n1 >> 6) + 1) * 8, 0);
        std::vector<int8_t> ms((size_t)n_sa, 0);
        std::vector<uint32_t> ls((size_t)n_sa, 0);
        if (!ref_files::write_bwt(prefix, n1, count, 0, cp.data(), ms.data(), ls.data(), n_sa)) return 1;
        const std::vector<uint8_t> text = ref_files::text_of(R);
        printf("ok l_pac=%lld contigs=%d holes=%lld text_checksum=%016llx\n", (long long)R.l_pac, (int)R.contigs.size(), (long long)R.holes.size(),
               (unsigned long long)ref_files::fnv1a(text.data(), text.size()));
    }
    return 0;
}
