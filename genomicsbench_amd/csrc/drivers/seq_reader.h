// seq_reader.h — the FASTA / FASTQ reader the `mem` and `mmseed` drivers share: plain text, FASTQ four lines a record, FASTA
// sequence lines may wrap.
#pragma once
#include "driver_common.h"

namespace {

// a FASTA / FASTQ file in memory, walked record by record
struct Reader {
    std::vector<char> text;
    std::vector<const char *> line;
    std::vector<int> llen;
    bool fastq = false;
    size_t at = 0;                        // next line
    bool open(const char *path, int threads)
    {
        if (!slurp(path, text)) { fprintf(stderr, "[E::main] fail to open file `%s'.\n", path); return false; }
        if (text.size() > 1 && text[text.size() - 2] != '\n') { text[text.size() - 1] = '\n'; text.push_back(0); }
        split_lines(text.data(), text.size() - 1, threads, line, llen);
        for (size_t k = 0; k < line.size(); ++k) if (llen[k] > 0 && line[k][llen[k] - 1] == '\r') llen[k] -= 1;
        while (at < line.size() && llen[at] == 0) ++at;
        fastq = at < line.size() && line[at][0] == '@';
        if (at < line.size() && !fastq && line[at][0] != '>') { fprintf(stderr, "%s: neither FASTA nor FASTQ\n", path); return false; }
        return true;
    }
    struct Rec { const char *head; int head_len; size_t seq0, seq1; const char *qual; int len; };
    // 1: a record, 0: the end, -1: malformed
    int next(Rec &r)
    {
        while (at < line.size() && llen[at] == 0) ++at;
        if (at >= line.size()) return 0;
        r.head = line[at] + 1; r.head_len = llen[at] - 1; r.qual = nullptr;
        if (fastq) {
            if (line[at][0] != '@' || at + 3 >= line.size() + 0 || line[at + 2][0] != '+' || llen[at + 3] != llen[at + 1]) return -1;
            r.seq0 = at + 1; r.seq1 = at + 2; r.len = llen[at + 1]; r.qual = line[at + 3];
            at += 4;
            return 1;
        }
        if (line[at][0] != '>') return -1;
        r.seq0 = ++at; r.len = 0;
        while (at < line.size() && !(llen[at] > 0 && line[at][0] == '>')) r.len += llen[at++];
        r.seq1 = at;
        return 1;
    }
};

}  // namespace
