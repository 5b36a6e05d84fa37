// bam_reader.h — a BGZF / BAM reader for the pileup driver, on zlib alone (no htslib).
//
// The file is read whole; its BGZF blocks are found by walking their headers, inflated in parallel (OpenMP, num_threads)
// into one buffer and checked (CRC-32 and size); then the header (contig names and lengths) and the records are parsed.
// No .bai: every record is looked at, and the pileup's reads are kept: the benchmark's filter (medaka_bamiter.c: no
// UNMAP / SECONDARY / SUPPLEMENTARY / QCFAIL / DUP flag, mapq >= 1), on the region's contig, overlapping [beg, end).
// Anything that is not BGZF, not BAM or cut short is refused with a message; every read of the file's bytes is checked
// against their end first.
#pragma once
#include <zlib.h>
#include <omp.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace bam {

struct Contig { std::string name; int64_t len; };

struct Reads {                                   // gbx_pileup_reads' arrays, sorted by pos
    std::vector<int32_t> pos;
    std::vector<int64_t> cigar_off{0};
    std::vector<uint32_t> cigar;
    std::vector<int64_t> seq_off{0}, seq_boff;
    std::vector<uint8_t> seq, qual, rev;
    std::vector<int8_t> dtype;
    std::vector<std::string> names;
};

inline uint16_t rd16(const uint8_t *p) { uint16_t v; memcpy(&v, p, 2); return v; }
inline int32_t rd32(const uint8_t *p) { int32_t v; memcpy(&v, p, 4); return v; }
inline uint32_t rdu32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// the inflated bytes of a BGZF file; false with *err set on anything else
inline bool bgzf_inflate(const std::vector<uint8_t> &raw, int threads, std::vector<uint8_t> &out, std::string *err)
{
    struct Blk { size_t at, cdata, clen, isize, out; uint32_t crc; };
    std::vector<Blk> blks;
    size_t at = 0, total = 0;
    char msg[256];
    while (at < raw.size()) {
        const uint8_t *p = raw.data() + at;
        const size_t left = raw.size() - at;
        if (left < 18) { snprintf(msg, sizeof msg, "truncated BGZF block header at byte %zu", at); *err = msg; return false; }
        if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) {
            snprintf(msg, sizeof msg, "not a BGZF file (bad block header at byte %zu)", at);
            *err = msg;
            return false;
        }
        const size_t xlen = rd16(p + 10);
        if (12 + xlen > left) { snprintf(msg, sizeof msg, "truncated BGZF extra field at byte %zu", at); *err = msg; return false; }
        size_t bsize = 0;
        for (size_t x = 12; x + 4 <= 12 + xlen;) {
            const size_t slen = rd16(p + x + 2);
            if (p[x] == 66 && p[x + 1] == 67 && slen == 2 && x + 6 <= 12 + xlen) bsize = (size_t)rd16(p + x + 4) + 1;
            x += 4 + slen;
        }
        if (!bsize) { snprintf(msg, sizeof msg, "not a BGZF file (no BC field at byte %zu)", at); *err = msg; return false; }
        if (bsize < 12 + xlen + 8 || bsize > left) { snprintf(msg, sizeof msg, "truncated BGZF block at byte %zu", at); *err = msg; return false; }
        const size_t isize = rdu32(p + bsize - 4);
        if (isize > 65536) { snprintf(msg, sizeof msg, "corrupt BGZF block at byte %zu (size %zu)", at, isize); *err = msg; return false; }
        blks.push_back(Blk{at, at + 12 + xlen, bsize - 12 - xlen - 8, isize, total, rdu32(p + bsize - 8)});
        total += isize;
        at += bsize;
    }
    out.assign(total, 0);
    std::vector<char> bad(blks.size(), 0);
#pragma omp parallel for num_threads(threads < 1 ? 1 : threads) schedule(dynamic, 64)
    for (long b = 0; b < (long)blks.size(); ++b) {
        const Blk &k = blks[(size_t)b];
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) { bad[(size_t)b] = 1; continue; }
        z.next_in = const_cast<uint8_t *>(raw.data() + k.cdata);
        z.avail_in = (uInt)k.clen;
        uint8_t dummy = 0;
        z.next_out = k.isize ? out.data() + k.out : &dummy;
        z.avail_out = (uInt)k.isize;
        const int rc = inflate(&z, Z_FINISH);
        const bool ok = rc == Z_STREAM_END && z.total_out == k.isize;
        inflateEnd(&z);
        if (!ok || (uint32_t)crc32(0L, k.isize ? out.data() + k.out : &dummy, (uInt)k.isize) != k.crc) bad[(size_t)b] = 1;
    }
    for (size_t b = 0; b < blks.size(); ++b)
        if (bad[b]) { snprintf(msg, sizeof msg, "corrupt BGZF block at byte %zu (inflate, size or CRC)", blks[b].at); *err = msg; return false; }
    return true;
}

// The DT:Z value of a record's aux bytes [p, e), or false (absent, or an aux block that cannot be walked)
inline bool aux_z(const uint8_t *p, const uint8_t *e, const char *tag, std::string *val)
{
    while (p + 3 <= e) {
        const char t0 = (char)p[0], t1 = (char)p[1], typ = (char)p[2];
        p += 3;
        int sz = 0;
        switch (typ) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': {
            const uint8_t *z = (const uint8_t *)memchr(p, 0, (size_t)(e - p));
            if (!z) return false;
            if (typ == 'Z' && t0 == tag[0] && t1 == tag[1]) { val->assign((const char *)p, (size_t)(z - p)); return true; }
            p = z + 1;
            continue;
        }
        case 'B': {
            if (p + 5 > e) return false;
            const char sub = (char)p[0];
            const int64_t cnt = rd32(p + 1);
            const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0 || cnt * es > e - p - 5) return false;
            p += 5 + cnt * es;
            continue;
        }
        default: return false;
        }
        if (sz > e - p) return false;
        p += sz;
    }
    return false;
}

inline bool ref_op(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

struct Region { std::string contig; int64_t beg = 0, end = 0; };

// hts_parse_decimal: digits with ',' separators; false when there is none
inline bool parse_dec(const char *s, const char *e, int64_t *v, const char **stop)
{
    int64_t x = 0;
    bool seen = false;
    for (; s < e; ++s) {
        if (*s == ',') continue;
        if (*s < '0' || *s > '9') break;
        x = x * 10 + (*s - '0');
        if (x > INT32_MAX) x = INT32_MAX;
        seen = true;
    }
    *v = x; *stop = s;
    return seen;
}

// hts_parse_reg as the driver uses it: 'chr', 'chr:beg', 'chr:beg-end' (beg 1-based, clamped at 0; end inclusive);
// an open end is the contig's length
inline bool parse_region(const std::string &reg, const std::vector<Contig> &contigs, Region *out, std::string *err)
{
    auto len_of = [&](const std::string &n) -> int64_t { for (const Contig &c : contigs) if (c.name == n) return c.len; return -1; };
    if (len_of(reg) >= 0 || reg.rfind(':') == std::string::npos) {
        out->contig = reg; out->beg = 0; out->end = std::max<int64_t>(0, len_of(reg));
        if (len_of(reg) < 0) { *err = "contig '" + reg + "' is not in the BAM header"; return false; }
        return true;
    }
    const size_t c = reg.rfind(':');
    out->contig = reg.substr(0, c);
    const int64_t clen = len_of(out->contig);
    if (out->contig.empty()) { *err = "Failed to parse region: '" + reg + "'"; return false; }
    if (clen < 0) { *err = "contig '" + out->contig + "' is not in the BAM header"; return false; }
    const char *s = reg.c_str() + c + 1, *e = reg.c_str() + reg.size(), *stop = s;
    int64_t beg = 0, end = clen;
    const char *dash = (const char *)memchr(s, '-', (size_t)(e - s));
    if (dash) {
        if (!parse_dec(s, dash, &beg, &stop) && dash != s) { *err = "Failed to parse region: '" + reg + "'"; return false; }
        int64_t v = 0;
        if (parse_dec(dash + 1, e, &v, &stop)) end = v;
    } else if (!parse_dec(s, e, &beg, &stop)) { *err = "Failed to parse region: '" + reg + "'"; return false; }
    beg = std::max<int64_t>(beg - 1, 0);
    if (end < beg) { *err = "Failed to parse region: '" + reg + "' (end before start)"; return false; }
    out->beg = beg; out->end = end;
    return true;
}

// the header and the pileup's reads of [beg, end) on `contig` (dtype: index among dtypes, -1 without a match; 0 for all
// when there is at most one dtype).  false with *err set on a malformed file.
struct File {
    std::vector<Contig> contigs;
    std::vector<uint8_t> data;                   // inflated
    size_t first_record = 0;
};

inline bool open_bam(const char *path, int threads, File &f, std::string *err)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) { *err = std::string("Failed to read .bam file '") + path + "'"; return false; }
    std::vector<uint8_t> raw;
    fseek(fp, 0, SEEK_END);
    const long n = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    raw.resize(n > 0 ? (size_t)n : 0);
    const size_t got = n > 0 ? fread(raw.data(), 1, (size_t)n, fp) : 0;
    fclose(fp);
    raw.resize(got);
    if (!bgzf_inflate(raw, threads, f.data, err)) return false;
    const std::vector<uint8_t> &d = f.data;
    if (d.size() < 12 || memcmp(d.data(), "BAM\1", 4) != 0) { *err = "not a BAM file (no BAM magic)"; return false; }
    const int64_t l_text = rd32(d.data() + 4);
    if (l_text < 0 || (size_t)l_text > d.size() - 12) { *err = "truncated BAM header"; return false; }
    size_t at = 8 + (size_t)l_text;
    const int64_t n_ref = rd32(d.data() + at);
    at += 4;
    if (n_ref < 0) { *err = "bad BAM header (negative reference count)"; return false; }
    for (int64_t k = 0; k < n_ref; ++k) {
        // l_name, the name and l_ref: 8 bytes at least before the name's length is even compared with what is left
        if (d.size() - at < 8) { *err = "truncated BAM header (inside the reference list)"; return false; }
        const int64_t ln = rd32(d.data() + at);
        if (ln < 1 || (size_t)ln > d.size() - at - 8) { *err = "truncated or bad BAM reference list"; return false; }
        f.contigs.push_back(Contig{std::string((const char *)d.data() + at + 4, (size_t)ln - 1), rd32(d.data() + at + 4 + ln)});
        at += 8 + (size_t)ln;
    }
    f.first_record = at;
    return true;
}

inline bool region_reads(const File &f, const Region &reg, const std::vector<std::string> &dtypes, Reads &R, std::string *err)
{
    int tid = -1;
    for (size_t k = 0; k < f.contigs.size(); ++k) if (f.contigs[k].name == reg.contig) { tid = (int)k; break; }
    if (tid < 0) { *err = "contig '" + reg.contig + "' is not in the BAM header"; return false; }
    const std::vector<uint8_t> &d = f.data;
    struct Keep { size_t at; int32_t pos; };
    std::vector<Keep> keep;
    char msg[160];
    for (size_t at = f.first_record; at < d.size();) {
        if (d.size() - at < 4) { snprintf(msg, sizeof msg, "truncated BAM record at byte %zu", at); *err = msg; return false; }
        const int64_t bs = rd32(d.data() + at);
        if (bs < 32 || (size_t)bs > d.size() - at - 4) { snprintf(msg, sizeof msg, "truncated or bad BAM record at byte %zu", at); *err = msg; return false; }
        const uint8_t *p = d.data() + at + 4;
        const int32_t rtid = rd32(p), pos = rd32(p + 4);
        const int l_rn = p[8], mapq = p[9], n_cig = rd16(p + 12), flag = rd16(p + 14);
        const int64_t l_seq = rd32(p + 16);
        if (l_seq < 0 || l_rn < 1 || 32 + l_rn + 4ll * n_cig + (l_seq + 1) / 2 + l_seq > bs) {
            snprintf(msg, sizeof msg, "bad BAM record at byte %zu", at);
            *err = msg;
            return false;
        }
        if (rtid == tid && !(flag & (0x4 | 0x100 | 0x200 | 0x400 | 0x800)) && mapq >= 1 && pos >= 0) {
            const uint8_t *c = p + 32 + l_rn;
            int64_t rlen = 0;
            for (int k = 0; k < n_cig; ++k) { const uint32_t w = rdu32(c + 4 * k); if (ref_op((int)(w & 15u))) rlen += w >> 4; }
            if (pos + rlen > reg.beg && pos < reg.end) keep.push_back(Keep{at, pos});
        }
        at += 4 + (size_t)bs;
    }
    std::stable_sort(keep.begin(), keep.end(), [](const Keep &a, const Keep &b) { return a.pos < b.pos; });
    for (const Keep &k : keep) {
        const uint8_t *p = d.data() + k.at + 4, *e = p + rd32(d.data() + k.at);
        const int l_rn = p[8], n_cig = rd16(p + 12), flag = rd16(p + 14);
        const int64_t l_seq = rd32(p + 16);
        const uint8_t *c = p + 32 + l_rn, *sq = c + 4 * n_cig, *ql = sq + (l_seq + 1) / 2, *aux = ql + l_seq;
        R.pos.push_back(k.pos);
        for (int j = 0; j < n_cig; ++j) R.cigar.push_back(rdu32(c + 4 * j));
        R.cigar_off.push_back((int64_t)R.cigar.size());
        R.seq_boff.push_back((int64_t)R.seq.size());
        R.seq.insert(R.seq.end(), sq, sq + (l_seq + 1) / 2);
        R.qual.insert(R.qual.end(), ql, ql + l_seq);
        R.seq_off.push_back(R.seq_off.back() + l_seq);
        R.rev.push_back((uint8_t)((flag >> 4) & 1));
        int8_t dt = 0;
        if (dtypes.size() > 1) {
            std::string v;
            dt = -1;
            if (aux_z(aux, e, "DT", &v))
                for (size_t j = 0; j < dtypes.size(); ++j) if (dtypes[j] == v) { dt = (int8_t)j; break; }
        }
        R.dtype.push_back(dt);
        R.names.emplace_back((const char *)p + 32, (size_t)l_rn - 1);
    }
    return true;
}

// The dbg driver's reads: every record of [beg, end) on `contig` in file order, as htslib's region iterator returns them
// (UPSTREAM: pos < end and bam_endpos > beg, bam_endpos = pos + reference length, or pos + 1 when unmapped or of length 0),
// with no flag or mapq filter.  Per record: the BAM name, flag, pos, bam_endpos, CIGAR words, l_seq, packed bases and
// qualities (pointers into f.data).
struct Record {
    const char *name; int l_name;
    uint16_t flag; int32_t pos; int64_t endpos;
    const uint8_t *cigar; int n_cigar;
    const uint8_t *seq, *qual; int64_t l_seq;
};
inline bool region_records(const File &f, const Region &reg, std::vector<Record> &out, std::string *err)
{
    int tid = -1;
    for (size_t k = 0; k < f.contigs.size(); ++k) if (f.contigs[k].name == reg.contig) { tid = (int)k; break; }
    if (tid < 0) { *err = "contig '" + reg.contig + "' is not in the BAM header"; return false; }
    const std::vector<uint8_t> &d = f.data;
    char msg[160];
    for (size_t at = f.first_record; at < d.size();) {
        if (d.size() - at < 4) { snprintf(msg, sizeof msg, "truncated BAM record at byte %zu", at); *err = msg; return false; }
        const int64_t bs = rd32(d.data() + at);
        if (bs < 32 || (size_t)bs > d.size() - at - 4) { snprintf(msg, sizeof msg, "truncated or bad BAM record at byte %zu", at); *err = msg; return false; }
        const uint8_t *p = d.data() + at + 4;
        const int32_t rtid = rd32(p), pos = rd32(p + 4);
        const int l_rn = p[8], n_cig = rd16(p + 12), flag = rd16(p + 14);
        const int64_t l_seq = rd32(p + 16);
        if (l_seq < 0 || l_rn < 1 || 32 + l_rn + 4ll * n_cig + (l_seq + 1) / 2 + l_seq > bs) {
            snprintf(msg, sizeof msg, "bad BAM record at byte %zu", at);
            *err = msg;
            return false;
        }
        if (rtid == tid && pos >= 0 && pos < reg.end) {
            const uint8_t *c = p + 32 + l_rn;
            int64_t rlen = 0;
            if (!(flag & 0x4))
                for (int k = 0; k < n_cig; ++k) { const uint32_t w = rdu32(c + 4 * k); if (ref_op((int)(w & 15u))) rlen += w >> 4; }
            const int64_t e = pos + (rlen > 0 ? rlen : 1);
            if (e > reg.beg)
                out.push_back(Record{(const char *)p + 32, l_rn - 1, (uint16_t)flag, pos, e, c, n_cig, c + 4 * n_cig, c + 4 * n_cig + (l_seq + 1) / 2, l_seq});
        }
        at += 4 + (size_t)bs;
    }
    return true;
}

}  // namespace bam
