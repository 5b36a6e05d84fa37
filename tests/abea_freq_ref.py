"""f5c meth-freq (freq.c) restated in Python, statement by statement: get_tsv_line's strtok / atoi / strtod, the hash table as a
dict with first-insert semantics, cmp_key and the printf line.  The tests hold the library against this, and this against the
compiled reference's own outputs (tests/golden/abea_freq_reference.json)."""
import functools
import math
import re

IN_HEADERS = {
    b"chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_cpgs\tsequence\n": (1, 1),
    b"chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_motifs\tsequence\n": (1, 2),
    b"chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_cpgs\tsequence\n": (2, 1),
    b"chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_motifs\tsequence\n": (2, 2),
}
OUT_HEADERS = {1: b"chromosome\tstart\tend\tnum_cpgs_in_group\tcalled_sites\tcalled_sites_methylated\tmethylated_frequency\tgroup_sequence\n",
               2: b"chromosome\tstart\tend\tnum_motifs_in_group\tcalled_sites\tcalled_sites_methylated\tmethylated_frequency\tgroup_sequence\n"}
CORRUPTED = "Corrupted tsv file? Offending line is line number %d (1-based index)\n"
NEGATIVE_COORD = "chromosome coordinates cannot be negative. Offending line is line number %d (1-based index)\n"
NEGATIVE_COUNT = "num_cpgs cannot be negative. Offending line is line number %d (1-based index)\n"
MORE_COLUMNS = "encountered more columns than expected. Offending line is line number %d (1-based index)\n"
NO_HEADER = "Bad file format with no header?\n"


class RefExit(Exception):
    """where freq.c prints to stderr and exits with EXIT_FAILURE"""

    def __init__(self, message, line=0):
        super().__init__(message)
        self.message, self.line = message, line


def atoi(b):
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?[0-9]+)", b)
    v = int(m.group(1)) if m else 0
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31                 # (what the usual atoi gives past the range; the tests stay inside)


_FLOAT = re.compile(rb"[ \t\n\v\f\r]*([+-]?(?:inf(?:inity)?|nan|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?))", re.I)


def strtod(b):
    m = _FLOAT.match(b)
    return float(m.group(1).decode()) if m else 0.0


class _Strtok:
    def __init__(self, line):
        self.s, self.at = line.split(b"\0")[0], 0             # a C string

    def next(self, delim):
        s, i = self.s, self.at
        while i < len(s) and s[i] in delim:
            i += 1
        if i >= len(s):
            self.at = len(s)
            return None
        b = i
        while i < len(s) and s[i] not in delim:
            i += 1
        self.at = i + 1 if i < len(s) else len(s)
        return s[b:i]


def parse(text):
    """-> (version, kind, [(chromosome, start, end, llr, num_cpgs, sequence)]); RefExit where get_tsv_line or the header check exits"""
    lines = text.split(b"\n")
    lines = [l + b"\n" for l in lines[:-1]] + ([lines[-1]] if lines[-1] else [])       # getline keeps the newline
    if not lines:
        raise RefExit(NO_HEADER)
    if lines[0] not in IN_HEADERS:
        raise RefExit("Incorrect header: %s\n" % lines[0].split(b"\0")[0].decode("latin-1"))
    version, kind = IN_HEADERS[lines[0]]
    records, line_num = [], 2
    for line in lines[1:]:
        t = _Strtok(line)

        def need(delim=b"\t"):
            tok = t.next(delim)
            if tok is None:
                raise RefExit(CORRUPTED % line_num, line_num)
            return tok
        chrom = need()
        if version == 2:
            need()
        start = atoi(need())
        end = atoi(need())
        if start < 0 or end < 0:
            raise RefExit(NEGATIVE_COORD % line_num, line_num)
        need()
        llr = strtod(need())
        t.next(b"\t")
        t.next(b"\t")
        need()
        n = atoi(need())
        if n < 0:
            raise RefExit(NEGATIVE_COUNT % line_num, line_num)
        seq = need(b"\t\n")
        if t.next(b"\t\n") is not None:
            raise RefExit(MORE_COLUMNS % line_num, line_num)
        records.append((chrom, start, end, llr, n, seq))
        line_num += 1
    return version, kind, records


def cmp_key(a, b):
    if a[0] != b[0]:
        return -1 if a[0] < b[0] else 1                       # strcmp: unsigned bytes, as Python compares bytes
    if a[1] == b[1]:
        return a[2] - b[2]
    return a[1] - b[1]


def table(records, threshold=2.5, split_groups=False):
    """-> [(chromosome, start, end, group_size, called_sites, called_sites_methylated, sequence)] in output order"""
    sites = {}

    def update(key, n, is_methylated, seq):
        if key not in sites:
            sites[key] = [n, 0, 0, seq]                        # group_size, called_sites, called_sites_methylated, sequence
        s = sites[key]
        s[1] += n
        if is_methylated:
            s[2] += n

    for chrom, start, end, llr, n, seq in records:
        if math.fabs(llr) < threshold:
            continue
        is_methylated = llr > 0
        if split_groups and n > 1:
            cg_pos = seq.find(b"CG")
            first = cg_pos
            while cg_pos != -1:
                update((chrom, start + cg_pos - first, start + cg_pos - first), 1, is_methylated, b"split-group")
                cg_pos = seq.find(b"CG", cg_pos + 1)
        else:
            update((chrom, start, end), n, is_methylated, seq)
    out = []
    for key in sorted(sites, key=functools.cmp_to_key(cmp_key)):
        g, c, m, seq = sites[key]
        if c > 0:
            out.append((key[0], key[1], key[2], g, c, m, seq))
    return out


def text_of(rows, kind=1):
    out = [OUT_HEADERS[kind]]
    for chrom, start, end, g, c, m, seq in rows:
        out.append(b"%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (chrom, start, end, g, c, m, ("%.3f" % (m / c)).encode(), seq))
    return b"".join(out)


def meth_freq(text, threshold=2.5, split_groups=False):
    """freq_main on the bytes of its input -> the bytes of its output"""
    version, kind, records = parse(text)
    return text_of(table(records, threshold, split_groups), kind)


def llr_as_read(x):
    """what meth-freq reads where call-methylation printed the double x"""
    return float("%.2f" % x)
