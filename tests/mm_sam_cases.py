"""Hand-built cases for the mm sam stage (tests/mm_sam_ref.py is the restatement): regions whose records and CIGAR words are given
directly, no DP needed, chosen at the edges of a kernel that walks 64 columns and 64 words a step.  The generators assert their
own coverage."""
import functools
import random

import numpy as np

import mm_sam_ref as SR

REG_KEYS = ("id", "parent", "score", "subsc", "cnt", "as", "rid", "rev", "rs", "re", "qs", "qe", "mlen", "blen", "n_sub", "mapq", "hash", "read")
ALN_KEYS = ("rs", "re", "qs", "qe", "mlen", "blen", "n_ambi", "nm", "dp_score", "dp_max", "n_cigar", "flags", "cigar_off")

OPTION_SETS = {
    "paf_plain": {}, "paf_cs": dict(cs=1), "paf_cs_long": dict(cs=2), "paf_md": dict(md=1), "paf_eqx": dict(eqx=1), "paf_all": dict(cs=1, md=1, eqx=1),
    "sam": dict(format=1), "sam_cs": dict(format=1, cs=1), "sam_cs_long": dict(format=1, cs=2), "sam_md": dict(format=1, md=1),
    "sam_eqx": dict(format=1, eqx=1), "sam_all": dict(format=1, cs=1, md=1, eqx=1), "sam_all_long": dict(format=1, cs=2, md=1, eqx=1),
    "sam_Y": dict(format=1, cs=1, md=1, eqx=1, softclip=1),
}
SAM_SETS = [k for k, v in OPTION_SETS.items() if v.get("format")]


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def other(b, k=1):
    """a base that differs from b as a code"""
    c = SR.code(b)
    return b"ACGT"[(c + k) % 4] if c < 4 else b"ACGT"[k % 4]


def revcomp(s):
    return SR.oriented(s, 1)


class Batch:
    """One call's input, built a read at a time"""

    def __init__(self, with_qual=True):
        self.refs, self.tnames, self.reads, self.qnames, self.quals, self.rep_len = [], [], [], [], ([] if with_qual else None), []
        self.regs, self.reg_off, self.alns, self.cigar = [], [0], [], []

    def ref(self, text, name=None):
        self.refs.append(bytes(text))
        self.tnames.append(name or "ctg%d" % len(self.refs))
        return len(self.refs) - 1

    def read(self, text, name=None, rng=None):
        self.reads.append(bytes(text))
        self.qnames.append(name or "read%d" % len(self.reads))
        self.rep_len.append(3 * len(self.reads) % 50)
        if self.quals is not None:
            self.quals.append(bytes(33 + (7 * i + len(self.reads)) % 60 for i in range(len(text))))
        self.reg_off.append(self.reg_off[-1])
        return len(self.reads) - 1

    def region(self, rid, rev, rs, q0, words, own=True, flags=1, aln_over=None, **over):
        """a region of the last read: `words` [(op, len)] from column rs of contig rid and q0 of the oriented read; own: parent == id"""
        r = len(self.reads) - 1
        qlen, T, Q = len(self.reads[r]), self.refs[rid] if 0 <= rid < len(self.refs) else b"", SR.oriented(self.reads[r], rev)
        t, q, nm, amb, mlen, blen = rs, q0, 0, 0, 0, 0
        for op, ln in words:
            if op == 0:
                for i in range(ln):
                    if t + i < len(T) and q + i < qlen:
                        a, b = SR.code(T[t + i]), SR.code(Q[q + i])
                        amb += a > 3 or b > 3
                        mlen += a == b and a < 4
                        blen += a < 4 and b < 4
                        nm += a != b or a > 3
                t, q = t + ln, q + ln
            elif op == 1:
                q, nm, blen = q + ln, nm + ln, blen + ln
            elif op == 2:
                t, nm, blen = t + ln, nm + ln, blen + ln
        idx = self.reg_off[-1] - self.reg_off[-2]
        a = dict(rs=rs, re=t, qs=qlen - q if rev else q0, qe=qlen - q0 if rev else q, mlen=mlen, blen=blen, n_ambi=amb, nm=nm, dp_score=2 * mlen - 3 * nm,
                 dp_max=2 * mlen, n_cigar=len(words), flags=flags, cigar_off=len(self.cigar))
        a.update(aln_over or {})
        g = dict(id=idx, parent=idx if own else 0, score=mlen + 40, subsc=idx * 7, cnt=5 + idx, rid=rid, rev=rev, rs=max(rs - 1, 0), re=t + 1, qs=a["qs"], qe=a["qe"],
                 mlen=max(mlen - 3, 0), blen=blen + 2, n_sub=0, mapq=(60 - 11 * idx) % 61, hash=0x9e3779b9 ^ len(self.regs), read=r)
        g["as"] = 0
        g.update(over)
        self.cigar += [ln << 4 | op for op, ln in words]
        self.regs.append(g)
        self.alns.append(a)
        self.reg_off[-1] += 1
        return g, a

    def arrays(self):
        """-> the arguments of mm_sam.sam_host / sam_cpu after the parameters"""
        import genomicsbench_amd.mm_align as MA
        import genomicsbench_amd.mm_map as MM
        g, a = np.zeros(len(self.regs), MM.REG_DTYPE), np.zeros(len(self.alns), MA.ALN_DTYPE)
        for i, (r, x) in enumerate(zip(self.regs, self.alns)):
            for k in REG_KEYS:
                g[k][i] = r[k]
            for k in ALN_KEYS:
                a[k][i] = x[k]
        return (g, np.array(self.reg_off, np.int64), a, np.array(self.cigar, np.uint32), self.qnames, self.reads, self.quals, np.array(self.rep_len, np.int32),
                self.tnames, self.refs)

    def expected(self, **opts):
        return SR.sam_text(SR.params(**opts), self.regs, self.reg_off, self.alns, self.cigar, self.qnames, self.reads, self.quals, self.rep_len, self.tnames,
                           self.refs)

    def named(self):
        """(reads, refs) as validate() takes them"""
        return ([(n, s.decode("latin-1")) for n, s in zip(self.qnames, self.reads)], [(n, s.decode("latin-1")) for n, s in zip(self.tnames, self.refs)])


def compose(rng, recipe, clip5=0, clip3=0, flank=(5, 7)):
    """recipe: [("M", n, {unequal columns}) | ("I", n) | ("D", n)] -> (contig, oriented read, rs, q0, words).  An inserted base and
    the base behind a deletion are chosen so that the recipe's columns are what the texts show."""
    T, Q, words = bytearray(rand_seq(rng, flank[0])), bytearray(rand_seq(rng, clip5)), []
    rs = len(T)
    for step in recipe:
        if step[0] == "M":
            _, n, bad = step
            s = rand_seq(rng, n)
            T += s
            Q += bytes(other(b, 1 + i % 3) if i in bad else b for i, b in enumerate(s))
            words.append((0, n))
        elif step[0] == "I":
            Q += rand_seq(rng, step[1])
            words.append((1, step[1]))
        else:
            T += rand_seq(rng, step[1])
            words.append((2, step[1]))
    T += rand_seq(rng, flank[1])
    Q += rand_seq(rng, clip3)
    return bytes(T), bytes(Q), rs, clip5, words


def add(b, rng, recipe, rev=0, clip5=0, clip3=0, name=None, tname=None, **kw):
    """a contig, a read and its one region from a recipe"""
    T, Q, rs, q0, words = compose(rng, recipe, clip5, clip3)
    rid = b.ref(T, tname)
    b.read(revcomp(Q) if rev else Q, name)
    return b.region(rid, rev, rs, q0, words, **kw)


def recipes():
    """name -> recipe, at the edges of a 64-column and a 64-word step"""
    R = {}
    for n in (1, 63, 64, 65, 128, 129, 200):
        R["m%d" % n] = [("M", n, {n // 2})]
        R["m%d_clean" % n] = [("M", n, set())]
    R["edges"] = [("M", 200, {0, 62, 63, 64, 65, 199})]
    for p in (0, 62, 63, 64, 65, 199):
        R["one_at_%d" % p] = [("M", 200, {p})]
    R["pair_63_64"] = [("M", 150, {63, 64})]
    R["all_unequal_130"] = [("M", 130, set(range(130)))]
    R["all_equal_200"] = [("M", 200, set())]
    for n in (9, 10, 99, 100, 1000):
        R["run%d" % n] = [("M", 60 + n + 30, {59, 60 + n})]            # the run starts at column 60 and crosses column 64
        R["run%d_to_end" % n] = [("M", 60 + n, {59})]
        R["run%d_from_start" % n] = [("M", n + 1, {n}), ("I", 2), ("M", n, set())]
    R["gaps_at_unequal"] = [("M", 10, {9}), ("I", 3), ("M", 10, {0, 9}), ("D", 4), ("M", 10, {0})]
    R["d_over_step"] = [("M", 62, {30}), ("D", 5), ("M", 70, {1}), ("D", 70), ("M", 5, set())]
    R["i70"] = [("M", 20, {3}), ("I", 70), ("M", 20, {19})]
    R["md_across_i"] = [("M", 40, set()), ("I", 2), ("M", 40, {39}), ("I", 1), ("M", 70, set())]
    for nw in (1, 63, 64, 65, 130):
        rec = []
        for k in range(nw):
            rec.append(("M", 3 + k % 3, {1} if k % 4 == 0 else set()) if k % 2 == 0 else (("I", 1 + k % 2) if k % 4 == 1 else ("D", 1 + k % 5)))
        R["words%d" % nw] = rec
    return R


@functools.lru_cache(maxsize=None)
def edge_batch(with_qual=True):
    """every recipe on both strands, with clips of 0 and above 0 on either side"""
    rng, b = random.Random(20), Batch(with_qual)
    clips = [(0, 0), (4, 0), (0, 6), (3, 5)]
    for i, (name, rec) in enumerate(sorted(recipes().items())):
        for rev in (0, 1):
            c5, c3 = clips[(i + rev) % 4]
            add(b, rng, rec, rev, c5, c3, name="%s_%s" % (name, "rf"[rev == 0]))
    assert len(b.reads) == 2 * len(recipes()) and max(a["n_cigar"] for a in b.alns) == 130
    return b


@functools.lru_cache(maxsize=None)
def letters_batch():
    """N, IUPAC letters and lower case in read and contig, N against N included, names of 1 and 300 bytes"""
    b = Batch()
    T = b"ACGTNNRYacgtnACGTKMacgGTTAACCGGTT"
    #     0123456789...
    rid = b.ref(T, "c")
    Q = b"ACGTNARCacgtAACGTKAacgGTTAACCGGTT"
    for rev in (0, 1):
        b.read(revcomp(Q) if rev else Q, "q" if rev == 0 else "n" * 300)
        b.region(rid, rev, 0, 0, [(0, len(T))])
    rid2 = b.ref(b"ttNNacgtRRnnACGT" * 9, "t" * 300)
    Q2 = (b"ttNNacgtRRnnACGT" * 9)[:70] + b"NNnn" + (b"ttNNacgtRRnnACGT" * 9)[70 + 6:]
    for rev in (0, 1):
        b.read((b"xy" + revcomp(Q2)) if rev else (Q2 + b"yx"), "iupac%d" % rev)
        b.region(rid2, rev, 0, 0, [(0, 70), (1, 4), (2, 6), (0, len(Q2) - 74)])
    return b


@functools.lru_cache(maxsize=None)
def kinds_batch(with_qual=True):
    """per read: a primary alone; a primary with a supplementary and a secondary; no region; only regions that do not print; a
    second supplementary; a first region that does not print in front of the primary"""
    rng, b = random.Random(21), Batch(with_qual)
    T1, Q1, rs1, q1, w1 = compose(rng, [("M", 80, {5, 64}), ("I", 2), ("M", 30, set())], 3, 4)
    r1 = b.ref(T1)
    b.read(Q1, "alone")
    b.region(r1, 0, rs1, q1, w1)
    # one read, three contigs: the read's first part on contig A forward, its second part on contig B reverse, all of it on C
    partA = [("M", 70, {10}), ("D", 3), ("M", 20, set())]
    partB = [("M", 66, {63, 64}), ("I", 1), ("M", 9, {0})]
    TA, QA, rsA, _, wA = compose(rng, partA)
    TB, QB, rsB, _, wB = compose(rng, partB)
    read = QA + b"GG" + revcomp(QB) + b"T"                                  # stored read: A forward, then B as its reverse complement
    rA, rB = b.ref(TA, "ctgA"), b.ref(TB, "ctgB")
    rC = b.ref(b"AC" + QA + b"TT")
    for name, order in (("three", "ABC"), ("three_supp_first_secondary_last", "BCA")):
        b.read(read, name)
        for k in order:
            if k == "A":
                b.region(rA, 0, rsA, 0, wA)
            elif k == "B":
                b.region(rB, 1, rsB, 1, wB)                                 # oriented: T' + QB + CC + rc(QA): B starts at 1
            else:
                b.region(rC, 0, 2, 0, [(0, len(QA))], own=False)
    b.read(rand_seq(rng, 40), "none")
    b.read(rand_seq(rng, 33), "silent")
    b.region(rA, 0, 0, 0, [(0, 10)], flags=0)
    b.region(rA, 0, 0, 0, [(0, 10)], flags=1 | 64)
    b.region(rA, 1, 0, 0, [(0, 10)], flags=1 | 32)
    b.read(read, "silent_then_three")
    b.region(rA, 0, rsA, 0, wA, flags=0)
    b.region(rB, 1, rsB, 1, wB)
    b.region(rA, 0, rsA, 0, wA)
    b.region(rC, 0, 2, 0, [(0, len(QA))], own=False)
    b.read(read, "no_target")
    b.region(-1, 0, 0, 0, [(0, 10)], flags=0)
    assert [b.reg_off[i + 1] - b.reg_off[i] for i in range(len(b.reads))] == [1, 3, 3, 0, 3, 4, 1]
    return b


@functools.lru_cache(maxsize=None)
def malformed_batch():
    """words that run past the read or the contig, ops above 2, a start past the end: cut, never read past"""
    rng, b = random.Random(22), Batch()
    T, Q = rand_seq(rng, 100), rand_seq(rng, 90)
    rid = b.ref(T)
    b.read(Q, "past_read")
    b.region(rid, 0, 5, 10, [(0, 50), (1, 5), (0, 200), (2, 7), (1, 3), (0, 4), (2, 500)])
    b.read(Q, "past_contig")
    b.region(rid, 1, 60, 0, [(0, 30), (2, 30), (0, 5), (1, 9), (1, 500), (0, 1)])
    b.read(Q, "odd_ops")
    b.region(rid, 0, 0, 0, [(0, 20), (3, 10), (7, 5), (0, 10), (9, 1), (15, 2)])
    b.read(Q, "start_past_end")
    b.region(rid, 0, 0, 0, [(0, 20), (2, 3)], aln_over=dict(rs=4000, qs=95, qe=2000))
    b.read(Q, "many_cut")
    b.region(rid, 0, 90, 80, [(0, 5)] * 70 + [(2, 2)] * 70 + [(1, 3)] * 70)
    return b


def same(got, want):
    """the text, the line offsets, the counts and the reported need of a call equal to the restatement's"""
    if got["text"] != want["text"]:
        gl, wl = got["text"].split(b"\n"), want["text"].split(b"\n")
        k = next((i for i, (x, y) in enumerate(zip(gl, wl)) if x != y), min(len(gl), len(wl)))
        raise AssertionError("line %d of %d / %d:\n got  %r\n want %r" % (k, len(gl), len(wl), gl[k:k + 1], wl[k:k + 1]))
    assert list(got["line_off"]) == list(want["line_off"]) and got["counts"] == tuple(want["counts"]) and got["n_text"] == len(want["text"])


def all_batches():
    return dict(edges=edge_batch(True), edges_noqual=edge_batch(False), letters=letters_batch(), kinds=kinds_batch(True), kinds_noqual=kinds_batch(False),
                malformed=malformed_batch())
