"""Hand-built k-mer counting calls that sit on the edges of csrc/kmer_kernels.hip: reads whose position counts end on, before
and behind a unit of the count pass, at every start residue of its 16-byte words; bytes above 3; palindromes and k-mers
given by their reverse strand alone; read counts around the unit kernel's 1024 threads with unit-less reads in awkward
places; counters on both sides of a lane's, a wavefront's, a round's and a workgroup's share of the sweeps and of the
selection scan's second trip; histogram bins at the clamp; selections cut at chosen places; k-mers on both sides of the
slice borders of k = 16 and 17.  Builders only: no GPU.  Every case carries its expectation (a dict canonical code -> count,
from which stats, histogram and selection follow without tests/kmer_ref.py) and a `facts` dict that says what the case is
named for; tests/test_kmer_edges_cpu.py checks both on the restatement, tests/test_kmer_edges_gpu.py runs the same cases on
the device.

The kernels' unit size, sweep split and slice rule (csrc/kmer_split.h) are restated here in plain Python, so that the cases
get their boundaries by computation: a change of them has to be repeated here, and the CPU test (which holds the
restatement against the header, host build) then says which claim no longer holds."""
import collections
import functools

import numpy as np

from genomicsbench_amd import kmer as K

# ------------------------------------------------------------------------------------------------- the split, restated
KC_CHUNK = 256                           # positions per unit of the count pass
KC_THREADS = 256
KC_SWEEP = KC_THREADS * 4                # counters a sweep workgroup covers per round
KC_MAX_BLOCKS = 2048
KC_SLICE = 1 << 30
UNITS_THREADS = 1024                     # kmer_units_kernel is one workgroup of this many threads
SCAN_TRIP = 1024                         # workgroup counts kmer_sel_scan_kernel scans per trip
LANE, WAVE = 4, 64 * 4                   # counters a lane and a wavefront of the sweeps take per round
WORD = 16                                # the count pass reads the bases as aligned words of this many bytes


def sweep_split(n):
    """(nb, per): the sweeps' workgroups over a slice of n counters, and the counters of each"""
    rounds = -(-n // KC_SWEEP)
    per = -(-rounds // KC_MAX_BLOCKS) * KC_SWEEP
    return -(-n // per), per


def slice_rule(k):
    """(slice_n, n_slices) of the 4^k counters"""
    slice_n = min(4 ** k, KC_SLICE)
    return slice_n, 4 ** k // slice_n


def read_units(length, k):
    return (max(0, length - k) + KC_CHUNK - 1) // KC_CHUNK


def unit_share(n_reads):
    """reads per thread of kmer_units_kernel"""
    return -(-n_reads // UNITS_THREADS)


def workgroup_of(code, k):
    """the sweep workgroup that holds a code's counter, numbered through the slices"""
    slice_n, _ = slice_rule(k)
    nb, per = sweep_split(slice_n)
    return code // slice_n * nb + code % slice_n // per


def cut_kind(c1, c2, k):
    """what lies between two codes in the sweeps: the narrowest share of work that holds both"""
    slice_n, _ = slice_rule(k)
    per = sweep_split(slice_n)[1]
    for kind, unit in (("lane", LANE), ("lanes", WAVE), ("wave", KC_SWEEP), ("round", per), ("workgroup", slice_n)):
        if c1 // unit == c2 // unit:
            return kind
    return "slice"


# ------------------------------------------------------------------------------------------------- codes
def revcomp(code, k):
    r = 0
    for _ in range(k):
        r = r << 2 | 3 - (code & 3)
        code >>= 2
    return r


def is_canonical(code, k):
    return code <= revcomp(code, k)


def bases(code, k):
    return np.array([code >> 2 * (k - 1 - i) & 3 for i in range(k)], dtype=np.uint8)


def code_of(text):
    return int(text.translate(str.maketrans("ACGT", "0123")), 4)


def _canonical_mask(c, k):
    r, f = np.zeros_like(c), c.copy()
    for _ in range(k):
        r = r << np.uint64(2) | np.uint64(3) - (f & np.uint64(3))
        f = f >> np.uint64(2)
    return c <= r


def canonical_codes(k, lo, hi):
    """the canonical codes in [lo, hi), ascending, as Python ints"""
    c = np.arange(lo, hi, dtype=np.uint64)
    return [int(x) for x in c[_canonical_mask(c, k)]]


def canonical_below(k, code):
    """the largest canonical code <= code"""
    hi = code + 1
    while hi > 0:
        got = canonical_codes(k, max(0, hi - (1 << 16)), hi)
        if got:
            return got[-1]
        hi -= 1 << 16
    raise ValueError("no canonical code at or below %d" % code)


def canonical_above(k, code):
    """the smallest canonical code >= code"""
    lo = code
    while lo < 4 ** k:
        got = canonical_codes(k, lo, min(4 ** k, lo + (1 << 16)))
        if got:
            return got[0]
        lo += 1 << 16
    raise ValueError("no canonical code at or above %d" % code)


# ------------------------------------------------------------------------------------------------- expectation
def expect(table, n_hist, min_freq, max_freq):
    """(stats, hist, kmers, counts) as genomicsbench_amd.kmer.count_host returns them, the whole selection, from a dict
    canonical code -> count alone (include/gbx.h: bin min(count, n_hist - 1); selected: min_freq != 0, count >= min_freq
    and, with max_freq != 0, count <= max_freq; ascending code)"""
    codes = sorted(table)
    counts = [table[c] for c in codes]
    hist = np.zeros(n_hist, dtype=np.int64)
    if n_hist:
        for c in counts:
            hist[min(c, n_hist - 1)] += 1
    sel = [(c, n) for c, n in zip(codes, counts) if min_freq != 0 and n >= min_freq and (max_freq == 0 or n <= max_freq)]
    stats = dict(n_positions=sum(counts), n_distinct=len(codes), n_ge16=sum(n >= 16 for n in counts),
                 max_count=max(counts) if counts else 0, n_selected=len(sel))
    return stats, hist, np.array([c for c, _ in sel], dtype=np.uint64), np.array([n for _, n in sel], dtype=np.uint32)


_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_DIGIT = bytes.maketrans(b"ACGT", b"0123")


def text_table(seqs, k):
    """canonical code -> count of the k-mers at positions 0 .. len - k - 1 of every sequence (ACGT bytes), by text: the
    smaller of the window and its reversed complement ('A' < 'C' < 'G' < 'T' as bytes and as codes)"""
    cnt = collections.Counter()
    for s in seqs:
        for p in range(len(s) - k):
            w = s[p:p + k]
            cnt[min(w, w.translate(_COMP)[::-1])] += 1
    return {int(w.translate(_DIGIT), 4): n for w, n in cnt.items()}


def read_texts(reads):
    """the reads of a KmerReadSet as ACGT bytes, from the low two bits of their bytes of enc"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [acgt[reads.enc[o:o + n] & 3].tobytes() for o, n in zip(reads.read_off.tolist(), reads.read_len.tolist())]


def merged(*tables):
    out = collections.Counter()
    for t in tables:
        out.update(t)
    return dict(out)


class Case:
    def __init__(self, name, family, k, reads, table, n_hist=32, min_freq=1, max_freq=0, sel_cap=None, facts=None, seqs=None):
        self.name, self.family, self.k, self.reads, self.table = name, family, k, reads, dict(table)
        self.n_hist, self.min_freq, self.max_freq = n_hist, min_freq, max_freq
        self._cap = sel_cap
        self.facts = facts or {}
        self.seqs = seqs                 # laid_out cases: the reads' text as the builder made it

    @functools.lru_cache(maxsize=None)
    def want(self):
        """the whole selection, whatever sel_cap is"""
        return expect(self.table, self.n_hist, self.min_freq, self.max_freq)

    @property
    def need(self):
        return self.want()[0]["n_selected"]

    @property
    def sel_cap(self):
        return self.need if self._cap is None else self._cap

    def params(self):
        return dict(n_hist=self.n_hist, min_freq=self.min_freq, max_freq=self.max_freq)

    def but(self, name, family=None, facts=None, **kw):
        """the same reads under another name, with other parameters"""
        c = Case(name, family or self.family, self.k, self.reads, self.table, self.n_hist, self.min_freq, self.max_freq, self._cap,
                 dict(self.facts) if facts is None else facts, self.seqs)
        for f, v in kw.items():
            setattr(c, "_cap" if f == "sel_cap" else f, v)
        return c


# ------------------------------------------------------------------------------------------------- the two builders
def planted_reads(k, table, strand="both", salt=0):
    """sum(counts) reads of k + 1 bases, each contributing exactly its first k-mer (the last window of a read is not
    counted): copy i of a code is the code itself (i even) or its reverse complement (i odd) - strand="rev": always the
    reverse complement - and the last base, which no counted window holds, varies."""
    out, j = [], salt
    for code in sorted(table):
        n = table[code]
        if not (isinstance(n, int) and n >= 1 and 0 <= code < 4 ** k):
            raise ValueError("planted: code %r, count %r" % (code, n))
        if not is_canonical(code, k):
            raise ValueError("planted: %d is not canonical for k = %d (its reverse complement is %d)" % (code, k, revcomp(code, k)))
        both = bases(code, k), bases(revcomp(code, k), k)
        for i in range(n):
            out.append(np.append(both[1 if strand == "rev" else i & 1], np.uint8(j & 3)))
            j += 1
    return out


def planted(k, table, **kw):
    return K.KmerReadSet.from_codes(planted_reads(k, table, **kw))


def laid_out(k, specs, fill="zeros", seed=0, tail=5):
    """specs: (len, start residue mod 16 or None, gap bytes) per read -> (KmerReadSet, the reads' texts).  A read starts `gap`
    bytes behind the end of what is laid out so far, moved on to the next offset with the asked residue; a negative gap (residue
    None) starts it inside the reads before it, whose bytes it shares.  Bytes that belong to no read are zeros, or ("hostile")
    random codes 1..3 that would make other k-mers if read, or ("mixed") one kind and the other in turn; `tail` of them end enc."""
    rng = np.random.default_rng(seed)
    place, cur = [], 0
    for length, residue, gap in specs:
        start = cur + gap
        if residue is not None:
            start += (residue - start) % WORD
        if start < 0 or (gap < 0 and residue is not None):
            raise ValueError("laid_out: %r" % ((length, residue, gap),))
        place.append((start, length, cur))
        cur = max(cur, start + length)
    enc = np.zeros(cur + tail, dtype=np.uint8)
    edges = [p[2] for p in place] + [cur]
    for i, (start, length, was) in enumerate(place):
        if start > was and (fill == "hostile" or (fill == "mixed" and i & 1)):
            enc[was:start] = rng.integers(1, 4, start - was)
        new = max(start, was)                                          # a read that starts inside others keeps their bytes
        enc[new:start + length] = rng.integers(0, 4, max(0, start + length - new))
    if tail and fill != "zeros":
        enc[cur:] = rng.integers(1, 4, tail)
    assert edges[-1] == cur
    reads = K.KmerReadSet(enc, np.array([p[0] for p in place], dtype=np.int64), np.array([p[1] for p in place], dtype=np.int32))
    return reads, read_texts(reads)


def with_junk(case, name, seed):
    """the same call with every byte of enc as code | junk << 2, junk random in 0..63: the kernels use the low two bits"""
    rng = np.random.default_rng(seed)
    r = case.reads
    junk = rng.integers(0, 64, r.enc.size).astype(np.uint8)
    reads = K.KmerReadSet(r.enc | junk << 2, r.read_off, r.read_len)
    return Case(name, "high_bits", case.k, reads, case.table, case.n_hist, case.min_freq, case.max_freq, case._cap,
                dict(case.facts, junk_of=case.name), case.seqs)


# ------------------------------------------------------------------------------------------------- chunk_word
DELTAS = (1, 2, 255, 256, 257, 511, 512, 513)        # len - k: one position, and the unit's ends from both sides


def chunk_word_cases():
    out = []
    for k, fills in ((1, ("zeros", "hostile")), (2, ("zeros", "hostile")), (9, ("zeros", "hostile")), (16, ("mixed",)), (17, ("mixed",))):
        for fill in fills:
            specs = [(k + d, res, (i + res) % 3) for i, d in enumerate(DELTAS) for res in range(WORD)]
            reads, seqs = laid_out(k, specs, fill, seed=100 + k)
            out.append(Case("chunk_word_k%d_%s" % (k, fill), "chunk_word", k, reads, text_table(seqs, k), n_hist=64, min_freq=2, max_freq=40,
                            seqs=seqs, facts=dict(residues={d: list(range(WORD)) for d in DELTAS}, fill=fill)))
    k = 3
    reads, seqs = laid_out(k, [(40, 0, 0), (7, 5, 3), (16, 0, 1), (4, 12, 0), (5, 3, 2)], "hostile", seed=120)
    out.append(Case("chunk_word_one_word", "chunk_word", k, reads, text_table(seqs, k), seqs=seqs, facts=dict(one_word=[1, 2, 3, 4], fill="hostile")))
    k = 9
    reads, seqs = laid_out(k, [(300, 3, 0), (k + 256, 7, 2), (k + 257, 9, 0)], "hostile", seed=121, tail=0)
    out.append(Case("chunk_word_enc_end", "chunk_word", k, reads, text_table(seqs, k), seqs=seqs, facts=dict(enc_end=True, fill="hostile")))
    reads, seqs = laid_out(k, [(300, 5, 2), (400, None, -120), (50, None, -50), (k + 256, None, -(k + 256))], "hostile", seed=122)
    out.append(Case("chunk_word_overlap", "chunk_word", k, reads, text_table(seqs, k), seqs=seqs, facts=dict(overlap=[(0, 1), (1, 2), (1, 3)], fill="hostile")))
    return out


# ------------------------------------------------------------------------------------------------- sweep
COUNTS = (1, 2, 15, 16, 17)              # the summary's two thresholds (bin 1 in a register, >= 16) from both sides


def boundary_pairs(k):
    """(what, unit, b, lo, hi): the canonical codes nearest below and at the first counter b of a lane's, a wavefront's, a
    round's, a workgroup's share and of the selection scan's second trip, where the slice has them"""
    slice_n, _ = slice_rule(k)
    nb, per = sweep_split(slice_n)
    want = [("lane", LANE, LANE * 6 if slice_n > LANE * 6 else LANE), ("wave", WAVE, WAVE), ("round", KC_SWEEP, KC_SWEEP), ("workgroup", per, per),
            ("workgroup", per, canonical_below(k, 4 ** k - 1) % slice_n // per * per), ("scan", SCAN_TRIP * per, SCAN_TRIP * per)]
    out = []
    for what, unit, b in want:
        if 0 < b < slice_n and (what, b) not in [(o[0], o[2]) for o in out]:
            out.append((what, unit, b, canonical_below(k, b - 1), canonical_above(k, b)))
    return out


@functools.lru_cache(maxsize=None)
def sweep_table(k):
    """-> (table, facts): counts COUNTS in turn on the boundary codes of k, on the first and the last canonical code and on
    the lane mates of the lane pair's upper code"""
    pairs = boundary_pairs(k)
    last = canonical_below(k, 4 ** k - 1)
    codes = {0, last}
    for _, _, _, lo, hi in pairs:
        codes |= {lo, hi}
    lane_hi = [p[4] for p in pairs if p[0] == "lane"]
    if lane_hi:
        codes |= set(canonical_codes(k, lane_hi[0], lane_hi[0] // LANE * LANE + LANE))
    table = {c: COUNTS[i % len(COUNTS)] for i, c in enumerate(sorted(codes))}
    return table, dict(pairs=pairs, last_canonical=last)


SWEEP_SPLITS = {1: (1, 1024), 2: (1, 1024), 6: (4, 1024), 11: (2048, 2048)}      # (nb, per) the family is built for


def sweep_cases():
    out = []
    for k in (1, 2, 6, 11):
        table, facts = sweep_table(k)
        out.append(Case("sweep_k%d" % k, "sweep", k, planted(k, table), table, facts=dict(facts, split=SWEEP_SPLITS[k])))
    k = 6
    base, facts = sweep_table(k)
    for n_hist in (2, 3, 17, 4096):
        free = [c for c in canonical_codes(k, 100, 400) if c not in base][:4]
        at = {c: n for c, n in zip(free, (n_hist - 2, n_hist - 1, n_hist, n_hist + 5)) if n > 0}
        table = merged(base, at)
        out.append(Case("sweep_hist_%d" % n_hist, "sweep", k, planted(k, table), table, n_hist=n_hist,
                        facts=dict(facts, split=SWEEP_SPLITS[k], bins=sorted(at.values()))))
    return out


# ------------------------------------------------------------------------------------------------- select
def cut_between(table, k, min_freq, max_freq, kind):
    """(sel_cap, c1, c2): the first place in the selection where cut_kind(last kept, first dropped) is `kind`"""
    sel = [int(c) for c in expect(table, 0, min_freq, max_freq)[2]]
    for i in range(1, len(sel)):
        if cut_kind(sel[i - 1], sel[i], k) == kind:
            return i, sel[i - 1], sel[i]
    raise ValueError("no %s cut in the selection" % kind)


def select_cases():
    out = []
    k = 11
    table, facts = sweep_table(k)
    reads = planted(k, table)
    facts = dict(facts, split=SWEEP_SPLITS[k])
    for lo, hi in ((1, 0), (2, 2), (2, 16), (16, 0), (3, 2), (0, 5), (1, 2 ** 32 - 1)):
        out.append(Case("select_min%d_max%d" % (lo, hi), "select", k, reads, table, min_freq=lo, max_freq=hi, facts=facts))
    need = len(table)
    for what, cap in (("0", 0), ("1", 1), ("need_less_1", need - 1), ("need", need), ("need_and_1", need + 1)):
        out.append(Case("select_cap_%s" % what, "select", k, reads, table, sel_cap=cap, facts=dict(facts, need=need)))
    for kind in ("lane", "wave", "round", "workgroup"):
        cap, c1, c2 = cut_between(table, k, 1, 0, kind)
        out.append(Case("select_cut_%s" % kind, "select", k, reads, table, sel_cap=cap, facts=dict(facts, cut=(kind, c1, c2))))
    _, per = sweep_split(slice_rule(k)[0])
    wg = 1500                                                          # every selected k-mer in one workgroup, in both its rounds
    inside = canonical_codes(k, wg * per, (wg + 1) * per)
    chosen = inside[:3] + inside[len(inside) // 2 - 2:len(inside) // 2 + 2] + inside[-3:]
    noise = [0, canonical_below(k, wg * per - 1), canonical_above(k, (wg + 1) * per), canonical_below(k, 4 ** k - 1)]
    table = merged({c: 3 for c in chosen}, {c: 1 for c in noise})
    out.append(Case("select_one_workgroup", "select", k, planted(k, table), table, min_freq=2, facts=dict(workgroups=[wg])))
    wgs = list(range(0, KC_MAX_BLOCKS, 64))                            # a selected k-mer in every 64th workgroup only
    chosen = [canonical_above(k, w * per + 1000 + w // 2) for w in wgs]
    noise = [canonical_above(k, (w + 1) * per + 3) for w in wgs]
    table = merged({c: 2 for c in chosen}, {c: 1 for c in noise})
    one = Case("select_every_64th", "select", k, planted(k, table), table, min_freq=2, facts=dict(workgroups=wgs))
    cap = SCAN_TRIP // 64 + 1                                          # the first of the scan's second trip is the last kept
    out += [one, one.but("select_every_64th_cut", sel_cap=cap, facts=dict(workgroups=wgs, cut=("workgroup", chosen[cap - 1], chosen[cap])))]
    return out


# ------------------------------------------------------------------------------------------------- strands
def strands_cases():
    out = []
    for k in (2, 10, 16):
        h = k // 2
        halves = ["A" * h, "T" * h, ("CG" * h)[:h], ("GATTACA" * 3)[:h]]
        pals = sorted({code_of(s) << 2 * h | revcomp(code_of(s), h) for s in halves})
        rev_only = [c for c in (canonical_above(k, 4 ** k // 3), canonical_above(k, 4 ** k // 5 + 1), canonical_below(k, 4 ** k // 2))
                    if c not in pals and c != revcomp(c, k)]
        homo = [np.zeros(k + 3, dtype=np.uint8), np.full(k + 3, 3, dtype=np.uint8)]       # all-A and all-T: one counter, both strands
        for tag, odd_first in (("a", 1), ("b", 0)):
            pt = {c: 3 + (i + odd_first) % 2 + 2 * (i // 2) for i, c in enumerate(pals)}
            rt = {c: 1 + i for i, c in enumerate(rev_only)}
            reads = K.KmerReadSet.from_codes(planted_reads(k, pt) + planted_reads(k, rt, strand="rev", salt=1) + homo)
            out.append(Case("strands_k%d_%s" % (k, tag), "strands", k, reads, merged(pt, rt, {0: 6}), n_hist=8,
                            facts=dict(palindromes={c: n & 1 for c, n in pt.items()}, reverse_only=rev_only, homopolymers=(len(reads.read_len) - 2, len(reads.read_len) - 1))))
    return out


# ------------------------------------------------------------------------------------------------- units
def units_cases():
    out = []
    k = 9
    pool = [c for c in canonical_codes(k, 1, 60000)][::7]
    for n in (1, 1023, 1024, 1025, 2049, 3000):
        share = unit_share(n)
        slots = ["P"] * n
        facts = dict(n_reads=n, share=share)
        if n > 1:
            run = (n // 2, share + 2)                                  # a run longer than a thread's share, in the middle
            singles = [2, 7 * share, n - 3]                            # one at a time between reads that have units
            for i in [0, n - 1] + singles + list(range(run[0], run[0] + run[1])):
                slots[i] = "E"
            slots[4] = "L"                                             # three units among one-unit reads
            facts.update(run=run, singles=singles, long=4)
        n_planted = slots.count("P")
        table = {c: 2 for c in pool[:n_planted // 2]}
        if n_planted & 1:
            table[pool[n_planted // 2]] = 1
        plant = iter(planted_reads(k, table))
        empty = (0, k - 1, k)
        reads, e = [], 0
        for s in slots:
            if s == "P":
                reads.append(next(plant))
            elif s == "L":
                reads.append(np.zeros(k + 600, dtype=np.uint8))
            else:
                reads.append(np.full(empty[e % 3], 1 + e % 3, dtype=np.uint8))
                e += 1
        if n > 1:
            reads[0], reads[-1] = reads[0][:0], np.full(k, 2, dtype=np.uint8)          # length 0 first, length k last
            table = merged(table, {0: 600})
        out.append(Case("units_%d_reads" % n, "units", k, K.KmerReadSet.from_codes(reads), table, n_hist=8, min_freq=2, facts=facts))
    return out


# ------------------------------------------------------------------------------------------------- slices
def slices_cases():
    out = []
    k = 16
    slice_n, n_slices = slice_rule(k)
    borders = [(j * slice_n, canonical_below(k, j * slice_n - 1), canonical_above(k, j * slice_n)) for j in range(1, n_slices)]
    top = canonical_below(k, 4 ** k - 1)
    codes = sorted({0, top} | {c for b in borders for c in b[1:]})
    table = {c: 1 + i % 3 for i, c in enumerate(codes)}
    facts = dict(borders=borders, last_canonical=top, top_text="T" * 8 + "A" * 8)
    out.append(Case("slices_k16_borders", "slices", k, planted(k, table), table, n_hist=8, facts=facts))
    (_, below1, at1), (_, below2, at2), (_, below3, at3) = borders
    mid1 = canonical_above(k, slice_n + slice_n // 2)
    table = merged({0: 2, below1: 2}, {at1: 2, mid1: 3, below2: 2}, {at2: 1, below3: 1}, {at3: 2, top: 2})
    gap = Case("slices_k16_gap", "slices", k, planted(k, table), table, n_hist=8, min_freq=2, facts=dict(facts, slices_selected=[2, 3, 0, 2]))
    out += [gap, gap.but("slices_k16_cut_in_1", sel_cap=3, facts=dict(gap.facts, cut=("workgroup", at1, mid1))),
            gap.but("slices_k16_cut_end_1", sel_cap=5, facts=dict(gap.facts, cut=("slice", below2, at3)))]
    k = 17
    slice_n, n_slices = slice_rule(k)
    top = code_of("T" * 8 + "C" + "A" * 8)
    table = {0: 2, canonical_above(k, 7 * slice_n): 3, canonical_below(k, 8 * slice_n - 1): 1, top: 2}
    st = Case("slices_k17_stats", "slices", k, planted(k, table), table, n_hist=8, min_freq=0,
              facts=dict(last_canonical=top, slices_held=[0, 7, 15]))
    out += [st, st.but("slices_k17_select", min_freq=2, facts=dict(st.facts, slices_selected=[1] + [0] * 6 + [1] + [0] * 7 + [1]))]
    return out


# ------------------------------------------------------------------------------------------------- high_bits
def high_bits_cases(chunk_word, sweep):
    by = {c.name: c for c in chunk_word + sweep}
    return [with_junk(by["chunk_word_k9_hostile"], "high_bits_chunk_word", 300), with_junk(by["sweep_k11"], "high_bits_planted", 301)]


@functools.lru_cache(maxsize=None)
def families():
    f = dict(chunk_word=chunk_word_cases(), strands=strands_cases(), units=units_cases(), sweep=sweep_cases(), select=select_cases(),
             slices=slices_cases())
    f["high_bits"] = high_bits_cases(f["chunk_word"], f["sweep"])
    return f


def all_cases():
    return [c for fam in families().values() for c in fam]
