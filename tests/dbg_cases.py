"""Hand-built dbg calls that sit on the edges of csrc/dbg_kernels.hip: k-mers that share a node slot's tag and home, tables
at the load their sizing allows, node counts and first-touch keys on the 256-rank rounds of the finish kernel, its record
buffer at exact capacity, long successor lists, the quality / 'N' / flag filter at its thresholds and a call whose windows
and reads are laid out awkwardly.  Builders only: no GPU, no BAM, no make_windows.  Every case carries a check that asserts,
on the restatement (tests/dbg_ref.py) and the restated hash below, that it is what it claims to be;
tests/test_dbg_edges_cpu.py calls every check and holds the restated hash against the product's header
(csrc/dbg_hash.h, host build), tests/test_dbg_edges_gpu.py runs the same cases on the device.

The kernel's hash, sizing and finish-kernel constants are restated here in numpy / plain Python: a change of them has to be
repeated here, and the CPU test then says which claim no longer holds."""
import functools

import numpy as np

import dbg_ref as R

FNV_BASIS, FNV_PRIME = np.uint64(0xcbf29ce484222325), np.uint64(0x100000001b3)
TAG_SHIFT = 41
FIN_THREADS = 256                        # ranks (and first-touch keys) per round of dbg_finish_kernel
MAX_K, MIN_K = 64, 3
REC_MAX = MAX_K + 14 + 4 * 12            # a node's digest record at most; the kernel's LDS holds FIN_THREADS of them
ACGT = b"ACGT"
ODD = b"=ACMGRSVTWYHKDBacgtn"            # what a BAM can spell besides 'N', and lower case (a FASTA's soft mask)


# ------------------------------------------------------------------------------------------------- the hash, restated
def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def fnv_rows(rows, h=None):
    """FNV-1a over every row of a (n, k) uint8 array, from h (default: the basis) -> uint64[n]"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.uint8))
    h = np.full(rows.shape[0], FNV_BASIS, dtype=np.uint64) if h is None else h.copy()
    for j in range(rows.shape[1]):
        h = (h ^ rows[:, j].astype(np.uint64)) * FNV_PRIME
    return h


def mix64(h):
    h = _u64(h).copy()
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xff51afd7ed558ccd)
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xc4ceb9fe1a85ec53)
    h ^= h >> np.uint64(33)
    return h


def node_hash(rows):
    return mix64(fnv_rows(rows))


def node_tag_home(kmers, nc):
    """kmers: a list of equally long bytes -> (tag, home) lists of Python ints"""
    h = node_hash(np.frombuffer(b"".join(kmers), dtype=np.uint8).reshape(len(kmers), -1))
    return [int(x) for x in h >> np.uint64(TAG_SHIFT)], [int(x) for x in h & np.uint64(nc - 1)]


def edge_home(slot, byte, ec):
    key = np.array([(slot + 1) << 8 | byte], dtype=np.uint64)
    return int(mix64(key)[0] & np.uint64(ec - 1))


def sizes(C):
    """(nc, ec): the first powers of two >= 2C + 1 and >= C + 1, both at least 2"""
    nc = ec = 2
    while nc < 2 * C + 1:
        nc <<= 1
    while ec < C + 1:
        ec <<= 1
    return nc, ec


# ------------------------------------------------------------------------------------------------- the searches (kept; their finds are frozen below)
HOME_BITS = 6                            # the frozen k-mers agree on the tag and on the low 6 bits: one home for nc = 32 and 64


def _key(h):
    return (h >> np.uint64(TAG_SHIFT)) << np.uint64(HOME_BITS) | (h & np.uint64((1 << HOME_BITS) - 1))


def search_pair(where, alphabet, seed, k=15, chunk=1 << 20, max_chunks=400):
    """Two k-mers that differ in the byte at `where` alone (both bytes from `alphabet`, the rest random ACGT) and agree on tag
    and home: random contexts, every byte of the alphabet at `where`, until one context holds two equal keys."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    for _ in range(max_chunks):
        rows = np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, (chunk, k))]
        pre = fnv_rows(rows[:, :where]) if where else np.full(chunk, FNV_BASIS, dtype=np.uint64)
        keys = np.empty((chunk, alpha.size), dtype=np.uint64)
        for a, v in enumerate(alpha):
            h = (pre ^ np.uint64(v)) * FNV_PRIME
            keys[:, a] = _key(mix64(fnv_rows(rows[:, where + 1:], h)))
        order = np.argsort(keys, axis=1)
        srt = np.take_along_axis(keys, order, axis=1)
        hit = np.argwhere(srt[:, 1:] == srt[:, :-1])
        if hit.size:
            r, c = (int(x) for x in hit[0])
            out = []
            for a in (order[r, c], order[r, c + 1]):
                km = rows[r].copy()
                km[where] = alpha[a]
                out.append(km.tobytes())
            return tuple(sorted(out))
    raise RuntimeError("no pair found")


def search_triple(seed, k=15, n=1 << 23):
    """Three random ACGT k-mers that agree on tag and home"""
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, (n, k))]
    keys = _key(node_hash(rows))
    order = np.argsort(keys, kind="stable")
    srt = keys[order]
    hit = np.flatnonzero((srt[2:] == srt[:-2]))
    for x in hit:
        kms = {rows[order[x + d]].tobytes() for d in range(3)}
        if len(kms) == 3:
            return tuple(sorted(kms))
    raise RuntimeError("no triple found")


# what the searches found (search_pair(where, alphabet, 100 + where) for where = 0, 7, 14; search_triple(11)), frozen so
# that import costs nothing; check_collide re-derives tag and home, so a changed hash fails on the CPU
PAIRS = {
    "first": (0, b"SATCTGCATGCAGCG", b"cATCTGCATGCAGCG"),          # search_pair(0, ODD, 100)
    "middle": (7, b"CCTCCCABAGCCTGT", b"CCTCCCAVAGCCTGT"),         # search_pair(7, ODD, 107)
    "last": (14, b"CTTGCAACAACCCCA", b"CTTGCAACAACCCCT"),          # search_pair(14, ACGT, 114)
}
TRIPLE = (b"AAATTCACCACTGTG", b"TATTGCTGCAATAGG", b"TGAGTCGACTTCCAT")   # search_triple(11)


def frozen_kmers():
    return [km for _, a, b in PAIRS.values() for km in (a, b)] + list(TRIPLE)


# ------------------------------------------------------------------------------------------------- a call
class Case:
    """One call: reads [(seq, qual, flag)], wins [(ref bytes, ref_pos, read_lo, read_hi)], k, min_qual; check(case) asserts
    what the case is there for; facts: what its builder knows (for the check)."""

    def __init__(self, name, k, min_qual, reads, wins, check=None, **facts):
        self.name, self.k, self.min_qual, self.reads, self.wins, self.check, self.facts = name, k, min_qual, reads, wins, check, facts
        self._want = self._packed = None

    @property
    def n_win(self):
        return len(self.wins)

    def slots(self, n):
        return max(0, n - self.k - 1)

    def occ(self, w):
        """C of window w: its occurrence slots"""
        ref, _, lo, hi = self.wins[w]
        return self.slots(len(ref)) + sum(self.slots(len(self.reads[r][0])) for r in range(lo, hi))

    def tables(self, w):
        return sizes(self.occ(w))

    def want(self):
        """the restatement: (stats, graphs), one entry per window, computed once"""
        if self._want is None:
            res = [R.graph(ref, pos, self.reads[lo:hi], self.k, self.min_qual) for ref, pos, lo, hi in self.wins]
            self._want = ([st for _, st in res], [g for g, _ in res])
        return self._want

    def first_keys(self, w):
        """{kmer: first-touch key 2 * slot + side} of window w and the number of occurrences kept, by the contract's filter
        (slot: the reference's occurrences, then the reads' by index and offset, skipped ones counted)"""
        ref, _, lo, hi = self.wins[w]
        k, keys, c, kept = self.k, {}, 0, 0
        for i in range(self.slots(len(ref))):
            keys.setdefault(ref[i:i + k], 2 * c)
            keys.setdefault(ref[i + 1:i + 1 + k], 2 * c + 1)
            c, kept = c + 1, kept + 1
        for seq, qual, flag in self.reads[lo:hi]:
            for i in range(self.slots(len(seq))):
                if not flag & 0x200 and b"N" not in seq[i:i + k + 1] and min(qual[i:i + k + 1]) >= self.min_qual:
                    keys.setdefault(seq[i:i + k], 2 * c)
                    keys.setdefault(seq[i + 1:i + 1 + k], 2 * c + 1)
                    kept += 1
                c += 1
        assert c == self.occ(w)
        return keys, kept

    def src_numbers(self, w):
        """the value of gbx_dbg_node.src for every node of window w, from the restatement's ('ref', j) / ('read', r, j)"""
        ref_off = sum(len(x[0]) for x in self.wins[:w])
        seq_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in self.reads])])
        lo = self.wins[w][2]
        return [ref_off + s[1] if s[0] == "ref" else -1 - (int(seq_off[lo + s[1]]) + s[2]) for s in (n["src"] for n in self.want()[1][w])]

    def packed(self):
        """(DbgReads, DbgWins, params) of the library's Python side"""
        if self._packed is None:
            from genomicsbench_amd import dbg as D
            rs = D.DbgReads.from_list([(s, q, f, 0, len(s)) for s, q, f in self.reads])
            off = np.concatenate([[0], np.cumsum([len(x[0]) for x in self.wins])]).astype(np.int64)
            ws = D.DbgWins(off, np.frombuffer(b"".join(x[0] for x in self.wins), dtype=np.uint8), [x[1] for x in self.wins],
                           [x[2] for x in self.wins], [x[3] for x in self.wins])
            self._packed = (rs, ws, D.make_params(self.k, self.min_qual))
        return self._packed


def concat(name, cases, check=None, **facts):
    """the cases' windows as one call (same k and min_qual), each with reads of its own"""
    reads, wins = [], []
    for c in cases:
        assert (c.k, c.min_qual) == (cases[0].k, cases[0].min_qual)
        wins += [(ref, pos, lo + len(reads), hi + len(reads)) for ref, pos, lo, hi in c.wins]
        reads += c.reads
    return Case(name, cases[0].k, cases[0].min_qual, reads, wins, check, parts=cases, **facts)


def rnd(rng, n, alphabet=ACGT):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def read(seq, q=30, flag=0):
    return (seq, bytes([q]) * len(seq) if isinstance(q, int) else bytes(q), flag)


def node_of(graph, kmer):
    hit = [n for n in graph if n["kmer"] == kmer]
    assert len(hit) == 1, kmer
    return hit[0]


# ------------------------------------------------------------------------------------------------- a. collisions
def check_collide(c):
    """the frozen k-mers differ in the one byte, are nodes of their own with different successors, and share tag and home at
    the window's own nc (32 or 64)"""
    kms, where = c.facts["kmers"], c.facts["where"]
    nc = c.tables(0)[0]
    assert nc in (32, 64), nc
    tag, home = node_tag_home(list(kms), nc)
    assert len(set(tag)) == 1 and len(set(home)) == 1 and len(set(kms)) == len(kms), (tag, home)
    if where is not None:
        assert [j for j in range(c.k) if kms[0][j] != kms[1][j]] == [where]
    g = c.want()[1][0]
    succ = [tuple(g[e]["kmer"] for e, _ in node_of(g, km)["edges"]) for km in kms]
    assert all(succ) and len(set(succ)) == len(kms), succ
    if "short_ref" in c.facts:
        assert c.slots(len(c.wins[0][0])) == 0


def collide(where, form):
    pos, a, b = PAIRS[where]
    rng = np.random.default_rng(1000 + 10 * pos + len(form))
    if form == "ref_ab":                                   # 16 slots: nc = 64
        reads, ref = [], a + b + rnd(rng, 2)
    elif form == "ref_ba":
        reads, ref = [], b + a + rnd(rng, 2)
    elif form == "ref_a_read_b":                           # 8 + 5 slots: nc = 32
        reads, ref = [read(b + b"G" + rnd(rng, 5))], a + b"A" + rnd(rng, 8)
    else:                                                  # "reads": 5 + 5 slots, none of the reference's: nc = 32
        reads, ref = [read(a + b"A" + rnd(rng, 5), 33), read(b + b"G" + rnd(rng, 5), 35)], rnd(rng, 10)
    extra = {"short_ref": True} if form == "reads" else {}
    return Case("collide_%s_%s" % (where, form), 15, 20, reads, [(ref, 500, 0, len(reads))], check_collide, kmers=(a, b), where=pos, **extra)


def collide_triple():
    rng = np.random.default_rng(1999)
    reads = [read(km + rnd(rng, 6), 30 + j) for j, km in enumerate(TRIPLE)]      # 15 slots: nc = 32
    return Case("collide_triple", 15, 20, reads, [(rnd(rng, 12), 0, 0, 3)], check_collide, kmers=TRIPLE, where=None, short_ref=True)


FORMS = ("ref_ab", "ref_ba", "ref_a_read_b", "reads")


# ------------------------------------------------------------------------------------------------- b. one window many times
def check_replicated(c):
    part = c.facts["parts"][0]
    assert c.n_win == len(c.facts["parts"]) >= FIN_THREADS and all(p is part for p in c.facts["parts"])
    part.check(part)
    assert all(c.occ(w) == part.occ(0) and c.wins[w][0] == part.wins[0][0] for w in range(c.n_win))


def replicated(case, n=256):
    c = concat("replicated_" + case.name, [case] * n, check_replicated)
    st, g = case.want()
    c._want = (st * n, g * n)                               # (the copies are the same window: one restatement)
    return c


# ------------------------------------------------------------------------------------------------- c. full tables
def probe_layout(kmers, nc):
    """slot of every k-mer after linear probing from its home (the set of taken slots does not depend on the order)"""
    _, home = node_tag_home(kmers, nc)
    taken, slot = set(), []
    for h in home:
        while h in taken:
            h = (h + 1) & (nc - 1)
        taken.add(h)
        slot.append(h)
    return home, slot


def check_full_tables(c):
    """2C = nc - 2 nodes and C = ec - 1 edges; a node's home is one of the last two slots and a probe wraps past the end"""
    C = c.facts["C"]
    nc, ec = c.tables(0)
    st, g = c.want()
    assert c.occ(0) == C and (st[0]["n_nodes"], st[0]["n_edges"]) == (2 * C, C) == (nc - 2, ec - 1)
    home, slot = probe_layout([n["kmer"] for n in g[0]], nc)
    assert max(home) >= nc - 2 and any(s < h for s, h in zip(slot, home))


def full_tables(C):
    for seed in range(100):
        rng = np.random.default_rng(3000 + 7 * C + seed)
        c = Case("full_tables_%d" % C, 15, 20, [read(rnd(rng, 17)) for _ in range(C)], [(b"", 0, 0, C)], check_full_tables, C=C)
        kms = [s[i:i + 15] for s, _, _ in c.reads for i in (0, 1)]
        home, slot = probe_layout(kms, sizes(C)[0])
        if len(set(kms)) == 2 * C and max(home) >= sizes(C)[0] - 2 and any(s < h for s, h in zip(slot, home)):
            return c
    raise AssertionError("no seed")


# ------------------------------------------------------------------------------------------------- d. 256-rank rounds
WIDE = bytes(range(33, 127))             # a reference is not filtered: any byte makes a node


def check_rounds(c):
    """n_nodes, C and the last first-touch key(s) are where the case puts them"""
    st, g = c.want()
    keys, _ = c.first_keys(0)
    C = c.occ(0)
    assert st[0]["n_nodes"] == c.facts["n_nodes"] == len(keys) and C == c.facts["C"]
    assert [n["kmer"] for n in g[0]] == sorted(keys, key=keys.get)
    last = sorted(keys.values())[-len(c.facts["last_keys"]):]
    assert last == [2 * C - d for d in c.facts["last_keys"]], (last, C)
    if "last_mod" in c.facts:
        assert [x % FIN_THREADS for x in last] == c.facts["last_mod"]
    if "few" in c.facts:
        assert len(keys) * 8 < 2 * C


def rounds(n, k=15):
    """a reference that is a path of n distinct k-mers, no reads: n_nodes = n, C = n - 1"""
    for seed in range(100):
        ref = rnd(np.random.default_rng(4000 + n + 1000 * k + seed), n + k, ACGT if k > 8 else WIDE)
        if len({ref[i:i + k] for i in range(n)}) == n:
            return Case("rounds_%d_k%d" % (n, k), k, 20, [], [(ref, 100, 0, 0)], check_rounds, n_nodes=n, C=n - 1, last_keys=[1])
    raise AssertionError("no seed")


def two_c(m, k=15):
    """2C = m exactly: half the slots the reference's, the rest fresh reads of up to 60 slots; every k-mer new"""
    rng = np.random.default_rng(4500 + m)
    C = m // 2
    left, reads = C - C // 2, []
    while left:
        s = min(left, 60 if len(reads) % 2 else 37)
        reads.append(read(rnd(rng, s + k + 1), 25 + len(reads)))
        left -= s
    return Case("two_c_%d" % m, k, 20, reads, [(rnd(rng, C // 2 + k + 1), 7, 0, len(reads))], check_rounds, n_nodes=C + 1 + len(reads), C=C,
                last_keys=[1], last_mod=[FIN_THREADS - 1])


def late_key(tail, k=15):
    """reads that repeat the reference, so C is in the hundreds and the first-touch keys are few, and then a new k-mer in the
    last occurrence.  tail 255: C = 256, its end node alone is new, key 2C - 1 = 255 (mod 256).  tail 0: C = 257, both of its
    nodes are new, keys 2C - 2 = 0 and 2C - 1 = 1 (mod 256) (a key = 0 (mod 256) is a start node's: 2C - 1 is odd)."""
    rng = np.random.default_rng(4700 + tail)
    ref = rnd(rng, 40 + k + 1)
    C, n_last = (256, 9) if tail == 255 else (257, 1)
    left, reads = C - 40 - n_last, []
    while left:
        s = min(left, 5 + 7 * len(reads) % 31)
        at = int(rng.integers(0, 41 - s))
        reads.append(read(ref[at:at + s + k + 1], 21 + len(reads)))
        left -= s
    if tail == 255:
        last = bytearray(ref[3:3 + n_last + k + 1])
        last[-2] = ACGT[(ACGT.index(last[-2]) + 1) % 4]      # the last byte an occurrence reads; the one after it is read by none
        reads.append(read(bytes(last)))
        facts = dict(n_nodes=42, last_keys=[1], last_mod=[255])
    else:
        reads.append(read(rnd(rng, k + 2)))
        facts = dict(n_nodes=43, last_keys=[2, 1], last_mod=[0, 1])
    return Case("late_key_%d" % tail, k, 20, reads, [(ref, 9000, 0, len(reads))], check_rounds, C=C, few=True, **facts)


ROUND_SIZES = (255, 256, 257, 511, 512, 513)


def rounds_call():
    """the k = 15 paths as one call: empty, 255, 256, 257, 511, 512, empty, 513"""
    empty = Case("empty", 15, 20, [], [(b"", 0, 0, 0)])
    parts = [empty] + [rounds(n) for n in ROUND_SIZES[:5]] + [empty, rounds(513)]
    return concat("rounds_call", parts, lambda c: [p.check(p) for p in c.facts["parts"] if p.check])


# ------------------------------------------------------------------------------------------------- e. the record buffer
def check_records_full(c):
    """ranks 0..255 keep 4 edges each and their records fill the finish kernel's buffer to the byte; the second variant
    drops successors in that round as well"""
    st, g = c.want()
    assert c.k == MAX_K and st[0]["n_nodes"] == 1181 + c.facts["dropped"] and st[0]["n_dropped"] == c.facts["dropped"]
    assert all(len(n["edges"]) == 4 for n in g[0][:FIN_THREADS])
    assert sum(len(R.record(n)) for n in g[0][:FIN_THREADS]) == FIN_THREADS * REC_MAX == 32256
    if c.facts["dropped"]:
        dropped_in_round = sum(1 for n in g[0][:FIN_THREADS] for r in c.reads if r[0][:c.k] == n["kmer"] and r[0][c.k:c.k + 1] in b"RY")
        assert dropped_in_round == 2 * 26 and c.facts["dropped"] == 2 * 30      # every tenth of ranks 0..255, of all 295


def records_full(extra=False):
    rng = np.random.default_rng(5000)
    k = MAX_K
    S = rnd(rng, k + FIN_THREADS + 40)
    reads = [read(S[i:i + k] + bytes([x]) + b"A") for i in range(len(S) - k - 1) for x in ACGT if x != S[i + k]]
    if extra:
        reads += [read(S[i:i + k] + x + b"C", 41) for i in range(0, len(S) - k - 1, 10) for x in (b"R", b"Y")]
    return Case("records_full" + "_dropped" * extra, k, 20, reads, [(S, 77, 0, len(reads))], check_records_full,
                dropped=2 * len(range(0, len(S) - k - 1, 10)) if extra else 0)


# ------------------------------------------------------------------------------------------------- f. many successors
def check_fanout(c):
    """the start k-mer keeps the reference's 'N' edge and the three read edges of least first appearance, their weights
    summed over the repeats that come later; everything else is dropped"""
    st, g = c.want()
    n, start = c.facts["n_succ"], node_of(c.want()[1][0], c.facts["start"])
    assert len(start["edges"]) == 4 and st[0]["n_dropped"] == n + 1 - 4
    assert [(g[0][e]["kmer"][-1], w) for e, w in start["edges"]] == c.facts["kept"]
    assert st[0]["n_nodes"] == 1 + n + 1 and st[0]["n_edges"] == 4


def fanout(n_succ):
    rng = np.random.default_rng(6000 + n_succ)
    k = 15
    start = rnd(rng, k)
    pool = [int(x) for x in rng.permutation(256) if x not in (ord("N"), 0, 255, ord("n"), ord("C"))]
    succ = ([ord("C"), 0, 255, ord("n")] + pool)[:n_succ]           # every byte value but 'N' may follow in a read
    order = [(succ[0], 30), (succ[1], 31), (succ[0], 25)] + [(b, 40) for b in succ[2:]]
    order += [(succ[1], 22), (succ[2], 50), (succ[0], 21)] + [(b, 33) for b in succ[3:4]]
    reads = [read(start + bytes([b]) + b"A", q) for b, q in order]
    kept = [(ord("N"), 1), (succ[0], 30 + 25 + 21), (succ[1], 31 + 22), (succ[2], 40 + 50)]
    return Case("fanout_%d" % n_succ, k, 20, reads, [(start + b"NA", 40, 0, len(reads))], check_fanout, n_succ=n_succ, start=start, kept=kept)


# ------------------------------------------------------------------------------------------------- g. the filter's thresholds
def check_quality(c):
    """occurrences at min_qual exactly are kept with that weight and those one below skipped, whichever of the k + 1 bytes
    holds the minimum; 'N' skips at byte 0 and byte k, 'n' does not; 0x200 reads add nothing; a window of skipped
    occurrences alone has slots but no node, and the digest of nothing"""
    st, g = c.want()
    mq, k = c.min_qual, c.k
    for w in (0, 1):
        keys, kept = c.first_keys(w)
        assert kept == c.facts["kept"][w] == st[w]["n_occ"] and len(keys) == st[w]["n_nodes"]
    assert c.occ(1) > 0 and st[1]["n_nodes"] == 0 and st[1]["digest"] == R.FNV_BASIS and c.slots(len(c.wins[1][0])) == 0
    kms = {n["kmer"]: n for n in g[0]}
    for name, (seq, present) in c.facts["marks"].items():
        assert (seq[:k] in kms) == present, name
    assert kms[c.facts["marks"]["q255"][0][:k]]["weight"] == 255
    assert kms[c.facts["marks"]["at_mq"][0][:k]]["weight"] == mq


def quality_edges(mq, k=11):
    rng = np.random.default_rng(7000 + mq)
    hi = 255 if mq == 255 else max(mq + 9, 30)
    one = lambda: rnd(rng, k + 2)                              # noqa: E731  (a read of one slot: its own start k-mer)
    lowq = lambda n, at: bytes(mq - 1 if j == at else hi for j in range(n))   # noqa: E731
    reads, kept, marks = [], 0, {}

    def add(name, seq, q, flag, n_kept, present=None):
        nonlocal kept
        reads.append(read(seq, q, flag))
        kept += n_kept
        if present is not None:
            marks[name] = (seq, present)
    add("at_mq", one(), mq, 0, 1, True)
    add("q255", one(), 255, 0, 1, True)
    add("flagged", one(), hi, 0x200, 0, False)
    add("other_flags", one(), hi, 0x400 | 0x10 | 0x1, 1, True)
    add("n_at_0", b"N" + rnd(rng, k + 1), hi, 0, 0, False)
    s = one()
    add("n_at_k", s[:k] + b"N" + s[k + 1:], hi, 0, 0, False)
    add("n_after", one()[:k + 1] + b"N", hi, 0, 1, True)       # (the byte no occurrence reads)
    add("flagged_2", rnd(rng, 3 * k), hi, 0x200 | 0x4, 0, False)
    s = one()
    add("lower_n", s[:2] + b"n" + s[3:], hi, 0, 1, True)
    long_ = rnd(rng, 3 * k + 4)                                # 2k + 3 slots
    add("n_inside", long_[:k + 4] + b"N" + long_[k + 5:], hi, 0, (2 * k + 3) - (k + 1), None)
    if mq > 0:
        add("low_at_0", one(), lowq(k + 2, 0), 0, 0, False)
        add("low_at_k", one(), lowq(k + 2, k), 0, 0, False)
        add("low_after", one(), lowq(k + 2, k + 1), 0, 1, True)
        add("low_inside", rnd(rng, 3 * k + 4), lowq(3 * k + 4, k + 4), 0, (2 * k + 3) - (k + 1), None)
    add("flagged_last", one(), hi, 0x200, 0, False)
    ref = rnd(rng, 30)
    n0 = len(reads)
    # the second window: every occurrence skipped, the reference too short for one
    reads += [read(rnd(rng, 20), hi, 0x200), read(b"N".join(rnd(rng, k) for _ in range(4)), hi),
              read(rnd(rng, 12), mq - 1 if mq else hi, 0 if mq else 0x200)]
    return Case("quality_%d" % mq, k, mq, reads, [(ref, 10, 0, n0), (rnd(rng, k + 1), 3, n0, len(reads))], check_quality,
                kept=[30 - k - 1 + kept, 0], marks=marks)


# ------------------------------------------------------------------------------------------------- h. layout
LAYOUT_KINDS = ("empty", "ordinary", "empty", "empty", "ref_only", "reads_only", "all_skipped", "ordinary", "empty")


def check_layout(c):
    """the nine windows are of the kinds listed, the two ordinary ones share reads, and reads without a slot (length 0, 1, k
    and k + 1) stand first, in the middle and last in a window's read range"""
    st, _ = c.want()
    k = c.k
    assert c.n_win == len(LAYOUT_KINDS)
    for w, kind in enumerate(LAYOUT_KINDS):
        ref, _, lo, hi = c.wins[w]
        C, nref = c.occ(w), c.slots(len(ref))
        if kind == "empty":
            assert C == 0 and st[w]["n_nodes"] == 0
        elif kind == "ordinary":
            assert nref and C > nref and st[w]["n_both"] and st[w]["n_read"] and st[w]["n_ref"]
        elif kind == "ref_only":
            assert C == nref > 0 and lo == hi and st[w]["n_nodes"] == st[w]["n_ref"] == nref + 1
        elif kind == "reads_only":
            assert len(ref) == 0 and C > 0 and st[w]["n_nodes"] == st[w]["n_read"] > 0
        else:
            assert nref == 0 and C > 0 and st[w]["n_nodes"] == 0 and st[w]["digest"] == R.FNV_BASIS
    (lo1, hi1), (lo7, hi7) = c.wins[1][2:], c.wins[7][2:]
    assert lo1 < lo7 < hi1 < hi7
    lens = [len(r[0]) for r in c.reads]
    assert {0, 1, k, k + 1} <= set(lens)
    for w in (1, 5, 7):
        lo, hi = c.wins[w][2:]
        zero = [c.slots(n) == 0 for n in lens[lo:hi]]
        assert zero[0] and zero[-1] and any(zero[1:-1]) and not all(zero)
    assert all(c.slots(n) == 0 for n in lens[c.wins[3][2]:c.wins[3][3]]) and c.wins[3][3] - c.wins[3][2] == 2
    assert c.wins[8][2] == c.wins[8][3] == len(c.reads)
    assert c.wins[4][1] + len(c.wins[4][0]) == 2 ** 31 - 1          # positions up to the contract's limit


def layout():
    rng = np.random.default_rng(8000)
    k = 15
    ref1, ref7 = rnd(rng, 60), rnd(rng, 40)

    def piece(src, n, q=30):                                    # a read off a reference, one base changed
        at = int(rng.integers(0, len(src) - n + 1))
        s = bytearray(src[at:at + n])
        s[n // 2] = ACGT[(ACGT.index(s[n // 2]) + 1) % 4]
        return read(bytes(s), q)
    z = lambda n: read(rnd(rng, n))                             # noqa: E731
    reads = [z(0), piece(ref1, 30), piece(ref1, 25, 22), z(k), z(1), piece(ref7, 28), piece(ref1, 40, 37), piece(ref7, 19), z(k + 1),   # 0..8
             z(k + 1), z(0), piece(ref7, 33), z(k), read(rnd(rng, 26), 21), z(1), read(rnd(rng, 17), 255), z(k),                           # 9..16
             read(rnd(rng, 30), 30, 0x200), read(b"N".join(rnd(rng, k) for _ in range(3))), read(rnd(rng, 22), 19)]                        # 17..19
    wins = [(b"", 0, 0, 0), (ref1, 1000, 0, 9), (rnd(rng, k + 1), 2000, 3, 3), (b"", 2100, 9, 11), (rnd(rng, 50), 2 ** 31 - 1 - 50, 11, 11),
            (b"", 5, 9, 17), (rnd(rng, 5), 6000, 17, 20), (ref7, 7000, 4, 13), (b"", 8000, 20, 20)]
    return Case("layout", k, 20, reads, wins, check_layout)


# ------------------------------------------------------------------------------------------------- all of them
@functools.lru_cache(maxsize=None)
def families():
    """{family: [Case]}; every case built once"""
    col = [collide(where, form) for where in PAIRS for form in FORMS] + [collide_triple()]
    return {
        "collide": col,
        "replicated": [replicated(col[FORMS.index("reads") + 4 * list(PAIRS).index("last")]), replicated(col[0]), replicated(col[-1])],
        "full_tables": [full_tables(C) for C in (31, 127, 511)],
        "rounds": [rounds(n, k) for k in (15, MIN_K) for n in ROUND_SIZES] + [two_c(m) for m in (256, 512, 768)] + [late_key(255), late_key(0)],
        "records_full": [records_full(), records_full(extra=True)],
        "fanout": [fanout(200), fanout(3), fanout(4)],
        "quality": [quality_edges(mq) for mq in (0, 20, 255)],
        "layout": [layout()],
        "rounds_call": [rounds_call()],
    }


def all_cases():
    return [c for cases in families().values() for c in cases]
